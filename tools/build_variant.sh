#!/bin/bash
# Build an A/B variant of libatx.so into anemoi-transform_amd/lib/variants/ (git-ignored, travels to the GPU box).
#   bash tools/build_variant.sh NAME [-DATX_KNOB=VALUE ...]          current sources with extra defines
#   bash tools/build_variant.sh NAME --rev <git-rev> [-D...]          the csrc/ + include/ of an earlier commit
# The knobs that are left choose the math routes (ATX_FAST_EXP, ATX_FAST_LOG, ATX_FAST_SINCOS, ATX_SNOW_TANH, ATX_FMA_SGPR, ATX_SINCOS_FMA) and
# the grid cap (ATX_MAX_GRID).  The per-point, the gather, the combine and the relayout kernels' knobs are frozen (HISTORY.md): their other
# sides need a --rev build of a commit that still had them (402a730 for the gather, e6acba1 for combine and relayout).  The store
# policy of the gather kernels (ATX_STORE_POLICY=OutStore::nt|sc1|sc0sc1|sc1nt) is tools/experiments/gather_store_policy.patch, applied to the
# csrc/ of the parent of the commit that added it.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
SRC=$ROOT/anemoi-transform_amd/csrc
if [ "$1" == "--rev" ]; then
  REV=$2; shift 2
  TMP=$ROOT/gpurun_out/scratch/rev_$NAME
  rm -rf $TMP && mkdir -p $TMP/anemoi-transform_amd/csrc $TMP/include
  for f in $(git -C $ROOT ls-tree --name-only $REV anemoi-transform_amd/csrc/ include/); do git -C $ROOT show $REV:$f > $TMP/$f; done
  SRC=$TMP/anemoi-transform_amd/csrc
fi
mkdir -p $ROOT/anemoi-transform_amd/lib/variants
cd $SRC
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -Wno-unused-function "$@" \
  -o $ROOT/anemoi-transform_amd/lib/variants/libatx_$NAME.so *.hip
echo built $ROOT/anemoi-transform_amd/lib/variants/libatx_$NAME.so
