"""The ulp budgets of the single-function operators (exp, log, sincos, tanh, atan2, hypot), derived from the code of the route the
library takes for each — plain data and one function, shared by tests/test_gpu_ulp_budgets.py and tests/pointwise_route_checks.py.
A library built with other knobs (tools/build_variant.sh, loaded through ATX_LIBRARY) is measured against the budgets of ITS routes
when ATX_LIBRARY_DEFINES names the defines it was built with (e.g. ``ATX_LIBRARY_DEFINES="-DATX_FAST_EXP=0"``)."""

from __future__ import annotations

import os
import re

import numpy as np


def _define(name: str, default: int) -> int:
    m = re.search(r"-D%s=(\d+)" % name, os.environ.get("ATX_LIBRARY_DEFINES", ""))
    return int(m.group(1)) if m else default


FAST_EXP, FAST_LOG, FAST_SINCOS, SNOW_TANH = _define("ATX_FAST_EXP", 1), _define("ATX_FAST_LOG", 2), _define("ATX_FAST_SINCOS", 1), _define("ATX_SNOW_TANH", 0)

# The device math library's routes: the maximum errors of the HIP / CUDA math API tables — float64 exp, log 1; sin, cos, tanh, atan2,
# hypot 2; float32 expf, sinf, cosf, tanhf 2; atan2f, hypotf 3 — and float32 logf 2: the library evaluates it from the hardware's log2
# (v_log_f32) and a product with ln 2, 1.85 ulps measured on these cases, not within the 1 ulp of a correctly rounded log.
LIB64 = {"exp": 1.0, "log": 1.0, "sincos": 2.0, "tanh": 2.0, "atan2": 2.0, "hypot": 2.0}
LIB32 = {"exp": 2.0, "log": 2.0, "sincos": 2.0, "tanh": 2.0, "atan2": 3.0, "hypot": 3.0}


def budgets(dtype) -> dict:
    """(statement, output) -> max ulps, from the code of the route the library takes."""
    if dtype == np.float32:  # float32 takes the device library everywhere
        b = LIB32
        sincos = b["sincos"]
        return {("exp", 0): b["exp"], ("log", 0): b["log"], ("cos_sin", 0): sincos, ("cos_sin", 1): sincos, ("cos_sin_deg", 0): sincos,
                ("cos_sin_deg", 1): sincos, ("atan2", 0): b["atan2"], ("snow_cover", 0): b["tanh"], ("xy_to_polar", 0): b["hypot"],
                ("polar_to_xy", 0): 2 * sincos + 0.5, ("polar_to_xy", 1): 2 * sincos + 0.5}
    b = LIB64
    # atx_exp (ATX_FAST_EXP=1): reduction exact to 2^-100, polynomial 0.15 x 2^-53, 1 + r(1 + r q) with two roundings below 1 ulp —
    # <= 1 ulp (the comment in atx_common.hpp: 0.9 on its host prototype); the library's: 1
    exp = 1.0 if FAST_EXP else b["exp"]
    # atx_log (ATX_FAST_LOG=2, =1): fdlibm's reduction and R with the quotient s = f / (2 + f) within 1 ulp — < 1 ulp (0.73 measured on the
    # host prototype); the library's: 1
    log = 1.0 if FAST_LOG else b["log"]
    # sincos_moderate (ATX_FAST_SINCOS=1, |a| < 1e5): exact Cody-Waite reduction, fdlibm's kernels — < 1 ulp; the rest takes the library's
    # sincos.  The per-case budget of "beyond 1e5" is the library's (test below); everything else is the own routine's.
    sincos = 1.0 if FAST_SINCOS else b["sincos"]
    # snow cover's tanh (ATX_SNOW_TANH=0): e = expm1(2x) (1.2 ulp), e + 2 (0.5), quotient_1ulp (1) — tanh = e / (e + 2) carries e's error
    # scaled by 2 / (e + 2) <= 1: 1.2 + 0.5 + 1 = 2.7 -> 3.  ATX_SNOW_TANH=1: the library's tanh
    tanh = 3.0 if SNOW_TANH == 0 else b["tanh"]
    return {("exp", 0): exp, ("log", 0): log, ("cos_sin", 0): sincos, ("cos_sin", 1): sincos, ("cos_sin_deg", 0): sincos,
            ("cos_sin_deg", 1): sincos, ("atan2", 0): b["atan2"], ("snow_cover", 0): tanh, ("xy_to_polar", 0): b["hypot"],
            # speed * cos(a): cos's error is up to twice as many ulps of the product (their mantissas), plus the product's rounding
            ("polar_to_xy", 0): 2 * sincos + 0.5, ("polar_to_xy", 1): 2 * sincos + 0.5}
