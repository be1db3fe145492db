"""Every launch form of ``atx_pointwise_stack`` on the device, held to numpy's bits by the checks of tests/pointwise_route_checks.py:
each case declares the route it is written for and asserts ``native.last_route()`` took it, then compares every element — COPY
levels as bit copies, arithmetic levels bit for bit in float32 as in float64, exp / log levels against exact arithmetic at the
budgets of tests/test_gpu_ulp_budgets.py, padding and canaries untouched, in place equal to out of place.
tests/test_pointwise_route_checks_catch_defects.py shows each assertion failing on a planted defect."""

from __future__ import annotations

import time

import numpy as np
import pytest
import torch

import pointwise_route_checks as C
from anemoi_transform_amd import native

pytestmark = pytest.mark.gpu

CASES = C.all_cases()


@pytest.fixture
def kern():
    return C.Kernels(pointwise_stack=native.pointwise_stack, last_route=native.last_route, level_program=native.level_program)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_takes_its_route_and_gives_numpys_bits(dev, kern, case):
    taken = C.check_case(kern, dev, case)
    assert taken == {mode: case.expected(mode) for mode in case.modes}


def test_a_stack_without_points_launches_nothing(dev, kern):
    C.check_no_points(kern, dev)


def test_every_route_has_a_case():
    """Adding a launch form without a case written for it fails here."""
    assert C.declared_routes(CASES) == set(C.ROUTES)


def test_row_chunk_kernel_past_the_grid_cap(dev, kern):
    """The row-chunk kernel past ``kStreamGrid`` workgroups.  It serves only pitches no vector walk takes (unequal, odd, loose under a
    per-level program, a base off 16 bytes); the full-size tests build their stacks with ``Stack.empty``'s tight aligned pitch and none
    reaches it at a size that wraps (DESIGN.md §4 "Per-point routes").  256 float32 levels under an odd pitch are one row per pass,
    ``kPwUnroll`` rows per workgroup and sweep, so two sweeps and one row of the capped grid are 2 · 65536 · 4 + 1 rows = 539 MB.  In
    place, y = x · 1.5 - 3 on x = row % 1021 + level (exact in float32), numpy on the host.  Measured on an MI355X: 0.2 s wall."""
    grid = C.K.stream_grid
    n_lev, pitch = C.K.block, C.K.block + 1
    n_pts = 2 * grid * C.K.unroll + 1
    t0 = time.perf_counter()
    rows = torch.arange(n_pts, device=dev, dtype=torch.int32).remainder_(1021).to(torch.float32)
    buf = torch.full((n_pts + 2, pitch), -7.0, dtype=torch.float32, device=dev)  # a canary row before and after, a padding column
    body = buf[1:-1]
    body[:, :n_lev] = rows[:, None] + torch.arange(n_lev, device=dev, dtype=torch.float32)[None, :]
    prog = kern.level_program([[C.AFF] * n_lev], dev)
    kern.pointwise_stack(body, body, n_pts=n_pts, n_lev=n_lev, x_pitch=pitch, y_pitch=pitch, layout=C.COLUMNS, prog=prog, n_stage=1)
    assert kern.last_route() == "row_chunk_scalar"
    got = buf.cpu().numpy()
    want = ((np.arange(n_pts, dtype=np.int32) % 1021).astype(np.float32)[:, None] + np.arange(n_lev, dtype=np.float32)[None, :]) * np.float32(1.5) + np.float32(-3.0)
    assert np.array_equal(got[1:-1, :n_lev], want)
    assert (got[0] == -7.0).all() and (got[-1] == -7.0).all() and (got[:, n_lev] == -7.0).all()
    print(f"row-chunk kernel past the cap: {n_pts} rows, {buf.numel() * 4 / 1e6:.0f} MB, {time.perf_counter() - t0:.2f} s wall")


def test_flat_kernel_past_the_grid_cap(dev, kern):
    """The flat kernel serves stacks too tall for the per-level tables, which no full-size test has (DESIGN.md §4 "Per-point routes"):
    2001 float64 levels, two stages with parameters of every level's own, and enough points for two 16 KB chunks more than
    ``kStreamGrid`` — every workgroup of the launch strides on to a second chunk; 1.07 GB, the smallest stack that does.  In place, on
    x = point % 1021 + level / 2 (exact), numpy on the host.  Measured on an MI355X: 1.1 s wall, nearly all of it the host
    copy and numpy's four passes over 134 M doubles."""
    grid = C.K.stream_grid
    n_lev = C.K.tall_levels()
    cols = -(-n_lev // 2)
    n_pts = -(-((grid + 1) * C.K.block * C.K.unroll + 1) // cols)
    t0 = time.perf_counter()
    a = 1.0 + 0.001 * np.arange(n_lev)
    b = -0.25 * np.arange(n_lev)
    g = 1.0 + 1.0 / (1.0 + np.arange(n_lev))
    stages = [[(native.OP_AFFINE, 0, float(a[l]), float(b[l])) for l in range(n_lev)],
              [(native.OP_CLIP, 0, 250.0, 300.0) if l % 3 else (native.OP_MUL, 0, float(g[l]), 0.0) for l in range(n_lev)]]
    buf = torch.full((n_pts + 2, 2 * cols), -7.0, dtype=torch.float64, device=dev)  # a canary row before and after
    body = buf[1:-1]
    body[:, :n_lev] = torch.arange(n_pts, device=dev, dtype=torch.int32).remainder_(1021).to(torch.float64)[:, None]
    body[:, :n_lev] += 0.5 * torch.arange(n_lev, device=dev, dtype=torch.float64)[None, :]
    prog = kern.level_program(stages, dev)
    kern.pointwise_stack(body, body, n_pts=n_pts, n_lev=n_lev, x_pitch=2 * cols, y_pitch=2 * cols, layout=C.COLUMNS, prog=prog, n_stage=2)
    assert kern.last_route() == "flat"
    got = buf.cpu().numpy()
    del buf, body
    want = (np.arange(n_pts) % 1021).astype(np.float64)[:, None] + 0.5 * np.arange(n_lev)[None, :]
    want *= a[None, :]
    want += b[None, :]
    scaled = np.arange(n_lev) % 3 == 0
    want[:, scaled] *= g[None, scaled]
    want[:, ~scaled] = np.clip(want[:, ~scaled], 250.0, 300.0)
    assert np.array_equal(got[1:-1, :n_lev], want)
    assert (got[0] == -7.0).all() and (got[-1] == -7.0).all()
    print(f"flat kernel past the cap: {n_pts} points x {n_lev} levels, {got.nbytes / 1e6:.0f} MB, {time.perf_counter() - t0:.2f} s wall")
