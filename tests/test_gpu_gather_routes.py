"""Every launch form of the gather on the device, held to scipy's and numpy's bits by the checks of tests/gather_route_checks.py: each
case declares the route it is written for and asserts ``native.last_gather_route()`` took it, then compares every element — the plain
gather with scipy's csr_matvec bit for bit in float32 as in float64 (the pure k = 1 gather as a bit copy), arithmetic program levels with
the chain csr_matvec -> numpy bit for bit, exp / log levels against exact arithmetic at the budgets of tests/ulp_budgets.py, the same
bits on every route that serves the same program, canaries and padding untouched, inputs unchanged.
tests/test_gather_route_checks_catch_defects.py shows each assertion failing on a planted defect."""

from __future__ import annotations

import pytest

import gather_route_checks as G
from anemoi_transform_amd import native

pytestmark = pytest.mark.gpu

CASES = G.all_cases()


@pytest.fixture
def kern():
    try:
        yield G.Kernels(regrid_ell=native.regrid_ell, regrid_ell_batch=native.regrid_ell_batch, regrid_csr=native.regrid_csr,
                        last_gather_route=native.last_gather_route, last_route=native.last_route, level_program=native.level_program,
                        set_tuning=native.set_tuning)
    finally:
        native.set_tuning(0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_takes_its_route_and_gives_the_chains_bits(dev, kern, case):
    assert G.check_case(kern, dev, case) == case.route


def test_a_gather_without_targets_launches_nothing(dev, kern):
    G.check_nothing_launched(kern, dev)


def test_every_route_has_a_case():
    """Adding a launch form without a case written for it fails here (the list is next to the constants: ``G.ROUTE_CLASSES``)."""
    assert G.declared_route_classes(CASES) == set(G.ROUTE_CLASSES)
