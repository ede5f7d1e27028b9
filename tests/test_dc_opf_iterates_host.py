"""CPU checks behind ``tests/test_dc_opf_iterates_gpu.py``: the two float64 references of the DC optimal power flow against each
other.  ``dc_opf_reduced_reference`` follows the contract's method (include/gns_powerflow.h, "DC optimal power flow": shift factors,
a Gn x Gn matrix, a scalar lambda, the figures with |p|_inf); ``dc_opf_reference`` solves the full (theta, p) KKT system.  Theta
stays the DC solution at p in the full formulation, so both take the same dp, dz, dmu and step lengths: their iterates after k
updates agree to rounding, and how far they are apart is the yardstick of the device's iterates (``dc_opf_pin_cases.yardstick``).
Their iteration counts differ (theta is in the full reference's termination figures), so only the reduced one pins the count.

Measured on the CPU, the largest over the sets of each group (relative, ``dc_opf_pin_cases.yardstick``):

    k                         0          1          2          3
    dc_opf_cases.SETS         2.3e-13    9.1e-13    3.3e-11    1.5e-10
    dc_opf_pin_cases.SETS     7.9e-14    1.6e-12    3.8e-12    5.0e-10

and the iteration counts at tol = 1e-8: equal on 44 of the 54 grids, the reduced reference's one above on 8 (the three path sets,
hub150_qp[1], hub150_lp[0]) and two above on 2 (hub150_qp[0], hub150_lp[1]); near ties (``dc_opf_reduced_reference.near_tie``):
13 of 54, all in ``dc_opf_cases.SETS`` (the new sets' seeds are drawn so that they add none, ``dc_opf_pin_cases.SEEDS``)."""
import numpy as np
import pytest

import dc_opf_cases as cases
import dc_opf_pin_cases as pin
import dc_opf_reduced_reference as reduced

YARDSTICK_BAR = 1e-8


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_two_references_agree_iterate_by_iterate(name):
    """pg, mu_line, mu_pmax and mu_pmin after k = 0, 1, 2, 3 updates, every grid: within 1e-8 relative."""
    for k in pin.KS:
        y = pin.yardstick(name, k)
        print(f'{name} k {k}: reduced - full {y:.2e}')
        assert y < YARDSTICK_BAR, (name, k, y)
    for r in pin.iterates(name, 0):
        assert r['lam'] == 0.0 and r['iterations'] == 0


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_two_references_agree_at_the_optimum(name):
    bars = cases.bars(name)
    for g, (r, f) in enumerate(zip(pin.runs(name), cases.optimum(name))):
        assert r['converged'] and f['converged'], (name, g)
        assert len(r['worst']) == r['iterations'] + 1
        print(f"{name}[{g}] iterations reduced {r['iterations']} full {f['iterations']}")
        assert abs(r['objective'] - f['objective']) / max(1.0, abs(f['objective'])) <= bars['objective'], (name, g)
        assert np.abs(r['pg'] - f['pg']).max() <= bars['pg'], (name, g)
        assert np.abs(r['lmp'] - f['lmp']).max() <= bars['lmp'], (name, g)


def test_reduced_reference_at_the_start_and_by_hand():
    """k = 0 on the closed-form grid: the midpoint, mu = 1 / z, lambda = 0, lmp = -PTDF^T mu_line; and the closed-form optimum."""
    p = cases.problems('three_bus')[0]
    r = reduced.iterate(*p, 0)
    assert np.array_equal(r['pg'], [1.0, 1.0]) and r['lam'] == 0.0 and r['objective'] == 40.0
    assert np.array_equal(r['mu_pmax'], [1.0, 1.0]) and np.array_equal(r['mu_pmin'], [1.0, 1.0])
    # the flow of line 1-3 at the midpoint: 2/3 of the load from the slack less 1/3 of unit 2's output (the slack's unit has a zero
    # column of S), 1/3 under a rating of 0.5: both slacks start at 1, mu_line = 0
    assert np.array_equal(r['z0_line'], [1.0, 1.0]) and np.array_equal(r['mu_line'], [0.0, 0.0, 0.0])
    assert abs(r['line_flow'][1] - 1.0 / 3.0) <= 1e-12
    opt = reduced.solve(*p)
    assert opt['converged'] and np.abs(opt['pg'] - np.array(cases.THREE_BUS_PG)).max() <= 1e-7
    assert np.abs(opt['lmp'] - np.array(cases.THREE_BUS_LMP)).max() <= 1e-5 and abs(opt['mu_line'][1] - cases.THREE_BUS_MU) <= 1e-5


def test_the_new_sets_keep_their_promises():
    print(pin.check())
    assert not set(pin.SETS) & set(cases.SETS) and set(pin.ALL_SETS) == set(pin.SETS) | set(cases.SETS)


def test_near_ties_are_at_most_a_quarter_of_the_grids():
    """The count test lets a near tie differ by one; that must stay the exception."""
    total = sum(len(pin.runs(name)) for name in pin.ALL_SETS)
    ties = pin.near_ties()
    print(f'near ties: {len(ties)} of {total}: {ties}')
    assert 4 * len(ties) <= total, (ties, total)
    assert reduced.near_tie([1.0, 1.9e-8, 1e-9]) and reduced.near_tie([1.0, 5e-9]) and not reduced.near_tie([1.0, 2.1e-8, 4.9e-9])
