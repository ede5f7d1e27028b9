"""CPU checks behind ``tests/test_dc_scopf_iterates_gpu.py``: what the sets of ``dc_scopf_pin_cases`` promise, the two float64
references of the security-constrained DC optimal power flow against each other iterate by iterate, and the bookkeeping of the
iteration count.

``dc_scopf_reference.solve`` follows the contract's method with the rows of the rebuilt networks' shift factors;
``solve_full`` carries an angle vector per network.  Every network's angles stay its DC solution at p, so both take the same dp,
dz, dmu and step lengths: after k updates they agree to rounding on pg, mu_line, mu_row, mu_pmax and mu_pmin, and how far they are
apart is the yardstick of the device's iterates (``dc_scopf_pin_cases.yardstick``).  The lmp is left out: away from the optimum the
full formulation's balance multipliers and the reduced ``-lambda - PTDF^T mu`` are different quantities (O(1) apart at k = 0).

Measured on the CPU, the largest over the sets of each group (relative):

    k                          0          1          2          3
    dc_scopf_cases.SETS        2.1e-15    2.1e-13    7.7e-12    5.3e-10
    dc_scopf_pin_cases.SETS    8.2e-14    9.6e-13    1.8e-10    1.5e-10

The count.  At the default tolerance 26 of the 40 grids are near ties (``dc_opf_reduced_reference.near_tie``; 14 of the 20 grids of
``dc_scopf_cases.SETS``): the largest figure falls tenfold per iteration at the end, so [tol / 2, 2 tol] catches most runs.  Per
grid ``dc_scopf_pin_cases.count_at`` therefore takes the tolerance in [1e-9, 1e-7] that is farthest from every figure of the
reference's run to 1e-10; with a tenfold fall that is a factor sqrt(10) = 3.16 from the nearest figure, and ``check()`` asserts
at least 2.2 on every grid."""
import numpy as np
import pytest

import dc_scopf_cases as cases
import dc_scopf_pin_cases as pin
import dc_scopf_reference as ref

YARDSTICK_BAR = 1e-8


def test_the_new_sets_keep_their_promises():
    print(pin.check())
    assert not set(pin.SETS) & set(cases.SETS) and set(pin.ALL_SETS) == set(pin.SETS) | set(cases.SETS)
    assert set(cases.OTHER_SETS) >= set(pin.SETS)


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_two_formulations_agree_iterate_by_iterate(name):
    """pg, mu_line, mu_row, mu_pmax and mu_pmin after k = 0, 1, 2, 3 updates, every grid: within 1e-8 relative."""
    for k in pin.KS:
        y = pin.yardstick(name, k)
        print(f'{name} k {k}: reduced - full {y:.2e}')
        assert y < YARDSTICK_BAR, (name, k, y)
    for r in pin.iterates(name, 0):
        assert r['lam'] == 0.0 and r['iterations'] == 0 and len(r['figures']) == 1


def test_the_full_reference_path_is_its_run_to_k():
    """``solve_full(path=...)``'s iterate k is what ``solve_full(max_iter=k)`` returns, bit for bit."""
    name = 'case14_qp'
    p, rc, rows = pin.grids(name)[1]
    for k in (0, 2):
        want, got = ref.solve_full(*p, rows, rc, max_iter=k), pin.full_iterates(name, k)[1]
        assert want['iterations'] == got['iterations'] == k
        assert all(np.array_equal(want[key], got[key]) for key in pin.FIELDS + ('lmp',))


def test_the_additive_returns_of_the_reference():
    """``figures`` is the largest figure of every termination test; ``solve_full``'s multipliers at the optimum are ``solve``'s."""
    name = 'case14_qp'
    (p, rc), r = cases.problems(name)[0], cases.optimum(name)[0]
    assert len(r['figures']) == r['iterations'] + 1 and r['figures'][-1] == r['worst'] < ref.DEFAULT_TOL
    assert all(f >= ref.DEFAULT_TOL for f in r['figures'][:-1])
    f = ref.solve_full(*p, cases.rows_of(name, 0), rc)
    bar = cases.bars(name)['lmp']
    for key in ('mu_line', 'mu_pmax', 'mu_pmin', 'mu_row'):
        assert f[key].shape == r[key].shape and np.abs(f[key] - r[key]).max() <= bar, key


def test_the_count_is_pinned_where_no_tie_exists():
    """``tol_of`` on runs written by hand; per grid the reference run again at its own tolerance stops where ``count_at`` says, and
    no figure of that run lies within a factor 2.2 of the tolerance."""
    tol, ratio = pin.tol_of([1.0, 1e-2, 5e-8, 5e-9, 5e-10])       # the ends are a factor 2 from a figure, the gaps' middles sqrt(10)
    assert any(abs(tol - np.sqrt(10.0) * f) <= 1e-20 for f in (5e-9, 5e-10)) and abs(ratio - np.sqrt(10.0)) <= 1e-9
    tol, ratio = pin.tol_of([1.0, 3e-8])                          # the only gap's middle is outside the range: an end of it
    assert tol == pin.TOL_RANGE[0] and abs(ratio - 30.0) <= 1e-9
    assert pin.tol_of([1.6e-7 * 0.5 ** i for i in range(10)])[1] < pin.TIE_MARGIN      # a run that halves its figure has no such tolerance
    total = 0
    for name in pin.ALL_SETS:
        for g, ((p, rc, rows), (tol, ratio, count)) in enumerate(zip(pin.grids(name), pin.count_at(name))):
            assert pin.TOL_RANGE[0] <= tol <= pin.TOL_RANGE[1] and ratio >= pin.TIE_MARGIN, (name, g, tol, ratio)
            r = ref.solve(*p, rows, rc, tol=tol)
            assert r['converged'] and r['iterations'] == count, (name, g, r['iterations'], count)
            assert not any(tol / pin.TIE_MARGIN <= f <= pin.TIE_MARGIN * tol for f in r['figures']), (name, g)
            total += 1
    ties = pin.near_ties()
    print(f'near ties at the default tolerance: {len(ties)} of {total}: {ties}')
    assert total == sum(len(cases.problems(name)) for name in pin.ALL_SETS)
