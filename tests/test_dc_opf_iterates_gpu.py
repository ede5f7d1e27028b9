"""GPU checks of the path ``powerflow.dc_optimal_power_flow`` takes, not only of where it ends (include/gns_powerflow.h, "DC optimal
power flow"): the start (``max_iter = 0``), the iterate after 1, 2 and 3 updates against ``dc_opf_reduced_reference`` (the contract's
method in dense float64 numpy), the iteration count at the default tolerance, bit-identity of an early iterate, and the sets of
``dc_opf_pin_cases`` through the checks of ``tests/test_dc_opf_gpu.py``.  An interior point corrects itself: a wrong normal
matrix, gamma, step length or tile edge still reaches the optimum, by another path; these tests look at the path.

Bars.  The start: the project's DC bar ``1e-9 max(1, max|ref|)``.  An iterate: ten times the set's yardstick at that k (how far
the reduced and the full float64 reference are apart there, ``dc_opf_pin_cases.yardstick``, computed on the CPU) plus the DC bar,
at the scale of the reference's value (``dc_opf_pin_cases.iterate_bar``).  The count: equal, except that a near tie
(``dc_opf_reduced_reference.near_tie``: the reference's worst figure within [tol / 2, 2 tol] at some test) may differ by one.

Measured: yardstick (CPU) and the device's worst difference on an MI355X, both relative (``max|a - b| / max(1, max|ref|)``, the
largest over the grids and over pg, mu_line, mu_pmax, mu_pmin; for the device also objective and lmp), per set and k:

    set               yardstick k = 0 / 1 / 2 / 3                 device k = 0 / 1 / 2 / 3
    three_bus         0.0e+00 / 1.1e-15 / 1.8e-15 / 1.6e-13       0.0e+00 / 4.4e-16 / 1.8e-15 / 4.1e-15
    case14_qp         0.0e+00 / 6.8e-14 / 1.3e-12 / 6.1e-12       0.0e+00 / 1.8e-15 / 1.4e-12 / 1.2e-12
    case14_lp         8.9e-16 / 8.0e-15 / 5.4e-13 / 3.9e-12       8.9e-16 / 1.7e-15 / 6.1e-13 / 2.5e-12
    case14_no_rating  0.0e+00 / 5.6e-15 / 3.4e-13 / 2.2e-12       2.0e-16 / 6.2e-16 / 8.9e-14 / 1.7e-12
    one_unit          7.8e-16 / 3.1e-14 / 1.1e-13 / 3.1e-12       4.2e-15 / 8.9e-15 / 4.9e-13 / 3.2e-13
    slack_unit        0.0e+00 / 1.7e-14 / 1.9e-12 / 2.1e-12       0.0e+00 / 1.3e-15 / 1.4e-13 / 1.2e-13
    stacked_units     5.6e-16 / 7.4e-14 / 9.1e-13 / 2.9e-11       1.4e-15 / 1.8e-15 / 2.0e-12 / 2.7e-12
    ring30            2.1e-15 / 1.0e-14 / 2.6e-12 / 1.6e-11       1.6e-15 / 3.4e-15 / 4.0e-13 / 9.6e-13
    path64            6.1e-15 / 5.6e-13 / 2.3e-11 / 1.5e-10       4.8e-14 / 8.2e-13 / 8.3e-12 / 8.3e-12
    path65            5.1e-15 / 9.1e-13 / 2.4e-11 / 2.3e-11       1.9e-14 / 2.4e-13 / 3.3e-11 / 3.3e-11
    path66_pv         2.3e-13 / 5.5e-13 / 3.3e-11 / 4.5e-12       5.3e-13 / 6.8e-13 / 2.3e-12 / 2.5e-12
    hub150_qp         9.8e-14 / 9.2e-13 / 1.1e-12 / 7.0e-13       1.3e-13 / 2.5e-13 / 2.1e-13 / 9.7e-12
    hub150_lp         9.3e-14 / 1.4e-13 / 1.8e-13 / 5.6e-12       1.5e-13 / 2.4e-13 / 2.7e-13 / 2.0e-12
    gn3               0.0e+00 / 1.2e-13 / 4.6e-13 / 9.4e-12       0.0e+00 / 6.6e-16 / 5.7e-13 / 7.6e-13
    gn4               0.0e+00 / 1.4e-14 / 3.0e-13 / 1.2e-11       0.0e+00 / 1.3e-15 / 2.8e-13 / 1.0e-11
    gn5               0.0e+00 / 4.2e-14 / 2.9e-13 / 3.6e-12       0.0e+00 / 1.3e-15 / 2.8e-13 / 3.9e-12
    gn40              0.0e+00 / 4.1e-14 / 1.4e-12 / 1.7e-11       1.8e-16 / 7.0e-15 / 2.2e-12 / 2.4e-11
    gn41              0.0e+00 / 1.7e-14 / 1.6e-12 / 5.0e-10       1.8e-16 / 1.7e-15 / 1.1e-12 / 2.0e-11
    gn63              0.0e+00 / 4.5e-14 / 1.1e-12 / 2.2e-11       0.0e+00 / 3.6e-15 / 8.5e-13 / 5.1e-11
    gn64              0.0e+00 / 6.4e-14 / 3.8e-12 / 6.5e-11       1.3e-16 / 1.0e-14 / 1.9e-12 / 1.3e-10
    gn65              0.0e+00 / 1.3e-13 / 1.6e-12 / 1.5e-11       2.3e-16 / 1.0e-14 / 1.2e-12 / 1.5e-11
    narrow_chunk      9.9e-14 / 1.6e-12 / 8.0e-13 / 1.3e-12       6.9e-14 / 5.5e-14 / 7.2e-14 / 1.6e-13
    mixed_c2          0.0e+00 / 1.4e-14 / 7.0e-13 / 3.1e-12       1.3e-16 / 1.0e-15 / 2.5e-13 / 2.1e-12
    low_pmin          0.0e+00 / 1.9e-14 / 6.0e-13 / 2.9e-12       0.0e+00 / 2.0e-15 / 6.6e-13 / 3.2e-12
    wide              3.3e-16 / 6.3e-14 / 1.9e-12 / 8.9e-12       5.6e-16 / 2.7e-15 / 2.5e-13 / 2.5e-12
    mixed_ratings     1.2e-15 / 2.9e-13 / 4.4e-13 / 4.7e-11       1.8e-15 / 3.6e-15 / 1.1e-12 / 4.7e-12

Every bar above is (10 yardstick + 1e-9), so the device stays a factor of 7 or more inside it.  The device's iteration count equals
the reduced reference's on all 54 grids, the 13 near ties included.
"""
import numpy as np
import pytest
import torch

import dc_opf_cases as cases
import dc_opf_pin_cases as pin
import dc_opf_reduced_reference as reduced
import dc_reference
import test_dc_opf_gpu as base

pytestmark = pytest.mark.gpu
COMPARED = ('pg', 'mu_line', 'mu_pmax', 'mu_pmin', 'objective', 'lmp')
EARLY = (1, 2, 3)

_AT = {}


def _at(name, k):
    """The device's result on a set after at most k updates, computed once and left unchanged."""
    if (name, k) not in _AT:
        _AT[name, k] = base._run(cases.batch(name), max_iter=k)
        torch.cuda.synchronize()
    return _AT[name, k]


def _dc_bar(want):
    return cases.DC_BAR * max(1.0, float(np.abs(want).max()))


def _rel(got, want):
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _check_theta_and_flows(res, name):
    """theta and line_flow are the DC power flow at the returned dispatch, whatever the iterate."""
    for g, p in enumerate(cases.problems(name)):
        r = base._grid(res, g)
        gens = p[2].copy()
        gens[:, 6] = r['pg']
        theta, flow, _ = dc_reference.dc_power_flow(torch.from_numpy(p[0]), torch.from_numpy(p[1]), torch.from_numpy(gens), p[5])
        for got, want in ((r['theta'], theta.numpy()), (r['line_flow'], flow.numpy())):
            assert np.abs(got - want).max() <= _dc_bar(want), (name, g)


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_start(name):
    res, b = _at(name, 0), cases.batch(name)
    Bt = b.buses.shape[0]
    assert res.iterations.tolist() == [0] * Bt and not bool(res.converged.any())
    assert torch.equal(res.pg.cpu(), 0.5 * (b.gens[:, :, 1].double() + b.gens[:, :, 2].double()))
    worst = 0.0
    for g, (p, want) in enumerate(zip(cases.problems(name), pin.iterates(name, 0))):
        r = base._grid(res, g)
        nl = want['z0_line'].size // 2
        lim = np.isfinite(p[4])
        # the start rule, written out: mu = 1 / z with z = max(1, -h) at the midpoint, lambda = 0
        pmid, flow = 0.5 * (p[2][:, 1] + p[2][:, 2]), want['line_flow']
        mu_line = np.zeros(lim.size)
        mu_line[lim] = 1.0 / np.maximum(1.0, p[4][lim] - flow[lim]) - 1.0 / np.maximum(1.0, p[4][lim] + flow[lim])
        rule = dict(mu_pmax=1.0 / np.maximum(1.0, p[2][:, 1] - pmid), mu_pmin=1.0 / np.maximum(1.0, pmid - p[2][:, 2]), mu_line=mu_line,
                    objective=np.float64(p[3][:, 0] @ pmid ** 2 + p[3][:, 1] @ pmid))
        assert nl == int(lim.sum()) and want['lam'] == 0.0
        for k, v in rule.items():
            assert np.abs(want[k] - v).max() <= 1e-13 * max(1.0, np.abs(v).max()), (name, g, k)      # the reference obeys it
            assert np.abs(r[k] - v).max() <= _dc_bar(v), (name, g, k)
        assert np.all(r['mu_line'][~lim] == 0.0)
        assert np.abs(r['lmp'] - want['lmp']).max() <= _dc_bar(want['lmp']), (name, g)               # -PTDF^T mu_line: lambda = 0
        worst = max([worst] + [_rel(r[k], want[k]) for k in COMPARED])
    print(f'PIN {name} k 0 yardstick {pin.yardstick(name, 0):.1e} device {worst:.1e}')
    _check_theta_and_flows(res, name)


@pytest.mark.parametrize('k', EARLY)
@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_iterate_after_k_updates(name, k):
    res = _at(name, k)
    Bt = res.pg.shape[0]
    assert res.iterations.tolist() == [k] * Bt and not bool(res.converged.any())
    worst, over = 0.0, []
    for g, want in enumerate(pin.iterates(name, k)):
        r = base._grid(res, g)
        for key in COMPARED:
            diff, bar = float(np.abs(r[key] - want[key]).max()), pin.iterate_bar(name, k, want[key])
            worst = max(worst, _rel(r[key], want[key]))
            if not diff <= bar:
                over.append((g, key, diff, bar))
    print(f'PIN {name} k {k} yardstick {pin.yardstick(name, k):.1e} device {worst:.1e}')
    assert not over, (name, k, over)
    _check_theta_and_flows(res, name)


@pytest.mark.parametrize('name', pin.ALL_SETS)
def test_the_iteration_count(name):
    res = base._result(name)
    wrong = []
    for g, want in enumerate(pin.runs(name)):
        got, tie = int(res.iterations[g]), reduced.near_tie(want['worst'])
        print(f"COUNT {name}[{g}] device {got} reference {want['iterations']}" + (' (near tie)' if tie else ''))
        assert bool(res.converged[g]) and want['converged']
        if abs(got - want['iterations']) > (1 if tie else 0):
            wrong.append((g, got, want['iterations'], tie))
    assert not wrong, (name, wrong)


def test_an_early_iterate_is_bit_identical_alone_in_a_batch_and_permuted():
    name, k = 'gn65', 2
    b = cases.batch(name)
    assert b.gens.shape[1] > 64 and b.cost.dim() == 3 and b.rating.dim() == 2
    whole = _at(name, k)
    assert whole.iterations.tolist() == [k, k]
    assert base._same_bits(whole, base._run(b, max_iter=k))
    perm = [1, 0]
    got = base._run(cases.Batch(b.buses[perm], b.lines[perm], b.gens[perm], b.cost[perm].contiguous(), b.rating[perm].contiguous(), b.slack),
                    max_iter=k)
    assert base._same_bits([t[perm] for t in whole], got)
    for g in range(2):
        alone = base._run(cases.Batch(b.buses[g:g + 1], b.lines[g:g + 1], b.gens[g:g + 1], b.cost[g:g + 1].contiguous(),
                                      b.rating[g:g + 1].contiguous(), b.slack), max_iter=k)
        assert base._same_bits([t[g:g + 1] for t in whole], alone)


@pytest.mark.parametrize('name', tuple(pin.SETS))
def test_the_new_sets_through_the_existing_checks(name):
    """Convergence with a KKT certificate, theta and the flows at the dispatch, the optimum against the full reference."""
    base.test_every_grid_converges_with_a_kkt_certificate(name)
    base.test_theta_and_flows_are_the_dc_power_flow_at_the_dispatch(name)
    base.test_optimum_against_the_reference(name)
