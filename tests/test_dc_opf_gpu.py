"""GPU checks of ``powerflow.dc_optimal_power_flow`` (include/gns_powerflow.h, "DC optimal power flow") on the sets of
``dc_opf_cases``: every grid converges; the KKT certificate recomputed on the host in float64 from the returned tensors alone
(``dc_opf_reference.kkt_residuals``) is within ``tol + 1e-12 max(1, scale)``; the multipliers' signs; ``theta`` and ``line_flow``
against ``dc_reference.dc_power_flow`` at the returned dispatch kept in float64, within the project's DC bar
``1e-9 max(1, max|ref|)``; ``objective``, ``pg`` and ``lmp`` against the reference optimum; bitwise reproducibility; per-grid
failures; the LDS refusal.

The bars of ``objective``, ``pg`` and ``lmp`` (``dc_opf_cases.bars``): ten times how far the reference's own values move between
``tol`` and ``tol / 1000`` (``yardstick``: what stopping inside the tolerance ball alone allows), plus the DC bar.  Yardsticks
measured on the CPU at tol = 1e-8, and the device's worst differences measured on an MI355X (objective relative, pg and lmp
absolute), per set:

    set               yardstick objective / pg / lmp     device objective / pg / lmp
    three_bus         4.4e-11 / 4.4e-11 / 1.2e-09        0.00e+00 / 0.00e+00 / 2.91e-13
    case14_qp         3.9e-11 / 1.5e-09 / 1.0e-07        2.33e-15 / 3.60e-14 / 2.63e-11
    case14_lp         3.0e-11 / 1.4e-10 / 6.8e-08        6.99e-16 / 1.89e-15 / 7.48e-12
    case14_no_rating  3.4e-11 / 7.8e-10 / 7.8e-09        7.50e-16 / 2.11e-15 / 4.26e-14
    one_unit          1.1e-15 / 2.2e-15 / 1.4e-07        4.29e-15 / 8.44e-15 / 1.21e-13
    slack_unit        1.1e-11 / 7.0e-11 / 9.0e-08        3.53e-16 / 2.66e-15 / 5.83e-13
    stacked_units     7.5e-12 / 6.9e-10 / 9.7e-08        7.67e-16 / 8.95e-14 / 3.54e-12
    ring30            4.7e-12 / 1.4e-10 / 4.3e-08        1.01e-15 / 7.55e-15 / 1.15e-11
    path64            7.2e-14 / 8.6e-13 / 2.6e-06        5.16e-14 / 6.18e-13 / 2.38e-06
    path65            2.6e-14 / 5.0e-13 / 3.0e-06        3.59e-14 / 6.82e-13 / 2.70e-06
    path66_pv         4.9e-12 / 3.9e-10 / 1.4e-06        4.49e-12 / 3.49e-10 / 1.24e-06
    hub150_qp         5.5e-11 / 8.3e-09 / 2.5e-07        5.49e-11 / 8.19e-09 / 2.50e-07
    hub150_lp         5.8e-11 / 2.2e-09 / 4.2e-07        5.73e-11 / 2.15e-09 / 4.15e-07
"""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow
import dc_opf_cases as cases
import dc_opf_reference as ref
import dc_reference
import pf_topologies as pt

pytestmark = pytest.mark.gpu
TOL = ref.DEFAULT_TOL
FIELDS = powerflow.DcOpfResult._fields


def _run(b, **kw):
    dev = 'cuda'
    return powerflow.dc_optimal_power_flow(b.buses.to(dev), b.lines.to(dev), b.gens.to(dev), cost=b.cost, rating=b.rating,
                                           slack_bus=b.slack, **kw)


_RESULTS = {}


def _result(name):
    """The device's result on a set, computed once and left unchanged."""
    if name not in _RESULTS:
        _RESULTS[name] = _run(cases.batch(name))
        torch.cuda.synchronize()
    return _RESULTS[name]


def _grid(res, g):
    return {k: getattr(res, k)[g].cpu().numpy() for k in FIELDS}


def _same_bits(a, b):
    def bits(x):
        return x.reshape(-1).contiguous().view(torch.uint8).cpu()
    a, b = list(a), list(b)
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_every_grid_converges_with_a_kkt_certificate(name):
    res = _result(name)
    b = cases.batch(name)
    assert res.pg.dtype == torch.float64 and res.converged.dtype == torch.bool and res.iterations.dtype == torch.int32
    assert tuple(res.pg.shape) == tuple(b.gens.shape[:2]) and tuple(res.lmp.shape) == tuple(b.buses.shape[:2])
    assert tuple(res.mu_line.shape) == tuple(b.lines.shape[:2]) and res.pg.device.type == 'cuda'
    for g, p in enumerate(cases.problems(name)):
        r = _grid(res, g)
        assert r['converged'] and 0 < r['iterations'] <= ref.DEFAULT_MAX_ITER, (name, g, r['iterations'])
        k = ref.kkt_residuals(r, p)
        bar = TOL + 1e-12 * k['scale']
        print(f"{name}[{g}] it {r['iterations']} feas {k['feas']:.2e} grad {k['grad']:.2e} comp {k['comp']:.2e} "
              f"mu_off {k['mu_off']:.2e} min_mu {k['min_mu']:.2e} bar {bar:.2e}")
        assert k['feas'] <= bar and k['grad'] <= bar and k['comp'] <= bar, (name, g, k)
        assert k['min_mu'] >= 0.0 and np.all(r['mu_pmax'] >= 0.0) and np.all(r['mu_pmin'] >= 0.0), (name, g)
        assert k['mu_off'] <= bar, (name, g, k)
        assert np.all(r['mu_line'][~np.isfinite(p[4])] == 0.0)
        c2, c1 = p[3][:, 0], p[3][:, 1]
        assert abs(r['objective'] - float(c2 @ r['pg'] ** 2 + c1 @ r['pg'])) <= 1e-12 * max(1.0, abs(r['objective']))


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_theta_and_flows_are_the_dc_power_flow_at_the_dispatch(name):
    res = _result(name)
    for g, p in enumerate(cases.problems(name)):
        r = _grid(res, g)
        gens = p[2].copy()
        gens[:, 6] = r['pg']                                              # the returned dispatch, kept in float64
        theta, flow, _ = dc_reference.dc_power_flow(torch.from_numpy(p[0]), torch.from_numpy(p[1]), torch.from_numpy(gens), p[5])
        for got, want in ((r['theta'], theta.numpy()), (r['line_flow'], flow.numpy())):
            assert np.abs(got - want).max() <= cases.DC_BAR * max(1.0, np.abs(want).max()), (name, g)


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_optimum_against_the_reference(name):
    res, bars = _result(name), cases.bars(name)
    worst = dict(objective=0.0, pg=0.0, lmp=0.0)
    for g, want in enumerate(cases.optimum(name)):
        r = _grid(res, g)
        worst['objective'] = max(worst['objective'], abs(r['objective'] - want['objective']) / max(1.0, abs(want['objective'])))
        worst['pg'] = max(worst['pg'], np.abs(r['pg'] - want['pg']).max())
        worst['lmp'] = max(worst['lmp'], np.abs(r['lmp'] - want['lmp']).max())
    print(f'{name}: device - reference ' + ' '.join(f'{k} {worst[k]:.2e} (bar {bars[k]:.2e})' for k in worst))
    for k in worst:
        assert worst[k] <= bars[k], (name, k, worst[k], bars[k])


def test_closed_form_three_bus():
    r = _grid(_result('three_bus'), 0)
    assert np.abs(r['pg'] - np.array(cases.THREE_BUS_PG)).max() <= 1e-7
    assert np.abs(r['lmp'] - np.array(cases.THREE_BUS_LMP)).max() <= 1e-5
    assert abs(r['mu_line'][1] - cases.THREE_BUS_MU) <= 1e-5


def test_single_grid_and_cpu_inputs():
    b = cases.batch('case14_qp')
    one = powerflow.dc_optimal_power_flow(b.buses[1], b.lines[1], b.gens[1], cost=b.cost[1], rating=b.rating[1], slack_bus=b.slack)
    assert one.pg.dim() == 1 and one.converged.dim() == 0 and one.pg.device.type == 'cpu'
    want = _result('case14_qp')
    assert _same_bits([t for t in one], [t[1].cpu() for t in want])


@pytest.mark.parametrize('name', ('case14_qp', 'case14_lp', 'hub150_lp', 'path66_pv'))
def test_bitwise_alone_in_a_batch_permuted_and_again(name):
    b = cases.batch(name)
    Bt = b.buses.shape[0]
    whole = _result(name)
    again = _run(b)
    assert _same_bits(whole, again)
    cost3 = b.cost if b.cost.dim() == 3 else b.cost.expand(Bt, -1, -1)
    rating2 = None if b.rating is None else (b.rating if b.rating.dim() == 2 else b.rating.expand(Bt, -1))
    perm = list(range(Bt))[::-1]
    p = cases.Batch(b.buses[perm], b.lines[perm], b.gens[perm], cost3[perm].contiguous(),
                    None if rating2 is None else rating2[perm].contiguous(), b.slack)
    got = _run(p)
    assert _same_bits([t[perm] for t in whole], got)
    for g in range(Bt):
        alone = _run(cases.Batch(b.buses[g:g + 1], b.lines[g:g + 1], b.gens[g:g + 1], cost3[g:g + 1].contiguous(),
                                 None if rating2 is None else rating2[g:g + 1].contiguous(), b.slack))
        assert _same_bits([t[g:g + 1] for t in whole], alone)


def _others_untouched(clean, got, bad):
    keep = [g for g in range(clean.pg.shape[0]) if g != bad]
    assert _same_bits([t[keep] for t in clean], [t[keep] for t in got])


def _not_solved(got, g):
    assert int(got.iterations[g]) == -1 and not bool(got.converged[g])
    for k in FIELDS[:8]:
        assert bool(torch.isnan(getattr(got, k)[g]).all()), k


def test_per_grid_failures_leave_the_other_grids_alone():
    b = cases.batch('case14_qp')
    clean = _result('case14_qp')
    # a NaN Pd
    buses = b.buses.clone()
    buses[1, 3, 2] = float('nan')
    got = _run(b._replace(buses=buses))
    _not_solved(got, 1)
    _others_untouched(clean, got, 1)
    # Pmin > Pmax at one unit
    gens = b.gens.clone()
    gens[0, 2, 1], gens[0, 2, 2] = gens[0, 2, 2].item(), gens[0, 2, 1].item()
    got = _run(b._replace(gens=gens))
    _not_solved(got, 0)
    _others_untouched(clean, got, 0)
    # demand above sum Pmax
    buses = b.buses.clone()
    buses[2, 5, 2] += 2.0 * b.gens[2, :, 1].sum()
    got = _run(b._replace(buses=buses))
    _not_solved(got, 2)
    _others_untouched(clean, got, 2)
    # a rating that no dispatch within the bounds meets: not converged, the last iterate finite
    rating = b.rating.clone()
    rating[1] = 1e-6                                                      # every line: no flow at all, with loads of 0.1 and more
    got = _run(b._replace(rating=rating), max_iter=40)
    assert not bool(got.converged[1]) and 0 <= int(got.iterations[1]) <= 40
    for k in FIELDS[:8]:
        assert bool(torch.isfinite(getattr(got, k)[1]).all()), k
    _others_untouched(clean, got, 1)


def test_max_iter_keeps_the_last_iterate():
    b = cases.batch('case14_lp')
    got = _run(b, max_iter=3)
    assert not bool(got.converged.any()) and got.iterations.tolist() == [3, 3, 3]
    assert all(bool(torch.isfinite(getattr(got, k)).all()) for k in FIELDS[:8])
    zero = _run(b, max_iter=0)
    pmid = 0.5 * (b.gens[:, :, 1].double() + b.gens[:, :, 2].double())
    assert torch.equal(zero.pg.cpu(), pmid) and zero.iterations.tolist() == [0, 0, 0]


def test_lds_refusal_raises_and_launches_nothing():
    tp = pt.star(251, 'pv')                                               # 251 units: the packed normal matrix alone is 253 008 B
    n, e, gn = tp.n, tp.f.size, tp.g.size
    buses = torch.zeros(1, n, 6)
    buses[0, :, 0], buses[0, :, 1], buses[0, :, 2] = torch.arange(1, n + 1), 1.0, 0.1
    lines = torch.zeros(1, e, 7)
    lines[0, :, 0], lines[0, :, 1], lines[0, :, 3], lines[0, :, 5] = torch.from_numpy(tp.f), torch.from_numpy(tp.t), 0.1, 1.0
    gens = torch.zeros(1, gn, 7)
    gens[0, :, 0], gens[0, :, 1] = torch.from_numpy(tp.g), 1.0
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as err:
        powerflow.dc_optimal_power_flow(buses.cuda(), lines.cuda(), gens.cuda(), cost=torch.ones(gn, 2, dtype=torch.float64),
                                        slack_bus=tp.slack)
    assert 'Gn (Gn + 1) / 2' in str(err.value)
    torch.cuda.synchronize()
