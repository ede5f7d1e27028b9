"""GPU checks of ``powerflow.dc_security_constrained_opf`` and ``powerflow.dc_secure_dispatch`` (include/gns_powerflow.h,
"Security-constrained DC optimal power flow") on the sets of ``dc_scopf_cases``, against ``dc_scopf_reference``, which takes every
row from the network rebuilt without the outaged line and never from the line-outage formula.

Bars.  ``objective``, ``pg``, ``lmp``: ``dc_opf_cases.bars``' rule computed for these sets (``dc_scopf_cases.bars``): ten times how far
the reference's own values move between ``tol`` and ``tol / 1000``, plus the DC bar ``1e-9 max(1, max|ref|)``.  ``line_flow`` and
``row_flow``: the DC bar against the reference evaluated at the device's own ``pg`` kept in float64.  ``mu_row``: through the KKT
certificate recomputed in float64 from the returned values alone (``dc_scopf_reference.kkt_residuals``), within
``tol + 1e-12 scale`` like ``dc_optimal_power_flow``'s; that certificate also holds the returned ``lmp`` against its definition from
the returned multipliers on the rebuilt networks' own distribution factors, and every row's feasibility."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import powerflow
import dc_opf_cases as base_cases
import dc_scopf_cases as cases
import dc_scopf_reference as ref
import dc_reference
import dc_wide_cases as wide

pytestmark = pytest.mark.gpu
TOL = ref.DEFAULT_TOL
FIELDS = powerflow.DcScopfResult._fields
DEV = 'cuda'


def _run(c, rows=None, rows_on=DEV, **kw):
    b = c.batch
    kw.setdefault('contingency_rating', c.rating_c)
    kw.setdefault('rating', b.rating)
    rows = c.rows if rows is None else rows
    return powerflow.dc_security_constrained_opf(b.buses.to(DEV), b.lines.to(DEV), b.gens.to(DEV), cost=b.cost, rows=rows.to(rows_on),
                                                 slack_bus=b.slack, **kw)


def _opf(b, **kw):
    return powerflow.dc_optimal_power_flow(b.buses.to(DEV), b.lines.to(DEV), b.gens.to(DEV), cost=b.cost, rating=b.rating,
                                           slack_bus=b.slack, **kw)


_RESULTS = {}


def _result(name):
    """The device's result on a set, computed once and left unchanged."""
    if name not in _RESULTS:
        _RESULTS[name] = _run(cases.case(name))
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
def test_optimum_against_the_reference(name):
    res, bars, c = _result(name), cases.bars(name), cases.case(name)
    Bt, R = c.batch.buses.shape[0], c.rows.shape[-2]
    assert res.pg.dtype == torch.float64 and res.converged.dtype == torch.bool and res.iterations.dtype == torch.int32
    assert tuple(res.mu_row.shape) == (Bt, R) == tuple(res.row_flow.shape) and res.mu_row.dtype == torch.float64
    worst = dict(objective=0.0, pg=0.0, lmp=0.0)
    for g, want in enumerate(cases.optimum(name)):
        r = _grid(res, g)
        assert r['converged'] and 0 < r['iterations'] <= ref.DEFAULT_MAX_ITER, (name, g, r['iterations'])
        worst['objective'] = max(worst['objective'], abs(r['objective'] - want['objective']) / max(1.0, abs(want['objective'])))
        worst['pg'] = max(worst['pg'], np.abs(r['pg'] - want['pg']).max())
        worst['lmp'] = max(worst['lmp'], np.abs(r['lmp'] - want['lmp']).max())
        print(f"{name}[{g}] iterations device {r['iterations']} reference {want['iterations']}")
    print(f'{name}: device - reference ' + ' '.join(f'{k} {worst[k]:.2e} (bar {bars[k]:.2e})' for k in worst))
    for k in worst:
        assert worst[k] <= bars[k], (name, k, worst[k], bars[k])


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_flows_rows_and_the_kkt_certificate(name):
    res = _result(name)
    for g, (p, rc) in enumerate(cases.problems(name)):
        r, rows = _grid(res, g), cases.rows_of(name, g)
        empty = (rows[:, 0] < 0) | ~np.isfinite(rc[np.maximum(rows[:, 0], 0)])     # (-1, -1), or a line without a contingency rating
        gens = p[2].copy()
        gens[:, 6] = r['pg']                                              # the returned dispatch, kept in float64
        theta, flow, _ = dc_reference.dc_power_flow(torch.from_numpy(p[0]), torch.from_numpy(p[1]), torch.from_numpy(gens), p[5])
        want_rows, _ = ref.row_values(p[0], p[1], p[2], p[5], rows, r['pg'])
        for what, got, want in (('theta', r['theta'], theta.numpy()), ('line_flow', r['line_flow'], flow.numpy()),
                                ('row_flow', r['row_flow'][~empty], want_rows[~empty])):
            err, bar = np.abs(got - want).max(), base_cases.DC_BAR * max(1.0, np.abs(want).max())
            print(f'{name}[{g}] {what} {err:.2e} (bar {bar:.2e})')
            assert err <= bar, (name, g, what)
        assert np.all(np.isnan(r['row_flow'][empty])) and np.all(r['mu_row'][empty] == 0.0), (name, g)
        k = ref.kkt_residuals(r, p, rows, rc)
        bar = TOL + 1e-12 * k['scale']
        print(f"{name}[{g}] grad {k['grad']:.2e} comp {k['comp']:.2e} lmp_def {k['lmp_def']:.2e} max_h {k['max_h']:.2e} "
              f"min_mu {k['min_mu']:.2e} bar {bar:.2e}")
        assert k['grad'] <= bar and k['comp'] <= bar and k['lmp_def'] <= bar, (name, g, k)
        assert k['min_mu'] >= 0.0 and k['max_h'] <= bar * k['feas_scale'], (name, g, k)      # every row and line within its limit
        lim = np.array([rc[l] for l in rows[~empty, 0]])
        assert np.all(np.abs(r['row_flow'][~empty]) <= lim + bar * k['feas_scale']), (name, g)


def test_closed_form_three_bus():
    r = _grid(_result('three_bus'), 0)
    rows = cases.rows_of('three_bus', 0)
    at = int(np.flatnonzero(rows[:, 0] >= 0)[0])
    assert np.abs(r['pg'] - np.array(cases.THREE_BUS_PG)).max() <= 1e-7 and abs(r['objective'] - cases.THREE_BUS_OBJECTIVE) <= 1e-6
    assert abs(r['mu_row'][at] - cases.THREE_BUS_MU_ROW) <= 1e-5 and abs(r['row_flow'][at] - 0.6) <= 1e-7
    assert np.abs(r['lmp'] - np.array(cases.THREE_BUS_LMP)).max() <= 1e-5
    assert np.all(r['mu_line'] == 0.0)


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_every_slot_empty_is_dc_optimal_power_flow_bit_for_bit(name):
    c = cases.case(name)
    want = _opf(c.batch)
    got = _run(c, rows=torch.full_like(c.rows, -1))
    assert _same_bits(list(want), list(got)[:10])
    assert bool((got.mu_row == 0).all()) and bool(torch.isnan(got.row_flow).all())
    # and so is a list whose monitored lines have no contingency rating
    got = _run(c, contingency_rating=torch.full_like(c.rating_c, float('inf')))
    assert _same_bits(list(want), list(got)[:10])
    assert bool((got.mu_row == 0).all()) and bool(torch.isnan(got.row_flow).all())


def _per_grid(c):
    """The case with cost, ratings and rows per grid."""
    b, Bt = c.batch, c.batch.buses.shape[0]
    cost = b.cost if b.cost.dim() == 3 else b.cost.expand(Bt, -1, -1).contiguous()
    rating = None if b.rating is None else (b.rating if b.rating.dim() == 2 else b.rating.expand(Bt, -1).contiguous())
    rating_c = c.rating_c if c.rating_c.dim() == 2 else c.rating_c.expand(Bt, -1).contiguous()
    rows = c.rows if c.rows.dim() == 3 else c.rows.expand(Bt, -1, -1).contiguous()
    return c._replace(batch=b._replace(cost=cost, rating=rating), rating_c=rating_c, rows=rows)


def _take(c, idx):
    b = c.batch
    return c._replace(batch=b._replace(buses=b.buses[idx], lines=b.lines[idx], gens=b.gens[idx], cost=b.cost[idx].contiguous(),
                                       rating=None if b.rating is None else b.rating[idx].contiguous()),
                      rating_c=c.rating_c[idx].contiguous(), rows=c.rows[idx].contiguous())


@pytest.mark.parametrize('name', ('case14_qp', 'case14_lp', 'meshed14', 'wheel_lp_r65'))
def test_bitwise_alone_in_a_batch_reversed_shared_and_again(name):
    c = cases.case(name)
    Bt = c.batch.buses.shape[0]
    whole = _result(name)
    assert _same_bits(whole, _run(c))
    pg = _per_grid(c)
    assert _same_bits(whole, _run(pg))                                     # shared against per-grid lists, costs and ratings
    perm = list(range(Bt))[::-1]
    assert _same_bits([t[perm] for t in whole], _run(_take(pg, perm)))
    for g in range(Bt):
        assert _same_bits([t[g:g + 1] for t in whole], _run(_take(pg, [g])))


def test_single_grid_and_cpu_inputs():
    c = cases.case('case14_qp')
    b = c.batch
    one = powerflow.dc_security_constrained_opf(b.buses[1], b.lines[1], b.gens[1], cost=b.cost[1], rating=b.rating[1],
                                                contingency_rating=c.rating_c[1], rows=c.rows[1].tolist(), slack_bus=b.slack)
    assert one.pg.dim() == 1 and one.mu_row.dim() == 1 and one.pg.device.type == 'cpu'
    assert _same_bits(list(one), [t[1].cpu() for t in _result('case14_qp')])


def _not_solved(got, g):
    assert int(got.iterations[g]) == -1 and not bool(got.converged[g])
    for k in FIELDS[:8] + FIELDS[10:]:
        assert bool(torch.isnan(getattr(got, k)[g]).all()), k


def _others_untouched(clean, got, bad):
    keep = [g for g in range(clean.pg.shape[0]) if g != bad]
    assert _same_bits([t[keep] for t in clean], [t[keep] for t in got])


def test_failure_rows_fail_their_grid_alone():
    c = _per_grid(cases.case('meshed14'))
    clean = _result('meshed14')
    E = c.batch.lines.shape[1]
    f, t = c.batch.lines[0, :, 0].long().numpy() - 1, c.batch.lines[0, :, 1].long().numpy() - 1
    bridge = int(np.flatnonzero(powerflow._bridges(c.batch.buses.shape[1], f, t))[0])
    other = 0 if bridge != 0 else 1
    slot = 4                                                              # an empty slot of every list
    assert bool((c.rows[:, slot] == -1).all())
    for g, bad in ((0, (E, 0)), (1, (0, E)), (0, (-1, 3)), (1, (3, -2)), (0, (5, 5)), (1, (other, bridge))):
        rows = c.rows.clone()
        rows[g, slot] = torch.tensor(bad, dtype=rows.dtype)
        got = _run(c, rows=rows)                                          # a device tensor: passed through, the kernel's rule applies
        _not_solved(got, g)
        _others_untouched(clean, got, g)
        with pytest.raises(ValueError, match=r'rows\[%d, %d\]' % (g, slot)):
            _run(c, rows=rows, rows_on='cpu')                             # the same list on the CPU: refused by name
    # a bridge whose monitored line has no contingency rating is an empty slot
    rows = c.rows.clone()
    rows[1, slot] = torch.tensor((other, bridge), dtype=rows.dtype)
    rc = c.rating_c.clone()
    rc[1, other] = float('inf')
    got = _run(c, rows=rows, contingency_rating=rc)
    assert bool(got.converged.all()) and float(got.mu_row[1, slot]) == 0.0 and bool(torch.isnan(got.row_flow[1, slot]))


def test_zero_denominator_fails_its_grid_alone():
    """``dc_wide_cases.zero_den_batch``: the outage of the b = 2 line has den = 1 - 2 * 1/2 = 0 exactly and is no bridge."""
    buses, lines, gens, slack = wide.zero_den_batch()
    gens = gens.clone()
    gens[..., 1], gens[..., 2] = 3.0, 0.0
    Gn, E = gens.shape[1], lines.shape[1]
    cost = torch.tensor([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0]], dtype=torch.float64)[:Gn]
    rc = torch.full((E,), 10.0, dtype=torch.float64)

    def run(rows):
        return powerflow.dc_security_constrained_opf(buses.to(DEV), lines.to(DEV), gens.to(DEV), cost=cost, contingency_rating=rc,
                                                     rows=torch.tensor(rows, dtype=torch.int32, device=DEV), slack_bus=slack)
    clean = run([[[0, 1], [-1, -1]], [[0, 1], [-1, -1]]])
    assert bool(clean.converged.all())
    got = run([[[0, 1], [-1, -1]], [[0, 1], [0, wide.ZD_B2]]])
    _not_solved(got, 1)
    _others_untouched(clean, got, 1)


def test_contingency_rating_none_falls_back_to_rating():
    """Rows on lines with a base rating and on lines without one: without a contingency rating the first are held to the base
    rating and the second are empty slots, bit for bit what passing the rating as the contingency rating gives.  The rows on rated
    lines are chosen on the CPU so that the problem is feasible on every grid (the set's reference optimum keeps them below 0.98
    of the base rating) and means something (the base optimum of some grid overloads them)."""
    name = 'case14_lp'
    c = cases.case(name)
    rating = c.batch.rating
    assert rating is not None and rating.dim() == 1 and bool(torch.isinf(rating).any()) and bool(torch.isfinite(rating).any())
    E, rt = rating.numel(), rating.numpy()
    at_opt, at_base = [], []
    for (p, rc), opt in zip(cases.problems(name), cases.optimum(name)):
        base = ref.solve(*p, np.zeros((0, 2), dtype=int), rc)
        at_opt.append(np.abs(ref.post_flows(p[0], p[1], p[2], p[5], opt['pg'], c.outages)) / rt[None, :])
        at_base.append(np.abs(ref.post_flows(p[0], p[1], p[2], p[5], base['pg'], c.outages)) / rt[None, :])
    at_opt, at_base = np.max(at_opt, axis=0), np.max(at_base, axis=0)                  # [K,E], the worst over the grids
    rated = [(l, int(k)) for i, k in enumerate(c.outages) for l in range(E)
             if l != k and np.isfinite(rt[l]) and at_opt[i, l] <= 0.98 and at_base[i, l] > 1.0][:3]
    assert len(rated) >= 1, 'no pair is both feasible at the set optimum and overloaded at the base optimum'
    k0 = int(c.outages[0])
    free = [(l, k0) for l in torch.isinf(rating).nonzero().flatten().tolist() if l != k0][:2]
    rows = torch.tensor(rated + free + [(-1, -1)], dtype=torch.int32)
    got = _run(c, rows=rows, contingency_rating=None)
    assert _same_bits(got, _run(c, rows=rows, contingency_rating=rating))
    flow, n = got.row_flow.cpu(), len(rated)
    lim = rating[[l for l, _ in rated]]
    print('rows', rated, 'converged', got.converged.tolist(), 'row_flow / rating', (flow[:, :n].abs() / lim).tolist())
    assert bool(got.converged.all())
    assert bool(torch.isfinite(flow[:, :n]).all()) and bool(torch.isnan(flow[:, n:]).all())
    assert bool((got.mu_row.cpu()[:, n:] == 0).all())
    assert bool((flow[:, :n].abs() <= lim * (1 + 1e-7)).all())
    assert bool((flow[:, :n].abs() > lim * (1 - 1e-6)).any())                        # a row binds at its base rating


def test_an_infeasible_grid_leaves_its_neighbours_alone():
    c = _per_grid(cases.case('case14_qp'))
    clean = _result('case14_qp')
    rc = c.rating_c.clone()
    rc[1] = 1e-6                                    # no post-outage flow at all, with loads of 0.05 and more: no dispatch meets it
    got = _run(c, contingency_rating=rc, max_iter=40)
    assert not bool(got.converged[1]) or bool(torch.isnan(got.pg[1]).all())
    _others_untouched(clean, got, 1)


def test_a_bridge_in_a_cpu_list_is_refused_by_name():
    c = cases.case('meshed14')
    b = c.batch
    f, t = b.lines[0, :, 0].long().numpy() - 1, b.lines[0, :, 1].long().numpy() - 1
    bridge = int(np.flatnonzero(powerflow._bridges(b.buses.shape[1], f, t))[0])
    with pytest.raises(ValueError, match=r'rows\[1\] = \(\d+, %d\): the outage of line %d disconnects the grid' % (bridge, bridge)):
        powerflow.dc_security_constrained_opf(b.buses.to(DEV), b.lines.to(DEV), b.gens.to(DEV), cost=b.cost, rating=b.rating,
                                              contingency_rating=c.rating_c, rows=[[-1, -1], [(bridge + 1) % b.lines.shape[1], bridge]],
                                              slack_bus=b.slack)


@pytest.mark.parametrize('name', sorted(cases.DRIVER_SETS))
def test_dc_secure_dispatch_gpu(name):
    """The driver against the reference optimum with every row listed, at the same bars as the set (``dc_scopf_cases.bars``);
    ``secure`` everywhere; the reference's float64 post-outage loading at the returned dispatch within ``1 + violation_tol``."""
    c = cases.case(name)
    b = c.batch
    rounds, per_round = cases.DRIVER_SETS[name]
    out = powerflow.dc_secure_dispatch(b.buses.to(DEV), b.lines.to(DEV), b.gens.to(DEV), cost=b.cost, rating=b.rating,
                                       contingency_rating=c.rating_c, rounds=rounds, rows_per_round=per_round, slack_bus=b.slack)
    Bt = b.buses.shape[0]
    assert tuple(out.rows.shape) == (Bt, rounds * per_round, 2) and out.rows.dtype == torch.int32
    assert tuple(out.worst_loading.shape) == (Bt,) and out.secure.dtype == torch.bool
    want, bars = cases.secure_optimum(name), cases.bars(name)
    res = out.result
    for g, (p, rc) in enumerate(cases.problems(name)):
        r = _grid(res, g)
        err = dict(objective=abs(r['objective'] - want[g]['objective']) / max(1.0, abs(want[g]['objective'])),
                   pg=np.abs(r['pg'] - want[g]['pg']).max(), lmp=np.abs(r['lmp'] - want[g]['lmp']).max())
        load = np.abs(ref.post_flows(p[0], p[1], p[2], p[5], r['pg'], c.outages)) / rc[None, :]
        n_rows = int((out.rows[g, :, 0] >= 0).sum())
        print(f"{name}[{g}] rows {n_rows} worst loading device {float(out.worst_loading[g]):.9f} reference {load.max():.9f} " +
              ' '.join(f'{k} {err[k]:.2e} (bar {bars[k]:.2e})' for k in err))
        assert r['converged'] and bool(out.secure[g]), (name, g)
        assert load.max() <= 1.0 + cases.VIOLATION_TOL, (name, g, load.max())
        for k in err:
            assert err[k] <= bars[k], (name, g, k, err[k], bars[k])
        assert n_rows >= 1


def test_a_grid_secure_from_the_start_returns_dc_optimal_power_flow():
    b, rating_c, _ = cases.SECURE_FROM_THE_START()
    out = powerflow.dc_secure_dispatch(b.buses.to(DEV), b.lines.to(DEV), b.gens.to(DEV), cost=b.cost, rating=b.rating,
                                       contingency_rating=rating_c, rounds=2, rows_per_round=4, slack_bus=b.slack)
    assert bool((out.rows == -1).all()) and bool(out.secure.all())
    assert _same_bits(list(_opf(b)), list(out.result)[:10])
