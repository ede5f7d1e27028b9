"""The AC contingency screen on the MI355X (``powerflow.ac_contingency_screen``, include/gns_powerflow.h "AC contingency
screening"): every (grid, outage) row against the float64 reference (``ac_contingency_reference``: the line's row deleted, the
reference Newton-Raphson warm-started from the reference's own base solution, the flows from the dense makeYbus quantities), against
the product's other route (``newton_raphson(mixed_topologies=True)`` on the expanded batch, one analysis per outage), bit identity
of rows, failure rows, ratings, parallel lines and a line from a bus to itself.

Bars: where the reference converges with at least two iterations to spare the device row has converged with the same iteration
count, ``v`` and ``theta`` within 1e-9 absolute (the bar of test_powerflow_mixed_gpu), flows and summaries within 1e-8; the index
outputs are equal wherever the reference's runner-up is more than 1e-6 away.  Rows the reference leaves unconverged (overloaded
post-outage grids) are left out of the value comparison only; at least 60 % of the non-islanding pairs must be compared."""
import functools

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import ac_contingency_reference as aref
import nr_reference as nr
import pf_topologies as pt
from test_ac_contingency_host import toy
from test_powerflow_mixed_gpu import _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL, MAX_IT = 1e-8, 10
ROWS = ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus',
        'converged', 'iterations', 'mismatch')


def _screen(s, **kw):
    return powerflow.ac_contingency_screen(s[0], s[1], s[2], slack_bus=s[3], **kw)


@functools.lru_cache(maxsize=None)
def _case(case, batch, seed=0):
    """(buses, lines, gens, slack) of ``solvable_grids`` on the device, and the screen of every line: made once, never changed."""
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, batch, seed=seed, device=DEV)
    s = (buses, lines, gens, slack)
    return s, _screen(s)


@functools.lru_cache(maxsize=None)
def _reference(case, batch, seed=0):
    """{(grid, line): Row or None} for every line of every grid of ``_case`` and the reference's base solutions: computed once."""
    (buses, lines, gens, slack), _ = _case(case, batch, seed)
    b, l, g = (t.cpu().double().numpy() for t in (buses, lines, gens))
    rows, bases = {}, []
    for i in range(batch):
        base = aref.base_case(b[i], l[i], g[i], slack, TOL, MAX_IT)
        bases.append(base)
        for k in range(l.shape[1]):
            rows[i, k] = aref.outage(b[i], l[i], g[i], slack, k, base[0], base[1], TOL, MAX_IT)
    return rows, bases


def _not_solved(res, g, j):
    for k in ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'v_min', 'v_max', 'mismatch'):
        assert bool(getattr(res, k)[g, j].isnan().all()), k
    for k in ('worst_line', 'v_min_bus', 'v_max_bus', 'iterations'):
        assert bool((getattr(res, k)[g, j] == -1).all()), k
    assert not bool(res.converged[g, j].any())


def _compare(res, s, rows, outages, grids, name, rating=None):
    """Rows ``res[i, j]`` of grid ``grids[i]`` and line ``outages[j]`` against the reference rows; returns (compared, non-islanding)."""
    buses, lines, gens, slack = s
    b, l, g = (t.cpu().double().numpy() for t in (buses, lines, gens))
    host = {k: getattr(res, k).cpu().numpy() for k in ROWS}
    n_cmp = n_pairs = 0
    worst = dict(v=0.0, theta=0.0, flow=0.0, summary=0.0)
    for i, gi in enumerate(grids):
        rt = None if rating is None else (rating if rating.dim() == 1 else rating[i]).cpu().numpy()
        for j, k in enumerate(outages):
            want = rows[gi, k]
            assert (want is None) == bool(res.islanding[j]), (name, gi, k)
            if want is None:
                _not_solved(res, i, j)
                continue
            n_pairs += 1
            got = {key: host[key][i, j] for key in ROWS}
            print(f"{name} grid {gi} line {k}: reference converged {want.converged} in {want.iterations}, device {bool(got['converged'])} "
                  f"in {int(got['iterations'])}, mismatch {float(got['mismatch']):.2e}")
            assert np.isfinite(got['v']).all() and np.isfinite(got['theta']).all(), (name, gi, k)
            assert got['p_from'][k] == got['q_from'][k] == got['p_to'][k] == got['q_to'][k] == 0.0, (name, gi, k)
            if got['converged']:
                assert got['mismatch'] < TOL, (name, gi, k)
                rest = np.delete(l[gi], k, axis=0)
                assert nr.mismatch(b[gi], rest, g[gi], slack, got['v'], got['theta']) < 1e-7, (name, gi, k)
            if not (want.converged and want.iterations <= MAX_IT - 2):
                continue
            n_cmp += 1
            assert got['converged'] and int(got['iterations']) == want.iterations, (name, gi, k, int(got['iterations']), want.iterations)
            ev, et = np.max(np.abs(got['v'] - want.v)), np.max(np.abs(got['theta'] - want.theta))
            ef = max(np.max(np.abs(got[key] - getattr(want, key))) for key in ('p_from', 'q_from', 'p_to', 'q_to'))
            load = aref.loading(want, rt)
            wl, wi, wgap = aref.extreme(load)
            lo, lo_i, lo_gap = aref.extreme(want.v, largest=False)
            hi, hi_i, hi_gap = aref.extreme(want.v)
            es = max(abs(got['worst_loading'] - wl), abs(got['v_min'] - lo), abs(got['v_max'] - hi))
            worst = dict(v=max(worst['v'], ev), theta=max(worst['theta'], et), flow=max(worst['flow'], ef), summary=max(worst['summary'], es))
            assert ev <= 1e-9 and et <= 1e-9, (name, gi, k, ev, et)
            assert ef <= 1e-8 and es <= 1e-8, (name, gi, k, ef, es)
            if wgap > 1e-6:
                assert int(got['worst_line']) == wi, (name, gi, k)
            if lo_gap > 1e-6:
                assert int(got['v_min_bus']) == lo_i, (name, gi, k)
            if hi_gap > 1e-6:
                assert int(got['v_max_bus']) == hi_i, (name, gi, k)
    print(f'{name}: compared {n_cmp} of {n_pairs} non-islanding pairs; worst errors {worst}')
    return n_cmp, n_pairs


def _check_base(res, s):
    base = powerflow.newton_raphson(s[0], s[1], s[2], slack_bus=s[3], tol=TOL, max_iter=MAX_IT)
    for k in base._fields:
        assert _same(getattr(res.base, k), getattr(base, k)), k


def _check_summaries_from_flows(res, rating=None):
    """The summaries against torch on the returned tensors (the lowest index among equals), bit for bit but for the square root."""
    s = torch.maximum(torch.hypot(res.p_from, res.q_from), torch.hypot(res.p_to, res.q_to))
    load = s if rating is None else s / (rating if rating.dim() == 1 else rating.unsqueeze(-2))
    top = load.amax(dim=-1)
    ok = ~res.islanding & res.base.converged.unsqueeze(-1) & torch.isfinite(top)
    bar = 1e-12 * top.clamp(min=1.0)               # the kernel's sqrt(p^2 + q^2) against hypot: a few ulp of the value
    assert bool(((res.worst_loading - top).abs() <= bar)[ok].all())
    at_line = load.gather(-1, res.worst_line.clamp(min=0).long().unsqueeze(-1)).squeeze(-1)
    assert bool(((at_line - top).abs() <= bar)[ok].all())
    N = res.v.shape[-1]
    for val, idx, ext in ((res.v_min, res.v_min_bus, res.v.amin(dim=-1)), (res.v_max, res.v_max_bus, res.v.amax(dim=-1))):
        assert torch.equal(val[ok], ext[ok])
        first = torch.where(res.v == ext.unsqueeze(-1), torch.arange(N, device=res.v.device), N).amin(dim=-1)
        assert torch.equal(idx[ok].long(), first[ok])


def test_case14_every_line_against_the_reference():
    s, res = _case(14, 3)
    E, N = 20, 14
    rows, bases = _reference(14, 3)
    assert res.outages.tolist() == list(range(E)) and res.outages.dtype == torch.int64
    assert res.v.shape == res.theta.shape == (3, E, N) and res.p_from.shape == res.q_to.shape == (3, E, E)
    for k in ('worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus', 'converged', 'iterations', 'mismatch'):
        assert getattr(res, k).shape == (3, E), k
    assert res.v.dtype == res.q_from.dtype == res.worst_loading.dtype == res.v_min.dtype == res.mismatch.dtype == torch.float64
    assert res.worst_line.dtype == res.v_min_bus.dtype == res.v_max_bus.dtype == res.iterations.dtype == torch.int32
    assert res.converged.dtype == res.islanding.dtype == torch.bool and res.islanding.shape == (E,)
    f, t, _ = synth.case_topology(14)
    assert res.islanding.tolist() == powerflow._bridges(14, f - 1, t - 1).tolist() and int(res.islanding.sum()) == 1
    _check_base(res, s)
    assert bool(res.base.converged.all())
    for i, base in enumerate(bases):                     # the reference's own base solution is the device's to the bar
        assert base[2] and np.max(np.abs(res.base.v[i].cpu().numpy() - base[0])) <= 1e-9
    n_cmp, n_pairs = _compare(res, s, rows, list(range(E)), range(3), 'case14')
    assert n_pairs == 57 and n_cmp >= 0.6 * n_pairs, (n_cmp, n_pairs)
    _check_summaries_from_flows(res)


def test_rows_are_bit_identical_in_any_list_batch_and_option(monkeypatch):
    s, full = _case(14, 3)
    buses, lines, gens, slack = s
    E = lines.shape[1]

    def same_rows(part, grids, cols, fields=ROWS):
        for k in fields:
            assert _same(getattr(part, k), getattr(full, k)[grids][:, cols]), k

    again = _screen(s)                                                           # from run to run
    same_rows(again, slice(None), list(range(E)))
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1)).tolist()
    p = _screen(s, outages=torch.tensor(perm, device=DEV))                        # a permuted list, as a device tensor
    same_rows(p, slice(None), perm)
    assert torch.equal(p.islanding, full.islanding[perm]) and p.outages.tolist() == perm
    dup = [7, 3, 7, 19, 0, 7]                                                    # duplicates are independent rows
    p = _screen(s, outages=dup)
    same_rows(p, slice(None), dup)
    p = _screen(s, outages=[11])                                                 # one outage
    same_rows(p, slice(None), [11])
    p = _screen((buses[1:2], lines[1:2], gens[1:2], slack))                      # one grid
    same_rows(p, slice(1, 2), list(range(E)))
    single = powerflow.ac_contingency_screen(buses[2], lines[2], gens[2], slack_bus=slack, outages=[4, 17])     # 2-D
    assert single.v.shape == (2, 14) and single.worst_loading.shape == (2,) and single.base.v.shape == (14,)
    for k in ROWS:
        assert _same(getattr(single, k), getattr(full, k)[2][[4, 17]]), k
    slim = _screen(s, flows=False)
    assert slim.p_from is None and slim.q_from is None and slim.p_to is None and slim.q_to is None
    same_rows(slim, slice(None), list(range(E)), [k for k in ROWS if k[:2] not in ('p_', 'q_')])
    slim = _screen(s, states=False)
    assert slim.v is None and slim.theta is None
    same_rows(slim, slice(None), list(range(E)), [k for k in ROWS if k not in ('v', 'theta')])
    slim = _screen(s, states=False, flows=False, outages=dup)
    same_rows(slim, slice(None), dup, ROWS[6:])
    cpu = powerflow.ac_contingency_screen(buses.cpu(), lines.cpu(), gens.cpu(), slack_bus=slack, outages=[1, 2])
    assert all(t.device.type == 'cpu' for t in (cpu.v, cpu.p_from, cpu.worst_line, cpu.converged, cpu.islanding, cpu.outages, cpu.base.v))
    for k in ROWS:
        assert _same(getattr(cpu, k), getattr(full, k)[:, [1, 2]].cpu()), k
    req = lines.clone().requires_grad_(True)                                     # not differentiable
    r = powerflow.ac_contingency_screen(buses, req, gens, slack_bus=slack, outages=[0])
    assert not r.v.requires_grad and not r.p_from.requires_grad and not r.base.v.requires_grad
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', True)                      # nothing is read that nothing wrote
    poisoned = _screen(s)
    same_rows(poisoned, slice(None), list(range(E)))


def test_agrees_with_the_expanded_route():
    """The other route: every (grid, outage) pair as a grid of its own with the line's row deleted, one analysis per outage,
    ``newton_raphson(mixed_topologies=True)`` warm-started from the base.  The base analysis serves every outage."""
    s, res = _case(14, 3)
    buses, lines, gens, slack = s
    E = lines.shape[1]
    keep = torch.tensor([[e for e in range(E) if e != k] for k in range(E)], device=DEV)            # [E, E-1]
    xl = lines[:, keep].reshape(3 * E, E - 1, 7).contiguous()
    xb, xg = buses.repeat_interleave(E, dim=0), gens.repeat_interleave(E, dim=0)
    v0, th0 = res.base.v.repeat_interleave(E, dim=0), res.base.theta.repeat_interleave(E, dim=0)
    mixed = powerflow.newton_raphson(xb, xl, xg, slack_bus=slack, mixed_topologies=True, v0=v0, theta0=th0, tol=TOL, max_iter=MAX_IT)
    conv = mixed.converged.reshape(3, E)
    assert torch.equal(conv, res.converged)
    assert torch.equal((mixed.iterations == -1).reshape(3, E), res.islanding.expand(3, E))
    assert int(conv.sum()) >= 0.6 * 57
    dv = (mixed.v.reshape(3, E, -1) - res.v).abs().amax(dim=-1)[conv]
    dth = (mixed.theta.reshape(3, E, -1) - res.theta).abs().amax(dim=-1)[conv]
    print(f'expanded route: {int(conv.sum())} converged pairs, max |dv| {float(dv.max()):.2e}, max |dtheta| {float(dth.max()):.2e}')
    assert float(dv.max()) <= 1e-9 and float(dth.max()) <= 1e-9


def test_a_grid_without_a_base_solution_fails_alone_and_ratings():
    s, good = _case(14, 3)
    buses, lines, gens, slack = s
    E = lines.shape[1]
    bad = buses.clone()
    bad[1, :, 2:4] *= 40.0                                                       # loads no network of this size can serve
    res = _screen((bad, lines, gens, slack))
    assert res.base.converged.tolist() == [True, False, True]
    _not_solved(res, 1, slice(None))
    for k in ROWS:
        assert _same(getattr(res, k)[[0, 2]], getattr(good, k)[[0, 2]]), k
    assert torch.equal(res.islanding, good.islanding)
    rows, _ = _reference(14, 3)
    g = torch.Generator().manual_seed(E)
    for shape in ((E,), (3, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=g, dtype=torch.float64)).to(DEV)
        rated = _screen(s, rating=rating)
        for k in ROWS:
            if k not in ('worst_loading', 'worst_line'):
                assert _same(getattr(rated, k), getattr(good, k)), k
        _check_summaries_from_flows(rated, rating)
        n_cmp, n_pairs = _compare(rated, s, rows, list(range(E)), range(3), f'case14 rating {shape}', rating=rating)
        assert n_cmp >= 0.6 * n_pairs
        slim = _screen(s, rating=rating, flows=False, states=False)
        assert _same(slim.worst_loading, rated.worst_loading) and torch.equal(slim.worst_line, rated.worst_line)
    r32 = _screen(s, rating=torch.ones(E, dtype=torch.float32))                  # converted to float64
    assert _same(r32.worst_loading, good.worst_loading)


@pytest.mark.parametrize('name', ['toy_parallel_selfloop', 'random40_parallel_selfloop'])
def test_parallel_lines_and_a_line_from_a_bus_to_itself(name):
    tp = toy() if name == 'toy_parallel_selfloop' else pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, lines, gens, tp.slack)
    res = _screen(s)
    E = tp.f.size
    b, l, g = (t.cpu().double().numpy() for t in (buses, lines, gens))
    rows = {}
    for i in range(2):
        base = aref.base_case(b[i], l[i], g[i], tp.slack, TOL, MAX_IT)
        assert base[2]
        for k in range(E):
            rows[i, k] = aref.outage(b[i], l[i], g[i], tp.slack, k, base[0], base[1], TOL, MAX_IT)
    _check_base(res, s)
    n_cmp, n_pairs = _compare(res, s, rows, list(range(E)), range(2), name)
    assert n_cmp >= 0.6 * n_pairs
    pairs = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    loops = [e for e, (a_, b_) in enumerate(pairs) if a_ == b_]
    doubled = [e for e, p in enumerate(pairs) if pairs.count(p) > 1 and p[0] != p[1]]
    assert loops and len(doubled) >= 2
    assert not bool(res.islanding[loops + doubled].any())                        # neither is ever a bridge
    if name == 'toy_parallel_selfloop':
        assert not bool(res.islanding.any())                                     # no bridge at all
        assert bool(res.converged[:, loops + doubled].all())                     # both lines of the pair and the loop are solved
    _check_summaries_from_flows(res)


def test_full_size_case118_every_line():
    s, res = _case(118, 1)
    rows, bases = _reference(118, 1)
    E = 186
    assert int(res.islanding.sum()) == 20 and bases[0][2]
    _check_base(res, s)
    n_cmp, n_pairs = _compare(res, s, rows, list(range(E)), range(1), 'case118')
    assert n_pairs == 166 and n_cmp >= 0.6 * n_pairs, (n_cmp, n_pairs)
    _check_summaries_from_flows(res)


def test_case300_fits_and_a_larger_image_is_refused_by_name():
    """case300's Newton-Raphson image fits the 160 KiB, so it is screened (every seventh line and some bridges); a chain whose
    image does not fit is refused with Newton-Raphson's message."""
    buses, lines, gens, slack, _, _ = synth.solvable_grids(300, 1, seed=0, device=DEV)
    s = (buses, lines, gens, slack)
    f, t, _ = synth.case_topology(300)
    bridges = np.flatnonzero(powerflow._bridges(300, f - 1, t - 1))
    outages = sorted(set(range(0, 411, 7)) | set(bridges[:5].tolist()))
    res = _screen(s, outages=outages)
    b, l, g = (x.cpu().double().numpy() for x in (buses, lines, gens))
    base = aref.base_case(b[0], l[0], g[0], slack, TOL, MAX_IT)
    assert base[2]
    rows = {(0, k): aref.outage(b[0], l[0], g[0], slack, k, base[0], base[1], TOL, MAX_IT) for k in outages}
    _check_base(res, s)
    n_cmp, n_pairs = _compare(res, s, rows, outages, range(1), 'case300')
    assert n_cmp >= 0.6 * n_pairs and int(res.islanding.sum()) >= 5
    tp = pt.path(4096)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, 0, device=DEV)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.ac_contingency_screen(buses, lines, gens, slack_bus=tp.slack, outages=[0])
    assert 'nnz(L+U) + dim + 8 N' in str(e.value)
