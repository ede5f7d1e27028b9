"""The AC N-2 contingency screen on the MI355X (``powerflow.ac_n2_contingency_screen``, include/gns_powerflow.h "AC N-2 contingency
screening"): every (grid, pair) row against the float64 reference (``ac_n2_reference``: both line rows deleted, the reference
Newton-Raphson warm-started from the reference's own base solution, the flows from the dense makeYbus quantities), against the
product's other route (``newton_raphson(mixed_topologies=True)`` on the expanded batch, one analysis per pair), bit identity of
rows, failure rows, ratings, and the pairs whose eight Y-bus entries overlap: lines that share a bus, parallel lines, a line from a
bus to itself.

Bars (those of test_ac_contingency_gpu): where the reference converges with at least two iterations to spare the device row has
converged with the same iteration count, ``v`` and ``theta`` within 1e-9 absolute, flows and summaries within 1e-8; the index
outputs are equal wherever the reference's runner-up is more than 1e-6 away; ``mismatch < tol`` and the reference's own mismatch of
the device state on the grid without both rows below 1e-7.  Rows the reference leaves unconverged (overloaded post-outage grids) are
left out of the value comparison only.  How many rows the reference delivers is stated with each test, counted on the CPU with the
reference alone; a cap is at or under that count."""
import functools

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import ac_contingency_reference as aref
import ac_n2_reference as n2ref
from ac_n2_pairs import every_pair, pair_kinds
import nr_reference as nr
import pf_topologies as pt
from test_ac_contingency_gpu import MAX_IT, ROWS, TOL, _check_base, _check_summaries_from_flows, _not_solved
from test_ac_contingency_host import toy
from test_powerflow_mixed_gpu import _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SUMMARIES = ROWS[6:]


def _screen(s, **kw):
    return powerflow.ac_n2_contingency_screen(s[0], s[1], s[2], slack_bus=s[3], **kw)


def _full(s, **kw):
    return _screen(s, flows=True, states=True, **kw)


def reference_rows(s, pairs, grids):
    """({(grid, j, k): Row or None}, the reference's base solutions) of the given pairs (j < k) of the given grids."""
    b, l, g = (t.cpu().double().numpy() for t in s[:3])
    rows, bases = {}, {}
    for i in grids:
        bases[i] = aref.base_case(b[i], l[i], g[i], s[3], TOL, MAX_IT)
        for j, k in pairs:
            rows[i, j, k] = n2ref.pair(b[i], l[i], g[i], s[3], j, k, bases[i][0], bases[i][1], TOL, MAX_IT)
    return rows, bases


@functools.lru_cache(maxsize=None)
def _grids14(device=DEV):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 3, seed=0, device=device)
    return buses, lines, gens, slack


@functools.lru_cache(maxsize=None)
def _case14():
    """case14 x 3 grids on the device and the screen of every pair with states and flows: made once, never changed."""
    s = _grids14()
    return s, _full(s)


@functools.lru_cache(maxsize=None)
def _reference14():
    """Every pair of every grid of ``_case14``: computed once."""
    return reference_rows(_grids14(), every_pair(20), range(3))


def _compare(res, s, rows, pairs, grids, name, rating=None):
    """Rows ``res[i, p]`` of grid ``grids[i]`` and pair ``pairs[p]`` (either order) against the reference rows; returns (compared,
    non-islanding, the compared (grid, j, k))."""
    buses, lines, gens, slack = s
    b, l, g = (t.cpu().double().numpy() for t in (buses, lines, gens))
    host = {k: getattr(res, k).cpu().numpy() for k in ROWS}
    isl = res.islanding.cpu().numpy()
    n_pairs, compared = 0, []
    worst = dict(v=0.0, theta=0.0, flow=0.0, summary=0.0)
    for i, gi in enumerate(grids):
        rt = None if rating is None else (rating if rating.dim() == 1 else rating[i]).cpu().numpy()
        for p, (j, k) in enumerate(pairs):
            want = rows[gi, min(j, k), max(j, k)]
            assert (want is None) == bool(isl[p]), (name, gi, j, k)
            if want is None:
                _not_solved(res, i, p)
                continue
            n_pairs += 1
            got = {key: host[key][i, p] for key in ROWS}
            print(f"{name} grid {gi} pair ({j}, {k}): reference converged {want.converged} in {want.iterations}, device "
                  f"{bool(got['converged'])} in {int(got['iterations'])}, mismatch {float(got['mismatch']):.2e}")
            assert np.isfinite(got['v']).all() and np.isfinite(got['theta']).all(), (name, gi, j, k)
            for key in ('p_from', 'q_from', 'p_to', 'q_to'):
                assert got[key][j] == 0.0 and got[key][k] == 0.0, (name, gi, j, k, key)
            if got['converged']:
                assert got['mismatch'] < TOL, (name, gi, j, k)
                rest = np.delete(l[gi], [j, k], axis=0)
                assert nr.mismatch(b[gi], rest, g[gi], slack, got['v'], got['theta']) < 1e-7, (name, gi, j, k)
            if not n2ref.spare(want, MAX_IT):
                continue
            compared.append((gi, min(j, k), max(j, k)))
            assert got['converged'] and int(got['iterations']) == want.iterations, (name, gi, j, k, int(got['iterations']), want.iterations)
            ev, et = np.max(np.abs(got['v'] - want.v)), np.max(np.abs(got['theta'] - want.theta))
            ef = max(np.max(np.abs(got[key] - getattr(want, key))) for key in ('p_from', 'q_from', 'p_to', 'q_to'))
            wl, wi, wgap = aref.extreme(aref.loading(want, rt))
            lo, lo_i, lo_gap = aref.extreme(want.v, largest=False)
            hi, hi_i, hi_gap = aref.extreme(want.v)
            es = max(abs(got['worst_loading'] - wl), abs(got['v_min'] - lo), abs(got['v_max'] - hi))
            worst = dict(v=max(worst['v'], ev), theta=max(worst['theta'], et), flow=max(worst['flow'], ef), summary=max(worst['summary'], es))
            assert ev <= 1e-9 and et <= 1e-9, (name, gi, j, k, ev, et)
            assert ef <= 1e-8 and es <= 1e-8, (name, gi, j, k, ef, es)
            if wgap > 1e-6:
                assert int(got['worst_line']) == wi, (name, gi, j, k)
            if lo_gap > 1e-6:
                assert int(got['v_min_bus']) == lo_i, (name, gi, j, k)
            if hi_gap > 1e-6:
                assert int(got['v_max_bus']) == hi_i, (name, gi, j, k)
    print(f'{name}: compared {len(compared)} of {n_pairs} non-islanding rows; worst errors {worst}')
    return len(compared), n_pairs, compared


def test_case14_every_pair_against_the_reference():
    """570 rows: 81 islanding (27 per grid), 489 not; the reference alone converges 329 of the 489 with two iterations to spare
    (67 %, counted on the CPU), so at least 60 % of the 489 must be compared."""
    s, res = _case14()
    E, N, P = 20, 14, 190
    rows, bases = _reference14()
    assert res.pairs.tolist() == [list(p) for p in every_pair(E)] and res.pairs.dtype == torch.int64 and res.pairs.shape == (P, 2)
    assert res.v.shape == res.theta.shape == (3, P, N) and res.p_from.shape == res.q_to.shape == (3, P, E)
    for k in SUMMARIES:
        assert getattr(res, k).shape == (3, P), k
    assert res.v.dtype == res.q_from.dtype == res.worst_loading.dtype == res.v_min.dtype == res.mismatch.dtype == torch.float64
    assert res.worst_line.dtype == res.v_min_bus.dtype == res.v_max_bus.dtype == res.iterations.dtype == torch.int32
    assert res.converged.dtype == res.islanding.dtype == torch.bool and res.islanding.shape == (P,)
    assert int(res.islanding.sum()) == 27
    _check_base(res, s)
    assert bool(res.base.converged.all())
    for i, base in bases.items():                        # the reference's own base solution is the device's to the bar
        assert base[2] and np.max(np.abs(res.base.v[i].cpu().numpy() - base[0])) <= 1e-9
    n_cmp, n_pairs, _ = _compare(res, s, rows, every_pair(E), range(3), 'case14')
    assert n_pairs == 489 and n_cmp >= 0.6 * 489, (n_cmp, n_pairs)
    _check_summaries_from_flows(res)
    slim = _screen(s)                                    # the defaults: the summaries alone
    assert all(getattr(slim, k) is None for k in ROWS[:6])


def test_rows_are_bit_identical_in_any_list_order_batch_and_option(monkeypatch):
    s, full = _case14()
    buses, lines, gens, slack = s
    every = every_pair(20)
    P = len(every)

    def same_rows(part, grids, cols, fields=ROWS):
        for k in fields:
            assert _same(getattr(part, k), getattr(full, k)[grids][:, cols]), k

    again = _full(s)                                                                 # from run to run
    same_rows(again, slice(None), list(range(P)))
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(1)).tolist()
    p = _full(s, pairs=torch.tensor([every[i] for i in perm], device=DEV))            # a permuted list, as a device tensor
    same_rows(p, slice(None), perm)
    assert torch.equal(p.islanding, full.islanding[perm]) and p.pairs.tolist() == [list(every[i]) for i in perm]
    p = _full(s, pairs=[(k, j) for j, k in every])                                    # (k, j) is (j, k)
    same_rows(p, slice(None), list(range(P)))
    assert p.pairs.tolist() == [[k, j] for j, k in every] and torch.equal(p.islanding, full.islanding)
    dup = [77, 3, 77, 189, 0, 77]                                                    # duplicates are independent rows
    p = _full(s, pairs=[every[i] for i in dup])
    same_rows(p, slice(None), dup)
    p = _full(s, pairs=[every[111]])                                                 # one pair
    same_rows(p, slice(None), [111])
    p = _full((buses[1:2], lines[1:2], gens[1:2], slack))                            # one grid
    same_rows(p, slice(1, 2), list(range(P)))
    single = powerflow.ac_n2_contingency_screen(buses[2], lines[2], gens[2], slack_bus=slack, pairs=[every[4], every[170]],
                                                flows=True, states=True)             # 2-D
    assert single.v.shape == (2, 14) and single.worst_loading.shape == (2,) and single.base.v.shape == (14,)
    assert single.p_from.shape == (2, 20) and single.islanding.shape == (2,) and single.pairs.shape == (2, 2)
    for k in ROWS:
        assert _same(getattr(single, k), getattr(full, k)[2][[4, 170]]), k
    slim = _screen(s, states=True)
    assert slim.p_from is None and slim.q_from is None and slim.p_to is None and slim.q_to is None
    same_rows(slim, slice(None), list(range(P)), [k for k in ROWS if k[:2] not in ('p_', 'q_')])
    slim = _screen(s, flows=True)
    assert slim.v is None and slim.theta is None
    same_rows(slim, slice(None), list(range(P)), [k for k in ROWS if k not in ('v', 'theta')])
    slim = _screen(s, pairs=[every[i] for i in dup])                                 # the defaults
    assert all(getattr(slim, k) is None for k in ROWS[:6])
    same_rows(slim, slice(None), dup, SUMMARIES)
    cpu = powerflow.ac_n2_contingency_screen(buses.cpu(), lines.cpu(), gens.cpu(), slack_bus=slack, pairs=[every[1], every[2]],
                                             flows=True, states=True)
    assert all(t.device.type == 'cpu' for t in (cpu.v, cpu.p_from, cpu.worst_line, cpu.converged, cpu.islanding, cpu.pairs, cpu.base.v))
    for k in ROWS:
        assert _same(getattr(cpu, k), getattr(full, k)[:, [1, 2]].cpu()), k
    req = [t.clone().requires_grad_(True) for t in (buses, lines, gens)]             # not differentiable, and no error
    r = powerflow.ac_n2_contingency_screen(*req, slack_bus=slack, pairs=[every[0]], flows=True, states=True)
    assert not any(t.requires_grad for t in (r.v, r.theta, r.p_from, r.q_to, r.worst_loading, r.v_min, r.v_max, r.mismatch, r.base.v,
                                             r.base.theta))
    same_rows(r, slice(None), [0])
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', True)                          # nothing is read that nothing wrote
    poisoned = _full(s)
    same_rows(poisoned, slice(None), list(range(P)))


def test_agrees_with_the_expanded_route():
    """The other route: each (grid, pair) as a grid of its own with both line rows deleted, one analysis per pair,
    ``newton_raphson(mixed_topologies=True)`` warm-started from the base, on a seeded sample of 40 pairs."""
    s, res = _case14()
    buses, lines, gens, slack = s
    E, S = 20, 40
    every = every_pair(E)
    pick = np.sort(np.random.default_rng(14).choice(len(every), S, replace=False))
    keep = torch.tensor([[e for e in range(E) if e not in every[p]] for p in pick], device=DEV)        # [S, E-2]
    xl = lines[:, keep].reshape(3 * S, E - 2, 7).contiguous()
    xb, xg = buses.repeat_interleave(S, dim=0), gens.repeat_interleave(S, dim=0)
    v0, th0 = res.base.v.repeat_interleave(S, dim=0), res.base.theta.repeat_interleave(S, dim=0)
    mixed = powerflow.newton_raphson(xb, xl, xg, slack_bus=slack, mixed_topologies=True, v0=v0, theta0=th0, tol=TOL, max_iter=MAX_IT)
    cols = torch.from_numpy(pick).to(DEV)
    conv = mixed.converged.reshape(3, S)
    assert torch.equal(conv, res.converged[:, cols])
    assert torch.equal((mixed.iterations == -1).reshape(3, S), res.islanding[cols].expand(3, S))
    assert 0 < int(res.islanding[cols].sum()) < S and int(conv.sum()) > 0
    dv = (mixed.v.reshape(3, S, -1) - res.v[:, cols]).abs().amax(dim=-1)[conv]
    dth = (mixed.theta.reshape(3, S, -1) - res.theta[:, cols]).abs().amax(dim=-1)[conv]
    print(f'expanded route: {int(conv.sum())} converged rows of {3 * S}, max |dv| {float(dv.max()):.2e}, max |dtheta| {float(dth.max()):.2e}')
    assert float(dv.max()) <= 1e-9 and float(dth.max()) <= 1e-9


# (rows the reference alone converges with two iterations to spare, non-islanding rows) of two grids and every pair, counted on the
# CPU with the reference alone: 80 % and 70 %.  The tests ask for 60 % of the non-islanding rows, the cap of the N-1 tests.
FAMILY_SHARE = {'toy_parallel_selfloop': (24, 30), 'random40_parallel_selfloop': (2158, 3062)}


@pytest.mark.parametrize('name', ['toy_parallel_selfloop', 'random40_parallel_selfloop'])
def test_pairs_whose_entries_overlap(name):
    """Parallel lines (all four entries shared, zeros inside the pattern when no third line joins the two buses), lines that share a
    bus (its diagonal entry twice in the set), the line from a bus to itself (one entry four times) with a line at its bus and with
    a line elsewhere: each kind is in the list and among the rows compared with the reference.  One exception, found by the graph
    search: random40's self-loop sits at a bus whose only other line is a bridge, so its pair with that line islands; that kind is
    solved on the toy grid.  (random40's 3 906 reference solves are the slow part: 23 s of CPU time on the MI355X's host.)"""
    tp = toy() if name == 'toy_parallel_selfloop' else pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, lines, gens, tp.slack)
    every = every_pair(tp.f.size)
    res = _full(s)
    rows, bases = reference_rows(s, every, range(2))
    assert all(base[2] for base in bases.values())
    _check_base(res, s)
    n_cmp, n_pairs, compared = _compare(res, s, rows, every, range(2), name)       # the islanding mask against the graph search too
    ref_share, ref_pairs = FAMILY_SHARE[name]
    assert 0.6 * ref_pairs <= ref_share
    assert n_pairs == ref_pairs and n_cmp >= 0.6 * ref_pairs, (n_cmp, n_pairs)
    kinds = pair_kinds(tp)
    solved = {}
    for _, j, k in compared:
        if (j, k) in kinds:
            solved[kinds[j, k]] = solved.get(kinds[j, k], 0) + 1
    print(f'{name}: kinds in the list {sorted(set(kinds.values()))}, compared rows per kind {solved}')
    for kind in ('parallel', 'shared_bus', 'loop_at_bus', 'loop_elsewhere'):
        assert kind in kinds.values(), (name, kind)
        if (name, kind) == ('random40_parallel_selfloop', 'loop_at_bus'):
            assert all(rows[0, j, k] is None for (j, k), kd in kinds.items() if kd == kind)       # islanding, by the graph search
        else:
            assert solved.get(kind, 0) > 0, (name, kind)
    if name == 'toy_parallel_selfloop':
        assert not bool(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1).any())           # no bridge: a pair islands only as a pair
        assert 0 < int(res.islanding.sum()) < len(every)
    _check_summaries_from_flows(res)


def test_a_grid_without_a_base_solution_fails_alone_and_ratings():
    s, good = _case14()
    buses, lines, gens, slack = s
    E = 20
    every = every_pair(E)
    bad = buses.clone()
    bad[1, :, 2:4] *= 40.0                                                       # loads no network of this size can serve
    res = _full((bad, lines, gens, slack))
    assert res.base.converged.tolist() == [True, False, True]
    _not_solved(res, 1, slice(None))
    for k in ROWS:
        assert _same(getattr(res, k)[[0, 2]], getattr(good, k)[[0, 2]]), k
    assert torch.equal(res.islanding, good.islanding)
    rows, _ = _reference14()
    g = torch.Generator().manual_seed(E)
    for shape in ((E,), (3, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=g, dtype=torch.float64)).to(DEV)
        rated = _full(s, rating=rating)
        for k in ROWS:
            if k not in ('worst_loading', 'worst_line'):
                assert _same(getattr(rated, k), getattr(good, k)), k
        _check_summaries_from_flows(rated, rating)
        n_cmp, n_pairs, _ = _compare(rated, s, rows, every, range(3), f'case14 rating {shape}', rating=rating)
        assert n_pairs == 489 and n_cmp >= 0.6 * 489
        slim = _screen(s, rating=rating)
        assert _same(slim.worst_loading, rated.worst_loading) and torch.equal(slim.worst_line, rated.worst_line)
    r32 = _screen(s, rating=torch.ones(E, dtype=torch.float32))                  # converted to float64
    assert _same(r32.worst_loading, good.worst_loading) and torch.equal(r32.worst_line, good.worst_line)


def chosen_pairs(s, n_spare, n_other, n_islanding, seed):
    """The list of a large case, from the reference alone: a seeded shuffle of every pair of grid 0, walked until it has given the
    first ``n_spare`` non-islanding pairs the reference converges with two iterations to spare, the first ``n_other`` non-islanding
    pairs it does not, and the first ``n_islanding`` islanding pairs.  Returns (pairs, {(0, j, k): Row or None}, the three lists)."""
    b, l, g = (t[0].cpu().double().numpy() for t in s[:3])
    every = every_pair(l.shape[0])
    base = aref.base_case(b, l, g, s[3], TOL, MAX_IT)
    assert base[2]
    spare, other, island, rows = [], [], [], {}
    for p in np.random.default_rng(seed).permutation(len(every)):
        j, k = every[p]
        if n2ref.pair_islands(b.shape[0], l, s[3], j, k):
            if len(island) < n_islanding:
                island.append((j, k))
                rows[0, j, k] = None
        elif len(spare) < n_spare or len(other) < n_other:
            row = n2ref.pair(b, l, g, s[3], j, k, base[0], base[1], TOL, MAX_IT)
            into = spare if n2ref.spare(row, MAX_IT) else other
            if len(into) < (n_spare if into is spare else n_other):
                into.append((j, k))
                rows[0, j, k] = row
        if len(spare) == n_spare and len(other) == n_other and len(island) == n_islanding:
            break
    assert len(spare) == n_spare and len(other) == n_other and len(island) == n_islanding
    return spare + other + island, rows, (spare, other, island)


def _check_chosen(name, s, n_spare, n_other, n_islanding, seed):
    pairs, rows, (spare, other, island) = chosen_pairs(s, n_spare, n_other, n_islanding, seed)
    res = _full(s, pairs=pairs)
    _check_base(res, s)
    n_cmp, n_pairs, _ = _compare(res, s, rows, pairs, range(1), name)           # islanding rows: NaN / -1; the others: finite,
    assert n_cmp == n_spare and n_pairs == n_spare + n_other                    # converged consistently; every spare row compared
    assert res.islanding.tolist() == [False] * (n_spare + n_other) + [True] * n_islanding
    _check_summaries_from_flows(res)
    slim = _screen(s, pairs=pairs)
    for k in SUMMARIES:
        assert _same(getattr(slim, k), getattr(res, k)), k


def test_full_size_case118_pairs_chosen_by_the_reference():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(118, 1, seed=0, device=DEV)
    _check_chosen('case118', (buses, lines, gens, slack), 48, 8, 8, seed=118)


def test_case300_fits_and_a_larger_image_is_refused_by_name():
    """case300's Newton-Raphson image fits the 160 KiB, so its pairs are screened (a dozen, chosen as case118's); a chain whose image
    does not fit is refused with Newton-Raphson's message."""
    buses, lines, gens, slack, _, _ = synth.solvable_grids(300, 1, seed=0, device=DEV)
    _check_chosen('case300', (buses, lines, gens, slack), 8, 2, 2, seed=300)
    tp = pt.path(4096)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, 0, device=DEV)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.ac_n2_contingency_screen(buses, lines, gens, slack_bus=tp.slack, pairs=[[0, 1]])
    assert 'nnz(L+U) + dim + 8 N' in str(e.value)
