"""Every row of the AC contingency screen (``gns_acn1_screen``, include/gns_powerflow.h "AC contingency screening") on the MI355X,
pinned without waiting for Newton-Raphson to converge: after zero steps a row is the reference start bit for bit with the reference
mismatch and flows, and after one step its update solves the reference Jacobian of the grid with the row deleted to
``pt.STEP_TOL``.  Both hold on 100 % of the non-bridge pairs (later iterates of ill-conditioned rows drift apart by O(1), which is
why ``test_ac_contingency_gpu`` can compare only the rows that converge).  Also here: the flags the caller owns, the failure rows of
the contract (a zero pivot, a non-finite mismatch, id columns that name no bus or no pattern entry), summaries on real ties, and bit
identity at the wave-edge shapes.

The calls go through ``ac_contingency_raw.screen``: ``base_theta`` is 0.3 at the slack, so the start's subtraction matters, and
``max_iter`` of 0 or 1 applies to the rows only.  Grids are ``pt.grids(tp, regime, 2, seed=11)`` in both value regimes; the shapes
put N or E at 63 / 64 / 65, N above 64, 190 lines, and 70 lines at one bus (``pt.wheel``)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow
import ac_contingency_raw as raw
import ac_contingency_reference as aref
import nr_reference as nr
import pf_topologies as pt
from test_ac_contingency_host import emulate_row, one_step_ratios, shifted_base, toy

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = np.finfo(np.float64).eps
FLOWS = ('p_from', 'q_from', 'p_to', 'q_to')
FAMILIES = ('toy', 'random40_parallel_selfloop', 'random97_parallel_selfloop', 'lattice8x8', 'complete20', 'random24_stacked_gens',
            'ring62', 'ring63', 'ring64', 'lattice16x16', 'wheel71')


def _topo(name):
    """(topology, stride of the outage list)."""
    if name == 'toy':
        return toy(), 1
    if name.startswith('ring'):
        return pt.ring_slack_without_generator(int(name[4:])), 1
    if name == 'wheel71':
        return pt.wheel(71), 1
    return pt.families()[name], 16 if name == 'lattice16x16' else 1


def _make(tp, regime, stride=1):
    buses, lines, gens, v, theta = pt.grids(tp, regime, 2, seed=11, device=DEV)
    return _setup_from(tp, buses, lines, gens, *shifted_base(tp, v, theta), stride)


def _setup_from(tp, buses, lines, gens, base_v, base_theta, stride=1):
    """What the tests of one (topology, values) share: the device inputs, their float64 host copies, the base state with
    base_theta[slack] = 0.3, the bridges, the outage list and the reference start of each grid."""
    b, l, g = (t.cpu().double().numpy() for t in (buses, lines, gens))
    assert np.all(base_theta[:, tp.slack - 1] == 0.3)
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    outages = list(range(0, tp.f.size, stride))
    starts = [nr.start(b[i], g[i], tp.slack, base_v[i], base_theta[i]) for i in range(b.shape[0])]
    return SimpleNamespace(tp=tp, buses=buses, lines=lines, gens=gens, b=b, l=l, g=g, base_v=base_v, base_theta=base_theta,
                           bridges=bridges, outages=outages, islanding=bridges[outages], starts=starts)


@functools.lru_cache(maxsize=None)
def _setup(name, regime):
    tp, stride = _topo(name)
    return _make(tp, regime, stride)


def _run(s, max_iter, tol, outages=None, islanding=None, base_converged=None, rating=None, grids=slice(None), lines=None,
         base_v=None, gens=None):
    outages = s.outages if outages is None else outages
    islanding = s.bridges[outages] if islanding is None else islanding
    base_v = s.base_v if base_v is None else base_v
    Bt = s.buses[grids].shape[0]
    base_converged = np.ones(Bt, dtype=np.uint8) if base_converged is None else base_converged
    return raw.screen(s.tp, s.buses[grids], (s.lines if lines is None else lines)[grids], (s.gens if gens is None else gens)[grids],
                      outages, base_v[grids], s.base_theta[grids], base_converged, islanding, rating, max_iter, tol)


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in raw.ROWS}


def _same(a, b):
    """Bit-identical, NaN included."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0, a), torch.where(b.isnan(), 0, b))


def _same_rows(x, y, gx=slice(None), jx=slice(None), gy=slice(None), jy=slice(None), fields=raw.ROWS):
    for k in fields:
        assert _same(getattr(x, k)[gx][:, jx], getattr(y, k)[gy][:, jy]), k


def _not_solved(res, g, j):
    for k in ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'v_min', 'v_max', 'mismatch'):
        assert bool(getattr(res, k)[g, j].isnan().all()), k
    for k in ('worst_line', 'v_min_bus', 'v_max_bus', 'iterations'):
        assert bool((getattr(res, k)[g, j] == -1).all()), k
    assert not bool(res.converged[g, j].any())


def _check_summaries(res, ok, rating=None):
    """The rules of ``test_ac_contingency_gpu._check_summaries_from_flows`` on the returned rows ``ok`` ([Bt,K] bool): the summaries
    against torch on the returned tensors (the lowest index among equals), bit for bit but for the square root."""
    s = torch.maximum(torch.hypot(res.p_from, res.q_from), torch.hypot(res.p_to, res.q_to))
    load = s if rating is None else s / (rating if rating.dim() == 1 else rating.unsqueeze(-2))
    top = load.amax(dim=-1)
    assert bool(torch.isfinite(top[ok]).all())
    bar = 1e-12 * top.clamp(min=1.0)               # the kernel's sqrt(p^2 + q^2) against hypot: a few ulp of the value
    assert bool(((res.worst_loading - top).abs() <= bar)[ok].all())
    at_line = load.gather(-1, res.worst_line.clamp(min=0).long().unsqueeze(-1)).squeeze(-1)
    assert bool(((at_line - top).abs() <= bar)[ok].all())
    N = res.v.shape[-1]
    for val, idx, ext in ((res.v_min, res.v_min_bus, res.v.amin(dim=-1)), (res.v_max, res.v_max_bus, res.v.amax(dim=-1))):
        assert torch.equal(val[ok], ext[ok])
        first = torch.where(res.v == ext.unsqueeze(-1), torch.arange(N, device=res.v.device), N).amin(dim=-1)
        assert torch.equal(idx[ok].long(), first[ok])


def _ok_mask(s, res):
    """[Bt,K] bool: the rows of a call on ``s.outages`` that are solved (no bridge)."""
    return torch.as_tensor(~s.islanding, device=res.v.device).expand(res.v.shape[0], -1)


def _flow_bar(line, vm):
    """64 EPS max(1, max_l(|Y_ff| + |Y_ft| + |Y_tf| + |Y_tt|) max|V|^2): the state is the reference's own, so only the roundings of
    the stamps and of the eight products per end differ."""
    _, _, yff, ytt, yft, ytf = aref.line_admittances(line)
    return 64 * EPS * max(1.0, float(np.max(np.abs(yff) + np.abs(yft) + np.abs(ytf) + np.abs(ytt))) * float(np.max(np.abs(vm))) ** 2)


def _mismatch_and_bar(bus, line, gen, slack, k, vm, va):
    """(||F||_inf of the reference on the grid with row k, or every row of the sequence k, deleted, 4 deg EPS scale): the bar and the
    scale of ``test_zero_steps_return_the_start_and_its_mismatch`` on the post-outage Y-bus."""
    rest = np.delete(line, k, axis=0)
    Y = nr.ybus(bus, rest)
    F = nr.mismatch_vector(bus, rest, gen, slack, vm, va, Y)
    V = vm * np.exp(1j * va)
    scale = np.max(np.abs(V) * (abs(Y) @ np.abs(V)) + np.abs(nr.specified(bus, gen)))
    deg = int(np.max(np.diff(Y.indptr))) + 2
    return float(np.max(np.abs(F))), 4 * deg * EPS * scale


def _check_flows(got, line, vm, va, k, what):
    """The four flows of one returned row against the reference at (vm, va); exactly 0 at line k (at every line of the sequence k).
    Returns the worst error / bar."""
    k = np.atleast_1d(k)
    bar = _flow_bar(line, vm)
    worst = 0.0
    for key, want in zip(FLOWS, aref.branch_flows(line, vm, va, k)):
        assert np.all(got[key][k] == 0.0), (what, key)
        err = float(np.max(np.abs(got[key] - want)))
        worst = max(worst, err / bar)
        assert err <= bar, (what, key, err, bar)
    return worst


def _check_zero_step_row(s, got, i, k, tol, what):
    """Row (grid i, line k or the pair of lines k) after zero steps: the start bit for bit, the reference mismatch, flows from the
    start."""
    vm0, va0 = s.starts[i]
    assert int(got['iterations']) == 0, what
    assert np.array_equal(got['v'], vm0) and np.array_equal(got['theta'], va0), what
    want, bar = _mismatch_and_bar(s.b[i], s.l[i], s.g[i], s.tp.slack, k, vm0, va0)
    assert abs(float(got['mismatch']) - want) <= bar, (what, float(got['mismatch']), want, bar)
    assert bool(got['converged']) == (float(got['mismatch']) < tol), what
    return _check_flows(got, s.l[i], vm0, va0, k, what)


@pytest.mark.parametrize('regime', pt.REGIMES)
@pytest.mark.parametrize('name', FAMILIES)
def test_zero_steps_every_pair(name, regime):
    s = _setup(name, regime)
    tol = 1e-8
    res = _run(s, 0, tol)
    host = _host(res)
    n_cmp, worst = 0, 0.0
    for i in range(2):
        for j, k in enumerate(s.outages):
            if s.bridges[k]:
                _not_solved(res, i, j)
                continue
            got = {key: host[key][i, j] for key in raw.ROWS}
            worst = max(worst, _check_zero_step_row(s, got, i, k, tol, (name, regime, i, k)))
            n_cmp += 1
    n_pairs = 2 * int((~s.islanding).sum())
    print(f'{name} ({regime}) zero steps: compared {n_cmp} of {n_pairs} non-bridge pairs ({100 * n_cmp // n_pairs} %), '
          f'worst flow error {worst:.2f} of its bar')
    assert n_cmp == n_pairs > 0
    _check_summaries(res, _ok_mask(s, res))


@pytest.mark.parametrize('regime', pt.REGIMES)
@pytest.mark.parametrize('name', FAMILIES)
def test_one_step_every_pair(name, regime):
    s = _setup(name, regime)
    res = _run(s, 1, 0.0)
    host = _host(res)
    n_cmp, worst, worst_flow = 0, 0.0, 0.0
    for i in range(2):
        vm0, va0 = s.starts[i]
        for j, k in enumerate(s.outages):
            if s.bridges[k]:
                _not_solved(res, i, j)
                continue
            what = (name, regime, i, k)
            got = {key: host[key][i, j] for key in raw.ROWS}
            assert int(got['iterations']) == 1 and not got['converged'], what
            assert np.isfinite(got['v']).all() and np.isfinite(got['theta']).all() and np.isfinite(got['mismatch']), what
            r_scipy, r_dev = one_step_ratios(s.b[i], s.l[i], s.g[i], s.tp.slack, k, vm0, va0, got['v'], got['theta'])
            assert r_scipy <= pt.STEP_TOL, (what, r_scipy)              # the post-outage grid is conditioned well enough ...
            assert r_dev <= pt.STEP_TOL, (what, r_dev)                  # ... so a failure here is the kernel's
            worst = max(worst, r_dev)
            worst_flow = max(worst_flow, _check_flows(got, s.l[i], got['v'], got['theta'], k, what))
            n_cmp += 1
    n_pairs = 2 * int((~s.islanding).sum())
    print(f'{name} ({regime}) one step: compared {n_cmp} of {n_pairs} non-bridge pairs ({100 * n_cmp // n_pairs} %), '
          f'worst one-step ratio {worst:.1e}, worst flow error {worst_flow:.2f} of its bar')
    assert n_cmp == n_pairs > 0
    _check_summaries(res, _ok_mask(s, res))


@pytest.mark.parametrize('name', ['toy', 'random40_parallel_selfloop', 'ring64'])
def test_flags_and_ratings_are_the_callers(name):
    s = _setup(name, 'wide')
    E = s.tp.f.size
    clean = _run(s, 1, 0.0)
    j0 = int(np.flatnonzero(~s.islanding)[E // 3 % int((~s.islanding).sum())])         # a line that is no bridge, flagged anyway
    flagged = s.islanding.copy()
    flagged[j0] = True
    res = _run(s, 1, 0.0, islanding=flagged)
    _not_solved(res, slice(None), j0)
    others = [j for j in range(len(s.outages)) if j != j0]
    _same_rows(res, clean, jx=others, jy=others)
    assert int(clean.iterations[0, j0]) == 1
    res = _run(s, 1, 0.0, base_converged=np.array([1, 0], dtype=np.uint8))
    _not_solved(res, 1, slice(None))
    _same_rows(res, clean, gx=slice(0, 1), gy=slice(0, 1))
    gen = torch.Generator().manual_seed(E)
    ok = _ok_mask(s, clean)
    for shape in ((E,), (2, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=gen, dtype=torch.float64)).to(DEV)
        rated = _run(s, 1, 0.0, rating=rating)
        _same_rows(rated, clean, fields=[k for k in raw.ROWS if k not in ('worst_loading', 'worst_line')])
        _check_summaries(rated, ok, rating)
        assert not torch.equal(rated.worst_loading[ok], clean.worst_loading[ok])
    _check_summaries(clean, ok)


def _pendant_lattice():
    """lattice8x8 with a 65th bus (PQ) hung on bus 64 by one line, the last: the only bridge."""
    tp = pt.lattice(8)
    return pt.Topo('lattice8x8_pendant', 65, np.r_[tp.f, 64], np.r_[tp.t, 65], tp.g, tp.slack)


def test_a_zero_pivot_keeps_the_start():
    """The bridge to a leaf without shunt, left unflagged: the leaf's Jacobian rows and columns are exact zeros, so the first
    factorisation meets a zero pivot.  The row has converged = 0, iterations = 0, the start bit for bit, its finite mismatch and the
    flows of the start."""
    tp = _pendant_lattice()
    buses, lines, gens, v, theta = pt.grids(tp, 'reference', 2, seed=11, device=DEV)
    buses = buses.clone()
    buses[:, 64, 4:6] = 0.0
    s = _setup_from(tp, buses, lines, gens, *shifted_base(tp, v, theta))
    k = tp.f.size - 1
    assert s.bridges.tolist() == [False] * k + [True]
    w = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host
    with np.errstate(all='ignore'), pytest.raises(AssertionError):             # the replay trips its zero-pivot assertion
        emulate_row(w, s.b[0], s.l[0], s.g[0], k, s.base_v[0], s.base_theta[0], tol=1e-8, max_iter=5)
    outages = [0, k, 57]
    res = _run(s, 5, 1e-8, outages=outages, islanding=np.zeros(3, dtype=bool))
    host = _host(res)
    for i in range(2):
        got = {key: host[key][i, 1] for key in raw.ROWS}
        assert not got['converged'] and np.isfinite(got['mismatch']) and got['mismatch'] > 1e-8
        _check_zero_step_row(s, got, i, k, 1e-8, ('zero pivot', i))
    assert bool((res.iterations[:, [0, 2]] >= 1).all())                        # its neighbours in the list iterate
    _check_summaries(res, torch.ones(2, 3, dtype=torch.bool, device=DEV))
    zero = _run(s, 0, 1e-8, outages=outages, islanding=np.zeros(3, dtype=bool))
    _same_rows(res, zero, jx=[1], jy=[1])                                     # the row after zero steps, bit for bit


def test_a_non_finite_mismatch_stops_the_rows_of_its_grid():
    s = _setup('random40_parallel_selfloop', 'reference')
    tp = s.tp
    f, t = tp.f - 1, tp.t - 1
    _, _, pq = nr.roles(s.b[0], s.g[0], tp.slack)
    bus = int(next(i for i in pq if np.sum(((f == i) | (t == i)) & (f != t)) >= 3))
    touching = (f == bus) | (t == bus)
    base_v = s.base_v.copy()
    base_v[1, bus] = np.nan
    clean = _run(s, 3, 1e-8)
    res = _run(s, 3, 1e-8, base_v=base_v)
    _same_rows(res, clean, gx=slice(0, 1), gy=slice(0, 1))
    host = _host(res)
    vm0, va0 = s.starts[1]
    n = 0
    for j, k in enumerate(s.outages):
        if s.bridges[k]:
            _not_solved(res, 1, j)
            continue
        got = {key: host[key][1, j] for key in raw.ROWS}
        assert not got['converged'] and int(got['iterations']) == 0 and np.isnan(got['mismatch']), k
        assert np.array_equal(np.isnan(got['v']), np.arange(tp.n) == bus) and np.array_equal(got['theta'], va0), k
        assert np.array_equal(np.delete(got['v'], bus), np.delete(vm0, bus)), k
        assert np.isnan(got['v_min']) and np.isnan(got['v_max']) and int(got['v_min_bus']) == int(got['v_max_bus']) == bus, k
        want_nan = touching & (np.arange(f.size) != k)
        for key in FLOWS:
            assert np.array_equal(np.isnan(got[key]), want_nan), (k, key)
            assert got[key][k] == 0.0, (k, key)
        assert np.isnan(got['worst_loading']) and int(got['worst_line']) == int(np.flatnonzero(want_nan)[0]), k
        n += 1
    assert n == int((~s.islanding).sum())


def test_id_columns_that_name_no_bus_or_no_entry():
    """The solve reads the blob's stamps, never the id columns, so only the tampered line's own flows and row change."""
    s = _setup('random40_parallel_selfloop', 'reference')
    tp = s.tp
    N, E = tp.n, tp.f.size
    pairs = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    e = next(k for k in range(E) if not s.bridges[k] and pairs[k][0] != pairs[k][1] and pairs.count(pairs[k]) == 1)
    clean = _run(s, 2, 1e-8)
    others = [k for k in range(E) if k != e]
    solved = [k for k in others if not s.bridges[k]]
    not_flow = [k for k in raw.ROWS if k not in FLOWS + ('worst_loading', 'worst_line')]
    for bad in (0.0, float(N + 1), 2.5):
        lines = s.lines.clone()
        lines[:, e, 0] = bad
        res = _run(s, 2, 1e-8, lines=lines)
        _not_solved(res, slice(None), e)
        _same_rows(res, clean, jx=others, jy=others, fields=not_flow)
        for key in FLOWS:
            assert bool(getattr(res, key)[:, solved, e].isnan().all()), (bad, key)
            assert _same(getattr(res, key)[:, others][:, :, others], getattr(clean, key)[:, others][:, :, others]), (bad, key)
        assert bool(res.worst_loading[:, solved].isnan().all()) and bool((res.worst_line[:, solved] == e).all()), bad
        for k in others:
            if s.bridges[k]:
                _not_solved(res, slice(None), k)
    # two buses of the grid that no line joins: the pattern has no such entry
    adjacent = set(pairs)
    a, b = next((a, b) for a in range(1, N + 1) for b in range(a + 1, N + 1) if (a, b) not in adjacent)
    lines = s.lines.clone()
    lines[:, e, 0], lines[:, e, 1] = float(a), float(b)
    res = _run(s, 2, 1e-8, lines=lines)
    _not_solved(res, slice(None), e)
    _same_rows(res, clean, jx=others, jy=others, fields=not_flow)
    for key in FLOWS:
        assert bool(getattr(res, key)[:, solved, e].isfinite().all()), key
        assert _same(getattr(res, key)[:, others][:, :, others], getattr(clean, key)[:, others][:, :, others]), key


def test_two_identical_parallel_lines_tie_at_the_lower_index():
    """Lines 0 (1 -> 2) and 5 (2 -> 1) of the toy with identical parameters, tau = 1 and no shift: S_from of one line is S_to of the
    other (the same two products summed in the other order; the library is built without contraction of products into sums), so
    their loadings are equal bit for bit, and a rating makes the two the worst: worst_line is the lower index.  Once with the
    perturbed voltages and once with the same voltage at both buses, where all four flows of the two lines are equal bit for bit
    whatever the evaluation order; then with the two lines listed in the other order."""
    s = _setup('toy', 'reference')
    lines = s.lines.clone()
    lines[:, [0, 5], 2:] = torch.tensor([0.01, 0.1, 0.04, 1.0, 0.0], device=DEV)       # r, x, b, tau, shift
    rating = torch.ones(7, dtype=torch.float64, device=DEV)
    rating[[0, 5]] = 1e-6
    outages = [1, 2, 3, 4, 6]
    every = torch.ones(2, 5, dtype=torch.bool, device=DEV)
    perm = [5, 1, 2, 3, 4, 0, 6]
    swapped = s.tp._replace(name='toy_swapped', f=s.tp.f[perm], t=s.tp.t[perm])
    for equal_v in (False, True):
        base_v, base_theta = s.base_v.copy(), s.base_theta.copy()
        if equal_v:
            base_v[:, 1] = s.starts[0][0][0], s.starts[1][0][0]          # bus 2 (PQ) at the slack's vg, and at its angle
            base_theta[:, 1] = base_theta[:, 0]
        for tp, ln in ((s.tp, lines), (swapped, lines[:, perm].contiguous())):
            res = raw.screen(tp, s.buses, ln, s.gens, outages, base_v, base_theta, np.ones(2), np.zeros(5), rating, 0, 1e-8)
            assert bool((res.iterations == 0).all())
            assert bool(((res.v[:, :, 0] == res.v[:, :, 1]) & (res.theta[:, :, 0] == res.theta[:, :, 1])).all()) == equal_v
            for a, b in (('p_from', 'p_to'), ('q_from', 'q_to'), ('p_to', 'p_from'), ('q_to', 'q_from')):
                assert torch.equal(getattr(res, a)[:, :, 0], getattr(res, b)[:, :, 5]), (equal_v, a)
                if equal_v:
                    assert torch.equal(getattr(res, a)[:, :, 0], getattr(res, a)[:, :, 5]), a
            load = torch.maximum(res.p_from ** 2 + res.q_from ** 2, res.p_to ** 2 + res.q_to ** 2).sqrt() / rating
            assert torch.equal(load[:, :, 0], load[:, :, 5])
            assert bool((load[:, :, 0] > 2 * load[:, :, [1, 2, 3, 4, 6]].amax(dim=-1)).all())        # the two worst, by far
            _check_summaries(res, every, rating)
            assert bool((res.worst_line == 0).all()), (equal_v, tp.name, res.worst_line)


def test_equal_voltages_tie_at_the_lowest_bus():
    """Equal float32 set points on buses 3, 67 and 70 of random97 (0-based 2 and 66 share a lane, 69 is in another) above every other
    |V|: v_max_bus is 2.  Equal base voltages at three PQ buses placed the same way, below every other |V|: v_min_bus is the first."""
    base = pt.families()['random97_parallel_selfloop']
    tp = base._replace(name='random97_tied_gens', g=np.array(sorted(set(base.g.tolist()) | {3, 67, 70}), dtype=np.int64))
    buses, lines, gens, v, theta = pt.grids(tp, 'reference', 2, seed=11, device=DEV)
    gens = gens.clone()
    tied = torch.as_tensor(np.isin(tp.g, [3, 67, 70]), device=DEV)
    gens[:, tied, 4] = 1.25
    s = _setup_from(tp, buses, lines, gens, *shifted_base(tp, v, theta))
    _, pv, pq = nr.roles(s.b[0], s.g[0], tp.slack)
    assert {2, 66, 69} <= set(pv.tolist()) | {tp.slack - 1}
    a = int(next(i for i in pq if i + 64 in pq))
    c = int(max(i for i in pq if i % 64 != a % 64))
    assert a < c and a < a + 64 < tp.n
    base_v = s.base_v.copy()
    base_v[:, [a, a + 64, c]] = 0.5
    outages = [int(k) for k in np.flatnonzero(~s.bridges)[:6]]
    res = _run(s, 0, 1e-8, outages=outages, base_v=base_v)
    assert bool((res.v_max == float(np.float32(1.25))).all()) and bool((res.v_max_bus == 2).all()), res.v_max_bus
    assert bool((res.v_min == 0.5).all()) and bool((res.v_min_bus == a).all()), (a, res.v_min_bus)
    for i in (2, 66, 69):
        assert bool((res.v[:, :, i] == res.v_max).all())
    for i in (a, a + 64, c):
        assert bool((res.v[:, :, i] == 0.5).all())
    _check_summaries(res, torch.ones(2, 6, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize('name', ['ring64', 'wheel71'])
def test_rows_are_bit_identical_at_the_wave_edges(name, monkeypatch):
    s = _setup(name, 'wide')
    E = s.tp.f.size
    full = _run(s, 1, 0.0)
    assert bool((full.iterations == 1).all())
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(E)).tolist()
    _same_rows(_run(s, 1, 0.0, outages=perm), full, jy=perm)
    dup = [E - 1, 3, E - 1, 64, 0, 63, E - 1, 64]
    _same_rows(_run(s, 1, 0.0, outages=dup), full, jy=dup)
    _same_rows(_run(s, 1, 0.0, grids=slice(1, 2)), full, gy=slice(1, 2))
    _same_rows(_run(s, 1, 0.0, outages=[E - 1], grids=slice(1, 2)), full, gy=slice(1, 2), jy=[E - 1])
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', True)                      # nothing is read that nothing wrote
    _same_rows(_run(s, 1, 0.0), full)
    _same_rows(_run(s, 1, 0.0, outages=dup, grids=slice(1, 2)), full, gy=slice(1, 2), jy=dup)
