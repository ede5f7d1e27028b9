"""Every listed row of the AC N-2 contingency screen (``gns_acn2_screen``, include/gns_powerflow.h "AC N-2 contingency screening")
on the MI355X, pinned without waiting for Newton-Raphson to converge, as ``test_ac_contingency_rows_gpu`` pins the single outages:
after zero steps a row is the reference start bit for bit with the reference mismatch and flows of the grid without both lines, and
after one step its update solves the reference Jacobian of that grid to ``pt.STEP_TOL``.  Both hold on 100 % of the non-islanding
pairs of a list, where ``test_ac_n2_gpu`` can compare only the rows the reference converges (about two thirds).  What is the N-2
kernel's own is its prologue (the order of the pair, whether the row is solved, eight CSR positions, the eight-entry Y-bus view
every later read goes through): a wrong or missed entry moves the zero-step mismatch by the size of a stamp, orders above its bar.
Also here: the flags the caller owns, the failure rows of the contract (a zero pivot, a non-finite mismatch, id columns that name no
bus or no pattern entry, each refusal met twice per row), a real tie of loadings, and bit identity at the wave-edge shapes.

The calls go through ``ac_contingency_raw.screen_pairs``: ``base_theta`` is 0.3 at the slack and ``max_iter`` of 0 or 1 applies to
the rows only.  Grids are ``pt.grids(tp, regime, 2, seed=11)`` in both value regimes on the topologies of the N-1 file; the pairs are
``ac_n2_pairs.rows_pairs`` (at most 128: the first pair of each overlap kind, every pair among lines 0, 62, 63, 64, 65 and
E - 1, a seeded fill), the islanding mask the reference's graph search.  The reference's own one-step guard (scipy's step within
``pt.STEP_TOL``) was run on the CPU on every non-islanding row of these lists: worst 2.2e-16, no pair had to be replaced.  The bars
are those of the N-1 file: ``_mismatch_and_bar``, ``_flow_bar``, ``pt.STEP_TOL``."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow
import ac_contingency_raw as raw
from ac_n2_pairs import pair_kinds, rows_islanding, rows_pairs
import nr_reference as nr
import pf_topologies as pt
from test_ac_contingency_host import emulate_row, one_step_ratios, shifted_base
from test_ac_contingency_rows_gpu import (DEV, FAMILIES, FLOWS, _check_flows, _check_summaries, _check_zero_step_row, _host,
                                          _not_solved, _ok_mask, _same, _same_rows, _topo)

pytestmark = pytest.mark.gpu
# non-islanding rows of the two grids of each list, counted on the CPU with the reference alone (the same in both regimes)
N_ROWS = {'toy': 30, 'random40_parallel_selfloop': 188, 'random97_parallel_selfloop': 178, 'lattice8x8': 254, 'complete20': 256,
          'random24_stacked_gens': 196, 'ring62': 130, 'ring63': 128, 'ring64': 150, 'lattice16x16': 254, 'wheel71': 256}
# the overlap kinds that must be among the compared rows; random40's line from a bus to itself sits at a bus whose only other line
# is a bridge, so that kind islands there (test_ac_n2_gpu.test_pairs_whose_entries_overlap) and is solved on the toy grid
KINDS_COMPARED = {'toy': {'parallel', 'shared_bus', 'loop_at_bus', 'loop_elsewhere'},
                  'random40_parallel_selfloop': {'parallel', 'shared_bus', 'loop_elsewhere'}}


def _setup_from(tp, buses, lines, gens, base_v, base_theta, pairs=None):
    """What the tests of one (topology, values) share: the device inputs, their float64 host copies, the base state with
    base_theta[slack] = 0.3, the pair list with its islanding mask and the reference start of each grid."""
    b, l, g = (t.cpu().double().numpy() for t in (buses, lines, gens))
    assert np.all(base_theta[:, tp.slack - 1] == 0.3)
    pairs = rows_pairs(tp) if pairs is None else pairs
    starts = [nr.start(b[i], g[i], tp.slack, base_v[i], base_theta[i]) for i in range(b.shape[0])]
    return SimpleNamespace(tp=tp, buses=buses, lines=lines, gens=gens, b=b, l=l, g=g, base_v=base_v, base_theta=base_theta,
                           pairs=pairs, islanding=rows_islanding(tp, pairs), starts=starts)


@functools.lru_cache(maxsize=None)
def _setup(name, regime):
    tp = _topo(name)[0]
    buses, lines, gens, v, theta = pt.grids(tp, regime, 2, seed=11, device=DEV)
    return _setup_from(tp, buses, lines, gens, *shifted_base(tp, v, theta))


def _run(s, max_iter, tol, pairs=None, islanding=None, base_converged=None, rating=None, grids=slice(None), lines=None, base_v=None):
    """``s.pairs`` (or ``pairs`` with their ``islanding``) of the grids ``grids`` of ``s``."""
    assert pairs is None or islanding is not None
    pairs = s.pairs if pairs is None else pairs
    islanding = s.islanding if islanding is None else islanding
    base_v = s.base_v if base_v is None else base_v
    Bt = s.buses[grids].shape[0]
    base_converged = np.ones(Bt, dtype=np.uint8) if base_converged is None else base_converged
    return raw.screen_pairs(s.tp, s.buses[grids], (s.lines if lines is None else lines)[grids], s.gens[grids], pairs, base_v[grids],
                            s.base_theta[grids], base_converged, islanding, rating, max_iter, tol)


def _kinds_compared(name, s):
    """The overlap kinds among the non-islanding pairs of the list: with every such row compared, the kinds that were compared."""
    kinds = pair_kinds(s.tp)
    seen = {}
    for p, island in zip(s.pairs, s.islanding):
        if not island and p in kinds:
            seen[kinds[p]] = seen.get(kinds[p], 0) + 1
    assert KINDS_COMPARED.get(name, set()) <= set(seen), (name, seen)
    return seen


@pytest.mark.parametrize('regime', pt.REGIMES)
@pytest.mark.parametrize('name', FAMILIES)
def test_zero_steps_every_listed_pair(name, regime):
    """Non-islanding rows compared, of two grids (all of them, in either regime): toy 30 of 42 rows, random40 188, random97 178,
    lattice8x8 254, complete20 256, random24_stacked_gens 196, ring62 130, ring63 128, ring64 150, lattice16x16 254, wheel71 256 of
    256 rows each."""
    s = _setup(name, regime)
    tol = 1e-8
    res = _run(s, 0, tol)
    host = _host(res)
    n_cmp, worst = 0, 0.0
    for i in range(2):
        for p, (j, k) in enumerate(s.pairs):
            if s.islanding[p]:
                _not_solved(res, i, p)
                continue
            got = {key: host[key][i, p] for key in raw.ROWS}
            worst = max(worst, _check_zero_step_row(s, got, i, [j, k], tol, (name, regime, i, j, k)))
            n_cmp += 1
    n_rows = 2 * int((~s.islanding).sum())
    print(f'{name} ({regime}) zero steps: compared {n_cmp} of {n_rows} non-islanding rows ({100 * n_cmp // n_rows} %), '
          f'worst flow error {worst:.2f} of its bar, kinds compared {_kinds_compared(name, s)}')
    assert n_cmp == n_rows == N_ROWS[name] > 0
    _check_summaries(res, _ok_mask(s, res))


@pytest.mark.parametrize('regime', pt.REGIMES)
@pytest.mark.parametrize('name', FAMILIES)
def test_one_step_every_listed_pair(name, regime):
    """The rows of ``test_zero_steps_every_listed_pair`` after one Newton step.  Non-islanding rows compared, of two grids (all of
    them, in either regime): toy 30 of 42 rows, random40 188, random97 178, lattice8x8 254, complete20 256, random24_stacked_gens
    196, ring62 130, ring63 128, ring64 150, lattice16x16 254, wheel71 256 of 256 rows each."""
    s = _setup(name, regime)
    res = _run(s, 1, 0.0)
    host = _host(res)
    n_cmp, worst, worst_flow = 0, 0.0, 0.0
    for i in range(2):
        vm0, va0 = s.starts[i]
        for p, (j, k) in enumerate(s.pairs):
            if s.islanding[p]:
                _not_solved(res, i, p)
                continue
            what = (name, regime, i, j, k)
            got = {key: host[key][i, p] for key in raw.ROWS}
            assert int(got['iterations']) == 1 and not got['converged'], what
            assert np.isfinite(got['v']).all() and np.isfinite(got['theta']).all() and np.isfinite(got['mismatch']), what
            r_scipy, r_dev = one_step_ratios(s.b[i], s.l[i], s.g[i], s.tp.slack, [j, k], vm0, va0, got['v'], got['theta'])
            assert r_scipy <= pt.STEP_TOL, (what, r_scipy)              # the grid without both lines is conditioned well enough ...
            assert r_dev <= pt.STEP_TOL, (what, r_dev)                  # ... so a failure here is the kernel's
            worst = max(worst, r_dev)
            worst_flow = max(worst_flow, _check_flows(got, s.l[i], got['v'], got['theta'], [j, k], what))
            n_cmp += 1
    n_rows = 2 * int((~s.islanding).sum())
    print(f'{name} ({regime}) one step: compared {n_cmp} of {n_rows} non-islanding rows ({100 * n_cmp // n_rows} %), '
          f'worst one-step ratio {worst:.1e}, worst flow error {worst_flow:.2f} of its bar, kinds compared {_kinds_compared(name, s)}')
    assert n_cmp == n_rows == N_ROWS[name] > 0
    _check_summaries(res, _ok_mask(s, res))


@pytest.mark.parametrize('name', ['toy', 'random40_parallel_selfloop', 'ring64'])
def test_flags_and_ratings_are_the_callers(name):
    s = _setup(name, 'wide')
    E, P = s.tp.f.size, len(s.pairs)
    clean = _run(s, 1, 0.0)
    solved = np.flatnonzero(~s.islanding)
    p0 = int(solved[E // 3 % solved.size])                                     # a pair that does not island, flagged anyway
    flagged = s.islanding.copy()
    flagged[p0] = True
    res = _run(s, 1, 0.0, pairs=s.pairs, islanding=flagged)
    _not_solved(res, slice(None), p0)
    others = [p for p in range(P) if p != p0]
    _same_rows(res, clean, jx=others, jy=others)
    assert int(clean.iterations[0, p0]) == 1
    res = _run(s, 1, 0.0, base_converged=np.array([1, 0], dtype=np.uint8))
    _not_solved(res, 1, slice(None))
    _same_rows(res, clean, gx=slice(0, 1), gy=slice(0, 1))
    gen = torch.Generator().manual_seed(E)
    ok = _ok_mask(s, clean)
    for shape in ((E,), (2, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=gen, dtype=torch.float64)).to(DEV)
        rated = _run(s, 1, 0.0, rating=rating)
        _same_rows(rated, clean, fields=[k for k in raw.ROWS if k not in ('worst_loading', 'worst_line')])
        _check_summaries(rated, ok, rating)                                   # against the returned flows
        assert not torch.equal(rated.worst_loading[ok], clean.worst_loading[ok])
    _check_summaries(clean, ok)


def test_a_zero_pivot_keeps_the_start():
    """Lines 2 (3 -> 4) and 3 (4 -> 5) of the toy are the two lines of PQ bus 4.  With the bus's shunt zeroed and the pair left
    unflagged, the bus's Jacobian rows and columns are exact zeros (its three Y-bus entries are among the pair's eight and have no
    stamp left), so the first factorisation meets a zero pivot: the contract's data path for a singular Jacobian.  The row has
    converged = 0, iterations = 0, the start bit for bit, its finite mismatch and the flows of the start."""
    tp = _topo('toy')[0]
    assert (tp.f[2], tp.t[2], tp.f[3], tp.t[3]) == (3, 4, 4, 5) and 4 not in tp.g and tp.slack != 4
    assert sorted(np.flatnonzero((tp.f == 4) | (tp.t == 4)).tolist()) == [2, 3]
    buses, lines, gens, v, theta = pt.grids(tp, 'reference', 2, seed=11, device=DEV)
    buses = buses.clone()
    buses[:, 3, 4:6] = 0.0
    s = _setup_from(tp, buses, lines, gens, *shifted_base(tp, v, theta))
    at = s.pairs.index((2, 3))
    assert s.islanding[at]                                                     # it islands bus 4, and the caller does not say so
    w = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host
    with np.errstate(all='ignore'), pytest.raises(AssertionError):             # the replay trips its zero-pivot assertion
        emulate_row(w, s.b[0], s.l[0], s.g[0], [2, 3], s.base_v[0], s.base_theta[0], tol=1e-8, max_iter=5)
    near = [int(p) for p in np.flatnonzero(~s.islanding)[:2]]
    pairs = [s.pairs[near[0]], (2, 3), s.pairs[near[1]]]
    res = _run(s, 5, 1e-8, pairs=pairs, islanding=np.zeros(3, dtype=bool))
    host = _host(res)
    for i in range(2):
        got = {key: host[key][i, 1] for key in raw.ROWS}
        assert not got['converged'] and np.isfinite(got['mismatch']) and got['mismatch'] > 1e-8
        _check_zero_step_row(s, got, i, [2, 3], 1e-8, ('zero pivot', i))
    assert bool((res.iterations[:, [0, 2]] >= 1).all())                        # its neighbours in the list iterate
    _check_summaries(res, torch.ones(2, 3, dtype=torch.bool, device=DEV))
    zero = _run(s, 0, 1e-8, pairs=pairs, islanding=np.zeros(3, dtype=bool))
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
    for p, (j, k) in enumerate(s.pairs):
        if s.islanding[p]:
            _not_solved(res, 1, p)
            continue
        got = {key: host[key][1, p] for key in raw.ROWS}
        assert not got['converged'] and int(got['iterations']) == 0 and np.isnan(got['mismatch']), (j, k)
        assert np.array_equal(np.isnan(got['v']), np.arange(tp.n) == bus) and np.array_equal(got['theta'], va0), (j, k)
        assert np.array_equal(np.delete(got['v'], bus), np.delete(vm0, bus)), (j, k)
        assert np.isnan(got['v_min']) and np.isnan(got['v_max']) and int(got['v_min_bus']) == int(got['v_max_bus']) == bus, (j, k)
        want_nan = touching & ~np.isin(np.arange(f.size), [j, k])
        assert want_nan.any()                                                 # three proper lines at the bus, two lines out at most
        for key in FLOWS:
            assert np.array_equal(np.isnan(got[key]), want_nan), (j, k, key)
            assert got[key][j] == 0.0 and got[key][k] == 0.0, (j, k, key)
        assert np.isnan(got['worst_loading']) and int(got['worst_line']) == int(np.flatnonzero(want_nan)[0]), (j, k)
        n += 1
    assert n == int((~s.islanding).sum()) > 0
    assert any(touching[j] or touching[k] for (j, k), island in zip(s.pairs, s.islanding) if not island)    # a pair at the bus too


def test_id_columns_that_name_no_bus_or_no_entry():
    """The solve reads the blob's stamps, never the id columns, so only the tampered line's own flows and the rows of the pairs that
    hold it change.  ``pf_line_ends`` and ``pf_find_entry`` run once per line of the pair: the list holds the tampered line as
    the lower line of a pair and as the higher."""
    s = _setup('random40_parallel_selfloop', 'reference')
    tp = s.tp
    N, E = tp.n, tp.f.size
    bridges = powerflow._bridges(N, tp.f - 1, tp.t - 1)
    ends = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    e = next(k for k in range(E) if not bridges[k] and ends[k][0] != ends[k][1] and ends.count(ends[k]) == 1)
    lower = next((e, k) for k in range(e + 1, E) if not rows_islanding(tp, [(e, k)])[0])
    higher = next((j, e) for j in range(e) if not rows_islanding(tp, [(j, e)])[0])
    assert lower[0] == higher[1] == e
    pairs = list(dict.fromkeys(s.pairs + [lower, higher]))
    isl = rows_islanding(tp, pairs)
    with_e = [p for p, pr in enumerate(pairs) if e in pr]
    others = [p for p, pr in enumerate(pairs) if e not in pr]
    solved = [p for p in others if not isl[p]]
    assert len(with_e) >= 2 and solved
    clean = _run(s, 2, 1e-8, pairs=pairs, islanding=isl)
    assert bool((clean.iterations[:, [pairs.index(lower), pairs.index(higher)]] >= 1).all())            # solved while the ids are right
    not_flow = [k for k in raw.ROWS if k not in FLOWS + ('worst_loading', 'worst_line')]
    rest = [l for l in range(E) if l != e]

    def flows_elsewhere_unchanged(res, what):
        for key in FLOWS:
            assert _same(getattr(res, key)[:, others][:, :, rest], getattr(clean, key)[:, others][:, :, rest]), (what, key)

    for bad in (0.0, float(N + 1), 2.5):
        lines = s.lines.clone()
        lines[:, e, 0] = bad
        res = _run(s, 2, 1e-8, pairs=pairs, islanding=isl, lines=lines)
        _not_solved(res, slice(None), with_e)
        _same_rows(res, clean, jx=others, jy=others, fields=not_flow)
        flows_elsewhere_unchanged(res, bad)
        for key in FLOWS:
            assert bool(getattr(res, key)[:, solved, e].isnan().all()), (bad, key)
        assert bool(res.worst_loading[:, solved].isnan().all()) and bool((res.worst_line[:, solved] == e).all()), bad
    # two buses of the grid that no line joins: the pattern has no such entry
    adjacent = set(ends)
    a, b = next((a, b) for a in range(1, N + 1) for b in range(a + 1, N + 1) if (a, b) not in adjacent)
    lines = s.lines.clone()
    lines[:, e, 0], lines[:, e, 1] = float(a), float(b)
    res = _run(s, 2, 1e-8, pairs=pairs, islanding=isl, lines=lines)
    _not_solved(res, slice(None), with_e)
    _same_rows(res, clean, jx=others, jy=others, fields=not_flow)
    flows_elsewhere_unchanged(res, 'no entry')
    for key in FLOWS:
        assert bool(getattr(res, key)[:, solved, e].isfinite().all()), key


def test_two_identical_parallel_lines_tie_at_the_lower_index():
    """``test_ac_contingency_rows_gpu``'s tie on the toy's lines 0 (1 -> 2) and 5 (2 -> 1), identical, tau = 1 and no shift, in the
    rows of the non-islanding pairs that leave both in: their loadings are equal bit for bit and a rating makes the two the worst,
    so worst_line is the lower index.  With perturbed and with equal voltages, and with the two lines listed in the other order."""
    s = _setup('toy', 'reference')
    pairs = [(1, 6), (2, 6), (3, 6), (4, 6)]
    assert not rows_islanding(s.tp, pairs).any()
    assert sorted(pairs) == sorted(p for p, island in zip(s.pairs, s.islanding) if not island and 0 not in p and 5 not in p)
    lines = s.lines.clone()
    lines[:, [0, 5], 2:] = torch.tensor([0.01, 0.1, 0.04, 1.0, 0.0], device=DEV)       # r, x, b, tau, shift
    rating = torch.ones(7, dtype=torch.float64, device=DEV)
    rating[[0, 5]] = 1e-6
    every = torch.ones(2, 4, dtype=torch.bool, device=DEV)
    perm = [5, 1, 2, 3, 4, 0, 6]
    swapped = s.tp._replace(name='toy_swapped', f=s.tp.f[perm], t=s.tp.t[perm])
    for equal_v in (False, True):
        base_v, base_theta = s.base_v.copy(), s.base_theta.copy()
        if equal_v:
            base_v[:, 1] = s.starts[0][0][0], s.starts[1][0][0]          # bus 2 (PQ) at the slack's vg, and at its angle
            base_theta[:, 1] = base_theta[:, 0]
        for tp, ln in ((s.tp, lines), (swapped, lines[:, perm].contiguous())):
            res = raw.screen_pairs(tp, s.buses, ln, s.gens, pairs, base_v, base_theta, np.ones(2), np.zeros(4), rating, 0, 1e-8)
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


@pytest.mark.parametrize('name', ['ring64', 'wheel71'])
def test_rows_are_bit_identical_at_the_wave_edges(name, monkeypatch):
    s = _setup(name, 'wide')
    E, P = s.tp.f.size, len(s.pairs)
    full = _run(s, 1, 0.0)
    ok = _ok_mask(s, full)
    assert bool((full.iterations[ok] == 1).all()) and bool((full.iterations[~ok] == -1).all())

    def run(at, grids=slice(None), flip=False):
        pairs = [s.pairs[p][::-1] if flip else s.pairs[p] for p in at]
        return _run(s, 1, 0.0, pairs=pairs, islanding=s.islanding[at], grids=grids)

    perm = torch.randperm(P, generator=torch.Generator().manual_seed(E)).tolist()
    _same_rows(run(perm), full, jy=perm)
    _same_rows(run(list(range(P)), flip=True), full)                            # (k, j) is (j, k)
    where = {e: next(p for p, pr in enumerate(s.pairs) if e in pr and not s.islanding[p]) for e in (63, 64, E - 1)}
    dup = [where[E - 1], 3, where[E - 1], where[64], 0, where[63], where[E - 1], where[64]]
    _same_rows(run(dup), full, jy=dup)
    _same_rows(run(list(range(P)), grids=slice(1, 2)), full, gy=slice(1, 2))
    _same_rows(run([where[E - 1]], grids=slice(1, 2)), full, gy=slice(1, 2), jy=[where[E - 1]])
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', True)                      # nothing is read that nothing wrote
    _same_rows(_run(s, 1, 0.0), full)
    _same_rows(run(perm), full, jy=perm)
    _same_rows(run(list(range(P)), flip=True), full)
    _same_rows(run(dup), full, jy=dup)
    _same_rows(run(dup, grids=slice(1, 2), flip=True), full, gy=slice(1, 2), jy=dup)
    _same_rows(run([where[E - 1]], grids=slice(1, 2)), full, gy=slice(1, 2), jy=[where[E - 1]])
