"""Every listed row of the AC generator contingency screen (``gns_acg1_screen``, include/gns_powerflow.h "AC generator contingency
screening") on the MI355X, pinned without waiting for Newton-Raphson to converge, as ``test_ac_contingency_rows_gpu`` and
``test_ac_n2_rows_gpu`` pin the line screens: after zero steps a row is the reference start bit for bit with the reference mismatch
and flows of the grid without the unit (its row deleted, the pickup applied: ``ac_generator_contingency_reference.without``) and
without the line, and after one step its update solves the reference Jacobian of that grid to ``pt.STEP_TOL``, with the roles of
the reduced generator table.  Both hold on 100 % of the non-islanding rows of a list, where ``test_ac_generator_contingency_gpu``
can compare only the rows the reference converges.  What is this kernel's own is the choice of a blob per row, the lost unit, W_g and
the pickup share in the specified P: a wrong share, role, set point, blob or W_g moves the zero-step mismatch by the size of an
injection, orders above its bar.  Also here: the flags the caller owns, the kernel's own refusals (reached by tampering with the
DEVICE copy of a list alone, so that the host's checks pass), a member of another shape, id columns that name no bus or no pattern
entry, which rows a NaN in ``base_v`` at a unit's bus stops, and bit identity at the wave-edge shapes with members of two dimensions.

The calls go through ``ac_contingency_raw.screen_generators``: ``base_theta`` is 0.3 at the slack and ``max_iter`` of 0 or 1 applies
to the rows only.  Grids are ``pt.grids(tp, regime, 2, seed=11)`` in both value regimes on ``ac_generator_rows.FAMILIES``: N, E or
the list at 63 / 64 / 65 with a line out, N 71 and 150, parallel lines and a self-loop, four units on one bus and two on the slack
(members of two dimensions), a slack without a unit, 70 lines at one bus, and 66 and 70 generator rows (more than a wave's lanes).
The rows are ``ac_generator_rows.rows_list`` (at most 256), the islanding mask ``powerflow._bridges``.

Non-islanding rows of the two grids of each list, counted on the CPU with the reference alone (the same in both regimes and with
every pickup): toy 32 of 32 rows, random40_parallel_selfloop 460 of 512, random24_stacked_gens 444 of 512, ring63 390 of 390,
ring64 396 of 396, ring65 402 of 402, wheel71 512 of 512, hub150_70lines_70gens 140 of 512, wheel71_66gens 512 of 512.  The
reference's own one-step guard (scipy's step within ``pt.STEP_TOL``) was run on the CPU on every one of these rows in both
regimes: worst 2.7e-16, no row had to be replaced.  The bars are those of the N-1 file: ``_mismatch_and_bar``, ``_flow_bar``,
``pt.STEP_TOL``."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow
import ac_contingency_raw as raw
import ac_generator_contingency_reference as gref
from ac_generator_rows import FAMILIES, PICKUPS, pickup_weights, row_reference, rows_islanding, rows_list, topology
import nr_reference as nr
import pf_topologies as pt
from test_ac_contingency_host import one_step_ratios, shifted_base
from test_ac_contingency_rows_gpu import (DEV, FLOWS, _check_flows, _check_summaries, _check_zero_step_row, _host, _not_solved,
                                          _ok_mask, _same, _same_rows)

pytestmark = pytest.mark.gpu
N_ROWS = {'toy': 32, 'random40_parallel_selfloop': 460, 'random24_stacked_gens': 444, 'ring63': 390, 'ring64': 396, 'ring65': 402,
          'wheel71': 512, 'hub150_70lines_70gens': 140, 'wheel71_66gens': 512}


@functools.lru_cache(maxsize=None)
def _setup(name, regime):
    """What the tests of one (topology, values) share: the device inputs, their float64 host copies, the base state with
    base_theta[slack] = 0.3, the row list and its islanding mask."""
    tp = topology(name)
    buses, lines, gens, v, theta = pt.grids(tp, regime, 2, seed=11, device=DEV)
    b, l, g = (t.cpu().double().numpy() for t in (buses, lines, gens))
    base_v, base_theta = shifted_base(tp, v, theta)
    assert np.all(base_theta[:, tp.slack - 1] == 0.3)
    rows = rows_list(tp)
    return SimpleNamespace(tp=tp, buses=buses, lines=lines, gens=gens, b=b, l=l, g=g, base_v=base_v, base_theta=base_theta, rows=rows,
                           islanding=rows_islanding(tp, rows))


def _run(s, max_iter, tol, at=None, islanding=None, base_converged=None, rating=None, pickup=None, grids=slice(None), lines=None,
         base_v=None, tamper=None, extra=()):
    """The rows ``s.rows`` (or those at the positions ``at`` of the list) of the grids ``grids`` of ``s``."""
    rows = s.rows if at is None else [s.rows[p] for p in at]
    if islanding is None:
        islanding = s.islanding if at is None else s.islanding[at]
    base_v = s.base_v if base_v is None else base_v
    Bt = s.buses[grids].shape[0]
    base_converged = np.ones(Bt, dtype=np.uint8) if base_converged is None else base_converged
    if pickup is not None and np.ndim(pickup) == 2:
        pickup = pickup[grids]
    return raw.screen_generators(s.tp, s.buses[grids], (s.lines if lines is None else lines)[grids], s.gens[grids], rows,
                                 base_v[grids], s.base_theta[grids], base_converged, islanding, rating, pickup, max_iter, tol,
                                 tamper=tamper, extra=extra)


@pytest.mark.parametrize('kind', PICKUPS)
@pytest.mark.parametrize('regime', pt.REGIMES)
@pytest.mark.parametrize('name', FAMILIES)
def test_zero_steps_every_listed_row(name, regime, kind):
    """``v`` and ``theta`` are ``nr.start`` on the grid without the unit bit for bit (a freed bus at its old set point, a shared bus at
    the next unit's ``vg``, a slack without a unit at 1), the mismatch is the reference's with the pickup in the specified P, the
    flows are the reference's and exactly 0 at line k.  Pickups: None; random weights [Bt,Gn] in [0.1, 1.1) with one column exactly
    zero; weights that are zero but for the last unit's, so that W_g is exactly 0 in that unit's rows alone and every other row sends
    the whole lost output to it.  Rows compared: ``N_ROWS``, all of the non-islanding rows."""
    s = _setup(name, regime)
    tol = 1e-8
    w = pickup_weights(kind, 2, s.tp.g.size)
    res = _run(s, 0, tol, pickup=w)
    host = _host(res)
    n_cmp, worst = 0, 0.0
    for i in range(2):
        for p, (g, k) in enumerate(s.rows):
            if s.islanding[p]:
                _not_solved(res, i, p)
                continue
            got = {key: host[key][i, p] for key in raw.ROWS}
            view, out = row_reference(s, i, g, k, gref.weights(w, s.g[i], i))
            worst = max(worst, _check_zero_step_row(view, got, i, out, tol, (name, regime, kind, i, g, k)))
            n_cmp += 1
    n_rows = 2 * int((~s.islanding).sum())
    print(f'{name} ({regime}, pickup {kind}) zero steps: compared {n_cmp} of {n_rows} non-islanding rows '
          f'({100 * n_cmp // n_rows} %), worst flow error {worst:.2f} of its bar')
    assert n_cmp == n_rows == N_ROWS[name] > 0
    _check_summaries(res, _ok_mask(s, res))


@pytest.mark.parametrize('name,units', [('random24_stacked_gens', (2, 3, 6, 7)), ('wheel71_66gens', (5, 64, 65))])
def test_zero_steps_a_list_that_names_some_of_the_units(name, units):
    """The listed rows of ``units`` alone: the set then holds a member per unit of the list, so a row's position into ``gen_list``
    is not its generator row, and the blob is the one at ``member_off[position]``.  On random24_stacked_gens units 2 and 6 are sole
    units (a freed bus, one unknown more) and 3 and 7 share bus 4.  Every row against the reference, and with the full list's bits."""
    s = _setup(name, 'reference')
    tol = 1e-8
    w = pickup_weights('random', 2, s.tp.g.size)
    at = [p for p, (g, _) in enumerate(s.rows) if g in units]
    st = raw.generator_set(s.tp, [s.rows[p] for p in at])
    assert st.gen_list.tolist() == list(units) and not np.array_equal(st.gen_list, np.arange(len(units)))
    res = _run(s, 0, tol, at=at, pickup=w)
    _same_rows(res, _run(s, 0, tol, pickup=w), jy=at)
    host = _host(res)
    n_cmp = 0
    for i in range(2):
        for j, p in enumerate(at):
            if s.islanding[p]:
                _not_solved(res, i, j)
                continue
            g, k = s.rows[p]
            view, out = row_reference(s, i, g, k, gref.weights(w, s.g[i], i))
            _check_zero_step_row(view, {key: host[key][i, j] for key in raw.ROWS}, i, out, tol, (name, i, g, k))
            n_cmp += 1
    assert n_cmp == 2 * int((~s.islanding[at]).sum()) >= 2 * len(units)


@pytest.mark.parametrize('regime', pt.REGIMES)
@pytest.mark.parametrize('name', FAMILIES)
def test_one_step_every_listed_row(name, regime):
    """The rows of ``test_zero_steps_every_listed_row`` (random weights) after one Newton step: the step solves the reference Jacobian
    of the grid without the unit and the line, ``pq`` / ``pvpq`` from ``nr.roles`` on the reduced generator table."""
    s = _setup(name, regime)
    w = pickup_weights('random', 2, s.tp.g.size)
    res = _run(s, 1, 0.0, pickup=w)
    host = _host(res)
    n_cmp, worst, worst_flow = 0, 0.0, 0.0
    for i in range(2):
        for p, (g, k) in enumerate(s.rows):
            if s.islanding[p]:
                _not_solved(res, i, p)
                continue
            what = (name, regime, i, g, k)
            got = {key: host[key][i, p] for key in raw.ROWS}
            assert int(got['iterations']) == 1 and not got['converged'], what
            assert np.isfinite(got['v']).all() and np.isfinite(got['theta']).all() and np.isfinite(got['mismatch']), what
            view, out = row_reference(s, i, g, k, gref.weights(w, s.g[i], i))
            vm0, va0 = view.starts[i]
            r_scipy, r_dev = one_step_ratios(s.b[i], s.l[i], view.g[i], s.tp.slack, out, vm0, va0, got['v'], got['theta'])
            assert r_scipy <= pt.STEP_TOL, (what, r_scipy)              # the grid without the unit and the line is conditioned well enough ...
            assert r_dev <= pt.STEP_TOL, (what, r_dev)                  # ... so a failure here is the kernel's
            _, pv, pq = nr.roles(s.b[i], view.g[i], s.tp.slack)
            fixed = np.setdiff1d(np.arange(s.tp.n), pq)
            assert np.array_equal(got['v'][fixed], vm0[fixed]) and got['theta'][s.tp.slack - 1] == 0.0, what
            worst = max(worst, r_dev)
            worst_flow = max(worst_flow, _check_flows(got, s.l[i], got['v'], got['theta'], out, what))
            n_cmp += 1
    n_rows = 2 * int((~s.islanding).sum())
    print(f'{name} ({regime}) one step: compared {n_cmp} of {n_rows} non-islanding rows ({100 * n_cmp // n_rows} %), '
          f'worst one-step ratio {worst:.1e}, worst flow error {worst_flow:.2f} of its bar')
    assert n_cmp == n_rows == N_ROWS[name] > 0
    _check_summaries(res, _ok_mask(s, res))


@pytest.mark.parametrize('name', ['toy', 'random40_parallel_selfloop', 'ring64'])
def test_flags_and_ratings_are_the_callers(name):
    s = _setup(name, 'wide')
    E, P = s.tp.f.size, len(s.rows)
    w = pickup_weights('random', 2, s.tp.g.size)
    clean = _run(s, 1, 0.0, pickup=w)
    solved = np.flatnonzero(~s.islanding)
    p0 = int(solved[E // 3 % solved.size])                                     # a row that does not island, flagged anyway
    flagged = s.islanding.copy()
    flagged[p0] = True
    res = _run(s, 1, 0.0, pickup=w, islanding=flagged)
    _not_solved(res, slice(None), p0)
    others = [p for p in range(P) if p != p0]
    _same_rows(res, clean, jx=others, jy=others)
    assert int(clean.iterations[0, p0]) == 1
    res = _run(s, 1, 0.0, pickup=w, base_converged=np.array([1, 0], dtype=np.uint8))
    _not_solved(res, 1, slice(None))
    _same_rows(res, clean, gx=slice(0, 1), gy=slice(0, 1))
    gen = torch.Generator().manual_seed(E)
    ok = _ok_mask(s, clean)
    for shape in ((E,), (2, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=gen, dtype=torch.float64)).to(DEV)
        rated = _run(s, 1, 0.0, pickup=w, rating=rating)
        _same_rows(rated, clean, fields=[k for k in raw.ROWS if k not in ('worst_loading', 'worst_line')])
        _check_summaries(rated, ok, rating)                                   # against the returned flows
        assert not torch.equal(rated.worst_loading[ok], clean.worst_loading[ok])
    _check_summaries(clean, ok)


def _members_of_both_dimensions(s):
    """(a position of the list whose member is the base dimension, one whose member has a freed bus), both solved rows with a line
    out where the list has one."""
    dims = {g: raw.analysed_without(s.tp, g).info['dim'] for g in {g for g, _ in s.rows}}
    small, large = min(dims.values()), max(dims.values())
    assert large == small + 1

    def first(dim):
        at = [p for p, (g, k) in enumerate(s.rows) if dims[g] == dim and not s.islanding[p]]
        return next((p for p in at if s.rows[p][1] >= 0), at[0])

    return first(small), first(large)


@pytest.mark.parametrize('name', ['random24_stacked_gens', 'wheel71_66gens'])
def test_the_kernels_own_refusals(name):
    """The device copy of one list tampered with, one change per call; the host copies stay valid, so the host checks pass.  Each of
    these values is decided by a comparison before anything is read through it (``pf_set_member``, ``gi >= 0 && gi < Gn``,
    ``cg < n_member``): the rows that name it are not solved in every grid, every other row has the clean call's bits."""
    s = _setup(name, 'reference')
    Gn = s.tp.g.size
    at = list(range(Gn)) + list(range(Gn, len(s.rows), 5))                      # every unit alone, and every fifth row after them
    rows = [s.rows[p] for p in at]
    assert rows[:Gn] == [(g, -1) for g in range(Gn)]
    w = pickup_weights('random', 2, s.tp.g.size)
    clean = _run(s, 1, 0.0, at=at, pickup=w)
    st = raw.generator_set(s.tp, rows)
    n_member = st.member_off.size
    assert n_member == Gn >= 3 and st.host.size % 16 == 0
    m = n_member // 2                                                          # a member in the middle of the set
    hit_m = [j for j in range(len(rows)) if st.row_cols[j, 0] == m]
    j0 = len(rows) // 2
    cases = [('member_off', m, -16, hit_m), ('member_off', m, int(st.member_off[m]) + 4, hit_m),
             ('member_off', m, st.host.size, hit_m), ('gen_list', m, -1, hit_m), ('gen_list', m, Gn, hit_m),
             ('row_cols', (j0, 0), -1, [j0]), ('row_cols', (j0, 0), n_member, [j0])]
    solved_hit = 0
    for key, where, value, hit in cases:
        bad = getattr(st, key).copy()
        bad[where] = value
        res = _run(s, 1, 0.0, at=at, pickup=w, tamper={key: bad})
        assert hit, (key, value)
        _not_solved(res, slice(None), hit)
        others = [j for j in range(len(rows)) if j not in hit]
        _same_rows(res, clean, jx=others, jy=others)
        solved_hit += int((clean.iterations[:, hit] == 1).sum())
    assert solved_hit >= len(cases)                                             # rows the clean call solves


def test_a_member_of_another_shape_is_not_solved():
    """An analysis of another topology (ring63: another N, E and Gn) laid out in the set after the members, at a valid offset that
    only the device copy of ``member_off`` names: ``pf_set_member`` reads its header and refuses it."""
    s = _setup('random24_stacked_gens', 'reference')
    other = topology('ring63')
    foreign = powerflow.analyse_topology(other.n, other.f, other.t, other.g, other.slack).host
    at = list(range(0, len(s.rows), 5))
    rows = [s.rows[p] for p in at]
    clean = _run(s, 1, 0.0, at=at, extra=[foreign])
    _same_rows(clean, _run(s, 1, 0.0, at=at))                                   # words no list names change nothing
    st = raw.generator_set(s.tp, rows, [foreign])
    assert st.extra_off.size == 1 and st.extra_off[0] % 16 == 0 and st.extra_off[0] + foreign.size <= st.host.size
    m = 1
    bad = st.member_off.copy()
    bad[m] = st.extra_off[0]
    hit = [j for j in range(len(rows)) if st.row_cols[j, 0] == m]
    res = _run(s, 1, 0.0, at=at, extra=[foreign], tamper={'member_off': bad})
    assert hit and bool((clean.iterations[:, hit] == 1).any())
    _not_solved(res, slice(None), hit)
    others = [j for j in range(len(rows)) if j not in hit]
    _same_rows(res, clean, jx=others, jy=others)


def test_id_columns_that_name_no_bus_or_no_entry():
    """``test_ac_n2_rows_gpu``'s test on the rows (g, e) of a unit whose bus is freed: the solve reads the blob's stamps, never the id
    columns, so only the tampered line's own flows and the rows that hold it change."""
    s = _setup('random40_parallel_selfloop', 'reference')
    tp = s.tp
    N, E = tp.n, tp.f.size
    bridges = powerflow._bridges(N, tp.f - 1, tp.t - 1)
    ends = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    e = next(k for k in range(E) if not bridges[k] and ends[k][0] != ends[k][1] and ends.count(ends[k]) == 1)
    sole = [g for g in range(tp.g.size) if tp.g[g] != tp.slack and int((tp.g == tp.g[g]).sum()) == 1]
    assert len(sole) >= 2
    rows = list(dict.fromkeys([r for r in s.rows[:96]] + [(sole[0], e), (sole[-1], e)]))
    isl = rows_islanding(tp, rows)
    with_e = [p for p, (_, k) in enumerate(rows) if k == e]
    others = [p for p in range(len(rows)) if p not in with_e]
    solved = [p for p in others if not isl[p]]
    assert len(with_e) >= 2 and solved

    def run(lines=None):
        return raw.screen_generators(tp, s.buses, s.lines if lines is None else lines, s.gens, rows, s.base_v, s.base_theta,
                                     np.ones(2), isl, None, pickup_weights('random', 2, tp.g.size), 2, 1e-8)

    clean = run()
    assert bool((clean.iterations[:, with_e] >= 1).all())                       # solved while the ids are right
    not_flow = [k for k in raw.ROWS if k not in FLOWS + ('worst_loading', 'worst_line')]
    rest = [l for l in range(E) if l != e]

    def flows_elsewhere_unchanged(res, what):
        for key in FLOWS:
            assert _same(getattr(res, key)[:, others][:, :, rest], getattr(clean, key)[:, others][:, :, rest]), (what, key)

    for bad in (0.0, float(N + 1), 2.5):
        lines = s.lines.clone()
        lines[:, e, 0] = bad
        res = run(lines)
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
    res = run(lines)
    _not_solved(res, slice(None), with_e)
    _same_rows(res, clean, jx=others, jy=others, fields=not_flow)
    flows_elsewhere_unchanged(res, 'no entry')
    for key in FLOWS:
        assert bool(getattr(res, key)[:, solved, e].isfinite().all()), key


def test_a_nan_at_a_units_bus_stops_the_rows_that_free_it():
    """The start rule: |V| at the row's PQ buses comes from ``base_v``, at PV and slack buses from the row's set points.  A NaN in
    ``base_v`` at the bus of a sole unit (PV in the base case) is overwritten by the set point in every row that keeps the bus PV:
    those rows solve, with the clean call's bits.  The rows of that unit free the bus and start from the NaN: they stop with
    ``iterations == 0``, a NaN mismatch, the NaN in ``v`` at that bus alone and the reference start elsewhere."""
    s = _setup('random40_parallel_selfloop', 'reference')
    tp = s.tp
    f, t = tp.f - 1, tp.t - 1
    sole = [g for g in range(tp.g.size) if tp.g[g] != tp.slack and int((tp.g == tp.g[g]).sum()) == 1]
    u = max(sole, key=lambda g: int(np.sum(((f == tp.g[g] - 1) | (t == tp.g[g] - 1)) & (f != t))))        # the one with most lines
    bus = int(tp.g[u]) - 1
    touching = (f == bus) | (t == bus)
    assert int(np.sum(touching & (f != t))) >= 2                               # a line of the bus is left in every row
    base_v = s.base_v.copy()
    base_v[1, bus] = np.nan
    clean = _run(s, 3, 1e-8)
    res = _run(s, 3, 1e-8, base_v=base_v)
    _same_rows(res, clean, gx=slice(0, 1), gy=slice(0, 1))
    keeps = [p for p, (g, _) in enumerate(s.rows) if g != u]
    _same_rows(res, clean, jx=keeps, jy=keeps)
    assert bool((clean.iterations[1, [p for p in keeps if not s.islanding[p]]] >= 1).all())
    host = _host(res)
    n = 0
    for p, (g, k) in enumerate(s.rows):
        if g != u:
            continue
        if s.islanding[p]:
            _not_solved(res, 1, p)
            continue
        view, _ = row_reference(s, 1, g, k, None)
        vm0, va0 = view.starts[1]
        got = {key: host[key][1, p] for key in raw.ROWS}
        assert not got['converged'] and int(got['iterations']) == 0 and np.isnan(got['mismatch']), (g, k)
        assert np.array_equal(np.isnan(got['v']), np.arange(tp.n) == bus) and np.array_equal(got['theta'], va0), (g, k)
        assert np.array_equal(np.delete(got['v'], bus), np.delete(vm0, bus)), (g, k)
        assert np.isnan(got['v_min']) and np.isnan(got['v_max']) and int(got['v_min_bus']) == int(got['v_max_bus']) == bus, (g, k)
        want_nan = touching & (np.arange(f.size) != k)
        for key in FLOWS:
            assert np.array_equal(np.isnan(got[key]), want_nan), (g, k, key)
        assert np.isnan(got['worst_loading']) and int(got['worst_line']) == int(np.flatnonzero(want_nan)[0]), (g, k)
        n += 1
    assert n >= 2 and any(k >= 0 for p, (g, k) in enumerate(s.rows) if g == u and not s.islanding[p])


@pytest.mark.parametrize('name', ['ring64', 'wheel71_66gens', 'random24_stacked_gens'])
def test_rows_are_bit_identical_at_the_wave_edges(name, monkeypatch):
    s = _setup(name, 'wide')
    E, P = s.tp.f.size, len(s.rows)
    w = pickup_weights('random', 2, s.tp.g.size)
    full = _run(s, 1, 0.0, pickup=w)
    ok = _ok_mask(s, full)
    assert bool((full.iterations[ok] == 1).all()) and bool((full.iterations[~ok] == -1).all())

    def run(at, grids=slice(None)):
        return _run(s, 1, 0.0, at=at, pickup=w, grids=grids)

    perm = torch.randperm(P, generator=torch.Generator().manual_seed(E)).tolist()
    solved = [p for p in range(P) if not s.islanding[p]]
    where = {e: next((p for p in solved if s.rows[p][1] == e), solved[-1]) for e in (63, 64, E - 1)}
    dup = [where[E - 1], 3, where[E - 1], where[64], 0, where[63], where[E - 1], where[64]]
    lists = [perm, dup]
    if name == 'ring64':                                                       # no unit on the slack or on a shared bus: one dimension
        assert len({raw.analysed_without(s.tp, g).info['dim'] for g in range(s.tp.g.size)}) == 1
        lists.append([where[E - 1]])
    else:
        small, large = _members_of_both_dimensions(s)
        # one row whose member is the larger image; a smaller member first and a larger last, and the reverse
        lists += [[large], [small, 1, large], [large, 1, small]]
    for at in lists:
        _same_rows(run(at), full, jy=at)
    _same_rows(run(list(range(P)), grids=slice(1, 2)), full, gy=slice(1, 2))
    _same_rows(run(lists[2], grids=slice(1, 2)), full, gy=slice(1, 2), jy=lists[2])
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', True)                      # nothing is read that nothing wrote
    _same_rows(_run(s, 1, 0.0, pickup=w), full)
    for at in lists:
        _same_rows(run(at), full, jy=at)
    _same_rows(run(dup, grids=slice(1, 2)), full, gy=slice(1, 2), jy=dup)
    _same_rows(run(lists[-1], grids=slice(1, 2)), full, gy=slice(1, 2), jy=lists[-1])
