"""CPU checks of the AC N-2 contingency screen's host side (include/gns_powerflow.h, "AC N-2 contingency screening"): the exports,
the refusals of the Python wrapper and of the C entry points (each before a launch, so no device is needed), the pair islanding
against a graph search, and the claim the kernel rests on: each of the at most eight Y-bus entries of a pair, summed from the blob's
own stamp lists in order with both lines skipped, is the entry of the Y-bus of the grid without the two lines, and no other entry
changes; then one Newton step of the kernel's algorithm replayed in numpy on those entries, on every pair of the lists
(``rows_pairs``) that ``test_ac_n2_rows_gpu`` runs on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import _lib, powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig
from helpers import ROOT
import ac_contingency_reference as aref
import ac_n2_reference as n2ref
from ac_n2_pairs import pair_kinds, rows_islanding, rows_pairs
import nr_reference as nr
import pf_topologies as pt
from test_ac_contingency_host import EINVAL, ESIZE, EUNSUPPORTED, _case14, emulate_row, one_step_ratios, shifted_base, toy
from test_powerflow_grad_host import H, _arr

FIELDS = ('base', 'pairs', 'v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'worst_line', 'v_min', 'v_min_bus',
          'v_max', 'v_max_bus', 'converged', 'iterations', 'mismatch', 'islanding')


def test_exports_are_there_and_disjoint():
    lib = amd.load_library()
    assert _lib.ACN2_EXPORTS == ('gns_acn2_workspace_bytes', 'gns_acn2_screen')
    others = (_lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.DCN2_EXPORTS +
              _lib.DCN2_ADJOINT_EXPORTS + _lib.ACN1_EXPORTS + _lib.ACN1_ADJOINT_EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    for f in _lib.ACN2_EXPORTS:
        assert hasattr(lib, f) and f not in others, f
        assert getattr(lib, f).restype is ctypes.c_int
        assert f'int {f}(' in hdr
    assert 'AC N-2 contingency screening' in hdr
    assert callable(powerflow.ac_n2_contingency_screen) and powerflow.AcN2ContingencyResult._fields == FIELDS
    assert FIELDS == tuple('pairs' if k == 'outages' else k for k in powerflow.AcContingencyResult._fields)
    assert powerflow._ACN2.prefix == 'gns_acn2' and powerflow._ACN2.formula == powerflow._LDS_FORMULA


def test_python_refusals_come_before_a_device_is_needed():
    buses, lines, gens = synth.synth_grids(14, 3)
    E = lines.shape[1]

    def screen(**kw):
        return powerflow.ac_n2_contingency_screen(buses, lines, gens, slack_bus=1, **kw)

    for bad in ([], np.zeros((0, 2), dtype=np.int64), torch.zeros(0, 2, dtype=torch.long)):
        with pytest.raises(ValueError, match='pairs is empty'):
            screen(pairs=bad)
    for bad in ([0, 1], [[0, 1, 2]], np.zeros((2, 2, 2), dtype=np.int64), [[0], [1]]):
        with pytest.raises(ValueError, match=r'pairs must be a \[P,2\]'):
            screen(pairs=bad)
    for bad in ([[0.0, 1.0]], [[0, 1.5]], np.array([[True, False]])):
        with pytest.raises(ValueError, match='pairs must hold integers'):
            screen(pairs=bad)
    for bad in ([[0, E]], [[-1, 2]], [[0, 1], [3, E + 5]], torch.tensor([[E, 0]])):
        with pytest.raises(ValueError, match='pairs must lie in'):
            screen(pairs=bad)
    with pytest.raises(ValueError, match=r"two different lines, got \(4, 4\) at row 1: a single outage is ac_contingency_screen's"):
        screen(pairs=[[0, 1], [4, 4]])
    # the DC screen's refusal of the same list is what it was
    with pytest.raises(ValueError) as e:
        powerflow.dc_n2_contingency_screen(buses, lines, gens, slack_bus=1, pairs=[[0, 1], [4, 4]])
    assert str(e.value) == ("pairs must name two different lines, got (4, 4) at row 1: a single outage is dc_contingency_screen's")
    with pytest.raises(ValueError) as e:
        powerflow._pair_list([[2, 2]], E)
    assert str(e.value) == ("pairs must name two different lines, got (2, 2) at row 0: a single outage is dc_contingency_screen's")
    for bad in (torch.zeros(E), -torch.ones(E), torch.full((3, E), float('nan'))):
        with pytest.raises(ValueError, match='rating must be positive and finite'):
            screen(rating=bad)
    for bad in (torch.ones(E - 1), torch.ones(2, E), 1.0):
        with pytest.raises(ValueError, match='rating must be'):
            screen(rating=bad)
    with pytest.raises(ValueError, match='flows must be a bool'):
        screen(flows=1)
    with pytest.raises(ValueError, match='states must be a bool'):
        screen(states=None)
    for bad in (-1e-9, float('nan')):
        with pytest.raises(ValueError, match='tol must be'):
            screen(tol=bad)
    for bad in (-1, 2.5, None):
        with pytest.raises(ValueError, match='max_iter must be'):
            screen(max_iter=bad)
    with pytest.raises(TypeError):
        screen(differentiable=True)                       # not a keyword of this call
    with pytest.raises(ValueError, match='float32'):
        powerflow.ac_n2_contingency_screen(buses.double(), lines, gens, slack_bus=1)
    with pytest.raises(ValueError, match='batch sizes'):
        powerflow.ac_n2_contingency_screen(buses[:2], lines, gens, slack_bus=1)
    mixed = lines.clone()
    mixed[1, 0, 1] = 5
    with pytest.raises(ValueError, match='differ across the batch: ac_n2_contingency_screen solves one topology'):
        powerflow._topology_key(buses, mixed, gens, 1, 'ac_n2_contingency_screen')
    # the default list and what a list keeps
    assert powerflow._pair_list(None, 4, 'ac_contingency_screen').tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert powerflow._pair_list([[3, 1], [3, 1], [1, 3]], 4, 'ac_contingency_screen').tolist() == [[3, 1], [3, 1], [1, 3]]


@pytest.mark.parametrize('case,islanding,pairs', [(14, 27, 190), (30, 208, 820)])
def test_pair_islanding_is_the_graph_search(case, islanding, pairs):
    f, t, g = synth.case_topology(case)
    every = powerflow._pair_list(None, f.size, 'ac_contingency_screen')
    assert every.shape == (pairs, 2)
    got = powerflow._pair_islanding(case, f - 1, t - 1, every)
    lines = np.stack([f, t], axis=1).astype(np.float64)
    want = np.array([n2ref.pair_islands(case, lines, synth._solvable_slack(case), j, k) for j, k in every.tolist()])
    assert np.array_equal(got, want) and int(got.sum()) == islanding
    assert np.array_equal(powerflow._pair_islanding(case, f - 1, t - 1, every[:, ::-1]), got)       # either order
    topo = powerflow.analyse_topology(case, f, t, g, synth._solvable_slack(case))
    args = (case, f.astype(np.int32), t.astype(np.int32))
    assert np.array_equal(powerflow._topology_pair_islanding(topo, args, every), want)              # what the call uses


def _screen(lib, cfg, blob, pairs, ws_bytes=None, **kw):
    """gns_acn2_screen on dummy (never dereferenced) device pointers; a keyword replaces one argument.  Only calls the host refuses
    are made."""
    d = blob.ctypes.data
    o = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, pairs_host=o.ctypes.data,
             pairs_dev=d, P=o.shape[0], isl=d, rating=None, per_grid=0, base_v=d, base_theta=d, base_conv=d, v=None, theta=None,
             p_from=None, q_from=None, p_to=None, q_to=None, worst=d, worst_line=d, v_min=d, v_min_bus=d, v_max=d, v_max_bus=d, conv=d,
             iters=d, mis=d, ws=d, ws_bytes=0 if ws_bytes is None else ws_bytes)
    a.update(kw)
    return lib.gns_acn2_screen(*(a[k] for k in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'Bt', 'pairs_host', 'pairs_dev', 'P',
                                                'isl', 'rating', 'per_grid', 'base_v', 'base_theta', 'base_conv', 'v', 'theta',
                                                'p_from', 'q_from', 'p_to', 'q_to', 'worst', 'worst_line', 'v_min', 'v_min_bus',
                                                'v_max', 'v_max_bus', 'conv', 'iters', 'mis', 'ws', 'ws_bytes')), None)


def test_entry_points_return_the_documented_codes_before_any_launch():
    lib = amd.load_library()
    tp = _case14()
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    E = tp.f.size
    cfg = PfConfig(tp.n, E, tp.g.size, 10, 1e-8)
    d = topo.host.ctypes.data
    need, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for Bt in (1, 4, 77):
        assert lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), d, Bt, E, ctypes.byref(n1)) == 0
        for P in (1, 190, 100000):                                               # the base Y-bus only, whatever P
            assert lib.gns_acn2_workspace_bytes(ctypes.byref(cfg), d, Bt, P, ctypes.byref(need)) == 0
            assert need.value == n1.value >= Bt * 16 * topo.info['nnz_ybus'], (Bt, P)
    for args in ((None, d, 4, 3, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, 3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 3, None), (ctypes.byref(cfg), d, 0, 3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, -3, ctypes.byref(need))):
        assert lib.gns_acn2_workspace_bytes(*args) == EINVAL, args
    # NULL pointers (v, theta, the four flows and the rating may be NULL: they are in every call here)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'pairs_host', 'pairs_dev', 'isl', 'base_v', 'base_theta', 'base_conv',
                 'worst', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus', 'conv', 'iters', 'mis', 'ws'):
        assert _screen(lib, None if name == 'cfg' else cfg, topo.host, [[0, 3]], **({} if name == 'cfg' else {name: None})) == EINVAL, name
    # a config that does not match the blob, or that gns_pf_solve refuses
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8), PfConfig(tp.n, E + 1, tp.g.size, 10, 1e-8),
                PfConfig(tp.n, E, tp.g.size + 1, 10, 1e-8), PfConfig(tp.n, E, tp.g.size, -1, 1e-8),
                PfConfig(tp.n, E, tp.g.size, 10, -1.0)):
        assert _screen(lib, bad, topo.host, [[0, 1]]) == EINVAL
    assert lib.gns_acn2_workspace_bytes(ctypes.byref(PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8)), d, 4, 3, ctypes.byref(need)) == EINVAL
    # a fast-decoupled blob where a Newton-Raphson blob is expected
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert _screen(lib, cfg, fd.host, [[0, 1]]) == EINVAL
    assert lib.gns_acn2_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 4, 3, ctypes.byref(need)) == EINVAL
    # the pairs: an index outside 0 .. E-1 at either position, twice the same line
    for bad in ([[0, E]], [[E, 0]], [[-1, 2]], [[2, -1]], [[0, 1], [2, 3], [4, E]], [[2 ** 31 - 1, 0]], [[5, 5]], [[0, 1], [7, 7]]):
        assert _screen(lib, cfg, topo.host, bad, ws_bytes=2 ** 40) == EINVAL, bad
    assert _screen(lib, cfg, topo.host, [[0, 1]], P=0) == EINVAL and _screen(lib, cfg, topo.host, [[0, 1]], P=-1) == EINVAL
    assert _screen(lib, cfg, topo.host, [[0, 1]], Bt=0) == EINVAL and _screen(lib, cfg, topo.host, [[0, 1]], Bt=-1) == EINVAL
    assert _screen(lib, cfg, topo.host, [[0, 1]], per_grid=2) == EINVAL
    assert _screen(lib, cfg, topo.host, [[0, 1], [1, 2], [2, 3]], Bt=0x7FFFFFFF, ws_bytes=2 ** 62) == EINVAL     # more workgroups than a launch takes
    # a short workspace: one byte less than the query asks for
    assert lib.gns_acn2_workspace_bytes(ctypes.byref(cfg), d, 1, 2, ctypes.byref(need)) == 0
    assert _screen(lib, cfg, topo.host, [[0, 3], [3, 0]], ws_bytes=need.value - 1) == ESIZE
    assert _screen(lib, cfg, topo.host, [[0, 3], [3, 3]], ws_bytes=need.value - 1) == EINVAL      # GNS_EINVAL wins


def test_lds_refusal_is_newton_raphsons():
    lib = amd.load_library()
    tp = pt.path(4096)
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert topo.info['lds_bytes'] > pt.LDS_LIMIT
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
    need = ctypes.c_size_t(0)
    assert lib.gns_acn2_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 1, 1, ctypes.byref(need)) == 0
    assert _screen(lib, cfg, topo.host, [[0, 1]], ws_bytes=need.value) == EUNSUPPORTED
    assert _screen(lib, cfg, topo.host, [[0, 1]], ws_bytes=need.value - 1) == ESIZE               # GNS_ESIZE wins, as in gns_acn1_screen
    assert _screen(lib, cfg, topo.host, [[0, tp.f.size]], ws_bytes=need.value) == EINVAL
    with pytest.raises(amd.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_acn2_screen', topo.info['lds_bytes'], powerflow._ACN2.formula)
    assert 'nnz(L+U) + dim + 8 N' in str(e.value)


# ---- the eight entries of a pair in numpy, from the blob's own pattern and stamp lists: what gns_acn2_kernel holds in registers

def pair_entries(w, bus, line, j, k):
    """[(row, column, CSR position, value)] x 8: ff, tt, ft, tf of the lower line, then of the higher, each value the sum of the
    entry's stamps in their order with the stamps of both lines skipped (gns_acn1_device.h, acn_entry_without)."""
    N, E, nnzy = int(w[H['N']]), int(w[H['E']]), int(w[H['NNZY']])
    y_ptr, y_col, y_diag = _arr(w, 'Y_PTR', N + 1), _arr(w, 'Y_COL', nnzy), _arr(w, 'Y_DIAG', N)
    st_ptr, st = _arr(w, 'ST_PTR', nnzy + 1), _arr(w, 'ST', 4 * E)
    f, t, yff, ytt, yft, ytf = aref.line_admittances(line)
    kinds = (yff, ytt, yft, ytf)

    def find(i, c):
        p = y_ptr[i] + int(np.searchsorted(y_col[y_ptr[i]:y_ptr[i + 1]], c))
        assert p < y_ptr[i + 1] and y_col[p] == c
        return int(p)

    out = []
    for e in sorted((j, k)):
        for i, c in ((f[e], f[e]), (t[e], t[e]), (f[e], t[e]), (t[e], f[e])):
            p = int(y_diag[i]) if i == c else find(i, c)
            val = complex(bus[i, 4], bus[i, 5]) if p == y_diag[i] else 0j
            for q in range(st_ptr[p], st_ptr[p + 1]):
                if (int(st[q]) >> 2) not in (j, k):
                    val += kinds[int(st[q]) & 3][int(st[q]) >> 2]
            out.append((int(i), int(c), p, val))
    return out


@pytest.mark.parametrize('name', ['case14', 'toy_parallel_selfloop'])
def test_the_eight_entries_are_the_ybus_without_both_lines(name):
    """Every pair, given in both orders: the eight entries against the dense Y-bus with both lines' stamps skipped and against the
    Y-bus of the grid with both rows deleted, at 1e-12 relative; copies of a shared entry are equal; no other entry changes."""
    tp = _case14() if name == 'case14' else toy()
    buses, lines, gens, _, _ = pt.grids(tp, 'wide', 1, 0)
    bus, line = buses[0].double().numpy(), lines[0].double().numpy()
    w = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host
    base = n2ref.ybus_skipping(bus, line)
    assert np.max(np.abs(base - nr.ybus(bus, line).toarray())) <= 1e-12 * max(1.0, float(np.abs(base).max()))
    E = tp.f.size
    ends = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    seen = dict(parallel=0, shared_bus=0, loop_at_bus=0, loop_elsewhere=0, zero_in_pattern=0)
    for j, k in powerflow._pair_list(None, E, 'ac_contingency_screen').tolist():
        want = n2ref.ybus_skipping(bus, line, (j, k))
        deleted = nr.ybus(bus, np.delete(line, [j, k], axis=0)).toarray()
        scale = max(1.0, float(np.abs(want).max()))
        assert np.max(np.abs(want - deleted)) <= 1e-12 * scale, (name, j, k)
        got = pair_entries(w, bus, line, j, k)
        assert [x[3] for x in got] == [x[3] for x in pair_entries(w, bus, line, k, j)]                  # either order: the same bits
        assert len(got) == 8
        touched = np.zeros_like(base, dtype=bool)
        by_pos = {}
        for i, c, p, val in got:
            assert abs(val - want[i, c]) <= 1e-12 * scale, (name, j, k, i, c)
            assert by_pos.setdefault(p, val) == val, (name, j, k, p)                                    # copies of a shared entry agree
            touched[i, c] = True
        assert np.array_equal(want[~touched], base[~touched]), (name, j, k)                             # nothing else changes
        assert not np.any((deleted != 0) & (base == 0))                                                # the pair adds no entry
        a, b = ends[j], ends[k]
        loops = [e for e in (j, k) if ends[e][0] == ends[e][1]]
        seen['parallel'] += a == b and a[0] != a[1]
        seen['shared_bus'] += a != b and bool(set(a) & set(b)) and not loops
        seen['loop_at_bus'] += len(loops) == 1 and bool(set(a) & set(b))
        seen['loop_elsewhere'] += len(loops) == 1 and not set(a) & set(b)
        seen['zero_in_pattern'] += any(val == 0 and base[i, c] != 0 for i, c, _, val in got)
        if a == b and a[0] != a[1]:
            assert len(by_pos) == 4                                                                    # all four entries are shared
        if loops:
            assert len({p for (i, c, p, _), e in zip(got, np.repeat(sorted((j, k)), 4)) if e == loops[0]}) == 1
    print(name, seen)
    assert seen['shared_bus'] > 0
    if name != 'case14':
        assert all(v > 0 for v in seen.values()), seen


def test_reference_rows_are_solutions_of_the_grid_without_both_lines():
    """The reference's own rows on case14: None exactly on the islanding pairs, zero flows at both lines, power balance at every bus
    whose equations the power flow solves."""
    buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 1, seed=0)
    b, l, g = (x[0].double().numpy() for x in (buses, lines, gens))
    f, t, _ = synth.case_topology(14)
    every = powerflow._pair_list(None, f.size, 'ac_contingency_screen')
    isl = powerflow._pair_islanding(14, f - 1, t - 1, every)
    _, pv, pq = nr.roles(b, g, slack)
    v0, th0, conv, _, _ = aref.base_case(b, l, g, slack, tol=1e-12)
    assert conv
    n_checked = 0
    for (j, k), island in list(zip(every.tolist(), isl.tolist()))[::7]:
        row = n2ref.pair(b, l, g, slack, j, k, v0, th0, tol=1e-12)
        assert (row is None) == island, (j, k)
        if row is None or not row.converged:
            continue
        for x in (row.p_from, row.q_from, row.p_to, row.q_to):
            assert x[j] == x[k] == 0.0
        pf, qf, pt_, qt = row.p_from, row.q_from, row.p_to, row.q_to
        V = row.v * np.exp(1j * row.theta)
        s = np.zeros(14, dtype=np.complex128)
        np.add.at(s, f - 1, pf + 1j * qf)
        np.add.at(s, t - 1, pt_ + 1j * qt)
        bal = s + np.abs(V) ** 2 * np.conj(b[:, 4] + 1j * b[:, 5]) - nr.specified(b, g)
        assert np.max(np.abs(bal.real[np.r_[pv, pq]])) <= 1e-10 and np.max(np.abs(bal.imag[pq])) <= 1e-10, (j, k)
        n_checked += 1
    assert n_checked >= 8, n_checked


# ---- the pair lists of the row-level tests (ac_n2_pairs.rows_pairs) and one Newton step of the replay on each of them

def test_the_lists_of_the_row_tests():
    fam = pt.families()
    for tp in (toy(), fam['random40_parallel_selfloop'], fam['lattice16x16'], pt.ring_slack_without_generator(64), pt.wheel(71)):
        E = tp.f.size
        pairs = rows_pairs(tp)
        assert pairs == rows_pairs(tp) and len(set(pairs)) == len(pairs) == min(128, E * (E - 1) // 2), tp.name
        assert all(0 <= j < k < E for j, k in pairs), tp.name
        if E * (E - 1) // 2 > 128:
            kinds = pair_kinds(tp)
            n_kinds = len(set(kinds.values()))
            assert sorted(kinds[p] for p in pairs[:n_kinds]) == sorted(set(kinds.values())), tp.name
            edge = [e for e in (0, 62, 63, 64, 65, E - 1) if e < E]
            assert {(j, k) for j in edge for k in edge if j < k} <= set(pairs), tp.name
        isl = rows_islanding(tp, pairs)
        assert 0 < int((~isl).sum()), tp.name
    assert len(rows_pairs(toy())) == 21


@pytest.mark.parametrize('regime', pt.REGIMES)
def test_one_step_of_the_replay_on_every_listed_pair(regime):
    """``test_ac_contingency_host.test_one_step_of_the_replay_on_every_pair`` for double outages, from a start with
    base_theta[slack] = 0.3, on EVERY non-islanding pair of ``rows_pairs`` (no convergence needed): after zero steps the replay's
    state is the reference start bit for bit; after one its update solves the reference Jacobian of the grid with both rows deleted
    to ``pt.STEP_TOL``, scipy's own step asserted first as the guard.  Pins "the base blob serves every pair" at 100 %.
    Non-islanding rows of two grids, in either regime: toy 30 (of 42), random40 188, random24_stacked_gens 196, ring63 128 (of 256
    each)."""
    fam = pt.families()
    topos = [toy(), fam['random40_parallel_selfloop'], fam['random24_stacked_gens'], pt.ring_slack_without_generator(63)]
    for tp in topos:
        buses, lines, gens, v, theta = pt.grids(tp, regime, 2, seed=11)
        base_v, base_theta = shifted_base(tp, v, theta)
        w = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host
        pairs = rows_pairs(tp)
        isl = rows_islanding(tp, pairs)
        n_cmp, worst = 0, 0.0
        for i in range(2):
            b, l, g = (x[i].double().numpy() for x in (buses, lines, gens))
            assert base_theta[i, tp.slack - 1] == 0.3
            vm0, va0 = nr.start(b, g, tp.slack, base_v[i], base_theta[i])
            for (j, k), island in zip(pairs, isl):
                if island:
                    continue
                z = emulate_row(w, b, l, g, [j, k], base_v[i], base_theta[i], tol=0.0, max_iter=0)
                assert np.array_equal(z[0], vm0) and np.array_equal(z[1], va0) and z[3] == 0, (tp.name, i, j, k)
                v1, th1, conv, it, _ = emulate_row(w, b, l, g, [j, k], base_v[i], base_theta[i], tol=0.0, max_iter=1)
                assert it == 1 and not conv, (tp.name, i, j, k)
                r_scipy, r_replay = one_step_ratios(b, l, g, tp.slack, [j, k], vm0, va0, v1, th1)
                assert r_scipy <= pt.STEP_TOL, (tp.name, regime, i, j, k, r_scipy)
                assert r_replay <= pt.STEP_TOL, (tp.name, regime, i, j, k, r_replay)
                worst = max(worst, r_replay)
                n_cmp += 1
        n_rows = 2 * int((~isl).sum())
        print(f'{tp.name} ({regime}): {n_cmp} of {n_rows} non-islanding rows compared, worst one-step ratio {worst:.1e}')
        assert n_cmp == n_rows > 0
