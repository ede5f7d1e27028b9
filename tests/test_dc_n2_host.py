"""CPU checks of the DC N-2 contingency screen's host side (include/gns_powerflow.h, "DC N-2 contingency screening"): the Python
argument refusals, the host's pair-islanding function against brute force, the exports, the argument checks of the C entry points
and their order, the LDS image and the workspace formula, and the two kernels' algorithm replayed in numpy on the fast-decoupled
blob (z_c by the blob's solve program as one lane runs it, H, the 2x2 formulas) against the direct reference
(``dc_n2_reference.pair_flows``: both lines removed and the grid solved again).

The bar is the project's DC bar per (grid, pair): max|out - ref| <= 1e-9 max(1, max|ref|).  No pair is left out."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
import dc_n2_reference as n2ref
import pf_topologies as pt
from test_dc_contingency_host import _lane_solve
from test_dcpf_host import _factor, _line_b, _shifted, emulate_solve
from test_fdpf_host import FH, _arr, _programs
from test_powerflow_programs_host import TOPOLOGIES

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
TOL = 1e-9
# islanding pairs / pairs in which neither line is a bridge, of every pair j < k
ISLANDING = {'case14': (27, 8), 'case30': (208, 18), 'case118': (3554, 44), 'case300': (31418, 138),
             'ring30_slack_no_gen': (211, 211), 'lattice8x8': (4, 4), 'star65_pv': (2016, 0), 'path65': (2016, 0)}


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _cfg(tp):
    return PfConfig(tp.n, tp.f.size, tp.g.size, 0, 0.0)


# ---- the Python argument checks (refused before a device is needed)

def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 3)
    E = lines.shape[1]

    def screen(**kw):
        return powerflow.dc_n2_contingency_screen(buses, lines, gens, slack_bus=1, **kw)

    for bad in ([0, 1], [[0, 1, 2]], torch.zeros(2, 3, dtype=torch.int64), np.zeros((1, 2, 2), dtype=np.int64), [[0], [1]]):
        with pytest.raises(ValueError, match=r'pairs must be a \[P,2\]'):
            screen(pairs=bad)
    for bad in ([], torch.zeros(0, 2, dtype=torch.int64), np.zeros((0, 2), dtype=np.int32)):
        with pytest.raises(ValueError, match='pairs is empty'):
            screen(pairs=bad)
    for bad in ([[0.0, 1.0]], [[1.5, 2]], torch.tensor([[1.0, 2.0]]), np.array([[True, False]])):
        with pytest.raises(ValueError, match='pairs must hold integers'):
            screen(pairs=bad)
    for bad in ([[0, E]], [[-1, 2]], [[0, 1], [E + 5, 0]], torch.tensor([[0, E]])):
        with pytest.raises(ValueError, match='pairs must lie in'):
            screen(pairs=bad)
    for bad in ([[3, 3]], [[0, 1], [5, 5]], torch.tensor([[E - 1, E - 1]])):
        with pytest.raises(ValueError, match='pairs must name two different lines'):
            screen(pairs=bad)
    with pytest.raises(ValueError, match='has no pair of lines'):              # the default on a grid with one line
        tp = pt.families()['pair']
        b1, l1, g1, _, _ = pt.grids(tp, 'reference', 1, 0)
        powerflow.dc_n2_contingency_screen(b1, l1, g1, slack_bus=tp.slack)
    for bad in (torch.zeros(E), -torch.ones(E), torch.full((3, E), float('nan'))):
        with pytest.raises(ValueError, match='rating must be positive and finite'):
            screen(rating=bad)
    for bad in (torch.ones(E - 1), torch.ones(2, E), 1.0):
        with pytest.raises(ValueError, match='rating must be'):
            screen(rating=bad)
    with pytest.raises(ValueError, match='flows must be a bool'):
        screen(flows=1)
    with pytest.raises(ValueError, match='float32'):
        powerflow.dc_n2_contingency_screen(buses.double(), lines, gens, slack_bus=1)
    mixed = lines.clone()
    mixed[1, 0, 1] = 5
    with pytest.raises(ValueError, match='differ across the batch: dc_n2_contingency_screen solves one topology'):
        powerflow._topology_key(buses, mixed, gens, 1, 'dc_n2_contingency_screen')
    # the default list: every j < k in lexicographic order; duplicates and both orders are kept as given
    assert powerflow._pair_list(None, 4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert powerflow._pair_list(None, E).shape == (E * (E - 1) // 2, 2)
    got = powerflow._pair_list(np.array([[4, 1], [1, 4], [4, 1]], dtype=np.int16), 5)
    assert got.dtype == np.int64 and got.tolist() == [[4, 1], [1, 4], [4, 1]]
    assert powerflow.DcN2ContingencyResult._fields == ('base', 'pairs', 'line_flow', 'worst_loading', 'worst_line', 'islanding',
                                                       'converged')
    assert powerflow._DCN2.prefix == 'gns_dcn2' and powerflow._DCN2.formula == powerflow._DCN2_LDS_FORMULA


# ---- islanding of a pair, on the host

def _brute_force(tp, pairs):
    return np.array([n2ref.pair_islands(tp.n, tp.f, tp.t, tp.slack, j, k) for j, k in pairs.tolist()])


@pytest.mark.parametrize('name', ['case14', 'case30', 'random24_stacked_gens', 'random40_parallel_selfloop', 'ring30_slack_no_gen',
                                  'lattice8x8'])
def test_pair_islanding_equals_brute_force(name):
    tp = TOPOLOGIES[name]
    E = tp.f.size
    pairs = powerflow._pair_list(None, E)
    got = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    assert got.dtype == np.bool_ and got.shape == (pairs.shape[0],)
    assert np.array_equal(got, _brute_force(tp, pairs)), name
    # symmetric in the two lines; any order and duplicates of the list give the same answers
    assert np.array_equal(powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs[:, ::-1]), got)
    perm = np.random.default_rng(E).permutation(pairs.shape[0])
    twice = np.concatenate([perm, perm[:7]])
    assert np.array_equal(powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs[twice]), got[twice])


@pytest.mark.parametrize('name', sorted(ISLANDING))
def test_pair_islanding_counts(name):
    tp = TOPOLOGIES[name]
    pairs = powerflow._pair_list(None, tp.f.size)
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    got = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    neither = got & ~bridges[pairs[:, 0]] & ~bridges[pairs[:, 1]]
    assert (int(got.sum()), int(neither.sum())) == ISLANDING[name]
    assert bool(got[bridges[pairs[:, 0]] | bridges[pairs[:, 1]]].all())
    assert pairs.shape[0] == {'case14': 190, 'case30': 820, 'case118': 17205, 'case300': 84255, 'ring30_slack_no_gen': 465,
                              'lattice8x8': 6216, 'star65_pv': 2016, 'path65': 2016}[name]


def test_pair_islanding_with_parallel_lines_and_self_loops_and_its_cache():
    # 1 - 2 = 3 - 4, 4 - 4: a doubled line (1, 2), two bridges (0, 3), a self-loop (4)
    f, t = np.array([0, 1, 1, 2, 3]), np.array([1, 2, 2, 3, 3])
    pairs = powerflow._pair_list(None, 5)
    got = dict(zip(map(tuple, pairs.tolist()), powerflow._pair_islanding(4, f, t, pairs).tolist()))
    assert got[(1, 2)] is True                           # both parallel lines: neither a bridge, together they island
    assert got[(1, 4)] is False and got[(2, 4)] is False  # a parallel line and the self-loop
    assert all(v for (j, k), v in got.items() if j in (0, 3) or k in (0, 3))
    tp = pt.Topo('toy', 4, f + 1, t + 1, np.array([1]), 1)
    assert np.array_equal(_brute_force(tp, pairs), np.array(list(got.values())))
    # the cache lives with the topology: one search per distinct lower line that is not a bridge, none the second time
    tp = TOPOLOGIES['case30']
    topo = _fd(tp)
    args = (tp.n, tp.f.astype(np.float64), tp.t.astype(np.float64))
    pairs = powerflow._pair_list(None, tp.f.size)
    first = powerflow._topology_pair_islanding(topo, args, pairs)
    bridges = powerflow._topology_bridges(topo, args)
    assert sorted(topo.bridges_without) == [j for j in range(tp.f.size - 1) if not bridges[j]]
    rows = {j: id(r) for j, r in topo.bridges_without.items()}
    again = powerflow._topology_pair_islanding(topo, args, pairs[::-1, ::-1].copy())
    assert np.array_equal(again, first[::-1]) and {j: id(r) for j, r in topo.bridges_without.items()} == rows
    assert int(first.sum()) == 208


# ---- the C entry points

def test_exports_are_there_and_disjoint():
    lib = amd.load_library()
    assert _lib.DCN2_EXPORTS == ('gns_dcn2_lds_bytes', 'gns_dcn2_workspace_bytes', 'gns_dcn2_screen')
    others = (_lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.ACN1_EXPORTS +
              _lib.ACN1_ADJOINT_EXPORTS)
    for f in _lib.DCN2_EXPORTS:
        assert hasattr(lib, f), f
        assert f not in others
        assert getattr(lib, f).restype is ctypes.c_int
    assert _lib.DCN1_EXPORTS == ('gns_dcn1_lds_bytes', 'gns_dcn1_workspace_bytes', 'gns_dcn1_screen', 'gns_dcn1_adjoint_lds_bytes',
                                 'gns_dcn1_adjoint_workspace_bytes', 'gns_dcn1_adjoint')
    assert callable(powerflow.dc_n2_contingency_screen)


def _screen(lib, cfg, blob, cand, cols, **kw):
    """gns_dcn2_screen on dummy (never dereferenced) device pointers; a keyword replaces one argument."""
    d = blob.ctypes.data
    c = np.asarray(cand, dtype=np.int32)
    p = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).reshape(-1, 2))
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, cand_host=c.ctypes.data,
             cand_dev=d, n_cand=c.size, cols_host=p.ctypes.data, cols_dev=d, P=p.shape[0], isl=d, rating=None, per_grid=0, flow=None,
             worst=d, worst_line=d, conv=d, ws=d, ws_bytes=1 << 40)
    a.update(kw)
    return lib.gns_dcn2_screen(a['cfg'], a['host'], a['dev'], a['buses'], a['lines'], a['gens'], a['Bt'], a['cand_host'], a['cand_dev'],
                               a['n_cand'], a['cols_host'], a['cols_dev'], a['P'], a['isl'], a['rating'], a['per_grid'], a['flow'],
                               a['worst'], a['worst_line'], a['conv'], a['ws'], a['ws_bytes'], None)


def _ws_bytes(Bt, n_cand, E):
    return (8 * Bt * (n_cand * E + 2 * E + n_cand + 1) + 255) // 256 * 256


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host: nothing is launched, so the test needs no device."""
    lib = amd.load_library()
    tp = TOPOLOGIES['case14']
    fd, cfg = _fd(tp), _cfg(tp)
    E = tp.f.size
    need = ctypes.c_size_t(123)
    d = fd.host.ctypes.data
    # the workspace: Bt * (n_cand * E + 2 E + n_cand + 1) doubles, rounded up to 256 bytes
    for Bt, n_cand in ((1, 2), (4, E), (7, 5), (512, 3)):
        assert lib.gns_dcn2_workspace_bytes(ctypes.byref(cfg), d, Bt, n_cand, ctypes.byref(need)) == 0
        assert need.value == _ws_bytes(Bt, n_cand, E) and need.value % 256 == 0
    for args in ((None, d, 4, E, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, None), (ctypes.byref(cfg), d, 0, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, -3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E + 1, ctypes.byref(need))):
        assert lib.gns_dcn2_workspace_bytes(*args) == EINVAL, args
    cand, cols = [0, 3, 7], [[0, 1], [2, 0]]
    # null arguments (line_flow and rating may be NULL: they are in every call here)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'cand_host', 'cand_dev', 'cols_host', 'cols_dev', 'isl', 'worst',
                 'worst_line', 'conv', 'ws'):
        assert _screen(lib, None if name == 'cfg' else cfg, fd.host, cand, cols, **({} if name == 'cfg' else {name: None})) == EINVAL, name
    # wrong shapes
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 0, 0.0), PfConfig(tp.n, E + 1, tp.g.size, 0, 0.0),
                PfConfig(tp.n, E, tp.g.size + 1, 0, 0.0)):
        assert _screen(lib, bad, fd.host, cand, cols) == EINVAL
        assert lib.gns_dcn2_workspace_bytes(ctypes.byref(bad), d, 4, E, ctypes.byref(need)) == EINVAL
    assert _screen(lib, cfg, fd.host, cand, cols, Bt=0) == EINVAL and _screen(lib, cfg, fd.host, cand, cols, Bt=-1) == EINVAL
    assert _screen(lib, cfg, fd.host, cand, cols, per_grid=2) == EINVAL
    assert _screen(lib, cfg, fd.host, cand, cols, Bt=2 ** 31) == EINVAL                      # counts above 2^31 - 1
    assert _screen(lib, cfg, fd.host, cand, [[0, 1]] * 9, Bt=0x7FFFFFFF) == EINVAL            # more workgroups than one launch takes
    # a Newton-Raphson blob where an FD blob is expected
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert _screen(lib, cfg, nr.host, cand, cols) == EINVAL
    assert lib.gns_dcn2_workspace_bytes(ctypes.byref(cfg), nr.host.ctypes.data, 4, E, ctypes.byref(need)) == EINVAL
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    assert lib.gns_dcn2_lds_bytes(nr.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn2_lds_bytes(None, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn2_lds_bytes(d, None, ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn2_lds_bytes(d, ctypes.byref(lds), None) == 0
    # candidates: in range, ascending, distinct
    for bad in ([0, E], [-1, 2], [3, 0, 7], [0, 3, 3], [0, 3, 2 ** 31 - 1]):
        assert _screen(lib, cfg, fd.host, bad, [[0, 1]]) == EINVAL, bad
    assert _screen(lib, cfg, fd.host, cand, cols, n_cand=0) == EINVAL and _screen(lib, cfg, fd.host, cand, cols, n_cand=-1) == EINVAL
    # pairs: both columns positions into cand, and different
    for bad in ([[0, 3]], [[-1, 0]], [[0, 1], [1, 1]], [[2, 2]], [[0, 1], [2, 0], [1, 2 ** 31 - 1]]):
        assert _screen(lib, cfg, fd.host, cand, bad) == EINVAL, bad
    assert _screen(lib, cfg, fd.host, cand, cols, P=0) == EINVAL and _screen(lib, cfg, fd.host, cand, cols, P=-1) == EINVAL
    # a short workspace: GNS_ESIZE, after every GNS_EINVAL
    want = _ws_bytes(3, 3, E)
    assert _screen(lib, cfg, fd.host, cand, cols, Bt=3, ws_bytes=want - 1) == ESIZE
    assert _screen(lib, cfg, fd.host, cand, cols, Bt=3, ws_bytes=0) == ESIZE
    assert _screen(lib, cfg, fd.host, cand, [[1, 1]], Bt=3, ws_bytes=0) == EINVAL
    assert _screen(lib, cfg, fd.host, [3, 0], [[0, 1]], Bt=3, ws_bytes=0) == EINVAL


def test_lds_image_workspace_and_refusal():
    lib = amd.load_library()
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    lds1, lanes1 = ctypes.c_int64(), ctypes.c_int32()
    need = ctypes.c_size_t()
    for name in ('case14', 'case30', 'case118', 'case300', 'lattice16x16', 'complete33', 'star200_pq'):
        tp = TOPOLOGIES[name]
        fd = _fd(tp)
        assert lib.gns_dcn2_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == 0
        assert lib.gns_dcn1_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds1), ctypes.byref(lanes1)) == 0
        assert (lds.value, lanes.value) == (lds1.value, lanes1.value) == powerflow._dcn1_lds_bytes(fd.host), name
        assert lds.value <= pt.LDS_LIMIT and 24 * tp.f.size <= lds.value              # the pair kernel's image is the smaller one
        E = tp.f.size
        cfg = _cfg(tp)
        assert lib.gns_dcn2_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, E, ctypes.byref(need)) == 0
        assert need.value == _ws_bytes(3, E, E)
    # path(6000): the image of one candidate at a time is above the limit already
    tp = pt.path(6000)
    fd = _fd(tp)
    want = 8 * (fd.info['nnz_lu_p'] + fd.info['dim_p'] + fd.info['n_bus'] + 3 * fd.info['n_line'] + fd.info['dim_p'] * 2)
    assert powerflow._dcn1_lds_bytes(fd.host) == (want, 1) and want > pt.LDS_LIMIT
    assert _screen(lib, _cfg(tp), fd.host, [0, 1], [[0, 1]]) == EUNSUPPORTED
    assert _screen(lib, _cfg(tp), fd.host, [0, 1], [[0, 1]], ws_bytes=0) == EUNSUPPORTED      # before the workspace is looked at
    assert _screen(lib, _cfg(tp), fd.host, [0, tp.f.size], [[0, 1]]) == EINVAL                 # GNS_EINVAL wins
    assert _screen(lib, _cfg(tp), fd.host, [0, 1], [[1, 1]]) == EINVAL
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcn2_screen', lambda: powerflow._dcn1_lds_bytes(fd.host)[0], powerflow._DCN2.formula)
    assert str(want) in str(e.value) and 'dim_p (W + 1)' in str(e.value) and 'W = 1' in str(e.value)


# ---- the two kernels' algorithm in numpy on the FD blob: what gns_dcn2.hip does, operation for operation but for the order of sums

def emulate_factor(w, bus, line, gen, cand):
    """(H [n_cand, E], base flow [E], b [E]): the factor kernel's workspace of one grid."""
    N = w[FH['N']]
    p_idx = _arr(w, 'P_IDX', N)
    _, flow, _ = emulate_solve(w, bus, line, gen)
    F, nnz1 = _factor(w, line)
    ops = _programs(w)['s1'][1]
    f, t = line[:, 0].astype(int) - 1, line[:, 1].astype(int) - 1
    H = np.zeros((len(cand), line.shape[0]))
    for c, e in enumerate(cand):
        Fk = F.copy()
        Fk[nnz1:] = 0.0
        pf, pt_ = p_idx[f[e]], p_idx[t[e]]
        if pf != pt_:
            if pf >= 0:
                Fk[nnz1 + pf] = 1.0
            if pt_ >= 0:
                Fk[nnz1 + pt_] = -1.0
        _lane_solve(Fk, nnz1, ops)
        z = np.array([Fk[nnz1 + p_idx[i]] if p_idx[i] >= 0 else 0.0 for i in range(N)])
        H[c] = z[f] - z[t]
    return H, flow, _line_b(line)


def emulate_pair(H, F, b, cand, cj, ck):
    """The pair kernel's row: the lower line first, the six scalars, then a line at a time."""
    if cj > ck:
        cj, ck = ck, cj
    ej, ek = cand[cj], cand[ck]
    m11, m12 = 1.0 - b[ej] * H[cj, ej], 0.0 - b[ej] * H[ck, ej]
    m21, m22 = 0.0 - b[ek] * H[cj, ek], 1.0 - b[ek] * H[ck, ek]
    det = m11 * m22 - m12 * m21
    a_j = (F[ej] * m22 - m12 * F[ek]) / det
    a_k = (m11 * F[ek] - m21 * F[ej]) / det
    out = F + b * (H[cj] * a_j + H[ck] * a_k)
    out[[ej, ek]] = 0.0
    return out, det


def test_the_fd_blob_serves_the_n2_screen_on_case14():
    """Every pair of case14, islanding ones included, on two grids with shifts that matter."""
    tp = TOPOLOGIES['case14']
    E = tp.f.size
    buses, lines, gens = synth.synth_grids(14, 2, seed=0)
    lines = _shifted(lines, seed=14)
    w = _fd(tp).host
    pairs = powerflow._pair_list(None, E)
    isl = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    cand, cols = np.unique(pairs, return_inverse=True)
    cols = cols.reshape(-1, 2)
    assert cand.tolist() == list(range(E))
    worst, min_det = 0.0, np.inf
    for i in range(2):
        bus, line, gen = (x[i].double().numpy() for x in (buses, lines, gens))
        H, F, b = emulate_factor(w, bus, line, gen, cand.tolist())
        for p, (j, k) in enumerate(pairs.tolist()):
            want = n2ref.pair_flows(bus, line, gen, tp.slack, j, k)
            assert (want is None) == bool(isl[p]), (i, j, k)
            if want is None:
                continue
            got, det = emulate_pair(H, F, b, cand, cols[p, 0], cols[p, 1])
            swapped, _ = emulate_pair(H, F, b, cand, cols[p, 1], cols[p, 0])
            assert np.array_equal(got, swapped)
            err, scale = float(np.max(np.abs(got - want.numpy()))), max(1.0, float(want.abs().max()))
            worst, min_det = max(worst, err / scale), min(min_det, abs(det))
            assert err <= TOL * scale, (i, j, k, err, scale)
            assert got[j] == 0.0 and got[k] == 0.0
    print(f'case14: 190 pairs ({int(isl.sum())} islanding), worst scaled error {worst:.2e}, smallest |det| {min_det:.2e}')
    assert int(isl.sum()) == 27


def test_the_two_references_agree_on_case14():
    """``dense_rank2`` against ``pair_flows`` to 1e-10, every non-islanding pair: the probe the GPU test's families are held to."""
    tp = TOPOLOGIES['case14']
    buses, lines, gens = synth.synth_grids(14, 1, seed=3)
    bus, line, gen = (x[0].double() for x in (buses, _shifted(lines, seed=2), gens))
    for j, k in powerflow._pair_list(None, tp.f.size).tolist():
        want = n2ref.pair_flows(bus, line, gen, tp.slack, j, k)
        if want is None:
            continue
        got, det = n2ref.dense_rank2(bus, line, gen, tp.slack, j, k)
        assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())) and abs(det) > 1e-3, (j, k)
