"""CPU checks of the DC generator contingency screen's host side (include/gns_powerflow.h, "DC generator contingency screening"):
the Python argument refusals, the default list, the islanding mask against the reference's graph search, the exports, the argument
checks of the C entry points and their order, the LDS image and the workspace formula, and the two kernels' algorithm replayed in
numpy on the fast-decoupled blob (u_g and z_k by the blob's solve program as one lane runs it, then the row formulas) against the
direct reference (``dc_generator_contingency_reference.direct``: the generators redispatched, the line removed and the grid solved
again).

The bar is the project's DC bar per (grid, row): max|out - ref| <= 1e-9 max(1, max|ref|).  No row is left out."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
import dc_contingency_reference as cref
import dc_generator_contingency_reference as gref
import pf_topologies as pt
from test_dc_contingency_host import _lane_solve
from test_dcpf_host import _factor, _line_b, _shifted, emulate_solve
from test_fdpf_host import FH, _arr, _programs
from test_powerflow_programs_host import TOPOLOGIES

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
TOL = 1e-9
# islanding rows / rows of the default list: Gn bridges of Gn (E + 1)
ISLANDING = {'case14': (5, 105), 'case30': (30, 252), 'case118': (1080, 10098), 'random24_stacked_gens': (40, 312),
             'ring30_slack_no_gen': (0, 96), 'lattice8x8': (0, 1469), 'path65': (64, 65), 'path66_pv1': (130, 132)}


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _cfg(tp):
    return PfConfig(tp.n, tp.f.size, tp.g.size, 0, 0.0)


# ---- the Python argument checks (refused before a device is needed)

def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 3)
    E, Gn = lines.shape[1], gens.shape[1]

    def screen(**kw):
        return powerflow.dc_generator_contingency_screen(buses, lines, gens, slack_bus=1, **kw)

    for bad in ([0, 1], [[0, 1, 2]], torch.zeros(2, 3, dtype=torch.int64), np.zeros((1, 2, 2), dtype=np.int64), [[0], [1]]):
        with pytest.raises(ValueError, match=r'contingencies must be a \[P,2\]'):
            screen(contingencies=bad)
    for bad in ([], torch.zeros(0, 2, dtype=torch.int64), np.zeros((0, 2), dtype=np.int32)):
        with pytest.raises(ValueError, match='contingencies is empty'):
            screen(contingencies=bad)
    for bad in ([[0.0, 1.0]], [[1.5, 2]], torch.tensor([[1.0, 2.0]]), np.array([[True, False]])):
        with pytest.raises(ValueError, match='contingencies must hold integers'):
            screen(contingencies=bad)
    for bad in ([[Gn, 0]], [[-1, 2]], [[0, 1], [Gn + 5, -1]], torch.tensor([[Gn, -1]])):
        with pytest.raises(ValueError, match='contingencies must name generators in'):
            screen(contingencies=bad)
    for bad in ([[0, E]], [[0, -2]], [[0, 1], [1, E + 5]], torch.tensor([[Gn - 1, E]])):
        with pytest.raises(ValueError, match='contingencies must name lines in'):
            screen(contingencies=bad)
    for bad in (-torch.ones(Gn), torch.full((3, Gn), float('nan')), [float('inf')] * Gn, [1.0] * (Gn - 1) + [-1e-30]):
        with pytest.raises(ValueError, match='pickup must be non-negative and finite'):
            screen(pickup=bad)
    for bad in (torch.ones(Gn - 1), torch.ones(2, Gn), 1.0, torch.ones(3, Gn, 1)):
        with pytest.raises(ValueError, match='pickup must be'):
            screen(pickup=bad)
    for bad in ('pmin', 'PMAX', ''):
        with pytest.raises(ValueError, match="pickup must be None, 'pmax' or weights"):
            screen(pickup=bad)
    for bad in (torch.zeros(E), -torch.ones(E), torch.full((3, E), float('nan'))):
        with pytest.raises(ValueError, match='rating must be positive and finite'):
            screen(rating=bad)
    for bad in (torch.ones(E - 1), torch.ones(2, E), 1.0):
        with pytest.raises(ValueError, match='rating must be'):
            screen(rating=bad)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='flows must be a bool'):
            screen(flows=bad)
    with pytest.raises(ValueError, match='float32'):
        powerflow.dc_generator_contingency_screen(buses.double(), lines, gens, slack_bus=1)
    with pytest.raises(TypeError):                                            # no gradients in this call
        screen(differentiable=True)
    mixed = lines.clone()
    mixed[1, 0, 1] = 5
    with pytest.raises(ValueError, match='differ across the batch: dc_generator_contingency_screen solves one topology'):
        powerflow._topology_key(buses, mixed, gens, 1, 'dc_generator_contingency_screen')
    # a zero weight, 'pmax' and all-zero weights are allowed: checked and converted to float64
    w = powerflow._pickup([0.0, 1.0, 2.0, 0.0, 3.0], gens, False)
    assert w.dtype == torch.float64 and w.tolist() == [0.0, 1.0, 2.0, 0.0, 3.0]
    assert torch.equal(powerflow._pickup('pmax', gens, False), gens[:, :, 1].double())
    assert powerflow._pickup(torch.zeros(3, Gn, dtype=torch.float32), gens, False).shape == (3, Gn)
    assert powerflow._pickup(torch.ones(1, Gn), gens[:1], True).shape == (Gn,) and powerflow._pickup(None, gens, False) is None
    assert powerflow.DcGeneratorContingencyResult._fields == ('base', 'contingencies', 'line_flow', 'worst_loading', 'worst_line',
                                                               'islanding', 'converged')
    assert powerflow._DCG1.prefix == 'gns_dcg1' and powerflow._DCG1.formula == powerflow._DCG1_LDS_FORMULA


def test_the_default_list_and_its_order():
    assert powerflow._generator_contingency_list(None, 2, 3).tolist() == [[0, -1], [0, 0], [0, 1], [0, 2],
                                                                          [1, -1], [1, 0], [1, 1], [1, 2]]
    every = powerflow._generator_contingency_list(None, 54, 186)
    assert every.shape == (54 * 187, 2) == (10098, 2) and every.dtype == np.int64
    assert every[187].tolist() == [1, -1] and every[-1].tolist() == [53, 185]
    # duplicates and any order are kept as given
    got = powerflow._generator_contingency_list(np.array([[4, 1], [0, -1], [4, 1]], dtype=np.int16), 5, 3)
    assert got.dtype == np.int64 and got.tolist() == [[4, 1], [0, -1], [4, 1]]
    got = powerflow._generator_contingency_list(torch.tensor([[0, -1]], dtype=torch.int32), 1, 1)
    assert got.tolist() == [[0, -1]]


@pytest.mark.parametrize('name', sorted(ISLANDING))
def test_islanding_mask_equals_the_reference(name):
    """A generator outage never islands; row (g, k) islands exactly when the graph without line k does."""
    tp = TOPOLOGIES[name] if name in TOPOLOGIES else pt.families()[name]
    E, Gn = tp.f.size, tp.g.size
    rows = powerflow._generator_contingency_list(None, Gn, E)
    got = powerflow._generator_islanding(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1), rows)
    assert got.dtype == np.bool_ and got.shape == (rows.shape[0],)
    without = np.array([cref.islands(tp.n, np.delete(tp.f, k), np.delete(tp.t, k), tp.slack) for k in range(E)])
    assert not cref.islands(tp.n, tp.f, tp.t, tp.slack)
    want = np.array([k >= 0 and bool(without[k]) for _, k in rows.tolist()])
    assert np.array_equal(got, want), name
    assert (int(got.sum()), rows.shape[0]) == ISLANDING[name]
    perm = np.random.default_rng(E).permutation(rows.shape[0])[:50]
    assert np.array_equal(powerflow._generator_islanding(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1), rows[perm]), got[perm])


# ---- the C entry points

def test_exports_are_there_and_disjoint():
    lib = amd.load_library()
    assert _lib.DCG1_EXPORTS == ('gns_dcg1_lds_bytes', 'gns_dcg1_workspace_bytes', 'gns_dcg1_screen')
    others = (_lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.DCN2_EXPORTS +
              _lib.DCN2_ADJOINT_EXPORTS + _lib.ACN1_EXPORTS + _lib.ACN1_ADJOINT_EXPORTS + _lib.ACN2_EXPORTS + _lib.ACN2_ADJOINT_EXPORTS)
    for f in _lib.DCG1_EXPORTS:
        assert hasattr(lib, f), f
        assert f not in others
        assert getattr(lib, f).restype is ctypes.c_int
    assert callable(powerflow.dc_generator_contingency_screen)


def _screen(lib, cfg, blob, line_list, gen_list, cols, **kw):
    """gns_dcg1_screen on dummy (never dereferenced) device pointers; a keyword replaces one argument."""
    d = blob.ctypes.data
    li = np.asarray(line_list, dtype=np.int32)
    ge = np.asarray(gen_list, dtype=np.int32)
    p = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).reshape(-1, 2))
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, line_host=li.ctypes.data,
             line_dev=d, n_line=li.size, gen_host=ge.ctypes.data, gen_dev=d, n_gen=ge.size, cols_host=p.ctypes.data, cols_dev=d,
             P=p.shape[0], isl=d, rating=None, per_grid=0, pickup=None, pickup_per_grid=0, flow=None, worst=d, worst_line=d, conv=d,
             ws=d, ws_bytes=1 << 40)
    a.update(kw)
    return lib.gns_dcg1_screen(a['cfg'], a['host'], a['dev'], a['buses'], a['lines'], a['gens'], a['Bt'], a['line_host'], a['line_dev'],
                               a['n_line'], a['gen_host'], a['gen_dev'], a['n_gen'], a['cols_host'], a['cols_dev'], a['P'], a['isl'],
                               a['rating'], a['per_grid'], a['pickup'], a['pickup_per_grid'], a['flow'], a['worst'], a['worst_line'],
                               a['conv'], a['ws'], a['ws_bytes'], None)


def _ws_bytes(Bt, n_cand, E):
    return (8 * Bt * (n_cand * E + 2 * E + n_cand + 1) + 255) // 256 * 256


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host: nothing is launched, so the test needs no device."""
    lib = amd.load_library()
    tp = TOPOLOGIES['case14']
    fd, cfg = _fd(tp), _cfg(tp)
    E, Gn = tp.f.size, tp.g.size
    need = ctypes.c_size_t(123)
    d = fd.host.ctypes.data
    # the workspace: Bt * (n_cand * E + 2 E + n_cand + 1) doubles with n_cand = n_line + n_gen, rounded up to 256 bytes
    for Bt, n_line, n_gen in ((1, 2, 1), (4, E, Gn), (7, 0, 3), (512, 3, 2)):
        assert lib.gns_dcg1_workspace_bytes(ctypes.byref(cfg), d, Bt, n_line, n_gen, ctypes.byref(need)) == 0
        assert need.value == _ws_bytes(Bt, n_line + n_gen, E) and need.value % 256 == 0
    for args in ((None, d, 4, E, Gn, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, E, Gn, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, Gn, None), (ctypes.byref(cfg), d, 0, E, Gn, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, -1, Gn, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, E, 0, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, -3, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, E + 1, Gn, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, Gn + 1, ctypes.byref(need))):
        assert lib.gns_dcg1_workspace_bytes(*args) == EINVAL, args
    li, ge, cols = [0, 3, 7], [1, 4], [[0, 1], [1, -1], [0, 2]]
    # null arguments (line_flow, rating and pickup may be NULL: they are in every call here)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'line_host', 'line_dev', 'gen_host', 'gen_dev', 'cols_host', 'cols_dev',
                 'isl', 'worst', 'worst_line', 'conv', 'ws'):
        assert _screen(lib, None if name == 'cfg' else cfg, fd.host, li, ge, cols, **({} if name == 'cfg' else {name: None})) == EINVAL, name
    # an empty line list needs no line pointers; its rows then hold -1 alone
    assert _screen(lib, cfg, fd.host, [], ge, [[0, -1], [1, -1]], line_host=None, line_dev=None, ws_bytes=0) == ESIZE
    assert _screen(lib, cfg, fd.host, [], ge, [[0, 0]], line_host=None, line_dev=None) == EINVAL
    # wrong shapes
    for bad in (PfConfig(tp.n + 1, E, Gn, 0, 0.0), PfConfig(tp.n, E + 1, Gn, 0, 0.0), PfConfig(tp.n, E, Gn + 1, 0, 0.0)):
        assert _screen(lib, bad, fd.host, li, ge, cols) == EINVAL
        assert lib.gns_dcg1_workspace_bytes(ctypes.byref(bad), d, 4, E, Gn, ctypes.byref(need)) == EINVAL
    assert _screen(lib, cfg, fd.host, li, ge, cols, Bt=0) == EINVAL and _screen(lib, cfg, fd.host, li, ge, cols, Bt=-1) == EINVAL
    for flag in ('per_grid', 'pickup_per_grid'):
        assert _screen(lib, cfg, fd.host, li, ge, cols, **{flag: 2}) == EINVAL and _screen(lib, cfg, fd.host, li, ge, cols, **{flag: -1}) == EINVAL
    assert _screen(lib, cfg, fd.host, li, ge, cols, Bt=2 ** 31) == EINVAL                    # counts above 2^31 - 1
    assert _screen(lib, cfg, fd.host, li, ge, [[0, 1]] * 9, Bt=0x7FFFFFFF) == EINVAL          # more workgroups than one launch takes
    # a Newton-Raphson blob where an FD blob is expected
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert _screen(lib, cfg, nr.host, li, ge, cols) == EINVAL
    assert lib.gns_dcg1_workspace_bytes(ctypes.byref(cfg), nr.host.ctypes.data, 4, E, Gn, ctypes.byref(need)) == EINVAL
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    assert lib.gns_dcg1_lds_bytes(nr.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcg1_lds_bytes(None, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcg1_lds_bytes(d, None, ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcg1_lds_bytes(d, ctypes.byref(lds), None) == 0
    # both lists: in range, ascending, distinct
    for bad in ([0, E], [-1, 2], [3, 0, 7], [0, 3, 3], [0, 3, 2 ** 31 - 1]):
        assert _screen(lib, cfg, fd.host, bad, ge, [[0, 1]]) == EINVAL, bad
    for bad in ([0, Gn], [-1, 2], [3, 0], [1, 1], [0, 2 ** 31 - 1]):
        assert _screen(lib, cfg, fd.host, li, bad, [[0, 1]]) == EINVAL, bad
    assert _screen(lib, cfg, fd.host, li, ge, cols, n_line=-1) == EINVAL and _screen(lib, cfg, fd.host, li, ge, cols, n_line=E + 1) == EINVAL
    assert _screen(lib, cfg, fd.host, li, ge, cols, n_gen=0) == EINVAL and _screen(lib, cfg, fd.host, li, ge, cols, n_gen=-1) == EINVAL
    # rows: a position into the generators, and a position into the lines or -1
    for bad in ([[2, 0]], [[-1, 0]], [[0, 3]], [[0, -2]], [[0, 1], [1, -1], [1, 2 ** 31 - 1]]):
        assert _screen(lib, cfg, fd.host, li, ge, bad) == EINVAL, bad
    assert _screen(lib, cfg, fd.host, li, ge, cols, P=0) == EINVAL and _screen(lib, cfg, fd.host, li, ge, cols, P=-1) == EINVAL
    # a short workspace: GNS_ESIZE, after every GNS_EINVAL
    want = _ws_bytes(3, 5, E)
    assert _screen(lib, cfg, fd.host, li, ge, cols, Bt=3, ws_bytes=want - 1) == ESIZE
    assert _screen(lib, cfg, fd.host, li, ge, cols, Bt=3, ws_bytes=0) == ESIZE
    assert _screen(lib, cfg, fd.host, li, ge, [[2, 1]], Bt=3, ws_bytes=0) == EINVAL
    assert _screen(lib, cfg, fd.host, [3, 0], ge, [[0, 1]], Bt=3, ws_bytes=0) == EINVAL


def test_lds_image_workspace_and_refusal():
    lib = amd.load_library()
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    lds1, lanes1 = ctypes.c_int64(), ctypes.c_int32()
    need = ctypes.c_size_t()
    for name in ('case14', 'case30', 'case118', 'case300', 'lattice16x16', 'complete33', 'star200_pq', 'hub150_70lines_70gens'):
        tp = TOPOLOGIES[name]
        fd = _fd(tp)
        info = fd.info
        assert lib.gns_dcg1_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == 0
        assert lib.gns_dcn1_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds1), ctypes.byref(lanes1)) == 0
        assert (lds.value, lanes.value) == (lds1.value, lanes1.value) == powerflow._dcn1_lds_bytes(fd.host), name
        W = lanes.value
        assert lds.value == 8 * (info['nnz_lu_p'] + info['dim_p'] + info['n_bus'] + 3 * info['n_line'] + info['dim_p'] * (W + 1))
        assert lds.value <= pt.LDS_LIMIT and 24 * tp.f.size <= lds.value              # the row kernel's image is the smaller one
        E, Gn = tp.f.size, tp.g.size
        cfg = _cfg(tp)
        assert lib.gns_dcg1_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, E, Gn, ctypes.byref(need)) == 0
        assert need.value == _ws_bytes(3, E + Gn, E)
    # path(6000): the image of one candidate at a time is above the limit already
    tp = pt.path(6000)
    fd = _fd(tp)
    want = 8 * (fd.info['nnz_lu_p'] + fd.info['dim_p'] + fd.info['n_bus'] + 3 * fd.info['n_line'] + fd.info['dim_p'] * 2)
    assert powerflow._dcn1_lds_bytes(fd.host) == (want, 1) and want > pt.LDS_LIMIT
    assert _screen(lib, _cfg(tp), fd.host, [0, 1], [0], [[0, 1]]) == EUNSUPPORTED
    assert _screen(lib, _cfg(tp), fd.host, [0, 1], [0], [[0, 1]], ws_bytes=0) == EUNSUPPORTED      # before the workspace is looked at
    assert _screen(lib, _cfg(tp), fd.host, [0, tp.f.size], [0], [[0, 1]]) == EINVAL                 # GNS_EINVAL wins
    assert _screen(lib, _cfg(tp), fd.host, [0, 1], [0], [[1, 1]]) == EINVAL
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcg1_screen', lambda: powerflow._dcn1_lds_bytes(fd.host)[0], powerflow._DCG1.formula)
    assert str(want) in str(e.value) and 'dim_p (W + 1)' in str(e.value) and 'W = 1' in str(e.value)


# ---- the two kernels' algorithm in numpy on the FD blob: what gns_dcg1.hip does, operation for operation

def _solve_column(w, F, nnz1, rhs):
    """One lane's solve of the reduced right-hand side ``rhs`` [dim_p] on the factor F; the solution by bus, 0 at the slack."""
    N = w[FH['N']]
    p_idx = _arr(w, 'P_IDX', N)
    Fk = F.copy()
    Fk[nnz1:] = rhs
    _lane_solve(Fk, nnz1, _programs(w)['s1'][1])
    return np.array([Fk[nnz1 + p_idx[i]] if p_idx[i] >= 0 else 0.0 for i in range(N)])


def emulate_factor(w, bus, line, gen, line_list, gen_list, pickup):
    """(H [n_line, E], D [n_gen, E], base flow [E], b [E]): the factor kernel's workspace of one grid."""
    N, Gn, d1 = w[FH['N']], w[FH['GN']], w[FH['DIM1']]
    p_idx, gen_ptr, gen_idx = _arr(w, 'P_IDX', N), _arr(w, 'GEN_PTR', N + 1), _arr(w, 'GEN_IDX', Gn)
    _, flow, _ = emulate_solve(w, bus, line, gen)
    F, nnz1 = _factor(w, line)
    f, t = line[:, 0].astype(int) - 1, line[:, 1].astype(int) - 1
    H = np.zeros((len(line_list), line.shape[0]))
    for c, e in enumerate(line_list):
        rhs = np.zeros(d1)
        pf, pt_ = p_idx[f[e]], p_idx[t[e]]
        if pf != pt_:
            if pf >= 0:
                rhs[pf] = 1.0
            if pt_ >= 0:
                rhs[pt_] = -1.0
        z = _solve_column(w, F, nnz1, rhs)
        H[c] = z[f] - z[t]
    D = np.zeros((len(gen_list), line.shape[0]))
    for c, gi in enumerate(gen_list):
        rhs = np.zeros(d1)
        pg = gen[gi, 6]
        W = 0.0
        if pickup is not None:
            for h in range(Gn):
                if h != gi:
                    W += pickup[h]
        for i in range(N):                                     # the generators of a bus, in generator-index order
            mine = gen_idx[gen_ptr[i]:gen_ptr[i + 1]].tolist()
            assert mine == sorted(mine)
            if not mine or p_idx[i] < 0:
                continue
            dp, any_ = 0.0, False
            if gi in mine:
                dp, any_ = 0.0 - pg, True
            if W > 0.0:
                for h in mine:
                    if h != gi:
                        dp += pg * (pickup[h] / W)
                        any_ = True
            if any_:
                rhs[p_idx[i]] = dp
        u = _solve_column(w, F, nnz1, rhs)
        D[c] = u[f] - u[t]
    return H, D, flow, _line_b(line)


def emulate_row(H, D, F, b, line_list, cg, ck):
    """The row kernel's row: the flows with the generator out, then the N-1 screen's update with den and alpha."""
    fg = F + b * D[cg]
    if ck < 0:
        return fg, 1.0
    ek = line_list[ck]
    den = 1.0 - b[ek] * H[ck, ek]
    alpha = fg[ek] / den
    out = fg + (b * H[ck]) * alpha
    out[ek] = 0.0
    return out, den


@pytest.mark.parametrize('pickup', [None, 'pmax', 'random'])
def test_the_fd_blob_serves_the_generator_screen_on_case14(pickup):
    """Every default row of case14, islanding ones included, on two grids with shifts that matter."""
    tp = TOPOLOGIES['case14']
    E, Gn = tp.f.size, tp.g.size
    buses, lines, gens = synth.synth_grids(14, 2, seed=0)
    lines = _shifted(lines, seed=14)
    if pickup == 'random':
        pickup = torch.rand(2, Gn, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        pickup[:, 2] = 0.0
    w = _fd(tp).host
    rows = powerflow._generator_contingency_list(None, Gn, E)
    isl = powerflow._generator_islanding(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1), rows)
    worst, min_den = 0.0, np.inf
    for i in range(2):
        bus, line, gen = (x[i].double().numpy() for x in (buses, lines, gens))
        wi = gref.weights(pickup, gen, i)
        H, D, F, b = emulate_factor(w, bus, line, gen, list(range(E)), list(range(Gn)), None if wi is None else wi.numpy())
        for p, (g, k) in enumerate(rows.tolist()):
            want = gref.direct(bus, line, gen, tp.slack, g, k, wi)
            assert (want is None) == bool(isl[p]), (i, g, k)
            if want is None:
                continue
            got, den = emulate_row(H, D, F, b, list(range(E)), g, k)
            err, scale = float(np.max(np.abs(got - want.numpy()))), max(1.0, float(want.abs().max()))
            worst, min_den = max(worst, err / scale), min(min_den, abs(den))
            assert err <= TOL * scale, (i, g, k, err, scale)
            assert k < 0 or got[k] == 0.0
    print(f'case14: 105 rows ({int(isl.sum())} islanding), worst scaled error {worst:.2e}, smallest |den| {min_den:.2e}')
    assert int(isl.sum()) == 5


def test_the_pins_hold_in_the_emulation():
    """Pg_g exactly 0, or a generator on the slack bus with no pickup: the column is zero, row (g, -1) is the base flow and row
    (g, k) the N-1 screen's row k, bit for bit."""
    tp = TOPOLOGIES['case14']
    E, Gn = tp.f.size, tp.g.size
    buses, lines, gens = synth.synth_grids(14, 1, seed=1)
    gens[0, 3, 6] = 0.0
    bus, line, gen = (x[0].double().numpy() for x in (buses, _shifted(lines, seed=3), gens))
    w = _fd(tp).host
    on_slack = int(np.flatnonzero(tp.g == tp.slack)[0])
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    for pickup, zero in ((None, (3, on_slack)), (np.array([1.0, 0.5, 0.0, 2.0, 1.0]), (3,))):
        H, D, F, b = emulate_factor(w, bus, line, gen, list(range(E)), list(range(Gn)), pickup)
        for g in zero:
            assert np.array_equal(emulate_row(H, D, F, b, list(range(E)), g, -1)[0], F)
            for k in np.flatnonzero(~bridges).tolist():
                den = 1.0 - b[k] * H[k, k]
                n1 = F + b * H[k] * (F[k] / den)
                n1[k] = 0.0
                assert np.array_equal(emulate_row(H, D, F, b, list(range(E)), g, k)[0], n1), (g, k)
        assert bool(np.any(D[[g for g in range(Gn) if g not in zero]] != 0.0))


@pytest.mark.parametrize('name', ['case14', 'random24_stacked_gens'])
def test_the_two_references_agree(name):
    """``by_factors`` against ``direct`` to 1e-10, every non-islanding default row: the probe the GPU test's families are held to."""
    tp = TOPOLOGIES[name] if name in TOPOLOGIES else pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, 3)
    bus, line, gen = (x[0].double() for x in (buses, _shifted(lines, seed=2), gens))
    for pickup in (None, 'pmax'):
        wi = gref.weights(pickup, gen)
        for g, k in powerflow._generator_contingency_list(None, tp.g.size, tp.f.size).tolist():
            want = gref.direct(bus, line, gen, tp.slack, g, k, wi)
            if want is None:
                continue
            got, den = gref.by_factors(bus, line, gen, tp.slack, g, k, wi)
            assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())) and abs(den) > 1e-3, (g, k)
