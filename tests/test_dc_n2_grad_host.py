"""The host side of the DC N-2 screen's gradients (``gns_dcn2_adjoint``; include/gns_powerflow.h, "DC N-2 contingency screening",
gradients): the exports, the refusals of the three entry points and their order, the workspace formula, the Python argument
check, and a numpy replay of the kernels' algorithm on the FD blob against the float64 autograd reference
(``dc_n2_grad_reference``) at max|out - ref| <= 1e-9 max(1, max|ref|) per contract column, every other column exactly 0.  No
device is needed: every C call below is refused on the host or has nothing to launch."""
import ctypes

import numpy as np
import pytest

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
import dc_n2_grad_reference as gref
import pf_topologies as pt
from dc_n2_grad_cases import special_pairs
from test_dc_contingency_host import _cfg, _fd, _lane_solve
from test_dcpf_gpu import _perturbed
from test_dcpf_host import _factor, _line_b, _shifted, emulate_solve
from test_fdpf_host import FH, _arr, _programs
from test_powerflow_programs_host import TOPOLOGIES

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
TOL = 1e-9
CONTRACT = {'buses': (2, 4), 'lines': (3, 5, 6), 'generators': (6,)}
NEW = ('gns_dcn2_adjoint_lds_bytes', 'gns_dcn2_adjoint_workspace_bytes', 'gns_dcn2_adjoint')


def test_exports_are_there():
    lib = amd.load_library()
    assert _lib.DCN2_EXPORTS == ('gns_dcn2_lds_bytes', 'gns_dcn2_workspace_bytes', 'gns_dcn2_screen')
    assert _lib.DCN2_ADJOINT_EXPORTS == NEW
    for f in NEW:
        assert hasattr(lib, f) and getattr(lib, f).restype is ctypes.c_int, f
    assert '2 dim_p (W + 1) + 3 W' in powerflow._DCN2_ADJOINT_LDS_FORMULA and '32 E' in powerflow._DCN2_ADJOINT_LDS_FORMULA


def _adjoint(lib, cfg, blob, cand, cols, **kw):
    """gns_dcn2_adjoint on dummy (never dereferenced) device pointers; a keyword replaces one argument."""
    d = blob.ctypes.data
    c = np.asarray(cand, dtype=np.int32)
    p = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).reshape(-1, 2))
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, cand_host=c.ctypes.data,
             cand_dev=d, n_cand=c.size, cols_host=p.ctypes.data, cols_dev=d, P=p.shape[0], isl=d, rating=None, per_grid=0, worst_line=d,
             conv=d, gflow=None, gworst=None, gb=d, gl=d, gg=d, ws=d, ws_bytes=0)
    a.update(kw)
    return lib.gns_dcn2_adjoint(a['cfg'], a['host'], a['dev'], a['buses'], a['lines'], a['gens'], a['Bt'], a['cand_host'], a['cand_dev'],
                                a['n_cand'], a['cols_host'], a['cols_dev'], a['P'], a['isl'], a['rating'], a['per_grid'],
                                a['worst_line'], a['conv'], a['gflow'], a['gworst'], a['gb'], a['gl'], a['gg'], a['ws'], a['ws_bytes'],
                                None)


def _want_bytes(tp, Bt, n_cand, P, lanes):
    """The workspace formula of the header: the forward's block, then T', the records, the pair chunks' partials of gF, gF,
    a count per candidate and the solve kernel's partials as doubles and a byte per grid, each of the two parts rounded up to 256
    bytes."""
    N, E = tp.n, tp.f.size
    Q = 32 if P >= 8192 else 8
    chunks_p, chunks_a = -(-P // Q), -(-(n_cand + 1) // lanes)
    forward = (Bt * 8 * (n_cand * E + 2 * E + n_cand + 1) + 255) // 256 * 256
    own = Bt * 8 * (n_cand * E + 6 * P + chunks_p * (E + 1) + E + n_cand + chunks_a * (N + 2 * E + 1)) + Bt
    return forward + (own + 255) // 256 * 256


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = amd.load_library()
    tp = TOPOLOGIES['case14']
    fd, cfg = _fd(tp), _cfg(tp)
    E = tp.f.size
    need = ctypes.c_size_t(123)
    d = fd.host.ctypes.data
    query = lib.gns_dcn2_adjoint_workspace_bytes
    assert query(ctypes.byref(cfg), d, 4, E, 190, ctypes.byref(need)) == 0 and need.value == _want_bytes(tp, 4, E, 190, 64)
    assert query(ctypes.byref(cfg), d, 3, 7, 9000, ctypes.byref(need)) == 0 and need.value == _want_bytes(tp, 3, 7, 9000, 64)
    tp300 = TOPOLOGIES['case300']
    assert query(ctypes.byref(_cfg(tp300)), _fd(tp300).host.ctypes.data, 2, 41, 60, ctypes.byref(need)) == 0
    assert need.value == _want_bytes(tp300, 2, 41, 60, 16)                            # three chunks of 16 columns
    ok = (ctypes.byref(cfg), d, 4, E, 190, ctypes.byref(need))
    for at, bad in ((0, None), (1, None), (5, None), (2, 0), (3, 0), (3, -3), (3, E + 1), (4, 0), (4, -1), (2, 0x7FFFFFFF)):
        args = list(ok)
        args[at] = bad
        assert query(*args) == EINVAL, (at, bad)
    cand, cols = [0, 3, 5], [[0, 1], [2, 1]]
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'cand_host', 'cand_dev', 'cols_host', 'cols_dev', 'isl', 'worst_line',
                 'conv', 'ws'):
        assert _adjoint(lib, None if name == 'cfg' else cfg, fd.host, cand, cols, **({} if name == 'cfg' else {name: None})) == EINVAL, name
    assert _adjoint(lib, cfg, fd.host, cand, cols) == ESIZE                           # every check passed but the workspace's size
    assert _adjoint(lib, cfg, fd.host, cand, cols, ws_bytes=_want_bytes(tp, 1, 3, 2, 64) - 1) == ESIZE
    assert _adjoint(lib, cfg, fd.host, cand, cols, gb=None, gl=None, gg=None) == 0    # nothing asked for: nothing launched
    assert _adjoint(lib, cfg, fd.host, cand, cols, gb=None, gl=None, gg=None, ws=None) == 0
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 0, 0.0), PfConfig(tp.n, E + 1, tp.g.size, 0, 0.0),
                PfConfig(tp.n, E, tp.g.size + 1, 0, 0.0)):
        assert _adjoint(lib, bad, fd.host, cand, cols) == EINVAL
        assert query(ctypes.byref(bad), d, 4, E, 190, ctypes.byref(need)) == EINVAL
    assert _adjoint(lib, cfg, fd.host, cand, cols, Bt=0) == EINVAL and _adjoint(lib, cfg, fd.host, cand, cols, Bt=-1) == EINVAL
    assert _adjoint(lib, cfg, fd.host, cand, cols, Bt=2 ** 31) == EINVAL
    assert _adjoint(lib, cfg, fd.host, cand, cols, per_grid=2) == EINVAL
    assert _adjoint(lib, cfg, fd.host, cand, cols, Bt=0x7FFFFFFF) == EINVAL           # more workgroups than one launch takes
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)                 # a Newton-Raphson blob
    assert _adjoint(lib, cfg, nr.host, cand, cols) == EINVAL
    assert query(ctypes.byref(cfg), nr.host.ctypes.data, 4, E, 190, ctypes.byref(need)) == EINVAL
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    assert lib.gns_dcn2_adjoint_lds_bytes(nr.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn2_adjoint_lds_bytes(None, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn2_adjoint_lds_bytes(d, None, ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn2_adjoint_lds_bytes(d, ctypes.byref(lds), None) == 0
    # the lists: candidates ascending, distinct and lines of the grid; columns two different positions into them
    for bad in ([0, E], [-1, 3], [3, 0], [3, 3]):
        assert _adjoint(lib, cfg, fd.host, bad, [[0, 1]]) == EINVAL, bad
    for bad in ([[0, 3]], [[-1, 0]], [[1, 1]]):
        assert _adjoint(lib, cfg, fd.host, cand, bad) == EINVAL, bad
    assert _adjoint(lib, cfg, fd.host, cand, cols, n_cand=0) == EINVAL and _adjoint(lib, cfg, fd.host, cand, cols, P=0) == EINVAL


def test_lds_image_chunk_width_and_refusal():
    lib = amd.load_library()
    for name, w in (('case14', 64), ('case118', 64), ('case300', 16)):
        fd = _fd(TOPOLOGIES[name])
        assert powerflow._dcn2_adjoint_lds_bytes(fd.host) == powerflow._dcn1_adjoint_lds_bytes(fd.host)     # 32 E is the smaller
        assert powerflow._dcn2_adjoint_lds_bytes(fd.host)[1] == w
    tp = pt.path(6000)
    fd = _fd(tp)
    want = 8 * (fd.info['nnz_lu_p'] + fd.info['dim_p'] + 6000 + 3 * 5999 + 2 * fd.info['dim_p'] * 2 + 3)
    assert powerflow._dcn2_adjoint_lds_bytes(fd.host) == (want, 1) and want > pt.LDS_LIMIT
    need = ctypes.c_size_t()
    assert _adjoint(lib, _cfg(tp), fd.host, [0, 1], [[0, 1]]) == EUNSUPPORTED
    assert lib.gns_dcn2_adjoint_workspace_bytes(ctypes.byref(_cfg(tp)), fd.host.ctypes.data, 2, 2, 1, ctypes.byref(need)) == EUNSUPPORTED
    assert _adjoint(lib, _cfg(tp), fd.host, [0, tp.f.size], [[0, 1]]) == EINVAL                             # GNS_EINVAL wins
    assert _adjoint(lib, _cfg(tp), fd.host, [0, 1], [[0, 1]], gb=None, gl=None, gg=None) == EUNSUPPORTED    # before "nothing asked for"
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcn2_adjoint', lambda: powerflow._dcn2_adjoint_lds_bytes(fd.host)[0],
                         powerflow._DCN2_ADJOINT_LDS_FORMULA)
    assert str(want) in str(e.value) and '2 dim_p (W + 1)' in str(e.value) and 'W = 1' in str(e.value)


def test_differentiable_must_be_a_bool():
    buses, lines, gens = synth.synth_grids(14, 2)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='differentiable must be a bool'):
            powerflow.dc_n2_contingency_screen(buses, lines, gens, slack_bus=1, pairs=[[0, 1]], differentiable=bad)


# ---- the adjoint kernels' algorithm in numpy on the FD blob: what gns_dcn2_adjoint does, stage for stage (the factor, pair, gather
# and solve kernels and the reduce), operation for operation but for the order of sums.  The solve program runs as a lane runs it.

def emulate_n2_adjoint(w, bus, line, gen, pairs, islanding, w_flow, w_worst, rating):
    """(d buses, d lines, d generators) of sum_p sum(w_flow_p F'_p) + w_worst_p worst_loading_p; islanding pairs are skipped."""
    N, E, d1 = w[FH['N']], line.shape[0], w[FH['DIM1']]
    p_idx = _arr(w, 'P_IDX', N)
    theta, flow, _ = emulate_solve(w, bus, line, gen)
    F, nnz1 = _factor(w, line)
    ops = _programs(w)['s1'][1]
    b = _line_b(line)
    f, t = line[:, 0].astype(int) - 1, line[:, 1].astype(int) - 1
    pf, pt_ = p_idx[f], p_idx[t]

    def solve(rhs_r):
        Fk = F.copy()
        Fk[nnz1:] = rhs_r
        _lane_solve(Fk, nnz1, ops)
        return np.array([Fk[nnz1 + p_idx[i]] if p_idx[i] >= 0 else 0.0 for i in range(N)])

    def stamp(q, l, x):                           # q += x m_l in B' positions; m_l = 0 for a line from a bus to itself
        if pf[l] != pt_[l]:
            if pf[l] >= 0:
                q[pf[l]] += x
            if pt_[l] >= 0:
                q[pt_[l]] -= x

    def rhs(x):                                   # sum_l x_l b_l m_l, and whether any x_l is not zero (dcn2_lane_rhs)
        q = np.zeros(d1)
        for l in np.flatnonzero(x != 0.0):
            stamp(q, l, x[l] * b[l])
        return q, bool(np.any(x != 0.0))

    # factor kernel: a solve per candidate, H_c[l] = z_c[f_l] - z_c[t_l]
    pairs = np.asarray(pairs)
    cand, cols = np.unique(pairs, return_inverse=True)
    cols = np.sort(cols.reshape(-1, 2), axis=1)                                  # the lower candidate first
    H = np.zeros((cand.size, E))
    for c, e in enumerate(cand):
        a = np.zeros(d1)
        stamp(a, e, 1.0)
        z = solve(a)
        H[c] = z[f] - z[t]
    rt = np.ones(E) if rating is None else rating
    # pair kernel: a record per pair and gF
    gF = np.zeros(E)
    rec = []
    for p, (cj, ck) in enumerate(cols):
        if islanding[p]:
            rec.append(None)
            continue
        ej, ek = cand[cj], cand[ck]
        m11, m12 = 1.0 - b[ej] * H[cj, ej], 0.0 - b[ej] * H[ck, ej]
        m21, m22 = 0.0 - b[ek] * H[cj, ek], 1.0 - b[ek] * H[ck, ek]
        det = m11 * m22 - m12 * m21
        a_j, a_k = (flow[ej] * m22 - m12 * flow[ek]) / det, (m11 * flow[ek] - m21 * flow[ej]) / det
        post = flow + b * (H[cj] * a_j + H[ck] * a_k)
        post[[ej, ek]] = 0.0
        G = np.zeros(E) if w_flow is None else np.array(w_flow[p], dtype=np.float64)
        if w_worst is not None:
            load = np.abs(post) / rt
            at = int(np.flatnonzero(load == load.max())[0])                      # the forward's worst_line: the lowest of equals
            if at != ej and at != ek:
                G[at] += w_worst[p] * np.sign(post[at]) / rt[at]
        G[[ej, ek]] = 0.0
        if not np.any(G != 0.0):
            rec.append(None)
            continue
        gF += G
        x = G * b
        ga_j, ga_k = float(np.sum(x * H[cj])), float(np.sum(x * H[ck]))
        v_j, v_k = (ga_j * m22 - m21 * ga_k) / det, (m11 * ga_k - m12 * ga_j) / det
        gF[ej] += v_j
        gF[ek] += v_k
        rec.append((a_j, a_k, v_j, v_k, G))
    # gather kernel: T'_c and the number of contributing pairs that do not hold c
    T = np.zeros((cand.size, E))
    others = np.zeros(cand.size, dtype=int)
    for p, (cj, ck) in enumerate(cols):
        if rec[p] is None:
            continue
        a_j, a_k, v_j, v_k, G = rec[p]
        others += 1
        others[[cj, ck]] -= 1
        for c, a_c in ((cj, a_j), (ck, a_k)):
            T[c] += G * a_c
            T[c, cand[cj]] += v_j * a_c
            T[c, cand[ck]] += v_k * a_c
    # solve kernel: column 0 is y_0, column c + 1 candidate c
    dth = theta[f] - theta[t]
    q, has = rhs(gF)
    y0 = solve(q) if has else np.zeros(N)
    sw = gF - (y0[f] - y0[t]) if has else np.zeros(E)
    d_b = sw * (dth - line[:, 6])
    for c in range(cand.size):
        q, has = rhs(T[c])
        if has:
            y = solve(q)
            d_b += H[c] * (T[c] - (y[f] - y[t]))
    own = cand[others == 0]                                                      # lines every contributing pair holds: exact zeros
    d_b[own] = 0.0
    sw[own] = 0.0
    d_p = y0
    gb, gl, gg = np.zeros_like(bus), np.zeros_like(line), np.zeros_like(gen)
    gb[:, 2] = gb[:, 4] = -d_p
    gg[:, 6] = d_p[gen[:, 0].astype(int) - 1]
    gl[:, 3] = -d_b * b / line[:, 3]
    gl[:, 5] = -d_b * b / line[:, 5]
    gl[:, 6] = -b * sw
    return gb, gl, gg


def _replay(tp, buses, lines, gens, name, with_flow=True, with_worst=True):
    """Every non-islanding pair of the topology, no pair left out, against the autograd reference at the host bar."""
    w = _fd(tp).host
    E = tp.f.size
    pairs = powerflow._pair_list(None, E)
    isl = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    assert not isl.all()
    rng = np.random.default_rng(len(name))
    for i in range(buses.shape[0]):
        bus, line, gen = (x[i].double().numpy() for x in (buses, lines, gens))
        w_flow = rng.standard_normal((pairs.shape[0], E)) if with_flow else None
        w_worst = rng.standard_normal(pairs.shape[0]) if with_worst else None
        rating = 0.5 + 2.0 * rng.random(E)
        got = emulate_n2_adjoint(w, bus, line, gen, pairs, isl, w_flow, w_worst, rating)
        want, flows = gref.gradients(bus, line, gen, tp.slack, pairs.tolist(), w_flow, w_worst, rating)
        assert np.array_equal(np.isnan(flows.numpy()).all(axis=1), isl)                 # the reference islands at the same pairs
        worst = 0.0
        for x, y, what in zip(got, want, ('buses', 'lines', 'generators')):
            y = y.numpy()
            for c in range(y.shape[1]):
                if c not in CONTRACT[what]:
                    assert np.all(x[:, c] == 0.0) and np.all(y[:, c] == 0.0), (name, i, what, c)
                    continue
                err, scale = float(np.max(np.abs(x[:, c] - y[:, c]))), max(1.0, float(np.max(np.abs(y[:, c]))))
                worst = max(worst, err / (TOL * scale))
                assert err <= TOL * scale, (name, i, what, c, err, scale)
        print(f'{name}[{i}]: {int((~isl).sum())} of {isl.size} pairs, worst error / bar {worst:.3g}')
        # a pair alone gives exact zeros to its own two lines
        j, k = pairs[~isl][i].tolist()
        alone = emulate_n2_adjoint(w, bus, line, gen, [[j, k]], [False], rng.standard_normal((1, E)), rng.standard_normal(1), rating)
        assert np.all(alone[1][[j, k]] == 0.0) and np.any(alone[1] != 0.0), (name, i, j, k)


def test_the_fd_blob_serves_the_n2_adjoint_on_case14():
    """Every non-islanding pair of case14 (163 of 190), both incoming gradients, then each alone."""
    tp = TOPOLOGIES['case14']
    buses, lines, gens = synth.synth_grids(14, 2, seed=0)
    lines = _shifted(lines, seed=14)
    _replay(tp, buses, lines, gens, 'case14')
    _replay(tp, buses[:1], lines[:1], gens[:1], 'case14 flow only', with_worst=False)
    _replay(tp, buses[:1], lines[:1], gens[:1], 'case14 worst only', with_flow=False)


def test_the_fd_blob_serves_the_n2_adjoint_on_case30_with_perturbed_lines():
    """Every non-islanding pair of case30 (612 of 820) with shifts and taps redrawn."""
    tp = TOPOLOGIES['case30']
    buses, lines, gens = synth.synth_grids(30, 1, seed=0)
    _replay(tp, buses, _perturbed(lines, 30), gens, 'case30')


def test_the_fd_blob_serves_the_n2_adjoint_on_a_family_with_a_self_loop_and_parallel_lines():
    """random40_parallel_selfloop, every non-islanding pair (1531 of 1953): pairs of parallel lines and pairs with the self-loop."""
    tp = TOPOLOGIES['random40_parallel_selfloop']
    assert np.any(tp.f == tp.t) and len(special_pairs(tp)) == 2
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, 0)
    _replay(tp, buses, _perturbed(lines, 40), gens, 'random40_parallel_selfloop')
