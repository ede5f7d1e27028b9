"""The host side of the DC generator screen's gradients (``gns_dcg1_adjoint``; include/gns_powerflow.h, "Gradients of the DC
generator screen"): the exports, the refusals of the three entry points and their order, the workspace formula, the Python
argument checks, and a numpy replay of the five kernels' algorithm on the FD blob against the float64 autograd reference
(``dc_generator_contingency_grad_reference``: the unit redispatched by tensor arithmetic, the line removed, the smaller grid solved
densely) at max|out - ref| <= 1e-9 max(1, max|ref|) per contract column, ``grad_pickup`` included, every other column exactly 0.
No device is needed: every C call below is refused on the host or has nothing to launch."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
import dc_generator_contingency_grad_reference as gref
import pf_topologies as pt
from test_dc_contingency_host import _cfg, _fd
from test_dc_generator_contingency_host import _solve_column, emulate_factor
from test_dcpf_gpu import _perturbed
from test_dcpf_host import _factor, _shifted, emulate_solve
from test_fdpf_host import FH, _arr
from test_powerflow_programs_host import TOPOLOGIES

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
TOL = 1e-9
CONTRACT = {'buses': (2, 4), 'lines': (3, 5, 6), 'generators': (6,)}
NEW = ('gns_dcg1_adjoint_lds_bytes', 'gns_dcg1_adjoint_workspace_bytes', 'gns_dcg1_adjoint')


def test_exports_are_there():
    lib = amd.load_library()
    assert _lib.DCG1_EXPORTS == ('gns_dcg1_lds_bytes', 'gns_dcg1_workspace_bytes', 'gns_dcg1_screen')
    assert _lib.DCG1_ADJOINT_EXPORTS == NEW
    for f in NEW:
        assert hasattr(lib, f) and getattr(lib, f).restype is ctypes.c_int, f
    assert '2 dim_p (W + 1) + 3 W' in powerflow._DCG1_ADJOINT_LDS_FORMULA and '32 E' in powerflow._DCG1_ADJOINT_LDS_FORMULA
    assert callable(powerflow.dc_generator_contingency_screen_differentiable)


def _adjoint(lib, cfg, blob, line_list, gen_list, cols, **kw):
    """gns_dcg1_adjoint on dummy (never dereferenced) device pointers; a keyword replaces one argument."""
    d = blob.ctypes.data
    li = np.asarray(line_list, dtype=np.int32)
    ge = np.asarray(gen_list, dtype=np.int32)
    p = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).reshape(-1, 2))
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, line_host=li.ctypes.data,
             line_dev=d, n_line=li.size, gen_host=ge.ctypes.data, gen_dev=d, n_gen=ge.size, cols_host=p.ctypes.data, cols_dev=d,
             P=p.shape[0], isl=d, rating=None, per_grid=0, pickup=None, pickup_per_grid=0, worst_line=d, conv=d, gflow=None,
             gworst=None, gb=d, gl=d, gg=d, gp=d, ws=d, ws_bytes=0)
    a.update(kw)
    return lib.gns_dcg1_adjoint(a['cfg'], a['host'], a['dev'], a['buses'], a['lines'], a['gens'], a['Bt'], a['line_host'], a['line_dev'],
                                a['n_line'], a['gen_host'], a['gen_dev'], a['n_gen'], a['cols_host'], a['cols_dev'], a['P'], a['isl'],
                                a['rating'], a['per_grid'], a['pickup'], a['pickup_per_grid'], a['worst_line'], a['conv'], a['gflow'],
                                a['gworst'], a['gb'], a['gl'], a['gg'], a['gp'], a['ws'], a['ws_bytes'], None)


def _want_bytes(tp, Bt, n_line, n_gen, P, lanes):
    """The workspace formula of the header: the forward's block, then T / S, the records, the row chunks' partials of gF, gF, a
    count per candidate, the solve kernel's partials, the generators' y by bus and three doubles per listed generator as doubles and
    a byte per grid, each of the two parts rounded up to 256 bytes."""
    N, E = tp.n, tp.f.size
    n_cand = n_line + n_gen
    Q = 32 if P >= 8192 else 8
    chunks_p, chunks_a = -(-P // Q), -(-(n_cand + 1) // lanes)
    forward = (Bt * 8 * (n_cand * E + 2 * E + n_cand + 1) + 255) // 256 * 256
    own = Bt * 8 * (n_cand * E + 4 * P + chunks_p * (E + 1) + E + n_cand + chunks_a * (N + 2 * E + 1) + n_gen * N + 3 * n_gen) + Bt
    return forward + (own + 255) // 256 * 256


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = amd.load_library()
    tp = TOPOLOGIES['case14']
    fd, cfg = _fd(tp), _cfg(tp)
    E, Gn = tp.f.size, tp.g.size
    need = ctypes.c_size_t(123)
    d = fd.host.ctypes.data
    query = lib.gns_dcg1_adjoint_workspace_bytes
    assert query(ctypes.byref(cfg), d, 4, E, Gn, 105, ctypes.byref(need)) == 0 and need.value == _want_bytes(tp, 4, E, Gn, 105, 64)
    assert query(ctypes.byref(cfg), d, 3, 0, 2, 9000, ctypes.byref(need)) == 0 and need.value == _want_bytes(tp, 3, 0, 2, 9000, 64)
    tp300 = TOPOLOGIES['case300']
    assert query(ctypes.byref(_cfg(tp300)), _fd(tp300).host.ctypes.data, 2, 30, 11, 60, ctypes.byref(need)) == 0
    assert need.value == _want_bytes(tp300, 2, 30, 11, 60, 16)                        # three chunks of 16 columns
    ok = (ctypes.byref(cfg), d, 4, E, Gn, 105, ctypes.byref(need))
    for at, bad in ((0, None), (1, None), (6, None), (2, 0), (3, -1), (3, E + 1), (4, 0), (4, -3), (4, Gn + 1), (5, 0), (5, -1),
                    (2, 0x7FFFFFFF)):
        args = list(ok)
        args[at] = bad
        assert query(*args) == EINVAL, (at, bad)
    li, ge, cols = [0, 3, 7], [1, 4], [[0, 1], [1, -1], [0, 2]]
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'line_host', 'line_dev', 'gen_host', 'gen_dev', 'cols_host', 'cols_dev',
                 'isl', 'worst_line', 'conv', 'ws'):
        assert _adjoint(lib, None if name == 'cfg' else cfg, fd.host, li, ge, cols, **({} if name == 'cfg' else {name: None})) == EINVAL, name
    assert _adjoint(lib, cfg, fd.host, li, ge, cols) == ESIZE                         # every check passed but the workspace's size
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, ws_bytes=_want_bytes(tp, 1, 3, 2, 3, 64) - 1) == ESIZE
    none = dict(gb=None, gl=None, gg=None, gp=None)
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, **none) == 0                     # nothing asked for: nothing launched
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, ws=None, **none) == 0
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, gb=None, gl=None, gg=None) == ESIZE      # grad_pickup alone is an output
    # an empty line list needs no line pointers; its rows then hold -1 alone
    assert _adjoint(lib, cfg, fd.host, [], ge, [[0, -1], [1, -1]], line_host=None, line_dev=None) == ESIZE
    assert _adjoint(lib, cfg, fd.host, [], ge, [[0, 0]], line_host=None, line_dev=None) == EINVAL
    for bad in (PfConfig(tp.n + 1, E, Gn, 0, 0.0), PfConfig(tp.n, E + 1, Gn, 0, 0.0), PfConfig(tp.n, E, Gn + 1, 0, 0.0)):
        assert _adjoint(lib, bad, fd.host, li, ge, cols) == EINVAL
        assert query(ctypes.byref(bad), d, 4, E, Gn, 105, ctypes.byref(need)) == EINVAL
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, Bt=0) == EINVAL and _adjoint(lib, cfg, fd.host, li, ge, cols, Bt=-1) == EINVAL
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, Bt=2 ** 31) == EINVAL
    for flag in ('per_grid', 'pickup_per_grid'):
        assert _adjoint(lib, cfg, fd.host, li, ge, cols, **{flag: 2}) == EINVAL and _adjoint(lib, cfg, fd.host, li, ge, cols, **{flag: -1}) == EINVAL
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, Bt=0x7FFFFFFF) == EINVAL         # more workgroups than one launch takes
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)                 # a Newton-Raphson blob
    assert _adjoint(lib, cfg, nr.host, li, ge, cols) == EINVAL
    assert query(ctypes.byref(cfg), nr.host.ctypes.data, 4, E, Gn, 105, ctypes.byref(need)) == EINVAL
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    assert lib.gns_dcg1_adjoint_lds_bytes(nr.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcg1_adjoint_lds_bytes(None, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcg1_adjoint_lds_bytes(d, None, ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcg1_adjoint_lds_bytes(d, ctypes.byref(lds), None) == 0
    # gns_dcg1_screen's list checks: both lists in range, ascending, distinct; rows positions into them, or -1 for no line
    for bad in ([0, E], [-1, 2], [3, 0, 7], [0, 3, 3]):
        assert _adjoint(lib, cfg, fd.host, bad, ge, [[0, 1]]) == EINVAL, bad
    for bad in ([0, Gn], [-1, 2], [3, 0], [1, 1]):
        assert _adjoint(lib, cfg, fd.host, li, bad, [[0, 1]]) == EINVAL, bad
    for bad in ([[2, 0]], [[-1, 0]], [[0, 3]], [[0, -2]]):
        assert _adjoint(lib, cfg, fd.host, li, ge, bad) == EINVAL, bad
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, n_gen=0) == EINVAL and _adjoint(lib, cfg, fd.host, li, ge, cols, P=0) == EINVAL
    assert _adjoint(lib, cfg, fd.host, li, ge, cols, n_line=-1) == EINVAL


def test_lds_image_chunk_width_and_refusal():
    lib = amd.load_library()
    for name, w in (('case14', 64), ('case118', 64), ('case300', 16)):
        fd = _fd(TOPOLOGIES[name])
        assert powerflow._dcg1_adjoint_lds_bytes(fd.host) == powerflow._dcn1_adjoint_lds_bytes(fd.host)     # 32 E is the smaller
        assert powerflow._dcg1_adjoint_lds_bytes(fd.host)[1] == w
    tp = pt.path(6000)
    fd = _fd(tp)
    want = 8 * (fd.info['nnz_lu_p'] + fd.info['dim_p'] + 6000 + 3 * 5999 + 2 * fd.info['dim_p'] * 2 + 3)
    assert powerflow._dcg1_adjoint_lds_bytes(fd.host) == (want, 1) and want > pt.LDS_LIMIT
    need = ctypes.c_size_t()
    assert _adjoint(lib, _cfg(tp), fd.host, [0, 1], [0], [[0, 1]]) == EUNSUPPORTED
    assert lib.gns_dcg1_adjoint_workspace_bytes(ctypes.byref(_cfg(tp)), fd.host.ctypes.data, 2, 2, 1, 1, ctypes.byref(need)) == EUNSUPPORTED
    assert _adjoint(lib, _cfg(tp), fd.host, [0, tp.f.size], [0], [[0, 1]]) == EINVAL                        # GNS_EINVAL wins
    assert _adjoint(lib, _cfg(tp), fd.host, [0, 1], [0], [[0, 1]], gb=None, gl=None, gg=None, gp=None) == EUNSUPPORTED
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcg1_adjoint', lambda: powerflow._dcg1_adjoint_lds_bytes(fd.host)[0],
                         powerflow._DCG1_ADJOINT_LDS_FORMULA)
    assert str(want) in str(e.value) and '2 dim_p (W + 1)' in str(e.value) and 'W = 1' in str(e.value)


def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 2)
    Gn = gens.shape[1]

    def screen(**kw):
        return powerflow.dc_generator_contingency_screen_differentiable(buses, lines, gens, slack_bus=1, **kw)

    with pytest.raises(TypeError):                                            # the function differentiates: there is no flag
        screen(differentiable=True)
    with pytest.raises(ValueError, match=r'contingencies must be a \[P,2\]'):
        screen(contingencies=[0, 1])
    with pytest.raises(ValueError, match='contingencies must name generators in'):
        screen(contingencies=[[Gn, 0]])
    with pytest.raises(ValueError, match='pickup must be non-negative and finite'):
        screen(pickup=-torch.ones(Gn).requires_grad_(True))
    with pytest.raises(ValueError, match="pickup must be None, 'pmax' or weights"):
        screen(pickup='pmin')
    with pytest.raises(ValueError, match='flows must be a bool'):
        screen(flows=1)
    with pytest.raises(ValueError, match='rating must be positive and finite'):
        screen(rating=torch.zeros(lines.shape[1]))
    with pytest.raises(TypeError):                                            # the plain call keeps its signature
        powerflow.dc_generator_contingency_screen(buses, lines, gens, slack_bus=1, differentiable=True)


# ---- the adjoint kernels' algorithm in numpy on the FD blob: what gns_dcg1_adjoint does, stage for stage (the factor, row, gather
# and solve kernels and the reduce), operation for operation but for the order of sums.  The solve program runs as a lane runs it.

def emulate_g1_adjoint(w, bus, line, gen, rows, islanding, w_flow, w_worst, rating, pickup):
    """(d buses, d lines, d generators, d pickup) of sum_p sum(w_flow_p F'_p) + w_worst_p worst_loading_p; islanding rows are
    skipped.  ``pickup``: None or float64 weights [Gn]."""
    N, E, Gn, d1 = w[FH['N']], line.shape[0], gen.shape[0], w[FH['DIM1']]
    p_idx = _arr(w, 'P_IDX', N)
    theta, _, _ = emulate_solve(w, bus, line, gen)
    Ff, nnz1 = _factor(w, line)
    f, t = line[:, 0].astype(int) - 1, line[:, 1].astype(int) - 1
    pf, pt_ = p_idx[f], p_idx[t]
    gbus = gen[:, 0].astype(int) - 1

    def rhs(x, b):                                # sum_l x_l b_l m_l, and whether any x_l is not zero (dcn2_lane_rhs)
        q = np.zeros(d1)
        for l in np.flatnonzero(x != 0.0):
            if pf[l] != pt_[l]:
                if pf[l] >= 0:
                    q[pf[l]] += x[l] * b[l]
                if pt_[l] >= 0:
                    q[pt_[l]] -= x[l] * b[l]
        return q, bool(np.any(x != 0.0))

    # factor kernel: H_k per distinct line, D_g per distinct generator
    rows = np.asarray(rows).reshape(-1, 2)
    gen_list, cg = np.unique(rows[:, 0], return_inverse=True)
    k = rows[:, 1]
    line_list = np.unique(k[k >= 0])
    ck = np.where(k >= 0, np.searchsorted(line_list, k), -1)
    H, D, F, b = emulate_factor(w, bus, line, gen, line_list.tolist(), gen_list.tolist(), pickup)
    rt = np.ones(E) if rating is None else rating
    # row kernel: a record per row and gF
    gF = np.zeros(E)
    rec = []
    for p in range(rows.shape[0]):
        if islanding[p]:
            rec.append(None)
            continue
        fg = F + b * D[cg[p]]
        ek, alpha, den = -1, 0.0, 1.0
        post = fg
        if ck[p] >= 0:
            ek = line_list[ck[p]]
            den = 1.0 - b[ek] * H[ck[p], ek]
            alpha = fg[ek] / den
            post = fg + (b * H[ck[p]]) * alpha
            post[ek] = 0.0
        G = np.zeros(E) if w_flow is None else np.array(w_flow[p], dtype=np.float64)
        if w_worst is not None:
            load = np.abs(post) / rt
            at = int(np.flatnonzero(load == load.max())[0])                      # the forward's worst_line: the lowest of equals
            if at != ek:
                G[at] += w_worst[p] * np.sign(post[at]) / rt[at]
        if ek >= 0:
            G[ek] = 0.0
        if not np.any(G != 0.0):
            rec.append(None)
            continue
        gF += G
        v = 0.0
        if ek >= 0:
            v = float(np.sum((G * b) * H[ck[p]])) / den
            gF[ek] += v
        rec.append((alpha, v, G, ek))
    # gather kernel: T_k, S_g and the number of contributing rows that do not hold a line
    n_line = line_list.size
    T = np.zeros((n_line + gen_list.size, E))
    others = np.zeros(n_line, dtype=int)
    for p in range(rows.shape[0]):
        if rec[p] is None:
            continue
        alpha, v, G, ek = rec[p]
        others += 1
        if ck[p] >= 0:
            others[ck[p]] -= 1
            T[ck[p]] += G * alpha
            T[ck[p], ek] += v * alpha
        T[n_line + cg[p]] += G
        if ek >= 0:
            T[n_line + cg[p], ek] += v
    # solve kernel: column 0 is y_0, then the lines, then the generators
    HD = np.concatenate([H, D], axis=0)
    dth = theta[f] - theta[t]
    q, has = rhs(gF, b)
    y0 = _solve_column(w, Ff, nnz1, q) if has else np.zeros(N)
    sw = gF - (y0[f] - y0[t]) if has else np.zeros(E)
    d_b = sw * (dth - line[:, 6])
    ycols = np.zeros((gen_list.size, N))
    for c in range(T.shape[0]):
        q, has = rhs(T[c], b)
        if has:
            y = _solve_column(w, Ff, nnz1, q)
            d_b += HD[c] * (T[c] - (y[f] - y[t]))
            if c >= n_line:
                ycols[c - n_line] = y
    own = line_list[others == 0]                                                 # lines every contributing row holds: exact zeros
    d_b[own] = 0.0
    sw[own] = 0.0
    # reduce kernel: the contract, and the generators' Pg and w terms
    gb, gl, gg, gp = np.zeros_like(bus), np.zeros_like(line), np.zeros_like(gen), np.zeros(Gn)
    gb[:, 2] = gb[:, 4] = -y0
    gg[:, 6] = y0[gbus]
    gl[:, 3] = -d_b * b / line[:, 3]
    gl[:, 5] = -d_b * b / line[:, 5]
    gl[:, 6] = -b * sw
    for c, gi in enumerate(gen_list):
        y = ycols[c]
        W = 0.0
        if pickup is not None:
            for h in range(Gn):
                if h != gi:
                    W += pickup[h]
        s = 0.0
        if W > 0.0:
            for h in range(Gn):
                if h != gi:
                    s += (pickup[h] / W) * y[gbus[h]]
        gg[gi, 6] += s - y[gbus[gi]]
        if W > 0.0:
            coef = gen[gi, 6] / W
            for h in range(Gn):
                if h != gi:
                    gp[h] += coef * (y[gbus[h]] - s)
    return gb, gl, gg, gp


def _replay(tp, buses, lines, gens, name, pickup, with_flow=True, with_worst=True, grids=None):
    """Every default row of the topology, no row left out, against the autograd reference at the host bar."""
    w = _fd(tp).host
    E, Gn = tp.f.size, tp.g.size
    rows = powerflow._generator_contingency_list(None, Gn, E)
    isl = powerflow._generator_islanding(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1), rows)
    assert not isl.all()
    rng = np.random.default_rng(len(name))
    for i in (range(buses.shape[0]) if grids is None else grids):
        bus, line, gen = (x[i].double().numpy() for x in (buses, lines, gens))
        w_flow = rng.standard_normal((rows.shape[0], E)) if with_flow else None
        w_worst = rng.standard_normal(rows.shape[0]) if with_worst else None
        rating = 0.5 + 2.0 * rng.random(E)
        if pickup == 'random':
            wi = 0.1 + rng.random(Gn)
            wi[Gn // 2] = 0.0
        else:
            wi = gen[:, 1].copy() if pickup == 'pmax' else None
        got = emulate_g1_adjoint(w, bus, line, gen, rows, isl, w_flow, w_worst, rating, wi)
        want, want_w, flows = gref.gradients(bus, line, gen, tp.slack, rows.tolist(), w_flow, w_worst, rating,
                                             'pmax' if pickup == 'pmax' else wi)
        assert np.array_equal(np.isnan(flows.numpy()).all(axis=1), isl)                 # the reference islands at the same rows
        got_g = got[2].copy()
        if pickup == 'pmax':                                                            # the weights are the generators' column 1
            got_g[:, 1] = got[3]
        contract = dict(CONTRACT, generators=(1, 6) if pickup == 'pmax' else (6,))
        worst = 0.0
        for x, y, what in zip((got[0], got[1], got_g), want, ('buses', 'lines', 'generators')):
            y = y.numpy()
            for c in range(y.shape[1]):
                if c not in contract[what]:
                    assert np.all(x[:, c] == 0.0) and np.all(y[:, c] == 0.0), (name, i, what, c)
                    continue
                err, scale = float(np.max(np.abs(x[:, c] - y[:, c]))), max(1.0, float(np.max(np.abs(y[:, c]))))
                worst = max(worst, err / (TOL * scale))
                assert err <= TOL * scale, (name, i, what, c, err, scale)
        if pickup == 'random':
            y = want_w.numpy()
            err, scale = float(np.max(np.abs(got[3] - y))), max(1.0, float(np.max(np.abs(y))))
            worst = max(worst, err / (TOL * scale))
            assert err <= TOL * scale and np.any(y != 0.0), (name, i, 'pickup', err, scale)
        elif pickup is None:
            assert np.all(got[3] == 0.0) and want_w is None
        else:
            assert np.any(got[3] != 0.0)
        print(f'{name}[{i}] pickup {pickup}: {int((~isl).sum())} of {isl.size} rows, worst error / bar {worst:.3g}')
        # a row alone gives exact zeros to its own line
        g, k = rows[~isl & (rows[:, 1] >= 0)][i].tolist()
        alone = emulate_g1_adjoint(w, bus, line, gen, [[g, k]], [False], rng.standard_normal((1, E)), rng.standard_normal(1), rating, wi)
        assert np.all(alone[1][k] == 0.0) and np.any(alone[1] != 0.0), (name, i, g, k)


@pytest.mark.parametrize('pickup', [None, 'pmax', 'random'])
def test_the_fd_blob_serves_the_generator_adjoint_on_case14(pickup):
    """Every default row of case14 (100 of 105 do not island), both incoming gradients, then each alone."""
    tp = TOPOLOGIES['case14']
    buses, lines, gens = synth.synth_grids(14, 2, seed=0)
    lines = _shifted(lines, seed=14)
    _replay(tp, buses, lines, gens, 'case14', pickup)
    _replay(tp, buses[:1], lines[:1], gens[:1], 'case14 flow only', pickup, with_worst=False)
    _replay(tp, buses[:1], lines[:1], gens[:1], 'case14 worst only', pickup, with_flow=False)


@pytest.mark.parametrize('pickup', ['pmax', 'random'])
def test_the_fd_blob_serves_the_generator_adjoint_with_units_stacked_on_a_bus_and_on_the_slack(pickup):
    """random24_stacked_gens, every default row (272 of 312): several units on one bus, and units on the slack bus, whose y is 0."""
    tp = pt.families()['random24_stacked_gens']
    on = np.bincount(tp.g, minlength=tp.n + 1)
    assert on.max() > 1 and on[tp.slack] >= 1
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, 0)
    _replay(tp, buses, _perturbed(lines, 24), gens, 'random24_stacked_gens', pickup)
