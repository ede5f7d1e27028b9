"""CPU checks of the host side of the DC contingency screen's adjoint (include/gns_powerflow.h, "DC contingency screening",
gradients): the new exports, the argument checks and the LDS refusal of the three entry points, the image formula and the chunk
width, the Python argument check, and the kernel's algorithm replayed in numpy on the fast-decoupled blob (the B' programs with
the solve program run operation by operation as one lane runs it, the rank-1 forward, the adjoint right-hand side, the second
solve, the Sherman-Morrison correction, the accumulation and the contract) against the autograd reference
(``dc_contingency_grad_reference``: the line removed, the smaller grid solved densely, differentiated by autograd).

The bar is the project's DC bar per contract column: max|out - ref| <= 1e-9 max(1, max|ref|); every other column is exactly 0.
Every non-islanding outage of each grid is in the loss; no column is left out."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import DC_EXPORTS, EXPORTS, FD_EXPORTS, PF_EXPORTS, PfConfig
import dc_contingency_grad_reference as gref
import pf_topologies as pt
from test_dc_contingency_host import _cfg, _fd, _lane_solve
from test_dcpf_host import _factor, _line_b, _shifted, emulate_solve
from test_fdpf_host import FH, _arr, _programs
from test_powerflow_programs_host import TOPOLOGIES

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
TOL = 1e-9
NEW = ('gns_dcn1_adjoint_lds_bytes', 'gns_dcn1_adjoint_workspace_bytes', 'gns_dcn1_adjoint')
CONTRACT = {'buses': (2, 4), 'lines': (3, 5, 6), 'generators': (6,)}


def test_exports_are_there():
    lib = amd.load_library()
    assert _lib.DCN1_EXPORTS[:3] == ('gns_dcn1_lds_bytes', 'gns_dcn1_workspace_bytes', 'gns_dcn1_screen')      # it only grows
    for f in NEW:
        assert f in _lib.DCN1_EXPORTS and hasattr(lib, f), f
        assert f not in EXPORTS and f not in PF_EXPORTS and f not in FD_EXPORTS and f not in DC_EXPORTS
        assert getattr(lib, f).restype is ctypes.c_int
    assert '2 dim_p (W + 1) + 3 W' in powerflow._DCN1_ADJOINT_LDS_FORMULA


def _adjoint(lib, cfg, blob, outages, **kw):
    """gns_dcn1_adjoint on dummy (never dereferenced) device pointers; a keyword replaces one argument."""
    d = blob.ctypes.data
    o = np.asarray(outages, dtype=np.int32)
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, out_host=o.ctypes.data,
             out_dev=d, K=o.size, isl=d, rating=None, per_grid=0, worst_line=d, conv=d, gflow=None, gworst=None, gb=d, gl=d, gg=d,
             ws=d, ws_bytes=0)
    a.update(kw)
    return lib.gns_dcn1_adjoint(a['cfg'], a['host'], a['dev'], a['buses'], a['lines'], a['gens'], a['Bt'], a['out_host'], a['out_dev'],
                                a['K'], a['isl'], a['rating'], a['per_grid'], a['worst_line'], a['conv'], a['gflow'], a['gworst'],
                                a['gb'], a['gl'], a['gg'], a['ws'], a['ws_bytes'], None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host (or has nothing to launch): the test needs no device."""
    lib = amd.load_library()
    tp = TOPOLOGIES['case14']
    fd, cfg = _fd(tp), _cfg(tp)
    E = tp.f.size
    need = ctypes.c_size_t(123)
    d = fd.host.ctypes.data
    # one chunk of 20 outages per grid: a partial of N + 2 E + 1 doubles, rounded up to 256 bytes
    assert lib.gns_dcn1_adjoint_workspace_bytes(ctypes.byref(cfg), d, 4, E, ctypes.byref(need)) == 0
    assert need.value == (4 * 8 * (tp.n + 2 * E + 1) + 255) // 256 * 256
    assert lib.gns_dcn1_adjoint_workspace_bytes(ctypes.byref(cfg), d, 4, 65, ctypes.byref(need)) == 0
    assert need.value == (4 * 2 * 8 * (tp.n + 2 * E + 1) + 255) // 256 * 256
    for args in ((None, d, 4, E, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, None), (ctypes.byref(cfg), d, 0, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, -3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 0x7FFFFFFF, 4 * E, ctypes.byref(need))):
        assert lib.gns_dcn1_adjoint_workspace_bytes(*args) == EINVAL, args
    # null arguments (the rating, either incoming gradient and any gradient output may be NULL)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'out_host', 'out_dev', 'isl', 'worst_line', 'conv', 'ws'):
        assert _adjoint(lib, None if name == 'cfg' else cfg, fd.host, [0, 3], **({} if name == 'cfg' else {name: None})) == EINVAL, name
    assert _adjoint(lib, cfg, fd.host, [0, 3]) == ESIZE                              # every check passed but the workspace's size
    assert _adjoint(lib, cfg, fd.host, [0, 3], gb=None, gl=None, gg=None) == 0       # nothing asked for: nothing launched
    assert _adjoint(lib, cfg, fd.host, [0, 3], gb=None, gl=None, gg=None, ws=None) == 0
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 0, 0.0), PfConfig(tp.n, E + 1, tp.g.size, 0, 0.0),
                PfConfig(tp.n, E, tp.g.size + 1, 0, 0.0)):
        assert _adjoint(lib, bad, fd.host, [0]) == EINVAL
        assert lib.gns_dcn1_adjoint_workspace_bytes(ctypes.byref(bad), d, 4, E, ctypes.byref(need)) == EINVAL
    assert _adjoint(lib, cfg, fd.host, [0], Bt=0) == EINVAL and _adjoint(lib, cfg, fd.host, [0], Bt=-1) == EINVAL
    assert _adjoint(lib, cfg, fd.host, [0], per_grid=2) == EINVAL
    assert _adjoint(lib, cfg, fd.host, list(range(E)) * 4, Bt=0x7FFFFFFF) == EINVAL   # more workgroups than one launch takes
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)                 # a Newton-Raphson blob
    assert _adjoint(lib, cfg, nr.host, [0]) == EINVAL
    assert lib.gns_dcn1_adjoint_workspace_bytes(ctypes.byref(cfg), nr.host.ctypes.data, 4, E, ctypes.byref(need)) == EINVAL
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    assert lib.gns_dcn1_adjoint_lds_bytes(nr.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn1_adjoint_lds_bytes(None, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn1_adjoint_lds_bytes(d, None, ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn1_adjoint_lds_bytes(d, ctypes.byref(lds), None) == 0
    for bad in ([E], [-1], [0, 1, E, 2], [2 ** 31 - 1]):
        assert _adjoint(lib, cfg, fd.host, bad) == EINVAL, bad
    assert _adjoint(lib, cfg, fd.host, [0], K=0) == EINVAL and _adjoint(lib, cfg, fd.host, [0], K=-1) == EINVAL


def _image(info, lanes):
    return 8 * (info['nnz_lu_p'] + info['dim_p'] + info['n_bus'] + 3 * info['n_line'] + 2 * info['dim_p'] * (lanes + 1) + 3 * lanes)


def test_lds_image_chunk_width_and_refusal():
    lib = amd.load_library()
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    want_lanes = {'case14': 64, 'case30': 64, 'case118': 64, 'case300': 16}
    for name in ('case14', 'case30', 'case118', 'case300'):
        fd = _fd(TOPOLOGIES[name])
        assert lib.gns_dcn1_adjoint_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == 0
        w = lanes.value
        assert w == want_lanes[name] and lds.value == _image(fd.info, w) <= pt.LDS_LIMIT, name
        assert w == 64 or _image(fd.info, 2 * w) > pt.LDS_LIMIT, name           # the widest power of two that fits
        assert (lds.value, w) == powerflow._dcn1_adjoint_lds_bytes(fd.host)
        # the screen's image at the same width, a second array of right-hand sides and three doubles per outage
        screen = powerflow._dc_lds_bytes(fd.host) + 8 * (3 * fd.info['n_line'] + fd.info['dim_p'] * (w + 1))
        assert lds.value == screen + 8 * (fd.info['dim_p'] * (w + 1) + 3 * w)
        # the screen's own width and image are what they were
        assert powerflow._dcn1_lds_bytes(fd.host)[1] == {'case14': 64, 'case30': 64, 'case118': 64, 'case300': 32}[name]
    assert _image(_fd(TOPOLOGIES['case118']).info, 64) == 136912
    tp = pt.path(6000)
    fd = _fd(tp)
    want = _image(fd.info, 1)
    assert powerflow._dcn1_adjoint_lds_bytes(fd.host) == (want, 1) and want > pt.LDS_LIMIT
    need = ctypes.c_size_t()
    assert _adjoint(lib, _cfg(tp), fd.host, [0]) == EUNSUPPORTED
    assert lib.gns_dcn1_adjoint_workspace_bytes(ctypes.byref(_cfg(tp)), fd.host.ctypes.data, 2, 1, ctypes.byref(need)) == EUNSUPPORTED
    assert _adjoint(lib, _cfg(tp), fd.host, [tp.f.size]) == EINVAL                      # GNS_EINVAL wins
    assert _adjoint(lib, PfConfig(5999, 5999, 1, 0, 0.0), fd.host, [0]) == EINVAL
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcn1_adjoint', lambda: powerflow._dcn1_adjoint_lds_bytes(fd.host)[0],
                         powerflow._DCN1_ADJOINT_LDS_FORMULA)
    assert str(want) in str(e.value) and '2 dim_p (W + 1)' in str(e.value) and 'W = 1' in str(e.value)


def test_differentiable_must_be_a_bool():
    buses, lines, gens = synth.synth_grids(14, 2)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='differentiable must be a bool'):
            powerflow.dc_contingency_screen(buses, lines, gens, slack_bus=1, differentiable=bad)


# ---- the adjoint kernel's algorithm in numpy on the FD blob: what gns_dcn1_adjoint does, operation for operation but for the
# order of sums

def emulate_screen_adjoint(w, bus, line, gen, outages, bridges, w_flow, w_worst, rating):
    """(d buses, d lines, d generators) of sum_k sum(w_flow_k F'_k) + w_worst_k worst_loading_k; islanding outages are skipped."""
    N, E = w[FH['N']], line.shape[0]
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

    d_p, d_b, s_w = np.zeros(N), np.zeros(E), np.zeros(E)
    for j, k in enumerate(outages):
        if bridges[k]:
            continue
        a = np.zeros(w[FH['DIM1']])
        stamp(a, k, 1.0)
        z = solve(a)
        den = 1.0 - b[k] * (z[f[k]] - z[t[k]])
        alpha = flow[k] / den
        post = flow + b * (z[f] - z[t]) * alpha
        post[k] = 0.0
        G = np.zeros(E) if w_flow is None else np.array(w_flow[j], dtype=np.float64)
        if w_worst is not None:
            load = np.abs(post) if rating is None else np.abs(post) / rating
            at = int(np.flatnonzero(load == load.max())[0])                  # the forward's worst_line: the lowest of equals
            if at != k:
                G[at] += w_worst[j] * np.sign(post[at]) / (1.0 if rating is None else rating[at])
        q = np.zeros(w[FH['DIM1']])
        for l in range(E):
            if l != k and G[l] != 0.0:
                stamp(q, l, G[l] * b[l])
        u = solve(q)
        lam = u + z * (b[k] * (u[f[k]] - u[t[k]]) / den)
        wk = G - (lam[f] - lam[t])
        wk[k] = 0.0
        th_post = theta + alpha * z
        d_p += lam
        d_b += wk * (th_post[f] - th_post[t] - line[:, 6])
        s_w += wk
    gb, gl, gg = np.zeros_like(bus), np.zeros_like(line), np.zeros_like(gen)
    gb[:, 2] = gb[:, 4] = -d_p
    gg[:, 6] = d_p[gen[:, 0].astype(int) - 1]
    gl[:, 3] = -d_b * b / line[:, 3]
    gl[:, 5] = -d_b * b / line[:, 5]
    gl[:, 6] = -b * s_w
    return gb, gl, gg


def _replay(tp, buses, lines, gens, name, with_flow=True, with_worst=True):
    w = _fd(tp).host
    E = tp.f.size
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    outages = list(range(E))
    assert not bridges.all()
    rng = np.random.default_rng(len(name))
    for i in range(buses.shape[0]):
        bus, line, gen = (x[i].double().numpy() for x in (buses, lines, gens))
        w_flow = rng.standard_normal((E, E)) if with_flow else None
        w_worst = rng.standard_normal(E) if with_worst else None
        rating = 0.5 + 2.0 * rng.random(E)
        got = emulate_screen_adjoint(w, bus, line, gen, outages, bridges, w_flow, w_worst, rating)
        want, flows = gref.gradients(bus, line, gen, tp.slack, outages, w_flow, w_worst, rating)
        assert np.array_equal(np.isnan(flows.numpy()).all(axis=1), bridges)            # islanding exactly at the bridges
        for x, y, what in zip(got, want, ('buses', 'lines', 'generators')):
            y = y.numpy()
            for c in range(y.shape[1]):
                if c not in CONTRACT[what]:
                    assert np.all(x[:, c] == 0.0) and np.all(y[:, c] == 0.0), (name, i, what, c)
                    continue
                err, scale = float(np.max(np.abs(x[:, c] - y[:, c]))), max(1.0, float(np.max(np.abs(y[:, c]))))
                print(f'{name}[{i}] d/d{what}[{c}]: err {err:.3e} scale {scale:.3e}')
                assert err <= TOL * scale, (name, i, what, c, err, scale)
        # row k gives nothing to line k's own columns: outage k alone, all its weights on
        k = int(np.flatnonzero(~bridges)[i])
        alone = emulate_screen_adjoint(w, bus, line, gen, [k], bridges, rng.standard_normal((1, E)), rng.standard_normal(1), rating)
        assert np.all(alone[1][k] == 0.0) and np.any(alone[1] != 0.0), (name, i, k)


@pytest.mark.parametrize('case,batch', [(14, 2), (30, 2), (118, 1)])
def test_the_fd_blob_serves_the_screen_adjoint_on_the_cases(case, batch):
    """Every non-islanding outage of the case, with shifts that matter and a rating, both incoming gradients."""
    tp = TOPOLOGIES[f'case{case}']
    buses, lines, gens = synth.synth_grids(case, batch, seed=0)
    _replay(tp, buses, _shifted(lines, seed=case), gens, f'case{case}')


@pytest.mark.parametrize('name', ['random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen', 'lattice8x8'])
def test_the_fd_blob_serves_the_screen_adjoint_on_generated_families(name):
    """Parallel lines, a line from a bus to itself, stacked generators, a slack without a generator, lines at the slack."""
    tp = TOPOLOGIES[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0)
    _replay(tp, buses, _shifted(lines, seed=len(name)), gens, name)


def test_each_incoming_gradient_alone_on_case14():
    tp = TOPOLOGIES['case14']
    buses, lines, gens = synth.synth_grids(14, 1, seed=3)
    _replay(tp, buses, _shifted(lines, seed=3), gens, 'case14 flow only', with_worst=False)
    _replay(tp, buses, _shifted(lines, seed=3), gens, 'case14 worst only', with_flow=False)
