"""CPU checks of the host side of ``powerflow.solved_case`` (include/gns_powerflow.h, "The solved case"): the four exports, the
refusals of the entry points in the documented order (on dummy pointers: nothing is launched), the workspace figures, the Python
argument checks and the error where no device is visible; and the float64 reference (``solved_case_reference``) against
``nr_reference.mismatch`` and against central differences of its own forward."""
import ctypes
import os

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
from helpers import ROOT
import ac_contingency_reference as aref
import nr_reference as nr
import pf_topologies as pt
import solved_case_reference as sref

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
NEW = ('gns_pfs_workspace_bytes', 'gns_pfs_evaluate', 'gns_pfs_adjoint_workspace_bytes', 'gns_pfs_adjoint')
HEAD = ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'Bt', 'v', 'theta', 'rating', 'per_grid')
EVAL = HEAD + ('p_from', 'q_from', 'p_to', 'q_to', 'p_inj', 'q_inj', 'gen_p', 'gen_q', 'mismatch', 'slack_p', 'worst_loading',
               'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus', 'ws', 'ws_bytes')
ADJ = HEAD + ('worst_line', 'v_min_bus', 'v_max_bus', 'g_p_from', 'g_q_from', 'g_p_to', 'g_q_to', 'g_p_inj', 'g_q_inj', 'g_gen_p',
              'g_gen_q', 'g_slack_p', 'g_worst', 'g_v_min', 'g_v_max', 'grad_v', 'grad_theta', 'gb', 'gl', 'gg', 'ws', 'ws_bytes')
SCALARS = ('Bt', 'per_grid', 'ws_bytes', 'cfg')


def _topo(name='random24_stacked_gens'):
    tp = pt.families()[name]
    return tp, powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack), PfConfig(tp.n, tp.f.size, tp.g.size, 0, 0.0)


def test_the_four_symbols_are_exported_typed_and_declared():
    lib = amd.load_library()
    assert _lib.PFS_EXPORTS == NEW
    others = (_lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.DCN2_EXPORTS +
              _lib.DCN2_ADJOINT_EXPORTS + _lib.ACN1_EXPORTS + _lib.ACN1_ADJOINT_EXPORTS + _lib.ACN2_EXPORTS + _lib.ACN2_ADJOINT_EXPORTS +
              _lib.DCG1_EXPORTS + _lib.DCG1_ADJOINT_EXPORTS + _lib.ACG1_EXPORTS + _lib.ACG1_ADJOINT_EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    for f in NEW:
        assert hasattr(lib, f) and f not in others, f
        assert getattr(lib, f).restype is ctypes.c_int and f'int {f}(' in hdr
    for fn, names in ((lib.gns_pfs_evaluate, EVAL), (lib.gns_pfs_adjoint, ADJ)):
        at = fn.argtypes
        assert len(at) == len(names) + 1                                   # and the stream
        assert at[names.index('Bt')] is ctypes.c_int64 and at[names.index('per_grid')] is ctypes.c_int32
        assert at[names.index('ws_bytes')] is ctypes.c_size_t
        assert all(at[names.index(k)] is ctypes.c_void_p for k in names if k not in SCALARS)
    assert len(lib.gns_pfs_workspace_bytes.argtypes) == 4 and len(lib.gns_pfs_adjoint_workspace_bytes.argtypes) == 4


def _call(fn, names, cfg, blob, **kw):
    """An entry point on dummy (never dereferenced) device pointers; a keyword replaces one argument.  Only calls the host refuses,
    or that have nothing to launch, are made."""
    d = blob.ctypes.data
    a = {k: d for k in names}
    a.update(cfg=ctypes.byref(cfg) if cfg is not None else None, Bt=1, rating=None, per_grid=0, ws_bytes=0)
    a.update({k: None for k in names if k.startswith('g_')})
    a.update(kw)
    return fn(*(a[k] for k in names), None)


def test_workspace_queries():
    lib = amd.load_library()
    need, pf_need = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for name in ('pair', 'random24_stacked_gens', 'hub150_70lines_70gens'):
        tp, topo, cfg = _topo(name)
        d = topo.host.ctypes.data
        for Bt in (1, 3, 1000):
            assert lib.gns_pfs_workspace_bytes(ctypes.byref(cfg), d, Bt, ctypes.byref(need)) == 0
            assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), d, Bt, ctypes.byref(pf_need)) == 0
            assert need.value == pf_need.value == (Bt * 16 * topo.info['nnz_ybus'] + 255) // 256 * 256
            assert lib.gns_pfs_adjoint_workspace_bytes(ctypes.byref(cfg), d, Bt, ctypes.byref(need)) == 0 and need.value == 0
    tp, topo, cfg = _topo()
    d = topo.host.ctypes.data
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    wrong_n = PfConfig(tp.n + 1, tp.f.size, tp.g.size, 0, 0.0)
    for q in (lib.gns_pfs_workspace_bytes, lib.gns_pfs_adjoint_workspace_bytes):
        for args in ((None, d, 4, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, None),
                     (ctypes.byref(cfg), d, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, -2, ctypes.byref(need)),
                     (ctypes.byref(wrong_n), d, 4, ctypes.byref(need)), (ctypes.byref(cfg), fd.host.ctypes.data, 4, ctypes.byref(need))):
            assert q(*args) == EINVAL, args


def test_entry_points_refuse_in_the_documented_order_before_any_launch():
    lib = amd.load_library()
    tp, topo, cfg = _topo()
    E, Gn = tp.f.size, tp.g.size
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    need = ctypes.c_size_t(0)
    assert lib.gns_pfs_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 1, ctypes.byref(need)) == 0
    required = {'evaluate': ('host', 'dev', 'buses', 'lines', 'gens', 'v', 'theta', 'mismatch', 'slack_p', 'worst_loading', 'worst_line',
                             'v_min', 'v_min_bus', 'v_max', 'v_max_bus', 'ws'),
                'adjoint': ('host', 'dev', 'buses', 'lines', 'gens', 'v', 'theta', 'worst_line', 'v_min_bus', 'v_max_bus')}
    for fn, names, key in ((lib.gns_pfs_evaluate, EVAL, 'evaluate'), (lib.gns_pfs_adjoint, ADJ, 'adjoint')):
        big = dict(ws_bytes=2 ** 40)
        assert _call(fn, names, None, topo.host, **big) == EINVAL
        for name in required[key]:
            assert _call(fn, names, cfg, topo.host, **big, **{name: None}) == EINVAL, (key, name)
        assert _call(fn, names, cfg, fd.host, **big) == EINVAL                          # a fast-decoupled blob
        for bad in (PfConfig(tp.n + 1, E, Gn, 0, 0.0), PfConfig(tp.n, E + 1, Gn, 0, 0.0), PfConfig(tp.n, E, Gn + 1, 0, 0.0)):
            assert _call(fn, names, bad, topo.host, **big) == EINVAL
        for per_grid in (2, -1):
            assert _call(fn, names, cfg, topo.host, per_grid=per_grid, **big) == EINVAL
        for Bt in (0, -1, 2 ** 31):
            assert _call(fn, names, cfg, topo.host, Bt=Bt, ws_bytes=2 ** 62) == EINVAL
    # the forward's short workspace, after every GNS_EINVAL
    assert _call(lib.gns_pfs_evaluate, EVAL, cfg, topo.host, ws_bytes=need.value - 1) == ESIZE
    assert _call(lib.gns_pfs_evaluate, EVAL, cfg, topo.host, ws_bytes=need.value - 1, per_grid=2) == EINVAL
    assert _call(lib.gns_pfs_evaluate, EVAL, cfg, topo.host, ws_bytes=0) == ESIZE
    # the adjoint needs no workspace; with no output asked for it launches nothing
    nothing = dict(grad_v=None, grad_theta=None, gb=None, gl=None, gg=None)
    assert _call(lib.gns_pfs_adjoint, ADJ, cfg, topo.host, **nothing) == 0
    assert _call(lib.gns_pfs_adjoint, ADJ, cfg, topo.host, ws=None, **nothing) == 0
    assert _call(lib.gns_pfs_adjoint, ADJ, cfg, topo.host, per_grid=2, **nothing) == EINVAL


def test_the_lds_image_is_five_bus_vectors_and_the_limit_refuses_after_the_workspace():
    lib = amd.load_library()
    tp = pt.path(4097)                                                      # 40 N = 163 880 B, above the 163 840 B limit
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 0, 0.0)
    need = ctypes.c_size_t(0)
    assert lib.gns_pfs_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 1, ctypes.byref(need)) == 0
    assert _call(lib.gns_pfs_evaluate, EVAL, cfg, topo.host, ws_bytes=need.value - 1) == ESIZE
    assert _call(lib.gns_pfs_evaluate, EVAL, cfg, topo.host, ws_bytes=need.value) == EUNSUPPORTED
    assert _call(lib.gns_pfs_adjoint, ADJ, cfg, topo.host) == EUNSUPPORTED
    assert _call(lib.gns_pfs_adjoint, ADJ, cfg, topo.host, grad_v=None, grad_theta=None, gb=None, gl=None, gg=None) == EUNSUPPORTED
    assert 40 * 4096 == pt.LDS_LIMIT


def test_python_argument_checks_and_no_device_is_an_error():
    buses, lines, gens, slack, v, theta = synth.solvable_grids(14, 2)
    with pytest.raises(ValueError, match=r'v / theta must be \[2,14\]'):
        powerflow.solved_case(buses, lines, gens, v[:, :13], theta, slack_bus=slack)
    with pytest.raises(ValueError, match=r'v / theta must be \[2,14\]'):
        powerflow.solved_case(buses, lines, gens, v, theta[0], slack_bus=slack)
    with pytest.raises(ValueError, match='must be a float tensor'):
        powerflow.solved_case(buses, lines, gens, v.long(), theta, slack_bus=slack)
    with pytest.raises(ValueError, match='rating must be'):
        powerflow.solved_case(buses, lines, gens, v, theta, slack_bus=slack, rating=torch.ones(3))
    with pytest.raises(ValueError, match='rating must be positive'):
        powerflow.solved_case(buses, lines, gens, v, theta, slack_bus=slack, rating=torch.zeros(lines.shape[1]))
    assert powerflow.SolvedCase._fields == ('p_from', 'q_from', 'p_to', 'q_to', 'p_inj', 'q_inj', 'mismatch', 'gen_p', 'gen_q', 'slack_p',
                                            'worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus')
    if not torch.cuda.is_available():
        with pytest.raises(gns_mod.GNSError, match='no CPU fallback'):
            powerflow.solved_case(buses, lines, gens, v, theta, slack_bus=slack)


# ---- the reference

def _grid(name, regime, seed=0):
    tp = pt.families()[name]
    buses, lines, gens, v, theta = pt.grids(tp, regime, 1, seed)
    v0, th0 = pt.perturbed_start(v, theta, tp.slack, seed + 1)
    return tp, buses[0].double().numpy(), lines[0].double().numpy(), gens[0].double().numpy(), v0[0].numpy(), th0[0].numpy()


@pytest.mark.parametrize('name', ['pair', 'random24_stacked_gens', 'ring30_slack_no_gen', 'random40_parallel_selfloop'])
@pytest.mark.parametrize('regime', pt.REGIMES)
def test_reference_mismatch_is_nr_references_and_its_two_routes_to_the_injections_agree(name, regime):
    tp, bus, ln, gen, v, th = _grid(name, regime)
    case = sref.forward(bus, ln, gen, tp.slack, v, th)
    assert case.mismatch == nr.mismatch(bus, ln, gen, tp.slack, v, th)
    # the Y-bus route (forward) and the sum of the flows that leave a bus plus its shunt (the torch restatement)
    out = sref.torch_outputs(*(torch.as_tensor(a) for a in (bus, ln, gen, v, th)), tp.slack, None, case)
    for key in sref.DIFF_OUT:
        ref = np.asarray(getattr(case, key))
        assert np.max(np.abs(out[key].numpy() - ref), initial=0.0) <= 1e-13 * max(1.0, np.max(np.abs(ref), initial=0.0)), key
    # the balance: generation less demand is what every bus with units injects
    gb = gen[:, 0].astype(int) - 1
    q_by_bus = np.zeros(tp.n)
    np.add.at(q_by_bus, gb, case.gen_q)
    has = np.isin(np.arange(tp.n), gb)
    assert np.allclose(q_by_bus[has] - bus[has, 3], case.q_inj[has], rtol=0, atol=1e-12)
    p_slack = sum(case.gen_p[u] for u in range(gb.size) if gb[u] == tp.slack - 1)
    listed = sum(gen[u, 6] for u in range(gb.size) if gb[u] == tp.slack - 1)
    assert abs(listed + case.slack_p - bus[tp.slack - 1, 2] - case.p_inj[tp.slack - 1]) <= 1e-12
    if np.any(gb == tp.slack - 1):
        assert abs(p_slack - bus[tp.slack - 1, 2] - case.p_inj[tp.slack - 1]) <= 1e-12


EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize('name', ['pair', 'random24_stacked_gens'])
def test_reference_gradients_agree_with_central_differences(name):
    """Every one of the twelve differentiable outputs is weighted; the summaries' indices are frozen at the unperturbed state's.

    The step and the bar.  The central difference D(h) = (l(p + h) - l(p - h)) / 2h has the truncation error T = h^2 l''' / 6 + O(h^4)
    and a rounding error R.  T is estimated from the second difference, not assumed: D(2h) - D(h) = 3 T + O(h^4), so |D(2h) - D(h)| / 3
    estimates it; it is doubled for the O(h^4) remainder.  R: every output is a short chain of float64 operations (at most 16 on the
    way to a flow, an injection term or a generator's share) on intermediates no larger than A = max|stamp| max|V|^2 (the two
    products of a flow nearly cancel, so its rounding error scales with A, not with the flow), so an evaluation of the loss is off by
    at most 16 eps A sum|w|, and D(h) by that over h (two evaluations over 2h).  The estimate of T carries (R(h) + R(2h)) / 3 of its
    own, so the bar is 2 |D(2h) - D(h)| / 3 + 2 R(h).  h = 1e-4: with third derivatives of order 1 - 1e3 (the line parameters enter
    through 1 / (r + jx), x >= 0.04) T is about 1e-9 - 1e-6, and R(h) about 1e-7; a smaller step would only raise R."""
    tp, bus, ln, gen, v, th = _grid(name, 'reference')
    ln = ln.copy()
    ln[:, 6] += np.linspace(-0.2, 0.2, ln.shape[0])                       # shifts that matter
    rng = np.random.default_rng(7)
    N, E, Gn = tp.n, tp.f.size, tp.g.size
    shape = dict(p_from=E, q_from=E, p_to=E, q_to=E, p_inj=N, q_inj=N, gen_p=Gn, gen_q=Gn, slack_p=(), worst_loading=(), v_min=(),
                 v_max=())
    w = {k: rng.standard_normal(shape[k]) for k in sref.DIFF_OUT}
    rating = 0.5 + 2.0 * rng.random(E)
    at = sref.forward(bus, ln, gen, tp.slack, v, th, rating)
    grads = dict(zip(('buses', 'lines', 'generators', 'v', 'theta'), sref.gradients(bus, ln, gen, tp.slack, v, th, w, rating)))
    arrays = dict(buses=bus, lines=ln, generators=gen, v=v.reshape(-1, 1), theta=th.reshape(-1, 1))
    cols = dict(sref.DIFF_COLS, v=[0], theta=[0])

    def value(p):
        c = sref.forward(p['buses'], p['lines'], p['generators'], tp.slack, p['v'][:, 0], p['theta'][:, 0], rating)
        sf, st = np.hypot(c.p_from, c.q_from), np.hypot(c.p_to, c.q_to)
        frozen = c._replace(worst_loading=(sf if at.from_end else st)[at.worst_line] / rating[at.worst_line],
                            v_min=p['v'][at.v_min_bus, 0], v_max=p['v'][at.v_max_bus, 0])
        return sref.loss(frozen, w)

    h = 1e-4
    stamps = np.abs(np.concatenate(aref.line_admittances(ln)[2:]))
    A = float(stamps.max()) * (float(np.max(np.abs(v))) + 2 * h) ** 2 / min(1.0, float(rating.min()))
    R = 16 * EPS * A * sum(float(np.sum(np.abs(w[k]))) for k in sref.DIFF_OUT) / h
    worst = 0.0
    for what, arr in arrays.items():
        grad = grads[what].reshape(arr.shape)
        for c in range(arr.shape[1]):
            if c not in cols[what]:
                assert np.all(grad[:, c] == 0.0), (what, c)
                continue
            for i in range(arr.shape[0]):
                d = {}
                for step in (h, 2 * h):
                    vals = []
                    for s in (+step, -step):
                        p = {k: a.copy() for k, a in arrays.items()}
                        p[what][i, c] += s
                        vals.append(value(p))
                    d[step] = (vals[0] - vals[1]) / (2 * step)
                bar = 2.0 * abs(d[2 * h] - d[h]) / 3.0 + 2.0 * R
                err = abs(d[h] - grad[i, c])
                worst = max(worst, err / bar)
                assert err <= bar, (what, i, c, d[h], grad[i, c], bar)
    print(f'{name}: worst error / bar {worst:.3f}')
