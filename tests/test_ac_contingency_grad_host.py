"""CPU checks of the host side of the AC contingency screen's adjoint (include/gns_powerflow.h, "AC contingency screening",
gradients): the new exports and their argument types, the refusals of the two entry points in the documented order (on dummy
pointers: nothing is launched), the workspace formula and the chunk size, the Python argument check and the error where no device
is visible, and the float64 reference (``ac_contingency_grad_reference``) against central finite differences of the reference
solve on a toy grid with a parallel line and a line from a bus to itself."""
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
import ac_contingency_grad_reference as gref
import ac_contingency_reference as aref
import pf_topologies as pt
from test_ac_contingency_host import _case14, toy

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
NEW = ('gns_acn1_adjoint_workspace_bytes', 'gns_acn1_adjoint')
ARGS = ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'Bt', 'out_host', 'out_dev', 'K', 'isl', 'rating', 'per_grid', 'v', 'theta',
        'conv', 'worst_line', 'v_min_bus', 'v_max_bus', 'base_conv', 'g_v', 'g_theta', 'g_p_from', 'g_q_from', 'g_p_to', 'g_q_to',
        'g_worst', 'g_v_min', 'g_v_max', 'gb', 'gl', 'gg', 'ws', 'ws_bytes')


def test_exports_are_there_with_their_argument_types():
    lib = amd.load_library()
    assert _lib.ACN1_ADJOINT_EXPORTS == NEW
    others = _lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.ACN1_EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    for f in NEW:
        assert hasattr(lib, f) and f not in others, f
        assert getattr(lib, f).restype is ctypes.c_int and f'int {f}(' in hdr
    assert len(lib.gns_acn1_adjoint_workspace_bytes.argtypes) == 5
    at = lib.gns_acn1_adjoint.argtypes
    assert len(at) == len(ARGS) + 1                                     # and the stream
    assert at[ARGS.index('Bt')] is ctypes.c_int64 and at[ARGS.index('K')] is ctypes.c_int32
    assert at[ARGS.index('per_grid')] is ctypes.c_int32 and at[ARGS.index('ws_bytes')] is ctypes.c_size_t
    assert all(at[ARGS.index(k)] is ctypes.c_void_p for k in ARGS if k not in ('cfg', 'Bt', 'K', 'per_grid', 'ws_bytes'))


def _adjoint(lib, cfg, blob, outages, **kw):
    """gns_acn1_adjoint on dummy (never dereferenced) device pointers; a keyword replaces one argument.  Only calls the host refuses,
    or that have nothing to launch, are made."""
    d = blob.ctypes.data
    o = np.asarray(outages, dtype=np.int32)
    a = {k: d for k in ARGS}
    a.update(cfg=ctypes.byref(cfg) if cfg is not None else None, Bt=1, out_host=o.ctypes.data, K=o.size, rating=None, per_grid=0,
             ws_bytes=0, **{k: None for k in ARGS if k.startswith('g_')})
    a.update(kw)
    return lib.gns_acn1_adjoint(*(a[k] for k in ARGS), None)


def _partial(tp):
    """Doubles of one (grid, chunk) partial: four per bus, five per line, one per generator and the status."""
    return 4 * tp.n + 5 * tp.f.size + tp.g.size + 1


def _chunk(K):
    """Rows a wave walks: a wave per row up to 32 outages, then ceil(K / 32), at most 8."""
    return min(8, max(1, -(-K // 32)))


def _ws_bytes(topo, tp, Bt, K):
    up = lambda x: (x + 255) // 256 * 256                               # noqa: E731
    return up(Bt * 16 * topo.info['nnz_ybus']) + up(Bt * -(-K // _chunk(K)) * 8 * _partial(tp))


def test_workspace_formula_and_chunk_size():
    lib = amd.load_library()
    need = ctypes.c_size_t(0)
    for tp in (_case14(), toy()):
        topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
        cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
        for Bt, K in ((1, 1), (4, tp.f.size), (3, 32), (3, 33), (2, 64), (2, 65), (5, 255), (1, 257), (7, 1000)):
            assert lib.gns_acn1_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, K, ctypes.byref(need)) == 0
            assert need.value == _ws_bytes(topo, tp, Bt, K), (tp.name, Bt, K)
    # the chunk size comes from the list's length alone: the chunks of a grid are the same in any batch
    assert [_chunk(k) for k in (1, 16, 32, 33, 59, 64, 65, 166, 224, 225, 411, 5000)] == [1, 1, 1, 2, 2, 2, 3, 6, 7, 8, 8, 8]


def test_entry_points_refuse_in_the_documented_order_before_any_launch():
    lib = amd.load_library()
    tp = _case14()
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    E = tp.f.size
    cfg = PfConfig(tp.n, E, tp.g.size, 10, 1e-8)
    d = topo.host.ctypes.data
    need = ctypes.c_size_t(0)
    for args in ((None, d, 4, E, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, None), (ctypes.byref(cfg), d, 0, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, -3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 0x7FFFFFFF, 2, ctypes.byref(need))):
        assert lib.gns_acn1_adjoint_workspace_bytes(*args) == EINVAL, args
    # NULL pointers (the rating, every incoming gradient and every gradient output may be NULL)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'out_host', 'out_dev', 'isl', 'v', 'theta', 'conv', 'worst_line',
                 'v_min_bus', 'v_max_bus', 'base_conv', 'ws'):
        assert _adjoint(lib, None if name == 'cfg' else cfg, topo.host, [0, 3], **({} if name == 'cfg' else {name: None})) == EINVAL, name
    assert _adjoint(lib, cfg, topo.host, [0, 3]) == ESIZE                                # every check passed but the workspace's size
    assert lib.gns_acn1_adjoint_workspace_bytes(ctypes.byref(cfg), d, 1, 2, ctypes.byref(need)) == 0
    assert _adjoint(lib, cfg, topo.host, [0, 3], ws_bytes=need.value - 1) == ESIZE
    assert _adjoint(lib, cfg, topo.host, [0, E], ws_bytes=need.value - 1) == EINVAL       # GNS_EINVAL wins
    assert _adjoint(lib, cfg, topo.host, [0, 3], gb=None, gl=None, gg=None) == 0          # nothing asked for: nothing launched
    assert _adjoint(lib, cfg, topo.host, [0, 3], gb=None, gl=None, gg=None, ws=None) == 0
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8), PfConfig(tp.n, E + 1, tp.g.size, 10, 1e-8),
                PfConfig(tp.n, E, tp.g.size + 1, 10, 1e-8), PfConfig(tp.n, E, tp.g.size, -1, 1e-8),
                PfConfig(tp.n, E, tp.g.size, 10, -1.0)):
        assert _adjoint(lib, bad, topo.host, [0]) == EINVAL
    assert lib.gns_acn1_adjoint_workspace_bytes(ctypes.byref(PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8)), d, 4, E,
                                                ctypes.byref(need)) == EINVAL
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)                  # a fast-decoupled blob
    assert _adjoint(lib, cfg, fd.host, [0]) == EINVAL
    assert lib.gns_acn1_adjoint_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 4, E, ctypes.byref(need)) == EINVAL
    for bad in ([E], [-1], [0, 1, E, 2], [2 ** 31 - 1]):
        assert _adjoint(lib, cfg, topo.host, bad) == EINVAL, bad
    assert _adjoint(lib, cfg, topo.host, [0], K=0) == EINVAL and _adjoint(lib, cfg, topo.host, [0], K=-1) == EINVAL
    assert _adjoint(lib, cfg, topo.host, [0], Bt=0) == EINVAL and _adjoint(lib, cfg, topo.host, [0], Bt=-1) == EINVAL
    assert _adjoint(lib, cfg, topo.host, [0], per_grid=2) == EINVAL
    assert _adjoint(lib, cfg, topo.host, [0, 1, 2], Bt=0x7FFFFFFF, ws_bytes=2 ** 62) == EINVAL   # more workgroups than one launch takes


def test_lds_refusal_comes_from_the_query_too_and_names_newton_raphsons_image():
    lib = amd.load_library()
    tp = pt.path(4096)
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert topo.info['lds_bytes'] > pt.LDS_LIMIT
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
    need = ctypes.c_size_t(0)
    assert lib.gns_acn1_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 1, 1, ctypes.byref(need)) == EUNSUPPORTED
    assert _adjoint(lib, cfg, topo.host, [0], ws_bytes=2 ** 40) == EUNSUPPORTED
    assert _adjoint(lib, cfg, topo.host, [0], gb=None, gl=None, gg=None) == EUNSUPPORTED          # before "nothing asked for"
    assert _adjoint(lib, cfg, topo.host, [tp.f.size], ws_bytes=2 ** 40) == EINVAL                # GNS_EINVAL wins
    with pytest.raises(amd.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_acn1_adjoint_workspace_bytes', topo.info['lds_bytes'], powerflow._ACN1.formula)
    assert 'nnz(L+U) + dim + 8 N' in str(e.value)


def test_differentiable_must_be_a_bool_and_no_device_is_an_error():
    buses, lines, gens = synth.synth_grids(14, 2)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='differentiable must be a bool'):
            powerflow.ac_contingency_screen(buses, lines, gens, slack_bus=1, differentiable=bad)
    if not torch.cuda.is_available():
        with pytest.raises(gns_mod.GNSError, match='no CPU fallback'):
            powerflow.ac_contingency_screen(buses, lines.clone().requires_grad_(True), gens, slack_bus=1, differentiable=True)
        with pytest.raises(ValueError, match='outages must lie in'):                     # the shapes are still checked first
            powerflow.ac_contingency_screen(buses, lines.clone().requires_grad_(True), gens, slack_bus=1, differentiable=True,
                                            outages=[lines.shape[1]])


# ---- the reference against central finite differences of the reference solve

def _toy_grid(seed=0):
    tp = toy()
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, seed)
    lines = lines.clone()
    lines[..., 6] += torch.linspace(-0.2, 0.2, lines.shape[1])         # shifts that matter
    return tp, buses[0].double().numpy(), lines[0].double().numpy(), gens[0].double().numpy()


def _loss_value(bus, ln, gen, slack, k, v0, th0, w, rating, at):
    row = aref.outage(bus, ln, gen, slack, k, v0, th0, 1e-13, 30)
    assert row is not None and row.converged
    val = sum(float(np.dot(w[n], getattr(row, n))) for n in ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to'))
    sf, st = np.hypot(row.p_from, row.q_from), np.hypot(row.p_to, row.q_to)
    wi = at['worst_line']
    val += w['worst_loading'] * (sf[wi] if at['from_end'] else st[wi]) / rating[wi]
    return val + w['v_min'] * row.v[at['v_min_bus']] + w['v_max'] * row.v[at['v_max_bus']]


@pytest.mark.parametrize('k', [0, 5, 6])
def test_reference_agrees_with_central_differences_on_the_toy_grid(k):
    """Line 0 has a parallel line (5), line 6 runs from bus 3 to itself.  All nine outputs are weighted; the summaries' indices are
    frozen at the unperturbed row's (their runners-up are far from a 1e-6 step)."""
    tp, bus, ln, gen = _toy_grid()
    rng = np.random.default_rng(k)
    N, E = tp.n, tp.f.size
    w = dict(v=rng.standard_normal(N), theta=rng.standard_normal(N), worst_loading=float(rng.standard_normal()),
             v_min=float(rng.standard_normal()), v_max=float(rng.standard_normal()),
             **{n: rng.standard_normal(E) for n in ('p_from', 'q_from', 'p_to', 'q_to')})
    rating = 0.5 + 2.0 * rng.random(E)
    base = aref.base_case(bus, ln, gen, tp.slack, 1e-13, 30)
    row = aref.outage(bus, ln, gen, tp.slack, k, base[0], base[1], 1e-13, 30)
    assert row.converged
    load = aref.loading(row, rating)
    wi = int(np.argmax(load))
    at = dict(worst_line=wi, from_end=bool(np.hypot(row.p_from[wi], row.q_from[wi]) >= np.hypot(row.p_to[wi], row.q_to[wi])),
              v_min_bus=int(np.argmin(row.v)), v_max_bus=int(np.argmax(row.v)))
    (gb, gl, gg), cond = gref.row_gradient(bus, ln, gen, tp.slack, k, row, w, rating)
    assert np.all(gl[k] == 0.0) and cond < 1e4
    h = 1e-6
    worst = 0.0
    for what, arr, grad in (('buses', bus, gb), ('lines', ln, gl), ('generators', gen, gg)):
        for c in range(arr.shape[1]):
            if c not in gref.DIFF_COLS[what]:
                assert np.all(grad[:, c] == 0.0), (what, c)
                continue
            for i in range(arr.shape[0]):
                vals = []
                for s in (+h, -h):
                    p = {'buses': bus.copy(), 'lines': ln.copy(), 'generators': gen.copy()}
                    p[what][i, c] += s
                    vals.append(_loss_value(p['buses'], p['lines'], p['generators'], tp.slack, k, row.v, row.theta, w, rating, at))
                fd = (vals[0] - vals[1]) / (2 * h)
                err = abs(fd - grad[i, c])
                worst = max(worst, err / (1e-6 * max(1.0, abs(fd))))
                assert err <= 1e-6 * max(1.0, abs(fd)), (what, i, c, fd, grad[i, c])
    print(f'toy outage {k}: worst error / bar {worst:.3f}, cond {cond:.1f}')
