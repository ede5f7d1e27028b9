"""CPU checks of the host side of the AC N-2 screen's adjoint (include/gns_powerflow.h, "Gradients of the AC N-2 screen"): the new
exports and their argument types, the workspace formula and the chunk rule, the refusals of the two entry points in the documented
order (on dummy pointers: nothing is launched), the Python refusals of ``ac_n2_contingency_screen_differentiable`` and the error
where no device is visible, and the float64 reference (``ac_n2_grad_reference``) against central finite differences of the
reference solve on the toy grid, for the pair of parallel lines and for a pair with the line from a bus to itself."""
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
import ac_n2_grad_reference as g2ref
import ac_n2_reference as n2ref
import pf_topologies as pt
from test_ac_contingency_grad_host import ARGS, _partial, _toy_grid
from test_ac_contingency_host import _case14, toy

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
NEW = ('gns_acn2_adjoint_workspace_bytes', 'gns_acn2_adjoint')


def test_exports_are_there_with_their_argument_types():
    lib = amd.load_library()
    assert _lib.ACN2_ADJOINT_EXPORTS == NEW
    others = (_lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.DCN2_EXPORTS +
              _lib.DCN2_ADJOINT_EXPORTS + _lib.ACN1_EXPORTS + _lib.ACN1_ADJOINT_EXPORTS + _lib.ACN2_EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    for f in NEW:
        assert hasattr(lib, f) and f not in others, f
        assert getattr(lib, f).restype is ctypes.c_int and f'int {f}(' in hdr
    assert 'Gradients of the AC N-2 screen' in hdr and 'Not here: gradients' not in hdr
    assert len(lib.gns_acn2_adjoint_workspace_bytes.argtypes) == 5
    at = lib.gns_acn2_adjoint.argtypes                                  # gns_acn1_adjoint's list, the pairs in place of the outages
    assert at == lib.gns_acn1_adjoint.argtypes and len(at) == len(ARGS) + 1
    assert callable(powerflow.ac_n2_contingency_screen_differentiable)


def _adjoint(lib, cfg, blob, pairs, **kw):
    """gns_acn2_adjoint on dummy (never dereferenced) device pointers; a keyword replaces one argument.  Only calls the host refuses,
    or that have nothing to launch, are made."""
    d = blob.ctypes.data
    o = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    a = {k: d for k in ARGS}
    a.update(cfg=ctypes.byref(cfg) if cfg is not None else None, Bt=1, out_host=o.ctypes.data, K=o.shape[0], rating=None, per_grid=0,
             ws_bytes=0, **{k: None for k in ARGS if k.startswith('g_')})
    a.update(kw)
    return lib.gns_acn2_adjoint(*(a[k] for k in ARGS), None)


def _chunk(P):
    """Rows a wave walks: a wave per row up to 64 pairs, then ceil(P / 64), without a cap."""
    return max(1, -(-P // 64))


def _ws_bytes(topo, tp, Bt, P):
    up = lambda x: (x + 255) // 256 * 256                               # noqa: E731
    return up(Bt * 16 * topo.info['nnz_ybus']) + up(Bt * -(-P // _chunk(P)) * 8 * _partial(tp))


def test_workspace_formula_and_chunk_rule():
    lib = amd.load_library()
    need, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for tp in (_case14(), toy()):
        topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
        cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
        for Bt in (1, 3, 64):
            for P in (1, 64, 65, 190, 17205):
                assert lib.gns_acn2_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, P, ctypes.byref(need)) == 0
                assert need.value == _ws_bytes(topo, tp, Bt, P), (tp.name, Bt, P)
                # per grid: the base Y-bus and at most 64 partials, whatever P is
                assert need.value <= 256 + Bt * 16 * topo.info['nnz_ybus'] + 256 + Bt * 64 * 8 * _partial(tp)
        # up to 32 rows the two adjoints cut a list alike: the same bytes
        assert lib.gns_acn1_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 3, 20, ctypes.byref(n1)) == 0
        assert lib.gns_acn2_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 3, 20, ctypes.byref(need)) == 0
        assert need.value == n1.value
    # the chunk comes from the list's length alone (the chunks of a grid are the same in any batch): C and the chunks per grid
    assert [_chunk(p) for p in (1, 64, 65, 128, 129, 130, 190, 17205)] == [1, 1, 2, 2, 3, 3, 3, 269]
    assert [-(-p // _chunk(p)) for p in (1, 64, 65, 128, 129, 130, 190, 17205)] == [1, 64, 33, 64, 43, 44, 64, 64]


def test_entry_points_refuse_in_the_documented_order_before_any_launch():
    lib = amd.load_library()
    tp = _case14()
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    E = tp.f.size
    cfg = PfConfig(tp.n, E, tp.g.size, 10, 1e-8)
    d = topo.host.ctypes.data
    need = ctypes.c_size_t(0)
    for args in ((None, d, 4, 3, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, 3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 3, None), (ctypes.byref(cfg), d, 0, 3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, -3, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 0x7FFFFFFF, 2, ctypes.byref(need))):
        assert lib.gns_acn2_adjoint_workspace_bytes(*args) == EINVAL, args
    # NULL pointers (the rating, every incoming gradient and every gradient output may be NULL)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'out_host', 'out_dev', 'isl', 'v', 'theta', 'conv', 'worst_line',
                 'v_min_bus', 'v_max_bus', 'base_conv', 'ws'):
        assert _adjoint(lib, None if name == 'cfg' else cfg, topo.host, [[0, 3], [3, 5]],
                        **({} if name == 'cfg' else {name: None})) == EINVAL, name
    assert _adjoint(lib, cfg, topo.host, [[0, 3], [3, 0]]) == ESIZE                       # every check passed but the workspace's size
    assert lib.gns_acn2_adjoint_workspace_bytes(ctypes.byref(cfg), d, 1, 2, ctypes.byref(need)) == 0
    assert _adjoint(lib, cfg, topo.host, [[0, 3], [3, 0]], ws_bytes=need.value - 1) == ESIZE
    assert _adjoint(lib, cfg, topo.host, [[0, 3], [3, E]], ws_bytes=need.value - 1) == EINVAL     # GNS_EINVAL wins
    assert _adjoint(lib, cfg, topo.host, [[0, 3], [3, 3]], ws_bytes=need.value - 1) == EINVAL
    assert _adjoint(lib, cfg, topo.host, [[0, 3]], gb=None, gl=None, gg=None) == 0        # nothing asked for: nothing launched
    assert _adjoint(lib, cfg, topo.host, [[0, 3]], gb=None, gl=None, gg=None, ws=None) == 0
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8), PfConfig(tp.n, E + 1, tp.g.size, 10, 1e-8),
                PfConfig(tp.n, E, tp.g.size + 1, 10, 1e-8), PfConfig(tp.n, E, tp.g.size, -1, 1e-8),
                PfConfig(tp.n, E, tp.g.size, 10, -1.0)):
        assert _adjoint(lib, bad, topo.host, [[0, 1]]) == EINVAL
    assert lib.gns_acn2_adjoint_workspace_bytes(ctypes.byref(PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8)), d, 4, 3,
                                                ctypes.byref(need)) == EINVAL
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)                  # a fast-decoupled blob
    assert _adjoint(lib, cfg, fd.host, [[0, 1]]) == EINVAL
    assert lib.gns_acn2_adjoint_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 4, 3, ctypes.byref(need)) == EINVAL
    # the pairs: a line outside 0 .. E-1 at either position, twice the same line; with nothing asked for too (the list comes first)
    for bad in ([[0, E]], [[E, 0]], [[-1, 2]], [[2, -1]], [[0, 1], [2, 3], [4, E]], [[2 ** 31 - 1, 0]], [[5, 5]], [[0, 1], [7, 7]]):
        assert _adjoint(lib, cfg, topo.host, bad, ws_bytes=2 ** 40) == EINVAL, bad
        assert _adjoint(lib, cfg, topo.host, bad, gb=None, gl=None, gg=None) == EINVAL, bad
    assert _adjoint(lib, cfg, topo.host, [[0, 1]], K=0) == EINVAL and _adjoint(lib, cfg, topo.host, [[0, 1]], K=-1) == EINVAL
    assert _adjoint(lib, cfg, topo.host, [[0, 1]], Bt=0) == EINVAL and _adjoint(lib, cfg, topo.host, [[0, 1]], Bt=-1) == EINVAL
    assert _adjoint(lib, cfg, topo.host, [[0, 1]], per_grid=2) == EINVAL
    assert _adjoint(lib, cfg, topo.host, [[0, 1], [1, 2], [2, 3]], Bt=0x7FFFFFFF, ws_bytes=2 ** 62) == EINVAL   # more workgroups than one launch takes


def test_lds_refusal_comes_from_the_query_too_and_names_newton_raphsons_image():
    lib = amd.load_library()
    tp = pt.path(4096)
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert topo.info['lds_bytes'] > pt.LDS_LIMIT
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
    need = ctypes.c_size_t(0)
    assert lib.gns_acn2_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 1, 1, ctypes.byref(need)) == EUNSUPPORTED
    assert _adjoint(lib, cfg, topo.host, [[0, 1]], ws_bytes=2 ** 40) == EUNSUPPORTED
    assert _adjoint(lib, cfg, topo.host, [[0, 1]], gb=None, gl=None, gg=None) == EUNSUPPORTED      # before "nothing asked for"
    assert _adjoint(lib, cfg, topo.host, [[0, tp.f.size]], ws_bytes=2 ** 40) == EINVAL            # GNS_EINVAL wins
    assert _adjoint(lib, cfg, topo.host, [[2, 2]], ws_bytes=2 ** 40) == EINVAL
    with pytest.raises(amd.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_acn2_adjoint_workspace_bytes', topo.info['lds_bytes'], powerflow._ACN2.formula)
    assert 'nnz(L+U) + dim + 8 N' in str(e.value)


def test_python_refusals_come_before_a_device_is_needed():
    buses, lines, gens = synth.synth_grids(14, 2)
    E = lines.shape[1]

    def screen(**kw):
        return powerflow.ac_n2_contingency_screen_differentiable(buses, lines.clone().requires_grad_(True), gens, slack_bus=1, **kw)

    with pytest.raises(ValueError, match='pairs is empty'):
        screen(pairs=[])
    with pytest.raises(ValueError, match=r'pairs must be a \[P,2\]'):
        screen(pairs=[0, 1])
    with pytest.raises(ValueError, match='pairs must hold integers'):
        screen(pairs=[[0, 1.5]])
    with pytest.raises(ValueError, match='pairs must lie in'):
        screen(pairs=[[0, E]])
    with pytest.raises(ValueError, match=r"two different lines, got \(4, 4\) at row 1: a single outage is ac_contingency_screen's"):
        screen(pairs=[[0, 1], [4, 4]])
    with pytest.raises(ValueError, match='rating must be positive and finite'):
        screen(rating=torch.zeros(E))
    with pytest.raises(ValueError, match='flows must be a bool'):
        screen(flows=1)
    with pytest.raises(ValueError, match='states must be a bool'):
        screen(states=None)
    with pytest.raises(ValueError, match='tol must be'):
        screen(tol=-1e-9)
    with pytest.raises(ValueError, match='max_iter must be'):
        screen(max_iter=2.5)
    with pytest.raises(TypeError):
        screen(differentiable=True)                       # not a keyword: the call is the differentiable one
    if not torch.cuda.is_available():
        with pytest.raises(gns_mod.GNSError, match='no CPU fallback'):
            screen(pairs=[[0, 1]])
    # the plain call's signature is what it was
    import inspect
    plain = inspect.signature(powerflow.ac_n2_contingency_screen)
    assert inspect.signature(powerflow.ac_n2_contingency_screen_differentiable) == plain and 'differentiable' not in plain.parameters


# ---- the reference against central finite differences of the reference solve

def _loss_value(bus, ln, gen, slack, pair, v0, th0, w, rating, at):
    row = n2ref.pair(bus, ln, gen, slack, pair[0], pair[1], v0, th0, 1e-13, 30)
    assert row is not None and row.converged
    val = sum(float(np.dot(w[n], getattr(row, n))) for n in ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to'))
    sf, st = np.hypot(row.p_from, row.q_from), np.hypot(row.p_to, row.q_to)
    wi = at['worst_line']
    val += w['worst_loading'] * (sf[wi] if at['from_end'] else st[wi]) / rating[wi]
    return val + w['v_min'] * row.v[at['v_min_bus']] + w['v_max'] * row.v[at['v_max_bus']]


@pytest.mark.parametrize('pair', [(0, 5), (2, 6), (6, 1)])
def test_reference_agrees_with_central_differences_on_the_toy_grid(pair):
    """Lines 0 and 5 are parallel (both out: numeric zeros in the pattern), line 6 runs from bus 3 to itself: with line 2, which
    ends at bus 3, and, given the other way round, with line 1.  All nine outputs are weighted; the summaries' indices are frozen
    at the unperturbed row's (their runners-up are far from a 1e-6 step)."""
    tp, bus, ln, gen = _toy_grid()
    j, k = min(pair), max(pair)
    rng = np.random.default_rng(10 * j + k)
    N, E = tp.n, tp.f.size
    w = dict(v=rng.standard_normal(N), theta=rng.standard_normal(N), worst_loading=float(rng.standard_normal()),
             v_min=float(rng.standard_normal()), v_max=float(rng.standard_normal()),
             **{n: rng.standard_normal(E) for n in ('p_from', 'q_from', 'p_to', 'q_to')})
    rating = 0.5 + 2.0 * rng.random(E)
    base = aref.base_case(bus, ln, gen, tp.slack, 1e-13, 30)
    row = n2ref.pair(bus, ln, gen, tp.slack, j, k, base[0], base[1], 1e-13, 30)
    assert row is not None and row.converged
    load = aref.loading(row, rating)
    wi = int(np.argmax(load))
    assert wi not in (j, k)
    at = dict(worst_line=wi, from_end=bool(np.hypot(row.p_from[wi], row.q_from[wi]) >= np.hypot(row.p_to[wi], row.q_to[wi])),
              v_min_bus=int(np.argmin(row.v)), v_max_bus=int(np.argmax(row.v)))
    (gb, gl, gg), cond = g2ref.row_gradient(bus, ln, gen, tp.slack, pair, row, w, rating)
    assert np.all(gl[[j, k]] == 0.0) and np.any(gl != 0.0) and cond < 1e4
    swapped, _ = g2ref.row_gradient(bus, ln, gen, tp.slack, pair[::-1], row, w, rating)
    assert all(np.array_equal(a, b) for a, b in zip((gb, gl, gg), swapped))
    h = 1e-6
    worst = 0.0
    for what, arr, grad in (('buses', bus, gb), ('lines', ln, gl), ('generators', gen, gg)):
        for c in range(arr.shape[1]):
            if c not in g2ref.DIFF_COLS[what]:
                assert np.all(grad[:, c] == 0.0), (what, c)
                continue
            for i in range(arr.shape[0]):
                vals = []
                for s in (+h, -h):
                    p = {'buses': bus.copy(), 'lines': ln.copy(), 'generators': gen.copy()}
                    p[what][i, c] += s
                    vals.append(_loss_value(p['buses'], p['lines'], p['generators'], tp.slack, (j, k), row.v, row.theta, w, rating, at))
                fd = (vals[0] - vals[1]) / (2 * h)
                err = abs(fd - grad[i, c])
                worst = max(worst, err / (1e-6 * max(1.0, abs(fd))))
                assert err <= 1e-6 * max(1.0, abs(fd)), (what, i, c, fd, grad[i, c])
    print(f'toy pair {pair}: worst error / bar {worst:.3f}, cond {cond:.1f}')
