"""CPU checks of the host side of the AC generator screen's adjoint (include/gns_powerflow.h, "Gradients of the AC generator
screen"): the new exports and their argument types, the workspace formula and the chunk rule, the refusals of the two entry points in
the documented order (on dummy pointers: nothing is launched), the Python refusals of
``ac_generator_contingency_screen_differentiable`` and the error where no device is visible, and the float64 reference
(``ac_generator_contingency_grad_reference``) against central finite differences of the reference solve on the ring with two units
on one bus: a sole unit out, the first-listed unit of the shared bus out, the slack's unit out with pickup weights, and a row with a
line."""
import ctypes
import inspect
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
import ac_generator_contingency_grad_reference as ggref
import ac_generator_contingency_reference as agref
import pf_topologies as pt
from test_ac_contingency_host import _case14
from test_ac_generator_contingency_host import ORDER as SCREEN_ORDER
from test_ac_generator_contingency_host import _set, _without, two_on_a_bus
from test_powerflow_grad_host import H

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
NEW = ('gns_acg1_adjoint_workspace_bytes', 'gns_acg1_adjoint')
# gns_acg1_screen's arguments up to pickup_per_grid, the forward's state, the nine incoming gradients, the four outputs
ARGS = SCREEN_ORDER[:SCREEN_ORDER.index('pickup_per_grid') + 1] + (
    'v', 'theta', 'conv', 'worst_line', 'v_min_bus', 'v_max_bus', 'base_conv', 'g_v', 'g_theta', 'g_p_from', 'g_q_from', 'g_p_to',
    'g_q_to', 'g_worst', 'g_v_min', 'g_v_max', 'gb', 'gl', 'gg', 'gp', 'ws', 'ws_bytes')
INTS = {'set_words': ctypes.c_size_t, 'n_member': ctypes.c_int32, 'Bt': ctypes.c_int64, 'n_row': ctypes.c_int32,
        'per_grid': ctypes.c_int32, 'pickup_per_grid': ctypes.c_int32, 'ws_bytes': ctypes.c_size_t}


def test_exports_are_there_with_their_argument_types():
    lib = amd.load_library()
    assert _lib.ACG1_ADJOINT_EXPORTS == NEW
    assert _lib.ACG1_EXPORTS == ('gns_acg1_workspace_bytes', 'gns_acg1_screen')
    others = (_lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.DCN2_EXPORTS +
              _lib.DCN2_ADJOINT_EXPORTS + _lib.ACN1_EXPORTS + _lib.ACN1_ADJOINT_EXPORTS + _lib.ACN2_EXPORTS + _lib.ACN2_ADJOINT_EXPORTS +
              _lib.DCG1_EXPORTS + _lib.DCG1_ADJOINT_EXPORTS + _lib.ACG1_EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    for f in NEW:
        assert hasattr(lib, f) and f not in others, f
        assert getattr(lib, f).restype is ctypes.c_int and f'int {f}(' in hdr
    assert 'Gradients of the AC generator screen' in hdr and 'no gradients yet' not in hdr
    assert lib.gns_acg1_adjoint_workspace_bytes.argtypes == lib.gns_acg1_workspace_bytes.argtypes
    at = lib.gns_acg1_adjoint.argtypes
    assert len(at) == len(ARGS) + 1                                     # and the stream
    for k, name in enumerate(ARGS):
        want = INTS.get(name, ctypes.c_void_p)
        assert name == 'cfg' or at[k] is want, (name, at[k])
    # the same prefix as the screen's call
    n = ARGS.index('pickup_per_grid') + 1
    assert at[:n] == lib.gns_acg1_screen.argtypes[:n]
    assert callable(powerflow.ac_generator_contingency_screen_differentiable)
    plain = inspect.signature(powerflow.ac_generator_contingency_screen)
    assert inspect.signature(powerflow.ac_generator_contingency_screen_differentiable) == plain and 'differentiable' not in plain.parameters


def _adjoint(lib, cfg, words, off, gen_list, cols, **kw):
    """gns_acg1_adjoint on dummy (never dereferenced) device pointers; a keyword replaces one argument.  Only calls the host refuses,
    or that have nothing to launch, are made."""
    d = words.ctypes.data
    off, gl, c = (np.ascontiguousarray(x, dtype=np.int32) for x in (off, gen_list, cols))
    a = {k: d for k in ARGS}
    a.update(cfg=ctypes.byref(cfg) if cfg is not None else None, set_words=words.size, off_host=off.ctypes.data, n_member=off.size, Bt=1,
             gen_host=gl.ctypes.data, cols_host=c.ctypes.data, n_row=c.shape[0], rating=None, per_grid=0, pickup=None, pickup_per_grid=0,
             ws_bytes=0, **{k: None for k in ARGS if k.startswith('g_')})
    a.update(kw)
    return lib.gns_acg1_adjoint(*(a[k] for k in ARGS), None)


def _partial(tp):
    """Doubles of one (grid, chunk) partial: four per bus, five per line, four per generator row and the status."""
    return 4 * tp.n + 5 * tp.f.size + 4 * tp.g.size + 1


def _chunk(P):
    """Rows a wave walks: a wave per row up to 64 rows, then ceil(P / 64), without a cap (the N-2 adjoint's rule)."""
    return max(1, -(-P // 64))


def test_workspace_formula_and_chunk_rule():
    lib = amd.load_library()
    need, fwd = ctypes.c_size_t(0), ctypes.c_size_t(0)
    up = lambda x: (x + 255) // 256 * 256                               # noqa: E731
    for tp in (_case14(), two_on_a_bus()):
        base = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
        cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
        set_host, off = _set([_without(tp, g) for g in range(tp.g.size)])
        args = (ctypes.byref(cfg), set_host.ctypes.data, set_host.size, off.ctypes.data, off.size)
        for Bt in (1, 3, 64):
            for P in (1, 64, 65, 105, 127, 10098):
                assert lib.gns_acg1_adjoint_workspace_bytes(*args, Bt, P, ctypes.byref(need)) == 0
                assert lib.gns_acg1_workspace_bytes(*args, Bt, P, ctypes.byref(fwd)) == 0
                nchunks = -(-P // _chunk(P))
                assert fwd.value == up(Bt * 16 * base.info['nnz_ybus'])
                assert need.value == fwd.value + up(Bt * nchunks * 8 * _partial(tp)), (tp.name, Bt, P)
                assert nchunks <= 64                                      # per grid at most 64 partials, whatever P is
        # the figure does not depend on how many members the set holds
        assert lib.gns_acg1_adjoint_workspace_bytes(*args[:4], 1, 3, 20, ctypes.byref(fwd)) == 0
        assert lib.gns_acg1_adjoint_workspace_bytes(*args, 3, 20, ctypes.byref(need)) == 0 and need.value == fwd.value
    # the chunk comes from the list's length alone: C and the chunks per grid; 127 rows leave a last chunk of one row
    assert [_chunk(p) for p in (1, 64, 65, 105, 127, 128, 129, 10098)] == [1, 1, 2, 2, 2, 2, 3, 158]
    assert [-(-p // _chunk(p)) for p in (1, 64, 65, 105, 127, 128, 129, 10098)] == [1, 64, 33, 53, 64, 64, 43, 64]


def test_entry_points_refuse_in_the_documented_order_before_any_launch():
    lib = amd.load_library()
    tp = _case14()
    E, Gn = tp.f.size, tp.g.size
    cfg = PfConfig(tp.n, E, Gn, 10, 1e-8)
    gens = [1, 3, 4]
    set_host, off = _set([_without(tp, g) for g in gens])
    cols = [[0, -1], [1, 4], [2, 0], [1, -1]]
    d = set_host.ctypes.data
    need = ctypes.c_size_t(0)
    query = lib.gns_acg1_adjoint_workspace_bytes
    for args in ((None, d, set_host.size, off.ctypes.data, off.size, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), None, set_host.size, off.ctypes.data, off.size, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, None, off.size, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, 0, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 0, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 4, 0, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 4, 7, None),
                 (ctypes.byref(cfg), d, int(off[2]) + 8, off.ctypes.data, off.size, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 0x7FFFFFFF, 2, ctypes.byref(need))):
        assert query(*args) == EINVAL, args
    # 1. the arguments: NULL pointers (the rating, the pickup, every incoming gradient and every gradient output may be NULL)
    for name in ('cfg', 'set_host', 'set_dev', 'off_host', 'off_dev', 'buses', 'lines', 'gens', 'gen_host', 'gen_dev', 'cols_host',
                 'cols_dev', 'isl', 'v', 'theta', 'conv', 'worst_line', 'v_min_bus', 'v_max_bus', 'base_conv', 'ws'):
        assert _adjoint(lib, None if name == 'cfg' else cfg, set_host, off, gens, cols,
                        **({} if name == 'cfg' else {name: None})) == EINVAL, name
    for bad in (PfConfig(tp.n, E, Gn, -1, 1e-8), PfConfig(tp.n, E, Gn, 10, -1.0)):
        assert _adjoint(lib, bad, set_host, off, gens, cols) == EINVAL
    assert _adjoint(lib, cfg, set_host, off, gens, cols, n_row=0) == EINVAL and _adjoint(lib, cfg, set_host, off, gens, cols, n_row=-1) == EINVAL
    assert _adjoint(lib, cfg, set_host, off, gens, cols, Bt=0) == EINVAL and _adjoint(lib, cfg, set_host, off, gens, cols, Bt=-1) == EINVAL
    assert _adjoint(lib, cfg, set_host, off, gens, cols, per_grid=2) == EINVAL
    assert _adjoint(lib, cfg, set_host, off, gens, cols, pickup_per_grid=-1) == EINVAL
    # every check passed but the workspace's size; one byte short; GNS_EINVAL wins over it
    assert _adjoint(lib, cfg, set_host, off, gens, cols) == ESIZE
    assert query(ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 1, 4, ctypes.byref(need)) == 0
    assert _adjoint(lib, cfg, set_host, off, gens, cols, ws_bytes=need.value - 1) == ESIZE
    assert _adjoint(lib, cfg, set_host, off, gens, [[0, E]], ws_bytes=need.value - 1) == EINVAL
    # nothing asked for: nothing launched, after every other check
    none = dict(gb=None, gl=None, gg=None, gp=None)
    assert _adjoint(lib, cfg, set_host, off, gens, cols, **none) == 0
    assert _adjoint(lib, cfg, set_host, off, gens, cols, ws=None, **none) == 0
    assert _adjoint(lib, cfg, set_host, off, gens, cols, gb=None, gl=None, gg=None) == ESIZE      # the weights' gradient alone is an output
    # 2. the set scan: a config that does not match the members, a misaligned, negative or outlying offset, a set cut short, a
    # fast-decoupled blob, a member of another nnz(Y); with nothing asked for too
    for bad in (PfConfig(tp.n + 1, E, Gn, 10, 1e-8), PfConfig(tp.n, E + 1, Gn, 10, 1e-8), PfConfig(tp.n, E, Gn + 1, 10, 1e-8)):
        assert _adjoint(lib, bad, set_host, off, gens, cols, ws_bytes=2 ** 40) == EINVAL
    for bad in ([0, int(off[1]) + 4, int(off[2])], [0, -16, int(off[2])], [0, int(off[1]), set_host.size]):
        assert _adjoint(lib, cfg, set_host, bad, gens, cols, ws_bytes=2 ** 40) == EINVAL, bad
        assert _adjoint(lib, cfg, set_host, bad, gens, cols, **none) == EINVAL, bad
    assert _adjoint(lib, cfg, set_host, off, gens, cols, set_words=int(off[2]) + 8) == EINVAL
    assert _adjoint(lib, cfg, set_host, off, gens, cols, n_member=0) == EINVAL
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    fd_set, fd_off = _set([_without(tp, 1), fd])
    assert _adjoint(lib, cfg, fd_set, fd_off, [1, 3], [[0, -1]], ws_bytes=2 ** 40) == EINVAL
    other = set_host.copy()
    other[off[1] + H['NNZY']] -= 1
    assert _adjoint(lib, cfg, other, off, gens, cols, ws_bytes=2 ** 40) == EINVAL
    # 3. the lists: the generators ascending, distinct, rows of the grid, each member the analysis without its generator and its
    # by-bus lists generator rows; the rows positions into them and lines or -1
    for bad in ([3, 1, 4], [1, 1, 4], [1, 3, Gn], [-1, 3, 4], [0, 3, 4]):
        assert _adjoint(lib, cfg, set_host, off, bad, cols, ws_bytes=2 ** 40) == EINVAL, bad
    base = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    plain_set, plain_off = _set([base])
    assert _adjoint(lib, cfg, plain_set, plain_off, [2], [[0, -1]], ws_bytes=2 ** 40) == EINVAL
    wild = set_host.copy()
    wild[off[0] + wild[off[0] + H['GEN_IDX']]] = Gn + 3                  # a by-bus entry that is no generator row
    assert _adjoint(lib, cfg, wild, off, gens, cols, ws_bytes=2 ** 40) == EINVAL
    for bad in ([[3, -1]], [[-1, 0]], [[0, E]], [[0, -2]], [[0, 0], [1, 2 ** 31 - 1]]):
        assert _adjoint(lib, cfg, set_host, off, gens, bad, ws_bytes=2 ** 40) == EINVAL, bad
        assert _adjoint(lib, cfg, set_host, off, gens, bad, **none) == EINVAL, bad
    # 4. the chunks: more workgroups than one launch takes
    assert _adjoint(lib, cfg, set_host, off, gens, cols, Bt=0x7FFFFFFF, ws_bytes=2 ** 62) == EINVAL


def test_lds_refusal_comes_from_the_query_too_and_before_nothing_asked_for():
    """5. the LDS image of the largest member: after every GNS_EINVAL, before "nothing asked for" and before GNS_ESIZE; from the
    adjoint's workspace query too (the forward's query does not refuse it), so the Python wrapper can name it before any launch."""
    lib = amd.load_library()
    tp = pt.path(4096)
    member = _without(tp, 0)
    assert member.info['lds_bytes'] > pt.LDS_LIMIT
    set_host, off = _set([member])
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
    need = ctypes.c_size_t(0)
    args = (ctypes.byref(cfg), set_host.ctypes.data, set_host.size, off.ctypes.data, 1, 1, 1, ctypes.byref(need))
    assert lib.gns_acg1_workspace_bytes(*args) == 0
    assert lib.gns_acg1_adjoint_workspace_bytes(*args) == EUNSUPPORTED
    assert _adjoint(lib, cfg, set_host, off, [0], [[0, -1]], ws_bytes=2 ** 40) == EUNSUPPORTED
    assert _adjoint(lib, cfg, set_host, off, [0], [[0, -1]], ws_bytes=0) == EUNSUPPORTED               # before GNS_ESIZE
    assert _adjoint(lib, cfg, set_host, off, [0], [[0, -1]], gb=None, gl=None, gg=None, gp=None) == EUNSUPPORTED
    assert _adjoint(lib, cfg, set_host, off, [0], [[0, tp.f.size]], ws_bytes=2 ** 40) == EINVAL        # GNS_EINVAL wins
    assert _adjoint(lib, cfg, set_host, off, [1], [[0, -1]], ws_bytes=2 ** 40) == EINVAL
    with pytest.raises(amd.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_acg1_adjoint_workspace_bytes', lambda: powerflow._set_lds_bytes(set_host, off),
                         powerflow._ACG1.formula)
    assert 'nnz(L+U) + dim + 8 N' in str(e.value) and str(member.info['lds_bytes']) in str(e.value)


def test_python_refusals_come_before_a_device_is_needed():
    buses, lines, gens = synth.synth_grids(14, 2)
    E, Gn = lines.shape[1], gens.shape[1]

    def screen(**kw):
        return powerflow.ac_generator_contingency_screen_differentiable(buses, lines.clone().requires_grad_(True), gens, slack_bus=1, **kw)

    with pytest.raises(ValueError, match='contingencies is empty'):
        screen(contingencies=[])
    with pytest.raises(ValueError, match=r'contingencies must be a \[P,2\]'):
        screen(contingencies=[0, 1])
    with pytest.raises(ValueError, match='contingencies must hold integers'):
        screen(contingencies=[[0, 1.5]])
    with pytest.raises(ValueError, match='contingencies must name generators in'):
        screen(contingencies=[[Gn, 0]])
    with pytest.raises(ValueError, match='contingencies must name lines in'):
        screen(contingencies=[[0, E]])
    with pytest.raises(ValueError, match="pickup must be None, 'pmax' or weights"):
        screen(pickup='pmin')
    with pytest.raises(ValueError, match='pickup must be non-negative and finite'):
        screen(pickup=(-torch.ones(Gn)).requires_grad_(True))
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
            screen(contingencies=[[0, -1]])


# ---- the reference against central finite differences of the reference solve

def _ring():
    """One grid on the ring with two units on bus 3 (rows 1 and 2, with different set points) in float64 numpy."""
    tp = two_on_a_bus()
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, 0)
    bus, ln, gen = (x[0].double().numpy().copy() for x in (buses, lines, gens))
    gen[2, 4] = gen[1, 4] + 0.02
    return tp, bus, ln, gen


def _loss_value(bus, ln, gen, slack, g, k, pw, v0, th0, w, rating, at):
    row = agref.outage(bus, ln, gen, slack, g, k, v0, th0, pw, 1e-13, 30)
    assert row is not None and row.converged
    val = sum(float(np.dot(w[n], getattr(row, n))) for n in ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to'))
    sf, st = np.hypot(row.p_from, row.q_from), np.hypot(row.p_to, row.q_to)
    wi = at['worst_line']
    val += w['worst_loading'] * (sf[wi] if at['from_end'] else st[wi]) / rating[wi]
    return val + w['v_min'] * row.v[at['v_min_bus']] + w['v_max'] * row.v[at['v_max_bus']]


@pytest.mark.parametrize('g,k,weighted', [(3, -1, False), (1, -1, False), (0, -1, True), (3, 1, True), (2, 5, True)],
                         ids=['sole_unit', 'first_of_shared_bus', 'slack_unit_with_weights', 'sole_unit_and_line',
                              'second_of_shared_bus_and_line'])
def test_reference_agrees_with_central_differences_on_the_ring_with_two_units_on_a_bus(g, k, weighted):
    """Generator 3 is alone on bus 5 (the bus turns PQ: Qd and Bs take a gradient, no vg does), generators 1 and 2 share bus 3 (row 1
    out: the set point, and the vg gradient, move to row 2), generator 0 is the slack's (with weights the others pick its Pg up, so
    its Pg takes a gradient).  All nine outputs are weighted; the summaries' indices are frozen at the unperturbed row's."""
    tp, bus, ln, gen = _ring()
    rng = np.random.default_rng(10 * g + k + 7)
    N, E, Gn = tp.n, tp.f.size, tp.g.size
    pw = 0.5 + rng.random(Gn) if weighted else None
    w = dict(v=rng.standard_normal(N), theta=rng.standard_normal(N), worst_loading=float(rng.standard_normal()),
             v_min=float(rng.standard_normal()), v_max=float(rng.standard_normal()),
             **{n: rng.standard_normal(E) for n in ('p_from', 'q_from', 'p_to', 'q_to')})
    rating = 0.5 + 2.0 * rng.random(E)
    base = aref.base_case(bus, ln, gen, tp.slack, 1e-13, 30)
    row = agref.outage(bus, ln, gen, tp.slack, g, k, base[0], base[1], pw, 1e-13, 30)
    assert row is not None and row.converged
    wi = int(np.argmax(aref.loading(row, rating)))
    assert wi != k
    at = dict(worst_line=wi, from_end=bool(np.hypot(row.p_from[wi], row.q_from[wi]) >= np.hypot(row.p_to[wi], row.q_to[wi])),
              v_min_bus=int(np.argmin(row.v)), v_max_bus=int(np.argmax(row.v)))
    (gb, gl, gg, gw), cond = ggref.row_gradient(bus, ln, gen, tp.slack, g, k, row, w, pw, rating)
    # what the contract says of the lost unit and of the row's own line
    assert gg[g, 4] == 0.0 and gw[g] == 0.0 and (k < 0 or np.all(gl[k] == 0.0)) and np.any(gl != 0.0)
    if weighted:
        assert gg[g, 6] != 0.0 and np.all(gw[[h for h in range(Gn) if h != g]] != 0.0)
    else:
        assert gg[g, 6] == 0.0 and np.all(gw == 0.0)
    if g == 3:                                           # the freed bus 5: a Q equation there, no set point
        assert gb[4, 3] != 0.0 and gb[4, 5] != 0.0
    if g == 1:                                           # the set point of bus 3 is row 2's
        assert gg[2, 4] != 0.0
    if g == 2:                                           # row 1 stays the first listed
        assert gg[1, 4] != 0.0
    h = 1e-6
    worst = 0.0
    tables = (('buses', bus, gb), ('lines', ln, gl), ('generators', gen, gg)) + ((('weights', pw[:, None], gw[:, None]),) if weighted else ())
    for what, arr, grad in tables:
        for c in range(arr.shape[1]):
            if what != 'weights' and c not in ggref.DIFF_COLS[what]:
                assert np.all(grad[:, c] == 0.0), (what, c)
                continue
            for i in range(arr.shape[0]):
                vals = []
                for s in (+h, -h):
                    p = {'buses': bus.copy(), 'lines': ln.copy(), 'generators': gen.copy(), 'weights': None if pw is None else pw[:, None].copy()}
                    p[what][i, c] += s
                    vals.append(_loss_value(p['buses'], p['lines'], p['generators'], tp.slack, g, k,
                                            None if pw is None else p['weights'][:, 0], row.v, row.theta, w, rating, at))
                fd = (vals[0] - vals[1]) / (2 * h)
                err = abs(fd - grad[i, c])
                worst = max(worst, err / (1e-6 * max(1.0, abs(fd))))
                assert err <= 1e-6 * max(1.0, abs(fd)), (what, i, c, fd, grad[i, c])
    print(f'ring (g, k) = ({g}, {k}): worst error / bar {worst:.3f}, cond {cond:.1f}')
