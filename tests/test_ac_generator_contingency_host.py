"""CPU checks of the AC generator contingency screen's host side (include/gns_powerflow.h, "AC generator contingency screening"):
the analysis without one generator row (``gns_pf_prepare_topology_out_gen``: -1 is the plain analysis byte for byte; roles, the
dimension, the by-bus lists and the shared Y-bus words of every member), the exports, the list builder and the islanding mask, every
refusal of the two C entry points in the order the header states (all come before a launch, so no device is needed), the Python
wrapper's argument errors, the LDS refusal, and the claim the kernel rests on: the row routine of the AC line screens, replayed in
numpy on the blob without generator g, is the reference Newton-Raphson on the grid with the generator row deleted."""
import ctypes
import os

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
from helpers import ROOT
import ac_generator_contingency_reference as gref
import ac_contingency_reference as aref
import pf_topologies as pt
from test_ac_contingency_host import _case14, emulate_row
from test_powerflow_grad_host import H, _arr

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
FIELDS = ('base', 'contingencies', 'v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'worst_line', 'v_min',
          'v_min_bus', 'v_max', 'v_max_bus', 'converged', 'iterations', 'mismatch', 'islanding')


def two_on_a_bus():
    """A ring of five buses with a chord; the slack (bus 1) has one unit, bus 3 has two (rows 1 and 2), bus 5 one."""
    f, t = np.array([1, 2, 3, 4, 5, 2]), np.array([2, 3, 4, 5, 1, 4])
    return pt.Topo('ring5_two_on_a_bus', 5, f, t, np.array([1, 3, 3, 5]), 1)


def _without(tp, g):
    return powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack, out_gen=g)


def _set(topos):
    """(set words, member_off) of the blobs of ``topos`` in the set layout: 16-word aligned offsets."""
    off, words = [], 0
    for tp in topos:
        off.append(words)
        words += (tp.host.size + 15) // 16 * 16
    host = np.zeros(words, dtype=np.int32)
    for o, tp in zip(off, topos):
        host[o:o + tp.host.size] = tp.host
    return host, np.asarray(off, dtype=np.int32)


def test_exports_are_there_and_disjoint():
    lib = amd.load_library()
    assert _lib.ACG1_EXPORTS == ('gns_acg1_workspace_bytes', 'gns_acg1_screen')
    others = (_lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS + _lib.DCN2_EXPORTS +
              _lib.DCN2_ADJOINT_EXPORTS + _lib.ACN1_EXPORTS + _lib.ACN1_ADJOINT_EXPORTS + _lib.ACN2_EXPORTS + _lib.ACN2_ADJOINT_EXPORTS +
              _lib.DCG1_EXPORTS + _lib.DCG1_ADJOINT_EXPORTS)
    hdr = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    topology = ('gns_pf_topology_bytes_out_gen', 'gns_pf_prepare_topology_out_gen', 'gns_pf_topology_slots_out_gen')
    for f in _lib.ACG1_EXPORTS:
        assert f not in others, f
    for f in _lib.ACG1_EXPORTS + topology:
        assert hasattr(lib, f) and getattr(lib, f).restype is ctypes.c_int and f'int {f}(' in hdr, f
    assert set(topology) <= set(_lib.PF_EXPORTS)
    assert 'AC generator contingency screening' in hdr and 'another analysis' not in hdr
    assert callable(powerflow.ac_generator_contingency_screen) and powerflow.AcGeneratorContingencyResult._fields == FIELDS


@pytest.mark.parametrize('name', ['case14', 'ring5_two_on_a_bus', 'random24_stacked_gens'])
def test_minus_one_is_the_plain_analysis_byte_for_byte(name):
    tp = {'case14': _case14(), 'ring5_two_on_a_bus': two_on_a_bus()}.get(name) or pt.families()[name]
    plain = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert plain.host.tobytes() == _without(tp, -1).host.tobytes()
    assert plain.info == _without(tp, -1).info
    lib = amd.load_library()
    f, t, g = (np.ascontiguousarray(a - 1, dtype=np.int32) for a in (tp.f, tp.t, tp.g))
    args = (tp.n, f.size, g.size, f.ctypes.data, t.ctypes.data, g.ctypes.data, tp.slack - 1)
    a, b, sa, sb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.gns_pf_topology_bytes(*args, ctypes.byref(a)) == 0 and lib.gns_pf_topology_bytes_out_gen(*args, -1, ctypes.byref(b)) == 0
    assert a.value == b.value == plain.host.nbytes
    assert lib.gns_pf_topology_slots(*args, ctypes.byref(sa)) == 0 and lib.gns_pf_topology_slots_out_gen(*args, -1, ctypes.byref(sb)) == 0
    assert sa.value == sb.value == plain.info['nnz_lu'] + plain.info['dim']
    for bad in (-2, g.size, g.size + 7):
        assert lib.gns_pf_topology_bytes_out_gen(*args, bad, ctypes.byref(b)) == EINVAL
        assert lib.gns_pf_topology_slots_out_gen(*args, bad, ctypes.byref(sb)) == EINVAL
        assert lib.gns_pf_prepare_topology_out_gen(*args, bad, plain.host.ctypes.data, plain.host.nbytes) == EINVAL
        with pytest.raises(ValueError, match='is not a generator row'):
            _without(tp, bad)
    small = np.zeros(plain.host.size, dtype=np.int32)
    assert lib.gns_pf_prepare_topology_out_gen(*args, 0, small.ctypes.data, 16) == ESIZE


@pytest.mark.parametrize('name', ['case14', 'ring5_two_on_a_bus'])
def test_the_analysis_without_each_generator(name):
    """Roles, the dimension, the by-bus lists and the shared Y-bus words of every member."""
    tp = _case14() if name == 'case14' else two_on_a_bus()
    base = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    w0 = base.host
    N, E, Gn, slack = tp.n, tp.f.size, tp.g.size, tp.slack - 1
    nnzy = int(w0[H['NNZY']])
    gb = tp.g - 1
    freed = 0
    for g in range(Gn):
        member = _without(tp, g)
        w = member.host
        assert (w[H['N']], w[H['E']], w[H['GN']], w[H['SLACK']], w[H['NNZY']]) == (N, E, Gn, slack, nnzy)      # PH_GN stays Gn
        left = [h for h in range(Gn) if h != g]
        want = np.zeros(N, dtype=np.int32)
        want[gb[left]] = 1
        want[slack] = 2
        role = _arr(w, 'ROLE', N)
        assert role.tolist() == want.tolist(), (name, g)
        sole = gb[g] != slack and not np.any(gb[left] == gb[g])
        freed += sole
        assert role[gb[g]] == (2 if gb[g] == slack else 0 if sole else 1)
        assert member.info['dim'] == base.info['dim'] + int(sole), (name, g)
        assert member.info['n_pv'] == base.info['n_pv'] - int(sole) and member.info['n_pq'] == base.info['n_pq'] + int(sole)
        th, vm = _arr(w, 'TH_IDX', N), _arr(w, 'VM_IDX', N)
        assert np.array_equal(vm >= 0, want == 0) and np.array_equal(th >= 0, want != 2)
        assert sorted(np.r_[th[th >= 0], vm[vm >= 0]].tolist()) == list(range(member.info['dim']))
        # the by-bus lists omit g and keep the row numbers, in row order on each bus
        gen_ptr, gen_idx = _arr(w, 'GEN_PTR', N + 1), _arr(w, 'GEN_IDX', max(Gn, 1))
        assert gen_ptr[N] == Gn - 1
        for i in range(N):
            assert gen_idx[gen_ptr[i]:gen_ptr[i + 1]].tolist() == [h for h in left if gb[h] == i], (name, g, i)
        # the Y-bus pattern and its stamps: the same words in every member
        for key, n in (('Y_PTR', N + 1), ('Y_COL', nnzy), ('Y_DIAG', N), ('ST_PTR', nnzy + 1), ('ST', 4 * E)):
            assert np.array_equal(_arr(w, key, n), _arr(w0, key, n)), (name, g, key)
        assert member.info['lds_bytes'] == 8 * (member.info['nnz_lu'] + member.info['dim'] + 8 * N)
    assert freed == (4 if name == 'case14' else 1)


def test_the_list_builder_and_the_islanding_mask():
    tp = _case14()
    E, Gn = tp.f.size, tp.g.size
    rows = powerflow._generator_contingency_list(None, Gn, E)
    assert rows.shape == (Gn * (E + 1), 2) == (105, 2)
    assert rows[:E + 2].tolist() == [[0, k] for k in range(-1, E)] + [[1, -1]]
    dup = powerflow._generator_contingency_list([[2, 5], [2, 5], [0, -1], [2, 5]], Gn, E)
    assert dup.tolist() == [[2, 5], [2, 5], [0, -1], [2, 5]]                     # duplicates are independent rows
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    assert int(bridges.sum()) == 1
    isl = powerflow._generator_islanding(bridges, rows)
    assert int(isl.sum()) == Gn                                                   # one bridge row per generator ...
    assert not isl[rows[:, 1] < 0].any()                                          # ... and a generator outage alone never islands
    assert np.array_equal(isl, (rows[:, 1] >= 0) & bridges[np.maximum(rows[:, 1], 0)])
    for g in range(Gn):                                                          # the reference decides it on the graph
        for k in (-1, 0, int(np.flatnonzero(bridges)[0])):
            buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 1, seed=0)
            b, l, ge = (x[0].double().numpy() for x in (buses, lines, gens))
            row = gref.outage(b, l, ge, slack, g, k, np.ones(14), np.zeros(14), max_iter=0)
            assert (row is None) == bool(k >= 0 and bridges[k])


def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 3)
    E, Gn = lines.shape[1], gens.shape[1]

    def screen(**kw):
        return powerflow.ac_generator_contingency_screen(buses, lines, gens, slack_bus=1, **kw)

    for bad in ([[Gn, 0]], [[-1, 0]], torch.tensor([[0, 0], [Gn + 3, -1]])):
        with pytest.raises(ValueError, match='contingencies must name generators in'):
            screen(contingencies=bad)
    for bad in ([[0, E]], [[0, -2]]):
        with pytest.raises(ValueError, match='contingencies must name lines in'):
            screen(contingencies=bad)
    for bad in ([[0.0, 1.0]], np.array([[True, False]])):
        with pytest.raises(ValueError, match='contingencies must hold integers'):
            screen(contingencies=bad)
    with pytest.raises(ValueError, match='contingencies is empty'):
        screen(contingencies=[])
    for bad in ([0, 1], [[0, 1, 2]]):
        with pytest.raises(ValueError, match=r'contingencies must be a \[P,2\]'):
            screen(contingencies=bad)
    with pytest.raises(ValueError, match="pickup must be None, 'pmax' or weights"):
        screen(pickup='pmin')
    for bad in (torch.ones(Gn - 1), torch.ones(2, Gn)):
        with pytest.raises(ValueError, match='pickup must be'):
            screen(pickup=bad)
    for bad in (-torch.ones(Gn), torch.full((3, Gn), float('inf'))):
        with pytest.raises(ValueError, match='pickup must be non-negative and finite'):
            screen(pickup=bad)
    for bad in (torch.zeros(E), torch.full((3, E), float('nan'))):
        with pytest.raises(ValueError, match='rating must be positive and finite'):
            screen(rating=bad)
    with pytest.raises(ValueError, match='rating must be'):
        screen(rating=torch.ones(E - 1))
    with pytest.raises(ValueError, match='flows must be a bool'):
        screen(flows=1)
    with pytest.raises(ValueError, match='states must be a bool'):
        screen(states=None)
    with pytest.raises(ValueError, match='tol must be'):
        screen(tol=-1e-9)
    with pytest.raises(ValueError, match='max_iter must be'):
        screen(max_iter=2.5)
    with pytest.raises(TypeError):
        screen(differentiable=True)                                              # forward only: there is no such argument
    with pytest.raises(ValueError, match='float32'):
        powerflow.ac_generator_contingency_screen(buses.double(), lines, gens, slack_bus=1)
    with pytest.raises(ValueError, match='batch sizes'):
        powerflow.ac_generator_contingency_screen(buses[:2], lines, gens, slack_bus=1)
    mixed = lines.clone()
    mixed[1, 0, 1] = 5
    with pytest.raises(ValueError, match='differ across the batch: ac_generator_contingency_screen solves one topology'):
        powerflow._topology_key(buses, mixed, gens, 1, 'ac_generator_contingency_screen')


ORDER = ('cfg', 'set_host', 'set_dev', 'set_words', 'off_host', 'off_dev', 'n_member', 'buses', 'lines', 'gens', 'Bt', 'gen_host',
         'gen_dev', 'cols_host', 'cols_dev', 'n_row', 'isl', 'rating', 'per_grid', 'pickup', 'pickup_per_grid', 'base_v', 'base_theta',
         'base_conv', 'v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus',
         'conv', 'iters', 'mis', 'ws', 'ws_bytes')


def _screen(lib, cfg, words, off, gen_list, cols, ws_bytes=None, **kw):
    """gns_acg1_screen on dummy (never dereferenced) device pointers; a keyword replaces one argument.  Only calls the host refuses
    are made."""
    d = words.ctypes.data
    off, gl, c = (np.ascontiguousarray(x, dtype=np.int32) for x in (off, gen_list, cols))
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, set_host=d, set_dev=d, set_words=words.size, off_host=off.ctypes.data,
             off_dev=d, n_member=off.size, buses=d, lines=d, gens=d, Bt=1, gen_host=gl.ctypes.data, gen_dev=d, cols_host=c.ctypes.data,
             cols_dev=d, n_row=c.shape[0], isl=d, rating=None, per_grid=0, pickup=None, pickup_per_grid=0, base_v=d, base_theta=d,
             base_conv=d, v=None, theta=None, p_from=None, q_from=None, p_to=None, q_to=None, worst=d, worst_line=d, v_min=d,
             v_min_bus=d, v_max=d, v_max_bus=d, conv=d, iters=d, mis=d, ws=d, ws_bytes=0 if ws_bytes is None else ws_bytes)
    a.update(kw)
    return lib.gns_acg1_screen(*(a[k] for k in ORDER), None)


def test_entry_points_return_the_documented_codes_before_any_launch():
    lib = amd.load_library()
    tp = _case14()
    E, Gn = tp.f.size, tp.g.size
    cfg = PfConfig(tp.n, E, Gn, 10, 1e-8)
    gens = [1, 3, 4]
    topos = [_without(tp, g) for g in gens]
    set_host, off = _set(topos)
    cols = [[0, -1], [1, 4], [2, 0], [1, -1]]
    d = set_host.ctypes.data
    need, acn1, one = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)

    def query(*args):
        return lib.gns_acg1_workspace_bytes(*args)

    assert query(ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 4, 7, ctypes.byref(need)) == 0
    base = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), base.host.ctypes.data, 4, E, ctypes.byref(acn1)) == 0
    assert need.value == acn1.value >= 4 * 16 * base.info['nnz_ybus']            # gns_acn1_workspace_bytes' figure: one Y-bus per grid
    assert query(ctypes.byref(cfg), d, set_host.size, off.ctypes.data, 1, 4, 1, ctypes.byref(one)) == 0 and one.value == need.value
    for args in ((None, d, set_host.size, off.ctypes.data, off.size, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), None, set_host.size, off.ctypes.data, off.size, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, None, off.size, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, 0, 4, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 0, 7, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 4, 0, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 4, 7, None),
                 (ctypes.byref(cfg), d, int(off[2]) + 8, off.ctypes.data, off.size, 4, 7, ctypes.byref(need))):
        assert query(*args) == EINVAL, args
    # NULL pointers (v, theta, the four flows, the rating and the pickup may be NULL: they are in every call here)
    for name in ('cfg', 'set_host', 'set_dev', 'off_host', 'off_dev', 'buses', 'lines', 'gens', 'gen_host', 'gen_dev', 'cols_host',
                 'cols_dev', 'isl', 'base_v', 'base_theta', 'base_conv', 'worst', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus',
                 'conv', 'iters', 'mis', 'ws'):
        assert _screen(lib, None if name == 'cfg' else cfg, set_host, off, gens, cols, **({} if name == 'cfg' else {name: None})) == EINVAL, name
    # a config that does not match the members, or that gns_pf_solve refuses
    for bad in (PfConfig(tp.n + 1, E, Gn, 10, 1e-8), PfConfig(tp.n, E + 1, Gn, 10, 1e-8), PfConfig(tp.n, E, Gn + 1, 10, 1e-8),
                PfConfig(tp.n, E, Gn, -1, 1e-8), PfConfig(tp.n, E, Gn, 10, -1.0)):
        assert _screen(lib, bad, set_host, off, gens, cols) == EINVAL
    # the set: a misaligned, negative or outlying offset, a set cut short, a fast-decoupled blob, a member of another nnz(Y)
    for bad in ([0, int(off[1]) + 4, int(off[2])], [0, -16, int(off[2])], [0, int(off[1]), set_host.size]):
        assert _screen(lib, cfg, set_host, bad, gens, cols) == EINVAL, bad
    assert _screen(lib, cfg, set_host, off, gens, cols, set_words=int(off[2]) + 8) == EINVAL
    assert _screen(lib, cfg, set_host, off, gens, cols, n_member=0) == EINVAL
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    fd_set, fd_off = _set([topos[0], fd])
    assert _screen(lib, cfg, fd_set, fd_off, [1, 3], [[0, -1]]) == EINVAL
    other = set_host.copy()
    other[off[1] + H['NNZY']] -= 1
    assert _screen(lib, cfg, other, off, gens, cols) == EINVAL
    # the generator list: ascending, distinct, rows of the grid, each member the analysis without its generator
    for bad in ([3, 1, 4], [1, 1, 4], [1, 3, Gn], [-1, 3, 4]):
        assert _screen(lib, cfg, set_host, off, bad, cols) == EINVAL, bad
    assert _screen(lib, cfg, set_host, off, [0, 3, 4], cols) == EINVAL            # member 0 is the analysis without row 1, not row 0
    plain_set, plain_off = _set([base])
    assert _screen(lib, cfg, plain_set, plain_off, [2], [[0, -1]]) == EINVAL      # the plain analysis holds every generator
    six_set, six_off = _set([_without(tp, g) for g in (0, 1, 2, 3, 4, 4)])
    assert _screen(lib, cfg, six_set, six_off, [0, 1, 2, 3, 4, 5], [[0, -1]]) == EINVAL     # more members than generators
    # the rows
    for bad in ([[3, -1]], [[-1, 0]], [[0, E]], [[0, -2]], [[0, 0], [1, 2 ** 31 - 1]]):
        assert _screen(lib, cfg, set_host, off, gens, bad) == EINVAL, bad
    assert _screen(lib, cfg, set_host, off, gens, cols, n_row=0) == EINVAL and _screen(lib, cfg, set_host, off, gens, cols, n_row=-1) == EINVAL
    assert _screen(lib, cfg, set_host, off, gens, cols, Bt=0) == EINVAL and _screen(lib, cfg, set_host, off, gens, cols, Bt=-1) == EINVAL
    assert _screen(lib, cfg, set_host, off, gens, cols, per_grid=2) == EINVAL
    assert _screen(lib, cfg, set_host, off, gens, cols, pickup_per_grid=-1) == EINVAL
    assert _screen(lib, cfg, set_host, off, gens, cols, Bt=0x7FFFFFFF, ws_bytes=2 ** 62) == EINVAL      # more workgroups than one launch takes
    # a short workspace: one byte less than the query asks for; GNS_EINVAL wins
    assert query(ctypes.byref(cfg), d, set_host.size, off.ctypes.data, off.size, 1, 4, ctypes.byref(need)) == 0
    assert _screen(lib, cfg, set_host, off, gens, cols, ws_bytes=need.value - 1) == ESIZE
    assert _screen(lib, cfg, set_host, off, gens, [[0, E]], ws_bytes=need.value - 1) == EINVAL


def test_a_chain_whose_image_does_not_fit_is_refused_by_name():
    """One member above the limit refuses the whole call (GNS_EUNSUPPORTED), after GNS_EINVAL and GNS_ESIZE; the Python wrapper names
    the largest member's image with Newton-Raphson's message."""
    lib = amd.load_library()
    tp = pt.path(4096)
    member = _without(tp, 0)
    assert member.info['lds_bytes'] > pt.LDS_LIMIT and member.info['dim'] == 2 * 4095
    set_host, off = _set([member])
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
    need = ctypes.c_size_t(0)
    assert lib.gns_acg1_workspace_bytes(ctypes.byref(cfg), set_host.ctypes.data, set_host.size, off.ctypes.data, 1, 1, 1,
                                        ctypes.byref(need)) == 0
    assert _screen(lib, cfg, set_host, off, [0], [[0, -1]], ws_bytes=need.value) == EUNSUPPORTED
    assert _screen(lib, cfg, set_host, off, [0], [[0, -1]], ws_bytes=need.value - 1) == ESIZE          # GNS_ESIZE wins, as in gns_acn1_screen
    assert _screen(lib, cfg, set_host, off, [0], [[0, tp.f.size]], ws_bytes=need.value) == EINVAL
    assert powerflow._set_lds_bytes(set_host, off) == member.info['lds_bytes']
    with pytest.raises(amd.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_acg1_screen', lambda: powerflow._set_lds_bytes(set_host, off), powerflow._ACG1.formula)
    assert 'nnz(L+U) + dim + 8 N' in str(e.value) and str(member.info['lds_bytes']) in str(e.value)


@pytest.mark.parametrize('name', ['case14', 'ring5_two_on_a_bus'])
def test_the_blob_without_the_generator_serves_its_rows(name):
    """The row routine of the AC line screens, replayed in numpy (``test_ac_contingency_host.emulate_row``) on the blob without
    generator g and the remaining generators' table, against the reference on the grid with the generator row (and the line row)
    deleted: the same convergence and iteration count, v and theta within 1e-9, wherever the reference converges with two
    iterations to spare.  The pickup is the reference's own here: it only changes Pg."""
    if name == 'case14':
        tp = _case14()
        buses, lines, gens, _, _, _ = synth.solvable_grids(14, 2, seed=0)
    else:
        tp = two_on_a_bus()
        buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0)
        gens = gens.clone()
        gens[:, 2, 4] = gens[:, 1, 4] + 0.02                                     # the second unit of bus 3 holds another set point
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    n_cmp = n_rows = 0
    for g in range(tp.g.size):
        w = _without(tp, g).host
        for i in range(2):
            b, l, ge = (x[i].double().numpy() for x in (buses, lines, gens))
            v0, th0, conv, _, _ = aref.base_case(b, l, ge, tp.slack)
            assert conv
            for pick in (None, 'pmax'):
                rest = gref.without(ge, g, gref.weights(pick, ge))
                for k in (-1, *range(0, tp.f.size, 3)):
                    want = gref.outage(b, l, ge, tp.slack, g, k, v0, th0, gref.weights(pick, ge))
                    assert (want is None) == bool(k >= 0 and bridges[k])
                    if want is None:
                        continue
                    n_rows += 1
                    if not (want.converged and want.iterations <= 8):
                        continue
                    n_cmp += 1
                    vm, va, got_conv, it, mis = emulate_row(w, b, l, rest, k if k >= 0 else [], v0, th0)
                    assert got_conv and it == want.iterations and mis < 1e-8, (name, g, i, k, it, want.iterations)
                    assert np.max(np.abs(vm - want.v)) <= 1e-9 and np.max(np.abs(va - want.theta)) <= 1e-9, (name, g, i, k)
    print(f'{name}: {n_cmp} of {n_rows} non-islanding rows compared')
    assert n_cmp >= 0.5 * n_rows, (name, n_cmp, n_rows)


@pytest.mark.parametrize('regime', pt.REGIMES)
@pytest.mark.parametrize('name', ['toy', 'random24_stacked_gens', 'random40_parallel_selfloop', 'ring63'])
def test_zero_and_one_step_of_the_replay_on_every_listed_row(name, regime):
    """The replay on the blob without generator g from a start with base_theta[slack] = 0.3, on EVERY non-islanding row of
    ``ac_generator_rows.rows_list`` (no convergence needed), the pickup shared by random weights: after zero steps the state is the
    reference start on the grid without the unit exactly and the mismatch is the reference's to ``_mismatch_and_bar``; one step
    solves the reference Jacobian of the grid without the unit and the line to ``pt.STEP_TOL``, scipy's own step asserted first as
    the guard.  Pins "the blob without the generator serves its rows" at 100 %: toy 32, random24_stacked_gens 444,
    random40_parallel_selfloop 460 and ring63 390 rows of two grids."""
    from ac_generator_rows import pickup_weights, row_reference, rows_islanding, rows_list, topology
    from test_ac_contingency_host import one_step_ratios, shifted_base
    from test_ac_contingency_rows_gpu import _mismatch_and_bar
    from types import SimpleNamespace
    tp = topology(name)
    buses, lines, gens, v, theta = pt.grids(tp, regime, 2, seed=11)
    b, l, ge = (x.double().numpy() for x in (buses, lines, gens))
    base_v, base_theta = shifted_base(tp, v, theta)
    s = SimpleNamespace(tp=tp, b=b, l=l, g=ge, base_v=base_v, base_theta=base_theta)
    rows = rows_list(tp)
    isl = rows_islanding(tp, rows)
    pick = pickup_weights('random', 2, tp.g.size)
    n_cmp, worst = 0, 0.0
    for i in range(2):
        assert base_theta[i, tp.slack - 1] == 0.3
        for (g, k), island in zip(rows, isl):
            if island:
                continue
            w = _without(tp, g).host
            view, out = row_reference(s, i, g, k, pick[i])
            rest, (vm0, va0) = view.g[i], view.starts[i]
            z = emulate_row(w, b[i], l[i], rest, out, base_v[i], base_theta[i], tol=0.0, max_iter=0)
            assert np.array_equal(z[0], vm0) and np.array_equal(z[1], va0) and z[3] == 0, (name, i, g, k)
            want, bar = _mismatch_and_bar(b[i], l[i], rest, tp.slack, out, vm0, va0)
            assert abs(z[4] - want) <= bar, (name, i, g, k, z[4], want, bar)
            v1, th1, conv, it, _ = emulate_row(w, b[i], l[i], rest, out, base_v[i], base_theta[i], tol=0.0, max_iter=1)
            assert it == 1 and not conv, (name, i, g, k)
            r_scipy, r_replay = one_step_ratios(b[i], l[i], rest, tp.slack, out, vm0, va0, v1, th1)
            assert r_scipy <= pt.STEP_TOL, (name, regime, i, g, k, r_scipy)
            assert r_replay <= pt.STEP_TOL, (name, regime, i, g, k, r_replay)
            worst = max(worst, r_replay)
            n_cmp += 1
    print(f'{name} ({regime}): {n_cmp} of {2 * int((~isl).sum())} non-islanding rows compared, worst one-step ratio {worst:.1e}')
    assert n_cmp == 2 * int((~isl).sum()) > 0
