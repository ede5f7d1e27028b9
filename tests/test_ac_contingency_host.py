"""CPU checks of the AC contingency screen's host side (include/gns_powerflow.h, "AC contingency screening"): the exports, the
argument checks of the Python wrapper and of the C entry points (every refusal comes before a launch, so no device is needed), the
claim the kernel rests on, that the Y-bus summed from the base pattern's stamps without one line's is the Y-bus of the grid with the
line's row deleted (in the reference and from the blob's own stamp lists), and the reference's branch flows against the bus balance."""
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
import ac_contingency_reference as aref
import nr_reference as nr
import pf_topologies as pt
from test_powerflow_grad_host import H, _arr

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
FIELDS = ('base', 'outages', 'v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'worst_line', 'v_min', 'v_min_bus',
          'v_max', 'v_max_bus', 'converged', 'iterations', 'mismatch', 'islanding')


def toy():
    """Five buses on a ring, a second line between buses 1 and 2 (listed the other way round) and a line from bus 3 to itself: no
    line is a bridge."""
    f, t = np.array([1, 2, 3, 4, 5, 2, 3]), np.array([2, 3, 4, 5, 1, 1, 3])
    return pt.Topo('toy_parallel_selfloop', 5, f, t, np.array([1, 3]), 1)


def _case14():
    f, t, g = synth.case_topology(14)
    return pt.Topo('case14', 14, f, t, g, synth._solvable_slack(14))


def test_exports_are_there_and_disjoint():
    lib = amd.load_library()
    assert _lib.ACN1_EXPORTS == ('gns_acn1_workspace_bytes', 'gns_acn1_screen')
    others = _lib.EXPORTS + _lib.PF_EXPORTS + _lib.FD_EXPORTS + _lib.DC_EXPORTS + _lib.DCN1_EXPORTS
    for f in _lib.ACN1_EXPORTS:
        assert hasattr(lib, f) and f not in others, f
        assert getattr(lib, f).restype is ctypes.c_int
    hdr = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    for f in _lib.ACN1_EXPORTS:
        assert f'int {f}(' in hdr
    assert callable(powerflow.ac_contingency_screen) and powerflow.AcContingencyResult._fields == FIELDS


def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 3)
    E = lines.shape[1]

    def screen(**kw):
        return powerflow.ac_contingency_screen(buses, lines, gens, slack_bus=1, **kw)

    for bad in ([E], [-1], [0, E + 5], torch.tensor([0, E])):
        with pytest.raises(ValueError, match='outages must lie in'):
            screen(outages=bad)
    for bad in ([0.0, 1.0], [1.5], np.array([True, False])):
        with pytest.raises(ValueError, match='outages must hold integers'):
            screen(outages=bad)
    for bad in ([], range(0)):
        with pytest.raises(ValueError, match='outages is empty'):
            screen(outages=bad)
    with pytest.raises(ValueError, match='1-D'):
        screen(outages=[[0, 1]])
    for bad in (torch.zeros(E), -torch.ones(E), torch.full((3, E), float('nan'))):
        with pytest.raises(ValueError, match='rating must be positive and finite'):
            screen(rating=bad)
    for bad in (torch.ones(E - 1), torch.ones(2, E), 1.0):
        with pytest.raises(ValueError, match='rating must be'):
            screen(rating=bad)
    with pytest.raises(ValueError, match='flows must be a bool'):
        screen(flows=1)
    with pytest.raises(ValueError, match='states must be a bool'):
        screen(states=None)
    for bad in (-1e-9, float('nan')):
        with pytest.raises(ValueError, match='tol must be'):
            screen(tol=bad)
    for bad in (-1, 2.5, None):
        with pytest.raises(ValueError, match='max_iter must be'):
            screen(max_iter=bad)
    with pytest.raises(ValueError, match='float32'):
        powerflow.ac_contingency_screen(buses.double(), lines, gens, slack_bus=1)
    with pytest.raises(ValueError, match='batch sizes'):
        powerflow.ac_contingency_screen(buses[:2], lines, gens, slack_bus=1)
    with pytest.raises(ValueError, match='2-D .* or all 3-D'):
        powerflow.ac_contingency_screen(buses[0], lines, gens, slack_bus=1)
    mixed = lines.clone()
    mixed[1, 0, 1] = 5
    with pytest.raises(ValueError, match='differ across the batch: ac_contingency_screen solves one topology'):
        powerflow._topology_key(buses, mixed, gens, 1, 'ac_contingency_screen')


def _screen(lib, cfg, blob, outages, ws_bytes=None, **kw):
    """gns_acn1_screen on dummy (never dereferenced) device pointers; a keyword replaces one argument.  Only calls the host refuses
    are made."""
    d = blob.ctypes.data
    o = np.asarray(outages, dtype=np.int32)
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, out_host=o.ctypes.data,
             out_dev=d, K=o.size, isl=d, rating=None, per_grid=0, base_v=d, base_theta=d, base_conv=d, v=None, theta=None,
             p_from=None, q_from=None, p_to=None, q_to=None, worst=d, worst_line=d, v_min=d, v_min_bus=d, v_max=d, v_max_bus=d, conv=d,
             iters=d, mis=d, ws=d, ws_bytes=0 if ws_bytes is None else ws_bytes)
    a.update(kw)
    return lib.gns_acn1_screen(*(a[k] for k in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'Bt', 'out_host', 'out_dev', 'K', 'isl',
                                                'rating', 'per_grid', 'base_v', 'base_theta', 'base_conv', 'v', 'theta', 'p_from',
                                                'q_from', 'p_to', 'q_to', 'worst', 'worst_line', 'v_min', 'v_min_bus', 'v_max',
                                                'v_max_bus', 'conv', 'iters', 'mis', 'ws', 'ws_bytes')), None)


def test_entry_points_return_the_documented_codes_before_any_launch():
    lib = amd.load_library()
    tp = _case14()
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    E = tp.f.size
    cfg = PfConfig(tp.n, E, tp.g.size, 10, 1e-8)
    d = topo.host.ctypes.data
    need, plain = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), d, 4, E, ctypes.byref(need)) == 0
    assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), d, 4, ctypes.byref(plain)) == 0
    assert need.value == plain.value >= 4 * 16 * topo.info['nnz_ybus']          # one base Y-bus per grid ...
    one = ctypes.c_size_t(0)
    assert lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), d, 4, 1, ctypes.byref(one)) == 0 and one.value == need.value   # ... not per pair
    for args in ((None, d, 4, E, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, None), (ctypes.byref(cfg), d, 0, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, -3, ctypes.byref(need))):
        assert lib.gns_acn1_workspace_bytes(*args) == EINVAL, args
    # NULL pointers (v, theta, the four flows and the rating may be NULL: they are in every call here)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'out_host', 'out_dev', 'isl', 'base_v', 'base_theta', 'base_conv',
                 'worst', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus', 'conv', 'iters', 'mis', 'ws'):
        assert _screen(lib, None if name == 'cfg' else cfg, topo.host, [0, 3], **({} if name == 'cfg' else {name: None})) == EINVAL, name
    # a config that does not match the blob, or that gns_pf_solve refuses
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8), PfConfig(tp.n, E + 1, tp.g.size, 10, 1e-8),
                PfConfig(tp.n, E, tp.g.size + 1, 10, 1e-8), PfConfig(tp.n, E, tp.g.size, -1, 1e-8),
                PfConfig(tp.n, E, tp.g.size, 10, -1.0)):
        assert _screen(lib, bad, topo.host, [0]) == EINVAL
    assert lib.gns_acn1_workspace_bytes(ctypes.byref(PfConfig(tp.n + 1, E, tp.g.size, 10, 1e-8)), d, 4, E, ctypes.byref(need)) == EINVAL
    # a fast-decoupled blob where a Newton-Raphson blob is expected
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert _screen(lib, cfg, fd.host, [0]) == EINVAL
    assert lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 4, E, ctypes.byref(need)) == EINVAL
    # outages
    for bad in ([E], [-1], [0, 1, E, 2], [2 ** 31 - 1]):
        assert _screen(lib, cfg, topo.host, bad) == EINVAL, bad
    assert _screen(lib, cfg, topo.host, [0], K=0) == EINVAL and _screen(lib, cfg, topo.host, [0], K=-1) == EINVAL
    assert _screen(lib, cfg, topo.host, [0], Bt=0) == EINVAL and _screen(lib, cfg, topo.host, [0], Bt=-1) == EINVAL
    assert _screen(lib, cfg, topo.host, [0], per_grid=2) == EINVAL
    assert _screen(lib, cfg, topo.host, [0, 1, 2], Bt=0x7FFFFFFF, ws_bytes=2 ** 62) == EINVAL      # more workgroups than one launch takes
    # a short workspace: one byte less than the query asks for
    assert lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), d, 1, 2, ctypes.byref(need)) == 0
    assert _screen(lib, cfg, topo.host, [0, 3], ws_bytes=need.value - 1) == ESIZE
    assert _screen(lib, cfg, topo.host, [0, E], ws_bytes=need.value - 1) == EINVAL                  # GNS_EINVAL wins


def test_lds_refusal_is_newton_raphsons():
    lib = amd.load_library()
    tp = pt.path(4096)
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert topo.info['lds_bytes'] > pt.LDS_LIMIT
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 10, 1e-8)
    need = ctypes.c_size_t(0)
    assert lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, 1, 1, ctypes.byref(need)) == 0
    assert _screen(lib, cfg, topo.host, [0], ws_bytes=need.value) == EUNSUPPORTED
    assert _screen(lib, cfg, topo.host, [0], ws_bytes=need.value - 1) == ESIZE                    # GNS_ESIZE wins, as in gns_pf_solve
    assert _screen(lib, cfg, topo.host, [tp.f.size], ws_bytes=need.value) == EINVAL
    with pytest.raises(amd.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_acn1_screen', topo.info['lds_bytes'], powerflow._ACN1.formula)
    assert 'nnz(L+U) + dim + 8 N' in str(e.value)


def _blob_ybus_without(w, bus, line, k):
    """Dense Y-bus from the blob's own pattern and stamp lists with the stamps of line ``k`` (or of every line of the sequence ``k``)
    skipped: what the rows of gns_acn1.hip and gns_acn2.hip read."""
    out = {int(e) for e in np.atleast_1d(k)}
    N, E, nnzy = int(w[H['N']]), int(w[H['E']]), int(w[H['NNZY']])
    y_ptr, y_col, y_diag = _arr(w, 'Y_PTR', N + 1), _arr(w, 'Y_COL', nnzy), _arr(w, 'Y_DIAG', N)
    st_ptr, st = _arr(w, 'ST_PTR', nnzy + 1), _arr(w, 'ST', 4 * E)
    _, _, yff, ytt, yft, ytf = aref.line_admittances(line)
    kinds = np.stack([yff, ytt, yft, ytf])
    val = np.zeros(nnzy, dtype=np.complex128)
    val[y_diag] = bus[:, 4] + 1j * bus[:, 5]
    e, kind = st >> 2, st & 3
    keep = ~np.isin(e, list(out))
    np.add.at(val, np.repeat(np.arange(nnzy), np.diff(st_ptr))[keep], kinds[kind, e][keep])      # each entry's stamps, in their order
    Y = np.zeros((N, N), dtype=np.complex128)
    Y[np.repeat(np.arange(N), np.diff(y_ptr)), y_col] = val
    return Y


@pytest.mark.parametrize('name', ['case14', 'toy_parallel_selfloop', 'random40_parallel_selfloop'])
def test_skipping_the_stamps_is_deleting_the_row(name):
    """On parallel lines the entry keeps the other line's stamps; a line from a bus to itself has all four on one diagonal entry."""
    tp = {'case14': _case14(), 'toy_parallel_selfloop': toy()}.get(name) or pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'wide', 1, 0)
    bus, line = buses[0].double().numpy(), lines[0].double().numpy()
    w = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host
    pairs = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    if name != 'case14':
        assert any(a == b for a, b in pairs) and len(set(pairs)) < len(pairs)
    base = nr.ybus(bus, line).toarray()
    assert np.max(np.abs(aref.ybus_skipping(bus, line, None) - base)) <= 1e-12
    for k in range(tp.f.size):
        want = nr.ybus(bus, np.delete(line, k, axis=0)).toarray()
        scale = max(1.0, float(np.abs(want).max()))
        assert np.max(np.abs(aref.ybus_skipping(bus, line, k) - want)) <= 1e-12 * scale, (name, k)
        got = _blob_ybus_without(w, bus, line, k)
        assert np.max(np.abs(got - want)) <= 1e-12 * scale, (name, k)
        assert not np.any((want != 0) & (base == 0))                     # the outage adds no entry to the base pattern


def test_reference_flows_balance_at_every_bus():
    for case in (14, 30):
        buses, lines, gens, slack, _, _ = synth.solvable_grids(case, 2, seed=0)
        f, t, _ = synth.case_topology(case)
        bridges = powerflow._bridges(case, f - 1, t - 1)
        n_checked = 0
        for i in range(2):
            b, l, g = (x[i].double().numpy() for x in (buses, lines, gens))
            _, pv, pq = nr.roles(b, g, slack)
            v0, th0, conv, _, _ = aref.base_case(b, l, g, slack, tol=1e-12)
            assert conv
            bal = aref.bus_balance(b, l, g, v0, th0)
            assert np.max(np.abs(bal.real[np.r_[pv, pq]])) <= 1e-10 and np.max(np.abs(bal.imag[pq])) <= 1e-10
            for k in range(0, f.size, 3):
                row = aref.outage(b, l, g, slack, k, v0, th0, tol=1e-12)
                assert (row is None) == bool(bridges[k]), (case, i, k)
                if row is None or not row.converged:
                    continue
                assert row.p_from[k] == row.q_from[k] == row.p_to[k] == row.q_to[k] == 0.0
                bal = aref.bus_balance(b, l, g, row.v, row.theta, k)
                assert np.max(np.abs(bal.real[np.r_[pv, pq]])) <= 1e-10 and np.max(np.abs(bal.imag[pq])) <= 1e-10, (case, i, k)
                n_checked += 1
        assert n_checked >= 8, (case, n_checked)


# ---- the kernel's algorithm in numpy on the Newton-Raphson blob: what gns_acn1.hip does but for the order of sums

def emulate_row(w, bus, line, gen, k, v0, th0, tol=1e-8, max_iter=10):
    """Row k of one grid as the kernel computes it (``k`` one line, or the pair of lines of a double outage): the base pattern's Y-bus
    without the stamps of ``k``, the Jacobian into the base topology's factor slots (zeros where an entry lost its only lines), the
    base topology's program, warm-started from (v0, th0).  Returns (v, theta, converged, iterations, mismatch)."""
    from test_powerflow_programs_host import _programs, run_gather
    N, dim, nnzlu, nnzy, slack = (int(w[H[x]]) for x in ('N', 'DIM', 'NNZLU', 'NNZY', 'SLACK'))
    y_ptr, y_col = _arr(w, 'Y_PTR', N + 1), _arr(w, 'Y_COL', nnzy)
    th, vm_i, jslot, role = _arr(w, 'TH_IDX', N), _arr(w, 'VM_IDX', N), _arr(w, 'JSLOT', 4 * nnzy), _arr(w, 'ROLE', N)
    pivot = _arr(w, 'PIVOT', dim)
    step_ptr, ops = _programs(w)[0]['solve']
    Yd = _blob_ybus_without(w, bus, line, k)
    row = np.repeat(np.arange(N), np.diff(y_ptr))
    Y = Yd[row, y_col]                                               # the CSR values, patched
    S = nr.specified(bus, gen)
    vm, va = nr.start(bus, gen, slack + 1, v0, th0)
    assert np.all(vm[role == 0] == np.asarray(v0)[role == 0])
    it = 0
    while True:
        V = vm * np.exp(1j * va)
        cur = np.zeros(N, dtype=np.complex128)
        np.add.at(cur, row, Y * V[y_col])
        mis = V * np.conj(cur) - S
        F = np.zeros(nnzlu + dim)
        F[nnzlu + th[th >= 0]] = mis.real[th >= 0]
        F[nnzlu + vm_i[vm_i >= 0]] = mis.imag[vm_i >= 0]
        nrm = float(np.max(np.abs(F[nnzlu:]), initial=0.0))
        if nrm < tol:
            return vm, va, True, it, nrm
        if it >= max_iter:
            return vm, va, False, it, nrm
        c = V[row] * np.conj(Y * V[y_col])                           # V_i conj(Y_ik V_k)
        diag = row == y_col
        s_diag = (V * np.conj(cur))[row]
        d_th = -1j * c + np.where(diag, 1j * s_diag, 0)              # dS_i / dtheta_k
        d_vm = (c + np.where(diag, s_diag, 0)) / vm[y_col]           # dS_i / d|V_k|
        for col, val in enumerate((d_th.real, d_vm.real, d_th.imag, d_vm.imag)):
            s = jslot[col::4]
            on = (s >= 0) & (y_col != slack)
            F[s[on]] = val[on]
        run_gather(F, step_ptr, ops)
        assert np.all(np.isfinite(F[pivot])) and np.all(F[pivot] != 0.0), k
        va[th >= 0] -= F[nnzlu + th[th >= 0]]
        vm[vm_i >= 0] -= F[nnzlu + vm_i[vm_i >= 0]]
        it += 1


@pytest.mark.parametrize('name', ['case14', 'toy_parallel_selfloop', 'random40_parallel_selfloop'])
def test_the_base_blob_serves_every_outage(name):
    """The replay of the kernel's algorithm on the base topology's blob against the reference on the grid with the row deleted:
    the same convergence and iteration count, v and theta within 1e-9, wherever the reference converges with two iterations to spare."""
    if name == 'case14':
        tp = _case14()
        buses, lines, gens, _, _, _ = synth.solvable_grids(14, 2, seed=0)
    else:
        tp = toy() if name == 'toy_parallel_selfloop' else pt.families()[name]
        buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0)
    w = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    n_cmp = n_pairs = 0
    for i in range(2):
        b, l, g = (x[i].double().numpy() for x in (buses, lines, gens))
        v0, th0, conv, _, _ = aref.base_case(b, l, g, tp.slack)
        assert conv
        for k in range(tp.f.size):
            want = aref.outage(b, l, g, tp.slack, k, v0, th0)
            assert (want is None) == bool(bridges[k]), (name, i, k)
            if want is None:
                continue
            n_pairs += 1
            if not (want.converged and want.iterations <= 8):
                continue
            n_cmp += 1
            vm, va, got_conv, it, mis = emulate_row(w, b, l, g, k, v0, th0)
            assert got_conv and it == want.iterations and mis < 1e-8, (name, i, k, it, want.iterations)
            assert np.max(np.abs(vm - want.v)) <= 1e-9 and np.max(np.abs(va - want.theta)) <= 1e-9, (name, i, k)
    print(f'{name}: {n_cmp} of {n_pairs} non-islanding pairs compared')
    assert n_cmp >= 0.6 * n_pairs, (name, n_cmp, n_pairs)


def shifted_base(tp, v, theta, seed=4):
    """(base_v, base_theta) float64 numpy [B,N]: ``pt.perturbed_start`` of the manufactured solution with 0.3 rad added to every
    angle, so that base_theta[slack] = 0.3 and the start's ``theta - theta[slack]`` is a subtraction that matters."""
    v0, th0 = pt.perturbed_start(v.cpu(), theta.cpu(), tp.slack, seed)
    return v0.numpy(), (th0 + 0.3).numpy()


def one_step_ratios(bus, line, gen, slack_bus, k, vm0, va0, v1, th1):
    """(scipy's, the given step's) ``pt.one_step_ratio`` on the reference Jacobian and mismatch of the grid with row ``k`` (or every
    row of the sequence ``k``) of ``line`` deleted, at the start (vm0, va0); the step is read off the state (v1, th1) one update
    later."""
    import scipy.sparse.linalg as spla
    rest = np.delete(line, k, axis=0)
    _, pv, pq = nr.roles(bus, gen, slack_bus)
    pvpq = np.r_[pv, pq]
    J = nr.jacobian(bus, rest, gen, slack_bus, vm0, va0)
    F = nr.mismatch_vector(bus, rest, gen, slack_bus, vm0, va0)
    dx = np.r_[va0[pvpq] - th1[pvpq], vm0[pq] - v1[pq]]
    return pt.one_step_ratio(J, F, spla.spsolve(J, F)), pt.one_step_ratio(J, F, dx)


@pytest.mark.parametrize('regime', pt.REGIMES)
def test_one_step_of_the_replay_on_every_pair(regime):
    """One Newton step of the replay from a start with base_theta[slack] = 0.3, on EVERY non-bridge pair (no convergence needed):
    the step solves the reference Jacobian of the grid with the row deleted to ``pt.STEP_TOL``, scipy's own step asserted first as
    the guard; after zero steps the state is the reference start exactly.  Pins "the base blob serves every outage" at 100 %."""
    fam = pt.families()
    topos = [toy(), fam['random40_parallel_selfloop'], fam['random24_stacked_gens'], pt.ring_slack_without_generator(63)]
    for tp in topos:
        buses, lines, gens, v, theta = pt.grids(tp, regime, 2, seed=11)
        base_v, base_theta = shifted_base(tp, v, theta)
        w = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host
        bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
        n_cmp, worst = 0, 0.0
        for i in range(2):
            b, l, g = (x[i].double().numpy() for x in (buses, lines, gens))
            assert base_theta[i, tp.slack - 1] == 0.3
            vm0, va0 = nr.start(b, g, tp.slack, base_v[i], base_theta[i])
            for k in np.flatnonzero(~bridges):
                z = emulate_row(w, b, l, g, k, base_v[i], base_theta[i], tol=0.0, max_iter=0)
                assert np.array_equal(z[0], vm0) and np.array_equal(z[1], va0) and z[3] == 0, (tp.name, i, k)
                v1, th1, conv, it, _ = emulate_row(w, b, l, g, k, base_v[i], base_theta[i], tol=0.0, max_iter=1)
                assert it == 1 and not conv, (tp.name, i, k)
                r_scipy, r_replay = one_step_ratios(b, l, g, tp.slack, k, vm0, va0, v1, th1)
                assert r_scipy <= pt.STEP_TOL, (tp.name, regime, i, k, r_scipy)
                assert r_replay <= pt.STEP_TOL, (tp.name, regime, i, k, r_replay)
                worst = max(worst, r_replay)
                n_cmp += 1
        print(f'{tp.name} ({regime}): {n_cmp} of {2 * int((~bridges).sum())} non-bridge pairs compared, worst one-step ratio {worst:.1e}')
        assert n_cmp == 2 * int((~bridges).sum()) > 0
