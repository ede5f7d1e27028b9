"""CPU checks of the fast-decoupled power flow's host side: the float64 makeB + fdpf oracle (``fd_reference``) against manufactured
solutions and the reference NR, the FD blob (``gns_fd_prepare_topology``): its dimensions and fill, its four programs free of
in-step hazards and solving B' / B'' systems in any lane order, the refusals, the exports, and the Newton-Raphson blob unchanged."""
import ctypes
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import EXPORTS, FD_EXPORTS, FdConfig, PfConfig
import fd_reference as fref
import nr_reference as ref
import pf_topologies as pt
from test_powerflow_programs_host import TOPOLOGIES, hazards, run_gather, run_lanes

TRUTH_TOL = 5e-7        # the exact solution of the float32 inputs lies within this of the chosen point (test_powerflow_host)
SOLVE_TOL = 1e-10
# header words of the FD blob (opf-graph-neural-solver_amd/csrc/gns_pf_common.h, FH_*)
FH = {k: i for i, k in enumerate(['MAGIC', 'TOTAL', 'N', 'E', 'GN', 'SLACK', 'NPV', 'NPQ', 'NNZY', 'DIM1', 'NNZLU1', 'DIM2',
                                   'NNZLU2', 'NOPS_F1', 'NSTEPS_F1', 'NOPS_S1', 'NSTEPS_S1', 'NOPS_F2', 'NSTEPS_F2', 'NOPS_S2',
                                   'NSTEPS_S2', 'ROLE', 'P_IDX', 'Q_IDX', 'GEN_PTR', 'GEN_IDX', 'Y_PTR', 'Y_COL', 'Y_DIAG', 'ST_PTR',
                                   'ST', 'BSLOT', 'PIVOT1', 'PIVOT2', 'STEP_F1', 'OPS_F1', 'STEP_S1', 'OPS_S1', 'STEP_F2', 'OPS_F2',
                                   'STEP_S2', 'OPS_S2'])}
# sha256 of the Newton-Raphson blob of case118 (slack of solvable_grids) as the parent of the FD analysis wrote it
NR_CASE118_SHA256 = 'ad335848a2a43855220491d7bee77dc3c8a389b24ba8a9e9434298466d862d94'


def _arr(w, name, n):
    return w[w[FH[name]]:w[FH[name]] + n]


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _programs(w):
    """{'f1': (step_ptr, ops [nops, 2]), 's1': ..., 'f2': ..., 's2': ...}"""
    out = {}
    for k in ('F1', 'S1', 'F2', 'S2'):
        out[k.lower()] = (_arr(w, 'STEP_' + k, w[FH['NSTEPS_' + k]] + 1), _arr(w, 'OPS_' + k, 2 * w[FH['NOPS_' + k]]).reshape(-1, 2))
    return out


@pytest.mark.parametrize('case', [14, 30, 118])
@pytest.mark.parametrize('variant', ['XB', 'BX'])
def test_oracle_converges_to_the_manufactured_root(case, variant):
    """On the synthetic grids (taps in [0.8, 1.2], r/x up to 6) FD converges slowly: within PYPOWER's 30 iterations on every case14
    grid but on fewer than half of the case30 / case118 grids, so the root is checked with a larger budget."""
    buses, lines, gens, slack, v, theta = synth.solvable_grids(case, 6, seed=7)
    n_conv = 0
    for k in range(buses.shape[0]):
        bus, line, gen = (x[k].double().numpy() for x in (buses, lines, gens))
        vm, va, conv, it, mis = fref.fast_decoupled(bus, line, gen, slack, variant, max_iter=30 if case == 14 else 300)
        if case == 14:
            assert conv and 0 < it <= 30, (k, it, mis)
        if not conv:
            continue
        n_conv += 1
        assert mis < 1e-8
        assert np.max(np.abs(vm - v[k].numpy())) <= TRUTH_TOL and np.max(np.abs(va - theta[k].numpy())) <= TRUTH_TOL
        nv, nt, nconv, _, _ = ref.newton_raphson(bus, line, gen, slack)
        assert nconv
        assert np.max(np.abs(vm - nv)) <= 1e-7 and np.max(np.abs(va - nt)) <= 1e-7
    assert n_conv >= 3, n_conv


def test_oracle_edge_rules():
    buses, lines, gens, slack, v, theta = synth.solvable_grids(14, 1, seed=2)
    bus, line, gen = (x[0].double().numpy() for x in (buses, lines, gens))
    vm, va, conv, it, _ = fref.fast_decoupled(bus, line, gen, slack, 'XB')
    # a start that meets the test is converged with 0 iterations
    hot = fref.fast_decoupled(bus, line, gen, slack, 'XB', v0=vm, theta0=va + 0.3)
    assert hot[2] and hot[3] == 0
    # a non-finite mismatch at the start stops the grid there
    bad = line.copy()
    bad[3, 2] = np.nan
    r = fref.fast_decoupled(bus, bad, gen, slack, 'XB')
    assert not r[2] and r[3] == 0 and np.isnan(r[4])


def test_fd_info_dimensions_and_fill_against_splu():
    for name in ('case14', 'case30', 'case118', 'case300', 'lattice16x16', 'random97_parallel_selfloop', 'complete33'):
        tp = TOPOLOGIES[name]
        fd = _fd(tp)
        info = fd.info
        assert info['dim_p'] == tp.n - 1, name
        assert info['dim_pp'] == info['n_pq'] == powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).info['n_pq'], name
        assert info['lds_bytes'] == 8 * (info['nnz_lu_p'] + info['dim_p'] + info['nnz_lu_pp'] + info['dim_pp'] + 6 * tp.n)
        buses, lines, gens, *_ = pt.grids(tp, 'reference', 1, 0)
        Bp, Bpp = fref.make_b(buses[0].double().numpy(), lines[0].double().numpy(), 'XB')
        slack, pv, pq = ref.roles(buses[0].numpy(), gens[0].numpy(), tp.slack)
        for M, idx, key in ((Bp, np.r_[pv, pq], 'nnz_lu_p'), (Bpp, pq, 'nnz_lu_pp')):
            if idx.size == 0:
                continue
            A = M[np.ix_(idx, idx)] + np.eye(idx.size) * 1e3            # its pattern, well conditioned
            lu = spla.splu(sp.csc_matrix(A))
            ref_nnz = lu.L.nnz + lu.U.nnz - idx.size                     # (scipy stores L's unit diagonal)
            assert info[key] <= 1.5 * ref_nnz, (name, key, info[key], ref_nnz)


def _random_b(w, m, seed):
    """A random diagonally dominant matrix of B' (m = 0) or B'''s (m = 1) pattern: its slot vector (factor slots, zero right-hand
    side) and dense form in the ordered unknowns."""
    N, nnzy = w[FH['N']], w[FH['NNZY']]
    dim, nnz = w[FH['DIM1' if m == 0 else 'DIM2']], w[FH['NNZLU1' if m == 0 else 'NNZLU2']]
    idx = _arr(w, 'P_IDX' if m == 0 else 'Q_IDX', N)
    y_ptr, y_col, bslot = _arr(w, 'Y_PTR', N + 1), _arr(w, 'Y_COL', nnzy), _arr(w, 'BSLOT', 2 * nnzy)[m::2]
    row = np.repeat(np.arange(N), np.diff(y_ptr))
    rng = np.random.default_rng(seed)
    F = np.zeros(nnz + dim)
    A = np.zeros((dim, dim))
    on = bslot >= 0
    assert np.array_equal(on, (idx[row] >= 0) & (idx[y_col] >= 0))
    val = rng.uniform(-1, 1, on.sum())
    F[bslot[on]] = val
    A[idx[row[on]], idx[y_col[on]]] = val
    big = np.abs(A).sum(axis=1) + np.abs(A).sum(axis=0) + 1.0
    piv = _arr(w, 'PIVOT1' if m == 0 else 'PIVOT2', dim)
    F[piv] = big
    A[np.arange(dim), np.arange(dim)] = big
    return F, A, nnz


def _factor_solve(run, progs, m, F0, nnz, b):
    F = F0.copy()
    run(F, *progs['f1' if m == 0 else 'f2'])
    assert np.all(F[nnz:] == 0)
    F[nnz:] = b
    run(F, *progs['s1' if m == 0 else 's2'])
    return F


@pytest.mark.parametrize('name', sorted(TOPOLOGIES))
def test_fd_programs_have_no_hazard_and_solve_in_any_lane_order(name):
    tp = TOPOLOGIES[name]
    w = _fd(tp).host
    assert w[FH['MAGIC']] == 0x44504631 and w[FH['TOTAL']] == w.size
    progs = _programs(w)
    for kind, (step_ptr, ops) in progs.items():
        assert step_ptr[0] == 0 and step_ptr[-1] == ops.shape[0] and np.all(np.diff(step_ptr) > 0), (name, kind)
        assert hazards(step_ptr, ops) == (0, 0), (name, kind)
    for m in (0, 1):
        F0, A, nnz = _random_b(w, m, seed=len(name) + m)
        if A.shape[0] == 0:
            continue
        b = np.random.default_rng(m).standard_normal(A.shape[0])
        want = _factor_solve(run_gather, progs, m, F0, nnz, b)
        x = spla.spsolve(sp.csc_matrix(A), b)
        assert np.max(np.abs(want[nnz:] - x)) <= SOLVE_TOL * max(np.max(np.abs(x)), 1.0), (name, m)
        for rev in (False, True):
            got = _factor_solve(lambda F, s, o: run_lanes(F, s, o, rev), progs, m, F0, nnz, b)
            assert np.array_equal(got, want), (name, m, rev)


def test_n_pq_zero_and_single_bus():
    tp = TOPOLOGIES['odd_hub_all_gens_b2_K4_d10_single']
    info = _fd(tp).info
    assert info['dim_pp'] == 0 and info['nnz_lu_pp'] == 0 and info['solve_pp_ops'] == 0 and info['dim_p'] == tp.n - 1
    one = powerflow.analyse_fd_topology(1, [], [], [1], 1).info
    assert one['dim_p'] == one['dim_pp'] == 0 and one['lds_bytes'] == 48


def test_errors_exports_and_unchanged_nr_blob():
    with pytest.raises(powerflow.IslandedTopology):
        powerflow.analyse_fd_topology(4, [1, 3], [2, 4], [1], 1)
    with pytest.raises(ValueError, match='slack_bus'):
        powerflow.analyse_fd_topology(4, [1, 2, 3], [2, 3, 4], [1], 5)
    # an over-limit topology: the analysis accepts it, the solve refuses it (before any launch) naming its LDS image
    tp = pt.path(1500)
    fd = _fd(tp)
    assert fd.info['lds_bytes'] > pt.LDS_LIMIT
    lib = amd.load_library()
    cfg = FdConfig(PfConfig(tp.n, tp.f.size, tp.g.size, 30, 1e-8), 2)
    dummy = fd.host.ctypes.data
    rc = lib.gns_fd_solve(ctypes.byref(cfg), fd.host.ctypes.data, dummy, dummy, dummy, dummy, 1, None, None, dummy, dummy, dummy,
                          dummy, dummy, dummy, 1 << 30, None)
    assert rc == powerflow.GNS_EUNSUPPORTED
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(rc, 'gns_fd_solve', fd.info['lds_bytes'], powerflow._FD_LDS_FORMULA)
    assert str(fd.info['lds_bytes']) in str(e.value) and "B''" in str(e.value)
    assert lib.gns_fd_solve(ctypes.byref(FdConfig(PfConfig(tp.n, tp.f.size, tp.g.size, 30, 1e-8), 1)), fd.host.ctypes.data, dummy,
                            dummy, dummy, dummy, 1, None, None, dummy, dummy, dummy, dummy, dummy, dummy, 1 << 30, None) == 1
    # a factor over the 65 535-slot limit is refused by the analysis with its slot count
    with pytest.raises(gns_mod.GNSError, match=r'needs (\d+) slots'):
        powerflow.analyse_fd_topology(*pt.complete(400)[1:])
    for f in FD_EXPORTS:
        assert hasattr(lib, f) and f not in EXPORTS
    f, t, g = synth.case_topology(118)
    w = powerflow.analyse_topology(118, f, t, g, synth._solvable_slack(118)).host
    assert hashlib.sha256(w.tobytes()).hexdigest() == NR_CASE118_SHA256
