"""CPU checks of the power-flow topology programs (``gns_pf_topology.cpp``) on generated families (``pf_topologies``), the case
shapes and the odd goldens: no in-step hazard in the solve or the transposed program, results that do not depend on the order the
lanes run a step in, both programs solving their systems, the header words and the limits of the analysis, and self-tests that
show the checkers catch what they are meant to."""
import ctypes
import glob
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from helpers import load_golden
import nr_grad_reference as gref
import nr_reference as ref
import pf_topologies as pt
from test_powerflow_grad_host import H, _arr

LANES = 64          # one wave: lane l runs operations start + l + 64 j of a step
SOLVE_TOL = 1e-10   # relative residual of a program's solve of a diagonally dominant system


def _odd_names():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(here, 'odd_*.npz')))


def _odd_topology(name):
    gd = load_golden(name)
    ln, gen = gd['lines'][0], gd['generators'][0]
    return pt.Topo(name, gd['buses'].shape[1], ln[:, 0].astype(np.int64), ln[:, 1].astype(np.int64), gen[:, 0].astype(np.int64),
                   int(gen[0, 0]))


def _islands(tp):
    return powerflow._islanded(tp.n, tp.f - 1, tp.t - 1, tp.slack - 1).size > 0


def _topologies():
    out = dict(pt.families())
    out.update({k: v for k, v in pt.boundary().items() if k != 'path_over'})
    for c, (n, _, _) in synth.CASE_SHAPES.items():
        f, t, g = synth.case_topology(c)
        out[f'case{c}'] = pt.Topo(f'case{c}', n, f, t, g, synth._solvable_slack(c))
    for name in _odd_names():
        tp = _odd_topology(name)
        if not _islands(tp):                        # (test_odd_goldens_that_island_are_refused)
            out[name] = tp
    return out


TOPOLOGIES = _topologies()


def test_odd_goldens_that_island_are_refused():
    islanding = [n for n in _odd_names() if n not in TOPOLOGIES]
    from test_powerflow_grad_host import ODD
    assert set(ODD) <= set(TOPOLOGIES) and len(islanding) <= 3
    for name in islanding:
        tp = _odd_topology(name)
        with pytest.raises(powerflow.IslandedTopology):
            powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _blob(tp):
    return powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host


def _programs(w):
    """{'solve': (step_ptr, ops [nops, 2]), 'transposed': ...} and the number of leading solve steps that factor J."""
    ts = _arr(w, 'T_STEP_PTR', w[H['T_NSTEPS']] + 2)
    return {'solve': (_arr(w, 'STEP_PTR', w[H['NSTEPS']] + 1), _arr(w, 'OPS', 2 * w[H['NOPS']]).reshape(-1, 2)),
            'transposed': (ts[:-1], _arr(w, 'T_OPS', 2 * w[H['T_NOPS']]).reshape(-1, 2))}, int(ts[-1])


def _fields(ops):
    return ops[:, 0] & 0xFFFF, (ops[:, 0].astype(np.uint32) >> 16).astype(np.int64), ops[:, 1].astype(np.int64)


def hazards(step_ptr, ops):
    """(destinations repeated within a step, operations that read a slot another operation of their step writes)."""
    step = np.repeat(np.arange(step_ptr.size - 1, dtype=np.int64), np.diff(step_ptr))
    dst, a, b = _fields(ops)
    wkey = step * 65536 + dst
    rkey = np.concatenate([step * 65536 + a, (step * 65536 + b)[b >= 0]])
    return wkey.size - np.unique(wkey).size, int(np.isin(rkey, wkey).sum())


def run_gather(F, step_ptr, ops):
    """Each step as one gather of every operand, then one scatter."""
    dst, a, b = _fields(ops)
    for s in range(step_ptr.size - 1):
        q = slice(step_ptr[s], step_ptr[s + 1])
        d, x, y = dst[q], a[q], b[q]
        div = y < 0
        F[d] = np.where(div, F[d] / F[x], F[d] - F[x] * F[np.where(div, 0, y)])


def run_lanes(F, step_ptr, ops, reverse=False):
    """The kernel's order (pf_run_program): round j of a step takes operations start + 64 j .. start + 64 j + 63, every lane of
    a round loads before any stores; with ``reverse`` the operations of each step are taken last to first."""
    dst, a, b = _fields(ops)
    for s in range(step_ptr.size - 1):
        idx = np.arange(step_ptr[s], step_ptr[s + 1])
        if reverse:
            idx = idx[::-1]
        for j in range(0, idx.size, LANES):
            q = idx[j:j + LANES]
            d, x, y = dst[q], a[q], b[q]
            div = y < 0
            F[d] = np.where(div, F[d] / F[x], F[d] - F[x] * F[np.where(div, 0, y)])


def _random_system(w, seed):
    """A random matrix of J's pattern, diagonally dominant: its slot vector (factor slots, zero right-hand side) and dense form
    in the ordered unknowns."""
    N, dim, nnzlu, nnzy = w[H['N']], w[H['DIM']], w[H['NNZLU']], w[H['NNZY']]
    y_ptr, y_col = _arr(w, 'Y_PTR', N + 1), _arr(w, 'Y_COL', nnzy)
    th, vm, jslot = _arr(w, 'TH_IDX', N), _arr(w, 'VM_IDX', N), _arr(w, 'JSLOT', 4 * nnzy)
    rng = np.random.default_rng(seed)
    F = np.zeros(nnzlu + dim)
    J = np.zeros((dim, dim))
    row = np.repeat(np.arange(N), np.diff(y_ptr))
    for c, (r_, c_) in enumerate(((th[row], th[y_col]), (th[row], vm[y_col]), (vm[row], th[y_col]), (vm[row], vm[y_col]))):
        s = jslot[c::4]
        on = s >= 0
        val = rng.uniform(-1, 1, on.sum())
        F[s[on]] = val
        J[r_[on], c_[on]] = val
    piv = _arr(w, 'PIVOT', dim)
    big = np.abs(J).sum(axis=1) + np.abs(J).sum(axis=0) + 1.0
    F[piv] = big
    J[np.arange(dim), np.arange(dim)] = big
    return F, J


def _solve_with(run, w, F0, b, progs):
    F = F0.copy()
    F[w[H['NNZLU']]:] = b
    run(F, *progs['solve'])
    return F


def _transpose_with(run, w, F0, g, progs, nf):
    F = F0.copy()
    sp_, ops = progs['solve']
    run(F, sp_[:nf + 1], ops)                       # the factor: the leading steps, on a zero right-hand side
    assert np.all(F[w[H['NNZLU']]:] == 0)
    F[w[H['NNZLU']]:] = g
    run(F, *progs['transposed'])
    return F


def _residual(A, x, b):
    return np.max(np.abs(A @ x - b), initial=0.0) / max(np.max(np.abs(A), initial=0.0) * np.max(np.abs(x), initial=0.0),
                                                         np.max(np.abs(b), initial=0.0), 1e-300)


@pytest.mark.parametrize('name', sorted(TOPOLOGIES))
def test_programs_have_no_in_step_hazard_and_solve_in_any_lane_order(name):
    w = _blob(TOPOLOGIES[name])
    progs, nf = _programs(w)
    for kind, (step_ptr, ops) in progs.items():
        assert step_ptr[0] == 0 and step_ptr[-1] == ops.shape[0] and np.all(np.diff(step_ptr) > 0), (name, kind)
        assert hazards(step_ptr, ops) == (0, 0), (name, kind)
    nnzlu, dim = w[H['NNZLU']], w[H['DIM']]
    F0, J = _random_system(w, seed=len(name))
    rng = np.random.default_rng(1)
    b, g = rng.standard_normal(dim), rng.standard_normal(dim)
    want = _solve_with(run_gather, w, F0, b, progs)
    assert _residual(J, want[nnzlu:], b) <= SOLVE_TOL, name
    for rev in (False, True):
        got = _solve_with(lambda F, s, o: run_lanes(F, s, o, rev), w, F0, b, progs)
        assert np.array_equal(got, want), (name, 'solve', rev)
    want_t = _transpose_with(run_gather, w, F0, g, progs, nf)
    assert _residual(J.T, want_t[nnzlu:], g) <= SOLVE_TOL, name
    for rev in (False, True):
        got = _transpose_with(lambda F, s, o: run_lanes(F, s, o, rev), w, F0, g, progs, nf)
        assert np.array_equal(got, want_t), (name, 'transposed', rev)


@pytest.mark.parametrize('name', sorted(TOPOLOGIES))
def test_header_words(name):
    tp = TOPOLOGIES[name]
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    info = topo.info
    assert info['lds_bytes'] == 8 * (info['nnz_lu'] + info['dim'] + 8 * info['n_bus'])
    assert info['lds_bytes'] <= pt.LDS_LIMIT
    assert info['n_adj_ops'] == info['nnz_lu'] and 0 <= info['n_factor_steps'] <= info['n_steps']
    slots = ctypes.c_int64()
    f, t, g = (np.ascontiguousarray(a - 1, dtype=np.int32) for a in (tp.f, tp.t, tp.g))
    lib = amd.load_library()
    assert lib.gns_pf_topology_slots(tp.n, f.size, g.size, f.ctypes.data, t.ctypes.data, g.ctypes.data, tp.slack - 1,
                                     ctypes.byref(slots)) == 0
    assert slots.value == info['nnz_lu'] + info['dim']


def test_diagonal_jacobian_star_has_no_factor_steps():
    for tp in (pt.star(200, 'pv'), pt.star(65, 'pv')):
        info = pt._info(tp)
        assert info['dim'] == tp.n - 1 and info['nnz_lu'] == info['dim'] and info['n_factor_steps'] == 0
        assert info['n_steps'] == 1 and info['n_adj_steps'] == 1


def test_family_coverage_near_multiples_of_64():
    cov = pt.coverage(pt.families().values())
    assert all(set(v) == {63, 0, 1} for v in cov.values()), cov


def test_lds_boundary_finders_straddle_the_limit():
    b = pt.boundary()
    fit, over, kfit = (pt._info(b[k]) for k in ('path_fit', 'path_over', 'complete_fit'))
    assert fit['lds_bytes'] <= pt.LDS_LIMIT < over['lds_bytes'] and over['n_bus'] == fit['n_bus'] + 1
    assert kfit['lds_bytes'] <= pt.LDS_LIMIT
    try:
        assert pt._info(pt.complete(kfit['n_bus'] + 1))['lds_bytes'] > pt.LDS_LIMIT
    except gns_mod.GNSError:
        pass


def test_overfill_topology_is_refused_with_its_slot_count():
    tp = pt.lattice(30)
    with pytest.raises(gns_mod.GNSError, match=pt.SLOTS_MESSAGE) as e:
        powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    import re
    slots = int(re.search(pt.SLOTS_MESSAGE, str(e.value)).group(1))
    assert slots > 65535
    assert 'latent_dim' not in str(e.value)


# ------------------------------------------------------------------------------------------------------ checker self-tests

def _move(step_ptr, ops, q, to):
    """The program with operation q moved to the end of step ``to``."""
    step = np.repeat(np.arange(step_ptr.size - 1), np.diff(step_ptr))
    step[q] = to
    order = np.argsort(step, kind='stable')
    counts = np.bincount(step, minlength=step_ptr.size - 1)
    return np.r_[0, np.cumsum(counts)].astype(step_ptr.dtype), ops[order]


def test_checkers_catch_a_misplaced_operation():
    tp = TOPOLOGIES['case118']
    w = _blob(tp)
    progs, _ = _programs(w)
    step_ptr, ops = progs['solve']
    step = np.repeat(np.arange(step_ptr.size - 1), np.diff(step_ptr))
    dst, a, _ = _fields(ops)
    # an operation whose operand a was written two or more steps before it
    last_write = {}
    pick = None
    for q in range(ops.shape[0]):
        s_w = last_write.get(int(a[q]))
        if s_w is not None and s_w >= 1 and step[q] >= s_w + 2 and pick is None:
            pick = (q, s_w)
        last_write[int(dst[q])] = int(step[q])
    q, s_w = pick
    # into the step of the operation that writes its input: an in-step hazard
    sp1, ops1 = _move(step_ptr, ops, q, s_w)
    assert hazards(sp1, ops1)[1] > 0
    # into the step before it: no in-step hazard, but it reads its input before it is written, and the solve is wrong
    sp2, ops2 = _move(step_ptr, ops, q, s_w - 1)
    F0, J = _random_system(w, seed=3)
    b = np.random.default_rng(2).standard_normal(w[H['DIM']])
    F = F0.copy()
    F[w[H['NNZLU']]:] = b
    run_gather(F, sp2, ops2)
    assert _residual(J, F[w[H['NNZLU']]:], b) > SOLVE_TOL


def _step_problem(tp, regime, seed=0):
    buses, lines, gens, v, theta = pt.grids(tp, regime, 1, seed)
    v0, th0 = pt.perturbed_start(v, theta, tp.slack, seed)
    bus, line, gen = (x[0].double().numpy() for x in (buses, lines, gens))
    vm, va = ref.start(bus, gen, tp.slack, v0[0].numpy(), th0[0].numpy())
    J = ref.jacobian(bus, line, gen, tp.slack, vm, va)
    F = ref.mismatch_vector(bus, line, gen, tp.slack, vm, va)
    return bus, line, gen, vm, va, J, F


@pytest.mark.parametrize('regime', pt.REGIMES)
def test_one_step_bound_catches_a_slightly_wrong_jacobian(regime):
    for name in ('pair', 'path65', 'star200_leaf_slack', 'lattice8x8', 'complete20', 'random40_parallel_selfloop',
                 'ring30_slack_no_gen', 'random24_stacked_gens', 'hub150_70lines_70gens'):
        *_, J, F = _step_problem(pt.families()[name], regime)
        dx = spla.spsolve(J, F)
        assert pt.one_step_ratio(J, F, dx) <= pt.STEP_TOL, name
        Jd = J.toarray()
        i, j = np.unravel_index(np.argmax(np.abs(Jd * dx[None, :])), Jd.shape)
        Jd[i, j] *= 1 + 1e-6
        assert pt.one_step_ratio(Jd, F, dx) > pt.STEP_TOL, name


@pytest.mark.parametrize('name', ['pair', 'random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen',
                                  'hub150_70lines_70gens', 'star200_pv'])
def test_reference_jacobian_matches_autograd(name):
    """nr_reference.jacobian (MATPOWER's dSbus_dV on the scipy Y-bus) against torch autograd of nr_grad_reference.mismatch (the
    Y-bus from incidence matrices): two independent statements of J, self-loop and parallel lines included, in the wide regime."""
    tp = pt.families()[name]
    bus, line, gen, vm, va, J, F = _step_problem(tp, 'wide', seed=4)
    grid = gref._Grid(bus, line, gen, tp.slack)
    x0 = torch.as_tensor(np.r_[va[grid.pvpq], vm[grid.pq]])
    gen_t = torch.as_tensor(gen).clone()
    gen_t[:, 4] = torch.as_tensor(vm[gen[:, 0].astype(int) - 1])             # the start's |V| at generator buses
    p = [torch.as_tensor(bus), torch.as_tensor(line), gen_t]
    Jt = torch.autograd.functional.jacobian(lambda x: gref.mismatch(grid, x, *p), x0).numpy()
    scale = np.max(np.abs(Jt))
    assert np.max(np.abs(J.toarray() - Jt)) <= 1e-12 * scale, name
    Ft = gref.mismatch(grid, x0, *p).numpy()
    assert np.max(np.abs(F - Ft)) <= 1e-12 * max(np.max(np.abs(Ft)), 1.0), name
