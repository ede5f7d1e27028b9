"""Fast-decoupled power flow on the MI355X over the generated topology families of ``pf_topologies`` in two value regimes, both
variants: the start and its scaled mismatch after zero steps, one iteration whose two half-steps must solve the reference B' and
B'' (the test that pins ``fd_b_row``, the slot maps and the four elimination programs on the device), iterations that compose
bit for bit, full solves from a flat start against the reference, the LDS limit of the fast-decoupled image (the largest
topologies that fit, a mixed batch of very different images, refusals) and the grids that cannot be factored, with neighbours."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow
from opf_graph_neural_solver_amd._lib import FdConfig, PfConfig
import fd_reference as fref
import nr_reference as ref
import pf_topologies as pt
from test_fdpf_host import (FAIL_BATCH, FAIL_ROW, FIT_REF_CONVERGED, FLAT_MAX_ITER, FLAT_REF_CONVERGED, VARIANTS, failure_cases,
                            half_steps, step_ratio)
from test_powerflow_topologies_gpu import CALM, CALM_START, _star_like

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = 3
FIELDS = ('v', 'theta', 'converged', 'iterations', 'mismatch')
# a topology's grids: float32 (buses, lines, generators) on the host (what the reference reads) and on the device, the chosen solution
Set = collections.namedtuple('Set', ['tp', 'cpu', 'dev', 'v', 'theta'])


def _set(tp, regime, batch, seed, **kw):
    buses, lines, gens, v, theta = pt.grids(tp, regime, batch, seed=seed, **kw)
    return Set(tp, (buses, lines, gens), tuple(t.to(DEV) for t in (buses, lines, gens)), v, theta)


@pytest.fixture(scope='module')
def sets():
    """(family, regime) -> Set: ``pt.fd_families()`` and the wheel, the grids of the host file's reference count."""
    fams = dict(pt.fd_families())
    fams['wheel71'] = pt.wheel()
    return {(name, regime): _set(tp, regime, BATCH, 11) for name, tp in fams.items() for regime in pt.REGIMES}


@pytest.fixture(scope='module')
def boundary_sets():
    b = pt.fd_boundary()
    out = {}
    for regime in pt.REGIMES:
        out['path_fit', regime] = _set(b['path_fit'], regime, 1, 0, **CALM)
        out['complete_fit', regime] = _set(b['complete_fit'], regime, 2, 0)
    return out


def _fd(s, variant, **kw):
    return powerflow.fast_decoupled(*s.dev, slack_bus=s.tp.slack, variant=variant, **kw)


def _same(a, b):
    """Bit-identical, NaN included."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b))


def _all_same(a, b, what, rows=None):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert _same(x if rows is None else x[rows], y), (what, k)


def _grid(s, i):
    return [t[i].double().numpy() for t in s.cpu]


def _start(s, seed, calm=False):
    return pt.perturbed_start(s.v, s.theta, s.tp.slack, seed, **(CALM_START if calm else {}))


def _np(t):
    return t.cpu().numpy()


def _check_norm(s, i, vm, va, got, what):
    """The returned mismatch is the reference's scaled norm at (vm, va), to float64 rounding."""
    bus, line, gen = _grid(s, i)
    pvpq, pq, Y, S = fref.setting(bus, line, gen, s.tp.slack)
    want = fref.scaled_norm(Y, S, pvpq, pq, vm, va)[2]
    bound = fref.norm_rounding_bound(Y, S, vm)
    assert abs(float(got) - want) <= bound, (what, float(got), want, bound)


def test_zero_steps_return_the_start_and_its_scaled_mismatch(sets):
    """max_iter = 0 from a warm start: the start exactly as include/gns_powerflow.h defines it, and the scaled norm of the reference."""
    for (name, regime), s in sets.items():
        v0, th0 = _start(s, 1)
        for variant in VARIANTS:
            res = _fd(s, variant, v0=v0, theta0=th0, max_iter=0)
            assert bool((res.iterations == 0).all()), (name, regime, variant)
            for i in range(BATCH):
                bus, line, gen = _grid(s, i)
                vm, va = ref.start(bus, gen, s.tp.slack, v0[i].numpy(), th0[i].numpy())
                assert np.array_equal(_np(res.v[i]), vm), (name, regime, variant, i)
                assert np.array_equal(_np(res.theta[i]), va), (name, regime, variant, i)
                _check_norm(s, i, vm, va, res.mismatch[i], (name, regime, variant, i))


def _one_iteration_ratios(s, variant, v0, th0, res, what):
    """(numpy's, the device's) residual ratios of the P and of the Q half-step of every grid of ``res``, one iteration with
    tol = 0 from (v0, theta0); what the iteration must leave alone and the mismatch it returns are checked on the way."""
    assert bool((res.iterations == 1).all()) and not bool(res.converged.any()), (what, res.iterations)
    out = []
    for i in range(s.cpu[0].shape[0]):
        bus, line, gen = _grid(s, i)
        slack, pv, pq = ref.roles(bus, gen, s.tp.slack)
        pvpq = np.r_[pv, pq]
        vm, va = ref.start(bus, gen, s.tp.slack, v0[i].numpy(), th0[i].numpy())
        v1, t1 = _np(res.v[i]), _np(res.theta[i])
        fixed = np.setdiff1d(np.arange(s.tp.n), pq)
        assert np.array_equal(v1[fixed], vm[fixed]) and t1[slack] == 0.0, (what, i)
        # Q at the device's own angles: an error of the P stage can neither hide nor fake one of the Q stage
        (Ap, P), (App, Q) = half_steps(bus, line, gen, s.tp.slack, variant, vm, va, va_q=t1)
        d_theta, d_v = va[pvpq] - t1[pvpq], vm[pq] - v1[pq]
        r_ref = max(step_ratio(Ap, P, np.linalg.solve(Ap, P)), step_ratio(App, Q, np.linalg.solve(App, Q) if pq.size else Q))
        out.append((r_ref, step_ratio(Ap, P, d_theta), step_ratio(App, Q, d_v)))
        _check_norm(s, i, v1, t1, res.mismatch[i], (what, i))
    return out


@pytest.mark.parametrize('mixed', [False, True])
def test_one_iteration_solves_the_reference_b_matrices(sets, boundary_sets, mixed):
    worst = {}
    for (name, regime), s in list(sets.items()) + list(boundary_sets.items()):
        v0, th0 = _start(s, 2, calm=name == 'path_fit')
        for variant in VARIANTS:
            what = (name, regime, variant)
            res = _fd(s, variant, v0=v0, theta0=th0, max_iter=1, tol=0.0, mixed_topologies=mixed)
            if mixed:
                _all_same(res, _fd(s, variant, v0=v0, theta0=th0, max_iter=1, tol=0.0), what)
            for k, (r_ref, r_p, r_q) in enumerate(_one_iteration_ratios(s, variant, v0, th0, res, what)):
                assert r_ref <= pt.STEP_TOL, (what, k, r_ref)                  # the grid is conditioned well enough ...
                assert r_p <= pt.STEP_TOL, (what, k, 'P half-step', r_p)       # ... so a failure here is the kernel's
                assert r_q <= pt.STEP_TOL, (what, k, 'Q half-step', r_q)
                worst[name] = max(worst.get(name, 0.0), r_p, r_q)
    print('largest half-step residual ratio per family (mixed=%s):' % mixed, {k: f'{r:.1e}' for k, r in worst.items()})


def _chained(s, variant, v0, th0, counts):
    res = None
    for n in counts:
        res = _fd(s, variant, v0=v0, theta0=th0, max_iter=n, tol=0.0)
        assert bool((res.iterations == n).all()), (s.tp.name, variant, n, res.iterations)
        v0, th0 = res.v, res.theta
    return res


def test_iterations_compose_exactly(sets):
    """Two (three) iterations in one call are bit-identical to one and one (one and two) chained through the warm start: no solve
    program clobbers a factor slot, no right-hand side survives a half-step, Vr / Vi never go stale."""
    for (name, regime), s in sets.items():
        v0, th0 = _start(s, 3)
        for variant in VARIANTS:
            runs = [((2,), (1, 1))]
            if name in ('lattice16x16', 'random97_parallel_selfloop', 'hub150_70lines_70gens'):
                runs.append(((3,), (1, 2)))
            for whole, parts in runs:
                a, b = _chained(s, variant, v0, th0, whole), _chained(s, variant, v0, th0, parts)
                for k in ('v', 'theta', 'mismatch'):
                    assert bool(torch.isfinite(getattr(a, k)).all()), (name, regime, variant, k)
                    assert torch.equal(getattr(a, k), getattr(b, k)), (name, regime, variant, whole, k)


def _compare_with_reference(s, res, variant, what, **kw):
    """``test_fdpf_gpu.test_against_the_oracle``'s rules on every grid; returns (reference-converged, of them equal iterations)."""
    n_conv, n_same = 0, 0
    for i in range(s.cpu[0].shape[0]):
        bus, line, gen = _grid(s, i)
        start = {k: x[i].numpy() for k, x in kw.items() if k in ('v0', 'theta0')}
        rest = {k: x for k, x in kw.items() if k not in ('v0', 'theta0')}
        with np.errstate(all='ignore'):
            vm, va, conv, it, mis = fref.fast_decoupled(bus, line, gen, s.tp.slack, variant, **rest, **start)
        assert bool(res.converged[i]) == conv, (what, i, float(res.mismatch[i]), mis, int(res.iterations[i]), it)
        if not conv:
            continue
        n_conv += 1
        assert np.max(np.abs(_np(res.v[i]) - vm)) <= 1e-9, (what, i)
        assert np.max(np.abs(_np(res.theta[i]) - va)) <= 1e-9, (what, i)
        d = abs(int(res.iterations[i]) - it)
        assert d <= 1, (what, i, int(res.iterations[i]), it)
        n_same += d == 0
    return n_conv, n_same


def test_flat_start_solves_match_the_reference(sets):
    """From a flat start with ``FLAT_MAX_ITER`` iterations on both sides; the floor is the reference's own count
    (test_fdpf_host.test_reference_convergence_count_from_a_flat_start, which also says why it is below a third)."""
    n_conv, n_same = 0, 0
    for (name, regime), s in sets.items():
        if name not in pt.fd_families():
            continue
        for variant in VARIANTS:
            res = _fd(s, variant, max_iter=FLAT_MAX_ITER)
            c, e = _compare_with_reference(s, res, variant, (name, regime, variant), max_iter=FLAT_MAX_ITER)
            n_conv, n_same = n_conv + c, n_same + e
    print(f'flat start, max_iter {FLAT_MAX_ITER}: the reference converged on {n_conv} grids, {n_same} with the same iteration count')
    assert n_conv >= FLAT_REF_CONVERGED and n_same >= 0.99 * n_conv, (n_conv, n_same)


def test_largest_fitting_topologies_solve(boundary_sets):
    """A warm-started solve of the largest path and complete graph whose fast-decoupled image fits, plain and mixed.  (The iteration
    itself diverges on the chain of 1462 PQ buses, from however close a start: there both sides must say so.)"""
    n_conv = 0
    for (name, regime), s in boundary_sets.items():
        info = pt._info(s.tp, powerflow.analyse_fd_topology)
        assert info['lds_bytes'] <= pt.LDS_LIMIT
        v0, th0 = _start(s, 0, calm=name == 'path_fit')
        for variant in VARIANTS:
            res = _fd(s, variant, v0=v0, theta0=th0, max_iter=FLAT_MAX_ITER)
            _all_same(_fd(s, variant, v0=v0, theta0=th0, max_iter=FLAT_MAX_ITER, mixed_topologies=True), res, (name, regime, variant))
            n_conv += _compare_with_reference(s, res, variant, (name, regime, variant), v0=v0, theta0=th0, max_iter=FLAT_MAX_ITER)[0]
            print(f'{name} ({regime}, {variant}): N={s.tp.n} lds={info["lds_bytes"]} B, solve steps B\'/B\'\'='
                  f'{info["solve_p_steps"]}/{info["solve_pp_steps"]}, converged={res.converged.tolist()}, '
                  f'iterations={res.iterations.tolist()}')
    assert n_conv >= FIT_REF_CONVERGED, n_conv


def test_mixed_batch_of_very_different_images_matches_plain_calls():
    """The fitting path interleaved with a star of its shape: ``ystride = nnzy_max`` and the one ``lds_bytes`` of gns_fd_set_kernel."""
    path = pt.fd_boundary()['path_fit']
    star = _star_like(path)
    ip, istar = (pt._info(tp, powerflow.analyse_fd_topology) for tp in (path, star))
    assert ip['lds_bytes'] > 1.3 * istar['lds_bytes'] and ip['nnz_lu_p'] > 2.5 * istar['nnz_lu_p']
    gp, gs = _set(path, 'reference', 3, 7, **CALM), _set(star, 'reference', 3, 7, **CALM)
    order = torch.tensor([0, 3, 1, 4, 2, 5])                 # interleaved: path, star, path, star, ...
    both = Set(path, None, tuple(torch.cat([x, y])[order.to(DEV)] for x, y in zip(gp.dev, gs.dev)), torch.cat([gp.v, gs.v])[order],
               torch.cat([gp.theta, gs.theta])[order])
    v0, th0 = pt.perturbed_start(both.v, both.theta, 1, 8, **CALM_START)
    srt = torch.tensor([0, 2, 4, 1, 3, 5])                   # the same grids sorted by topology
    for variant in VARIANTS:
        for kw in (dict(max_iter=1, tol=0.0), {}):
            mres = _fd(both, variant, v0=v0, theta0=th0, mixed_topologies=True, **kw)
            for idx in ([0, 2, 4], [1, 3, 5]):
                part = both._replace(dev=tuple(x[idx] for x in both.dev))
                _all_same(mres, _fd(part, variant, v0=v0[idx], theta0=th0[idx], **kw), (variant, kw, idx), rows=idx)
            sres = _fd(both._replace(dev=tuple(x[srt.to(DEV)] for x in both.dev)), variant, v0=v0[srt], theta0=th0[srt],
                       mixed_topologies=True, **kw)
            _all_same(mres, sres, (variant, kw, 'sorted'), rows=srt.to(DEV))
            if kw:
                assert bool((mres.iterations == 1).all()) and bool(torch.isfinite(mres.mismatch).all())


def _over():
    tp = pt.fd_boundary()['path_over']
    return tp, _set(tp, 'reference', 2, 1, **CALM)


def test_over_the_limit_is_refused_with_its_lds_image():
    tp, s = _over()
    lds = pt._info(tp, powerflow.analyse_fd_topology)['lds_bytes']
    assert lds > pt.LDS_LIMIT
    for variant in VARIANTS:
        for mixed in (False, True):
            with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
                _fd(s, variant, mixed_topologies=mixed)
            assert f'{lds} B' in str(e.value) and "B''" in str(e.value) and 'latent_dim' not in str(e.value)
        # a mixed batch with one member over the limit is refused as a whole
        st = _set(_star_like(tp), 'reference', 2, 1, **CALM)
        with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE):
            _fd(st._replace(dev=tuple(torch.cat([x, y]) for x, y in zip(st.dev, s.dev))), variant, mixed_topologies=True)
        # ... while its other member alone solves (BX takes more than PYPOWER's 30 iterations on one of the two)
        assert bool(_fd(st, variant, mixed_topologies=True, max_iter=FLAT_MAX_ITER).converged.all())


def test_raw_entries_refuse_over_the_limit_and_write_nothing():
    tp, s = _over()
    buses, lines, gens = s.dev
    lib = amd.load_library()
    topo = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack, device=DEV)
    Bt, N = buses.shape[0], tp.n
    ts = powerflow._PfTopologySet(DEV)
    off = ts.add(('over',), topo)
    ts.sync()
    members = np.array([off], dtype=np.int32)
    grid_off = torch.full((Bt,), off, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    sentinel = -12345.0
    for alg in (2, 3):
        cfg = FdConfig(PfConfig(N, tp.f.size, tp.g.size, 30, 1e-8), alg)
        need, need_s = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.gns_fd_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
        assert lib.gns_fd_workspace_bytes_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.words, members.ctypes.data, 1, Bt,
                                              ctypes.byref(need_s)) == powerflow.GNS_EUNSUPPORTED
        ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
        outs = dict(v=torch.full((Bt, N), sentinel, dtype=torch.float64, device=DEV),
                    th=torch.full((Bt, N), sentinel, dtype=torch.float64, device=DEV),
                    conv=torch.full((Bt,), 7, dtype=torch.uint8, device=DEV), it=torch.full((Bt,), -7, dtype=torch.int32, device=DEV),
                    mis=torch.full((Bt,), sentinel, dtype=torch.float64, device=DEV))
        o = [outs[k].data_ptr() for k in ('v', 'th', 'conv', 'it', 'mis')]
        assert lib.gns_fd_solve(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), buses.data_ptr(), lines.data_ptr(),
                                gens.data_ptr(), Bt, None, None, *o, ws.data_ptr(), need.value, stream) == powerflow.GNS_EUNSUPPORTED
        assert lib.gns_fd_solve_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.blob.data_ptr(), ts.words, members.ctypes.data, 1,
                                    grid_off.data_ptr(), None, buses.data_ptr(), lines.data_ptr(), gens.data_ptr(), Bt, None, None, *o,
                                    ws.data_ptr(), need.value, stream) == powerflow.GNS_EUNSUPPORTED
        torch.cuda.synchronize()
        for k in ('v', 'th', 'mis'):
            assert bool((outs[k] == sentinel).all()), k
        assert bool((outs['conv'] == 7).all()) and bool((outs['it'] == -7).all())


@pytest.mark.parametrize('case', ['pair_zero_pivot', 'pair_zero_pivot_start_meets_tol', 'path5_line0_x_zero', 'path5_line3_x_zero'])
def test_failure_rows_with_neighbours(case):
    """A grid whose B' or B'' has a zero or NaN pivot stops at its start point (unless the start already meets the test) with a
    finite mismatch, as the reference does, and the other grids of the batch are bit-identical to the call without it."""
    tp, buses, lines, gens, kw, expect = failure_cases()[case]
    s = Set(tp, (buses, lines, gens), tuple(t.to(DEV) for t in (buses, lines, gens)), None, None)
    others = [i for i in range(FAIL_BATCH) if i != FAIL_ROW]
    tol = kw.get('tol', 1e-8)
    for variant in VARIANTS:
        res = _fd(s, variant, **kw)
        rest = {k: (x[others] if k != 'tol' else x) for k, x in kw.items()}
        _all_same(res, _fd(s._replace(dev=tuple(x[others] for x in s.dev)), variant, **rest), (case, variant), rows=others)
        assert bool((res.iterations[others] > 0).all()), (case, variant, res.iterations)
        i = FAIL_ROW
        bus, line, gen = _grid(s, i)
        start = {k: kw[k][i].numpy() for k in ('v0', 'theta0') if k in kw}
        with np.errstate(all='ignore'):
            vm, va, conv, it, mis = fref.fast_decoupled(bus, line, gen, tp.slack, variant, tol=tol, **start)
        assert bool(res.converged[i]) == conv and bool(torch.isfinite(res.mismatch[i])), (case, variant)
        if expect[variant] == 'iterates':
            assert int(res.iterations[i]) > 0 and abs(int(res.iterations[i]) - it) <= 1, (case, variant, int(res.iterations[i]), it)
            if conv:
                assert np.max(np.abs(_np(res.v[i]) - vm)) <= 1e-9 and np.max(np.abs(_np(res.theta[i]) - va)) <= 1e-9, (case, variant)
            continue
        vm0, va0 = ref.start(bus, gen, tp.slack, start.get('v0'), start.get('theta0'))
        assert int(res.iterations[i]) == 0 and bool(res.converged[i]) == (expect[variant] == 'met'), (case, variant)
        assert np.array_equal(_np(res.v[i]), vm0) and np.array_equal(_np(res.theta[i]), va0), (case, variant)
        assert (float(res.mismatch[i]) < tol) == (expect[variant] == 'met'), (case, variant, float(res.mismatch[i]))
        _check_norm(s, i, vm0, va0, res.mismatch[i], (case, variant))
