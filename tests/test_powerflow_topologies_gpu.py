"""Newton-Raphson power flow on the MI355X over the generated topology families of ``pf_topologies`` in two value regimes: the
start and the mismatch after zero steps, one Newton step against the reference Jacobian (the test that pins the Jacobian, the
Y-bus stamps and the elimination program on the device), full solves from a flat start against the reference NR, the adjoint
against the float64 oracle, the LDS limit (the largest topologies that fit, a mixed batch of very different images, refusals)
and batch independence."""
import ctypes

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow
from opf_graph_neural_solver_amd._lib import PfConfig
import nr_grad_reference as gref
import nr_reference as ref
import pf_topologies as pt

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = 3
NAMES = ('buses', 'lines', 'generators')
EPS = np.finfo(np.float64).eps
# a chain of hundreds of PQ buses has a small Newton basin: its boundary grids get a smooth solution and a close start
CALM = dict(spread=1e-3, v_spread=1e-3)
CALM_START = dict(d_theta=5e-4, d_v=2.5e-4)


def _family_sets():
    """(family, regime) -> (topo, buses, lines, gens, v, theta) on the device."""
    out = {}
    for name, tp in pt.families().items():
        for regime in pt.REGIMES:
            out[name, regime] = (tp, *pt.grids(tp, regime, BATCH, seed=11, device=DEV))
    return out


@pytest.fixture(scope='module')
def sets():
    return _family_sets()


@pytest.fixture(scope='module')
def boundary_sets():
    b = pt.boundary()
    out = {}
    for regime in pt.REGIMES:
        out['path_fit', regime] = (b['path_fit'], *pt.grids(b['path_fit'], regime, 1, seed=0, device=DEV, **CALM))
        out['complete_fit', regime] = (b['complete_fit'], *pt.grids(b['complete_fit'], regime, 2, seed=0, device=DEV))
    return out


def _same(a, b):
    """Bit-identical, NaN included."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0, a), torch.where(b.isnan(), 0, b))


def _cpu(*ts):
    return [t.double().cpu().numpy() for t in ts]


def _start(tp, v, theta, seed, calm=False):
    return pt.perturbed_start(v.cpu(), theta.cpu(), tp.slack, seed, **(CALM_START if calm else {}))


def test_zero_steps_return_the_start_and_its_mismatch(sets):
    """max_iter = 0 from a warm start: the start exactly as include/gns_powerflow.h defines it, and ||F||_inf of the reference."""
    for (name, regime), (tp, buses, lines, gens, v, theta) in sets.items():
        v0, th0 = _start(tp, v, theta, 1)
        res = powerflow.newton_raphson(buses, lines, gens, slack_bus=tp.slack, v0=v0.to(DEV), theta0=th0.to(DEV), max_iter=0)
        assert bool((res.iterations == 0).all()), (name, regime)
        for i in range(BATCH):
            bus, line, gen = _cpu(buses[i], lines[i], gens[i])
            vm, va = ref.start(bus, gen, tp.slack, v0[i].numpy(), th0[i].numpy())
            assert np.array_equal(res.v[i].cpu().numpy(), vm), (name, regime, i)
            assert np.array_equal(res.theta[i].cpu().numpy(), va), (name, regime, i)
            F = ref.mismatch_vector(bus, line, gen, tp.slack, vm, va)
            Y = ref.ybus(bus, line)
            V = vm * np.exp(1j * va)
            scale = np.max(np.abs(V) * (abs(Y) @ np.abs(V)) + np.abs(ref.specified(bus, gen)))
            deg = int(np.max(np.diff(Y.indptr))) + 2
            assert abs(float(res.mismatch[i]) - np.max(np.abs(F))) <= 4 * deg * EPS * scale, (name, regime, i)


def _one_step_ratios(tp, buses, lines, gens, v0, th0, mixed, calm=False):
    """(scipy's, the device's) one-step residual ratios of every grid: max_iter = 1, tol = 0 from (v0, theta0)."""
    res = powerflow.newton_raphson(buses, lines, gens, slack_bus=tp.slack, v0=v0.to(DEV), theta0=th0.to(DEV), max_iter=1, tol=0.0,
                                   mixed_topologies=mixed)
    assert bool((res.iterations == 1).all()), (tp.name, res.iterations)
    out = []
    for i in range(buses.shape[0]):
        bus, line, gen = _cpu(buses[i], lines[i], gens[i])
        slack, pv, pq = ref.roles(bus, gen, tp.slack)
        pvpq = np.r_[pv, pq]
        vm, va = ref.start(bus, gen, tp.slack, v0[i].numpy(), th0[i].numpy())
        J = ref.jacobian(bus, line, gen, tp.slack, vm, va)
        F = ref.mismatch_vector(bus, line, gen, tp.slack, vm, va)
        v1, t1 = res.v[i].cpu().numpy(), res.theta[i].cpu().numpy()
        dx = np.r_[va[pvpq] - t1[pvpq], vm[pq] - v1[pq]]
        out.append((pt.one_step_ratio(J, F, spla.spsolve(J, F)), pt.one_step_ratio(J, F, dx)))
    return out


@pytest.mark.parametrize('mixed', [False, True])
def test_one_newton_step_solves_the_reference_jacobian(sets, boundary_sets, mixed):
    worst = {}
    every = list(sets.items()) + list(boundary_sets.items())
    for (name, regime), (tp, buses, lines, gens, v, theta) in every:
        v0, th0 = _start(tp, v, theta, 2, calm=name == 'path_fit')
        for k, (r_scipy, r_dev) in enumerate(_one_step_ratios(tp, buses, lines, gens, v0, th0, mixed)):
            assert r_scipy <= pt.STEP_TOL, (name, regime, k, r_scipy)          # the grid is conditioned well enough ...
            assert r_dev <= pt.STEP_TOL, (name, regime, k, r_dev)              # ... so a failure here is the kernel's
            worst[name] = max(worst.get(name, 0.0), r_dev)
    print('largest one-step residual ratio per family (mixed=%s):' % mixed, {k: f'{r:.1e}' for k, r in worst.items()})


def test_flat_start_solves_match_the_reference(sets, boundary_sets):
    n_ref_conv, n_same = 0, 0
    for (name, regime), (tp, buses, lines, gens, v, theta) in list(sets.items()) + list(boundary_sets.items()):
        res = powerflow.newton_raphson(buses, lines, gens, slack_bus=tp.slack)
        for i in range(buses.shape[0]):
            bus, line, gen = _cpu(buses[i], lines[i], gens[i])
            vm, va, conv, it, _ = ref.newton_raphson(bus, line, gen, tp.slack)
            if not conv:
                continue
            n_ref_conv += 1
            assert bool(res.converged[i]), (name, regime, i)
            assert np.max(np.abs(res.v[i].cpu().numpy() - vm)) <= 1e-9, (name, regime, i)
            assert np.max(np.abs(res.theta[i].cpu().numpy() - va)) <= 1e-9, (name, regime, i)
            d = abs(int(res.iterations[i]) - it)
            assert d <= 1, (name, regime, i, int(res.iterations[i]), it)
            n_same += d == 0
    assert n_ref_conv >= 60 and n_same >= 0.99 * n_ref_conv, (n_same, n_ref_conv)


def _grads(tp, buses, lines, gens, a, b, **kw):
    ins = [t.detach().clone().requires_grad_(True) for t in (buses, lines, gens)]
    res = powerflow.newton_raphson(*ins, slack_bus=tp.slack, **kw)
    return res, torch.autograd.grad((a * res.v + b * res.theta).sum(), ins)


def _weights(bt, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(bt, n, generator=g, dtype=torch.float64).to(DEV), torch.randn(bt, n, generator=g, dtype=torch.float64).to(DEV))


def _check_against_oracle(tp, buses, lines, gens, res, grads, a, b, rows, what):
    for i in rows:
        want = gref.implicit_gradient(buses[i].double().cpu(), lines[i].double().cpu(), gens[i].double().cpu(), tp.slack,
                                      res.v[i].cpu(), res.theta[i].cpu(), a[i].cpu(), b[i].cpu())
        for k in range(3):
            got = grads[k][i].double().cpu().numpy()
            err, scale = np.max(np.abs(got - want[k])), np.max(np.abs(want[k]))
            assert err <= 1e-5 * scale + 1e-7, (what, i, NAMES[k], err, scale)


def test_adjoint_matches_the_float64_oracle(sets):
    for (name, regime), (tp, buses, lines, gens, v, theta) in sets.items():
        v0, th0 = _start(tp, v, theta, 3, calm=True)
        a, b = _weights(BATCH, tp.n, 5)
        res, grads = _grads(tp, buses, lines, gens, a, b, v0=v0.to(DEV), theta0=th0.to(DEV))
        assert bool(res.converged.all()), (name, regime, res.mismatch)
        _check_against_oracle(tp, buses, lines, gens, res, grads, a, b, range(2), (name, regime))


def test_largest_fitting_topologies_solve_and_differentiate(boundary_sets):
    for (name, regime), (tp, buses, lines, gens, v, theta) in boundary_sets.items():
        info = pt._info(tp)
        assert info['lds_bytes'] <= pt.LDS_LIMIT
        v0, th0 = _start(tp, v, theta, 0, calm=name == 'path_fit')
        a, b = _weights(buses.shape[0], tp.n, 6)
        kw = dict(v0=v0.to(DEV), theta0=th0.to(DEV))
        res, grads = _grads(tp, buses, lines, gens, a, b, **kw)
        assert bool(res.converged.all()), (name, regime, res.mismatch)
        for i in range(buses.shape[0]):
            bus, line, gen = _cpu(buses[i], lines[i], gens[i])
            vm, va, conv, _, _ = ref.newton_raphson(bus, line, gen, tp.slack, v0=v0[i].numpy(), theta0=th0[i].numpy())
            assert conv, (name, regime, i)
            assert np.max(np.abs(res.v[i].detach().cpu().numpy() - vm)) <= 1e-9, (name, regime, i)
            assert np.max(np.abs(res.theta[i].detach().cpu().numpy() - va)) <= 1e-9, (name, regime, i)
        mres, mgrads = _grads(tp, buses, lines, gens, a, b, mixed_topologies=True, **kw)
        for k in res._fields:
            assert torch.equal(getattr(res, k), getattr(mres, k)), (name, regime, k)
        for g, h in zip(grads, mgrads):
            assert torch.equal(g, h), (name, regime)
        _check_against_oracle(tp, buses, lines, gens, res, grads, a, b, range(1), (name, regime))
        print(f'{name} ({regime}): N={tp.n} E={tp.f.size} lds={info["lds_bytes"]} B, steps={info["n_steps"]}, ops={info["n_ops"]}, '
              f'adjoint steps={info["n_factor_steps"] + info["n_adj_steps"]}, iterations={res.iterations.tolist()}')


def _star_like(tp):
    """A star of tp's N, E and Gn: hub bus 1 (tp's slack) with every other bus a leaf; generators on tp's generator buses."""
    assert tp.slack == 1 and tp.f.size == tp.n - 1
    f, t = np.ones(tp.n - 1, dtype=np.int64), np.arange(2, tp.n + 1, dtype=np.int64)
    return pt.Topo(f'star_like_{tp.name}', tp.n, f, t, tp.g.copy(), 1)


def test_mixed_batch_of_very_different_images_matches_plain_calls():
    path = pt.boundary()['path_fit']
    star = _star_like(path)
    ip, istar = pt._info(path), pt._info(star)
    assert ip['lds_bytes'] > 1.5 * istar['lds_bytes'] and ip['nnz_lu'] > 2.5 * istar['nnz_lu']
    gp = pt.grids(path, 'reference', 3, seed=7, device=DEV, **CALM)
    gs = pt.grids(star, 'reference', 3, seed=7, device=DEV, **CALM)
    # interleaved: path, star, path, star, ...
    order = torch.tensor([0, 3, 1, 4, 2, 5], device=DEV)
    bl = [torch.cat([x, y])[order] for x, y in zip(gp[:3], gs[:3])]
    v0 = torch.cat([gp[3], gs[3]])[order].cpu()
    th0 = torch.cat([gp[4], gs[4]])[order].cpu()
    v0, th0 = pt.perturbed_start(v0, th0, 1, 8, **CALM_START)
    a, b = _weights(6, path.n, 9)
    kw = dict(v0=v0.to(DEV), theta0=th0.to(DEV))
    mres, mgrads = _grads(path, *bl, a, b, mixed_topologies=True, **kw)
    for idx in ([0, 2, 4], [1, 3, 5]):
        sel = torch.tensor(idx, device=DEV)
        pres, pgrads = _grads(path, *(x[sel] for x in bl), a[sel], b[sel], v0=kw['v0'][sel], theta0=kw['theta0'][sel])
        for k in pres._fields:
            assert _same(getattr(mres, k)[sel], getattr(pres, k)), (idx, k)
        for g, h in zip(mgrads, pgrads):
            assert _same(g[sel], h), idx
    assert int(mres.converged.sum()) >= 3, mres.mismatch
    # the same grids sorted by topology
    srt = torch.tensor([0, 2, 4, 1, 3, 5], device=DEV)
    sres, sgrads = _grads(path, *(x[srt] for x in bl), a[srt], b[srt], mixed_topologies=True, v0=kw['v0'][srt],
                          theta0=kw['theta0'][srt])
    for k in sres._fields:
        assert _same(getattr(sres, k), getattr(mres, k)[srt]), k
    for g, h in zip(sgrads, mgrads):
        assert _same(g, h[srt])


def _over_grids():
    tp = pt.boundary()['path_over']
    return tp, pt.grids(tp, 'reference', 2, seed=1, device=DEV, **CALM)


def test_over_the_limit_is_refused_with_its_lds_image():
    tp, (buses, lines, gens, v, theta) = _over_grids()
    lds = pt._info(tp)['lds_bytes']
    assert lds > pt.LDS_LIMIT
    for mixed in (False, True):
        with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
            powerflow.newton_raphson(buses, lines, gens, slack_bus=tp.slack, mixed_topologies=mixed)
        assert f'{lds} B' in str(e.value) and 'latent_dim' not in str(e.value)
    # a mixed batch with one member over the limit is refused as a whole
    star = _star_like(tp)
    sb, sl, sg, _, _ = pt.grids(star, 'reference', 2, seed=1, device=DEV, **CALM)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE):
        powerflow.newton_raphson(torch.cat([sb, buses]), torch.cat([sl, lines]), torch.cat([sg, gens]), slack_bus=1,
                                 mixed_topologies=True)
    # ... while its other member alone solves
    assert bool(powerflow.newton_raphson(sb, sl, sg, slack_bus=1, mixed_topologies=True).converged.all())


def test_raw_entries_refuse_over_the_limit_and_write_nothing():
    tp, (buses, lines, gens, v, theta) = _over_grids()
    lib = amd.load_library()
    topo = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack, device=DEV)
    Bt, N = buses.shape[0], tp.n
    cfg = PfConfig(N, tp.f.size, tp.g.size, 10, 1e-8)
    need = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
    ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    ts = powerflow._PfTopologySet(DEV)
    off = ts.add(('over',), topo)
    ts.sync()
    members = np.array([off], dtype=np.int32)
    grid_off = torch.full((Bt,), off, dtype=torch.int32, device=DEV)
    need_s = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.words, members.ctypes.data, 1, Bt,
                                          ctypes.byref(need_s)) == 2
    stream = torch.cuda.current_stream().cuda_stream
    sentinel = -12345.0
    outs = dict(v=torch.full((Bt, N), sentinel, dtype=torch.float64, device=DEV),
                th=torch.full((Bt, N), sentinel, dtype=torch.float64, device=DEV),
                conv=torch.full((Bt,), 7, dtype=torch.uint8, device=DEV), it=torch.full((Bt,), -7, dtype=torch.int32, device=DEV),
                mis=torch.full((Bt,), sentinel, dtype=torch.float64, device=DEV))
    gin = [torch.full_like(t, sentinel) for t in (buses, lines, gens)]
    vin, thin = v.contiguous(), theta.contiguous()
    conv_in = torch.ones(Bt, dtype=torch.uint8, device=DEV)
    gv, gth = torch.ones_like(vin), torch.ones_like(thin)
    o = [outs[k].data_ptr() for k in ('v', 'th', 'conv', 'it', 'mis')]
    g_p = [t.data_ptr() for t in gin]
    assert lib.gns_pf_solve(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), buses.data_ptr(), lines.data_ptr(),
                            gens.data_ptr(), Bt, None, None, *o, ws.data_ptr(), need.value, stream) == 2
    assert lib.gns_pf_solve_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.blob.data_ptr(), ts.words, members.ctypes.data, 1,
                                grid_off.data_ptr(), None, buses.data_ptr(), lines.data_ptr(), gens.data_ptr(), Bt, None, None, *o,
                                ws.data_ptr(), need.value, stream) == 2
    assert lib.gns_pf_adjoint(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), buses.data_ptr(), lines.data_ptr(),
                              gens.data_ptr(), Bt, vin.data_ptr(), thin.data_ptr(), conv_in.data_ptr(), gv.data_ptr(),
                              gth.data_ptr(), *g_p, ws.data_ptr(), need.value, stream) == 2
    assert lib.gns_pf_adjoint_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.blob.data_ptr(), ts.words, members.ctypes.data, 1,
                                  grid_off.data_ptr(), None, buses.data_ptr(), lines.data_ptr(), gens.data_ptr(), Bt, vin.data_ptr(),
                                  thin.data_ptr(), conv_in.data_ptr(), gv.data_ptr(), gth.data_ptr(), *g_p, ws.data_ptr(),
                                  need.value, stream) == 2
    torch.cuda.synchronize()
    for k in ('v', 'th', 'mis'):
        assert bool((outs[k] == sentinel).all()), k
    assert bool((outs['conv'] == 7).all()) and bool((outs['it'] == -7).all())
    for t in gin:
        assert bool((t == sentinel).all())


def test_every_family_grid_alone_matches_its_batch(sets):
    for (name, regime), (tp, buses, lines, gens, v, theta) in sets.items():
        a, b = _weights(BATCH, tp.n, 10)
        res, grads = _grads(tp, buses, lines, gens, a, b)
        for i in range(BATCH):
            one, g1 = _grads(tp, buses[i], lines[i], gens[i], a[i], b[i])
            for k in res._fields:
                x, y = getattr(one, k), getattr(res, k)[i]
                assert torch.equal(x.isnan(), y.isnan()) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), (name, regime, i, k)
            for g, h in zip(g1, grads):
                assert torch.equal(g.isnan(), h[i].isnan()) and torch.equal(torch.nan_to_num(g), torch.nan_to_num(h[i])), (name, i)
