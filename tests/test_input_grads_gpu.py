"""Input gradients on the device: d loss / d buses, lines, generators through ``GNS`` (save_state 2, gns_backward_inputs) against the
reference's own autograd (tests/golden/igrad/*.npz) and the fp64 oracle, and the shapes a caller may hand in."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import assert_close, cfg_of, load_golden
from test_input_grads_oracle import IGRAD, LOSSES, load_igrad

pytestmark = pytest.mark.gpu

TOL = 5e-5


def _model(g, frozen=False):
    import opf_graph_neural_solver_amd as amd
    c = cfg_of(g)
    m = amd.GNS(c['latent_dim'], c['hidden_dim'], c['K'], c['gamma'], c['multiple_phi']).cuda()
    with torch.no_grad():
        m.flat_parameters().copy_(torch.as_tensor(g['params']))
    if frozen:
        for p in m.parameters():
            p.requires_grad_(False)
    return m


def _loss(out, ig, loss, dev='cuda'):
    v, th, tot, last = out
    if loss == 'mean':
        return tot.mean()
    w = {k: torch.as_tensor(ig[k], device=dev) for k in ('w_total', 'w_last', 'w_v', 'w_theta')}
    return (w['w_total'] * tot).sum() + (w['w_last'] * last).sum() + (w['w_v'] * v).sum() + (w['w_theta'] * th).sum()


def _inputs(g, dev='cuda'):
    return [torch.as_tensor(g[k]).to(dev).requires_grad_(True) for k in ('buses', 'lines', 'generators')]


def _check_against_golden(grads, ig, loss, what):
    for name, a in zip(('buses', 'lines', 'generators'), grads):
        assert_close(a.detach().cpu(), ig[f'{loss}_grad_{name}'], TOL, abs_floor=1e-6, what=f'{what} {loss} {name}')
    gb, gl, gg = (a.detach().cpu() for a in grads)
    assert torch.all(gb[..., 0:2] == 0) and torch.all(gl[..., 0:2] == 0) and torch.all(gg[..., 0] == 0)


@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('name', IGRAD)
def test_input_grads_match_reference(name, loss):
    g, ig = load_golden(name), load_igrad(name)
    m = _model(g)
    bu, li, ge = _inputs(g)
    _loss(m(bu, li, ge), ig, loss).backward()
    _check_against_golden((bu.grad, li.grad, ge.grad), ig, loss, name)
    if loss == 'mean':          # the parameter gradient of the same call is the existing goldens' one
        grad = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu()
        assert_close(grad, g['grad_params'], TOL if int(g['K']) <= 10 else 2e-4, abs_floor=1e-6, what=f'{name} grad_params')


@pytest.mark.parametrize('name', ['c14_b2_K4_d10_single', 'c118_b2_K4_d20_multi'])
def test_frozen_model_gives_input_grads_and_no_param_grads(name):
    g, ig = load_golden(name), load_igrad(name)
    m = _model(g, frozen=True)
    bu, li, ge = _inputs(g)
    _loss(m(bu, li, ge), ig, 'mixed').backward()
    _check_against_golden((bu.grad, li.grad, ge.grad), ig, 'mixed', name + ' frozen')
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize('case,bt,K,multi', [(14, 128, 4, True), (14, 128, 4, False), (118, 16384, 4, True)])
def test_param_grad_bit_identical_with_and_without_input_grads(case, bt, K, multi):
    import opf_graph_neural_solver_amd as amd
    torch.manual_seed(3)
    m = amd.GNS(20, 10, K, 0.9, multi).cuda()
    bu, li, ge = amd.synth.synth_grids(case, bt, seed=21, device='cuda')
    grads = []
    # a call with input gradients always runs the lane-per-grid forward + split backward; at case14 x 128 a plain call runs the
    # grid-per-workgroup pair by default (same gradient within rounding), and the lane-per-grid pair when asked: bit for bit
    old = amd.get_option('train_mapping')
    try:
        for want_inputs, mapping in ((False, old), (False, 1), (True, old)):
            amd.set_option('train_mapping', mapping)
            m.zero_grad()
            x = [t.clone().requires_grad_(want_inputs) for t in (bu, li, ge)]
            v, th, tot, last = m(*x)
            (tot.mean() + 0.5 * last.mean() + 1e-3 * v.sum()).backward()
            grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone())
            if want_inputs:
                assert all(torch.isfinite(t.grad).all() for t in x)
    finally:
        amd.set_option('train_mapping', old)
    assert torch.equal(grads[1], grads[2])
    assert_close(grads[2].cpu(), grads[0].cpu(), 2e-5, abs_floor=1e-7, what='default mapping')


@pytest.mark.parametrize('case,bt,K,d,multi,seed', [(118, 16384, 4, 20, True, 31), (300, 8192, 10, 20, True, 15)])
def test_full_size_input_grads_against_oracle(case, bt, K, d, multi, seed):
    import opf_graph_neural_solver_amd as amd
    from oracle import gns_oracle as orc
    torch.manual_seed(6)
    m = amd.GNS(d, 10, K, 0.9, multi).cuda()
    bu, li, ge = amd.synth.synth_grids(case, bt, seed=seed, device='cuda')
    sample = [0, bt // 2 + 1, bt - 1]
    w = torch.zeros(bt, device='cuda')
    w[sample] = 1.0
    runs = []
    for _ in range(2):
        x = [t.clone().requires_grad_(True) for t in (bu, li, ge)]
        _, _, tot, _ = m(*x)
        (tot * w).sum().backward()
        runs.append([t.grad.clone() for t in x])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                     # run-to-run bitwise
    assert all(torch.all(r[0][[i for i in range(bt) if i not in sample][:64]] == 0) for r in [runs[0]])
    po = orc.unflatten_params(m.flat_parameters().detach().cpu().double(), d, 10, K, multi)
    for b in sample:
        xo = [t[b].detach().cpu().double().requires_grad_(True) for t in (bu, li, ge)]
        _, _, toto, _ = orc.gns_forward(po, *xo, latent_dim=d, K=K, gamma=0.9, multiple_phi=multi)
        toto.backward()
        for name, a, o in zip(('buses', 'lines', 'generators'), runs[0], xo):
            assert_close(a[b].cpu(), o.grad, TOL, abs_floor=1e-6, what=f'case{case} grid {b} {name}')


def test_cpu_resident_inputs_get_cpu_grads():
    name = 'c14_b2_K4_d10_single'
    g, ig = load_golden(name), load_igrad(name)
    m = _model(g)
    bu, li, ge = _inputs(g, dev='cpu')
    out = m(bu, li, ge)
    assert out[2].device.type == 'cpu'
    _loss(out, ig, 'mixed', dev='cpu').backward()
    assert bu.grad.device.type == 'cpu'
    _check_against_golden((bu.grad, li.grad, ge.grad), ig, 'mixed', 'cpu-resident')


def test_permuted_column_maps_put_grads_in_caller_columns():
    import opf_graph_neural_solver_amd as amd
    name = 'c14_b3_K4_d20_multi_lowload'
    g, ig = load_golden(name), load_igrad(name)
    m = _model(g)
    B0, L0, G0 = amd.gns.get_BLG()
    pb, pl, pg = [5, 3, 0, 1, 4, 2], [6, 0, 4, 2, 1, 5, 3], [3, 6, 0, 5, 1, 4, 2]     # caller column c holds reference column p[c]
    maps = []
    for d0, perm in ((B0, pb), (L0, pl), (G0, pg)):
        inv = {ref: c for c, ref in enumerate(perm)}
        maps.append({k: inv[v] for k, v in d0.items()})
    x = [torch.as_tensor(g[k])[..., p].cuda().requires_grad_(True) for k, p in zip(('buses', 'lines', 'generators'), (pb, pl, pg))]
    _loss(m(*x, *maps), ig, 'mixed').backward()
    for t, perm, key in zip(x, (pb, pl, pg), ('buses', 'lines', 'generators')):
        assert_close(t.grad.cpu(), ig[f'mixed_grad_{key}'][..., perm], TOL, abs_floor=1e-6, what=f'permuted {key}')


def test_single_grid_2d_call():
    name = 'c14_b2_K4_d10_single'
    g, ig = load_golden(name), load_igrad(name)
    m = _model(g)
    x = [torch.as_tensor(g[k][1]).cuda().requires_grad_(True) for k in ('buses', 'lines', 'generators')]
    v, th, tot, last = m(*x)
    assert tot.dim() == 0
    (float(ig['w_total'][1]) * tot + float(ig['w_last'][1]) * last + (torch.as_tensor(ig['w_v'][1]).cuda() * v).sum()
     + (torch.as_tensor(ig['w_theta'][1]).cuda() * th).sum()).backward()
    for t, key in zip(x, ('buses', 'lines', 'generators')):
        assert_close(t.grad.cpu(), ig[f'mixed_grad_{key}'][1], TOL, abs_floor=1e-6, what=f'2-D {key}')


def test_bind_dataset_equals_per_call_packing():
    import opf_graph_neural_solver_amd as amd
    torch.manual_seed(4)
    m = amd.GNS(20, 10, 4, 0.9, True).cuda()
    bu, li, ge = amd.synth.synth_grids(118, 256, seed=8, device='cuda')
    res = []
    for bound in (False, True):
        if bound:
            m.bind_dataset(bu, li, ge)
        x = [t[64:192] for t in (bu, li, ge)]
        leaf = [t.detach().clone().requires_grad_(True) for t in x] if not bound else None
        if bound:        # a slice of the bound tensors themselves: the packed copy is read
            bu.requires_grad_(True); li.requires_grad_(True); ge.requires_grad_(True)
            x = [t[64:192] for t in (bu, li, ge)]
        else:
            x = leaf
        m.zero_grad()
        _, _, tot, last = m(*x)
        (tot.mean() + last.mean()).backward()
        gx = [t.grad[64:192].clone() for t in (bu, li, ge)] if bound else [t.grad.clone() for t in x]
        res.append((gx, torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()))
        if bound:
            assert m._resident is not None and m._resident['hits'] >= 1
            m.unbind_dataset()
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(res[0][1], res[1][1])


def test_grouped_plan_with_input_grads_raises():
    import opf_graph_neural_solver_amd as amd
    m = amd.GNS(10, 10, 3, 0.9, False).cuda()
    m.topology_check = 'group'
    a = [torch.as_tensor(load_golden('c14_b2_K4_d10_single')[k]).cuda() for k in ('buses', 'lines', 'generators')]
    b = [t.clone() for t in a]
    b[1][1, :, 0:2] = b[1][1, :, [1, 0]]            # second grid: every line reversed - another topology
    with pytest.raises(ValueError, match='mixes topologies'):
        m(*[t.requires_grad_(True) for t in b])


def test_poisoned_workspaces_give_the_same_grads():
    import opf_graph_neural_solver_amd as amd
    name = 'odd_ring_isolated_dupgen_b3_K4_d20_multi'
    g, ig = load_golden(name), load_igrad(name)
    m = _model(g)
    outs = []
    for poison in (False, True):
        amd.gns.POISON_WORKSPACES = poison
        try:
            x = _inputs(g)
            m.zero_grad()
            _loss(m(*x), ig, 'mixed').backward()
            outs.append([t.grad.clone() for t in x] + [torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()])
        finally:
            amd.gns.POISON_WORKSPACES = False
    for a, b in zip(*outs):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def test_raw_c_abi_null_param_grad_and_null_input_grad():
    import opf_graph_neural_solver_amd as amd
    from opf_graph_neural_solver_amd.gns import _check
    name = 'c14_b2_K4_d10_single'
    g, ig = load_golden(name), load_igrad(name)
    m = _model(g)
    lib = amd.load_library()
    bu, li, ge = (torch.as_tensor(g[k]).cuda().contiguous() for k in ('buses', 'lines', 'generators'))
    Bt, N, E, Gn = bu.shape[0], bu.shape[1], li.shape[1], ge.shape[1]
    c = cfg_of(g)
    cfg = amd._lib.GnsConfig(N, E, Gn, c['K'], c['latent_dim'], c['hidden_dim'], int(c['multiple_phi']), c['gamma'])
    topo = m._topology(li, ge, N)
    fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib.gns_workspace_bytes(ctypes.byref(cfg), Bt, 2, ctypes.byref(fb), ctypes.byref(bb)), 'ws')
    fb1, bb1 = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib.gns_workspace_bytes(ctypes.byref(cfg), Bt, 1, ctypes.byref(fb1), ctypes.byref(bb1)), 'ws')
    flat = m.flat_parameters()
    v = torch.empty((Bt, N), device='cuda'); th = torch.empty_like(v)
    tot = torch.empty(Bt, device='cuda'); last = torch.empty_like(tot)
    stream = torch.cuda.current_stream().cuda_stream
    gt = torch.full((Bt,), 1.0 / Bt, device='cuda')
    gb = torch.zeros_like(bu); gg = torch.zeros_like(ge)
    bws = torch.empty(bb.value, dtype=torch.uint8, device='cuda')
    # a workspace saved with save_state = 1 is refused
    ws1 = torch.zeros(max(fb1.value, fb.value), dtype=torch.uint8, device='cuda')
    _check(lib.gns_forward(ctypes.byref(cfg), topo.blob.data_ptr(), flat.data_ptr(), bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt,
                           None, v.data_ptr(), th.data_ptr(), tot.data_ptr(), last.data_ptr(), ws1.data_ptr(), fb1.value, 1, stream), 'fwd1')
    rc = lib.gns_backward_inputs(ctypes.byref(cfg), topo.blob.data_ptr(), flat.data_ptr(), bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt,
                                 None, ws1.data_ptr(), ws1.numel(), gt.data_ptr(), None, None, None, None, gb.data_ptr(), None,
                                 gg.data_ptr(), bws.data_ptr(), bws.numel(), stream)
    assert rc == 1
    ws = torch.empty(fb.value, dtype=torch.uint8, device='cuda')
    _check(lib.gns_forward(ctypes.byref(cfg), topo.blob.data_ptr(), flat.data_ptr(), bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt,
                           None, v.data_ptr(), th.data_ptr(), tot.data_ptr(), last.data_ptr(), ws.data_ptr(), ws.numel(), 2, stream), 'fwd2')
    _check(lib.gns_backward_inputs(ctypes.byref(cfg), topo.blob.data_ptr(), flat.data_ptr(), bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt,
                                   None, ws.data_ptr(), ws.numel(), gt.data_ptr(), None, None, None, None, gb.data_ptr(), None,
                                   gg.data_ptr(), bws.data_ptr(), bws.numel(), stream), 'gns_backward_inputs')
    torch.cuda.synchronize()
    assert_close(gb.cpu(), ig['mean_grad_buses'], TOL, abs_floor=1e-6, what='raw buses')
    assert_close(gg.cpu(), ig['mean_grad_generators'], TOL, abs_floor=1e-6, what='raw generators')
