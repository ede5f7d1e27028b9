"""Batches that mix topologies (N-1 contingency sets): ``topology_check = 'group'``, one topology per 64-grid group."""
import numpy as np
import pytest
import torch

from helpers import assert_close

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod

REL = 1e-5


# ---- host logic (no device) ----------------------------------------------------------------------------------------------------
def test_contingency_grids_remove_one_line_per_variant():
    outages = [0, 3, 7, 19]
    bu, li, ge, out = amd.synth.contingency_grids(14, 11, outages, seed=5)
    b0, l0, g0 = amd.synth.synth_grids(14, 11, seed=5)
    assert bu.shape == (11, 14, 6) and li.shape == (11, 19, 7) and ge.shape == (11, 5, 7) and out.shape == (11,)
    assert torch.equal(bu, b0) and torch.equal(ge, g0)
    assert out.tolist() == [outages[i % 4] for i in range(11)]                    # round-robin
    for i in range(11):
        j = int(out[i])
        assert torch.equal(li[i], torch.cat([l0[i, :j], l0[i, j + 1:]]))        # line j gone, the others in order
    _, _, _, out_s = amd.synth.contingency_grids(14, 200, outages, seed=5, shuffle=True)
    assert set(out_s.tolist()) == set(outages) and out_s.tolist() != [outages[i % 4] for i in range(200)]
    with pytest.raises(ValueError):
        amd.synth.contingency_grids(14, 4, [20])                                   # not a line of case14
    with pytest.raises(ValueError):
        amd.synth.contingency_grids(14, 4, [])


def test_contingency_grids_refuse_a_variant_that_breaks_the_bus_id_as_line_index_quirk(monkeypatch):
    # a 5-bus, 5-line case: without line 0 the bus id 5 is left on a line, and E-1 = 4 lines remain
    f = np.array([1, 2, 3, 4, 1]); t = np.array([2, 3, 4, 5, 5])
    monkeypatch.setitem(amd.synth.CASE_SHAPES, 14, (5, 5, 1))
    monkeypatch.setattr(amd.synth, 'case_topology', lambda c: (f, t, np.array([1])))
    with pytest.raises(ValueError, match='E-1'):
        amd.synth.contingency_grids(14, 4, [0])


def test_classification_of_id_rows():
    bu, li, ge, out = amd.synth.contingency_grids(14, 37, [2, 5, 11], seed=1, shuffle=True)
    ids, inverse, counts = gns_mod._classify_ids(li, ge)
    assert ids.shape == (3, 2 * 19 + 5) and counts.sum() == 37
    for i in range(37):                                                            # a grid's row is its own id columns
        row = torch.cat([li[i, :, 0:2].reshape(-1), ge[i, :, 0]]).double()
        assert torch.equal(ids[int(inverse[i])], row)
    same = out.unsqueeze(0) == out.unsqueeze(1)                                    # same class <=> same outage
    assert torch.equal(inverse.unsqueeze(0) == inverse.unsqueeze(1), same)
    bad = li.clone(); bad[4, 2, 0] += 0.5
    with pytest.raises(ValueError, match='integers'):
        gns_mod._classify_ids(bad, ge)


@pytest.mark.parametrize('counts', [[150], [1, 64, 65], [63, 1, 128, 2]])
def test_group_tables_keep_order_and_pad_each_topology_at_its_end(counts):
    g = torch.Generator().manual_seed(len(counts))
    inverse = torch.cat([torch.full((c,), t, dtype=torch.int64) for t, c in enumerate(counts)])
    inverse = inverse[torch.randperm(inverse.numel(), generator=g)]                # grids of the topologies interleaved
    group_idx, slot_grid = gns_mod._group_tables(inverse, torch.tensor(counts))
    gpt = [(c + 63) // 64 for c in counts]
    assert group_idx.tolist() == [t for t, n in enumerate(gpt) for _ in range(n)]
    sg = slot_grid.view(-1, 64)
    assert sg.shape[0] == sum(gpt)
    pos = 0
    for t, c in enumerate(counts):
        slots = sg[pos:pos + gpt[t]].reshape(-1)
        live = slots[:c]
        assert torch.equal(live, torch.nonzero(inverse == t).flatten().to(torch.int32))   # input order within the topology
        assert bool((slots[c:] == -1).all())                                      # padding only behind its last grid
        pos += gpt[t]
    # every input grid sits in exactly one slot: the inverse permutation round-trips
    flat = slot_grid.tolist()
    where = {b: s for s, b in enumerate(flat) if b >= 0}
    assert sorted(where) == list(range(inverse.numel()))
    assert all(flat[where[b]] == b for b in range(inverse.numel()))


def test_topology_check_group_is_documented_in_the_c_abi():
    import ctypes
    lib = amd.load_library()
    for f in ('gns_workspace_bytes_grouped', 'gns_forward_grouped', 'gns_backward_grouped', 'gns_team_status_grouped',
              'gns_team_status_offset_grouped'):
        assert hasattr(lib, f)
    cfg = amd._lib.GnsConfig(14, 19, 5, 3, 10, 10, 0, 0.9)
    fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.gns_workspace_bytes_grouped(ctypes.byref(cfg), 0, 1, ctypes.byref(fb), ctypes.byref(bb)) == 1      # G = 0
    bad = amd._lib.GnsConfig(14, 19, 5, 3, 30, 10, 0, 0.9)                                                        # no kernel holds d = 30
    assert lib.gns_workspace_bytes_grouped(ctypes.byref(bad), 3, 1, ctypes.byref(fb), ctypes.byref(bb)) == 2


# ---- on the device ---------------------------------------------------------------------------------------------------------------
def _oracle_sum(flat, bu, li, ge, idx, d, h, K, multi, wv=None, wth=None, w_tot=0.3, w_last=0.7, check=None):
    """Oracle forward per grid of ``idx`` (optionally checked against ``check = (v, th, tot, last)``) and the gradient of
    ``sum (v wv) + (th wth) + w_tot total + w_last last`` over those grids."""
    from oracle import gns_oracle as orc
    fo = flat.clone().requires_grad_(True)
    po = orc.unflatten_params(fo, d, h, K, multi)
    acc = 0.
    for b in idx:
        vo, tho, toto, lasto = orc.gns_forward(po, bu[b], li[b], ge[b], latent_dim=d, K=K, gamma=0.9, multiple_phi=multi)
        if check is not None:
            v, th, tot, last = check
            assert_close(v[b], vo.detach(), REL, what=f'v[{b}]')
            assert_close(th[b], tho.detach(), REL, what=f'theta[{b}]')
            assert_close(tot[b], toto.detach(), REL, what=f'total[{b}]')
            assert_close(last[b], lasto.detach(), REL, what=f'last[{b}]')
        term = w_tot * toto + w_last * lasto
        if wv is not None:
            term = term + (vo * wv[b]).sum() + (tho * wth[b]).sum()
        acc = acc + term
    acc.backward()
    return fo.grad


def _grad(m):
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('d,h,multi', [(20, 10, True), (10, 10, False), (16, 8, True)])
def test_case14_contingency_batch_matches_the_oracle(d, h, multi):
    torch.manual_seed(3)
    K = 3
    m = amd.GNS(d, h, K, 0.9, multi).cuda()
    m.topology_check = 'group'
    Bt = 150
    bu, li, ge, out = amd.synth.contingency_grids(14, Bt, [1, 4, 9, 13, 17], seed=11, shuffle=True)
    wv, wth = torch.randn(Bt, 14), torch.randn(Bt, 14)
    v, th, tot, last = m(bu.cuda(), li.cuda(), ge.cuda())
    loss = (v * wv.cuda()).sum() + (th * wth.cuda()).sum() + 0.3 * tot.sum() + 0.7 * last.sum()
    loss.backward()
    res = tuple(x.detach().cpu() for x in (v, th, tot, last))
    g_o = _oracle_sum(m.flat_parameters().detach().cpu(), bu, li, ge, range(Bt), d, h, K, multi, wv, wth, check=res)
    assert_close(_grad(m), g_o, 5e-5, abs_floor=1e-6, what=f'grad ({d},{h},{multi})')


def _c118_set(S=4096):
    outages = list(range(3, 186, 12))[:16]
    return amd.synth.contingency_grids(118, S, outages, seed=2, shuffle=True, device='cuda')


@pytest.mark.gpu
def test_case118_contingency_batch_against_oracle_and_single_topology_calls():
    torch.manual_seed(5)
    d, h, K, multi = 20, 10, 2, True
    m = amd.GNS(d, h, K, 0.9, multi).cuda()
    m.topology_check = 'group'
    bu, li, ge, out = _c118_set()
    S = bu.shape[0]
    wsel = torch.zeros(S, device='cuda')
    pick_g = [5, 1000, 2222, 4095]
    wsel[pick_g] = 1.0
    v, th, tot, last = m(bu, li, ge)
    (0.3 * (tot * wsel).sum() + 0.7 * (last * wsel).sum()).backward()
    res = tuple(x.detach().cpu() for x in (v, th, tot, last))
    bc, lc, gc = bu.cpu(), li.cpu(), ge.cpu()
    # forward on 6 grids, one of them the last grid of a topology whose last group is padded
    o = out.cpu()
    cnt = {int(j): int((o == j).sum()) for j in o.unique()}
    padded = next(j for j, c in cnt.items() if c % 64)
    last_of_padded = int(torch.nonzero(o == padded).flatten()[-1])
    flat = m.flat_parameters().detach().cpu()
    _oracle_sum(flat, bc, lc, gc, [0, 17, 777, 3001, 4094, last_of_padded], d, h, K, multi, check=res)
    g_o = _oracle_sum(flat, bc, lc, gc, pick_g, d, h, K, multi)
    assert_close(_grad(m), g_o, 5e-5, abs_floor=1e-6, what='0/1-weighted gradient')
    # per topology: a plain one-topology call on that topology's grids alone (same lane-per-grid kernels)
    old = amd.get_option('fwd_mapping')
    amd.set_option('fwd_mapping', 1)
    try:
        with torch.no_grad():
            for j in cnt:
                idx = torch.nonzero(out == j).flatten()
                ref = amd.GNS(d, h, K, 0.9, multi).cuda()
                ref.load_state_dict(m.state_dict())
                r = ref(bu[idx], li[idx], ge[idx])
                for a, b, what in zip(res, r, ('v', 'theta', 'total', 'last')):
                    assert_close(a[idx.cpu()], b.cpu(), 1e-6, abs_floor=0.0, what=f'{what}, outage {j}')
    finally:
        amd.set_option('fwd_mapping', old)


@pytest.mark.gpu
def test_mixed_batch_reads_nothing_unwritten():
    torch.manual_seed(9)
    m = amd.GNS(20, 10, 3, 0.9, True).cuda()
    m.topology_check = 'group'
    bu, li, ge, _ = amd.synth.contingency_grids(14, 333, [0, 5, 10, 15], seed=4, shuffle=True, device='cuda')
    old = gns_mod.POISON_WORKSPACES
    gns_mod.POISON_WORKSPACES = True
    try:
        v, th, tot, last = m(bu, li, ge)
        (v.sum() + th.sum() + tot.sum() + last.sum()).backward()
    finally:
        gns_mod.POISON_WORKSPACES = old
    for x in (v, th, tot, last):
        assert bool(torch.isfinite(x).all())
    assert bool(torch.isfinite(_grad(m)).all())


@pytest.mark.gpu
def test_mixed_batch_with_and_without_teams_agree():
    torch.manual_seed(2)
    m = amd.GNS(20, 10, 3, 0.9, True).cuda()
    m.topology_check = 'group'
    bu, li, ge, _ = amd.synth.contingency_grids(14, 300, [1, 2, 3], seed=8, shuffle=True, device='cuda')
    old = amd.get_option('team')
    outs = []
    try:
        for team in (0, 1):
            amd.set_option('team', team)
            m.zero_grad()
            v, th, tot, last = m(bu, li, ge)
            (tot.sum() + last.sum()).backward()
            outs.append([x.detach().cpu() for x in (v, th, tot, last)] + [_grad(m)])
    finally:
        amd.set_option('team', old)
    for a, b, what in zip(outs[0], outs[1], ('v', 'theta', 'total', 'last', 'grad')):
        assert_close(a, b, 1e-6, abs_floor=1e-7, what=what)


@pytest.mark.gpu
def test_fit_on_a_mixed_set_matches_an_eager_oracle_loop():
    from oracle import gns_oracle as orc
    torch.manual_seed(4)
    d, h, K, multi = 20, 10, 3, True
    m = amd.GNS(d, h, K, 0.9, multi).cuda()
    flat0 = m.flat_parameters().detach().cpu().clone()
    S = 96
    bu, li, ge, _ = amd.synth.contingency_grids(14, S, [2, 6, 12], seed=6, shuffle=True, device='cuda')
    hist = amd.training.fit(m, bu, li, ge, epochs=2, batch_size=S, lr=1e-3, case_nr=14, log=lambda s: None, mixed_topologies=True)
    assert m.topology_check == 'always'                                           # restored
    p = flat0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-3)
    finals = []
    bc, lc, gc = bu.cpu(), li.cpu(), ge.cpu()
    for _ in range(2):
        _, _, _, last, grad = orc.gns_forward_backward(p.detach(), bc, lc, gc, latent_dim=d, hidden_dim=h, K=K, gamma=0.9,
                                                       multiple_phi=multi)
        finals.append(float(torch.as_tensor(last).mean()))
        p.grad = torch.as_tensor(grad, dtype=p.dtype).reshape(p.shape)
        opt.step()
    assert_close(np.array(hist), np.array(finals), REL, abs_floor=0.0, what='epoch losses')
    # Adam's normalised update turns a gradient element that is fp32 rounding noise (the linear1 column fed by delta_q, main.py:83,103)
    # into +-lr in any two implementations (test_gpu_parity.py, the reference-loop test): 99 % of the weights agree to 5e-5 of max|w|,
    # none differs by more than the 2 steps x 2 lr of an opposite sign; the gradients themselves are compared at 5e-5 above
    mine, ref = m.flat_parameters().detach().cpu(), p.detach()
    assert float((mine - flat0).abs().max()) > 1e-4
    tol = 1e-7 + 5e-5 * float(ref.abs().max())
    diff = (mine - ref).abs()
    assert float((diff <= tol).double().mean()) >= 0.99, 'Adam: fewer than 99 % of the weights within 5e-5'
    assert float(diff.max()) <= 2 * 2 * 1e-3 + tol


@pytest.mark.gpu
def test_group_on_a_uniform_batch_is_bit_identical_to_always():
    torch.manual_seed(1)
    m = amd.GNS(20, 10, 3, 0.9, True).cuda()
    bu, li, ge = amd.synth.synth_grids(118, 300, seed=3, device='cuda')
    res = []
    for check in ('always', 'group'):
        m.topology_check = check
        m.zero_grad()
        v, th, tot, last = m(bu, li, ge)
        (tot.sum() + v.sum()).backward()
        res.append([x.detach().cpu() for x in (v, th, tot, last)] + [_grad(m)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_group_still_refuses_bad_ids_and_one_topology_paths_refuse_mixed_sets():
    m = amd.GNS(20, 10, 2, 0.9, True).cuda()
    m.topology_check = 'group'
    bu, li, ge, _ = amd.synth.contingency_grids(14, 70, [0, 1], seed=0, device='cuda')
    bad = li.clone(); bad[3, 2, 1] = 15.0                                          # bus id out of range in one grid
    with pytest.raises(ValueError):
        m(bu, bad, ge)
    bad = li.clone(); bad[5, 0, 0] = 1.5                                           # not an integer
    with pytest.raises(ValueError):
        m(bu, bad, ge)
    with pytest.raises(ValueError):
        m.bind_dataset(bu, li, ge)
    opt = amd.training.make_optimizer(m)
    with pytest.raises(ValueError):
        amd.training.GraphedStep(m, opt, bu[:64], li[:64], ge[:64])
    m.topology_check = 'always'
    with pytest.raises(ValueError):
        m(bu, li, ge)
