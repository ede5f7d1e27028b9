"""The training forward saves the first-layer activations of every L net where it used to save the hidden sum the net reads, and the
split backward's sweeps start from them: layer 1 is not recomputed, the hidden sum is rebuilt from the lines the phi net walks anyway
and the dW1 windows that hold its columns run after the bus's line loop (gns_backward_split.hip, BwdsL::bus / finish; option
``bwds_save``, read back as ``last.bwds_save``).  The change removes a recomputation whose result the forward already had and
rebuilds a sum in the forward's own order, so nothing may move: outputs and the flat gradient are bit-identical to ``bwds_save = 0``.

Shapes (latent 20, hidden 10, three phis): the smallest at which the rebuilt sum or the deferred windows can go wrong.
  case14 x 70   two groups, the second ragged; eight chunks of one or two buses.  A bus without in-line (the sum is rebuilt as zero and
                the line loop never runs, yet the deferred windows must), generator buses (the forward stores nothing for the v family
                there), a bus with three in-lines.  K = 1 (only the last step: no L_m sweep), 2 (a step-0 kernel beside a last step),
                3 (a middle step).
  case30 x 64   several buses per chunk, K = 2.
Reference: the float64 oracle (helpers.oracle64) on a sample of grids under a weighted loss that is zero outside the sample, with the
tolerances of tests/test_gpu_parity.py: 1e-5 of the tensor's scale (+1e-6) for outputs, 5e-5 (+1e-7) for the gradient."""
import numpy as np
import pytest
import torch

from helpers import assert_close, loss_weights, options, oracle64, weighted_loss

pytestmark = pytest.mark.gpu

REL, REL_GRAD = 1e-5, 5e-5
# name -> (case, batch, K, latent, sampled grids); eight bus chunks everywhere
SHAPES = {
    'c14x70_K1': (14, 70, 1, 20, [0, 63, 64, 69]),
    'c14x70_K2': (14, 70, 2, 20, [0, 63, 64, 69]),
    'c14x70_K3': (14, 70, 3, 20, [0, 1, 63, 64, 69]),
    'c30x64_K2': (30, 64, 2, 20, [0, 31, 63]),
    'c14x70_K2_d10': (14, 70, 2, 10, [0, 63, 64, 69]),
    'c14x150_K2_mixed': (14, 150, 2, 20, [0, 1, 77, 149]),       # a contingency set: three topologies, each in 64-grid groups of its own
}
OUTAGES = [1, 4, 9]
MAIN = ['c14x70_K1', 'c14x70_K2', 'c14x70_K3', 'c30x64_K2']
CHUNKS = 8
OUTS = ('v', 'theta', 'total', 'last')


class Data:
    pass


@pytest.fixture(scope='module')
def store():
    return {}


def _dataset(store, name):
    """Model, grids, loss weights and the oracle's results of a shape: computed once, shared by the tests, never changed."""
    if name not in store:
        import opf_graph_neural_solver_amd as amd
        case, bt, K, d, sample = SHAPES[name]
        D = Data()
        torch.manual_seed(2000 + case + bt + K + d)
        D.model = amd.GNS(d, 10, K, 0.9, True).cuda()
        D.model.topology_check = 'first'
        if name.endswith('_mixed'):
            D.x = amd.synth.contingency_grids(case, bt, OUTAGES, seed=case + K + 3, shuffle=True, device='cuda')[:3]
        else:
            D.x = amd.synth.synth_grids(case, bt, seed=case + K + 3, device='cuda')
        D.cfg = dict(latent_dim=d, hidden_dim=10, K=K, gamma=0.9, multiple_phi=True)
        D.sample = sample
        D.w = loss_weights(bt, D.x[0].shape[1], sample, seed=11 * bt + K)
        D.o32, D.o64 = oracle64(D.model.flat_parameters(), *D.x, D.cfg, sample, D.w)
        store[name] = D
    return store[name]


def _run(D, save=1, mode=1, variant=4, grouped=False, input_grads=False):
    """One training call through the lane-per-grid forward and its backward; returns the results and ``last.bwds_save``."""
    import opf_graph_neural_solver_amd as amd
    x = D.x
    if input_grads:
        x = (D.x[0].clone().requires_grad_(True), D.x[1], D.x[2])
    check = D.model.topology_check
    try:
        if grouped:
            D.model.topology_check = 'group'
        with options(train_mapping=1, bwd_variant=variant, dw_mfma=1, bwds_mode=mode, bwds_chunks=CHUNKS, bwds_save=save):
            D.model.zero_grad()
            out = D.model(*x)
            weighted_loss(out, D.w).backward()
            torch.cuda.synchronize()
            path = {n: amd.get_option('last.' + n) for n in ('bwd_kernel', 'bwds_mode', 'bwds_save')}
    finally:
        D.model.topology_check = check
    assert path['bwd_kernel'] == variant, path
    if variant == 4:
        assert path['bwds_mode'] == mode, path
    r = {k: o.detach() for k, o in zip(OUTS, out)}
    assert all(p.grad is not None for p in D.model.parameters())
    r['grad'] = torch.cat([p.grad.reshape(-1) for p in D.model.parameters()])
    return r, path['bwds_save']


def _assert_oracle(D, r, what):
    idx = torch.as_tensor(D.sample, device='cuda')
    for k in OUTS:
        assert_close(r[k][idx].cpu(), D.o64[k], REL, what=f'{what}: {k}')
    assert_close(r['grad'].cpu(), D.o64['grad_params'], REL_GRAD, abs_floor=1e-7, what=f'{what}: grad_params')


def test_case14_has_the_buses_this_file_is_about():
    import opf_graph_neural_solver_amd as amd
    f_bus, t_bus, gen_bus = amd.synth.case_topology(14)
    indeg = np.bincount(np.asarray(t_bus, dtype=np.int64), minlength=15)[1:]
    gens = set(int(b) for b in gen_bus)
    assert indeg.min() == 0 and indeg.max() >= 3, indeg            # a bus without in-line (sum rebuilt as zero), one with at least three
    assert gens and len(gens) < 14, gens                           # generator buses (no v-family rows) beside buses without one
    assert any(indeg[b - 1] > 0 for b in gens), (gens, indeg)      # ... one of them with in-lines: rows phi_v would have summed


@pytest.mark.parametrize('name', MAIN)
def test_saved_activations_match_float64_oracle(store, name):
    D = _dataset(store, name)
    r, saved = _run(D, save=1)
    assert saved == 1, saved
    _assert_oracle(D, r, f'{name} bwds_save 1')


@pytest.mark.parametrize('name', MAIN)
def test_saved_activations_give_the_bits_of_hidden_sums(store, name):
    D = _dataset(store, name)
    (a, sa), (b, sb) = _run(D, save=1), _run(D, save=0)
    assert (sa, sb) == (1, 0), (sa, sb)
    for k in OUTS + ('grad',):
        assert torch.equal(a[k], b[k]), f'{name}: {k} differs between bwds_save 1 and 0 (max {float((a[k] - b[k]).abs().max()):.3e})'


@pytest.mark.parametrize('name', MAIN)
def test_poisoned_workspaces_keep_the_bits(store, name, monkeypatch):
    """The v-family rows of generator buses are no longer written: nothing may read them (0xFF bytes would come back as NaN)."""
    import opf_graph_neural_solver_amd as amd
    D = _dataset(store, name)
    clean, _ = _run(D, save=1)
    monkeypatch.setattr(amd.gns, 'POISON_WORKSPACES', True)
    dirty, saved = _run(D, save=1)
    assert saved == 1, saved
    assert torch.isfinite(dirty['grad']).all(), f'{name}: non-finite gradient from a poisoned workspace'
    for k in OUTS + ('grad',):
        assert torch.equal(clean[k], dirty[k]), f'{name}: {k} depends on what the workspace held'


ROUTES = {
    'mode 0': ('c14x70_K2', dict(mode=0)),
    'mode 2': ('c14x70_K2', dict(mode=2)),
    'bwd_variant 2': ('c14x70_K2', dict(variant=2)),
    'latent 10': ('c14x70_K2_d10', dict()),
    'grouped': ('c14x150_K2_mixed', dict(grouped=True)),
    'input gradients': ('c14x70_K2', dict(input_grads=True)),
}


@pytest.mark.parametrize('route', list(ROUTES))
def test_every_other_call_keeps_the_hidden_sums(store, route):
    """The option is on (its default), yet none of these calls has a sweep that reads first-layer activations."""
    name, kw = ROUTES[route]
    D = _dataset(store, name)
    r, saved = _run(D, save=1, **kw)
    assert saved == 0, f'{route}: last.bwds_save = {saved}'
    _assert_oracle(D, r, f'{name} {route}')
