"""The split backward's sweeps request rows ahead of their use (the next in-line's rows, the next bus's top-of-bus rows:
gns_backward_split.hip, GNS_BWDS_LINE_AHEAD, GNS_BWDS_BUS_AHEAD), and one kernel of step K-1 - the L_m kernel, or with
GNS_BWDS_LASTK_FOLD the theta kernel - writes the zeros of the L_m / phi_m blocks that no gradient reaches.  None of this may change
a result, whichever way the switches are set.

Shapes: the smallest at which a look-ahead index or the moved zeroing can go wrong.
  case14   eight chunks hold one or two buses each ("next bus" is nearly always the clamped index); with the default layout of a
           small batch (32 chunks for 14 buses) most chunks are empty (n0 == n1).  Bus 1 has no in-line, bus 5 has three.
  case30   several buses per chunk.
  batches  70 (two groups, the second ragged) and 64;  K = 1 (no L_m sweep ever runs), 2, 3.
Reference: the float64 oracle (helpers.oracle64) on a sample of grids under a weighted loss that is zero outside the sample, with
the tolerances of tests/test_gpu_parity.py: 1e-5 of the tensor's scale (+1e-6) for outputs, 5e-5 (+1e-7) for the gradient."""
import numpy as np
import pytest
import torch

from helpers import assert_close, loss_weights, options, oracle64, weighted_loss

pytestmark = pytest.mark.gpu

REL, REL_GRAD = 1e-5, 5e-5
D_LAT, D_HID = 20, 10
# name -> (case, batch, K, bwds_chunks (0: the layout's own choice), sampled grids)
SHAPES = {
    'c14x70_K3': (14, 70, 3, 8, [0, 1, 63, 64, 69]),
    'c14x70_K2': (14, 70, 2, 8, [0, 63, 64, 69]),
    'c14x70_K1': (14, 70, 1, 8, [0, 63, 64, 69]),
    'c14x64_K3_empty_chunks': (14, 64, 3, 0, [0, 31, 63]),
    'c30x70_K3': (30, 70, 3, 8, [0, 1, 63, 64, 69]),
    'c30x64_K2': (30, 64, 2, 8, [0, 31, 63]),
    'c30x70_K1': (30, 70, 1, 8, [0, 63, 64, 69]),
}
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
        case, bt, K, chunks, sample = SHAPES[name]
        D = Data()
        torch.manual_seed(1000 + case + bt + K)
        D.model = amd.GNS(D_LAT, D_HID, K, 0.9, True).cuda()
        D.model.topology_check = 'first'
        D.x = amd.synth.synth_grids(case, bt, seed=case + K, device='cuda')
        D.cfg = dict(latent_dim=D_LAT, hidden_dim=D_HID, K=K, gamma=0.9, multiple_phi=True)
        D.K, D.chunks, D.sample = K, chunks, sample
        D.w = loss_weights(bt, D.x[0].shape[1], sample, seed=7 * bt + K)
        D.o32, D.o64 = oracle64(D.model.flat_parameters(), *D.x, D.cfg, sample, D.w)
        store[name] = D
    return store[name]


def _run(D, mode):
    """One training call through the lane-per-grid forward and the split backward in sweep mode ``mode``."""
    import opf_graph_neural_solver_amd as amd
    with options(train_mapping=1, bwd_variant=4, dw_mfma=1, bwds_mode=mode, bwds_chunks=D.chunks):
        D.model.zero_grad()
        out = D.model(*D.x)
        weighted_loss(out, D.w).backward()
        torch.cuda.synchronize()
        path = {n: amd.get_option('last.' + n) for n in ('bwd_kernel', 'bwds_mode', 'bwds_chunks')}
    assert path['bwd_kernel'] == 4 and path['bwds_mode'] == mode, path
    if D.chunks:
        assert path['bwds_chunks'] == D.chunks, path
    else:
        assert path['bwds_chunks'] > D.x[0].shape[1], path        # more chunks than buses: some chunks are empty (n0 == n1)
    r = {k: o.detach() for k, o in zip(OUTS, out)}
    assert all(p.grad is not None for p in D.model.parameters())
    r['grad'] = torch.cat([p.grad.reshape(-1) for p in D.model.parameters()])
    return r


def _last_step_m_blocks(D):
    """Slices of the flat gradient that hold L_m.{K-1} and phi_m.{K-1}: nothing reads m_K, so no gradient reaches them."""
    out, off = [], 0
    for n, p in D.model.named_parameters():
        if n.startswith((f'L_m.{D.K - 1}.', f'phi_m.{D.K - 1}.')):
            out.append((n, off, off + p.numel()))
        off += p.numel()
    assert len(out) == 6 + 6, [n for n, _, _ in out]          # three linear layers with bias each
    return out


def _assert_m_blocks_zero(D, grad, what):
    g = grad.cpu().numpy()
    for n, a, b in _last_step_m_blocks(D):
        blk = g[a:b]
        assert np.all(np.isfinite(blk)) and not np.any(blk), f'{what}: {n} is not exactly zero ({blk[np.nonzero(blk)][:4]})'


def test_case14_has_the_line_lists_this_file_is_about():
    import opf_graph_neural_solver_amd as amd
    f_bus, t_bus, _ = amd.synth.case_topology(14)
    indeg = np.bincount(np.asarray(t_bus, dtype=np.int64), minlength=15)[1:]
    assert indeg.min() == 0 and indeg.max() >= 3, indeg            # a bus without in-line, a bus with at least three


@pytest.mark.parametrize('mode', [1, 0, 2])
@pytest.mark.parametrize('name', list(SHAPES))
def test_split_backward_matches_float64_oracle(store, name, mode):
    D = _dataset(store, name)
    r = _run(D, mode)
    idx = torch.as_tensor(D.sample, device='cuda')
    for k in OUTS:
        assert_close(r[k][idx].cpu(), D.o64[k], REL, what=f'{name} mode {mode}: {k}')
    assert_close(r['grad'].cpu(), D.o64['grad_params'], REL_GRAD, abs_floor=1e-7, what=f'{name} mode {mode}: grad_params')
    _assert_m_blocks_zero(D, r['grad'], f'{name} mode {mode}')


@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('name', ['c14x70_K3', 'c30x70_K1'])
def test_two_identical_calls_give_the_same_bits(store, name, mode):
    D = _dataset(store, name)
    a, b = _run(D, mode), _run(D, mode)
    for k in OUTS + ('grad',):
        assert torch.equal(a[k], b[k]), f'{name} mode {mode}: {k} differs between two identical calls'


@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('name', ['c14x70_K1', 'c30x70_K1', 'c14x70_K3'])
def test_last_step_m_blocks_are_written_as_zeros_in_poisoned_workspaces(store, name, mode, monkeypatch):
    """K = 1: no L_m sweep runs, and exactly one kernel of the step has to write the L_m.0 / phi_m.0 blocks of every slab as zeros.
    Workspaces filled with 0xFF bytes: a block nobody wrote reaches the reduction as NaN."""
    import opf_graph_neural_solver_amd as amd
    D = _dataset(store, name)
    clean = _run(D, mode)
    monkeypatch.setattr(amd.gns, 'POISON_WORKSPACES', True)
    dirty = _run(D, mode)
    assert torch.isfinite(dirty['grad']).all(), f'{name} mode {mode}: non-finite gradient from a poisoned workspace'
    _assert_m_blocks_zero(D, dirty['grad'], f'{name} mode {mode} (poisoned)')
    for k in OUTS + ('grad',):
        assert torch.equal(clean[k], dirty[k]), f'{name} mode {mode}: {k} depends on what the workspace held'
