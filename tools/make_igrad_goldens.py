"""Generate tests/golden/igrad/<name>.npz: gradients of the REFERENCE'S OWN ``main.GNS`` with respect to its inputs (buses, lines,
generators), for the inputs and parameters of existing goldens.  Runs on the CPU where the reference is importable (it imports it
exactly as ``oracle/make_goldens.py`` does); the .npz files are data and are all the tests read.

Two losses per case:
  * ``mean``  : mean over the batch of total_loss (what the existing goldens use);
  * ``mixed`` : sum_b w_total[b] total_b + w_last[b] last_b + <w_v[b], v_b> + <w_theta[b], theta_b>, with the weights stored in the file,
                so that all four upstream gradients (total_loss, last_loss, the clamped v of main.py:201, theta) contribute.
Each grid is one call of ``main.GNS.forward`` on 2-D tensors, as the reference's training loop makes it (main.py:279-288).

usage: python tools/make_igrad_goldens.py [name ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

CASES = ['c14_b2_K4_d10_single', 'c14_b3_K4_d20_multi_lowload', 'c14_b2_K15_d10_multi', 'c14_b2_K4_d7_h5_single',
         'c118_b2_K4_d20_multi', 'c300_b1_K10_d20_multi', 'odd_ring_isolated_dupgen_b3_K4_d20_multi',
         'odd_hub_indegree_40_b2_K3_d10_multi', 'odd_chain_one_way_b2_K2_d20_single']


def mixed_weights(z, seed=7):
    g = torch.Generator().manual_seed(seed)
    bt, n = z['buses'].shape[0], z['buses'].shape[1]
    return dict(w_total=torch.rand(bt, generator=g, dtype=torch.float64).float(),
                w_last=torch.rand(bt, generator=g, dtype=torch.float64).float(),
                w_v=(torch.rand((bt, n), generator=g, dtype=torch.float64) - 0.5).float(),
                w_theta=(torch.rand((bt, n), generator=g, dtype=torch.float64) - 0.5).float())


def reference_input_grads(ref, z, loss):
    torch.manual_seed(0)
    model = ref.GNS(latent_dim=int(z['latent_dim']), hidden_dim=int(z['hidden_dim']), K=int(z['K']), gamma=float(z['gamma']),
                    multiple_phi=bool(int(z['multiple_phi'])))
    flat = torch.from_numpy(z['params'])
    off = 0
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
    assert off == flat.numel()
    for p in model.parameters():
        p.requires_grad_(False)
    B, L, G = ref.get_BLG()
    bu = torch.from_numpy(z['buses']).clone().requires_grad_(True)
    li = torch.from_numpy(z['lines']).clone().requires_grad_(True)
    ge = torch.from_numpy(z['generators']).clone().requires_grad_(True)
    bt = bu.shape[0]
    w = mixed_weights(z)
    terms = []
    for b in range(bt):
        v, th, tot, last = model(buses=bu[b], lines=li[b], generators=ge[b], B=B, L=L, G=G)
        if loss == 'mean':
            terms.append(tot / bt)
        else:
            terms.append(w['w_total'][b] * tot + w['w_last'][b] * last + (w['w_v'][b] * v).sum() + (w['w_theta'][b] * th).sum())
    torch.stack(terms).sum().backward()
    return [t.grad.detach().numpy().copy() for t in (bu, li, ge)], w


def main(names):
    from oracle.make_goldens import _import_reference
    import warnings
    warnings.filterwarnings('ignore')
    ref = _import_reference()
    for name in names:
        z = np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))
        out = dict(source=name)
        for loss in ('mean', 'mixed'):
            (gb, gl, gg), w = reference_input_grads(ref, z, loss)
            out[f'{loss}_grad_buses'], out[f'{loss}_grad_lines'], out[f'{loss}_grad_generators'] = gb, gl, gg
        out.update({k: v.numpy() for k, v in w.items()})
        # (a directory of their own: every .npz directly under tests/golden is read as a forward / backward golden)
        path = os.path.join(ROOT, 'tests', 'golden', 'igrad', name + '.npz')
        np.savez_compressed(path, **out)
        print(f'igrad/{name}: wrote {os.path.getsize(path) / 1024:.0f} KiB  max|g_gen| {np.abs(out["mean_grad_generators"]).max():.3g}')


if __name__ == '__main__':
    main(sys.argv[1:] or CASES)
