"""Input gradients (d loss / d buses, lines, generators) of the reference, pinned by tests/golden/igrad/*.npz
(tools/make_igrad_goldens.py: the reference's own main.GNS under autograd).  CPU only: the fp64 oracle reproduces them, the index
columns are exactly zero, and the C-ABI declares the entry point."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT, assert_close, cfg_of, load_golden
from oracle import gns_oracle as orc

IGRAD_DIR = os.path.join(GOLDEN, 'igrad')
IGRAD = sorted(os.path.splitext(n)[0] for n in os.listdir(IGRAD_DIR) if n.endswith('.npz'))


def load_igrad(name):
    z = np.load(os.path.join(IGRAD_DIR, name + '.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


LOSSES = ('mean', 'mixed')


def oracle_input_grads(g, w, loss):
    """fp64 autograd of the oracle with respect to the inputs, one grid per call like the reference."""
    c = cfg_of(g)
    flat = torch.as_tensor(g['params'], dtype=torch.float64)
    params = orc.unflatten_params(flat, c['latent_dim'], c['hidden_dim'], c['K'], c['multiple_phi'])
    bu = torch.as_tensor(g['buses'], dtype=torch.float64).requires_grad_(True)
    li = torch.as_tensor(g['lines'], dtype=torch.float64).requires_grad_(True)
    ge = torch.as_tensor(g['generators'], dtype=torch.float64).requires_grad_(True)
    bt = bu.shape[0]
    acc = 0.
    for b in range(bt):
        v, th, tot, last = orc.gns_forward(params, bu[b], li[b], ge[b], latent_dim=c['latent_dim'], K=c['K'], gamma=c['gamma'],
                                           multiple_phi=c['multiple_phi'])
        if loss == 'mean':
            acc = acc + tot / bt
        else:
            acc = acc + (float(w['w_total'][b]) * tot + float(w['w_last'][b]) * last
                         + (torch.as_tensor(w['w_v'][b], dtype=torch.float64) * v).sum()
                         + (torch.as_tensor(w['w_theta'][b], dtype=torch.float64) * th).sum())
    acc.backward()
    return bu.grad.numpy(), li.grad.numpy(), ge.grad.numpy()


def test_the_issue_cases_have_goldens():
    for name in ('c14_b2_K4_d10_single', 'c14_b3_K4_d20_multi_lowload', 'c14_b2_K15_d10_multi', 'c14_b2_K4_d7_h5_single',
                 'c118_b2_K4_d20_multi', 'c300_b1_K10_d20_multi', 'odd_ring_isolated_dupgen_b3_K4_d20_multi',
                 'odd_hub_indegree_40_b2_K3_d10_multi', 'odd_chain_one_way_b2_K2_d20_single'):
        assert name in IGRAD


@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('name', IGRAD)
def test_oracle_input_grads_match_reference(name, loss):
    g = load_golden(name)
    ig = load_igrad(name)
    ob, ol, og = oracle_input_grads(g, ig, loss)
    for what, a, b in (('buses', ob, ig[f'{loss}_grad_buses']), ('lines', ol, ig[f'{loss}_grad_lines']),
                       ('generators', og, ig[f'{loss}_grad_generators'])):
        assert_close(a, b, 2e-5, abs_floor=1e-6, what=f'{name} {loss} {what}')


@pytest.mark.parametrize('name', IGRAD)
def test_index_columns_get_exactly_zero(name):
    ig = load_igrad(name)
    for loss in LOSSES:
        assert np.all(ig[f'{loss}_grad_buses'][..., 0:2] == 0)          # bus_i, type
        assert np.all(ig[f'{loss}_grad_lines'][..., 0:2] == 0)          # f_bus, t_bus
        assert np.all(ig[f'{loss}_grad_generators'][..., 0] == 0)       # bus_i
        # the physics reaches the generators' set-points and the loads
        assert np.any(ig[f'{loss}_grad_generators'][..., 3:5] != 0) and np.any(ig[f'{loss}_grad_buses'][..., 2] != 0)


def test_c_abi_declares_input_gradients():
    hdr = open(os.path.join(ROOT, 'include', 'gns_hip.h')).read()
    assert re.search(r'\bint gns_backward_inputs\s*\(', hdr)
    decl = hdr[hdr.index('int gns_backward_inputs'):]
    decl = decl[:decl.index(';')]
    for arg in ('grad_params', 'grad_buses', 'grad_lines', 'grad_generators'):
        assert arg in decl
    assert 'save_state = 2' in hdr
