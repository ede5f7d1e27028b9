"""CPU checks of the Newton-Raphson power-flow solver's host side: the topology analysis (roles, dimension, fill of the LU
ordering), its refusals, the manufactured-solution generator and the test-side reference NR."""
import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import powerflow, synth
from helpers import load_golden
import nr_reference as ref

# solvable_grids rounds the manufactured powers to float32 (the solver's input type): that moves the exact solution of the
# float32 problem away from the chosen point by up to ~2.6e-7 at case300 (~4e-8 at case14)
TRUTH_TOL = 5e-7
# nnz(L+U) of the Jacobian pattern of synth.case_topology(c), slack = first generator bus, under minimum degree (SuperLU
# MMD_AT_PLUS_A, symmetric mode, no pivoting); natural order gives 348 / 1 505 / 14 145 / 57 732 / 115 554
MD_NNZ_LU = {14: 162, 30: 479, 118: 2115, 200: 5376, 300: 8400}


@pytest.mark.parametrize('case', sorted(synth.CASE_SHAPES))
def test_topology_analysis_roles_dimension_and_fill(case):
    f, t, g = synth.case_topology(case)
    n = synth.CASE_SHAPES[case][0]
    slack = int(g[0])
    info = powerflow.analyse_topology(n, f, t, g, slack).info
    n_pv = len(set(g.tolist()) - {slack})
    n_pq = n - 1 - n_pv
    assert (info['slack'], info['n_pv'], info['n_pq']) == (slack - 1, n_pv, n_pq)
    assert info['dim'] == (n - 1) + n_pq
    assert info['nnz_lu'] <= 1.5 * MD_NNZ_LU[case], info
    assert info['lds_bytes'] <= 160 * 1024
    assert info['n_steps'] < info['n_ops']


def test_topology_refusals():
    f, t, g = synth.case_topology(14)
    with pytest.raises(ValueError, match='integers'):
        powerflow.analyse_topology(14, f + 0.5, t, g, 1)
    with pytest.raises(ValueError, match='1..14'):
        powerflow.analyse_topology(14, np.r_[f[:-1], 15], t, g, 1)
    with pytest.raises(ValueError, match='1..14'):
        powerflow.analyse_topology(14, f, t, np.r_[g[:-1], 0], 1)
    for bad in (0, 15, 2.5):
        with pytest.raises(ValueError, match='slack_bus'):
            powerflow.analyse_topology(14, f, t, g, bad)


@pytest.mark.parametrize('name', ['odd_hub_indegree_40_b2_K3_d10_multi', 'odd_random_40_one_gen_b2_K4_d20_multi',
                                  'odd_ring_isolated_dupgen_b3_K4_d20_multi'])
def test_islands_are_refused_by_name(name):
    gd = load_golden(name)
    n = gd['buses'].shape[1]
    ln, gen = gd['lines'][0], gd['generators'][0]
    with pytest.raises(ValueError, match=r'buses \[.*\] have no path of lines to slack_bus'):
        powerflow.analyse_topology(n, ln[:, 0], ln[:, 1], gen[:, 0], int(gen[0, 0]))


def test_missing_slack_without_type_3_is_refused_on_the_host():
    buses, lines, gens = synth.synth_grids(14, 2)
    with pytest.raises(ValueError, match='slack_bus'):
        powerflow._topology(buses, lines, gens, None)
    buses[:, 3, 1] = 3
    buses[:, 5, 1] = 3
    with pytest.raises(ValueError, match='slack_bus'):
        powerflow._topology(buses, lines, gens, None)
    buses[:, 5, 1] = 1
    assert powerflow._topology(buses, lines, gens, None).info['slack'] == 3


def test_mixed_topology_is_refused_on_the_host():
    buses, lines, gens = synth.synth_grids(14, 3)
    lines[1, 0, 1] = 5
    with pytest.raises(ValueError, match='differ across the batch'):
        powerflow._topology(buses, lines, gens, 1)


@pytest.mark.parametrize('case', [14, 30, 118])
def test_manufactured_solution_is_a_solution(case):
    buses, lines, gens, slack, v, theta = synth.solvable_grids(case, 4, seed=2)
    b64, g64 = synth.manufacture_solution(buses.double(), lines.double(), gens.double(), slack, v, theta)
    for i in range(4):
        sl, pv, pq = ref.roles(b64[i], g64[i], slack)
        V = v[i].numpy() * np.exp(1j * theta[i].numpy())
        S = V * np.conj(ref.ybus(b64[i], lines[i].double()) @ V)
        spec = ref.specified(b64[i], g64[i])
        pvpq = np.r_[pv, pq]
        assert np.max(np.abs(S[pvpq].real - spec[pvpq].real)) <= 1e-12
        assert np.max(np.abs(S[pq].imag - spec[pq].imag)) <= 1e-12
        first = {}
        for j, bb in enumerate(g64[i][:, 0].long().tolist()):
            first.setdefault(bb, j)
        for bb, j in first.items():
            assert float(g64[i][j, 4]) == float(v[i, bb - 1])
    assert torch.all(theta[:, slack - 1] == 0)


@pytest.mark.parametrize('case', [14, 30, 118, 300])
def test_reference_nr_recovers_manufactured_solutions(case):
    buses, lines, gens, slack, v, theta = synth.solvable_grids(case, 3, seed=1)
    for i in range(3):
        vm, va, conv, it, mis = ref.newton_raphson(buses[i], lines[i], gens[i], slack)
        assert conv and 1 <= it <= 10 and mis < 1e-8
        assert np.max(np.abs(vm - v[i].numpy())) <= TRUTH_TOL
        assert np.max(np.abs(va - theta[i].numpy())) <= TRUTH_TOL


def test_library_exports_the_powerflow_abi():
    lib = amd.load_library()
    for sym in amd._lib.PF_EXPORTS:
        assert hasattr(lib, sym)
