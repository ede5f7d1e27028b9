"""CPU checks of the host side of Newton-Raphson on batches that mix topologies (``newton_raphson(..., mixed_topologies=True)``):
the planning step (topology index, launch order, islands, the blob set), the host refusals of ``gns_pf_workspace_bytes_set`` and
the solvable contingency sets of ``synth.solvable_contingency_grids``."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig
import nr_reference as ref

TRUTH_TOL = 5e-7                      # test_powerflow_host.TRUTH_TOL
PF_MAGIC = 0x47504631                 # csrc/gns_pf_common.h
# outages (0-based lines) that leave a bus without a path of lines to the slack of solvable_grids
ISLANDING = {14: {13}, 30: {12, 22, 26, 29, 30},
             118: {1, 12, 13, 15, 18, 51, 56, 57, 79, 104, 116, 125, 132, 134, 144, 158, 168, 171, 174, 180}}


def _islanding_by_search(case, slack):
    f, t, _ = synth.case_topology(case)
    n, e, _ = synth.CASE_SHAPES[case]
    out = set()
    for j in range(e):
        keep = np.arange(e) != j
        if powerflow._islanded(n, (f[keep] - 1).astype(np.int64), (t[keep] - 1).astype(np.int64), slack - 1).size:
            out.add(j)
    return out


@pytest.mark.parametrize('case', [14, 30, 118])
def test_islanding_outages_are_the_expected_ones(case):
    slack = synth.solvable_grids(case, 1)[3]
    assert _islanding_by_search(case, slack) == ISLANDING[case]


@pytest.mark.parametrize('case', [14, 30])
def test_plan_topology_index_order_islands_and_offsets(case):
    e = synth.CASE_SHAPES[case][1]
    buses, lines, gens, slack, _, _, outage = synth.solvable_contingency_grids(case, 3 * e + 5, range(e), seed=4, shuffle=True)
    plan = powerflow._plan_mixed(buses, lines, gens, slack)
    topo, order, grid_off = plan.topology.numpy(), plan.order.numpy(), plan.grid_off.numpy()
    out = outage.numpy()
    bt = out.size
    # one index per outage, the same index exactly for the same outage
    for i in range(bt):
        assert np.array_equal(topo == topo[i], out == out[i])
    assert plan.islanded.size == np.unique(out).size
    # the stable argsort of the topology index
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(bt))
    assert np.array_equal(order, np.argsort(topo, kind='stable'))
    # -1 exactly for the islanding outages
    isl = np.isin(out, sorted(ISLANDING[case]))
    assert np.array_equal(grid_off == -1, isl)
    assert np.array_equal(plan.islanded[topo], isl)
    # members: distinct, 16-word aligned, inside the set, each a blob of this shape; every solved grid points at one
    ts, members = plan.topo_set, plan.member_off
    assert members.size == len(set(out.tolist()) - ISLANDING[case]) == np.unique(members).size
    assert ts.host.size == ts.words and ts.blob.numel() == ts.words
    for m in members.tolist():
        assert m % 16 == 0
        h = ts.host[m:]
        assert h[0] == PF_MAGIC and tuple(h[2:5]) == (buses.shape[1], lines.shape[1], gens.shape[1])
        assert m + h[1] <= ts.words
    assert set(grid_off[~isl].tolist()) == set(members.tolist())
    assert torch.equal(ts.blob, torch.from_numpy(ts.host))


def test_plan_blob_matches_a_plain_analysis_and_is_cached():
    buses, lines, gens, slack, _, _, outage = synth.solvable_contingency_grids(14, 40, range(20), seed=1)
    plan = powerflow._plan_mixed(buses, lines, gens, slack)
    ts = plan.topo_set
    for i in (0, 7, 19):
        one = powerflow._topology(buses[i:i + 1], lines[i:i + 1], gens[i:i + 1], slack)
        off = int(plan.grid_off[i])
        assert np.array_equal(ts.host[off:off + one.host.size], one.host)
    calls = []
    real = powerflow.analyse_topology
    try:
        powerflow.analyse_topology = lambda *a, **k: calls.append(a) or real(*a, **k)
        words = ts.words
        again = powerflow._plan_mixed(buses, lines, gens, slack)
    finally:
        powerflow.analyse_topology = real
    assert calls == [] and again.topo_set is ts and ts.words == words
    assert torch.equal(again.grid_off, plan.grid_off)


def test_plan_takes_the_slack_from_grid_0_and_keeps_refusals():
    buses, lines, gens, slack, _, _, _ = synth.solvable_contingency_grids(14, 20, range(20), seed=2)
    with pytest.raises(ValueError, match='slack_bus'):
        powerflow._plan_mixed(buses, lines, gens, None)
    typed = buses.clone()
    typed[0, slack - 1, 1] = 3.0
    assert powerflow._plan_mixed(typed, lines, gens, None).slack_bus == slack
    with pytest.raises(ValueError, match='slack_bus'):
        powerflow._plan_mixed(buses, lines, gens, 15)
    bad = lines.clone()
    bad[3, 2, 1] = 15.0
    with pytest.raises(ValueError, match='1..14'):
        powerflow._plan_mixed(buses, bad, gens, slack)
    bad = lines.clone()
    bad[3, 2, 1] = 2.5
    with pytest.raises(ValueError, match='integers'):
        powerflow._plan_mixed(buses, bad, gens, slack)


def test_plain_analysis_still_refuses_an_islanding_outage_by_name():
    buses, lines, gens, slack, _, _, outage = synth.solvable_contingency_grids(14, 20, range(20), seed=0)
    i = int(np.flatnonzero(outage.numpy() == 13)[0])
    with pytest.raises(ValueError, match=r'buses \[8\] have no path of lines to slack_bus'):
        powerflow._topology(buses[i:i + 1], lines[i:i + 1], gens[i:i + 1], slack)


def _set_of(case, outages):
    buses, lines, gens, slack, _, _, _ = synth.solvable_contingency_grids(case, len(outages), outages, seed=3)
    plan = powerflow._plan_mixed(buses, lines, gens, slack)
    return plan, PfConfig(buses.shape[1], lines.shape[1], gens.shape[1], 10, 1e-8)


def test_workspace_bytes_set_size_and_refusals():
    lib = amd.load_library()
    plan, cfg = _set_of(30, [0, 1, 2, 5, 40])
    ts, members = plan.topo_set, plan.member_off
    host = ts.host

    def ws(mem, bt=16, cfg_=cfg, words=ts.words):
        m = np.ascontiguousarray(mem, dtype=np.int32)
        n = ctypes.c_size_t(0)
        rc = lib.gns_pf_workspace_bytes_set(ctypes.byref(cfg_), host.ctypes.data, words, m.ctypes.data, m.size, bt, ctypes.byref(n))
        return rc, n.value

    nnzy = max(int(host[m + 11]) for m in members.tolist())           # PH_NNZY
    assert ws(members) == (0, 16 * nnzy * 16)
    rc, n = ws(members, bt=7)
    assert rc == 0 and n == (7 * nnzy * 16 + 255) // 256 * 256
    assert ws(members[:1]) == (0, 16 * int(host[members[0] + 11]) * 16)
    assert ws(np.r_[members, members[1] + 8])[0] == 1                    # misaligned
    assert ws(np.r_[members, members[1] + 16])[0] == 1                   # aligned, but not at a blob
    assert ws(np.r_[members, ts.words])[0] == 1                          # out of bounds
    assert ws(np.r_[members, -16])[0] == 1
    assert ws(members, words=int(members.max()) + 16)[0] == 1            # the last blob runs past the set
    for bad in (PfConfig(cfg.n_bus + 1, cfg.n_line, cfg.n_gen, 10, 1e-8), PfConfig(cfg.n_bus, cfg.n_line - 1, cfg.n_gen, 10, 1e-8),
                PfConfig(cfg.n_bus, cfg.n_line, cfg.n_gen + 1, 10, 1e-8)):
        assert ws(members, cfg_=bad)[0] == 1
    assert ws(members[:0])[0] == 1                                       # no member
    assert ws(members, bt=0)[0] == 1


def test_solvable_contingency_grids():
    outages = list(range(20))
    buses, lines, gens, slack, v, theta, outage = synth.solvable_contingency_grids(14, 45, outages, seed=5, shuffle=True)
    b0, l0, g0, o0 = synth.contingency_grids(14, 45, outages, seed=5, shuffle=True)
    assert torch.equal(lines, l0) and torch.equal(outage, o0)
    assert slack == synth.solvable_grids(14, 1)[3]
    _, _, _, _, v_s, th_s = synth.solvable_grids(14, 45, seed=5)
    assert torch.equal(theta, th_s)                                      # the draws of solvable_grids
    assert torch.all(theta[:, slack - 1] == 0)
    n_checked = 0
    for i in range(45):
        if int(outage[i]) in ISLANDING[14]:
            continue
        assert ref.mismatch(buses[i], lines[i], gens[i], slack, v[i], theta[i]) <= TRUTH_TOL
        n_checked += 1
    assert n_checked >= 40
    for case, outs in ((30, [0, 3, 12, 40]), (118, [0, 1, 100])):
        buses, lines, gens, slack, v, theta, outage = synth.solvable_contingency_grids(case, 8, outs, seed=1)
        for i in range(8):
            if int(outage[i]) not in ISLANDING[case]:
                assert ref.mismatch(buses[i], lines[i], gens[i], slack, v[i], theta[i]) <= TRUTH_TOL
