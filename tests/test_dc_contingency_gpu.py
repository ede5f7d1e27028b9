"""The DC contingency screen on the MI355X (``powerflow.dc_contingency_screen``, include/gns_powerflow.h "DC contingency
screening"): every (grid, outage) row against the direct float64 reference (``dc_contingency_reference``: the line removed and the
grid solved again, no distribution factors), against the product's other route (``dc_power_flow(mixed_topologies=True)`` on the
expanded batch), the summaries against torch on the returned flows, bitwise reproducibility of rows, islanding rows, per-grid
failure and the LDS refusal.

The bar is the project's DC bar per (grid, outage): max|out - ref| <= 1e-9 max(1, max|ref|), and no outage is left out.

Generated families (``pf_topologies.families()``): a family is held to the bar only if a dense float64 LODF and the direct reference
agree to 1e-10 on it on the CPU (``dc_contingency_reference.dense_lodf`` against ``outage_flows``, two 'reference' grids, every
outage).  Measured worst scaled error (and islanding lines / lines) of the families included here: complete20 9.1e-16 (0/190),
lattice8x8 2.1e-14 (0/112), lattice16x16 9.7e-14 (0/480), random24_stacked_gens 6.5e-15 (5/38), random40_parallel_selfloop 3.0e-15
(7/63), random97_parallel_selfloop 1.9e-14 (21/148), ring30_slack_no_gen 3.9e-15 (0/31), and the all-bridge star65_pv, path65 and
pair (64/64, 64/64, 1/1: nothing to compare but the islanding rows).  No family failed the probe; the remaining ones (other paths
and stars, complete33, hub150) repeat these shapes.  These grids have x > 0 and taps near 1; the 'wide' regime (x of both signs, taps
0.5 .. 1.5, shifts within +-30 degrees) lives in ``test_dc_wide_gpu``."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import dc_contingency_reference as cref
import pf_topologies as pt
from test_dcpf_gpu import _perturbed, _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-9
FAMILIES = ('complete20', 'lattice8x8', 'lattice16x16', 'random24_stacked_gens', 'random40_parallel_selfloop',
            'random97_parallel_selfloop', 'ring30_slack_no_gen', 'star65_pv', 'path65', 'pair')


def _screen(s, **kw):
    return powerflow.dc_contingency_screen(s[0], s[1], s[2], slack_bus=s[3], **kw)


def _case(case, batch, seed):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, batch, seed=seed, device=DEV)
    return buses, _perturbed(lines, case), gens, slack


def _torch_summaries(flow, rating=None):
    """(worst loading, its line: the lowest of equals) from a returned line_flow [..., K, E]; NaN rows give (NaN, -1)."""
    load = flow.abs() if rating is None else flow.abs() / (rating if rating.dim() == 1 else rating.unsqueeze(-2))
    top = load.amax(dim=-1)
    E = flow.shape[-1]
    idx = torch.where(load == top.unsqueeze(-1), torch.arange(E, device=flow.device), E).amin(dim=-1)
    nan = flow.isnan().any(dim=-1)
    return torch.where(nan, float('nan'), top), torch.where(nan, -1, idx).to(torch.int32)


def _check_values(res, s, outages, name):
    """Every (grid, outage) row of res.line_flow against the direct reference; islanding exactly where the reference islands."""
    buses, lines, gens = (t.cpu() for t in s[:3])
    assert bool(res.converged.all()), name
    worst, n_isl = 0.0, 0
    for j, k in enumerate(outages):
        for i in range(buses.shape[0]):
            want = cref.outage_flows(buses[i], lines[i], gens[i], s[3], k)
            got = res.line_flow[i, j].cpu()
            assert (want is None) == bool(res.islanding[j]), (name, i, k)
            if want is None:
                n_isl += i == 0
                assert bool(got.isnan().all()) and bool(res.worst_loading[i, j].isnan()) and int(res.worst_line[i, j]) == -1, (name, i, k)
                continue
            err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (name, i, k, err, scale)
            assert float(got[k]) == 0.0, (name, i, k)
    print(f'{name}: {len(outages)} outages ({n_isl} islanding), worst scaled error {worst:.3e}')
    return n_isl


def _check_summaries(s, outages, res, name):
    """worst_loading / worst_line against torch on the returned flows, with and without a rating; flows=False gives the same bits."""
    Bt, E = s[1].shape[0], s[1].shape[1]
    wl, wi = _torch_summaries(res.line_flow)
    assert _same(res.worst_loading, wl) and torch.equal(res.worst_line, wi), name
    slim = _screen(s, outages=outages, flows=False)
    assert slim.line_flow is None and _same(slim.worst_loading, res.worst_loading) and torch.equal(slim.worst_line, res.worst_line)
    assert torch.equal(slim.islanding, res.islanding) and torch.equal(slim.converged, res.converged)
    g = torch.Generator().manual_seed(E)
    for shape in ((E,), (Bt, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=g, dtype=torch.float64)).to(DEV)
        for flows in (True, False):
            rated = _screen(s, outages=outages, rating=rating, flows=flows)
            wl, wi = _torch_summaries(res.line_flow, rating)
            assert _same(rated.worst_loading, wl) and torch.equal(rated.worst_line, wi), (name, shape, flows)
            if flows:
                assert _same(rated.line_flow, res.line_flow)
    r32 = _screen(s, outages=outages, rating=torch.ones(E, dtype=torch.float32), flows=False)      # converted to float64
    assert _same(r32.worst_loading, res.worst_loading)


@pytest.mark.parametrize('case', [14, 30, 118])
def test_every_outage_of_a_case_against_the_reference(case):
    s = _case(case, 3, seed=case)
    E = s[1].shape[1]
    res = _screen(s)
    assert res.outages.tolist() == list(range(E)) and res.outages.dtype == torch.int64
    assert res.line_flow.shape == (3, E, E) and res.worst_loading.shape == res.worst_line.shape == (3, E)
    assert res.line_flow.dtype == res.worst_loading.dtype == torch.float64 and res.worst_line.dtype == torch.int32
    assert res.islanding.dtype == res.converged.dtype == torch.bool and res.islanding.shape == (E,) and res.converged.shape == (3,)
    assert res.line_flow.device == s[0].device
    n_isl = _check_values(res, s, list(range(E)), f'case{case}')
    assert n_isl == {14: 1, 30: 5, 118: 20}[case] == int(res.islanding.sum())
    _check_summaries(s, None, res, f'case{case}')


def test_case300_with_islanding_lines_against_the_reference():
    s = _case(300, 2, seed=300)
    f, t, _ = synth.case_topology(300)
    bridges = np.flatnonzero(powerflow._bridges(300, f - 1, t - 1))
    assert bridges.size == 85
    outages = sorted(set(range(0, 411, 7)) | set(bridges[:24].tolist()) | {410})
    assert len(outages) >= 64
    res = _screen(s, outages=outages)
    n_isl = _check_values(res, s, outages, 'case300')
    assert 24 <= n_isl < len(outages) - 24
    _check_summaries(s, outages, res, 'case300')
    everything = _screen(s, flows=False)                        # all 411: seven chunks of 32 outages and a tail per grid
    pos = torch.tensor(outages, device=DEV)
    assert _same(everything.worst_loading[:, pos], res.worst_loading) and torch.equal(everything.worst_line[:, pos], res.worst_line)
    assert int(everything.islanding.sum()) == 85


@pytest.mark.parametrize('name', FAMILIES)
def test_generated_families_against_the_reference(name):
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, len(name)), gens, tp.slack)
    res = _screen(s)
    _check_values(res, s, list(range(tp.f.size)), name)
    _check_summaries(s, None, res, name)


@pytest.mark.parametrize('case', [14, 118])
def test_agrees_with_the_mixed_route_pair_by_pair(case):
    """Grid i of ``contingency_grids(case, E, range(E))`` is grid i of ``synth_grids`` without line i: row [i, i] of the screen."""
    E = synth.CASE_SHAPES[case][1]
    slack = synth._solvable_slack(case)
    buses, lines, gens = synth.synth_grids(case, E, seed=2, device=DEV)
    cb, cl, cg, outage = synth.contingency_grids(case, E, range(E), seed=2, device=DEV)
    assert outage.tolist() == list(range(E)) and torch.equal(cb, buses)
    mixed = powerflow.dc_power_flow(cb, cl, cg, slack_bus=slack, mixed_topologies=True)
    res = powerflow.dc_contingency_screen(buses, lines, gens, slack_bus=slack)
    assert bool(res.converged.all())
    assert torch.equal(res.islanding, ~mixed.converged)                      # islanding outages agree in being unsolved
    assert 1 <= int(res.islanding.sum()) < E
    worst = 0.0
    for i in range(E):
        got = res.line_flow[i, i]
        if bool(res.islanding[i]):
            assert bool(got.isnan().all()) and bool(mixed.line_flow[i].isnan().all())
            continue
        want = torch.cat([mixed.line_flow[i, :i], torch.zeros(1, dtype=torch.float64, device=DEV), mixed.line_flow[i, i:]])
        err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        worst = max(worst, err / scale)
        assert err <= TOL * scale, (case, i, err, scale)
    print(f'case{case} against the mixed route: worst scaled error {worst:.3e}')


def test_base_is_dc_power_flow_and_rows_are_bitwise_reproducible():
    s = _case(118, 70, seed=9)
    buses, lines, gens, slack = s
    E = lines.shape[1]
    a = _screen(s)
    base = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    for k in base._fields:
        assert _same(getattr(a.base, k), getattr(base, k)), k
    assert torch.equal(a.converged, base.converged) and bool(a.converged.all())
    rows = ('line_flow', 'worst_loading', 'worst_line')
    b = _screen(s)                                                            # from run to run
    for k in rows:
        assert _same(getattr(a, k), getattr(b, k)), k
    for bt in (1, 3, 65):                                                     # alone and in another batch
        p = _screen((buses[:bt], lines[:bt], gens[:bt], slack))
        for k in rows:
            assert _same(getattr(p, k), getattr(a, k)[:bt]), (bt, k)
    one = _screen((buses[5:6], lines[5:6], gens[5:6], slack), outages=[17])   # one grid, one outage
    for k in rows:
        assert _same(getattr(one, k)[0, 0], getattr(a, k)[5, 17]), k
    sub = [100, 3, 64, 63, 185, 0, 64]                                        # a sublist, out of order, with a duplicate
    p = _screen(s, outages=sub)
    assert p.outages.tolist() == sub
    for k in rows:
        assert _same(getattr(p, k), getattr(a, k)[:, sub]), k
    assert _same(p.line_flow[:, 2], p.line_flow[:, 6]) and _same(p.worst_loading[:, 2], p.worst_loading[:, 6])
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1))
    p = _screen(s, outages=perm.to(DEV))                                      # a permuted list, as a device tensor
    for k in rows:
        assert _same(getattr(p, k), getattr(a, k)[:, perm.to(DEV)]), k
    assert torch.equal(p.islanding, a.islanding[perm.to(DEV)])
    # an outage of a line at the slack
    f = lines[0, :, 0].long().cpu()
    t = lines[0, :, 1].long().cpu()
    at_slack = torch.nonzero((f == slack) | (t == slack)).flatten().tolist()
    assert at_slack
    p = _screen((buses[:2], lines[:2], gens[:2], slack), outages=at_slack)
    _check_values(p, (buses[:2], lines[:2], gens[:2], slack), at_slack, 'case118 lines at the slack')
    # a 2-D single grid; CPU tensors in, CPU tensors out
    single = powerflow.dc_contingency_screen(buses[5], lines[5], gens[5], slack_bus=slack, outages=[17, 4])
    assert single.line_flow.shape == (2, E) and single.worst_loading.shape == (2,) and single.converged.shape == ()
    assert single.base.theta.shape == (118,) and _same(single.line_flow, a.line_flow[5, [17, 4]])
    assert _same(single.worst_loading, a.worst_loading[5, [17, 4]]) and torch.equal(single.worst_line, a.worst_line[5, [17, 4]])
    cpu = powerflow.dc_contingency_screen(buses[:4].cpu(), lines[:4].cpu(), gens[:4].cpu(), slack_bus=slack, outages=[1, 2])
    for t_ in (cpu.line_flow, cpu.worst_loading, cpu.worst_line, cpu.islanding, cpu.converged, cpu.outages, cpu.base.theta):
        assert t_.device.type == 'cpu'
    assert _same(cpu.line_flow, a.line_flow[:4, [1, 2]].cpu())
    # not differentiable: the call runs as under no_grad
    req = lines.clone().requires_grad_(True)
    r = powerflow.dc_contingency_screen(buses, req, gens, slack_bus=slack, outages=[0])
    assert not r.line_flow.requires_grad and not r.worst_loading.requires_grad and not r.base.theta.requires_grad


def test_islanding_rows_and_only_those_are_nan_in_every_grid():
    s = _case(30, 9, seed=4)
    res = _screen(s)
    isl = res.islanding
    assert int(isl.sum()) == 5
    assert bool(res.line_flow[:, isl].isnan().all()) and bool(res.worst_loading[:, isl].isnan().all())
    assert bool((res.worst_line[:, isl] == -1).all())
    assert bool(torch.isfinite(res.line_flow[:, ~isl]).all()) and bool(torch.isfinite(res.worst_loading[:, ~isl]).all())
    assert bool((res.worst_line[:, ~isl] >= 0).all()) and bool(res.converged.all())
    f, t, _ = synth.case_topology(30)
    want = [cref.islands(30, np.delete(f, k), np.delete(t, k), s[3]) for k in range(f.size)]
    assert isl.tolist() == want


def test_a_bad_grid_fails_alone():
    buses, lines, gens, slack = _case(14, 8, seed=4)
    good = _screen((buses, lines, gens, slack))
    lines = lines.clone()
    lines[5, 7, 3] = 0.0
    res = _screen((buses, lines, gens, slack))
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert res.converged.tolist() == [True] * 5 + [False] + [True] * 2
    assert torch.equal(res.converged, res.base.converged)
    assert bool(res.line_flow[5].isnan().all()) and bool(res.worst_loading[5].isnan().all()) and bool((res.worst_line[5] == -1).all())
    for k in ('line_flow', 'worst_loading', 'worst_line'):
        assert _same(getattr(res, k)[keep], getattr(good, k)[keep]), k
    slim = _screen((buses, lines, gens, slack), flows=False)
    assert _same(slim.worst_loading, res.worst_loading) and torch.equal(slim.worst_line, res.worst_line)


def test_the_analysis_is_reused_and_mixed_batches_are_refused():
    buses, lines, gens, slack = _case(30, 4, seed=11)
    powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    n_topo, n_nr = len(powerflow._FD_TOPO_CACHE), len(powerflow._TOPO_CACHE)
    res = _screen((buses, lines, gens, slack), outages=[0, 1])
    assert bool(res.converged.all())
    assert len(powerflow._FD_TOPO_CACHE) == n_topo and len(powerflow._TOPO_CACHE) == n_nr
    mixed = lines.clone()
    mixed[2, 0, 1] = 6.0
    with pytest.raises(ValueError, match='dc_contingency_screen solves one topology'):
        _screen((buses, mixed, gens, slack))
    with pytest.raises(ValueError, match='outages must lie in'):
        _screen((buses, lines, gens, slack), outages=[lines.shape[1]])


def test_lds_refusal_names_the_bytes_and_the_formula():
    tp = pt.path(6000)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    want = 8 * (23994 + 6000 + 3 * 5999 + 5999 * 2)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.dc_contingency_screen(buses, lines, gens, slack_bus=tp.slack, outages=[0])
    assert str(want) in str(e.value) and 'nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)' in str(e.value)
