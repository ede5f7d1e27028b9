"""The DC N-2 contingency screen on the MI355X (``powerflow.dc_n2_contingency_screen``, include/gns_powerflow.h "DC N-2 contingency
screening"): every selected (grid, pair) row against the direct float64 reference (``dc_n2_reference.pair_flows``: both lines removed
and the grid solved again, no distribution factors), against the product's other route (``dc_power_flow(mixed_topologies=True)`` on
grids with both rows deleted), the summaries against torch on the returned flows, bitwise reproducibility of rows, islanding rows,
per-grid failure and the LDS refusal.

The bar is the project's DC bar per (grid, pair): max|out - ref| <= 1e-9 max(1, max|ref|).  No pair is left out of a comparison it
was selected for, and ``islanding`` is True exactly where the reference returns None.

Generated families (``pf_topologies.families()``): a family is held to the bar only if ``dc_n2_reference.dense_rank2`` and
``pair_flows`` agree to 1e-10 on it on the CPU (two 'reference' grids with ``_perturbed`` lines, the pairs ``_family_pairs``
selects: every pair up to 2000, else a seeded sample of 300 plus every pair that islands without a bridge).  Measured worst scaled
error, smallest |det| and islanding / selected pairs of the families included here:
  complete20 9.1e-16, 4.1e-1 (0/300);  lattice8x8 2.5e-14, 5.6e-3 (4/304);  lattice16x16 5.6e-14, 1.6e-2 (4/304);
  random24_stacked_gens 1.4e-14, 9.5e-3 (185/703);  random40_parallel_selfloop 1.0e-14, 3.8e-3 (422/1953);
  random97_parallel_selfloop 2.1e-14, 3.2e-3 (119/336);  ring30_slack_no_gen 2.3e-14, 9.8e-5 (211/465);
  star65_pv and path65 (2016/2016: nothing to compare but the islanding rows).
No family failed the probe.  These grids have x > 0 and taps near 1; the 'wide' regime (x of both signs, so determinants of both
signs, taps 0.5 .. 1.5, shifts within +-30 degrees) lives in ``test_dc_wide_gpu``."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import dc_n2_reference as n2ref
import pf_topologies as pt
from test_dc_contingency_gpu import _case, _torch_summaries
from test_dcpf_gpu import _perturbed, _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-9
FAMILIES = ('complete20', 'lattice8x8', 'lattice16x16', 'random24_stacked_gens', 'random40_parallel_selfloop',
            'random97_parallel_selfloop', 'ring30_slack_no_gen', 'star65_pv', 'path65')
ROWS = ('line_flow', 'worst_loading', 'worst_line')


def _screen(s, **kw):
    return powerflow.dc_n2_contingency_screen(s[0], s[1], s[2], slack_bus=s[3], **kw)


def _positions(pairs, E):
    """Rows of the default list (every j < k in lexicographic order) that hold ``pairs`` [P,2] with j < k."""
    j, k = pairs[:, 0], pairs[:, 1]
    return j * (2 * E - j - 1) // 2 + (k - j - 1)


def _family_pairs(name, tp):
    """The pairs of a family that go to the reference: every pair up to 2000, else a seeded sample of 300 of the default list and
    every pair that islands without a bridge; in the default list's order.  Sampled: lattice16x16 (114 960 pairs) and
    random97_parallel_selfloop (10 878), and also complete20 (17 955) and lattice8x8 (6 216): the reference solves a grid per
    (grid, pair) at about 0.5 ms each, so every pair of those two would take 18 s and 6 s of CPU per test, against the few seconds a
    test of this suite may take.  Their whole default lists are still launched and held to the sampled rows' bits, the host's
    islanding count and finiteness (``test_generated_families_against_the_reference``)."""
    E = tp.f.size
    pairs = powerflow._pair_list(None, E)
    if pairs.shape[0] <= 2000 or name in ('star65_pv', 'path65'):
        return pairs
    isl = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    pick = set(np.random.default_rng(len(name)).choice(pairs.shape[0], 300, replace=False).tolist())
    pick |= set(np.flatnonzero(isl & ~bridges[pairs[:, 0]] & ~bridges[pairs[:, 1]])[:40].tolist())
    return pairs[sorted(pick)]


def _check_values(res, s, name):
    """Every (grid, pair) row of res.line_flow against the direct reference; islanding exactly where the reference islands."""
    buses, lines, gens = (t.cpu() for t in s[:3])
    assert bool(res.converged.all()), name
    flow, wl, wi, isl = res.line_flow.cpu(), res.worst_loading.cpu(), res.worst_line.cpu(), res.islanding.cpu()
    worst, n_isl = 0.0, 0
    for p, (j, k) in enumerate(res.pairs.tolist()):
        for i in range(buses.shape[0]):
            want = n2ref.pair_flows(buses[i], lines[i], gens[i], s[3], j, k)
            got = flow[i, p]
            assert (want is None) == bool(isl[p]), (name, i, j, k)
            if want is None:
                n_isl += i == 0
                assert bool(got.isnan().all()) and bool(wl[i, p].isnan()) and int(wi[i, p]) == -1, (name, i, j, k)
                continue
            err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (name, i, j, k, err, scale)
            assert float(got[j]) == 0.0 and float(got[k]) == 0.0, (name, i, j, k)
    print(f'{name}: {res.pairs.shape[0]} pairs ({n_isl} islanding), worst scaled error {worst:.3e}')
    return n_isl


def _check_summaries(s, pairs, res, name):
    """worst_loading / worst_line against torch on the returned flows, with and without a rating; flows=False gives the same bits."""
    Bt, E = s[1].shape[0], s[1].shape[1]
    wl, wi = _torch_summaries(res.line_flow)
    assert _same(res.worst_loading, wl) and torch.equal(res.worst_line, wi), name
    slim = _screen(s, pairs=pairs)
    assert slim.line_flow is None and _same(slim.worst_loading, res.worst_loading) and torch.equal(slim.worst_line, res.worst_line)
    assert torch.equal(slim.islanding, res.islanding) and torch.equal(slim.converged, res.converged)
    g = torch.Generator().manual_seed(E)
    for shape in ((E,), (Bt, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=g, dtype=torch.float64)).to(DEV)
        for flows in (True, False):
            rated = _screen(s, pairs=pairs, rating=rating, flows=flows)
            wl, wi = _torch_summaries(res.line_flow, rating)
            assert _same(rated.worst_loading, wl) and torch.equal(rated.worst_line, wi), (name, shape, flows)
            if flows:
                assert _same(rated.line_flow, res.line_flow)
    r32 = _screen(s, pairs=pairs, rating=torch.ones(E, dtype=torch.float32))                     # converted to float64
    assert _same(r32.worst_loading, res.worst_loading)


@pytest.mark.parametrize('case,batch', [(14, 3), (30, 2)])
def test_every_pair_of_a_small_case_against_the_reference(case, batch):
    s = _case(case, batch, seed=case)
    E = s[1].shape[1]
    P = E * (E - 1) // 2
    res = _screen(s, flows=True)
    assert res.pairs.tolist() == powerflow._pair_list(None, E).tolist() and res.pairs.dtype == torch.int64
    assert res.pairs.shape == (P, 2) and P == {14: 190, 30: 820}[case]
    assert res.line_flow.shape == (batch, P, E) and res.worst_loading.shape == res.worst_line.shape == (batch, P)
    assert res.line_flow.dtype == res.worst_loading.dtype == torch.float64 and res.worst_line.dtype == torch.int32
    assert res.islanding.dtype == res.converged.dtype == torch.bool and res.islanding.shape == (P,) and res.converged.shape == (batch,)
    for t in (res.line_flow, res.worst_loading, res.worst_line, res.islanding, res.converged, res.pairs, res.base.theta):
        assert t.device == s[0].device
    n_isl = _check_values(res, s, f'case{case}')
    assert n_isl == {14: 27, 30: 208}[case] == int(res.islanding.sum())
    _check_summaries(s, None, res, f'case{case}')


def test_case118_sampled_against_the_reference_and_the_full_list():
    """Every 37th pair against the reference; then all 17 205 pairs (538 chunks of 32 and a ragged tail per grid, E = 186 lines in
    the lane loop) give the same bits at those positions."""
    s = _case(118, 2, seed=118)
    E = s[1].shape[1]
    every = powerflow._pair_list(None, E)
    assert every.shape[0] == 17205
    pos = np.arange(0, 17205, 37)
    assert pos.size == 465
    res = _screen(s, pairs=every[pos], flows=True)
    _check_values(res, s, 'case118, every 37th pair')
    full = _screen(s)
    assert full.line_flow is None and full.worst_loading.shape == (2, 17205)
    at = torch.from_numpy(pos).to(DEV)
    assert _same(full.worst_loading[:, at], res.worst_loading) and torch.equal(full.worst_line[:, at], res.worst_line)
    assert torch.equal(full.islanding[at], res.islanding)
    assert int(full.islanding.sum()) == 3554
    assert bool(full.worst_loading[:, full.islanding].isnan().all()) and bool((full.worst_line[:, full.islanding] == -1).all())
    assert bool(torch.isfinite(full.worst_loading[:, ~full.islanding]).all()) and bool((full.worst_line[:, ~full.islanding] >= 0).all())


def test_case300_with_bridges_and_pairs_that_island_without_one():
    s = _case(300, 1, seed=300)
    f, t, _ = synth.case_topology(300)
    E = f.size
    every = powerflow._pair_list(None, E)
    isl = powerflow._pair_islanding(300, f - 1, t - 1, every)
    assert every.shape[0] == 84255 and int(isl.sum()) == 31418           # the full count needs no launch
    bridges = powerflow._bridges(300, f - 1, t - 1)
    neither = np.flatnonzero(isl & ~bridges[every[:, 0]] & ~bridges[every[:, 1]])
    with_bridge = np.flatnonzero(bridges[every[:, 0]] | bridges[every[:, 1]])
    last = np.flatnonzero(every[:, 1] == 410)                            # the last line, whatever the pair does
    assert neither.size == 138 and last.size == 410
    pos = sorted(set(range(0, 84255, 401)) | set(neither[::5].tolist()) | set(with_bridge[::1499].tolist()) | set(last[::10].tolist()))
    assert 280 <= len(pos) <= 320
    res = _screen(s, pairs=every[pos], flows=True)
    n_isl = _check_values(res, s, 'case300')
    assert 40 <= n_isl < len(pos) - 100
    assert bool((res.pairs[:, 1] == 410).any())
    _check_summaries(s, every[pos], res, 'case300')


@pytest.mark.parametrize('name', FAMILIES)
def test_generated_families_against_the_reference(name):
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, len(name)), gens, tp.slack)
    E = tp.f.size
    pairs = _family_pairs(name, tp)
    res = _screen(s, pairs=pairs, flows=True)
    n_isl = _check_values(res, s, name)
    if name in ('star65_pv', 'path65'):
        assert n_isl == pairs.shape[0] == 2016
    # the whole default list gives the same bits at the selected rows, and the host's islanding count
    full = _screen(s)
    at = torch.from_numpy(_positions(pairs, E)).to(DEV)
    assert torch.equal(full.pairs[at].cpu(), torch.from_numpy(pairs))
    assert _same(full.worst_loading[:, at], res.worst_loading) and torch.equal(full.worst_line[:, at], res.worst_line)
    want = {'ring30_slack_no_gen': 211, 'lattice8x8': 4, 'star65_pv': 2016, 'path65': 2016, 'complete20': 0}
    if name in want:
        assert int(full.islanding.sum()) == want[name]
    assert bool(full.worst_loading[:, full.islanding].isnan().all())
    assert bool(torch.isfinite(full.worst_loading[:, ~full.islanding]).all())


def _without(lines, j, k):
    """[Bt,E,7] -> [Bt,E-2,7]: the batch with line rows j and k deleted."""
    keep = [e for e in range(lines.shape[1]) if e != j and e != k]
    return lines[:, keep], keep


def test_agrees_with_the_mixed_route_pair_by_pair():
    """40 non-islanding pairs of case14: row p of the screen against grid p of ``dc_power_flow(mixed_topologies=True)`` on the grids
    with both rows deleted."""
    slack = synth._solvable_slack(14)
    buses, lines, gens = synth.synth_grids(14, 40, seed=2, device=DEV)
    E = lines.shape[1]
    every = powerflow._pair_list(None, E)
    f, t, _ = synth.case_topology(14)
    ok = every[~powerflow._pair_islanding(14, f - 1, t - 1, every)]
    pairs = ok[:: ok.shape[0] // 40][:40]
    assert pairs.shape == (40, 2)
    cut = torch.cat([_without(lines[p:p + 1], j, k)[0] for p, (j, k) in enumerate(pairs.tolist())])
    mixed = powerflow.dc_power_flow(buses, cut, gens, slack_bus=slack, mixed_topologies=True)
    res = powerflow.dc_n2_contingency_screen(buses, lines, gens, slack_bus=slack, pairs=pairs, flows=True)
    assert bool(res.converged.all()) and bool(mixed.converged.all()) and not bool(res.islanding.any())
    worst = 0.0
    for p, (j, k) in enumerate(pairs.tolist()):
        keep = _without(lines[:1], j, k)[1]
        want = torch.zeros(E, dtype=torch.float64, device=DEV)
        want[keep] = mixed.line_flow[p]
        got = res.line_flow[p, p]
        err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        worst = max(worst, err / scale)
        assert err <= TOL * scale, (j, k, err, scale)
    print(f'case14 against the mixed route: worst scaled error {worst:.3e}')


def test_a_self_loop_and_a_parallel_pair():
    tp = pt.families()['random40_parallel_selfloop']
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, 7), gens, tp.slack)
    E = tp.f.size
    loop = int(np.flatnonzero(tp.f == tp.t)[0])
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    # a pair whose second line is the self-loop: the N-1 screen's row of the first line
    firsts = [e for e in range(E) if e != loop and not bridges[e]][:12]
    n1 = powerflow.dc_contingency_screen(*s[:3], slack_bus=tp.slack, outages=firsts)
    for order in ([[e, loop] for e in firsts], [[loop, e] for e in firsts]):
        res = _screen(s, pairs=order, flows=True)
        assert not bool(res.islanding.any())
        want = n1.line_flow.clone()
        want[:, :, loop] = 0.0                              # the N-2 row puts 0 at the self-loop too; nothing else changes
        err = (res.line_flow - want).abs().amax(dim=-1)
        scale = want.abs().amax(dim=-1).clamp(min=1.0)
        assert bool((err <= TOL * scale).all()), float((err / scale).max())
        assert bool((res.line_flow[:, :, loop] == 0.0).all())
    # two parallel lines: together they island when nothing else joins their buses, else against the reference
    ends = {}
    for e, (a, b) in enumerate(zip(tp.f.tolist(), tp.t.tolist())):
        if a != b:
            ends.setdefault((min(a, b), max(a, b)), []).append(e)
    parallel = [v[:2] for v in ends.values() if len(v) > 1]
    assert parallel
    res = _screen(s, pairs=parallel, flows=True)
    _check_values(res, s, 'random40_parallel_selfloop, parallel pairs')


def test_rows_are_bitwise_reproducible_and_base_is_dc_power_flow():
    s = _case(118, 5, seed=9)
    buses, lines, gens, slack = s
    E = lines.shape[1]
    every = powerflow._pair_list(None, E)
    pairs = every[np.arange(3, 17205, 29)]                                    # 594 pairs: chunks of 8 and a tail
    a = _screen(s, pairs=pairs, flows=True)
    base = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    for k in base._fields:
        assert _same(getattr(a.base, k), getattr(base, k)), k
    assert torch.equal(a.converged, base.converged) and bool(a.converged.all())
    b = _screen(s, pairs=pairs, flows=True)                                   # from run to run
    for k in ROWS:
        assert _same(getattr(a, k), getattr(b, k)), k
    for sl in (slice(0, 1), slice(2, 4)):                                     # a batch of one grid, another batch
        p = _screen((buses[sl], lines[sl], gens[sl], slack), pairs=pairs, flows=True)
        for k in ROWS:
            assert _same(getattr(p, k), getattr(a, k)[sl]), k
    live = int(np.flatnonzero(~a.islanding.cpu().numpy())[17])
    one = _screen((buses[3:4], lines[3:4], gens[3:4], slack), pairs=pairs[live:live + 1], flows=True)   # one grid, a row alone
    for k in ROWS:
        assert _same(getattr(one, k)[0, 0], getattr(a, k)[3, live]), k
    sub = [100, 3, 64, 63, 585, 0, 64]                                        # a sub-list, out of order, with a duplicate
    p = _screen(s, pairs=pairs[sub], flows=True)
    assert p.pairs.tolist() == pairs[sub].tolist()
    for k in ROWS:
        assert _same(getattr(p, k), getattr(a, k)[:, sub]), k
    assert _same(p.line_flow[:, 2], p.line_flow[:, 6])
    p = _screen(s, pairs=torch.from_numpy(pairs[::-1].copy()).to(DEV), flows=True)      # the reversed list, as a device tensor
    for k in ROWS:
        assert _same(getattr(p, k), getattr(a, k).flip(1)), k
    assert torch.equal(p.islanding, a.islanding.flip(0))
    p = _screen(s, pairs=pairs[:, ::-1].copy(), flows=True)                   # every pair swapped
    assert p.pairs.tolist() == pairs[:, ::-1].tolist()
    for k in ROWS:
        assert _same(getattr(p, k), getattr(a, k)), k
    full = _screen(s)                                                         # in the default list (chunks of 32)
    at = torch.from_numpy(_positions(pairs, E)).to(DEV)
    assert _same(full.worst_loading[:, at], a.worst_loading) and torch.equal(full.worst_line[:, at], a.worst_line)
    # a 2-D single grid; CPU tensors in, CPU tensors out
    single = powerflow.dc_n2_contingency_screen(buses[3], lines[3], gens[3], slack_bus=slack, pairs=pairs[[live, 5]], flows=True)
    assert single.line_flow.shape == (2, E) and single.worst_loading.shape == (2,) and single.converged.shape == ()
    assert single.base.theta.shape == (118,) and _same(single.line_flow, a.line_flow[3, [live, 5]])
    cpu = powerflow.dc_n2_contingency_screen(buses[:2].cpu(), lines[:2].cpu(), gens[:2].cpu(), slack_bus=slack, pairs=pairs[:3])
    for t_ in (cpu.worst_loading, cpu.worst_line, cpu.islanding, cpu.converged, cpu.pairs, cpu.base.theta):
        assert t_.device.type == 'cpu'
    assert cpu.line_flow is None and _same(cpu.worst_loading, a.worst_loading[:2, :3].cpu())
    # not differentiable: the call runs as under no_grad
    req = lines.clone().requires_grad_(True)
    r = powerflow.dc_n2_contingency_screen(buses, req, gens, slack_bus=slack, pairs=[[0, 1]], flows=True)
    assert not r.line_flow.requires_grad and not r.worst_loading.requires_grad and not r.base.theta.requires_grad


def test_a_bad_grid_fails_alone_and_mixed_batches_are_refused():
    buses, lines, gens, slack = _case(14, 8, seed=4)
    good = _screen((buses, lines, gens, slack), flows=True)
    bad = lines.clone()
    bad[5, 7, 3] = 0.0                                                        # x = 0: a numeric failure of that grid's base solve
    res = _screen((buses, bad, gens, slack), flows=True)
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert res.converged.tolist() == [True] * 5 + [False] + [True] * 2
    assert torch.equal(res.converged, res.base.converged)
    assert bool(res.line_flow[5].isnan().all()) and bool(res.worst_loading[5].isnan().all()) and bool((res.worst_line[5] == -1).all())
    for k in ROWS:
        assert _same(getattr(res, k)[keep], getattr(good, k)[keep]), k
    slim = _screen((buses, bad, gens, slack))
    assert _same(slim.worst_loading, res.worst_loading) and torch.equal(slim.worst_line, res.worst_line)
    mixed = lines.clone()
    mixed[2, 0, 1] = 6.0
    with pytest.raises(ValueError, match='dc_n2_contingency_screen solves one topology'):
        _screen((buses, mixed, gens, slack))
    with pytest.raises(ValueError, match='pairs must lie in'):
        _screen((buses, lines, gens, slack), pairs=[[0, lines.shape[1]]])


def test_lds_refusal_names_the_bytes_and_the_formula():
    tp = pt.path(6000)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    want = 8 * (23994 + 6000 + 3 * 5999 + 5999 * 2)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.dc_n2_contingency_screen(buses, lines, gens, slack_bus=tp.slack, pairs=[[0, 1]])
    assert str(want) in str(e.value) and 'nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)' in str(e.value)
