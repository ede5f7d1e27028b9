"""The DC generator contingency screen on the MI355X (``powerflow.dc_generator_contingency_screen``, include/gns_powerflow.h "DC
generator contingency screening"): every selected (grid, row) against the direct float64 reference
(``dc_generator_contingency_reference.direct``: the generators redispatched, the line removed and the grid solved again, no
distribution factors), against the product's other route (``dc_power_flow`` on modified copies), the two bit-for-bit pins of the
definition against ``dc_contingency_screen`` and the base flows, the summaries against torch on the returned flows, bitwise
reproducibility of rows, islanding rows, per-grid failure and the LDS refusal.

The bar is the project's DC bar per (grid, row): max|out - ref| <= 1e-9 max(1, max|ref|).  No row is left out of a comparison it was
selected for, and ``islanding`` is True exactly where the reference returns None.

Generated families (``pf_topologies.families()``): a family is held to the bar only if ``dc_generator_contingency_reference.by_factors``
and ``direct`` agree to 1e-10 on it on the CPU (two 'reference' grids with ``_perturbed`` lines, every non-islanding default row, with
no pickup, 'pmax' and random weights holding a zero).  Measured worst scaled difference, smallest |1 - b_k H_k[k]| and islanding /
default rows of the families included here:
  random24_stacked_gens 7.9e-15, 7.0e-2 (40/312);  random40_parallel_selfloop 3.5e-15, 5.4e-2 (42/384);
  ring30_slack_no_gen 1.2e-14, 6.4e-3 (0/96);  lattice8x8 2.3e-14, 6.7e-2 (0/1469);
  path64 and path65 0 (63/64, 64/65: the one generator sits on the slack), path66_pv1 4.0e-14 (130/132) and hub150_70lines_70gens
  6.2e-14 (10430/10500): every line is a bridge, only the generator-alone rows are compared.
No family failed the probe.  These grids have x > 0 and taps near 1; the 'wide' regime (x of both signs, taps 0.5 .. 1.5, shifts
within +-30 degrees) lives in ``test_dc_wide_gpu``."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import dc_generator_contingency_reference as gref
import pf_topologies as pt
from test_dc_contingency_gpu import _case, _torch_summaries
from test_dcpf_gpu import _perturbed, _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-9
ROWS = ('line_flow', 'worst_loading', 'worst_line')
PICKUPS = (None, 'pmax', 'random')


def _screen(s, **kw):
    return powerflow.dc_generator_contingency_screen(s[0], s[1], s[2], slack_bus=s[3], **kw)


def _pickup(kind, Bt, Gn, seed=0):
    """None, 'pmax', or random weights [Bt,Gn] in [0.1, 1.1) with one column exactly zero."""
    if kind != 'random':
        return kind
    w = 0.1 + torch.rand(Bt, Gn, generator=torch.Generator().manual_seed(Gn + seed), dtype=torch.float64)
    w[:, Gn // 2] = 0.0
    return w


def _positions(rows, E):
    """Rows of the default list (for each generator (g,-1), (g,0), ..., (g,E-1)) that hold ``rows`` [P,2]."""
    return rows[:, 0] * (E + 1) + rows[:, 1] + 1


def _check_values(res, s, pickup, name):
    """Every (grid, row) of res.line_flow against the direct reference; islanding exactly where the reference islands."""
    buses, lines, gens = (t.cpu() for t in s[:3])
    assert bool(res.converged.all()), name
    flow, wl, wi, isl = res.line_flow.cpu(), res.worst_loading.cpu(), res.worst_line.cpu(), res.islanding.cpu()
    worst, n_isl = 0.0, 0
    for i in range(buses.shape[0]):
        w = gref.weights(pickup, gens[i], i)
        for p, (g, k) in enumerate(res.contingencies.tolist()):
            want = gref.direct(buses[i], lines[i], gens[i], s[3], g, k, w)
            got = flow[i, p]
            assert (want is None) == bool(isl[p]), (name, i, g, k)
            if want is None:
                n_isl += i == 0
                assert bool(got.isnan().all()) and bool(wl[i, p].isnan()) and int(wi[i, p]) == -1, (name, i, g, k)
                continue
            err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (name, i, g, k, err, scale)
            assert k < 0 or float(got[k]) == 0.0, (name, i, g, k)
    print(f'{name}: {res.contingencies.shape[0]} rows ({n_isl} islanding), worst scaled error {worst:.3e}')
    return n_isl


def _check_summaries(s, rows, pickup, res, name):
    """worst_loading / worst_line against torch on the returned flows, with and without a rating; flows=False gives the same bits."""
    Bt, E = s[1].shape[0], s[1].shape[1]
    wl, wi = _torch_summaries(res.line_flow)
    assert _same(res.worst_loading, wl) and torch.equal(res.worst_line, wi), name
    slim = _screen(s, contingencies=rows, pickup=pickup)
    assert slim.line_flow is None and _same(slim.worst_loading, res.worst_loading) and torch.equal(slim.worst_line, res.worst_line)
    assert torch.equal(slim.islanding, res.islanding) and torch.equal(slim.converged, res.converged)
    g = torch.Generator().manual_seed(E)
    for shape in ((E,), (Bt, E)):
        rating = (0.5 + 2.0 * torch.rand(shape, generator=g, dtype=torch.float64)).to(DEV)
        for flows in (True, False):
            rated = _screen(s, contingencies=rows, pickup=pickup, rating=rating, flows=flows)
            wl, wi = _torch_summaries(res.line_flow, rating)
            assert _same(rated.worst_loading, wl) and torch.equal(rated.worst_line, wi), (name, shape, flows)
            if flows:
                assert _same(rated.line_flow, res.line_flow)
    r32 = _screen(s, contingencies=rows, pickup=pickup, rating=torch.ones(E, dtype=torch.float32))     # converted to float64
    assert _same(r32.worst_loading, res.worst_loading)


@pytest.mark.parametrize('kind', PICKUPS)
@pytest.mark.parametrize('case,batch', [(14, 3), (30, 2)])
def test_every_default_row_of_a_small_case_against_the_reference(case, batch, kind):
    s = _case(case, batch, seed=case)
    E, Gn = s[1].shape[1], s[2].shape[1]
    P = Gn * (E + 1)
    pickup = _pickup(kind, batch, Gn)
    res = _screen(s, pickup=pickup, flows=True)
    assert res.contingencies.tolist() == powerflow._generator_contingency_list(None, Gn, E).tolist()
    assert res.contingencies.dtype == torch.int64 and res.contingencies.shape == (P, 2) and P == {14: 105, 30: 252}[case]
    assert res.line_flow.shape == (batch, P, E) and res.worst_loading.shape == res.worst_line.shape == (batch, P)
    assert res.line_flow.dtype == res.worst_loading.dtype == torch.float64 and res.worst_line.dtype == torch.int32
    assert res.islanding.dtype == res.converged.dtype == torch.bool and res.islanding.shape == (P,) and res.converged.shape == (batch,)
    for t in (res.line_flow, res.worst_loading, res.worst_line, res.islanding, res.converged, res.contingencies, res.base.theta):
        assert t.device == s[0].device
    n_isl = _check_values(res, s, pickup, f'case{case}, pickup {kind}')
    assert n_isl == {14: 5, 30: 30}[case] == int(res.islanding.sum())
    _check_summaries(s, None, pickup, res, f'case{case}')
    if kind == 'random':                                     # the same weights shared by the grids, and as float32
        shared = _screen(s, pickup=pickup[1], flows=True)
        assert _same(shared.line_flow[1], res.line_flow[1]) and not _same(shared.line_flow[0], res.line_flow[0])
        w32 = pickup.float()
        assert _same(_screen(s, pickup=w32, flows=True).line_flow, _screen(s, pickup=w32.double().to(DEV), flows=True).line_flow)
    if kind == 'pmax':                                       # the generators' column 1, and every grid's own
        assert _same(_screen(s, pickup=s[2][:, :, 1].double(), flows=True).line_flow, res.line_flow)


def test_case118_sampled_against_the_reference_and_the_full_list():
    """Every 37th default row against the reference; then all 10 098 rows (315 chunks of 32 and a ragged tail of 18 per grid, E = 186
    lines in the lane loop, 240 candidates in chunks of W) give the same bits at those positions."""
    s = _case(118, 2, seed=118)
    E, Gn = s[1].shape[1], s[2].shape[1]
    every = powerflow._generator_contingency_list(None, Gn, E)
    assert every.shape[0] == 10098 and 10098 % 32 == 18
    pos = np.arange(0, 10098, 37)
    assert pos.size == 273
    res = _screen(s, contingencies=every[pos], pickup='pmax', flows=True)
    n_isl = _check_values(res, s, 'pmax', 'case118, every 37th row')
    assert 10 <= n_isl <= 60 and bool((res.contingencies[:, 1] == -1).any())
    full = _screen(s, pickup='pmax')
    assert full.line_flow is None and full.worst_loading.shape == (2, 10098)
    at = torch.from_numpy(pos).to(DEV)
    assert _same(full.worst_loading[:, at], res.worst_loading) and torch.equal(full.worst_line[:, at], res.worst_line)
    assert torch.equal(full.islanding[at], res.islanding)
    assert int(full.islanding.sum()) == 54 * 20
    assert bool(full.worst_loading[:, full.islanding].isnan().all()) and bool((full.worst_line[:, full.islanding] == -1).all())
    assert bool(torch.isfinite(full.worst_loading[:, ~full.islanding]).all()) and bool((full.worst_line[:, ~full.islanding] >= 0).all())


def _family_rows(name, tp):
    """The rows of a family that go to the reference, in the default list's order: every row up to 320, else every generator-alone
    row and every ``step``-th row (random40_parallel_selfloop: 198 of 384, every row of its self-loop among them; lattice8x8: 221 of
    1469; hub150_70lines_70gens: 210 of 10 500).  The whole default lists are still launched and held to the selected rows' bits and
    the host's islanding count."""
    E, Gn = tp.f.size, tp.g.size
    rows = powerflow._generator_contingency_list(None, Gn, E)
    if rows.shape[0] <= 320:
        return rows
    step = {'random40_parallel_selfloop': 2, 'lattice8x8': 7, 'hub150_70lines_70gens': 50}[name]
    pick = (rows[:, 1] == -1) | (np.arange(rows.shape[0]) % step == 0)
    loops = np.flatnonzero(tp.f == tp.t)
    if loops.size:
        pick |= rows[:, 1] == loops[0]
    return rows[pick]


@pytest.mark.parametrize('name,kind', [('random24_stacked_gens', None), ('random24_stacked_gens', 'random'), ('ring30_slack_no_gen', 'pmax'),
                                       ('random40_parallel_selfloop', 'random'), ('lattice8x8', 'random'), ('path64', None),
                                       ('path65', 'random'), ('path66_pv1', 'pmax'), ('hub150_70lines_70gens', 'random')])
def test_generated_families_against_the_reference(name, kind):
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, len(name)), gens, tp.slack)
    E, Gn = tp.f.size, tp.g.size
    pickup = _pickup(kind, 2, Gn)
    rows = _family_rows(name, tp)
    assert rows.shape[0] <= 330
    res = _screen(s, contingencies=rows, pickup=pickup, flows=True)
    n_isl = _check_values(res, s, pickup, f'{name}, pickup {kind}')
    alone = res.contingencies[:, 1] == -1
    assert int(alone.sum()) == Gn and not bool(res.islanding[alone].any())
    if name.startswith('path') or name.startswith('hub'):    # every line is a bridge: only the generator-alone rows are finite
        assert n_isl == rows.shape[0] - Gn and torch.equal(res.islanding, ~alone)
        assert bool(torch.isfinite(res.line_flow[:, alone]).all())
    if name == 'random40_parallel_selfloop':                 # the self-loop as the outaged line: the generator-alone row with 0 there
        loop = int(np.flatnonzero(tp.f == tp.t)[0])
        for g in range(Gn):
            both = res.line_flow[:, (res.contingencies[:, 0] == g) & (res.contingencies[:, 1] == loop)][:, 0]
            want = res.line_flow[:, (res.contingencies[:, 0] == g) & alone][:, 0].clone()
            want[:, loop] = 0.0
            assert _same(both, want), g
    # the whole default list gives the same bits at the selected rows, and the host's islanding count
    full = _screen(s, pickup=pickup)
    at = torch.from_numpy(_positions(rows, E)).to(DEV)
    assert torch.equal(full.contingencies[at].cpu(), torch.from_numpy(rows))
    assert _same(full.worst_loading[:, at], res.worst_loading) and torch.equal(full.worst_line[:, at], res.worst_line)
    want = {'random24_stacked_gens': 40, 'ring30_slack_no_gen': 0, 'lattice8x8': 0, 'path64': 63, 'path65': 64, 'path66_pv1': 130,
            'hub150_70lines_70gens': 70 * 149, 'random40_parallel_selfloop': 42}
    assert int(full.islanding.sum()) == want[name] and full.islanding.shape == (Gn * (E + 1),)
    assert bool(full.worst_loading[:, full.islanding].isnan().all())
    assert bool(torch.isfinite(full.worst_loading[:, ~full.islanding]).all())


def test_the_two_pins_of_the_definition_hold_bit_for_bit():
    """Pg_g exactly 0, or a generator on the slack bus with no pickup: row (g, -1) is the base flow and row (g, k) is row k of
    ``dc_contingency_screen``, bit for bit, islanding rows (NaN / -1 in both) included."""
    tp = pt.families()['random24_stacked_gens']              # generators 1 and 4 sit on the slack bus
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 3, 0, device=DEV)
    gens = gens.clone()
    gens[:, 2, 6] = 0.0
    gens[1, 6, 6] = 0.0
    s = (buses, _perturbed(lines, 5), gens, tp.slack)
    E, Gn = tp.f.size, tp.g.size
    assert tp.g.tolist() == [4, 1, 7, 4, 1, 4, 9, 4] and tp.slack == 1
    n1 = powerflow.dc_contingency_screen(*s[:3], slack_bus=tp.slack)
    assert bool(n1.islanding.any()) and not bool(n1.islanding.all())
    for kind, pinned in ((None, {0: (1, 2, 4), 1: (1, 2, 4, 6), 2: (1, 2, 4)}), ('random', {0: (2,), 1: (2, 6), 2: (2,)}),
                         ('pmax', {0: (2,), 1: (2, 6), 2: (2,)})):
        res = _screen(s, pickup=_pickup(kind, 3, Gn), flows=True)
        flow = res.line_flow.reshape(3, Gn, E + 1, E)
        wl, wi = res.worst_loading.reshape(3, Gn, E + 1), res.worst_line.reshape(3, Gn, E + 1)
        for i, gs in pinned.items():
            for g in range(Gn):
                same = _same(flow[i, g, 0], res.base.line_flow[i]) and _same(flow[i, g, 1:], n1.line_flow[i])
                assert same == (g in gs), (kind, i, g)
                if g in gs:
                    assert _same(wl[i, g, 1:], n1.worst_loading[i]) and torch.equal(wi[i, g, 1:], n1.worst_line[i])
    # the same on a case with taps and shifts, every generator's Pg zero in one grid
    buses, lines, gens, slack = _case(30, 2, seed=6)
    gens = gens.clone()
    gens[1, :, 6] = 0.0
    n1 = powerflow.dc_contingency_screen(buses, lines, gens, slack_bus=slack)
    res = _screen((buses, lines, gens, slack), pickup='pmax', flows=True)
    E, Gn = lines.shape[1], gens.shape[1]
    flow = res.line_flow.reshape(2, Gn, E + 1, E)
    for g in range(Gn):
        assert _same(flow[1, g, 0], res.base.line_flow[1]) and _same(flow[1, g, 1:], n1.line_flow[1]), g
    assert not _same(flow[0, 0, 0], res.base.line_flow[0])


def _exact(gens):
    """``gens`` with every Pg rounded to a multiple of 2^-8: a quarter of one added to another is then exact in float32."""
    gens = gens.clone()
    gens[..., 6] = torch.round(gens[..., 6] * 256) / 256
    return gens


@pytest.mark.parametrize('kind', [None, 'equal'])
def test_agrees_with_the_expanded_route_row_by_row(kind):
    """Row p of the screen on grid p against ``dc_power_flow`` on grid p's modified copy: Pg_g set to 0, the shares added to the other
    generators' Pg (equal weights on five generators: a quarter each, exact in float32 on Pg rounded to 2^-8), the line row deleted.
    The rows with a line run with ``mixed_topologies=True``; the rows without one in a second call, since they have another E."""
    slack = synth._solvable_slack(14)
    buses, lines, gens = synth.synth_grids(14, 25, seed=2, device=DEV)
    gens = _exact(gens)
    E, Gn = lines.shape[1], gens.shape[1]
    assert Gn == 5
    every = powerflow._generator_contingency_list(None, Gn, E)
    f, t, _ = synth.case_topology(14)
    ok = every[~powerflow._generator_islanding(powerflow._bridges(14, f - 1, t - 1), every)]
    with_line = ok[ok[:, 1] >= 0]
    rows = np.concatenate([with_line[:: with_line.shape[0] // 20][:20], ok[ok[:, 1] < 0]])
    assert rows.shape == (25, 2) and int((rows[:, 1] < 0).sum()) == 5
    pickup = None if kind is None else torch.ones(Gn, dtype=torch.float64)
    mod = gens.clone()
    for p, (g, _) in enumerate(rows.tolist()):
        pg = mod[p, g, 6].clone()
        mod[p, g, 6] = 0.0
        if pickup is not None:
            others = [h for h in range(Gn) if h != g]
            mod[p, others, 6] += pg * 0.25
            assert bool((mod[p, others, 6].double() == gens[p, others, 6].double() + pg.double() * 0.25).all())
    cut = torch.cat([lines[p:p + 1, [e for e in range(E) if e != k]] for p, (_, k) in enumerate(rows[:20].tolist())])
    mixed = powerflow.dc_power_flow(buses[:20], cut, mod[:20], slack_bus=slack, mixed_topologies=True)
    plain = powerflow.dc_power_flow(buses[20:], lines[20:], mod[20:], slack_bus=slack)
    res = powerflow.dc_generator_contingency_screen(buses, lines, gens, slack_bus=slack, contingencies=rows, pickup=pickup, flows=True)
    assert bool(res.converged.all()) and bool(mixed.converged.all()) and bool(plain.converged.all()) and not bool(res.islanding.any())
    worst = 0.0
    for p, (g, k) in enumerate(rows.tolist()):
        want = torch.zeros(E, dtype=torch.float64, device=DEV)
        if k >= 0:
            want[[e for e in range(E) if e != k]] = mixed.line_flow[p]
        else:
            want = plain.line_flow[p - 20]
        got = res.line_flow[p, p]
        err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        worst = max(worst, err / scale)
        assert err <= TOL * scale, (g, k, err, scale)
    print(f'case14 against the expanded route, pickup {kind}: worst scaled error {worst:.3e}')


def test_rows_are_bitwise_reproducible_and_base_is_dc_power_flow():
    s = _case(118, 5, seed=9)
    buses, lines, gens, slack = s
    E, Gn = lines.shape[1], gens.shape[1]
    every = powerflow._generator_contingency_list(None, Gn, E)
    rows = every[np.arange(3, 10098, 17)]                                     # 594 rows: chunks of 8 and a tail
    pickup = _pickup('random', 5, Gn)
    a = _screen(s, contingencies=rows, pickup=pickup, flows=True)
    base = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    for k in base._fields:
        assert _same(getattr(a.base, k), getattr(base, k)), k
    assert torch.equal(a.converged, base.converged) and bool(a.converged.all())
    b = _screen(s, contingencies=rows, pickup=pickup, flows=True)             # from run to run
    for k in ROWS:
        assert _same(getattr(a, k), getattr(b, k)), k
    for sl in (slice(0, 1), slice(2, 4)):                                     # a batch of one grid, another batch
        p = _screen((buses[sl], lines[sl], gens[sl], slack), contingencies=rows, pickup=pickup[sl], flows=True)
        for k in ROWS:
            assert _same(getattr(p, k), getattr(a, k)[sl]), k
    live = int(np.flatnonzero(~a.islanding.cpu().numpy() & (rows[:, 1] >= 0))[17])
    one = _screen((buses[3:4], lines[3:4], gens[3:4], slack), contingencies=rows[live:live + 1], pickup=pickup[3:4], flows=True)
    for k in ROWS:                                                            # one grid, a row alone: one line and one generator
        assert _same(getattr(one, k)[0, 0], getattr(a, k)[3, live]), k
    sub = [100, 3, 64, 63, 585, 0, 64]                                        # a sub-list, out of order, with a duplicate
    p = _screen(s, contingencies=rows[sub], pickup=pickup, flows=True)
    assert p.contingencies.tolist() == rows[sub].tolist()
    for k in ROWS:
        assert _same(getattr(p, k), getattr(a, k)[:, sub]), k
    assert _same(p.line_flow[:, 2], p.line_flow[:, 6])
    p = _screen(s, contingencies=torch.from_numpy(rows[::-1].copy()).to(DEV), pickup=pickup, flows=True)    # reversed, a device tensor
    for k in ROWS:
        assert _same(getattr(p, k), getattr(a, k).flip(1)), k
    assert torch.equal(p.islanding, a.islanding.flip(0))
    full = _screen(s, pickup=pickup)                                          # in the default list (chunks of 32)
    at = torch.from_numpy(_positions(rows, E)).to(DEV)
    assert _same(full.worst_loading[:, at], a.worst_loading) and torch.equal(full.worst_line[:, at], a.worst_line)
    # a 2-D single grid; CPU tensors in, CPU tensors out
    single = powerflow.dc_generator_contingency_screen(buses[3], lines[3], gens[3], slack_bus=slack, contingencies=rows[[live, 5]],
                                                       pickup=pickup[3], flows=True)
    assert single.line_flow.shape == (2, E) and single.worst_loading.shape == (2,) and single.converged.shape == ()
    assert single.base.theta.shape == (118,) and _same(single.line_flow, a.line_flow[3, [live, 5]])
    cpu = powerflow.dc_generator_contingency_screen(buses[:2].cpu(), lines[:2].cpu(), gens[:2].cpu(), slack_bus=slack,
                                                    contingencies=rows[:3], pickup=pickup[:2])
    for t_ in (cpu.worst_loading, cpu.worst_line, cpu.islanding, cpu.converged, cpu.contingencies, cpu.base.theta):
        assert t_.device.type == 'cpu'
    assert cpu.line_flow is None and _same(cpu.worst_loading, a.worst_loading[:2, :3].cpu())
    # rows without a line alone: no line candidate at all
    alone = every[every[:, 1] < 0]
    p = _screen(s, contingencies=alone, pickup=pickup, flows=True)
    at = torch.from_numpy(_positions(alone, E)).to(DEV)
    assert _same(p.worst_loading, full.worst_loading[:, at]) and not bool(p.islanding.any()) and bool(torch.isfinite(p.line_flow).all())
    # not differentiable: the call runs as under no_grad
    req = gens.clone().requires_grad_(True)
    r = powerflow.dc_generator_contingency_screen(buses, lines, req, slack_bus=slack, contingencies=[[0, 1]], flows=True)
    assert not r.line_flow.requires_grad and not r.worst_loading.requires_grad and not r.base.theta.requires_grad


def test_a_bad_grid_fails_alone_and_mixed_batches_are_refused():
    buses, lines, gens, slack = _case(14, 8, seed=4)
    good = _screen((buses, lines, gens, slack), pickup='pmax', flows=True)
    bad = lines.clone()
    bad[5, 7, 3] = 0.0                                                        # x = 0: a numeric failure of that grid's base solve
    res = _screen((buses, bad, gens, slack), pickup='pmax', flows=True)
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert res.converged.tolist() == [True] * 5 + [False] + [True] * 2
    assert torch.equal(res.converged, res.base.converged)
    assert bool(res.line_flow[5].isnan().all()) and bool(res.worst_loading[5].isnan().all()) and bool((res.worst_line[5] == -1).all())
    for k in ROWS:
        assert _same(getattr(res, k)[keep], getattr(good, k)[keep]), k
    slim = _screen((buses, bad, gens, slack), pickup='pmax')
    assert _same(slim.worst_loading, res.worst_loading) and torch.equal(slim.worst_line, res.worst_line)
    mixed = lines.clone()
    mixed[2, 0, 1] = 6.0
    with pytest.raises(ValueError, match='dc_generator_contingency_screen solves one topology'):
        _screen((buses, mixed, gens, slack))
    with pytest.raises(ValueError, match='contingencies must name lines in'):
        _screen((buses, lines, gens, slack), contingencies=[[0, lines.shape[1]]])
    with pytest.raises(ValueError, match='pickup must be non-negative and finite'):
        _screen((buses, lines, gens, slack), pickup=-torch.ones(gens.shape[1], device=DEV))


def test_lds_refusal_names_the_bytes_and_the_formula():
    tp = pt.path(6000)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    want = 8 * (23994 + 6000 + 3 * 5999 + 5999 * 2)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.dc_generator_contingency_screen(buses, lines, gens, slack_bus=tp.slack, contingencies=[[0, -1]])
    assert str(want) in str(e.value) and 'nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)' in str(e.value)
