"""Gradients of the DC generator contingency screen on the MI355X (``powerflow.dc_generator_contingency_screen_differentiable``,
include/gns_powerflow.h "Gradients of the DC generator screen"): against the float64 autograd reference
(``dc_generator_contingency_grad_reference``: the unit redispatched by tensor arithmetic, the line removed, the smaller grid solved
densely), against the product's other routes (``dc_power_flow``'s adjoint for the rows that equal the base; the sum over copies of
``dc_power_flow`` on the expanded, redispatched batch), the properties of the contract, bitwise reproducibility, per-row and per-grid
failure and the LDS refusal.

The bar is the project's DC gradient bar per contract column per grid, as ``test_dc_n2_grad_gpu._check`` applies it: the outputs
are float32, so max|out - ref| <= 1e-5 max|ref| + 1e-7; every column outside the contract is exactly 0 (with ``pickup='pmax'`` the
generators' column 1 joins the contract).  The gradient of a tensor pickup is float64 and is held to 1e-9 max(1, max|ref|), the bar
the CPU replay of the same algorithm meets against the same reference.  A loss reads the rows of ``~islanding`` only unless a test
says otherwise, so islanding rows get an incoming gradient of exactly zero.  Every test prints its worst error / bar.

Generated families (two 'reference' grids with ``_perturbed`` lines, at most 120 non-islanding rows of
``test_dc_generator_contingency_gpu._family_rows``: every generator-alone row, the others at an even stride): a family is held to the bar only if the reference's two
float64 methods (``method='remove'`` and ``method='factors'``) agree per contract column to 1e-8 max|ref| + 1e-10 on those rows on
the CPU.  Worst difference / that bar, both outputs in the loss, a rating and 'pmax':
  random24_stacked_gens 1.9e-6 (96 rows);  ring30_slack_no_gen 4.8e-5 (96);  lattice8x8 4.0e-6 (117);
  random40_parallel_selfloop 1.4e-6 (90).
No family failed the probe; none is dropped."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import dc_generator_contingency_grad_reference as gref
import dc_wide_cases as wide
import pf_topologies as pt
from test_dc_generator_contingency_gpu import _family_rows
from test_dcpf_gpu import _perturbed, _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('buses', 'lines', 'generators')
CONTRACT = {'buses': (2, 4), 'lines': (3, 5, 6), 'generators': (6,)}
FAMILIES = ('random24_stacked_gens', 'ring30_slack_no_gen', 'lattice8x8', 'random40_parallel_selfloop')


def _case(case, batch, seed):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, batch, seed=seed, device=DEV)
    return buses, _perturbed(lines, case), gens, slack


def _weights(bt, p, e, seed, flow=True, worst=True):
    g = torch.Generator().manual_seed(seed)
    wf, ww = torch.randn(bt, p, e, generator=g, dtype=torch.float64).to(DEV), torch.randn(bt, p, generator=g, dtype=torch.float64).to(DEV)
    return (wf if flow else None, ww if worst else None)


def _rating(e, seed, bt=None):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + 2.0 * torch.rand((e,) if bt is None else (bt, e), generator=g, dtype=torch.float64)).to(DEV)


def _pickup(kind, bt, gn, seed=0):
    """None, 'pmax', or random weights in [0.1, 1.1) with one entry exactly zero: 'shared' [Gn], 'per_grid' [Bt,Gn]."""
    if kind in (None, 'pmax'):
        return kind
    w = 0.1 + torch.rand((gn,) if kind == 'shared' else (bt, gn), generator=torch.Generator().manual_seed(gn + seed), dtype=torch.float64)
    w[..., gn // 2] = 0.0
    return w.to(DEV)


def _loss(res, weights, rows=None):
    """sum of the weighted line_flow and worst_loading over the rows of ``rows`` (default: the rows that do not island)."""
    rows = ~res.islanding if rows is None else rows
    loss = 0.0
    if weights[0] is not None:
        loss = loss + (weights[0][..., rows, :] * res.line_flow[..., rows, :]).sum()
    if weights[1] is not None:
        loss = loss + (weights[1][..., rows] * res.worst_loading[..., rows]).sum()
    return loss


def _grads(s, weights, cont=None, pickup=None, rating=None, flows=True, req=(True, True, True), rows=None):
    """(result, gradients of the inputs that require grad, gradient of a tensor pickup or None) of the weighted loss through the
    differentiable screen."""
    ins = [t.detach().clone().requires_grad_(r) for t, r in zip(s[:3], req)]
    leaf = pickup.detach().clone().requires_grad_(True) if isinstance(pickup, torch.Tensor) else None
    res = powerflow.dc_generator_contingency_screen_differentiable(*ins, slack_bus=s[3], contingencies=cont,
                                                                   pickup=pickup if leaf is None else leaf, rating=rating, flows=flows)
    leaves = [t for t in ins if t.requires_grad] + ([] if leaf is None else [leaf])
    g = torch.autograd.grad(_loss(res, weights, rows), leaves)
    return res, (g if leaf is None else g[:-1]), (None if leaf is None else g[-1])


def _reference(s, cont, weights, rating, pickup, grids, rows=None):
    """grid -> (gradients, pickup gradient, flows) of the reference on the rows of ``rows`` (positions in ``cont``; default all)."""
    buses, lines, gens = (t.cpu() for t in s[:3])
    rows = list(range(len(cont))) if rows is None else rows
    out = {}
    for i in grids:
        r = None if rating is None else (rating if rating.dim() == 1 else rating[i]).cpu()
        w = pickup if not isinstance(pickup, torch.Tensor) else (pickup if pickup.dim() == 1 else pickup[i]).cpu()
        out[i] = gref.gradients(buses[i], lines[i], gens[i], s[3], [cont[p] for p in rows],
                                *(None if x is None else x[i].cpu()[rows] for x in weights), rating=r, pickup=w)
    return out


def _check(grads, s, want, name, pickup=None, gp=None):
    contract = dict(CONTRACT, generators=(1, 6)) if isinstance(pickup, str) else CONTRACT
    worst = 0.0
    for i, (ref_grads, _, _) in want.items():
        for k, what in enumerate(NAMES):
            assert grads[k].dtype == torch.float32 and grads[k].shape == s[k].shape
            got, ref = grads[k][i].double().cpu().numpy(), ref_grads[k].numpy()
            for c in range(ref.shape[1]):
                if c not in contract[what]:
                    assert np.all(got[:, c] == 0), (name, i, what, c)
                    continue
                err, scale = np.max(np.abs(got[:, c] - ref[:, c])), np.max(np.abs(ref[:, c]))
                worst = max(worst, err / (1e-5 * scale + 1e-7))
                assert err <= 1e-5 * scale + 1e-7, (name, i, what, c, err, scale)
    if isinstance(pickup, torch.Tensor):                  # float64: the bar of the CPU replay
        assert gp.dtype == pickup.dtype == torch.float64 and gp.shape == pickup.shape
        per_grid = torch.stack([want[i][1] for i in sorted(want)])
        ref = (per_grid.sum(dim=0) if pickup.dim() == 1 else per_grid).numpy()
        got = (gp if pickup.dim() == 1 else gp[sorted(want)]).cpu().numpy()
        err, scale = float(np.max(np.abs(got - ref))), max(1.0, float(np.max(np.abs(ref))))
        worst = max(worst, err / (1e-9 * scale))
        assert err <= 1e-9 * scale and np.any(ref != 0), (name, 'pickup', err, scale)
    else:
        assert gp is None
    print(f'{name}: worst error / bar {worst:.3f}')


def _equal(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def case14():
    """case14, 3 grids, every default row: 105 rows, 25 candidates in one ragged chunk, 14 row chunks of 8 with the last one short."""
    s = _case(14, 3, seed=2)
    E, Gn = s[1].shape[1], s[2].shape[1]
    cont = powerflow._generator_contingency_list(None, Gn, E).tolist()
    assert len(cont) == 105 and E == 20 and Gn == 5
    return s, E, Gn, cont, _weights(3, 105, E, 5)


@pytest.mark.parametrize('kind', [None, 'pmax', 'shared', 'per_grid'])
def test_case14_every_row_against_the_reference_autograd_by_pickup(case14, kind):
    s, E, Gn, cont, weights = case14
    pickup, rating = _pickup(kind, 3, Gn), _rating(E, 6)
    res, grads, gp = _grads(s, weights, pickup=pickup, rating=rating)
    assert int((~res.islanding).sum()) == 100
    want = _reference(s, cont, weights, rating, pickup, range(3))
    for i, (_, _, flows) in want.items():
        assert torch.equal(flows.isnan().all(dim=1), res.islanding.cpu())
    _check(grads, s, want, f'case14 pickup {kind}', pickup, gp)
    if kind == 'pmax':
        assert bool((grads[2][:, :, 1] != 0).any())
    # the forward outputs and base.* are the plain call's, bit for bit
    plain = powerflow.dc_generator_contingency_screen(*s[:3], slack_bus=s[3], pickup=pickup, rating=rating, flows=True)
    assert not plain.worst_loading.requires_grad and res.worst_loading.requires_grad and res.line_flow.requires_grad
    for a, b in ((res.line_flow, plain.line_flow), (res.worst_loading, plain.worst_loading), (res.worst_line, plain.worst_line),
                 (res.converged, plain.converged), (res.islanding, plain.islanding), (res.base.theta, plain.base.theta),
                 (res.base.line_flow, plain.base.line_flow), (res.base.slack_p, plain.base.slack_p)):
        assert _same(a.detach(), b)


@pytest.mark.parametrize('rating_kind', ['none', 'per_line', 'per_grid'])
def test_case14_every_row_against_the_reference_autograd_by_rating(case14, rating_kind):
    s, E, Gn, cont, weights = case14
    rating = {'none': None, 'per_line': _rating(E, 6), 'per_grid': _rating(E, 7, 3)}[rating_kind]
    res, grads, gp = _grads(s, weights, pickup='pmax', rating=rating)
    _check(grads, s, _reference(s, cont, weights, rating, 'pmax', range(3)), f'case14 rating {rating_kind}', 'pmax', gp)


def test_case30_default_rows_pmax():
    s = _case(30, 2, seed=30)
    E, Gn = s[1].shape[1], s[2].shape[1]
    cont = powerflow._generator_contingency_list(None, Gn, E).tolist()
    weights, rating = _weights(2, len(cont), E, 31), _rating(E, 32)
    res, grads, gp = _grads(s, weights, pickup='pmax', rating=rating)
    assert len(cont) == 252 and int(res.islanding.sum()) == 30
    _check(grads, s, _reference(s, cont, weights, rating, 'pmax', range(2)), 'case30', 'pmax', gp)


def test_case14_each_incoming_gradient_alone_and_each_input_alone(case14):
    s, E, Gn, cont, weights = case14
    rating = _rating(E, 6)
    _, both, _ = _grads(s, weights, pickup='pmax', rating=rating)
    for name, w in (('line_flow', (weights[0], None)), ('worst_loading', (None, weights[1]))):
        _, g, _ = _grads(s, w, pickup='pmax', rating=rating)
        _check(g, s, _reference(s, cont, w, rating, 'pmax', range(3)), f'case14 {name} alone', 'pmax')
    # flows=False: the bits of the worst-only gradient taken with flows=True
    _, worst_only, _ = _grads(s, (None, weights[1]), pickup='pmax', rating=rating)
    res, g, _ = _grads(s, (None, weights[1]), pickup='pmax', rating=rating, flows=False)
    assert res.line_flow is None and _equal(g, worst_only)
    # each input requiring grad alone: the bits of all three (the generators carry the weights' column with them)
    for k in range(3):
        _, g, _ = _grads(s, weights, pickup='pmax', rating=rating, req=tuple(j == k for j in range(3)))
        assert len(g) == 1 and _same(g[0], both[k]), k
    # the weights alone: a tensor pickup that requires grad while no input does
    w = _pickup('per_grid', 3, Gn)
    _, all_in, gp_all = _grads(s, weights, pickup=w, rating=rating)
    _, none_in, gp = _grads(s, weights, pickup=w, rating=rating, req=(False, False, False))
    assert len(none_in) == 0 and _same(gp, gp_all)


@pytest.mark.parametrize('name', FAMILIES)
def test_generated_families_against_the_reference_autograd(name):
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, len(name)), gens, tp.slack)
    E = tp.f.size
    cont = family_rows(name, tp)
    assert 0 < len(cont) <= 120
    weights, rating = _weights(2, len(cont), E, len(name)), _rating(E, 8)
    res, grads, gp = _grads(s, weights, cont=cont, pickup='pmax', rating=rating)
    assert not bool(res.islanding.any())
    _check(grads, s, _reference(s, cont, weights, rating, 'pmax', range(2)), name, 'pmax', gp)


def family_rows(name, tp):
    """At most 120 non-islanding rows of ``_family_rows``, at an even stride through them, every generator-alone row kept first."""
    rows = _family_rows(name, tp)
    rows = rows[~powerflow._generator_islanding(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1), rows)]
    alone = rows[rows[:, 1] < 0]
    rest = rows[rows[:, 1] >= 0]
    room = 120 - alone.shape[0]
    assert room > 0
    step = max(1, -(-rest.shape[0] // room))
    return np.concatenate([alone, rest[::step]]).tolist()


@pytest.mark.parametrize('name', ['path64', 'path65', 'path66_pv1'])
def test_wave_edges_with_every_line_a_bridge(name):
    """E = 63, 64, 65: the last lane of a pass, a full pass, one line into the second pass.  Every line is a bridge, so the rows are
    the generator-alone ones."""
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, len(name)), gens, tp.slack)
    E, Gn = tp.f.size, tp.g.size
    assert E == {'path64': 63, 'path65': 64, 'path66_pv1': 65}[name]
    cont = [[g, -1] for g in range(Gn)]
    weights, rating = _weights(2, Gn, E, E), _rating(E, E + 1)
    res, grads, gp = _grads(s, weights, cont=cont, pickup='pmax', rating=rating)
    assert not bool(res.islanding.any())
    _check(grads, s, _reference(s, cont, weights, rating, 'pmax', range(2)), name, 'pmax', gp)


def test_a_unit_on_the_slack_with_no_pickup_is_the_base_case():
    """Row (g, -1) of a unit on the slack bus with pickup None equals the base: its gradient is that of the same loss on
    ``base.line_flow`` through ``dc_power_flow``'s adjoint, to the bar."""
    s = _case(14, 2, seed=7)
    E = s[1].shape[1]
    _, _, gbus = synth.case_topology(14)
    g = int(np.flatnonzero(gbus == s[3])[0])
    weights, rating = _weights(2, 1, E, 41), _rating(E, 42)
    res, grads, _ = _grads(s, weights, cont=[[g, -1]], rating=rating)
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    dc = powerflow.dc_power_flow(*ins, slack_bus=s[3])
    assert _same(res.line_flow[:, 0].detach(), dc.line_flow.detach())
    load = (dc.line_flow.abs() / rating).amax(dim=1)
    want = torch.autograd.grad((weights[0][:, 0] * dc.line_flow).sum() + (weights[1][:, 0] * load).sum(), ins)
    worst = 0.0
    for k, what in enumerate(NAMES):
        for i in range(2):
            for c in range(want[k].shape[2]):
                a, b = grads[k][i, :, c].double(), want[k][i, :, c].double()
                if c not in CONTRACT[what]:
                    assert bool((a == 0).all())
                    continue
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                worst = max(worst, err / (1e-5 * scale + 1e-7))
                assert err <= 1e-5 * scale + 1e-7, (what, i, c, err, scale)
    print(f'slack unit, no pickup: worst error / bar {worst:.3f}')


def test_properties_of_the_contract():
    s = _case(30, 2, seed=6)
    E, Gn = s[1].shape[1], s[2].shape[1]
    rating = _rating(E, 13)
    f, t, gbus = synth.case_topology(30)
    live = np.flatnonzero(~powerflow._bridges(30, f - 1, t - 1))
    k, k2 = int(live[3]), int(live[10])
    # a single row (g, k), and rows that all share line k: exact zeros in line k's columns
    for cont in ([[1, k]], [[0, k], [2, k], [3, k]]):
        _, g, _ = _grads(s, _weights(2, len(cont), E, k), cont=cont, pickup='pmax', rating=rating)
        assert bool(torch.isfinite(g[1]).all()) and bool((g[1] != 0).any()) and bool((g[1][:, k, :] == 0).all()), cont
    _, g, _ = _grads(s, _weights(2, 2, E, 3), cont=[[1, k], [1, k2]], pickup='pmax', rating=rating)
    assert bool((g[1][:, [k, k2]][..., [3, 5, 6]] != 0).all())
    # pickup None: the slack absorbs the loss, so row (g, -1) alone does not depend on Pg_g
    off = int(np.flatnonzero(gbus != s[3])[0])
    w = _weights(2, 1, E, 9)
    _, g, _ = _grads(s, w, cont=[[off, -1]], rating=rating)
    ref = _reference(s, [[off, -1]], w, rating, None, range(2))
    _check(g, s, ref, 'Pg of the outaged unit, no pickup')
    scale = float(g[2][:, :, 6].abs().max())
    assert float(g[2][:, off, 6].abs().max()) <= 1e-5 * scale + 1e-7 and scale > 0
    # 'pmax' reaches the generators' column 1; None leaves exact zeros there
    cont = [[0, -1], [2, k], [4, k2]]
    w3 = _weights(2, 3, E, 10)
    _, g, _ = _grads(s, w3, cont=cont, pickup='pmax', rating=rating)
    _, g0, _ = _grads(s, w3, cont=cont, rating=rating)
    assert bool((g[2][:, :, 1] != 0).any()) and bool((g0[2][:, :, 1] == 0).all())
    # W_g == 0: unit 0 out and every other weight exactly zero, so the slack picks up and the weights get exact zeros
    zero = torch.zeros(Gn, dtype=torch.float64, device=DEV)
    zero[0] = 2.0
    _, g, gp = _grads(s, tuple(x[:, :2] for x in w3), cont=[[0, -1], [0, k]], pickup=zero, rating=rating)
    assert bool((gp == 0).all()) and bool((g[2][:, :, 6] != 0).any())


def _expanded(s, cont, weights, rating):
    """Autograd through ``dc_power_flow`` on the expanded batch redispatched by 'pmax' (one copy per (grid, row), the line deleted,
    mixed topologies for the rows with a line), summed over copies."""
    bt, E, Gn = s[0].shape[0], s[1].shape[1], s[2].shape[1]
    ins = [x.detach().clone().requires_grad_(True) for x in s[:3]]
    w = ins[2][:, :, 1].double()
    total = torch.zeros((), dtype=torch.float64, device=DEV)
    for lined in (False, True):
        at = [p for p, (g, k) in enumerate(cont) if (k >= 0) == lined]
        if not at:
            continue
        copies_g = []
        for p in at:
            g = cont[p][0]
            out = torch.ones(Gn, dtype=torch.float64, device=DEV)
            out[g] = 0.0
            others = w * out
            pg = ins[2][:, :, 6].double() * out + ins[2][:, g, 6].double().unsqueeze(1) * (others / others.sum(dim=1, keepdim=True))
            copies_g.append(torch.cat([ins[2][:, :, :6], pg.float().unsqueeze(2)], dim=2))
        xg = torch.stack(copies_g, dim=1).reshape(bt * len(at), Gn, 7)
        xb = ins[0].repeat_interleave(len(at), dim=0)
        if lined:
            keep = torch.tensor(np.array([np.delete(np.arange(E), cont[p][1]) for p in at]), device=DEV)
            xl = ins[1][:, keep].reshape(bt * len(at), E - 1, 7)
            res = powerflow.dc_power_flow(xb, xl, xg, slack_bus=s[3], mixed_topologies=True)
            n = E - 1
            rt = rating[keep].unsqueeze(0)
            wf = torch.gather(weights[0][:, at], 2, keep.unsqueeze(0).expand(bt, len(at), n))
        else:
            xl = ins[1].repeat_interleave(len(at), dim=0)
            res = powerflow.dc_power_flow(xb, xl, xg, slack_bus=s[3])
            n, rt, wf = E, rating.view(1, 1, E), weights[0][:, at]
        assert bool(res.converged.all())
        flow = res.line_flow.reshape(bt, len(at), n)
        total = total + (wf * flow).sum() + (weights[1][:, at] * (flow.abs() / rt).amax(dim=2)).sum()
    return torch.autograd.grad(total, ins)


@pytest.mark.parametrize('case,count', [(14, 24), (118, 32)])
def test_agrees_with_the_sum_over_copies_of_the_expanded_route(case, count):
    """The route the adjoint replaces.  The copies' ``Pg`` is rounded to float32 on the way in, as that route has it."""
    bt = 2
    s = _case(case, bt, seed=case + 1)
    E, Gn = s[1].shape[1], s[2].shape[1]
    every = powerflow._generator_contingency_list(None, Gn, E)
    f, t, _ = synth.case_topology(case)
    live = every[~powerflow._generator_islanding(powerflow._bridges(case, f - 1, t - 1), every)]
    cont = live[np.linspace(0, live.shape[0] - 1, count).astype(int)].tolist()
    weights, rating = _weights(bt, len(cont), E, 11), _rating(E, 12)
    res, grads, _ = _grads(s, weights, cont=cont, pickup='pmax', rating=rating)
    assert not bool(res.islanding.any()) and any(k < 0 for _, k in cont) and any(k >= 0 for _, k in cont)
    want = _expanded(s, cont, weights, rating)
    worst = 0.0
    for k, what in enumerate(NAMES):
        for i in range(bt):
            for c in (CONTRACT[what] if what != 'generators' else (1, 6)):
                a, b = grads[k][i, :, c].double(), want[k][i, :, c].double()
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                worst = max(worst, err / (1e-5 * scale + 1e-7))
                assert err <= 1e-5 * scale + 1e-7, (what, i, c, err, scale)
    print(f'case{case} expanded route: worst error / bar {worst:.3f}')


def test_bits_alone_in_a_batch_of_five_and_from_run_to_run():
    s = _case(14, 5, seed=15)
    E, Gn = s[1].shape[1], s[2].shape[1]
    cont = powerflow._generator_contingency_list(None, Gn, E)[::3].tolist()
    w = _pickup('per_grid', 5, Gn)
    weights, rating = _weights(5, len(cont), E, 16), _rating(E, 17)
    _, a, gpa = _grads(s, weights, cont=cont, pickup=w, rating=rating)
    _, b, gpb = _grads(s, weights, cont=cont, pickup=w, rating=rating)
    assert _equal(a, b) and _same(gpa, gpb)
    for sel in ([3], [4, 0, 2]):                     # alone, and at other positions of a smaller batch
        sub = tuple(x[sel] for x in s[:3]) + (s[3],)
        _, p, gp = _grads(sub, tuple(x[sel] for x in weights), cont=cont, pickup=w[sel], rating=rating)
        assert _equal(p, [x[sel] for x in a]) and _same(gp, gpa[sel]), sel


def test_islanding_rows_and_failure_per_grid():
    s = _case(14, 4, seed=4)
    E, Gn = s[1].shape[1], s[2].shape[1]
    cont = powerflow._generator_contingency_list(None, Gn, E).tolist()
    weights = _weights(4, len(cont), E, 17)
    w = _pickup('per_grid', 4, Gn)
    res, good, gp_good = _grads(s, weights, pickup=w)
    isl = res.islanding
    assert int(isl.sum()) == 5 and all(bool(torch.isfinite(x).all()) for x in good) and bool(torch.isfinite(gp_good).all())
    # a non-zero weight into an islanding row of grid 2 (the loss reads every row): NaN rows for that grid only
    everything = torch.ones_like(isl)
    wf, wl = weights[0].clone(), weights[1].clone()
    wf[:, isl] = 0
    wl[:, isl] = 0
    wl[2, int(torch.nonzero(isl)[0])] = 1.5
    _, g, gp = _grads(s, (wf, wl), pickup=w, rows=everything)
    for x, y in zip((*g, gp), (*good, gp_good)):
        assert bool(x[2].isnan().all()) and _same(x[[0, 1, 3]], y[[0, 1, 3]])
    # weights that are exactly zero on the islanding rows, read through the NaN rows: as the indexed loss, bit for bit
    wl[2] = torch.where(isl, 0.0, wl[2])
    _, g, gp = _grads(s, (wf, wl), pickup=w, rows=everything)
    assert _equal(g, good) and _same(gp, gp_good)


def test_a_grid_whose_base_solve_fails():
    """The constructed zero-pivot grid of ``dc_wide_cases``: grid 1 is not solved."""
    buses, lines, gens, slack = wide.zero_pivot_batch()
    s = (buses.to(DEV), lines.to(DEV), gens.to(DEV), slack)
    E, Gn = lines.shape[1], gens.shape[1]
    cont = [[0, -1], [1, 0], [2, 1], [1, -1]]
    weights = _weights(3, len(cont), E, 5)
    w = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64, device=DEV).repeat(3, 1)
    res, g, gp = _grads(s, weights, cont=cont, pickup=w)
    assert res.converged.tolist() == [True, False, True] and bool(res.worst_loading[1].isnan().all()) and not bool(res.islanding.any())
    for x in (*g, gp):
        assert bool(x[1].isnan().all()) and bool(torch.isfinite(x[[0, 2]]).all())
    zero = tuple(x.clone() for x in weights)
    zero[0][1] = 0
    zero[1][1] = 0
    _, g0, gp0 = _grads(s, zero, cont=cont, pickup=w)
    for x, y in zip((*g0, gp0), (*g, gp)):
        assert bool((x[1] == 0).all()) and _same(x[[0, 2]], y[[0, 2]])


def test_lds_refusal_names_the_adjoints_image():
    tp = pt.path(6000)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    want = 8 * (23994 + 6000 + 3 * 5999 + 2 * 5999 * 2 + 3)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.dc_generator_contingency_screen_differentiable(buses, lines.requires_grad_(True), gens, slack_bus=tp.slack,
                                                                 contingencies=[[0, -1]])
    assert str(want) in str(e.value) and '2 dim_p (W + 1) + 3 W' in str(e.value)
    assert powerflow._DCG1_ADJOINT_LDS_FORMULA in str(e.value)
