"""Forward + backward of the differentiable DC generator contingency screen against the route it replaces.
``dc_generator_contingency_screen_differentiable(flows=False, pickup='pmax')`` on Bt grids and the default list (the shapes of
``gpu_time_dcg1.py``), with the loss ``worst_loading[~islanding].sum()``, is timed as the whole Python call and its backward between
HIP events; the forward alone (the same call, no backward) gives the backward's share.  The other route is ``dc_power_flow`` with
requires_grad on the expanded, redispatched batch (each grid once per row, the unit's ``Pg`` shared out by differentiable tensor
arithmetic, ``mixed_topologies=True`` and the line's row removed for the rows with a line), autograd summing over the copies, with
the loss ``max_l |flow|`` summed, on a seeded sample of at most ``sample`` non-islanding rows with a line and ``sample / 8`` rows
without one after its caches are warm; its time per (grid, row) is scaled to the whole list for the ratio, and said so.  5 repeats
after 2 warm-ups, each repeat timed on its own; the median is quoted with the spread.  The two routes' gradients are compared on the
sample (the screen run on the sampled rows alone) relative to the project's DC gradient bar (1e-5 max|ref| + 1e-7 per contract
column per grid, the generators' column 1 included).
usage: python tools/gpu_time_dcg1_grad.py [case:batch[:sample] ...] > profiles/dcg1_grad/gpu_time.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth

CONTRACT = ((2, 4), (3, 5, 6), (1, 6))


def event_ms(fn, reps=5, warm=2):
    for _ in range(warm):
        out = fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms), out


def show(ms):
    return f'{np.median(ms):.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})'


def redispatched(ge, rows):
    """[Bt * S, Gn, 7] float32 on the graph of ``ge``: grid i once per row of ``rows``, the row's generator out and its Pg shared in
    proportion to column 1."""
    bt, Gn = ge.shape[0], ge.shape[1]
    S = rows.shape[0]
    out = torch.zeros(S, Gn, dtype=torch.bool, device='cuda')
    out[torch.arange(S, device='cuda'), torch.from_numpy(rows[:, 0]).cuda()] = True
    pg = ge[:, :, 6].double().unsqueeze(1).expand(bt, S, Gn)
    lost = (pg * out).sum(dim=2, keepdim=True)
    w = ge[:, :, 1].double().unsqueeze(1) * ~out
    new = torch.where(out, torch.zeros_like(pg), pg) + lost * w / w.sum(dim=2, keepdim=True)
    x = torch.cat([ge[:, :, :6].unsqueeze(1).expand(bt, S, Gn, 6), new.float().unsqueeze(3)], dim=3)
    return x.reshape(bt * S, Gn, 7)


specs = sys.argv[1:] or ['14:512', '118:64', '300:8']
for spec in specs:
    case, bt, sample = (list(map(int, spec.split(':'))) + [1000])[:3]
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E, Gn = f.size, g.size
    rows = powerflow._generator_contingency_list(None, Gn, E)
    P = rows.shape[0]
    isl = powerflow._generator_islanding(powerflow._bridges(case, f - 1, t - 1), rows)
    live_dev = torch.from_numpy(np.flatnonzero(~isl)).cuda()
    print(f'case{case} x {bt} grids x {P} rows ({Gn} generators x (1 + {E} lines), {int(isl.sum())} islanding) = {bt * P} rows', flush=True)

    def forward(cont=None, grad=True):
        ins = [x.detach().clone().requires_grad_(grad) for x in (bu, li, ge)]
        return ins, powerflow.dc_generator_contingency_screen_differentiable(*ins, slack_bus=slack, contingencies=cont, pickup='pmax')

    def both(cont=None, at=live_dev):
        ins, res = forward(cont)
        return torch.autograd.grad(res.worst_loading[:, at].sum(), ins)

    ms_plain, _ = event_ms(lambda: powerflow.dc_generator_contingency_screen(bu, li, ge, slack_bus=slack, pickup='pmax').worst_loading)
    ms_fwd, _ = event_ms(lambda: forward()[1].worst_loading)
    ms_both, _ = event_ms(both)
    share = (np.median(ms_both) - np.median(ms_fwd)) / np.median(ms_both)
    print(f"  plain dc_generator_contingency_screen flows=False pickup='pmax' (no graph): {show(ms_plain)}", flush=True)
    print(f'  differentiable screen flows=False, forward alone (graph recorded): {show(ms_fwd)}', flush=True)
    print(f'  differentiable screen flows=False, forward + backward of worst_loading[~islanding].sum(): {show(ms_both)}; the backward '
          f'is {100 * share:.0f}% of it', flush=True)
    # the expanded batch of the other route on a sample: row (i, p) is grid i redispatched, without the row's line
    rng = np.random.default_rng(case)
    live = np.flatnonzero(~isl & (rows[:, 1] >= 0))
    alone = np.flatnonzero(rows[:, 1] < 0)
    pick = live if live.size <= sample else np.sort(rng.choice(live, sample, replace=False))
    pick_a = alone if alone.size <= max(1, sample // 8) else np.sort(rng.choice(alone, max(1, sample // 8), replace=False))
    S, Sa = pick.size, pick_a.size
    keep = torch.tensor(np.array([np.delete(np.arange(E), rows[p, 1]) for p in pick]), device='cuda')            # [S, E-1]

    def expanded_lined():
        ins = [x.detach().clone().requires_grad_(True) for x in (bu, li, ge)]
        xl = ins[1][:, keep].reshape(bt * S, E - 1, 7)
        flow = powerflow.dc_power_flow(ins[0].repeat_interleave(S, dim=0), xl, redispatched(ins[2], rows[pick]), slack_bus=slack,
                                       mixed_topologies=True).line_flow
        return torch.autograd.grad(flow.reshape(bt, S, E - 1).abs().amax(dim=2).sum(), ins)

    def expanded_alone():
        ins = [x.detach().clone().requires_grad_(True) for x in (bu, li, ge)]
        flow = powerflow.dc_power_flow(ins[0].repeat_interleave(Sa, dim=0), ins[1].repeat_interleave(Sa, dim=0),
                                       redispatched(ins[2], rows[pick_a]), slack_bus=slack).line_flow
        return torch.autograd.grad(flow.reshape(bt, Sa, E).abs().amax(dim=2).sum(), ins, allow_unused=True)

    ms_mixed, want = event_ms(expanded_lined)
    ms_alone, want_a = event_ms(expanded_alone)
    scaled = np.median(ms_mixed) * live.size / S + np.median(ms_alone) * alone.size / Sa
    want = [a + (0 if b is None else b) for a, b in zip(want, want_a)]
    got = both(rows[np.concatenate([pick, pick_a])], torch.arange(S + Sa, device='cuda'))
    worst = 0.0
    for a, b, cols in zip(got, want, CONTRACT):
        for c in cols:
            err = (a[:, :, c].double() - b[:, :, c].double()).abs().amax(dim=1)
            worst = max(worst, float((err / (1e-5 * b[:, :, c].double().abs().amax(dim=1) + 1e-7)).max()))
    print(f'  expanded dc_power_flow(mixed_topologies=True) forward + backward, {bt * S} grids on {np.unique(rows[pick, 1]).size} '
          f'topologies (a sample of the {live.size} non-islanding rows with a line), caches warm: {show(ms_mixed)}; dc_power_flow '
          f'forward + backward on {bt * Sa} grids (a sample of the {alone.size} rows without a line): {show(ms_alone)}; scaled to the '
          f'list: {scaled:.1f} ms', flush=True)
    print(f'  expanded (scaled) / screen, forward + backward: {scaled / np.median(ms_both):.1f}x'
          f"{'  (the screen is SLOWER here)' if scaled < np.median(ms_both) else ''}; worst difference of the two routes' gradients on "
          f'the sample / bar {worst:.3f}', flush=True)
