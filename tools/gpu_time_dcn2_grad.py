"""Forward + backward of the differentiable DC N-2 contingency screen against the route it replaces.
``dc_n2_contingency_screen(differentiable=True, flows=False)`` on Bt grids and a pair list (the shapes of ``gpu_time_dcn2.py``), with
the loss ``worst_loading[~islanding].sum()``, is timed as the whole Python call and its backward between HIP events; the forward
alone (the same call, no backward) gives the backward's share.  The other route is ``dc_power_flow(mixed_topologies=True)`` with
requires_grad on the expanded batch (each grid once per pair, with both line rows removed), autograd summing over the copies, with
the loss ``max_l |flow|`` summed, on a seeded sample of at most ``sample`` non-islanding pairs after its caches are warm; its time
per (grid, pair) is scaled to the whole list for the ratio, and said so.  5 repeats after 2 warm-ups, each repeat timed on its own;
the median is quoted with the spread.  The two routes' gradients are compared on the sample (the screen run on the sampled pairs
alone) relative to the project's DC gradient bar (1e-5 max|ref| + 1e-7 per contract column per grid).
usage: python tools/gpu_time_dcn2_grad.py [case:batch:pairs[:sample] ...] > profiles/dcn2_grad/gpu_time.txt     (pairs 0: every pair)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth

CONTRACT = ((2, 4), (3, 5, 6), (6,))


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


specs = sys.argv[1:] or ['14:512:0', '118:64:0', '300:8:20000']
for spec in specs:
    case, bt, n_pairs, sample = (list(map(int, spec.split(':'))) + [2000])[:4]
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    every = powerflow._pair_list(None, E)
    rng = np.random.default_rng(case)
    pairs = every if n_pairs <= 0 or n_pairs >= every.shape[0] else every[np.sort(rng.choice(every.shape[0], n_pairs, replace=False))]
    P = pairs.shape[0]
    isl = powerflow._pair_islanding(case, f - 1, t - 1, pairs)
    live = np.flatnonzero(~isl)
    live_dev = torch.from_numpy(live).cuda()
    print(f'case{case} x {bt} grids x {P} pairs ({int(isl.sum())} islanding) of {E} lines = {bt * P} rows', flush=True)

    def forward(pairs=pairs, grad=True):
        ins = [x.detach().clone().requires_grad_(grad) for x in (bu, li, ge)]
        return ins, powerflow.dc_n2_contingency_screen(*ins, slack_bus=slack, pairs=pairs, differentiable=True)

    def both(pairs=pairs, rows=live_dev):
        ins, res = forward(pairs)
        return torch.autograd.grad(res.worst_loading[:, rows].sum(), ins)

    ms_fwd, _ = event_ms(lambda: forward()[1].worst_loading)
    ms_both, _ = event_ms(both)
    share = (np.median(ms_both) - np.median(ms_fwd)) / np.median(ms_both)
    print(f'  screen flows=False, forward alone (graph recorded): {show(ms_fwd)}', flush=True)
    print(f'  screen flows=False, forward + backward of worst_loading[~islanding].sum(): {show(ms_both)}; the backward is '
          f'{100 * share:.0f}% of it', flush=True)
    # the expanded batch of the other route on a sample: pair (i, p) is grid i without the two lines of pair p
    pick = live if live.size <= sample else np.sort(rng.choice(live, sample, replace=False))
    S = pick.size
    keep = torch.tensor(np.array([np.delete(np.arange(E), pairs[p]) for p in pick]), device='cuda')          # [S, E-2]

    def expanded():
        ins = [x.detach().clone().requires_grad_(True) for x in (bu, li, ge)]
        xl = ins[1][:, keep].reshape(bt * S, E - 2, 7)
        xb, xg = ins[0].repeat_interleave(S, dim=0), ins[2].repeat_interleave(S, dim=0)
        flow = powerflow.dc_power_flow(xb, xl, xg, slack_bus=slack, mixed_topologies=True).line_flow
        return torch.autograd.grad(flow.reshape(bt, S, E - 2).abs().amax(dim=2).sum(), ins)

    ms_mixed, want = event_ms(expanded)
    scaled = np.median(ms_mixed) * live.size / S
    got = both(pairs[pick], torch.arange(S, device='cuda'))
    worst = 0.0
    for a, b, cols in zip(got, want, CONTRACT):
        for c in cols:
            err = (a[:, :, c].double() - b[:, :, c].double()).abs().amax(dim=1)
            worst = max(worst, float((err / (1e-5 * b[:, :, c].double().abs().amax(dim=1) + 1e-7)).max()))
    print(f'  expanded dc_power_flow(mixed_topologies=True) forward + backward, {bt * S} grids on {S} topologies (a sample of the '
          f'{live.size} non-islanding pairs), caches warm: {show(ms_mixed)}; scaled to {live.size} pairs: {scaled:.1f} ms', flush=True)
    print(f'  expanded (scaled) / screen, forward + backward: {scaled / np.median(ms_both):.1f}x'
          f"{'  (the screen is SLOWER here)' if scaled < np.median(ms_both) else ''}; worst difference of the two routes' gradients on "
          f'the sample / bar {worst:.3f}', flush=True)
