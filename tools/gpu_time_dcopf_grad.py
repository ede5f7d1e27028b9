"""Times ``powerflow.dc_optimal_power_flow_differentiable`` with its backward: the whole Python call between HIP events, the median
of 5 repeats after 2 warm-ups, on the shapes and problems of ``tools/gpu_time_dcopf.py`` (quadratic and linear costs, every line
rated).  Per shape: the plain forward (``dc_optimal_power_flow``, re-measured in the same run), forward + backward of
``objective.sum() + lmp.sum()`` with ``requires_grad`` on buses, generators, cost and rating, the backward's share of that, and how
many grids got NaN gradient rows (a grid that did not converge, or whose KKT order exceeds what the LDS image holds).
usage: python tools/gpu_time_dcopf_grad.py [case:batch ...] > profiles/dcopf_grad/gpu_time.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth


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


def problem(case, bt, quad, seed=1):
    """(buses, lines, gens, cost [Bt,Gn,2], rating [Bt,E], slack) on the device: ``tools/gpu_time_dcopf.py``'s recipe."""
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=seed, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(seed + 1000 * case + int(quad))
    Gn = ge.shape[1]
    bu = bu.clone()
    bu[:, :, 2] = bu[:, :, 2].abs() + 0.01                               # loads, so that the demand is positive
    demand = (bu[:, :, 2].double() + bu[:, :, 4].double()).sum(dim=1, keepdim=True)
    share = torch.rand(bt, Gn, generator=g, device='cuda', dtype=torch.float64) + 0.5
    p0 = demand * share / share.sum(dim=1, keepdim=True)
    ge = ge.clone()
    ge[:, :, 1] = (p0 * (1.1 + 0.7 * torch.rand(bt, Gn, generator=g, device='cuda', dtype=torch.float64))).float()
    ge[:, :, 2] = (p0 * (0.3 + 0.6 * torch.rand(bt, Gn, generator=g, device='cuda', dtype=torch.float64))).float()
    ge[:, :, 6] = p0.float()
    flow = powerflow.dc_power_flow(bu, li, ge, slack_bus=slack).line_flow
    rating = torch.clamp(1.05 * flow.abs(), min=0.02)
    cost = torch.zeros(bt, Gn, 2, dtype=torch.float64, device='cuda')
    cost[:, :, 1] = 10.0 + 30.0 * torch.rand(bt, Gn, generator=g, device='cuda', dtype=torch.float64)
    if quad:
        cost[:, :, 0] = 0.5 + 4.5 * torch.rand(bt, Gn, generator=g, device='cuda', dtype=torch.float64)
    return bu, li, ge, cost, rating, slack


specs = sys.argv[1:] or ['14:512', '118:64', '300:8', '118:4096']
for spec in specs:
    case, bt = map(int, spec.split(':'))
    for quad in (True, False):
        bu, li, ge, cost, rating, slack = problem(case, bt, quad)
        E, Gn = li.shape[1], ge.shape[1]
        leaves = [t.clone().requires_grad_() for t in (bu, ge, cost, rating)]

        def forward():
            return powerflow.dc_optimal_power_flow(bu, li, ge, cost=cost, rating=rating, slack_bus=slack)

        def twin_forward():
            return powerflow.dc_optimal_power_flow_differentiable(leaves[0], li, leaves[1], cost=leaves[2], rating=leaves[3], slack_bus=slack)

        def both():
            for t in leaves:
                t.grad = None
            res = twin_forward()
            (res.objective.sum() + res.lmp.sum()).backward()
            return res

        fwd, res = event_ms(forward)
        twin, _ = event_ms(twin_forward)
        fb, _ = event_ms(both)
        nan_rows = int(torch.isnan(leaves[0].grad[:, 0, 2]).sum())
        f, t, a = np.median(fwd), np.median(twin), np.median(fb)
        print(f"case{case} x {bt} {'QP' if quad else 'LP'} (E {E}, Gn {Gn}, every line rated): plain forward median {f:.3f} ms "
              f"(min {fwd.min():.3f}, max {fwd.max():.3f}); the twin's forward {t:.3f} ms; forward + backward {a:.3f} ms "
              f"(min {fb.min():.3f}, max {fb.max():.3f}) = {a / f:.2f}x the plain forward; the backward's share {(a - t) / a * 100:.1f} % "
              f"= {(a - t) * 1e3 / bt:.1f} us per grid; converged {int(res.converged.sum())} of {bt}; NaN gradient rows {nan_rows} of {bt}",
              flush=True)
