"""Times ``powerflow.dc_optimal_power_flow``: the whole Python call between HIP events, the median of 5 repeats after 2 warm-ups, on
case-shaped batches with quadratic (QP) and linear (LP) costs, next to one CPU core's time per grid of ``scipy.optimize.linprog``
(HiGHS) for the LPs and of the tests' numpy reference for the QPs (on the first ``cpu_grids`` grids of the batch; the reference for
both where SciPy is absent, and said so).  The problems follow the tests' recipe on the device: a dispatch p0 that meets the
demand, bounds around it, every line rated max(1.05 |flow(p0)|, 0.02), distinct costs.  Also printed: the distribution of the
iteration counts and the share of grids that converged.
usage: python tools/gpu_time_dcopf.py [case:batch ...] > profiles/dcopf/gpu_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth
import dc_opf_reference as ref

CPU_GRIDS = 2


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
    """(buses, lines, gens, cost [Bt,Gn,2], rating [Bt,E], slack) on the device."""
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


def cpu_seconds_per_grid(bu, li, ge, cost, rating, slack, quad):
    """(seconds per grid, solver name, worst relative objective difference to the device's on those grids is left to the caller)."""
    try:
        import scipy.optimize as so
    except ImportError:
        so = None
    n = min(CPU_GRIDS, bu.shape[0])
    t, objs = 0.0, []
    for i in range(n):
        p = (bu[i].double().cpu().numpy(), li[i].double().cpu().numpy(), ge[i].double().cpu().numpy(), cost[i].cpu().numpy(),
             rating[i].cpu().numpy(), slack)
        if quad or so is None:
            t0 = time.perf_counter()
            r = ref.solve(*p)
            t += time.perf_counter() - t0
            objs.append(r['objective'] if r['converged'] else float('nan'))
        else:
            m = ref._model(*p)
            nth, nl = m['nth'], m['lim'].size
            t0 = time.perf_counter()
            res = so.linprog(np.concatenate([np.zeros(nth), m['c1']]), A_ub=m['A'][:2 * nl], b_ub=m['ub'][:2 * nl], A_eq=m['G'],
                             b_eq=m['load'], bounds=[(None, None)] * nth + list(zip(m['pmin'], m['pmax'])), method='highs')
            t += time.perf_counter() - t0
            objs.append(res.fun if res.status == 0 else float('nan'))
    return t / n, ('numpy reference' if quad or so is None else 'scipy linprog (HiGHS)'), np.array(objs)


torch.set_num_threads(1)
specs = sys.argv[1:] or ['14:512', '118:64', '300:8', '118:4096']
for spec in specs:
    case, bt = map(int, spec.split(':'))
    for quad in (True, False):
        bu, li, ge, cost, rating, slack = problem(case, bt, quad)
        E, Gn = li.shape[1], ge.shape[1]
        ms, res = event_ms(lambda: powerflow.dc_optimal_power_flow(bu, li, ge, cost=cost, rating=rating, slack_bus=slack))
        it = res.iterations.cpu().numpy()
        conv = res.converged.cpu().numpy()
        q = np.percentile(it, [0, 25, 50, 75, 100]).astype(int).tolist()
        sec, solver, objs = cpu_seconds_per_grid(bu, li, ge, cost, rating, slack, quad)
        dev_obj = res.objective[:objs.size].cpu().numpy()
        rel = np.nanmax(np.abs(dev_obj - objs) / np.maximum(1.0, np.abs(objs))) if np.isfinite(objs).any() else float('nan')
        print(f"case{case} x {bt} {'QP' if quad else 'LP'} (E {E}, Gn {Gn}, every line rated): median {np.median(ms):.3f} ms "
              f"(min {ms.min():.3f}, max {ms.max():.3f}) = {np.median(ms) * 1e3 / bt:.1f} us per grid; converged {int(conv.sum())} of {bt}; "
              f"iterations min / quartiles / max {q}; one CPU core, {solver}, first {objs.size} grids: {sec * 1e3:.1f} ms per grid "
              f"({sec * 1e3 / (np.median(ms) / bt):.0f}x the device's time per grid); objective device vs CPU, worst relative "
              f"difference {rel:.1e}", flush=True)
