"""Times ``powerflow.dc_security_constrained_opf`` and ``powerflow.dc_secure_dispatch``: the whole Python call between HIP events, the
median of 5 repeats after 2 warm-ups, next to ``powerflow.dc_optimal_power_flow`` on the same problems in the same run.  Row lists
of R slots: every slot empty (the cost of the extra launches and of the rows' branches alone), 32 and 256 rows drawn from the pairs
(monitored line, outaged line that is not a bridge), one list for the batch.  The share of the row terms is what the call with R
rows takes beyond the call with the same R empty slots.  The driver runs ``rounds=4`` of 8 rows.

The problems follow ``tools/gpu_time_dcopf.py``'s recipe (a dispatch p0 that meets the demand, bounds around it, every line rated
max(1.05 |flow(p0)|, 0.02), distinct quadratic costs) with the contingency rating max(1.05 max_k |post-outage flow(p0)|, 0.02) from
``dc_contingency_screen`` at p0, so that p0 is feasible for every row.
usage: python tools/gpu_time_dcscopf.py [case:batch ...] > profiles/dcscopf/gpu_time.txt"""
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


def problem(case, bt, seed=1):
    """(buses, lines, gens, cost [Bt,Gn,2], rating [Bt,E], contingency rating [Bt,E], slack, the lines that are not bridges)."""
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=seed, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(seed + 1000 * case + 1)
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
    sc = powerflow.dc_contingency_screen(bu, li, ge, slack_bus=slack, flows=True)
    rating = torch.clamp(1.05 * sc.base.line_flow.abs(), min=0.02)
    post = sc.line_flow[:, ~sc.islanding].abs().amax(dim=1)
    rating_c = torch.clamp(1.05 * post, min=0.02)
    cost = torch.zeros(bt, Gn, 2, dtype=torch.float64, device='cuda')
    cost[:, :, 1] = 10.0 + 30.0 * torch.rand(bt, Gn, generator=g, device='cuda', dtype=torch.float64)
    cost[:, :, 0] = 0.5 + 4.5 * torch.rand(bt, Gn, generator=g, device='cuda', dtype=torch.float64)
    return bu, li, ge, cost, rating, rating_c, slack, torch.nonzero(~sc.islanding).flatten().cpu().numpy()


def row_list(R, n_rows, E, outages, seed):
    """[R,2] int32 on the device: n_rows pairs (l, k), k an outage that is no bridge, l != k, then empty slots."""
    rng = np.random.default_rng(seed)
    rows = np.full((R, 2), -1, dtype=np.int32)
    k = rng.choice(outages, n_rows)
    l = (k + rng.integers(1, E, n_rows)) % E
    rows[:n_rows, 0], rows[:n_rows, 1] = l, k
    return torch.from_numpy(rows).cuda()


def line(what, ms, bt, extra=''):
    print(f'  {what}: median {np.median(ms):.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}) = {np.median(ms) * 1e3 / bt:.1f} us per grid{extra}',
          flush=True)


torch.set_num_threads(1)
specs = sys.argv[1:] or ['14:512', '118:64', '118:4096']
for spec in specs:
    case, bt = map(int, spec.split(':'))
    bu, li, ge, cost, rating, rating_c, slack, outages = problem(case, bt)
    E, Gn = li.shape[1], ge.shape[1]
    print(f'case{case} x {bt} QP (E {E}, Gn {Gn}, every line rated, {outages.size} outages that are no bridge)', flush=True)
    ms0, res = event_ms(lambda: powerflow.dc_optimal_power_flow(bu, li, ge, cost=cost, rating=rating, slack_bus=slack))
    line('dc_optimal_power_flow', ms0, bt, f'; converged {int(res.converged.sum())} of {bt}; median iterations {int(res.iterations.median())}')
    for R in (32, 256):
        t = {}
        for n_rows in (0, R):
            rows = row_list(R, n_rows, E, outages, R)
            ms, res = event_ms(lambda: powerflow.dc_security_constrained_opf(bu, li, ge, cost=cost, rating=rating, rows=rows,
                                                                             contingency_rating=rating_c, slack_bus=slack))
            t[n_rows] = np.median(ms)
            active = int((res.mu_row.abs() > 1e-6).sum())
            line(f'dc_security_constrained_opf R {R}, {n_rows} rows', ms, bt,
                 f'; converged {int(res.converged.sum())} of {bt}; median iterations {int(res.iterations.median())}; '
                 f'rows with a multiplier above 1e-6: {active}; {np.median(ms) / np.median(ms0):.2f}x dc_optimal_power_flow')
        print(f'  share of the row terms at R {R}: {100 * (t[R] - t[0]) / t[R]:.1f} % of the call', flush=True)
    ms, out = event_ms(lambda: powerflow.dc_secure_dispatch(bu, li, ge, cost=cost, rating=rating, contingency_rating=rating_c, rounds=4,
                                                            slack_bus=slack))
    listed = (out.rows[:, :, 0] >= 0).sum(dim=1)
    line('dc_secure_dispatch rounds 4, 8 rows per round (5 solves, 5 screens)', ms, bt,
         f'; secure {int(out.secure.sum())} of {bt}; rows listed per grid median {int(listed.median())}, max {int(listed.max())}; '
         f'{np.median(ms) / np.median(ms0):.2f}x dc_optimal_power_flow')
