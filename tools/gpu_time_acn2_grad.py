"""Forward + backward of the differentiable AC N-2 screen against the route it replaces, on the same (grid, pair) rows:
``ac_n2_contingency_screen_differentiable`` with ``flows=False, states=False`` and the loss ``worst_loading[converged].sum()`` on Bt
grids and a pair list, and ``newton_raphson(mixed_topologies=True)`` with requires_grad on the expanded batch (each grid once per
non-islanding pair of the list, with both line rows deleted, warm-started from the base solution, every analysis cached), autograd
summing over the copies.  That route returns ``v`` and ``theta`` alone, so its loss weighs those on the rows both routes converge
on: the cheapest loss it can have (the worst loading would need the flows of every copy on top).  The screen is timed with that
loss too (``states=True``), and there the two routes' gradients are compared against the project's gradient bar (1e-5 max|ref| +
1e-7 per column per grid); the tool exits non-zero if they differ by more.
Each figure is one forward + backward between HIP events, after the caches are warm: 10 repeats after 3 warm-ups, the routes
alternating within a repeat, each repeat timed on its own; the median is quoted with the spread.  Also: the screen's forward alone
with and without gradients, the adjoint's workspace and the rows per wave.  The shapes are those of tools/gpu_time_acn2.py.
usage: python tools/gpu_time_acn2_grad.py [--no-expanded] [case:batch:pairs ...] > profiles/acn2_grad/gpu_time.txt   (pairs 0: every pair)"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig, load_library

CONTRACT = ((2, 3, 4, 5), (2, 3, 4, 5, 6), (4, 6))
TOL, MAX_IT = 1e-8, 10


def event_ms(fns, reps=10, warm=3):
    """Milliseconds [len(fns), reps] and the last outputs: within a repeat the functions run one after the other (alternating)."""
    out = [None] * len(fns)
    for _ in range(warm):
        out = [fn() for fn in fns]
    ms = np.zeros((len(fns), reps))
    for r in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            out[k] = fn()
            b.record()
            torch.cuda.synchronize()
            ms[k, r] = a.elapsed_time(b)
    return ms, out


def show(ms):
    return f'{np.median(ms):.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})'


failed = []
args = sys.argv[1:]
with_expanded = '--no-expanded' not in args
specs = [a for a in args if not a.startswith('--')] or ['14:512:0', '118:64:512', '300:8:256']
for spec in specs:
    case, bt, n_pairs = map(int, spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    topo = powerflow.analyse_topology(case, f, t, g, slack, device=bu.device)
    every = powerflow._pair_list(None, E)
    rng = np.random.default_rng(case)
    pairs = every if n_pairs <= 0 or n_pairs >= every.shape[0] else every[np.sort(rng.choice(every.shape[0], n_pairs, replace=False))]
    P = pairs.shape[0]
    isl = powerflow._pair_islanding(case, f - 1, t - 1, pairs)
    need = ctypes.c_size_t()
    cfg = PfConfig(case, E, g.size, MAX_IT, TOL)
    powerflow._check(load_library().gns_acn2_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, bt, P, ctypes.byref(need)),
                     'gns_acn2_adjoint_workspace_bytes')
    np_doubles = 4 * case + 5 * E + g.size + 1
    chunks = (need.value - (bt * 16 * topo.info['nnz_ybus'] + 255) // 256 * 256) // (8 * np_doubles * bt)      # the partials per grid
    print(f"case{case} x {bt} grids x {P} pairs ({int(isl.sum())} islanding) of {E} lines = {bt * P} rows: dim {topo.info['dim']} "
          f"nnz(L+U) {topo.info['nnz_lu']}, LDS {topo.info['lds_bytes']} B per wave; adjoint: {chunks} chunks per grid of up to "
          f"{-(-P // chunks)} rows, workspace {need.value / 1e6:.2f} MB", flush=True)

    def inputs():
        return [x.detach().clone().requires_grad_(True) for x in (bu, li, ge)]

    def screen(ins, **kw):
        return powerflow.ac_n2_contingency_screen_differentiable(*ins, slack_bus=slack, pairs=pairs, tol=TOL, max_iter=MAX_IT, **kw)

    plain = powerflow.ac_n2_contingency_screen(bu, li, ge, slack_bus=slack, pairs=pairs, tol=TOL, max_iter=MAX_IT)
    live = torch.from_numpy(np.flatnonzero(~isl)).cuda()
    S = live.numel()
    gen = torch.Generator().manual_seed(case)
    wv, wth = (torch.randn(bt, S, case, generator=gen, dtype=torch.float64).cuda() for _ in range(2))

    def summaries():
        ins = inputs()
        r = screen(ins)
        return torch.autograd.grad(r.worst_loading[r.converged].sum(), ins)

    fns = [summaries, lambda: powerflow.ac_n2_contingency_screen(bu, li, ge, slack_bus=slack, pairs=pairs, tol=TOL, max_iter=MAX_IT),
           lambda: screen(inputs())]
    if with_expanded:
        keep = torch.tensor(np.array([np.delete(np.arange(E), pairs[p]) for p in live.tolist()]), device='cuda')     # [S, E-2]
        xv = plain.base.v.repeat_interleave(S, dim=0).contiguous()
        xth = plain.base.theta.repeat_interleave(S, dim=0).contiguous()

        def expanded_forward(ins):
            xl = ins[1][:, keep].reshape(bt * S, E - 2, 7)
            xb, xg = ins[0].repeat_interleave(S, dim=0), ins[2].repeat_interleave(S, dim=0)
            return powerflow.newton_raphson(xb, xl, xg, slack_bus=slack, mixed_topologies=True, v0=xv, theta0=xth, tol=TOL,
                                            max_iter=MAX_IT)

        rows = plain.converged[:, live] & expanded_forward(inputs()).converged.reshape(bt, S)

        def expanded():
            ins = inputs()
            r = expanded_forward(ins)
            loss = (wv[rows] * r.v.reshape(bt, S, -1)[rows]).sum() + (wth[rows] * r.theta.reshape(bt, S, -1)[rows]).sum()
            return torch.autograd.grad(loss, ins)

        def states():
            ins = inputs()
            r = screen(ins, states=True)
            return torch.autograd.grad((wv[rows] * r.v[:, live][rows]).sum() + (wth[rows] * r.theta[:, live][rows]).sum(), ins)

        fns += [expanded, states]
    ms, out = event_ms(fns)
    n_conv = int(plain.converged.sum())
    print(f"  ac_n2_contingency_screen_differentiable flows=False states=False, forward + backward of worst_loading[converged].sum() "
          f"({n_conv} of {bt * S} non-islanding rows): {show(ms[0])}", flush=True)
    print(f"  the screen's forward alone (flows=False, states=False): {show(ms[1])} without gradients, {show(ms[2])} with (v and theta "
          f"kept for the backward, {16 * bt * P * case / 1e6:.1f} MB)", flush=True)
    if with_expanded:
        worst = 0.0
        for a, b, cols in zip(out[4], out[3], CONTRACT):
            for c in cols:
                err = (a[..., c].double() - b[..., c].double()).abs().amax(dim=1)
                bar = 1e-5 * b[..., c].double().abs().amax(dim=1) + 1e-7
                worst = max(worst, float((err / bar).max()))
        print(f"  expanded newton_raphson(mixed_topologies=True) forward + backward, {bt * S} grids on {S} topologies, loss on v and theta "
              f"of {int(rows.sum())} rows: {show(ms[3])}", flush=True)
        print(f"  the screen with states=True, forward + backward of the same loss: {show(ms[4])}", flush=True)
        print(f"  expanded / screen: {np.median(ms[3]) / np.median(ms[0]):.2f}x against the summaries' loss, "
              f"{np.median(ms[3]) / np.median(ms[4]):.2f}x on the same loss; largest gradient difference between the routes: "
              f"{worst:.3f} of the bar", flush=True)
        if worst > 1.0:
            failed.append(f'case{case}: the routes\' gradients differ by {worst:.3f} of the bar')
for msg in failed:
    print('FAILED: ' + msg, flush=True)
sys.exit(1 if failed else 0)
