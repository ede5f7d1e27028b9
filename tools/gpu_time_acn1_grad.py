"""Forward + backward of the differentiable AC contingency screen against the route it replaces, on the same (grid, outage) pairs:
``ac_contingency_screen(differentiable=True)`` on Bt grids and every non-islanding outage, and
``newton_raphson(mixed_topologies=True)`` with requires_grad on the expanded batch (each grid once per outage, with that line's row
deleted, warm-started from the base solution), autograd summing over the copies.  The loss weighs ``v`` and ``theta`` (what both
routes return) on the pairs both converge on.  Each figure is one forward + backward between HIP events, after the caches are warm:
5 repeats after 2 warm-ups, each repeat timed on its own, so the spread is shown next to the mean.  Also: the screen's forward
alone with and without gradients, a loss on the three summaries with ``states=False, flows=False``, the adjoint's workspace, and
the largest difference between the two routes' gradients relative to the project's gradient bar (1e-5 max|ref| + 1e-7 per column
per grid).  Exits non-zero if the routes' gradients differ by more than the bar.
usage: python tools/gpu_time_acn1_grad.py [case:batch ...] > profiles/acn1_grad/gpu_time.txt"""
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
    return f'{ms.mean():.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})'


failed = []
specs = sys.argv[1:] or ['14:512', '118:64', '300:8']
for spec in specs:
    case, bt = (int(x) for x in spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    topo = powerflow.analyse_topology(case, f, t, g, slack)
    outages = np.flatnonzero(~powerflow._bridges(case, f - 1, t - 1))
    K = outages.size
    print(f"case{case} x {bt} grids x {K} non-islanding outages of {E} lines = {bt * K} pairs: Jacobian dim {topo.info['dim']} nnz(L+U) "
          f"{topo.info['nnz_lu']}, LDS image {topo.info['lds_bytes']} B per wave", flush=True)
    plain = powerflow.ac_contingency_screen(bu, li, ge, slack_bus=slack, outages=outages)
    keep = torch.tensor(np.array([np.delete(np.arange(E), k) for k in outages]), device='cuda')           # [K, E-1]
    xv = plain.base.v.repeat_interleave(K, dim=0).contiguous()
    xth = plain.base.theta.repeat_interleave(K, dim=0).contiguous()
    gen = torch.Generator().manual_seed(case)
    wv, wth = (torch.randn(bt, K, case, generator=gen, dtype=torch.float64).cuda() for _ in range(2))
    ws = torch.randn(3, bt, K, generator=gen, dtype=torch.float64).cuda()

    def inputs():
        return [x.detach().clone().requires_grad_(True) for x in (bu, li, ge)]

    def expanded_forward(ins):
        xl = ins[1][:, keep].reshape(bt * K, E - 1, 7)
        xb, xg = ins[0].repeat_interleave(K, dim=0), ins[2].repeat_interleave(K, dim=0)
        return powerflow.newton_raphson(xb, xl, xg, slack_bus=slack, mixed_topologies=True, v0=xv, theta0=xth)

    rows = plain.converged & expanded_forward(inputs()).converged.reshape(bt, K)

    def expanded():
        ins = inputs()
        r = expanded_forward(ins)
        loss = (wv[rows] * r.v.reshape(bt, K, -1)[rows]).sum() + (wth[rows] * r.theta.reshape(bt, K, -1)[rows]).sum()
        return torch.autograd.grad(loss, ins)

    def screen():
        ins = inputs()
        r = powerflow.ac_contingency_screen(*ins, slack_bus=slack, outages=outages, flows=False, differentiable=True)
        return torch.autograd.grad((wv[rows] * r.v[rows]).sum() + (wth[rows] * r.theta[rows]).sum(), ins)

    def screen_summaries():
        ins = inputs()
        r = powerflow.ac_contingency_screen(*ins, slack_bus=slack, outages=outages, flows=False, states=False, differentiable=True)
        loss = (ws[0][rows] * r.worst_loading[rows]).sum() + (ws[1][rows] * r.v_min[rows]).sum() + (ws[2][rows] * r.v_max[rows]).sum()
        return torch.autograd.grad(loss, ins)

    ms_x, want = event_ms(expanded)
    ms_s, got = event_ms(screen)
    ms_sum, _ = event_ms(screen_summaries)
    ms_f, _ = event_ms(lambda: powerflow.ac_contingency_screen(bu, li, ge, slack_bus=slack, outages=outages, flows=False))
    ms_fd, _ = event_ms(lambda: powerflow.ac_contingency_screen(*inputs(), slack_bus=slack, outages=outages, flows=False,
                                                                differentiable=True))
    worst = 0.0
    for a, b, cols in zip(got, want, CONTRACT):
        for c in cols:
            err = (a[..., c].double() - b[..., c].double()).abs().amax(dim=1)
            bar = 1e-5 * b[..., c].double().abs().amax(dim=1) + 1e-7
            worst = max(worst, float((err / bar).max()))
    need = ctypes.c_size_t()
    cfg = PfConfig(case, E, g.size, 10, 1e-8)
    load_library().gns_acn1_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, bt, K, ctypes.byref(need))
    print(f"  expanded newton_raphson(mixed_topologies=True) forward + backward, {bt * K} grids on {K} topologies: {show(ms_x)}", flush=True)
    print(f"  ac_contingency_screen(differentiable=True) forward + backward, loss on v and theta: {show(ms_s)}", flush=True)
    print(f"  ... states=False flows=False, loss on worst_loading, v_min, v_max: {show(ms_sum)}", flush=True)
    print(f"  the screen's forward alone (flows=False): {show(ms_f)} without gradients, {show(ms_fd)} with", flush=True)
    print(f"  adjoint workspace {need.value / 1e6:.2f} MB; {int(rows.sum())} of {bt * K} pairs in the loss", flush=True)
    print(f"  expanded / screen: {ms_x.mean() / ms_s.mean():.2f}x forward + backward; largest gradient difference between the routes: "
          f"{worst:.3f} of the bar", flush=True)
    if worst > 1.0:
        failed.append(f'case{case}: the routes\' gradients differ by {worst:.3f} of the bar')
for msg in failed:
    print('FAILED: ' + msg, flush=True)
sys.exit(1 if failed else 0)
