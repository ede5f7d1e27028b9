"""DC power flow against fast-decoupled XB and Newton-Raphson on the same solvable_grids batches: each solver's time per call (HIP
events around the calls, mean of 5 after 2 warm-ups), the LDS images, DC's and NR's angle error against the grids' true solution,
DC's adjoint call; then a one-core CPU time per grid of the test reference (tests/dc_reference.py) on a sample.
usage: python tools/gpu_time_dc.py [case:batch ...] > profiles/dc/gpu_time_dc.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

from opf_graph_neural_solver_amd import powerflow, synth


def event_ms(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


specs = sys.argv[1:] or ['14:128', '118:16384', '300:8192']
for spec in specs:
    case, bt = (int(x) for x in spec.split(':'))
    bu, li, ge, slack, v, th = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    nr_i = powerflow.analyse_topology(case, f, t, g, slack).info
    fd = powerflow.analyse_fd_topology(case, f, t, g, slack)
    print(f"case{case} x {bt}: B' dim {fd.info['dim_p']} nnz(L+U) {fd.info['nnz_lu_p']} factor steps {fd.info['factor_p_steps']} "
          f"({fd.info['factor_p_ops']} ops) solve steps {fd.info['solve_p_steps']} ({fd.info['solve_p_ops']} ops); LDS DC "
          f"{powerflow._dc_lds_bytes(fd.host)} B, FD {fd.info['lds_bytes']} B, NR {nr_i['lds_bytes']} B", flush=True)
    runs = [('DC', lambda: powerflow.dc_power_flow(bu, li, ge, slack_bus=slack)),
            ('XB', lambda: powerflow.fast_decoupled(bu, li, ge, slack_bus=slack, variant='XB')),
            ('NR', lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack))]
    ms = {}
    for name, fn in runs:
        ms[name], res = event_ms(fn)
        ok = res.converged
        err = float((res.theta[ok] - th[ok]).abs().max()) if bool(ok.any()) else float('nan')
        print(f"  {name}: {ms[name]:.3f} ms (call, HIP events), solved {int(ok.sum())}/{bt}, max|theta - theta_true| on solved {err:.2e} rad",
              flush=True)
    print(f"  DC / XB call time: {ms['DC'] / ms['XB']:.3f}", flush=True)
    ins = [x.clone().requires_grad_(True) for x in (bu, li, ge)]
    res = powerflow.dc_power_flow(*ins, slack_bus=slack)
    loss = res.theta.sum() + res.line_flow.sum() + res.slack_p.sum()
    back, _ = event_ms(lambda: torch.autograd.grad(loss, ins, retain_graph=True))
    print(f"  DC adjoint: {back:.3f} ms (backward of one call: gns_dc_adjoint and autograd's bookkeeping)", flush=True)

import dc_reference as dref
torch.set_num_threads(1)
for case, sample in ((14, 32), (118, 8), (300, 4)):
    bu, li, ge, slack, v, th = synth.solvable_grids(case, sample, seed=1)
    t0 = time.perf_counter()
    for k in range(sample):
        dref.dc_power_flow(bu[k], li[k], ge[k], slack)
    dt = (time.perf_counter() - t0) / sample
    print(f"CPU reference case{case} DC (dense float64, one core): {dt * 1e3:.2f} ms per grid over {sample} grids", flush=True)
