"""Fast-decoupled (XB, BX) against Newton-Raphson power flow on solvable_grids batches: each solver's kernel time (HIP events around
one call, mean of 5 after 2 warm-ups), converged counts, mean iterations, the program step counts and LDS images of both
analyses; then a one-core CPU time per grid of the test oracles (tests/fd_reference.py, tests/nr_reference.py) on a sample.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_time_fd.py` for the kernel statistics.
usage: python tools/gpu_time_fd.py [case:batch ...]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
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
    fd_i = powerflow.analyse_fd_topology(case, f, t, g, slack).info
    print(f"case{case} x {bt}: NR dim {nr_i['dim']} nnz(L+U) {nr_i['nnz_lu']} steps/iteration {nr_i['n_steps']} "
          f"LDS {nr_i['lds_bytes']} B | FD B' dim {fd_i['dim_p']} nnz(L+U) {fd_i['nnz_lu_p']} factor steps {fd_i['factor_p_steps']} "
          f"solve steps {fd_i['solve_p_steps']} ({fd_i['solve_p_ops']} ops); B'' dim {fd_i['dim_pp']} nnz(L+U) {fd_i['nnz_lu_pp']} "
          f"factor steps {fd_i['factor_pp_steps']} solve steps {fd_i['solve_pp_steps']} ({fd_i['solve_pp_ops']} ops); "
          f"LDS {fd_i['lds_bytes']} B", flush=True)
    runs = [('NR', lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack))]
    runs += [(var, lambda var=var: powerflow.fast_decoupled(bu, li, ge, slack_bus=slack, variant=var)) for var in ('XB', 'BX')]
    for name, fn in runs:
        ms, res = event_ms(fn)
        ok = res.converged
        err = float((res.v[ok] - v[ok]).abs().max()) if bool(ok.any()) else float('nan')
        print(f"  {name}: {ms:.3f} ms (call, HIP events), converged {int(ok.sum())}/{bt}, mean iterations "
              f"{res.iterations.double().mean():.2f} (converged grids {res.iterations[ok].double().mean():.2f}), "
              f"max|v - v_true| on converged {err:.1e}", flush=True)

import fd_reference as fref
import nr_reference as ref
for case, sample in ((14, 32), (118, 8), (300, 4)):
    bu, li, ge, slack, v, th = synth.solvable_grids(case, sample, seed=1)
    for name, fn in (('NR', lambda k: ref.newton_raphson(bu[k], li[k], ge[k], slack)),
                     ('XB', lambda k: fref.fast_decoupled(bu[k], li[k], ge[k], slack, 'XB')),
                     ('BX', lambda k: fref.fast_decoupled(bu[k], li[k], ge[k], slack, 'BX'))):
        t0 = time.perf_counter()
        out = [fn(k) for k in range(sample)]
        dt = (time.perf_counter() - t0) / sample
        print(f"CPU oracle case{case} {name} (one core): {dt * 1e3:.2f} ms per grid over {sample} grids, converged "
              f"{sum(o[2] for o in out)}/{sample}, mean iterations {np.mean([o[3] for o in out]):.2f}", flush=True)
