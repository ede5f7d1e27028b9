"""Newton-Raphson power flow on solvable_grids batches: the NR kernel's time (HIP events around gns_pf_solve's launch, mean of
5 after 2 warm-ups), mean iterations, the GNS forward on the same grids (K=4, d=20, h=10, multi-phi) and NR warm-started from
that GNS prediction; then a one-core CPU baseline, the test-side scipy NR (tests/nr_reference.py) per grid on a sample.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_time_nr.py` for the kernel statistics.
usage: python tools/gpu_time_nr.py [case:batch ...]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch

import opf_graph_neural_solver_amd as amd
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
    t0 = time.perf_counter()
    bu, li, ge, slack, v, th = synth.solvable_grids(case, bt, seed=1, device='cuda')
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t0
    topo = powerflow._topology(bu, li, ge, slack)
    nr_ms, res = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack))
    model = amd.GNS(20, 10, 4, 0.9, True).cuda()
    model.topology_check = 'first'
    with torch.no_grad():
        gns_ms, (gv, gth, _, _) = event_ms(lambda: model(bu, li, ge))
    warm_ms, wres = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack, v0=gv, theta0=gth))
    err = float((res.v - v).abs().max())
    i = topo.info
    print(f"case{case} x {bt}: solvable_grids {gen_s:.2f} s | NR {nr_ms:.3f} ms (call, HIP events), converged "
          f"{int(res.converged.sum())}/{bt}, mean iterations {res.iterations.double().mean():.2f}, max|v - v_true| {err:.1e} | "
          f"GNS forward {gns_ms:.3f} ms | NR from GNS prediction {warm_ms:.3f} ms, converged {int(wres.converged.sum())}/{bt}, "
          f"mean iterations {wres.iterations.double().mean():.2f} | dim {i['dim']} nnz(L+U) {i['nnz_lu']} ops {i['n_ops']} "
          f"steps {i['n_steps']} LDS {i['lds_bytes']} B", flush=True)

import nr_reference as ref
for case, sample in ((14, 64), (118, 16), (300, 4)):
    bu, li, ge, slack, v, th = synth.solvable_grids(case, sample, seed=1)
    t0 = time.perf_counter()
    its = [ref.newton_raphson(bu[k], li[k], ge[k], slack)[3] for k in range(sample)]
    dt = (time.perf_counter() - t0) / sample
    print(f"CPU baseline case{case}: scipy NR (tests/nr_reference.py, one core) {dt * 1e3:.2f} ms per grid over {sample} grids, "
          f"mean iterations {sum(its) / sample:.2f}", flush=True)
