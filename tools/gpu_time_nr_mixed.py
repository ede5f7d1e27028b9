"""Newton-Raphson power flow on batches that mix topologies (newton_raphson(..., mixed_topologies=True), gns_pf_solve_set) on
case118 x 16384: HIP events around the kernel's launch through the C-ABI (plan prepared; mean of 5 after 2 warm-ups) and around
the whole newton_raphson call, for
  1. one topology (solvable_grids; the plain gns_pf_solve and the set path on the same grids)
  2. 128 non-islanding outages x 128 grids each (round-robin), sorted order
  3. every non-islanding outage (166), shuffled, sorted order
  4. row 3 with order = NULL (workgroups take the grids in input order)
plus the host wall time of a first mixed call (classification, one analysis per topology, blob upload) and of a repeat call, and
mean iterations / converged counts.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_time_nr_mixed.py` for the
kernel statistics.
usage: python tools/gpu_time_nr_mixed.py [batch]"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig


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


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def set_launcher(bu, li, ge, plan, use_order):
    """A closure that launches gns_pf_solve_set alone (outputs and workspace allocated once)."""
    lib = amd.load_library()
    Bt, N = bu.shape[0], bu.shape[1]
    cfg = PfConfig(N, li.shape[1], ge.shape[1], 10, 1e-8)
    ts, members = plan.topo_set, plan.member_off
    need = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.words, members.ctypes.data, members.size, Bt,
                                          ctypes.byref(need)) == 0
    ws = gns_mod._workspace(need.value, bu.device)
    out = powerflow._outputs(Bt, N, bu.device)
    order = plan.order.data_ptr() if use_order else None
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        rc = lib.gns_pf_solve_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.blob.data_ptr(), ts.words, members.ctypes.data,
                                  members.size, plan.grid_off.data_ptr(), order, bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt,
                                  None, None, *(t.data_ptr() for t in out), ws.data_ptr(), ws.numel(), stream)
        assert rc == 0, rc
        return out
    return run


def plain_launcher(bu, li, ge, slack):
    lib = amd.load_library()
    Bt, N = bu.shape[0], bu.shape[1]
    cfg = PfConfig(N, li.shape[1], ge.shape[1], 10, 1e-8)
    topo = powerflow._topology(bu, li, ge, slack)
    need = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
    ws = gns_mod._workspace(need.value, bu.device)
    out = powerflow._outputs(Bt, N, bu.device)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        rc = lib.gns_pf_solve(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                              ge.data_ptr(), Bt, None, None, *(t.data_ptr() for t in out), ws.data_ptr(), ws.numel(), stream)
        assert rc == 0, rc
        return out
    return run


def stats(out, Bt):
    conv, it = out[2].bool(), out[3]
    solved = it >= 0
    return (f"converged {int(conv.sum())}/{Bt}, not solved (islanded) {int((~solved).sum())}, mean iterations "
            f"{it[solved].double().mean():.2f}")


bt = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
e = synth.CASE_SHAPES[118][1]
f_bus, t_bus, _ = synth.case_topology(118)
slack = synth.solvable_grids(118, 1)[3]
ok = [j for j in range(e) if not powerflow._islanded(118, (np.delete(f_bus, j) - 1).astype(np.int64),
                                                      (np.delete(t_bus, j) - 1).astype(np.int64), slack - 1).size]
print(f"# case118 x {bt}; {len(ok)} non-islanding outages of {e}; HIP events, mean of 5 after 2 warm-ups", flush=True)

bu, li, ge, slack, _, _ = synth.solvable_grids(118, bt, seed=1, device='cuda')
k_ms, out = event_ms(plain_launcher(bu, li, ge, slack))
c_ms, _ = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack))
plan = powerflow._plan_mixed(bu, li, ge, slack)
s_ms, sout = event_ms(set_launcher(bu, li, ge, plan, True))
m_ms, _ = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack, mixed_topologies=True))
same = all(torch.equal(a, b) for a, b in zip(out, sout))
print(f"1. one topology: gns_pf_solve kernel {k_ms:.3f} ms, newton_raphson call {c_ms:.3f} ms | gns_pf_solve_set kernel "
      f"{s_ms:.3f} ms, mixed call {m_ms:.3f} ms | outputs bit-identical {same} | {stats(out, bt)}", flush=True)
base = k_ms

rows = [('2. 128 outages x 128 grids, sorted order', ok[:128], False, True),
        ('3. 166 outages, shuffled, sorted order', ok, True, True),
        ('4. 166 outages, shuffled, order = NULL', ok, True, False)]
for name, outs, shuffle, use_order in rows:
    bu, li, ge, slack, _, _, outage = synth.solvable_contingency_grids(118, bt, outs, seed=1, device='cuda', shuffle=shuffle)
    if use_order:
        # host wall time of a first call (fresh caches: classification, one analysis per topology, blob upload) and a repeat
        saved = powerflow._TOPO_CACHE, powerflow._ISLANDED, powerflow._SET_CACHE
        powerflow._TOPO_CACHE, powerflow._ISLANDED, powerflow._SET_CACHE = {}, set(), {}
        try:
            first_s, _ = wall_s(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack, mixed_topologies=True))
            again_s, _ = wall_s(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack, mixed_topologies=True))
            plan_s, _ = wall_s(lambda: powerflow._plan_mixed(bu, li, ge, slack))
        finally:
            powerflow._TOPO_CACHE, powerflow._ISLANDED, powerflow._SET_CACHE = saved
    plan = powerflow._plan_mixed(bu, li, ge, slack)
    k_ms, out = event_ms(set_launcher(bu, li, ge, plan, use_order))
    line = (f"{name}: gns_pf_solve_set kernel {k_ms:.3f} ms = {k_ms / base:.2f}x one topology | {stats(out, bt)} | "
            f"{len(plan.member_off)} blobs, set {plan.topo_set.words * 4 / 1e6:.2f} MB")
    if use_order:
        c_ms, _ = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack, mixed_topologies=True))
        line += (f" | mixed call {c_ms:.3f} ms | host wall to completion: first call {first_s:.3f} s, repeat call "
                 f"{again_s * 1e3:.2f} ms, repeat plan alone (classification + tables) {plan_s * 1e3:.2f} ms")
    print(line, flush=True)
    if name.startswith('3'):
        ref_out = [t.clone() for t in out]
    if name.startswith('4'):
        print(f"   rows 3 and 4 bit-identical: {all(torch.equal(a, b) for a, b in zip(ref_out, out))}", flush=True)
