"""The power-flow adjoint (gns_pf_adjoint / gns_pf_adjoint_set, the backward of powerflow.newton_raphson) against the solve it
differentiates: HIP events around one kernel launch through the C-ABI (buffers prepared; mean of 5 after 2 warm-ups), for
  case14 x 128, case118 x 16384, case300 x 8192 (solvable_grids): gns_pf_solve, gns_pf_adjoint, their ratio, and the whole
  backward of newton_raphson (autograd.grad of sum(a v + b theta));
  a case118 N-1 set (128 non-islanding outages x 128 grids, shuffled, sorted order): gns_pf_solve_set, gns_pf_adjoint_set.
usage: python tools/gpu_time_nr_grad.py"""
import ctypes
import os
import sys

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
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def launchers(lib, bu, li, ge, slack, plan=None):
    """(solve, adjoint) closures over one batch, the plain entries or with ``plan`` the set entries."""
    Bt, N = bu.shape[0], bu.shape[1]
    cfg = PfConfig(N, li.shape[1], ge.shape[1], 10, 1e-8)
    need = ctypes.c_size_t()
    if plan is None:
        topo = powerflow._topology(bu, li, ge, slack)
        assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
    else:
        ts, m = plan.topo_set, plan.member_off
        assert lib.gns_pf_workspace_bytes_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.words, m.ctypes.data, m.size, Bt,
                                              ctypes.byref(need)) == 0
    ws = gns_mod._workspace(need.value, bu.device)
    out = powerflow._outputs(Bt, N, bu.device)
    g = torch.Generator().manual_seed(0)
    gv, gth = (torch.randn(Bt, N, generator=g, dtype=torch.float64).to(bu.device) for _ in range(2))
    grads = [torch.empty_like(t) for t in (bu, li, ge)]
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [t.data_ptr() for t in out]

    def solve():
        if plan is None:
            rc = lib.gns_pf_solve(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                  ge.data_ptr(), Bt, None, None, *ptrs, ws.data_ptr(), ws.numel(), stream)
        else:
            rc = lib.gns_pf_solve_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.blob.data_ptr(), ts.words, m.ctypes.data, m.size,
                                      plan.grid_off.data_ptr(), plan.order.data_ptr(), bu.data_ptr(), li.data_ptr(), ge.data_ptr(),
                                      Bt, None, None, *ptrs, ws.data_ptr(), ws.numel(), stream)
        assert rc == 0, rc

    def adjoint():
        tail = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), gv.data_ptr(), gth.data_ptr(),
                *(t.data_ptr() for t in grads), ws.data_ptr(), ws.numel(), stream)
        if plan is None:
            rc = lib.gns_pf_adjoint(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                    ge.data_ptr(), Bt, *tail)
        else:
            rc = lib.gns_pf_adjoint_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.blob.data_ptr(), ts.words, m.ctypes.data,
                                        m.size, plan.grid_off.data_ptr(), plan.order.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                        ge.data_ptr(), Bt, *tail)
        assert rc == 0, rc
    return solve, adjoint, out, grads


def backward_call_ms(bu, li, ge, slack, **kw):
    """The whole backward of newton_raphson (the forward outside the events)."""
    ins = [t.clone().requires_grad_(True) for t in (bu, li, ge)]
    a = torch.ones(bu.shape[0], bu.shape[1], dtype=torch.float64, device=bu.device)

    def run():
        res = powerflow.newton_raphson(*ins, slack_bus=slack, **kw)
        loss = (a * res.v + a * res.theta).sum()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        torch.autograd.grad(loss, ins)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)
    for _ in range(2):
        run()
    return float(np.mean([run() for _ in range(5)]))


lib = amd.load_library()
print('# HIP events around one launch through the C-ABI, mean of 5 after 2 warm-ups; backward call = torch.autograd.grad of '
      'sum(v + theta) through newton_raphson', flush=True)
for case, bt in ((14, 128), (118, 16384), (300, 8192)):
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    solve, adjoint, out, grads = launchers(lib, bu, li, ge, slack)
    s_ms = event_ms(solve)
    a_ms = event_ms(adjoint)
    info = powerflow._topology(bu, li, ge, slack).info
    nan_rows = int(grads[0].isnan().flatten(1).any(1).sum())
    b_ms = backward_call_ms(bu, li, ge, slack)
    print(f"case{case} x {bt}: gns_pf_solve {s_ms:.3f} ms (mean iterations {out[3].double().mean():.2f}), gns_pf_adjoint "
          f"{a_ms:.3f} ms = {a_ms / s_ms:.2f}x the solve | backward call {b_ms:.3f} ms | NaN rows {nan_rows} (not converged "
          f"{int((out[2] == 0).sum())}) | steps: solve {info['n_steps']} per iteration, adjoint {info['n_factor_steps']} factor + "
          f"{info['n_adj_steps']} transposed", flush=True)

e = synth.CASE_SHAPES[118][1]
f_bus, t_bus, _ = synth.case_topology(118)
slack = synth.solvable_grids(118, 1)[3]
ok = [j for j in range(e) if not powerflow._islanded(118, (np.delete(f_bus, j) - 1).astype(np.int64),
                                                      (np.delete(t_bus, j) - 1).astype(np.int64), slack - 1).size]
bu, li, ge, slack, _, _, _ = synth.solvable_contingency_grids(118, 16384, ok[:128], seed=1, device='cuda', shuffle=True)
plan = powerflow._plan_mixed(bu, li, ge, slack)
solve, adjoint, out, grads = launchers(lib, bu, li, ge, slack, plan)
s_ms = event_ms(solve)
a_ms = event_ms(adjoint)
b_ms = backward_call_ms(bu, li, ge, slack, mixed_topologies=True)
print(f"case118 N-1 set x 16384 (128 outages, shuffled, sorted order): gns_pf_solve_set {s_ms:.3f} ms, gns_pf_adjoint_set "
      f"{a_ms:.3f} ms = {a_ms / s_ms:.2f}x | backward call {b_ms:.3f} ms | NaN rows {int(grads[0].isnan().flatten(1).any(1).sum())}",
      flush=True)
