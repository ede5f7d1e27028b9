"""Backward time with and without input gradients (gns_backward vs gns_backward_inputs), through the library's own HIP-event hooks:
the backward kernels' ms and the whole forward + backward loop.  usage: python tools/gpu_time_igrad.py [case:batch[:K] ...]"""
import sys, os, time, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import opf_graph_neural_solver_amd as amd
lib = amd.load_library()
specs = sys.argv[1:] or ['118:16384', '14:128']
for spec in specs:
    parts = [int(x) for x in spec.split(':')]
    case, bt, K = parts[0], parts[1], (parts[2] if len(parts) > 2 else 4)
    m = amd.GNS(20, 10, K, 0.9, True).cuda(); m.topology_check = 'first'
    bu, li, ge = amd.synth.synth_grids(case, bt, seed=1, device='cuda')
    for label, inputs in (('params only', False), ('params + inputs', True)):
        x = [t.clone().requires_grad_(inputs) for t in (bu, li, ge)]
        def step():
            out = m(*x); out[2].mean().backward(); m.zero_grad()
            for t in x: t.grad = None
        for _ in range(2): step()
        lib.gns_profile_enable(16)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(10): step()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        a, n = ctypes.c_float(), ctypes.c_int()
        lib.gns_profile_read(0, ctypes.byref(a), ctypes.byref(n)); f = a.value / max(n.value, 1)
        lib.gns_profile_read(1, ctypes.byref(a), ctypes.byref(n)); b = a.value / max(n.value, 1)
        lib.gns_profile_enable(0)
        print(f"case{case} x {bt} K={K} {label:16s}: fwd {f:.3f} ms   bwd {b:.3f} ms   fwd+bwd loop {(t1 - t0) / 10 * 1e3:.3f} ms", flush=True)
