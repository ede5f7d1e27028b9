"""Forward + backward time of batches that mix topologies (topology_check = 'group') against one topology, case118 x 16384, K=4,
d=20, h=10, three phi nets (the benchmark's model).  Inputs:
  uniform      one topology (today's path)
  128x128      128 N-1 variants x 128 grids: every 64-grid group full
  186x88       all 186 N-1 variants x ~88 grids: every variant's second group padded (372 groups instead of 256)
Per input: the library's kernel-time hooks (main forward kernel, backward kernel sequence) and the wall time of a whole eager
forward + backward, host-side classification included.  usage: python tools/gpu_time_mixed.py [steps] > profiles/.../mixed.txt"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import opf_graph_neural_solver_amd as amd  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
lib = amd.load_library()
S, K = 16384, 4
torch.manual_seed(0)
m = amd.GNS(20, 10, K, 0.9, True).cuda()
m.topology_check = 'group'
m.flat_grad = True
inputs = {'uniform': amd.synth.synth_grids(118, S, seed=1, device='cuda')}
inputs['128x128'] = amd.synth.contingency_grids(118, S, list(range(128)), seed=1, device='cuda')[:3]
inputs['186x88'] = amd.synth.contingency_grids(118, S, list(range(186)), seed=1, device='cuda')[:3]


def step(bu, li, ge):
    v, th, tot, last = m(bu, li, ge)
    tot.mean().backward()
    m.zero_grad()


base = None
for name, (bu, li, ge) in inputs.items():
    for _ in range(2):
        step(bu, li, ge)
    lib.gns_profile_enable(steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(bu, li, ge)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e3
    a, n = ctypes.c_float(), ctypes.c_int()
    lib.gns_profile_read(0, ctypes.byref(a), ctypes.byref(n))
    f = a.value / max(n.value, 1)
    lib.gns_profile_read(1, ctypes.byref(a), ctypes.byref(n))
    b = a.value / max(n.value, 1)
    lib.gns_profile_enable(0)
    if base is None:
        base = wall
    print(json.dumps(dict(input=name, grids=S, fwd_kernel_ms=round(f, 4), bwd_kernels_ms=round(b, 4), fwd_bwd_wall_ms=round(wall, 4),
                          vs_uniform=round(wall / base, 3))), flush=True)
