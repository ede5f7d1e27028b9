"""The forward launch of the solved case (``gns_pfs_evaluate``) alone, for the packing measurement: the library this process loads
(``GNS_LIB``: the shipped one, or a ``-DPFS_WAVES=W`` build of ``csrc/gns_pfs.hip`` with W grids per workgroup) is called through
the C entry point on outputs allocated once, 20 launches back to back between device events, so that what is timed is the kernel
and its launch and not the Python side of ``powerflow.solved_case``.  Prints, per shape, the median, minimum and maximum of 7
repeats of that per-launch time after 2 warm-ups.  One library per process: run the variants one after the other, twice.

    for w in 2 4 8; do SRC=gns_pfs KERNEL=gns_pfs_kernel bash tools/build_variant.sh pfs_w$w -DPFS_WAVES=$w; done
    python tools/gpu_time_solved_case_packing.py; GNS_LIB=tools/var_pfs_w4.so python tools/gpu_time_solved_case_packing.py; ...
usage: python tools/gpu_time_solved_case_packing.py [case:batch ...] >> profiles/solved_case/gpu_time_packing.txt"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig

LAUNCHES, REPS, WARM = 20, 7, 2


def main():
    lib = amd.load_library()
    print(f'library: {os.environ.get("GNS_LIB") or "the shipped build (one grid per workgroup)"}', flush=True)
    specs = [a for a in sys.argv[1:] if not a.startswith('--')] or ['14:16384', '118:16384', '300:2048']
    for spec in specs:
        case, bt = map(int, spec.split(':'))
        bu, li, ge, slack, v, th = synth.solvable_grids(case, bt, seed=1, device='cuda')
        bu, li, ge, v, th = bu.contiguous(), li.contiguous(), ge.contiguous(), v.double().contiguous(), th.double().contiguous()
        N, E, Gn = bu.shape[1], li.shape[1], ge.shape[1]
        f, t, g = synth.case_topology(case)
        topo = powerflow.analyse_topology(N, f, t, g, slack, device='cuda')
        cfg = PfConfig(N, E, Gn, 0, 0.0)
        need = ctypes.c_size_t(0)
        assert lib.gns_pfs_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, bt, ctypes.byref(need)) == 0
        out = {k: torch.empty(bt, dict(E=E, N=N, Gn=Gn)[d], dtype=torch.float64, device='cuda') for k, d in powerflow._PFS_ROWS}
        out.update({k: torch.empty(bt, dtype=dt, device='cuda') for k, dt in powerflow._PFS_SCALARS})
        ws = torch.empty(need.value, dtype=torch.uint8, device='cuda')
        stream = torch.cuda.current_stream().cuda_stream
        args = (ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(), ge.data_ptr(), bt,
                v.data_ptr(), th.data_ptr(), None, 0, *(out[k].data_ptr() for k in powerflow._PFS_C_ORDER), ws.data_ptr(), ws.numel(), stream)

        def launches():
            for _ in range(LAUNCHES):
                rc = lib.gns_pfs_evaluate(*args)
                assert rc == 0, rc

        ref = powerflow.solved_case(bu, li, ge, v, th, slack_bus=slack) if not os.environ.get('GNS_LIB') else None
        ms = []
        for rep in range(WARM + REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            launches()
            b.record()
            torch.cuda.synchronize()
            if rep >= WARM:
                ms.append(a.elapsed_time(b) / LAUNCHES)
        ms = np.array(ms)
        checksum = float(out['p_from'].sum() + out['q_inj'].sum() + out['gen_q'].sum() + out['worst_loading'].sum())
        same = '' if ref is None else f'; equals powerflow.solved_case bit for bit: {all(torch.equal(out[k], getattr(ref, k)) for k in out)}'
        print(f'  case{case} x {bt}: {1e3 * np.median(ms):.1f} us per launch (min {1e3 * ms.min():.1f}, max {1e3 * ms.max():.1f}); '
              f'checksum {checksum!r}{same}', flush=True)


if __name__ == '__main__':
    main()
