"""A direct call of ``gns_dcopf_adjoint`` (include/gns_powerflow.h, "DC optimal power flow: adjoint") for the tests that pin its
kernel: what the closure in ``powerflow._dc_opf`` does (the same analysed topology, the same workspace query, the same argument
order), with the eight forward outputs, ``converged`` and ``iterations`` as tensors the test supplies.  So the kernel can be fed the
float64 reference's optimum (the forward's stopping tolerance then does not enter a comparison at all) and tensors crafted for its
rules and its failure rows."""
import ctypes

import numpy as np
import torch

from opf_graph_neural_solver_amd import load_library, powerflow
from opf_graph_neural_solver_amd._lib import PfConfig

OUTPUTS = ('pg', 'theta', 'line_flow', 'lmp', 'mu_line', 'mu_pmax', 'mu_pmin', 'objective')
GRADS = ('buses', 'gens', 'cost', 'rating')


def stack(results):
    """The eight outputs of a list of per-grid result dicts (``dc_opf_reference.solve``) as float64 numpy ``[Bt, ...]`` arrays."""
    return {k: np.stack([np.asarray(r[k], dtype=np.float64) for r in results]) for k in OUTPUTS}


def adjoint(b, outputs, incoming, converged=None, iterations=None):
    """``gns_dcopf_adjoint`` on the ``dc_opf_cases.Batch`` ``b`` (cost and rating shared or per grid, as the set has them).
    ``outputs``: the eight outputs, ``[Bt, ...]`` numpy float64; ``incoming``: output name -> ``[Bt, ...]`` cotangent (a missing
    name, or None: NULL, which the kernel reads as zero); ``converged`` (default: all 1) and ``iterations`` (default: all 9) per
    grid.  Returns the four gradients as the kernel wrote them, per grid: ``buses`` ``[Bt,N,6]`` and ``gens`` ``[Bt,Gn,7]`` float32,
    ``cost`` ``[Bt,Gn,2]`` and ``rating`` ``[Bt,E]`` float64 (device tensors)."""
    dev = torch.device('cuda')
    lib = load_library()
    buses, lines, gens = b.buses.to(dev).contiguous(), b.lines.to(dev).contiguous(), b.gens.to(dev).contiguous()
    Bt, N, E, Gn = buses.shape[0], buses.shape[1], lines.shape[1], gens.shape[1]
    shapes = dict(pg=(Bt, Gn), theta=(Bt, N), line_flow=(Bt, E), lmp=(Bt, N), mu_line=(Bt, E), mu_pmax=(Bt, Gn), mu_pmin=(Bt, Gn),
                  objective=(Bt,))

    def f64(x, key):        # every tensor the kernel indexes has exactly the shape it indexes
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(dev).contiguous()
        assert tuple(t.shape) == shapes[key] and t.dtype == torch.float64, (key, tuple(t.shape))
        return t

    out = [f64(outputs[k], k) for k in OUTPUTS]
    inc = [None if incoming.get(k) is None else f64(incoming[k], k) for k in OUTPUTS]
    conv = torch.as_tensor(np.ones(Bt) if converged is None else np.asarray(converged)).to(torch.uint8).to(dev).contiguous()
    iters = torch.as_tensor(np.full(Bt, 9) if iterations is None else np.asarray(iterations)).to(torch.int32).to(dev).contiguous()
    assert tuple(conv.shape) == (Bt,) and tuple(iters.shape) == (Bt,)
    cost = b.cost.to(dev).contiguous()
    rating = None if b.rating is None else b.rating.to(dev).contiguous()
    assert cost.dtype == torch.float64 and tuple(cost.shape) in ((Gn, 2), (Bt, Gn, 2))
    assert rating is None or (rating.dtype == torch.float64 and tuple(rating.shape) in ((E,), (Bt, E)))
    cfg = PfConfig(N, E, Gn, 150, 1e-8)
    topo = powerflow._analysed(powerflow._FD, *powerflow._topology_key(buses, lines, gens, b.slack, 'dc_optimal_power_flow'), dev)
    nbytes = ctypes.c_size_t()
    powerflow._check(lib.gns_dcopf_adjoint_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(nbytes)),
                     'gns_dcopf_adjoint_workspace_bytes')
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    gin = [torch.empty_like(buses), torch.empty_like(gens), torch.empty(Bt, Gn, 2, dtype=torch.float64, device=dev),
           torch.empty(Bt, E, dtype=torch.float64, device=dev)]
    ptr = powerflow._ptr
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        powerflow._check(lib.gns_dcopf_adjoint(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), buses.data_ptr(),
                                               lines.data_ptr(), gens.data_ptr(), Bt, cost.data_ptr(), int(cost.dim() == 3), ptr(rating),
                                               int(rating is not None and rating.dim() == 2), *map(ptr, out), conv.data_ptr(),
                                               iters.data_ptr(), *map(ptr, inc), *map(ptr, gin), ws.data_ptr(), ws.numel(), stream),
                         'gns_dcopf_adjoint')
    torch.cuda.synchronize()
    return dict(zip(GRADS, gin))
