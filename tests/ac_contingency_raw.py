"""``gns_acn1_screen``, ``gns_acn2_screen`` and ``gns_acg1_screen`` (include/gns_powerflow.h, "AC contingency screening", "AC N-2
contingency screening" and "AC generator contingency screening") called through ctypes on device tensors, with the base solution,
``base_converged`` and ``islanding`` supplied by the caller as the C contract has it.  ``powerflow.ac_contingency_screen``,
``powerflow.ac_n2_contingency_screen`` and ``powerflow.ac_generator_contingency_screen`` compute those three themselves and apply
``max_iter`` to their base solve too, so zero or one Newton step of a row, a base angle that is not 0 at the slack and caller-owned
flags are reachable only from here; so are device copies of the generator screen's lists that differ from the host's."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow
from opf_graph_neural_solver_amd._lib import PfConfig

ROWS = ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus',
        'converged', 'iterations', 'mismatch')
Rows = namedtuple('Rows', ROWS)
_TOPO = {}


def analysed(tp, device):
    """The Newton-Raphson analysis of ``tp`` (from its own id arrays, never from a grid's id columns), made once per name."""
    key = (tp.name, str(device))
    if key not in _TOPO:
        _TOPO[key] = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack, device=device)
    return _TOPO[key]


def screen(tp, buses, lines, gens, outages, base_v, base_theta, base_converged, islanding, rating, max_iter, tol):
    """One ``gns_acn1_screen`` launch on the current stream: ``buses`` [Bt,N,6], ``lines`` [Bt,E,7], ``gens`` [Bt,Gn,7] float32 on
    the device, ``outages`` and ``islanding`` sequences [K], ``base_v``, ``base_theta`` [Bt,N], ``base_converged`` [Bt], ``rating``
    None, [E] or [Bt,E].  Returns ``Rows``: the fifteen outputs ([Bt,K,...], ``converged`` as bool), every one pre-filled with a
    sentinel that no row may keep."""
    out32 = np.ascontiguousarray(np.asarray(outages, dtype=np.int32).reshape(-1))
    return _call('gns_acn1', tp, buses, lines, gens, out32, out32.size, base_v, base_theta, base_converged, islanding, rating,
                 max_iter, tol)


def screen_pairs(tp, buses, lines, gens, pairs, base_v, base_theta, base_converged, islanding, rating, max_iter, tol):
    """One ``gns_acn2_screen`` launch: ``screen`` with ``pairs`` [P,2] (either order within a pair; passed as int32 [2P] on host and
    device) in the place of ``outages`` and ``islanding`` [P].  Returns ``Rows`` [Bt,P,...]."""
    p32 = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    return _call('gns_acn2', tp, buses, lines, gens, p32.reshape(-1), p32.shape[0], base_v, base_theta, base_converged, islanding,
                 rating, max_iter, tol)


GeneratorSet = namedtuple('GeneratorSet', ['host', 'member_off', 'gen_list', 'row_cols', 'extra_off'])


def analysed_without(tp, g, device=None):
    """The Newton-Raphson analysis of ``tp`` without generator row ``g``, made once per (name, row)."""
    key = (tp.name, str(device), int(g))
    if key not in _TOPO:
        _TOPO[key] = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack, device=device, out_gen=int(g))
    return _TOPO[key]


def generator_set(tp, rows, extra=()):
    """What ``gns_acg1_screen`` takes for the rows ``[(g, k)]``, built as the wrapper builds it: one analysis without the generator
    per distinct generator of the list, ascending, in the set layout (member m at the 16-word aligned ``member_off[m]``),
    ``gen_list`` and ``row_cols`` (position into ``gen_list``, line or -1), all int32 on the host.  The host blobs of ``extra`` are
    laid out after the members, at ``extra_off``: words of the set that no list names."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    gen_list, col = np.unique(r[:, 0], return_inverse=True)
    blobs = [analysed_without(tp, g).host for g in gen_list.tolist()] + list(extra)
    off, words = [], 0
    for w in blobs:
        off.append(words)
        words += (w.size + 15) // 16 * 16
    host = np.zeros(words, dtype=np.int32)
    for o, w in zip(off, blobs):
        host[o:o + w.size] = w
    cols = np.ascontiguousarray(np.stack([col.reshape(-1), r[:, 1]], axis=1), dtype=np.int32)
    n = gen_list.size
    return GeneratorSet(host, np.asarray(off[:n], dtype=np.int32), gen_list.astype(np.int32), cols, np.asarray(off[n:], dtype=np.int32))


def screen_generators(tp, buses, lines, gens, rows, base_v, base_theta, base_converged, islanding, rating, pickup, max_iter, tol,
                      tamper=None, extra=()):
    """One ``gns_acg1_workspace_bytes`` call and one ``gns_acg1_screen`` launch on the current stream: ``screen`` with ``rows``
    ``[(g, k)]`` (k = -1: no line out) and ``islanding`` [P] in the place of ``outages``, and ``pickup`` None, [Gn] or [Bt,Gn] float64.
    The set is ``generator_set(tp, rows, extra)``.  ``tamper``: {'member_off' | 'gen_list' | 'row_cols': int32 array} replaces the
    DEVICE copy of that list alone; the host copies stay the valid ones, so the host checks pass and the kernel's own decide.
    Returns ``Rows`` [Bt,P,...]."""
    lib = amd.load_library()
    dev = buses.device
    Bt, N, E, Gn = buses.shape[0], tp.n, tp.f.size, tp.g.size
    assert buses.shape == (Bt, N, 6) and lines.shape == (Bt, E, 7) and gens.shape == (Bt, Gn, 7)
    buses, lines, gens = (t.contiguous() for t in (buses, lines, gens))
    assert buses.dtype == lines.dtype == gens.dtype == torch.float32
    s = generator_set(tp, rows, extra)
    K = s.row_cols.shape[0]
    host_lists = dict(member_off=s.member_off, gen_list=s.gen_list, row_cols=s.row_cols)
    assert set(tamper or {}) <= set(host_lists)
    dev_lists = {}
    for k, a in host_lists.items():
        d = np.ascontiguousarray((tamper or {}).get(k, a), dtype=np.int32)
        assert d.shape == a.shape, k
        dev_lists[k] = torch.from_numpy(d.copy()).to(dev)
    set_dev = torch.from_numpy(s.host).to(dev)
    isl = torch.as_tensor(np.asarray(islanding).astype(np.uint8).reshape(K)).to(dev)
    v0 = torch.as_tensor(base_v, dtype=torch.float64).to(dev).contiguous()
    th0 = torch.as_tensor(base_theta, dtype=torch.float64).to(dev).contiguous()
    conv0 = torch.as_tensor(np.asarray(base_converged).astype(np.uint8).reshape(Bt)).to(dev)
    assert v0.shape == th0.shape == (Bt, N)
    rating_per_grid = pickup_per_grid = 0
    if rating is not None:
        rating = torch.as_tensor(rating, dtype=torch.float64).to(dev).contiguous()
        assert rating.shape in ((E,), (Bt, E))
        rating_per_grid = int(rating.dim() == 2)
    if pickup is not None:
        pickup = torch.as_tensor(pickup, dtype=torch.float64).to(dev).contiguous()
        assert pickup.shape in ((Gn,), (Bt, Gn))
        pickup_per_grid = int(pickup.dim() == 2)
    cfg = PfConfig(N, E, Gn, int(max_iter), float(tol))
    need = ctypes.c_size_t()
    assert lib.gns_acg1_workspace_bytes(ctypes.byref(cfg), s.host.ctypes.data, s.host.size, s.member_off.ctypes.data,
                                        s.member_off.size, Bt, K, ctypes.byref(need)) == 0
    ws = gns_mod._workspace(need.value, dev)
    f64, row_f64, row_i32, conv = _sentinels(Bt, K, N, E, dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.gns_acg1_screen(
            ctypes.byref(cfg), s.host.ctypes.data, set_dev.data_ptr(), s.host.size, s.member_off.ctypes.data,
            dev_lists['member_off'].data_ptr(), s.member_off.size, buses.data_ptr(), lines.data_ptr(), gens.data_ptr(), Bt,
            s.gen_list.ctypes.data, dev_lists['gen_list'].data_ptr(), s.row_cols.ctypes.data, dev_lists['row_cols'].data_ptr(), K,
            isl.data_ptr(), None if rating is None else rating.data_ptr(), rating_per_grid,
            None if pickup is None else pickup.data_ptr(), pickup_per_grid, v0.data_ptr(), th0.data_ptr(), conv0.data_ptr(),
            *(t.data_ptr() for t in f64), row_f64[0].data_ptr(), row_i32[0].data_ptr(), row_f64[1].data_ptr(), row_i32[1].data_ptr(),
            row_f64[2].data_ptr(), row_i32[2].data_ptr(), conv.data_ptr(), row_i32[3].data_ptr(), row_f64[3].data_ptr(), ws.data_ptr(),
            ws.numel(), stream)
        assert rc == 0, rc
        torch.cuda.synchronize(dev)
    return _rows(f64, row_f64, row_i32, conv)


SENTINEL = -12345.0


def _sentinels(Bt, K, N, E, dev):
    """The fifteen outputs, every one pre-filled with a sentinel that no row may keep."""
    f64 = [torch.full((Bt, K, n), SENTINEL, dtype=torch.float64, device=dev) for n in (N, N, E, E, E, E)]
    row_f64 = [torch.full((Bt, K), SENTINEL, dtype=torch.float64, device=dev) for _ in range(4)]        # worst, v_min, v_max, mismatch
    row_i32 = [torch.full((Bt, K), -7, dtype=torch.int32, device=dev) for _ in range(4)]               # their indices, iterations
    return f64, row_f64, row_i32, torch.full((Bt, K), 7, dtype=torch.uint8, device=dev)


def _rows(f64, row_f64, row_i32, conv):
    assert bool((conv <= 1).all()) and bool((row_i32[3] >= -1).all())
    for t in f64 + row_f64:
        assert not bool((t == SENTINEL).any())
    return Rows(*f64, row_f64[0], row_i32[0], row_f64[1], row_i32[1], row_f64[2], row_i32[2], conv.bool(), row_i32[3], row_f64[3])


def _call(prefix, tp, buses, lines, gens, list32, K, base_v, base_theta, base_converged, islanding, rating, max_iter, tol):
    """``<prefix>_workspace_bytes`` and ``<prefix>_screen`` on the ``K`` rows that the int32 array ``list32`` names."""
    lib = amd.load_library()
    dev = buses.device
    Bt, N, E = buses.shape[0], tp.n, tp.f.size
    assert buses.shape == (Bt, N, 6) and lines.shape == (Bt, E, 7) and gens.shape == (Bt, tp.g.size, 7)
    buses, lines, gens = (t.contiguous() for t in (buses, lines, gens))
    assert buses.dtype == lines.dtype == gens.dtype == torch.float32
    topo = analysed(tp, dev)
    list_dev = torch.from_numpy(list32).to(dev)
    isl = torch.as_tensor(np.asarray(islanding).astype(np.uint8).reshape(K)).to(dev)
    v0 = torch.as_tensor(base_v, dtype=torch.float64).to(dev).contiguous()
    th0 = torch.as_tensor(base_theta, dtype=torch.float64).to(dev).contiguous()
    conv0 = torch.as_tensor(np.asarray(base_converged).astype(np.uint8).reshape(Bt)).to(dev)
    assert v0.shape == th0.shape == (Bt, N)
    per_grid = 0
    if rating is not None:
        rating = torch.as_tensor(rating, dtype=torch.float64).to(dev).contiguous()
        assert rating.shape in ((E,), (Bt, E))
        per_grid = int(rating.dim() == 2)
    cfg = PfConfig(N, E, tp.g.size, int(max_iter), float(tol))
    need = ctypes.c_size_t()
    assert getattr(lib, prefix + '_workspace_bytes')(ctypes.byref(cfg), topo.host.ctypes.data, Bt, K, ctypes.byref(need)) == 0
    ws = gns_mod._workspace(need.value, dev)
    f64, row_f64, row_i32, conv = _sentinels(Bt, K, N, E, dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = getattr(lib, prefix + '_screen')(
            ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), buses.data_ptr(), lines.data_ptr(), gens.data_ptr(), Bt,
            list32.ctypes.data, list_dev.data_ptr(), K, isl.data_ptr(), None if rating is None else rating.data_ptr(), per_grid,
            v0.data_ptr(), th0.data_ptr(), conv0.data_ptr(), *(t.data_ptr() for t in f64), row_f64[0].data_ptr(),
            row_i32[0].data_ptr(), row_f64[1].data_ptr(), row_i32[1].data_ptr(), row_f64[2].data_ptr(), row_i32[2].data_ptr(),
            conv.data_ptr(), row_i32[3].data_ptr(), row_f64[3].data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert rc == 0, rc
        torch.cuda.synchronize(dev)
    return _rows(f64, row_f64, row_i32, conv)
