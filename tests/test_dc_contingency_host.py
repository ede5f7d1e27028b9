"""CPU checks of the DC contingency screen's host side (include/gns_powerflow.h, "DC contingency screening"): the exports, the
argument checks and the LDS refusal of the C entry points, the bridge finder against brute force, the Python argument checks, and
the kernel's algorithm replayed in numpy on the fast-decoupled blob (Bbus into the B' slots, the B' programs with the solve program
run operation by operation as one lane runs it, the rank-1 formulas) against the direct reference (``dc_contingency_reference``:
the line removed and the grid solved again).

The bar is the project's DC bar per (grid, outage): max|out - ref| <= 1e-9 max(1, max|ref|).  No outage is left out."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import DC_EXPORTS, EXPORTS, FD_EXPORTS, PF_EXPORTS, PfConfig
import dc_contingency_reference as cref
import pf_topologies as pt
from test_dcpf_host import _factor, _line_b, _shifted, emulate_solve
from test_fdpf_host import FH, _arr, _programs
from test_powerflow_programs_host import TOPOLOGIES, _fields

EINVAL, EUNSUPPORTED = 1, 2
TOL = 1e-9


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _cfg(tp):
    return PfConfig(tp.n, tp.f.size, tp.g.size, 0, 0.0)


def test_exports_are_there_and_disjoint():
    lib = amd.load_library()
    assert set(('gns_dcn1_lds_bytes', 'gns_dcn1_workspace_bytes', 'gns_dcn1_screen')) <= set(_lib.DCN1_EXPORTS)
    for f in _lib.DCN1_EXPORTS:
        assert hasattr(lib, f), f
        assert f not in EXPORTS and f not in PF_EXPORTS and f not in FD_EXPORTS and f not in DC_EXPORTS
        assert getattr(lib, f).restype is ctypes.c_int
    assert DC_EXPORTS == ('gns_dc_lds_bytes', 'gns_dc_workspace_bytes', 'gns_dc_solve', 'gns_dc_workspace_bytes_set',
                          'gns_dc_solve_set', 'gns_dc_adjoint', 'gns_dc_adjoint_set')
    assert callable(powerflow.dc_contingency_screen)
    assert powerflow.DcContingencyResult._fields == ('base', 'outages', 'line_flow', 'worst_loading', 'worst_line', 'islanding',
                                                     'converged')
    assert powerflow._DCN1.prefix == 'gns_dcn1' and powerflow._DCN1.formula == powerflow._DCN1_LDS_FORMULA


def _screen(lib, cfg, blob, outages, **kw):
    """gns_dcn1_screen on dummy (never dereferenced) device pointers; a keyword replaces one argument."""
    d = blob.ctypes.data
    o = np.asarray(outages, dtype=np.int32)
    a = dict(cfg=ctypes.byref(cfg) if cfg is not None else None, host=d, dev=d, buses=d, lines=d, gens=d, Bt=1, out_host=o.ctypes.data,
             out_dev=d, K=o.size, isl=d, rating=None, per_grid=0, flow=None, worst=d, worst_line=d, conv=d)
    a.update(kw)
    return lib.gns_dcn1_screen(a['cfg'], a['host'], a['dev'], a['buses'], a['lines'], a['gens'], a['Bt'], a['out_host'], a['out_dev'],
                               a['K'], a['isl'], a['rating'], a['per_grid'], a['flow'], a['worst'], a['worst_line'], a['conv'], None, 0,
                               None)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host: nothing is launched, so the test needs no device."""
    lib = amd.load_library()
    tp = TOPOLOGIES['case14']
    fd, cfg = _fd(tp), _cfg(tp)
    E = tp.f.size
    need = ctypes.c_size_t(123)
    d = fd.host.ctypes.data
    assert lib.gns_dcn1_workspace_bytes(ctypes.byref(cfg), d, 4, E, ctypes.byref(need)) == 0 and need.value == 0
    for args in ((None, d, 4, E, ctypes.byref(need)), (ctypes.byref(cfg), None, 4, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, E, None), (ctypes.byref(cfg), d, 0, E, ctypes.byref(need)),
                 (ctypes.byref(cfg), d, 4, 0, ctypes.byref(need)), (ctypes.byref(cfg), d, 4, -3, ctypes.byref(need))):
        assert lib.gns_dcn1_workspace_bytes(*args) == EINVAL, args
    # null arguments (line_flow and rating may be NULL: they are in every call here)
    for name in ('cfg', 'host', 'dev', 'buses', 'lines', 'gens', 'out_host', 'out_dev', 'isl', 'worst', 'worst_line', 'conv'):
        assert _screen(lib, None if name == 'cfg' else cfg, fd.host, [0, 3], **({} if name == 'cfg' else {name: None})) == EINVAL, name
    # wrong shapes
    for bad in (PfConfig(tp.n + 1, E, tp.g.size, 0, 0.0), PfConfig(tp.n, E + 1, tp.g.size, 0, 0.0),
                PfConfig(tp.n, E, tp.g.size + 1, 0, 0.0)):
        assert _screen(lib, bad, fd.host, [0]) == EINVAL
        assert lib.gns_dcn1_workspace_bytes(ctypes.byref(bad), d, 4, E, ctypes.byref(need)) == EINVAL
    assert _screen(lib, cfg, fd.host, [0], Bt=0) == EINVAL and _screen(lib, cfg, fd.host, [0], Bt=-1) == EINVAL
    assert _screen(lib, cfg, fd.host, [0], per_grid=2) == EINVAL
    assert _screen(lib, cfg, fd.host, list(range(E)) * 4, Bt=0x7FFFFFFF) == EINVAL       # more workgroups than one launch takes
    # a Newton-Raphson blob where an FD blob is expected
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert _screen(lib, cfg, nr.host, [0]) == EINVAL
    assert lib.gns_dcn1_workspace_bytes(ctypes.byref(cfg), nr.host.ctypes.data, 4, E, ctypes.byref(need)) == EINVAL
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    assert lib.gns_dcn1_lds_bytes(nr.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn1_lds_bytes(None, ctypes.byref(lds), ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn1_lds_bytes(d, None, ctypes.byref(lanes)) == EINVAL
    assert lib.gns_dcn1_lds_bytes(d, ctypes.byref(lds), None) == 0
    # a bad outage index, a bad outage count
    for bad in ([E], [-1], [0, 1, E, 2], [2 ** 31 - 1]):
        assert _screen(lib, cfg, fd.host, bad) == EINVAL, bad
    assert _screen(lib, cfg, fd.host, [0], K=0) == EINVAL and _screen(lib, cfg, fd.host, [0], K=-1) == EINVAL


def _image(info, lanes):
    return 8 * (info['nnz_lu_p'] + info['dim_p'] + info['n_bus'] + 3 * info['n_line'] + info['dim_p'] * (lanes + 1))


def test_lds_image_and_refusal():
    lib = amd.load_library()
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    want_lanes = {'case14': 64, 'case30': 64, 'case118': 64, 'case300': 32}
    for name in ('case14', 'case30', 'case118', 'case300', 'lattice16x16', 'complete33', 'star200_pq'):
        fd = _fd(TOPOLOGIES[name])
        assert lib.gns_dcn1_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == 0
        w = lanes.value
        assert w in (1, 2, 4, 8, 16, 32, 64) and lds.value == _image(fd.info, w) <= pt.LDS_LIMIT, name
        assert w == 64 or _image(fd.info, 2 * w) > pt.LDS_LIMIT, name           # the widest that fits
        assert (lds.value, w) == powerflow._dcn1_lds_bytes(fd.host)
        assert lds.value == powerflow._dc_lds_bytes(fd.host) + 8 * (3 * fd.info['n_line'] + fd.info['dim_p'] * (w + 1))
        if name in want_lanes:
            assert w == want_lanes[name], name
    # path(6000): the image of one outage at a time is above the limit already
    tp = pt.path(6000)
    fd = _fd(tp)
    want = _image(fd.info, 1)
    assert powerflow._dcn1_lds_bytes(fd.host) == (want, 1) and want > pt.LDS_LIMIT
    assert _screen(lib, _cfg(tp), fd.host, [0]) == EUNSUPPORTED
    assert _screen(lib, _cfg(tp), fd.host, [tp.f.size]) == EINVAL                      # GNS_EINVAL wins
    assert _screen(lib, PfConfig(5999, 5999, 1, 0, 0.0), fd.host, [0]) == EINVAL
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcn1_screen', lambda: powerflow._dcn1_lds_bytes(fd.host)[0], powerflow._DCN1.formula)
    assert str(want) in str(e.value) and 'dim_p (W + 1)' in str(e.value) and 'W = 1' in str(e.value)


def _brute_force(tp):
    f, t = tp.f - 1, tp.t - 1
    return np.array([powerflow._islanded(tp.n, np.delete(f, e), np.delete(t, e), tp.slack - 1).size > 0 for e in range(f.size)])


def _bridge_topologies():
    out = dict(TOPOLOGIES)
    out.update(pt.families())
    return out


@pytest.mark.parametrize('name', sorted(_bridge_topologies()))
def test_bridges_equal_brute_force_islanding(name):
    tp = _bridge_topologies()[name]
    if tp.f.size == tp.n - 1 and tp.n > 1500:              # the LDS boundary chain (brute force is quadratic): a tree, all bridges
        assert bool(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1).all())
        return
    got = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    assert got.dtype == np.bool_ and got.shape == tp.f.shape
    assert np.array_equal(got, _brute_force(tp)), name


def test_bridges_with_parallel_lines_and_self_loops():
    tp = TOPOLOGIES['random40_parallel_selfloop']
    pairs = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    assert any(a == b for a, b in pairs) and len(set(pairs)) < len(pairs)       # the family has both
    # 1 - 2 = 3 - 4, 4 - 4: a doubled line, two bridges, a self-loop
    f, t = np.array([0, 1, 1, 2, 3]), np.array([1, 2, 2, 3, 3])
    assert powerflow._bridges(4, f, t).tolist() == [True, False, False, True, False]
    tp = pt.Topo('toy', 4, f + 1, t + 1, np.array([1]), 1)
    assert _brute_force(tp).tolist() == [True, False, False, True, False]
    # the cache lives with the topology and is filled once
    tp = TOPOLOGIES['case30']
    topo = _fd(tp)
    args = (tp.n, tp.f.astype(np.float64), tp.t.astype(np.float64))
    first = powerflow._topology_bridges(topo, args)
    assert powerflow._topology_bridges(topo, args) is first and int(first.sum()) == 5
    counts = {14: 1, 30: 5, 118: 20, 300: 85}
    for case, want in counts.items():
        tp = TOPOLOGIES[f'case{case}']
        assert int(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1).sum()) == want


# ---- the kernel's algorithm in numpy on the FD blob: what gns_dcn1.hip does, operation for operation but for the order of sums

def _lane_solve(F, nnz1, ops):
    """The solve program as one lane runs it: every operation in the blob's order on the lane's own right-hand side."""
    dst, a, b = _fields(ops)
    assert np.all(dst >= nnz1) and np.all(a < nnz1) and np.all((b < 0) | (b >= nnz1))     # what dcn1_lane_solve relies on
    for d, x, y in zip(dst.tolist(), a.tolist(), b.tolist()):
        if y < 0:
            F[d] = F[d] / F[x]
        else:
            F[d] -= F[x] * F[y]


def emulate_screen(w, bus, line, gen, outages, bridges):
    """Post-outage flows [K, E] (NaN rows for bridges)."""
    N, d1 = w[FH['N']], w[FH['DIM1']]
    p_idx = _arr(w, 'P_IDX', N)
    _, flow, _ = emulate_solve(w, bus, line, gen)
    F, nnz1 = _factor(w, line)
    ops = _programs(w)['s1'][1]
    b = _line_b(line)
    f, t = line[:, 0].astype(int) - 1, line[:, 1].astype(int) - 1
    out = np.full((len(outages), line.shape[0]), np.nan)
    for j, k in enumerate(outages):
        if bridges[k]:
            continue
        Fk = F.copy()
        Fk[nnz1:] = 0.0
        pf, pt_ = p_idx[f[k]], p_idx[t[k]]
        if pf != pt_:
            if pf >= 0:
                Fk[nnz1 + pf] = 1.0
            if pt_ >= 0:
                Fk[nnz1 + pt_] = -1.0
        _lane_solve(Fk, nnz1, ops)
        assert np.array_equal(Fk[:nnz1], F[:nnz1])                         # the factor is read-only
        z = np.array([Fk[nnz1 + p_idx[i]] if p_idx[i] >= 0 else 0.0 for i in range(N)])
        assert Fk.size == nnz1 + d1
        alpha = flow[k] / (1.0 - b[k] * (z[f[k]] - z[t[k]]))
        out[j] = flow + b * (z[f] - z[t]) * alpha
        out[j, k] = 0.0
    return out


def _replay(tp, buses, lines, gens, outages, name):
    w = _fd(tp).host
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    worst = 0.0
    for i in range(buses.shape[0]):
        bus, line, gen = (x[i].double().numpy() for x in (buses, lines, gens))
        got = emulate_screen(w, bus, line, gen, outages, bridges)
        for j, k in enumerate(outages):
            want = cref.outage_flows(bus, line, gen, tp.slack, k)
            assert (want is None) == bool(bridges[k]), (name, i, k)
            if want is None:
                assert np.isnan(got[j]).all()
                continue
            err, scale = float(np.max(np.abs(got[j] - want.numpy()))), max(1.0, float(want.abs().max()))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (name, i, k, err, scale)
    print(f'{name}: worst scaled error {worst:.2e}')


@pytest.mark.parametrize('case', [14, 30, 118])
def test_the_fd_blob_serves_the_screen_on_the_cases(case):
    """Every outage of the case, islanding ones included, on two grids with shifts that matter."""
    tp = TOPOLOGIES[f'case{case}']
    buses, lines, gens = synth.synth_grids(case, 2, seed=0)
    _replay(tp, buses, _shifted(lines, seed=case), gens, list(range(tp.f.size)), f'case{case}')


@pytest.mark.parametrize('name', ['random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen', 'lattice8x8',
                                  'star65_pv', 'pair'])
def test_the_fd_blob_serves_the_screen_on_generated_families(name):
    """Families on which a dense float64 LODF and the direct reference agree to 1e-10 (the probe of test_dc_contingency_gpu's
    docstring), every outage: parallel lines, a line from a bus to itself, lines at the slack, all-bridge topologies."""
    tp = TOPOLOGIES[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0)
    _replay(tp, buses, _shifted(lines, seed=len(name)), gens, list(range(tp.f.size)), name)


# ---- the Python argument checks (refused before a device is needed)

def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 3)
    E = lines.shape[1]

    def screen(**kw):
        return powerflow.dc_contingency_screen(buses, lines, gens, slack_bus=1, **kw)

    for bad in ([E], [-1], [0, E + 5], torch.tensor([0, E])):
        with pytest.raises(ValueError, match='outages must lie in'):
            screen(outages=bad)
    for bad in ([0.0, 1.0], [1.5], torch.tensor([1.0]), np.array([True, False])):
        with pytest.raises(ValueError, match='outages must hold integers'):
            screen(outages=bad)
    for bad in ([], torch.zeros(0, dtype=torch.int64), range(0)):
        with pytest.raises(ValueError, match='outages is empty'):
            screen(outages=bad)
    with pytest.raises(ValueError, match='1-D'):
        screen(outages=[[0, 1]])
    for bad in (torch.zeros(E), -torch.ones(E), torch.full((E,), float('inf')), torch.full((3, E), float('nan'))):
        with pytest.raises(ValueError, match='rating must be positive and finite'):
            screen(rating=bad)
    for bad in (torch.ones(E - 1), torch.ones(2, E), torch.ones(3, E, 1), 1.0):
        with pytest.raises(ValueError, match='rating must be'):
            screen(rating=bad)
    with pytest.raises(ValueError, match='flows must be a bool'):
        screen(flows=1)
    with pytest.raises(ValueError, match='float32'):
        powerflow.dc_contingency_screen(buses.double(), lines, gens, slack_bus=1)
    # a batch that mixes topologies: the refusal of the other solvers, under this solver's name
    mixed = lines.clone()
    mixed[1, 0, 1] = 5
    with pytest.raises(ValueError, match='differ across the batch: dc_contingency_screen solves one topology'):
        powerflow._topology_key(buses, mixed, gens, 1, 'dc_contingency_screen')
    assert powerflow._outage_list(None, 5).tolist() == [0, 1, 2, 3, 4]
    assert powerflow._outage_list(range(3, 0, -1), 5).tolist() == [3, 2, 1]
    assert powerflow._outage_list(np.array([4, 4, 0], dtype=np.int16), 5).dtype == np.int64
