"""CPU checks of the DC power flow's host side (include/gns_powerflow.h, "DC power flow"): the exports, the argument checks and the
LDS refusal of the C entry points, the float64 reference (``dc_reference``) against power balance, and the kernel's algorithm
replayed in numpy on the fast-decoupled blob (Bbus into the B' slots, the two B' programs, the flows, the slack's row and the
adjoint's formulas) against that reference and its autograd."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import EXPORTS, FD_EXPORTS, PF_EXPORTS, PfConfig
import dc_reference as dref
import nr_reference as ref
import pf_topologies as pt
from test_fdpf_host import FH, _arr, _programs
from test_powerflow_programs_host import TOPOLOGIES, run_gather

EINVAL, EUNSUPPORTED = 1, 2
TOL = 1e-9        # the bar of the GPU tests: max|out - ref| <= TOL * max(1, max|ref|)


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _cfg(tp):
    return PfConfig(tp.n, tp.f.size, tp.g.size, 0, 0.0)


def test_exports_are_there_and_disjoint():
    lib = amd.load_library()
    assert len(_lib.DC_EXPORTS) >= 6
    for f in _lib.DC_EXPORTS:
        assert hasattr(lib, f), f
        assert f not in EXPORTS and f not in PF_EXPORTS and f not in FD_EXPORTS
    for f in ('gns_dc_workspace_bytes', 'gns_dc_workspace_bytes_set', 'gns_dc_solve', 'gns_dc_solve_set', 'gns_dc_adjoint',
              'gns_dc_adjoint_set'):
        assert f in _lib.DC_EXPORTS
    assert callable(powerflow.dc_power_flow)
    assert powerflow.DcPowerFlowResult._fields == ('v', 'theta', 'line_flow', 'slack_p', 'converged')


def _calls(lib, cfg, host, n_member=1):
    """The six entry points on dummy (never dereferenced) device pointers: name -> callable(cfg=, host=, dev=, out=) -> rc."""
    d = host.ctypes.data
    need = ctypes.c_size_t(123)
    member = np.zeros(n_member, dtype=np.int32)

    def ws(cfg=cfg, host=d, dev=d, out=d):
        return lib.gns_dc_workspace_bytes(cfg and ctypes.byref(cfg), host, 1, ctypes.byref(need) if out else None)

    def ws_set(cfg=cfg, host=d, dev=d, out=d):
        return lib.gns_dc_workspace_bytes_set(cfg and ctypes.byref(cfg), host, w_size, member.ctypes.data, member.size, 1,
                                              ctypes.byref(need) if out else None)

    def solve(cfg=cfg, host=d, dev=d, out=d):
        return lib.gns_dc_solve(cfg and ctypes.byref(cfg), host, dev, d, d, d, 1, out, d, d, d, None, 0, None)

    def solve_set(cfg=cfg, host=d, dev=d, out=d):
        return lib.gns_dc_solve_set(cfg and ctypes.byref(cfg), host, dev, w_size, member.ctypes.data, member.size, d, None, d, d, d,
                                    1, out, d, d, d, None, 0, None)

    def adjoint(cfg=cfg, host=d, dev=d, out=d):        # out: the forward's theta
        return lib.gns_dc_adjoint(cfg and ctypes.byref(cfg), host, dev, d, d, d, 1, out, d, None, None, None, d, d, d, None, 0, None)

    def adjoint_set(cfg=cfg, host=d, dev=d, out=d):
        return lib.gns_dc_adjoint_set(cfg and ctypes.byref(cfg), host, dev, w_size, member.ctypes.data, member.size, d, None, d, d,
                                      d, 1, out, d, None, None, None, d, d, d, None, 0, None)

    w_size = host.size
    return {'ws': ws, 'ws_set': ws_set, 'solve': solve, 'solve_set': solve_set, 'adjoint': adjoint, 'adjoint_set': adjoint_set}, need


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host: nothing is launched, so the test needs no device."""
    lib = amd.load_library()
    tp = TOPOLOGIES['case14']
    fd, cfg = _fd(tp), _cfg(tp)
    calls, need = _calls(lib, cfg, fd.host)
    assert calls['ws']() == 0 and need.value == 0                     # DC needs no workspace
    need.value = 123
    assert calls['ws_set']() == 0 and need.value == 0
    for name, call in calls.items():
        assert call(cfg=None) == EINVAL, name
        assert call(host=None) == EINVAL, name
        assert call(out=None) == EINVAL, name
        for bad in (PfConfig(tp.n + 1, tp.f.size, tp.g.size, 0, 0.0), PfConfig(tp.n, tp.f.size + 1, tp.g.size, 0, 0.0),
                    PfConfig(tp.n, tp.f.size, tp.g.size + 1, 0, 0.0)):
            assert call(cfg=bad) == EINVAL, name
        if not name.startswith('ws'):
            assert call(dev=None) == EINVAL, name
    # max_iter and tol are not read: values the other solvers refuse are accepted
    odd = PfConfig(tp.n, tp.f.size, tp.g.size, -5, -1.0)
    assert _calls(lib, odd, fd.host)[0]['ws']() == 0
    # a Newton-Raphson blob where an FD blob is expected
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    for name, call in _calls(lib, cfg, nr.host)[0].items():
        assert call() == EINVAL, name
    lds = ctypes.c_int64()
    assert lib.gns_dc_lds_bytes(nr.host.ctypes.data, ctypes.byref(lds)) == EINVAL
    assert lib.gns_dc_lds_bytes(None, ctypes.byref(lds)) == EINVAL


def test_lds_image_and_refusal():
    lib = amd.load_library()
    lds = ctypes.c_int64()
    for name in ('case14', 'case118', 'case300', 'lattice16x16', 'complete33'):
        fd = _fd(TOPOLOGIES[name])
        i = fd.info
        assert lib.gns_dc_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds)) == 0
        assert lds.value == 8 * (i['nnz_lu_p'] + i['dim_p'] + i['n_bus']) == powerflow._dc_lds_bytes(fd.host)
        assert lds.value < i['lds_bytes']                              # every topology fast_decoupled accepts, DC accepts
    # path(1500): fast_decoupled refuses it (167 904 B), DC's queries pass
    tp = pt.path(1500)
    fd = _fd(tp)
    assert fd.info['lds_bytes'] == 167904 > pt.LDS_LIMIT
    calls, need = _calls(lib, _cfg(tp), fd.host)
    assert calls['ws']() == 0 and calls['ws_set']() == 0
    assert powerflow._dc_lds_bytes(fd.host) == 8 * (fd.info['nnz_lu_p'] + 1499 + 1500) <= pt.LDS_LIMIT
    # path(6000): 23 994 slots for B' pass the analysis; factor and right-hand side alone are 191 952 B
    tp = pt.path(6000)
    fd = _fd(tp)
    assert fd.info['nnz_lu_p'] + fd.info['dim_p'] == 23994
    calls, need = _calls(lib, _cfg(tp), fd.host)
    assert calls['ws']() == 0                                         # the one-blob query does not look at the image (as FD's)
    for name in ('ws_set', 'solve', 'solve_set', 'adjoint', 'adjoint_set'):
        assert calls[name]() == EUNSUPPORTED, name
    assert calls['solve'](cfg=PfConfig(5999, 5999, 1, 0, 0.0)) == EINVAL       # GNS_EINVAL wins
    want = 191952 + 8 * 6000
    assert powerflow._dc_lds_bytes(fd.host) == want
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dc_solve', powerflow._dc_lds_bytes(fd.host), powerflow._DC.formula)
    assert str(want) in str(e.value) and 'nnz_lu_p + dim_p + N' in str(e.value) and "B''" not in str(e.value)


@pytest.mark.parametrize('case', [14, 30, 118, 300])
def test_reference_balances_power(case):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, 3, seed=7)
    lines = _shifted(lines, seed=case)
    for k in range(buses.shape[0]):
        bus, line, gen = (x[k].double() for x in (buses, lines, gens))
        theta, flow, slack_p = dref.dc_power_flow(bus, line, gen, slack)
        assert float(theta[slack - 1]) == 0.0
        n = bus.shape[0]
        f, t = line[:, 0].long() - 1, line[:, 1].long() - 1
        out = torch.zeros(n, dtype=torch.float64).index_add(0, f, flow).index_add(0, t, -flow)   # flow leaving each bus
        pg = torch.zeros(n, dtype=torch.float64).index_add(0, gen[:, 0].long() - 1, gen[:, 6])
        net = pg - bus[:, 2] - bus[:, 4]
        net[slack - 1] += slack_p
        scale = max(1.0, float(flow.abs().max()))
        assert float((out - net).abs().max()) <= TOL * scale, (case, k)
        total = float((bus[:, 2] + bus[:, 4]).sum() - gen[:, 6].sum())
        assert abs(float(slack_p) - total) <= TOL * max(1.0, abs(total)), (case, k)


def _shifted(lines, seed):
    """``lines`` with shifts of order +-0.1 rad on a third of the lines (the taps of the synthetic grids are away from 1 already)."""
    g = torch.Generator().manual_seed(seed)
    lines = lines.clone()
    on = torch.rand(lines.shape[:2], generator=g) < 1 / 3
    lines[..., 6] = torch.where(on, (torch.rand(lines.shape[:2], generator=g) - 0.5) * 0.4, lines[..., 6])
    return lines


# ---- the kernel's algorithm in numpy on the FD blob: what gns_dcpf.hip does, operation for operation but for the order of sums

def _line_b(line):
    return 1.0 / (line[:, 3] * line[:, 5])


def _entries(w, line):
    """Bbus by Y-bus entry, from the stamps: +b for ff / tt, -b for ft / tf."""
    nnzy = w[FH['NNZY']]
    st_ptr, st = _arr(w, 'ST_PTR', nnzy + 1), _arr(w, 'ST', 4 * w[FH['E']])
    b = _line_b(line)
    val = np.zeros(nnzy)
    for p in range(nnzy):
        for q in range(st_ptr[p], st_ptr[p + 1]):
            val[p] += b[st[q] >> 2] if (st[q] & 3) < 2 else -b[st[q] >> 2]
    return val


def _diag_stamps(w, i):
    nnzy = w[FH['NNZY']]
    st_ptr, st = _arr(w, 'ST_PTR', nnzy + 1), _arr(w, 'ST', 4 * w[FH['E']])
    d = _arr(w, 'Y_DIAG', w[FH['N']])[i]
    return [(s >> 2, s & 3) for s in st[st_ptr[d]:st_ptr[d + 1]] if (s & 3) < 2]


def _factor(w, line):
    nnzy, d1, nnz1 = w[FH['NNZY']], w[FH['DIM1']], w[FH['NNZLU1']]
    bslot = _arr(w, 'BSLOT', 2 * nnzy)[0::2]
    F = np.zeros(nnz1 + d1)
    on = bslot >= 0
    F[bslot[on]] = _entries(w, line)[on]
    run_gather(F, *_programs(w)['f1'])
    return F, nnz1


def _injection(w, bus, line, gen, i):
    N = w[FH['N']]
    gen_ptr, gen_idx = _arr(w, 'GEN_PTR', N + 1), _arr(w, 'GEN_IDX', max(w[FH['GN']], 1))
    p = sum(gen[gen_idx[q], 6] for q in range(gen_ptr[i], gen_ptr[i + 1])) - bus[i, 2] - bus[i, 4]
    b = _line_b(line)
    for e, kind in _diag_stamps(w, i):
        pfinj = -b[e] * line[e, 6]
        p -= pfinj if kind == 0 else -pfinj
    return p


def emulate_solve(w, bus, line, gen):
    N, slack = w[FH['N']], w[FH['SLACK']]
    p_idx = _arr(w, 'P_IDX', N)
    F, nnz1 = _factor(w, line)
    for i in range(N):
        if p_idx[i] >= 0:
            F[nnz1 + p_idx[i]] = _injection(w, bus, line, gen, i)
    run_gather(F, *_programs(w)['s1'])
    theta = np.array([F[nnz1 + p_idx[i]] if p_idx[i] >= 0 else 0.0 for i in range(N)])
    f, t = line[:, 0].astype(int) - 1, line[:, 1].astype(int) - 1
    b = _line_b(line)
    flow = b * (theta[f] - theta[t]) + (-b * line[:, 6])
    y_ptr, y_col = _arr(w, 'Y_PTR', N + 1), _arr(w, 'Y_COL', w[FH['NNZY']])
    val = _entries(w, line)
    row = slice(y_ptr[slack], y_ptr[slack + 1])
    slack_p = float(val[row] @ theta[y_col[row]]) - _injection(w, bus, line, gen, slack)
    return theta, flow, slack_p


def emulate_adjoint(w, bus, line, gen, theta, gth, gfl, gsp):
    N = w[FH['N']]
    p_idx = _arr(w, 'P_IDX', N)
    F, nnz1 = _factor(w, line)
    b = _line_b(line)
    for i in range(N):
        if p_idx[i] < 0:
            continue
        x = gth[i]
        for e, kind in _diag_stamps(w, i):
            x += gfl[e] * b[e] if kind == 0 else -gfl[e] * b[e]
        F[nnz1 + p_idx[i]] = x
    run_gather(F, *_programs(w)['s1'])
    lam = np.array([F[nnz1 + p_idx[i]] if p_idx[i] >= 0 else 0.0 for i in range(N)])
    gb, gl, gg = np.zeros_like(bus), np.zeros_like(line), np.zeros_like(gen)
    gb[:, 2] = gb[:, 4] = -(lam - gsp)
    gg[:, 6] = lam[gen[:, 0].astype(int) - 1] - gsp
    f, t = line[:, 0].astype(int) - 1, line[:, 1].astype(int) - 1
    wl = gfl - (lam[f] - lam[t])
    d_b = wl * (theta[f] - theta[t] - line[:, 6])
    gl[:, 3] = -d_b * b / line[:, 3]
    gl[:, 5] = -d_b * b / line[:, 5]
    gl[:, 6] = -b * wl
    return gb, gl, gg


def _close(got, want, what):
    want = np.asarray(want)
    assert np.max(np.abs(np.asarray(got) - want), initial=0.0) <= TOL * max(1.0, np.max(np.abs(want), initial=0.0)), what


GENERATED = ('case14', 'case30', 'lattice8x8', 'random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen',
             'star65_pv', 'path66_pv1', 'pair')


@pytest.mark.parametrize('name', GENERATED)
def test_the_fd_blob_serves_the_dc_solve_and_its_adjoint(name):
    tp = TOPOLOGIES[name]
    w = _fd(tp).host
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0)
    lines = _shifted(lines, seed=len(name))
    rng = np.random.default_rng(len(name))
    for k in range(buses.shape[0]):
        bus, line, gen = (x[k].double().numpy() for x in (buses, lines, gens))
        theta, flow, slack_p = emulate_solve(w, bus, line, gen)
        rt, rf, rs = dref.dc_power_flow(bus, line, gen, tp.slack)
        _close(theta, rt, (name, k, 'theta'))
        _close(flow, rf, (name, k, 'line_flow'))
        _close(slack_p, rs, (name, k, 'slack_p'))
        gth, gfl, gsp = rng.standard_normal(tp.n), rng.standard_normal(tp.f.size), float(rng.standard_normal())
        got = emulate_adjoint(w, bus, line, gen, theta, gth, gfl, gsp)
        want = dref.gradients(bus, line, gen, tp.slack, gth, gfl, gsp)
        for x, y, what in zip(got, want, ('buses', 'lines', 'generators')):
            y = y.numpy()
            assert np.max(np.abs(x - y)) <= 1e-9 * max(1.0, np.max(np.abs(y))), (name, k, what)
            keep = {'buses': [2, 4], 'lines': [3, 5, 6], 'generators': [6]}[what]
            other = [c for c in range(y.shape[1]) if c not in keep]
            assert np.max(np.abs(y[:, other]), initial=0.0) <= 1e-9 * max(1.0, np.max(np.abs(y))), (name, k, what)

