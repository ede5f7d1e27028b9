"""Batched Newton-Raphson AC power flow on the device: the baseline the reference evaluates a trained GNS against
(PYPOWER ``runpf(PF_ALG=1)``, ``GNS/evaluate.py:24-40``), for a whole batch of grids that share one topology, or with
``mixed_topologies=True`` for a batch that mixes them (an N-1 contingency set, ``synth.contingency_grids``).

    res = powerflow.newton_raphson(buses, lines, generators, slack_bus=1)
    res.v, res.theta, res.converged, res.iterations, res.mismatch

The semantics (bus roles, Y-bus, injections, starting point, convergence test, per-grid failure) are those of
``include/gns_powerflow.h``; the solve runs in one HIP kernel (``csrc/gns_powerflow.hip``) in float64.  The sparse structure of
the Jacobian and of its LU factor is analysed once per topology on the host (``csrc/gns_pf_topology.cpp``) and cached; a mixed
batch reads its topologies from a device set of those blobs (``gns_pf_solve_set``) that grows as new topologies appear.
With ``requires_grad`` on the inputs the solve is differentiable: its backward is one adjoint kernel (``gns_pf_adjoint`` /
``gns_pf_adjoint_set``) on the same analysis.

``fast_decoupled(..., variant='XB' | 'BX')`` is the second baseline of the reference's evaluation (PYPOWER ``runpf(PF_ALG=2 | 3)``,
``GNS/evaluate.py:42-58``): B' and B'' are factored once per grid in one HIP kernel (``csrc/gns_fdpf.hip``) from their own cached
analysis (``gns_fd_prepare_topology``); its gradients are the Newton-Raphson adjoint at its solution.

``dc_power_flow(...)`` is the linear baseline (PYPOWER ``makeBdc`` + ``dcpf``, the DC option of the reference's commented-out
``runpf``): angles, per-line active flows and the slack's balancing power from one factorisation and one solve per grid
(``csrc/gns_dcpf.hip``) on the fast-decoupled analysis, whose B' has the DC matrix's sparsity; its backward is a second solve on
the same factor (``gns_dc_adjoint``).

``dc_contingency_screen(...)`` screens a batch against a list of single-line outages (an N-1 set) from the base factor alone: one
more solve per outage gives the exact post-outage DC flows (line-outage distribution factors, ``csrc/gns_dcn1.hip``), with the worst
loading and its line per ``(grid, outage)``; outages that disconnect the grid are found on the host as the bridges of the topology.
With ``differentiable=True`` its backward is one ``gns_dcn1_adjoint`` call: a second solve on the base factor per outage.

``dc_n2_contingency_screen(...)`` screens a batch against a list of double-line outages (an N-2 set): a pair is a rank-2 change of
the DC matrix, so the single-outage solves (one per distinct line of the list) and a 2x2 system per pair give the exact flows
(``csrc/gns_dcn2.hip``); the pairs that disconnect the grid are found on the host.

``dc_generator_contingency_screen(...)`` screens a batch against a list of generator outages, each alone or with a line out as well
(the combined N-1 set): a generator outage changes the injections alone, so it is one more solve on the base factor per distinct
generator, and the line on top of it is the single-outage update again (``csrc/gns_dcg1.hip``).
``dc_generator_contingency_screen_differentiable(...)`` is the same call with a backward on the device (``gns_dcg1_adjoint``), the
pickup weights included.

``ac_contingency_screen(...)`` is the AC answer to the same question: Newton-Raphson on every ``(grid, outage)`` pair, warm-started
from the base solution, on the base topology's analysis alone (an outage only removes Jacobian entries), with the post-outage
voltages, the branch flows at both ends of every line, the worst loading and the voltage extremes (``csrc/gns_acn1.hip``).
With ``differentiable=True`` its backward is one ``gns_acn1_adjoint`` call: per pair one factorisation and one transposed solve
at the forward's state, on the same analysis.

``ac_n2_contingency_screen(...)`` is that screen for a list of double-line outages, such as the worst pairs
``dc_n2_contingency_screen`` ranked: Newton-Raphson on every ``(grid, pair)``, again on the base topology's analysis alone
(``csrc/gns_acn2.hip``).  ``ac_n2_contingency_screen_differentiable(...)`` is the same screen with a backward: one ``gns_acn2_adjoint`` call,
per pair one factorisation and one transposed solve at the forward's state.

``ac_generator_contingency_screen(...)`` is the AC screen of the rows ``dc_generator_contingency_screen`` takes, a generator out alone
or with a line out as well: the bus of a lost unit may turn from PV to PQ, so the topology is analysed once per distinct generator of
the list (``gns_pf_prepare_topology_out_gen``) and every row runs Newton-Raphson on its generator's analysis, the line on top of it
as in ``ac_contingency_screen`` (``csrc/gns_acg1.hip``).  ``ac_generator_contingency_screen_differentiable(...)`` is the same screen
with a backward: one ``gns_acg1_adjoint`` call, per row one factorisation and one transposed solve at the forward's state on the
row's own analysis, with the gradients of the dispatch, the set points and the pickup weights by generator row.

``solved_case(buses, lines, generators, v, theta)`` is the base row of that family and what PYPOWER's ``pfsoln`` adds to a solve: at
a given state (a solver's, or a GNS prediction) the flows at both ends of every line, the bus injections, Newton-Raphson's own
``||F||_inf``, the generators' ``P`` and ``Q``, the slack's balancing power and the screens' summaries, in one launch
(``csrc/gns_pfs.hip``), with a backward (``gns_pfs_adjoint``) to the state and the inputs that needs no linear solve.

``dc_optimal_power_flow(...)`` chooses the dispatch the other calls evaluate (PYPOWER ``dcopf`` without piecewise-linear costs): a
primal-dual interior point per grid on the problem reduced to the dispatch by generator shift factors (``csrc/gns_dcopf.hip``), with
the locational marginal prices and the multipliers.  ``dc_optimal_power_flow_differentiable(...)`` is the same call with a backward
(``gns_dcopf_adjoint``, ``csrc/gns_dcopf_adjoint.hip``): the implicit-function theorem on the KKT conditions of the active set, one
dense LU in LDS and three solves on the base factor per grid.

``dc_security_constrained_opf(...)`` is that problem with contingency rows ``(l, k)``: line ``l``'s flow after the outage of line ``k``
stays within its contingency rating (``csrc/gns_dcscopf.hip``: the screen's line-outage factor per row, then the same interior point
with the rows behind the lines').  ``dc_secure_dispatch(...)`` is the constraint-generation driver around it and
``dc_contingency_screen``: the cheapest dispatch that survives every single-line outage.
"""
from __future__ import annotations

import ctypes
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import gns as _gns
from ._lib import (GNS_ERRORS, GNS_ETOPOLOGY, GNS_EUNSUPPORTED, PF_LDS_MAX_BYTES, PF_MAX_SLOTS, FdConfig, FdInfo, PfConfig, PfInfo,
                   load_library)

PowerFlowResult = namedtuple('PowerFlowResult', ['v', 'theta', 'converged', 'iterations', 'mismatch'])

DcPowerFlowResult = namedtuple('DcPowerFlowResult', ['v', 'theta', 'line_flow', 'slack_p', 'converged'])

DcOpfResult = namedtuple('DcOpfResult', ['pg', 'theta', 'line_flow', 'lmp', 'mu_line', 'mu_pmax', 'mu_pmin', 'objective', 'converged',
                                         'iterations'])
DcScopfResult = namedtuple('DcScopfResult', DcOpfResult._fields + ('mu_row', 'row_flow'))
DcSecureDispatch = namedtuple('DcSecureDispatch', ['result', 'rows', 'worst_loading', 'secure'])

DcContingencyResult = namedtuple('DcContingencyResult', ['base', 'outages', 'line_flow', 'worst_loading', 'worst_line', 'islanding',
                                                         'converged'])

DcN2ContingencyResult = namedtuple('DcN2ContingencyResult', ['base', 'pairs', 'line_flow', 'worst_loading', 'worst_line', 'islanding',
                                                             'converged'])

DcGeneratorContingencyResult = namedtuple('DcGeneratorContingencyResult', ['base', 'contingencies', 'line_flow', 'worst_loading',
                                                                           'worst_line', 'islanding', 'converged'])

AcContingencyResult = namedtuple('AcContingencyResult', ['base', 'outages', 'v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to',
                                                         'worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus',
                                                         'converged', 'iterations', 'mismatch', 'islanding'])

AcN2ContingencyResult = namedtuple('AcN2ContingencyResult', ['base', 'pairs', 'v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to',
                                                             'worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus',
                                                             'converged', 'iterations', 'mismatch', 'islanding'])

AcGeneratorContingencyResult = namedtuple('AcGeneratorContingencyResult', ['base', 'contingencies', 'v', 'theta', 'p_from', 'q_from',
                                                                           'p_to', 'q_to', 'worst_loading', 'worst_line', 'v_min',
                                                                           'v_min_bus', 'v_max', 'v_max_bus', 'converged', 'iterations',
                                                                           'mismatch', 'islanding'])

SolvedCase = namedtuple('SolvedCase', ['p_from', 'q_from', 'p_to', 'q_to', 'p_inj', 'q_inj', 'mismatch', 'gen_p', 'gen_q', 'slack_p',
                                       'worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max', 'v_max_bus'])

MixedPlan = namedtuple('MixedPlan', ['topology', 'order', 'grid_off', 'member_off', 'topo_set', 'slack_bus', 'islanded'])

_TOPO_CACHE = {}
_ISLANDED = set()       # keys of _TOPO_CACHE's form whose topology leaves buses without a path of lines to the slack
_SET_CACHE = {}         # (N, E, Gn, slack_bus, device) -> _PfTopologySet
_FD_TOPO_CACHE = {}     # _TOPO_CACHE's keys -> FdTopology
_FD_SET_CACHE = {}      # _SET_CACHE's keys -> _PfTopologySet of FD blobs


class IslandedTopology(ValueError):
    """A topology with buses that have no path of lines to the slack (their angles are undetermined)."""


class PowerFlowTopology:
    """Host analysis of one topology (the blob on the host and, copied on first use, on the device) and what it found (``info``)."""

    INFO, INFO_FN = PfInfo, 'gns_pf_topology_info'     # the blob's info struct and the entry point that fills it

    def __init__(self, host, dev):
        self.host = host
        self._dev, self._blob = dev, None
        info = self.INFO()
        _check(getattr(load_library(), self.INFO_FN)(host.ctypes.data, ctypes.byref(info)), self.INFO_FN)
        self.info = {k: getattr(info, k) for k, _ in self.INFO._fields_}

    @property
    def blob(self):
        if self._blob is None and self._dev is not None:
            self._blob = torch.from_numpy(self.host).to(self._dev)
        return self._blob


class FdTopology(PowerFlowTopology):
    """Host analysis of one topology for the fast-decoupled solver (B' and B'', ``gns_fd_prepare_topology``): ``info`` holds both
    dimensions, both nnz(L+U), the four programs' operation and step counts and the LDS image."""

    INFO, INFO_FN = FdInfo, 'gns_fd_topology_info'


class _PfTopologySet:
    """The topologies mixed calls of one ``(N, E, Gn, slack, device)`` have met: their blobs concatenated at 16-word (64-byte) aligned
    word offsets, on the host (``host``, what gns_pf_solve_set validates) and in one device tensor (``blob``), grown as new topologies
    appear (the scheme of ``gns._TopologySet``).  A call on topologies the set already holds copies nothing."""

    ALIGN_WORDS = 16

    def __init__(self, dev):
        self.dev = dev
        self.offset = {}                # topology key -> word offset of its blob
        self.parts, self.words = [], 0
        self.host, self.blob = np.zeros(0, dtype=np.int32), None

    def add(self, key, topo):
        off = self.offset.get(key)
        if off is None:
            off = self.offset[key] = self.words
            self.parts.append((off, topo.host))
            self.words += (topo.host.size + self.ALIGN_WORDS - 1) // self.ALIGN_WORDS * self.ALIGN_WORDS
        return off

    def sync(self):
        """Bring ``host`` and ``blob`` up to every member added (a kernel still reading the old device tensor keeps it alive through
        the caching allocator's stream order)."""
        if self.host.size != self.words:
            host = np.zeros(self.words, dtype=np.int32)
            for off, h in self.parts:
                host[off:off + h.size] = h
            self.host, self.blob = host, torch.from_numpy(host).to(self.dev)


_LDS_FORMULA = '8 * (nnz(L+U) + dim + 8 N) bytes per grid'
_FD_LDS_FORMULA = "8 * (nnz_lu_p + dim_p + nnz_lu_pp + dim_pp + 6 N) bytes per grid: both factors of B' and B''"
_DC_LDS_FORMULA = "8 * (nnz_lu_p + dim_p + N) bytes per grid: the factor of B', its right-hand side and one bus vector"


# A solver as the launch code sees it: the prefix of its entry points, the class of its topologies, the LDS formula a refusal names
_Solver = namedtuple('_Solver', ['prefix', 'topology', 'formula'])
_NR = _Solver('gns_pf', PowerFlowTopology, _LDS_FORMULA)
_FD = _Solver('gns_fd', FdTopology, _FD_LDS_FORMULA)
_DC = _Solver('gns_dc', FdTopology, _DC_LDS_FORMULA)     # DC runs on the fast-decoupled analysis (_FD's caches), with its own LDS image
_DCN1_LDS_FORMULA = ("8 * (nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)) bytes per workgroup: DC's image, three doubles per line and "
                     "the right-hand sides of W outages side by side, here with W = 1, the narrowest")
_DCN1 = _Solver('gns_dcn1', FdTopology, _DCN1_LDS_FORMULA)   # the DC contingency screen: the same analysis again
_DCN2_LDS_FORMULA = ("8 * (nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)) bytes per workgroup of the factor kernel: the DC N-1 screen's image, "
                     "the right-hand sides of W candidate lines side by side, here with W = 1, the narrowest")
_DCN2 = _Solver('gns_dcn2', FdTopology, _DCN2_LDS_FORMULA)   # the DC N-2 screen: the N-1 screen's analysis and image
_DCG1_LDS_FORMULA = ("8 * (nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)) bytes per workgroup of the factor kernel: the DC N-1 screen's image, "
                     "the right-hand sides of W candidates (lines, then generators) side by side, here with W = 1, the narrowest")
_DCG1 = _Solver('gns_dcg1', FdTopology, _DCG1_LDS_FORMULA)   # the DC generator screen: the N-1 screen's analysis and image again
_ACN1 = _Solver('gns_acn1', PowerFlowTopology, _LDS_FORMULA)   # the AC contingency screen: Newton-Raphson's analysis and LDS image
_ACN2 = _Solver('gns_acn2', PowerFlowTopology, _LDS_FORMULA)   # the AC N-2 screen: the same analysis and image again
_ACG1 = _Solver('gns_acg1', PowerFlowTopology, _LDS_FORMULA)   # the AC generator screen: that analysis without the lost unit's row, one per unit
_DCN1_ADJOINT_LDS_FORMULA = ("8 * (nnz_lu_p + dim_p + N + 3 E + 2 dim_p (W + 1) + 3 W) bytes per workgroup: the screen's image, a second "
                             "array of W right-hand sides for the adjoint solves and three doubles per outage, here with W = 1, the "
                             "narrowest")


_DCN2_ADJOINT_LDS_FORMULA = ("max(8 * (nnz_lu_p + dim_p + N + 3 E + 2 dim_p (W + 1) + 3 W), 32 E) bytes per workgroup: the DC N-1 adjoint's image "
                             "(the screen's image and a second array of W right-hand sides) for the solves on the base factor, or "
                             "four doubles per line for the pair kernel, here with W = 1, the narrowest")


_DCG1_ADJOINT_LDS_FORMULA = ("max(8 * (nnz_lu_p + dim_p + N + 3 E + 2 dim_p (W + 1) + 3 W), 32 E) bytes per workgroup: the DC N-1 adjoint's image "
                             "(the screen's image and a second array of W right-hand sides) for the solves on the base factor (one "
                             "column per line, per generator and one more), or four doubles per line for the row kernel, here with "
                             "W = 1, the narrowest")


def _analysis(solver):
    """``(topology cache, set cache, analysis function)`` of a solver, as the module holds them when the call is made."""
    return (_FD_TOPO_CACHE, _FD_SET_CACHE, analyse_fd_topology) if solver is _FD else (_TOPO_CACHE, _SET_CACHE, analyse_topology)


def _check(rc, what, lds_bytes=None, formula=_LDS_FORMULA):
    """Raise GNSError for a non-zero return code.  A solve or adjoint call refuses a topology (GNS_EUNSUPPORTED) only for its LDS
    image: ``lds_bytes`` (the largest of a set's members, or a callable that finds it) is then named against the limit, not the
    GNS model text."""
    if rc == GNS_EUNSUPPORTED and lds_bytes is not None:
        lds_bytes = lds_bytes() if callable(lds_bytes) else lds_bytes
        raise _gns.GNSError(f'{what} failed: GNS_EUNSUPPORTED (the topology\'s LDS image of {int(lds_bytes)} B exceeds the '
                            f'{PF_LDS_MAX_BYTES} B (160 KiB) one workgroup may use: {formula})')
    if rc != 0:
        raise _gns.GNSError(f'{what} failed: {GNS_ERRORS.get(rc, rc)}')


def _set_lds_bytes(set_host, member_off, cls=PowerFlowTopology):
    """The largest LDS image among the members of a set (host words) of ``cls`` blobs."""
    lib, lds = load_library(), 0
    info, fn = cls.INFO(), cls.INFO_FN
    for off in member_off.tolist():
        _check(getattr(lib, fn)(set_host.ctypes.data + 4 * off, ctypes.byref(info)), fn)
        lds = max(lds, info.lds_bytes)
    return lds


def _dc_lds_bytes(host, member_off=(0,)):
    """The largest DC LDS image (``gns_dc_lds_bytes``) among the FD blobs at the word offsets ``member_off`` of ``host``."""
    lib, lds = load_library(), ctypes.c_int64()
    out = 0
    for off in member_off:
        _check(lib.gns_dc_lds_bytes(host.ctypes.data + 4 * int(off), ctypes.byref(lds)), 'gns_dc_lds_bytes')
        out = max(out, lds.value)
    return out


def _islanded(n_bus, f_bus, t_bus, slack):
    """0-based buses without a path of lines to the (0-based) slack."""
    adj = [[] for _ in range(n_bus)]
    for a, b in zip(f_bus.tolist(), t_bus.tolist()):
        adj[a].append(b)
        adj[b].append(a)
    seen = np.zeros(n_bus, dtype=bool)
    seen[slack] = True
    stack = [slack]
    while stack:
        i = stack.pop()
        for k in adj[i]:
            if not seen[k]:
                seen[k] = True
                stack.append(k)
    return np.flatnonzero(~seen)


def analyse_topology(n_bus, f_bus, t_bus, gen_bus, slack_bus, device=None, out_gen=None):
    """Analyse one topology from 1-based ``f_bus[E]``, ``t_bus[E]``, ``gen_bus[Gn]`` and the 1-based ``slack_bus`` (host arrays).
    Returns a ``PowerFlowTopology`` (its ``info`` dict holds the Jacobian dimension, nnz(L+U), ...); with ``device`` the blob is
    also copied there (on first use).  Raises ValueError for ids out of range or a slack that is not a bus, and its subclass
    ``IslandedTopology`` for buses islanded from the slack.

    ``out_gen``: a 0-based generator row that is out of service (``gns_pf_prepare_topology_out_gen``, what a row of
    ``ac_generator_contingency_screen`` is solved on): the row gives its bus no role and is left off the by-bus generator lists, which
    keep the others' row numbers; ``n_gen`` stays ``Gn``.  None or -1: the plain analysis, byte for byte."""
    return _analyse(n_bus, f_bus, t_bus, gen_bus, slack_bus, device, 'gns_pf', PowerFlowTopology, out_gen)


def analyse_fd_topology(n_bus, f_bus, t_bus, gen_bus, slack_bus, device=None):
    """The fast-decoupled analysis of one topology (arguments and errors as ``analyse_topology``): an ``FdTopology``."""
    return _analyse(n_bus, f_bus, t_bus, gen_bus, slack_bus, device, 'gns_fd', FdTopology)


def _analyse(n_bus, f_bus, t_bus, gen_bus, slack_bus, device, prefix, cls, out_gen=None):
    f = np.asarray(f_bus, dtype=np.float64).reshape(-1)
    t = np.asarray(t_bus, dtype=np.float64).reshape(-1)
    g = np.asarray(gen_bus, dtype=np.float64).reshape(-1)
    if not (np.all(f == np.round(f)) and np.all(t == np.round(t)) and np.all(g == np.round(g))):
        raise ValueError('bus id columns must hold integers')
    if f.size != t.size:
        raise ValueError('f_bus and t_bus differ in length')
    if min(f.min(initial=1), t.min(initial=1), g.min(initial=1)) < 1 or max(f.max(initial=1), t.max(initial=1), g.max(initial=1)) > n_bus:
        raise ValueError(f'bus ids must lie in 1..{n_bus}')
    s = float(slack_bus)
    if s != round(s) or not 1 <= s <= n_bus:
        raise ValueError(f'slack_bus = {slack_bus!r} is not a bus (1..{n_bus})')
    f32, t32, g32 = (np.ascontiguousarray(a - 1, dtype=np.int32) for a in (f, t, g))
    g_arg = g32 if g32.size else np.zeros(1, dtype=np.int32)
    slack = int(s) - 1
    lib = load_library()
    nbytes = ctypes.c_size_t()
    args = (int(n_bus), int(f32.size), int(g32.size), f32.ctypes.data, t32.ctypes.data, g_arg.ctypes.data, slack)
    suffix = ''
    if out_gen is not None:                  # the entry points that take the generator row that is out
        if out_gen != int(out_gen) or not -1 <= out_gen < g32.size:
            raise ValueError(f'out_gen = {out_gen!r} is not a generator row (0..{g32.size - 1}, or -1 for none)')
        args, suffix = (*args, int(out_gen)), '_out_gen'
    rc = getattr(lib, prefix + '_topology_bytes' + suffix)(*args, ctypes.byref(nbytes))
    if rc == GNS_ETOPOLOGY:
        isl = _islanded(int(n_bus), f32, t32, slack) + 1
        raise IslandedTopology(f'buses {isl.tolist()} have no path of lines to slack_bus {slack + 1}: their angles are undetermined '
                         '(the power-flow Jacobian is structurally singular)')
    if rc == GNS_EUNSUPPORTED:
        slots = ctypes.c_int64()
        _check(getattr(lib, prefix + '_topology_slots' + suffix)(*args, ctypes.byref(slots)), prefix + '_topology_slots' + suffix)
        raise _gns.GNSError(f'{prefix}_topology_bytes failed: GNS_EUNSUPPORTED (the factor of this topology needs {slots.value} slots, '
                            f'nnz(L+U) + dim, more than the {PF_MAX_SLOTS}-slot limit of the program\'s 16-bit operands)')
    _check(rc, prefix + '_topology_bytes')
    host = np.zeros(nbytes.value // 4, dtype=np.int32)
    _check(getattr(lib, prefix + '_prepare_topology' + suffix)(*args, host.ctypes.data, host.nbytes),
           prefix + '_prepare_topology' + suffix)
    return cls(host, device)


def _as_batch(buses, lines, generators, B, L, G):
    single = buses.dim() == 2
    if single:
        if lines.dim() != 2 or generators.dim() != 2:
            raise ValueError('buses, lines, generators must all be 2-D (one grid) or all 3-D (a batch)')
        buses, lines, generators = buses.unsqueeze(0), lines.unsqueeze(0), generators.unsqueeze(0)
    if not (buses.dim() == lines.dim() == generators.dim() == 3):
        raise ValueError('buses, lines, generators must all be 2-D (one grid) or all 3-D (a batch)')
    if not (buses.shape[0] == lines.shape[0] == generators.shape[0]) or buses.shape[0] == 0:
        raise ValueError('batch sizes of buses, lines, generators differ (or are zero)')
    buses, lines, generators = (_gns.GNS._remap(buses, B, _gns._B0), _gns.GNS._remap(lines, L, _gns._L0),
                                _gns.GNS._remap(generators, G, _gns._G0))
    if buses.shape[-1] != 6 or lines.shape[-1] != 7 or generators.shape[-1] != 7:
        raise ValueError('expected buses[...,6], lines[...,7], generators[...,7] (GNS/utils.py:4-13)')
    for name, t in (('buses', buses), ('lines', lines), ('generators', generators)):
        if t.dtype != torch.float32:
            raise ValueError(f'{name} must be float32')
    return single, buses, lines, generators


def _topology(buses, lines, gens, slack_bus):
    """The cached analysis of the batch's one topology.  One fused device compare of every grid's id columns against grid 0's,
    shipped to the host with grid 0's ids and type column: one synchronisation."""
    key, args = _topology_key(buses, lines, gens, slack_bus, 'newton_raphson')
    return _analysed(_NR, key, args, buses.device)


def _analysed(solver, key, args, device):
    """``solver``'s cached analysis of the topology ``_topology_key`` gave ``key`` and ``args`` for."""
    cache, _, analyse = _analysis(solver)
    topo = cache.get(key)
    if topo is None:
        topo = cache[key] = analyse(*args, device=device)
    return topo


def _topology_key(buses, lines, gens, slack_bus, solver):
    """The cache key of the batch's one topology (``_TOPO_CACHE``'s form) and the arguments of its analysis."""
    N, E, Gn = buses.shape[1], lines.shape[1], gens.shape[1]
    ids_l, ids_g = lines[0, :, 0:2], gens[0, :, 0]
    same = (lines[:, :, 0:2] == ids_l).all() & (gens[:, :, 0] == ids_g).all()
    host = torch.cat([same.to(torch.float64).reshape(1), ids_l.t().reshape(-1).double(), ids_g.double(),
                      buses[0, :, 1].double()]).cpu().numpy()
    if host[0] != 1.0:
        raise ValueError(f'f_bus / t_bus / generator bus columns differ across the batch: {solver} solves one topology per '
                         'call (group the grids by topology)')
    f_bus, t_bus, gen_bus, btype = host[1:1 + E], host[1 + E:1 + 2 * E], host[1 + 2 * E:1 + 2 * E + Gn], host[1 + 2 * E + Gn:]
    if slack_bus is None:
        slack_bus = _slack_from_type3(btype == 3)
    key = (N, E, Gn, slack_bus, str(buses.device), f_bus.tobytes(), t_bus.tobytes(), gen_bus.tobytes())
    return key, (N, f_bus, t_bus, gen_bus, slack_bus)


def _slack_from_type3(is3):
    """The 1-based slack from grid 0's buses of type 3 (a host bool array): there must be exactly one."""
    cand = np.flatnonzero(is3)
    if cand.size != 1:
        raise ValueError(f'slack_bus is not given and grid 0 has {cand.size} buses of type 3: pass slack_bus (1-based) '
                         'explicitly (synthetic grids write type 1 everywhere)')
    return int(cand[0]) + 1


def _plan_mixed(buses, lines, gens, slack_bus):
    """What a ``mixed_topologies`` call launches.  The grids are classified by id rows (``gns._classify_ids``: the call's one
    synchronisation, which also brings grid 0's type column when the slack is not given); each distinct topology is analysed once
    per ``(N, E, Gn, slack, device, ids)`` (``_TOPO_CACHE``; islanding ones are remembered in ``_ISLANDED``) and its blob added
    to the device set of ``(N, E, Gn, slack, device)``.  Returns a ``MixedPlan``:
      topology   [Bt] int64, device: each grid's index among the batch's distinct topologies
      order      [Bt] int32, device: the grids by topology (stable argsort), the order workgroups take them in
      grid_off   [Bt] int32, device: word offset of each grid's blob in the set, -1 for a topology that islands a bus
      member_off int32 numpy: the offsets of the blobs this call uses (distinct, ascending by topology index)
      topo_set   the ``_PfTopologySet``; slack_bus: the 1-based slack; islanded: bool numpy per distinct topology.
    Raises as ``analyse_topology`` does for ids out of range, non-integer ids or a bad slack; islands are not an error here."""
    return _planned(_NR, _classify(buses, lines, gens, slack_bus), buses, lines, gens)


def _planned(solver, classified, buses, lines, gens):
    """The ``MixedPlan`` of a classified batch on ``solver``'s blobs (its caches and analysis)."""
    return _plan_from(classified, buses, lines, gens, *_analysis(solver))


def _classify(buses, lines, gens, slack_bus):
    """The batch's distinct id rows (host), each grid's index among them (device) and the 1-based slack: one synchronisation."""
    if slack_bus is None:
        ids, inverse, _, is3 = _gns._classify_ids(lines, gens, extra=(buses[0, :, 1] == 3).to(torch.int64))
        slack_bus = _slack_from_type3(is3.numpy() != 0)
    else:
        ids, inverse, _ = _gns._classify_ids(lines, gens)
    return ids.numpy(), inverse.to(buses.device), slack_bus


def _plan_from(classified, buses, lines, gens, topo_cache, set_cache, analyse):
    """The ``MixedPlan`` of a classified batch on the analyses of ``topo_cache`` (made by ``analyse``) and a set of ``set_cache``."""
    ids_np, inverse, slack_bus = classified
    N, E, Gn = buses.shape[1], lines.shape[1], gens.shape[1]
    dev = buses.device
    set_key = (N, E, Gn, slack_bus, str(dev))
    topo_set = set_cache.get(set_key)
    if topo_set is None:
        topo_set = set_cache[set_key] = _PfTopologySet(dev)
    T = ids_np.shape[0]
    off = np.full(T, -1, dtype=np.int32)
    for k in range(T):
        f_bus, t_bus = (np.ascontiguousarray(ids_np[k, j:2 * E:2]) for j in (0, 1))
        gen_bus = np.ascontiguousarray(ids_np[k, 2 * E:])
        key = (N, E, Gn, slack_bus, str(dev), f_bus.tobytes(), t_bus.tobytes(), gen_bus.tobytes())
        if key in _ISLANDED:
            continue
        topo = topo_cache.get(key)
        if topo is None:
            try:
                topo = topo_cache[key] = analyse(N, f_bus, t_bus, gen_bus, slack_bus, device=dev)
            except IslandedTopology:
                _ISLANDED.add(key)
                continue
        off[k] = topo_set.add(key, topo)
    topo_set.sync()
    order = torch.argsort(inverse, stable=True).to(torch.int32)
    grid_off = torch.from_numpy(off).to(dev)[inverse].contiguous()
    return MixedPlan(inverse, order, grid_off, off[off >= 0].copy(), topo_set, slack_bus, off < 0)


def newton_raphson(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, v0=None, theta0=None, tol=1e-8,
                   max_iter=10, mixed_topologies=False):
    """Newton-Raphson AC power flow (polar, MATPOWER ``newtonpf``) of every grid of a batch that shares one topology, or with
    ``mixed_topologies=True`` of a batch whose id columns differ between grids.

    ``buses[Bt,N,6]``, ``lines[Bt,E,7]``, ``generators[Bt,Gn,7]``: float32, the tensors ``GNS.forward`` takes (per-unit powers,
    line shift in radians, tau as given); ``B, L, G`` column maps as in ``GNS.forward``; a 2-D single grid is accepted.
    ``slack_bus``: 1-based; by default the one bus of grid 0 whose type column is 3.  PV = every other bus with a generator,
    PQ = the rest.  Start: |V| = vg of the first generator listed on PV / slack buses, 1 elsewhere, theta = 0; a warm start
    ``v0`` / ``theta0 [Bt,N]`` sets |V| at PQ buses and theta (shifted so that theta_slack = 0).  ``||F||_inf < tol`` is tested
    before every update; at most ``max_iter`` updates.  Everything is computed in float64.

    Returns ``PowerFlowResult(v, theta, converged, iterations, mismatch)``: float64 ``[Bt,N]``, bool / int32 / float64 ``[Bt]``,
    on the inputs' device.  A grid that fails (zero or non-finite pivot, non-finite mismatch or iterate) has ``converged``
    False and keeps its last finite iterate; the other grids are unaffected, and every grid's result is bit-identical alone,
    in any batch and from run to run.

    ``mixed_topologies=True``: the batch is classified by id rows (one synchronisation) and solved in one launch, each grid on its
    own topology's blob; every grid's result is bit-identical to a plain call on its topology's grids.  The slack is one per call
    (given, or from grid 0's type column).  A grid whose topology leaves a bus without a path of lines to the slack is not solved:
    ``converged`` False, ``iterations`` -1, ``v`` / ``theta`` / ``mismatch`` NaN; the other grids are unaffected.  Without it a batch
    whose id columns differ, or an islanded topology, raises ValueError.

    Gradients: with grad mode on and ``requires_grad`` on any of ``buses`` / ``lines`` / ``generators``, ``v`` and ``theta`` are
    differentiable (``converged``, ``iterations``, ``mismatch`` are not).  The backward is exact at the returned solution (implicit
    function theorem in float64, one ``gns_pf_adjoint`` / ``gns_pf_adjoint_set`` launch on the forward's analysis, no host
    synchronisation): ``Pd, Qd, Gs, Bs``, the lines' ``r, x, b, tau, shift``, the generators' ``Pg`` and the ``vg`` of the first
    generator on a PV / slack bus; every other column gets 0.  A grid that did not converge (or is not solved) gets NaN gradient
    rows unless its incoming gradient is zero.  The forward outputs are bit-identical with and without gradients.  The warm
    start is not differentiated.  Contract: ``include/gns_powerflow.h``, "Gradients"."""
    single, in_dev, buses, lines, generators, v0, theta0 = _inputs(buses, lines, generators, B, L, G, v0, theta0, tol, max_iter,
                                                                   mixed_topologies)
    cfg = PfConfig(buses.shape[1], lines.shape[1], generators.shape[1], int(max_iter), float(tol))
    return _run(_NR, 'newton_raphson', cfg, buses, lines, generators, slack_bus, v0, theta0, mixed_topologies, in_dev, single)


def _inputs(buses, lines, generators, B, L, G, v0, theta0, tol, max_iter, mixed_topologies):
    """The checked inputs of a solver call: ``(single, input device, buses, lines, generators, v0, theta0)``, the tensors
    contiguous on the solve's device, the warm start float64 ``[Bt,N]`` there (both, or both None)."""
    single, buses, lines, generators = _as_batch(buses, lines, generators, B, L, G)
    if buses.device.type != 'cuda':
        if not torch.cuda.is_available():
            raise _gns.GNSError('the power-flow solver runs on a ROCm device only and none is visible (there is no CPU fallback)')
        dev = torch.device('cuda', torch.cuda.current_device())
    else:
        dev = buses.device
    in_dev = buses.device
    buses, lines, generators = (t.to(dev).contiguous() for t in (buses, lines, generators))
    Bt, N = buses.shape[0], buses.shape[1]
    _check_iteration(tol, max_iter)
    warm = v0 is not None or theta0 is not None
    if warm:
        def start(x, fill):
            if x is None:
                return torch.full((Bt, N), fill, dtype=torch.float64, device=dev)
            x = torch.as_tensor(x)
            x = x.unsqueeze(0) if (single and x.dim() == 1) else x
            if tuple(x.shape) != (Bt, N):
                raise ValueError(f'v0 / theta0 must be [{Bt},{N}], got {tuple(x.shape)}')
            return x.to(device=dev, dtype=torch.float64).contiguous()
        v0, theta0 = start(v0, 1.0), start(theta0, 0.0)
    if not isinstance(mixed_topologies, bool):
        raise ValueError(f'mixed_topologies must be a bool, got {mixed_topologies!r}')
    v0, theta0 = (v0, theta0) if warm else (None, None)
    return single, in_dev, buses, lines, generators, v0, theta0


def _check_iteration(tol, max_iter):
    """``tol`` and ``max_iter`` as every iterative solver and screen takes them."""
    if not (isinstance(max_iter, (int, np.integer)) and max_iter >= 0):
        raise ValueError(f'max_iter must be a non-negative integer, got {max_iter!r}')
    if not float(tol) >= 0.0:
        raise ValueError(f'tol must be >= 0, got {tol!r}')


def _run(solver, name, cfg, buses, lines, generators, slack_bus, v0, theta0, mixed_topologies, in_dev, single):
    """What ``newton_raphson`` and ``fast_decoupled`` (``name``) do with their checked inputs: the analysis of the batch's one
    topology, or with ``mixed_topologies`` its classification (one per call) and the ``MixedPlan`` on ``solver``'s blobs; the solve
    on it, through ``_NRFunction`` when an input requires grad; the result back on the input device.  The backward is the
    Newton-Raphson adjoint for either solver, so fast-decoupled then also gets the Newton-Raphson analysis of the same topologies."""
    lib = load_library()
    pf_cfg = cfg if solver is _NR else cfg.pf
    plain = (buses.detach(), lines.detach(), generators.detach())   # what the analysis reads (host copies of id columns)
    grad = torch.is_grad_enabled() and any(t.requires_grad for t in (buses, lines, generators))
    if mixed_topologies:
        classified = _classify(*plain, slack_bus)

        def target_of(s):
            plan = _planned(s, classified, *plain)
            ts = plan.topo_set                        # the set as this call sees it (a later call may grow it: offsets stay)
            return _set_members(plan, (ts.host, ts.blob), s.topology)
    else:
        key, args = _topology_key(*plain, slack_bus, name)

        def target_of(s):
            return _one_topology(_analysed(s, key, args, buses.device))
    target = target_of(solver)

    def solve(bu, li, ge):
        return _solve(lib, solver, cfg, target, bu, li, ge, v0, theta0)

    if grad:
        nr_target = target if solver is _NR else target_of(_NR)
        out = list(_NRFunction.apply(solve, lambda *args: _adjoint(lib, pf_cfg, nr_target, *args), buses, lines, generators))
    else:
        out = solve(*plain)
    if in_dev != buses.device:
        out = [t.to(in_dev) for t in out]
    if single:
        out = [t[0] for t in out]
    return PowerFlowResult(*out)


FD_VARIANTS = {'XB': 2, 'BX': 3}    # PYPOWER's PF_ALG


def fast_decoupled(buses, lines, generators, B=None, L=None, G=None, *, variant, slack_bus=None, v0=None, theta0=None, tol=1e-8,
                   max_iter=30, mixed_topologies=False):
    """Fast-decoupled AC power flow (PYPOWER ``makeB`` + ``fdpf``; ``runpf`` with ``PF_ALG`` 2 for ``variant='XB'``, 3 for
    ``'BX'``) of every grid of a batch, on the device.

    Inputs, column maps, the slack, PV / PQ roles, the start and the warm start, ``mixed_topologies`` and per-grid failure are those
    of ``newton_raphson``.  B' (PV+PQ buses: no shunts, no charging, tau 1, shifts kept, r = 0 with XB) and B'' (PQ buses: no
    shifts, r = 0 with BX) are factored once per grid; each iteration is a P half-step (theta -= B'^-1 P) and a Q half-step
    (|V| -= B''^-1 Q), each followed by the test ``max(||P||_inf, ||Q||_inf) < tol`` on the scaled mismatch
    ``(V conj(YV) - S) / |V|``, which is also tested at the start.  ``iterations`` counts P half-steps (at most ``max_iter``,
    PYPOWER's 30); ``mismatch`` is that scaled norm where the last test read it (NR reports the unscaled ``||F||_inf``).  A zero
    or non-finite pivot of either factor stops a grid at its start point unless the start already meets the test.

    Returns ``PowerFlowResult(v, theta, converged, iterations, mismatch)`` as ``newton_raphson`` does; a grid's result is
    bit-identical alone, in any batch and from run to run.

    Gradients: FD solves F = 0, the equations of ``newton_raphson``, so with grad mode on and ``requires_grad`` on an input ``v`` and
    ``theta`` are differentiable with NR's contract (its "Gradients" paragraph, include/gns_powerflow.h "Gradients"): the backward
    is one ``gns_pf_adjoint`` / ``gns_pf_adjoint_set`` launch on the Newton-Raphson analysis of the same topology, at FD's
    solution.  Contract: include/gns_powerflow.h, "Fast-decoupled"."""
    if variant not in FD_VARIANTS:
        raise ValueError(f"variant must be 'XB' or 'BX', got {variant!r}")
    single, in_dev, buses, lines, generators, v0, theta0 = _inputs(buses, lines, generators, B, L, G, v0, theta0, tol, max_iter,
                                                                   mixed_topologies)
    cfg = FdConfig(PfConfig(buses.shape[1], lines.shape[1], generators.shape[1], int(max_iter), float(tol)), FD_VARIANTS[variant])
    return _run(_FD, 'fast_decoupled', cfg, buses, lines, generators, slack_bus, v0, theta0, mixed_topologies, in_dev, single)


def dc_power_flow(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, mixed_topologies=False):
    """DC power flow (PYPOWER ``makeBdc`` + ``dcpf`` and the DC branch of ``runpf``) of every grid of a batch, on the device: the
    linear approximation a GNS is compared with next to Newton-Raphson.

    Inputs, column maps, the slack and ``mixed_topologies`` are those of ``newton_raphson``; PV and PQ buses are treated alike and
    there is no start to choose.  Per line ``b = 1 / (x tau)`` and ``Pfinj = -b shift``; ``Bbus`` gets ``+b`` at ff and tt, ``-b`` at
    ft and tf; ``P = sum Pg - Pd - Gs - Pbusinj``; ``theta`` is 0 at the slack and solves ``Bbus[r, r] theta_r = P_r`` elsewhere
    (float64, one sparse factorisation and one solve per grid).  ``r``, line charging and ``Bs`` are not used.

    Returns ``DcPowerFlowResult(v, theta, line_flow, slack_p, converged)``: float64 ``[Bt,N]``, ``[Bt,N]``, ``[Bt,E]``, ``[Bt]`` and
    bool ``[Bt]``, on the inputs' device.  ``v`` is 1; ``line_flow = b (theta_f - theta_t) + Pfinj`` is the active flow at each line's
    from end; ``slack_p = Bbus[slack, :] theta - P_slack`` is what the slack generates beyond its listed ``Pg``.  A grid with a zero or
    non-finite pivot or a non-finite ``theta`` (and, with ``mixed_topologies``, one whose topology islands a bus) has ``converged``
    False and NaN in ``theta``, ``line_flow`` and ``slack_p``; the other grids are unaffected, and every grid's result is
    bit-identical alone, in any batch, in any order and from run to run.

    The analysis is ``fast_decoupled``'s (B' has the sparsity of ``Bbus[r, r]``): a batch either of them has seen is not analysed
    again.  DC keeps less in LDS (the factor of B', its right-hand side, one bus vector), so it solves every topology
    ``fast_decoupled`` does, and larger ones.

    Gradients: with grad mode on and ``requires_grad`` on an input, ``theta``, ``line_flow`` and ``slack_p`` are differentiable: one
    ``gns_dc_adjoint`` / ``gns_dc_adjoint_set`` launch (a second solve on the same factor: the matrix is symmetric) gives the exact
    derivative with respect to ``Pd``, ``Gs``, the lines' ``x``, ``tau``, ``shift`` and the generators' ``Pg``; every other column
    gets 0.  A grid that is not solved gets NaN gradient rows unless all its incoming gradients are zero.  The forward outputs are
    bit-identical with and without gradients.  Contract: ``include/gns_powerflow.h``, "DC power flow"."""
    single, in_dev, buses, lines, generators, _, _ = _inputs(buses, lines, generators, B, L, G, None, None, 0.0, 0, mixed_topologies)
    lib = load_library()
    Bt, N = buses.shape[0], buses.shape[1]
    cfg = PfConfig(N, lines.shape[1], generators.shape[1], 0, 0.0)
    plain = (buses.detach(), lines.detach(), generators.detach())
    if mixed_topologies:
        plan = _planned(_FD, _classify(*plain, slack_bus), *plain)
        host, members = plan.topo_set.host, plan.member_off
        target = _set_members(plan, (host, plan.topo_set.blob), FdTopology)
        if target is not None:
            target = target._replace(lds=lambda: _dc_lds_bytes(host, members.tolist()))
    else:
        topo = _analysed(_FD, *_topology_key(*plain, slack_bus, 'dc_power_flow'), buses.device)
        target = _one_topology(topo)._replace(lds=_dc_lds_bytes(topo.host))

    def solve(bu, li, ge):
        return _dc_solve(lib, cfg, target, bu, li, ge)

    if torch.is_grad_enabled() and any(t.requires_grad for t in (buses, lines, generators)):
        out = list(_DCFunction.apply(solve, lambda *args: _dc_adjoint(lib, cfg, target, *args), buses, lines, generators))
    else:
        out = solve(*plain)
    out = [torch.ones(Bt, N, dtype=torch.float64, device=buses.device), *out]
    if in_dev != buses.device:
        out = [t.to(in_dev) for t in out]
    if single:
        out = [t[0] for t in out]
    return DcPowerFlowResult(*out)


class _DCFunction(torch.autograd.Function):
    """``dc_power_flow`` when an input requires grad, as ``_NRFunction``: the forward is the solve, the backward one adjoint launch on
    the forward's target."""

    @staticmethod
    def forward(ctx, solve, adjoint, buses, lines, gens):
        theta, flow, slack_p, conv = solve(buses, lines, gens)
        ctx.mark_non_differentiable(conv)
        ctx.set_materialize_grads(False)
        ctx.adjoint = adjoint
        ctx.save_for_backward(buses, lines, gens, theta, conv)
        return theta, flow, slack_p, conv

    @staticmethod
    @once_differentiable
    def backward(ctx, gth, gfl, gsp, _gconv):
        buses, lines, gens, theta, conv = ctx.saved_tensors
        grads = ctx.adjoint(buses, lines, gens, theta, conv, (gth, gfl, gsp), ctx.needs_input_grad[2:5])
        return (None, None, *grads)


def _dc_solve(lib, cfg, target, buses, lines, generators):
    """One DC solve launch (``gns_dc_solve[_set]``) on ``target``: ``[theta, line_flow, slack_p, converged]``."""
    Bt, N, E, dev = buses.shape[0], buses.shape[1], lines.shape[1], buses.device
    if target is None:                            # every topology islands a bus: no grid is solved
        nan = float('nan')
        return [torch.full((Bt, N), nan, dtype=torch.float64, device=dev), torch.full((Bt, E), nan, dtype=torch.float64, device=dev),
                torch.full((Bt,), nan, dtype=torch.float64, device=dev), torch.zeros(Bt, dtype=torch.bool, device=dev)]
    theta, flow = (torch.empty(Bt, n, dtype=torch.float64, device=dev) for n in (N, E))
    slack_p, conv = torch.empty(Bt, dtype=torch.float64, device=dev), torch.empty(Bt, dtype=torch.uint8, device=dev)
    _launch(lib, _DC, 'solve', cfg, target, (buses, lines, generators), (theta, flow, slack_p, conv))
    return [theta, flow, slack_p, conv.bool()]


def _dc_adjoint(lib, cfg, target, buses, lines, gens, theta, conv, incoming, need):
    """One DC adjoint launch (``gns_dc_adjoint[_set]``) on the forward's ``target``, ``incoming`` the gradients of ``theta``,
    ``line_flow`` and ``slack_p`` (None: zero); returns the gradients of the inputs ``need`` asks for."""
    Bt, dev = buses.shape[0], buses.device
    gin = [torch.empty_like(t) if n else None for t, n in zip((buses, lines, gens), need)]
    incoming = [None if g is None else g.to(device=dev, dtype=torch.float64).contiguous() for g in incoming]
    if target is None:
        return _unsolved_grads(gin, incoming, Bt, dev)
    _launch(lib, _DC, 'adjoint', cfg, target, (buses, lines, gens), (theta, conv, *incoming, *gin))
    return gin


_DCOPF_LDS_FORMULA = ("max(8 * (nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)) + 32 Gn, 8 * (Gn (Gn + 1) / 2 + 14 Gn + 10 E)) bytes per "
                      "workgroup: the DC N-1 screen's image with the solves of W units side by side (here W = 1, the narrowest) and "
                      "a generator block of zeros, or the interior point's packed Gn x Gn normal matrix and its iterate")
_DCOPF = _Solver('gns_dcopf', FdTopology, _DCOPF_LDS_FORMULA)   # the DC optimal power flow: the DC analysis and the screens' image


def _dcopf_cost(cost, Bt, Gn, single):
    """The checked cost: float64 ``[Gn,2]`` / ``[Bt,Gn,2]`` of ``(c2, c1)``, finite, ``c2 >= 0``."""
    if cost is None:
        raise ValueError('cost is required: float64 [Gn,2] or [Bt,Gn,2] of (c2, c1) per unit')
    c = torch.as_tensor(cost)
    if c.dtype != torch.float64:
        raise ValueError(f'cost must be float64, got {c.dtype}')
    if single and c.dim() == 3 and c.shape[0] == 1:
        c = c[0]
    if tuple(c.shape) not in ((Gn, 2), (Bt, Gn, 2)):
        raise ValueError(f'cost must be [{Gn},2] or [{Bt},{Gn},2], got {tuple(c.shape)}')
    if not bool(torch.isfinite(c).all()):
        raise ValueError('cost must be finite')
    if not bool((c[..., 0] >= 0).all()):
        raise ValueError('cost: c2 (column 0) must be >= 0')
    return c


def _dcopf_rating(rating, Bt, E, single):
    """The checked rating of the optimal power flow: None, or float64 ``[E]`` / ``[Bt,E]``, positive; ``+inf``: no limit there."""
    if rating is None:
        return None
    r = torch.as_tensor(rating)
    if r.dtype != torch.float64:
        raise ValueError(f'rating must be float64, got {r.dtype}')
    if single and r.dim() == 2 and r.shape[0] == 1:
        r = r[0]
    if tuple(r.shape) not in ((E,), (Bt, E)):
        raise ValueError(f'rating must be [{E}] or [{Bt},{E}], got {tuple(r.shape)}')
    if not bool((r > 0).all()):
        raise ValueError('rating must be positive (+inf: the line has no limit)')
    return r


def dc_optimal_power_flow(buses, lines, generators, B=None, L=None, G=None, *, cost, rating=None, slack_bus=None, tol=1e-8,
                          max_iter=150):
    """DC optimal power flow (PYPOWER ``dcopf`` / ``dcopf_solver`` without piecewise-linear costs) of every grid of a batch, on the
    device: the dispatch that is cheapest within the units' bounds and the lines' ratings, and what a megawatt costs at each bus.

    Inputs, column maps, the slack and single-grid handling are ``dc_power_flow``'s; the batch has one topology.  The dispatch of
    every listed unit is the variable: the listed ``Pg`` is ignored, the bounds are the ``Pmin`` and ``Pmax`` columns.  ``cost``:
    float64 ``[Gn,2]`` or ``[Bt,Gn,2]`` of ``(c2, c1)`` per unit, the objective ``sum_g c2_g p_g^2 + c1_g p_g`` in per-unit ``p``;
    ``c2 >= 0``, all entries finite (``c2 == 0`` everywhere is a linear program).  ``rating``: None, or float64 ``[E]`` / ``[Bt,E]``,
    positive; ``+inf`` (or None) means the line has no limit.  ``tol``: the termination tolerance; ``max_iter``: iterations allowed.

    Per grid, in float64: ``min f(p)`` subject to ``Bbus[r,r] theta_r = P_r(p)``, ``theta_slack = 0``, ``|b_l (theta_f - theta_t) +
    Pfinj_l| <= rating_l`` and ``Pmin <= p <= Pmax``, with ``b``, ``Pfinj``, ``Pbusinj`` and ``P = sum p - Pd - Gs - Pbusinj`` exactly
    ``dc_power_flow``'s.  A primal-dual interior point with PIPS's steps and termination, on the problem reduced to ``p`` by generator
    shift factors (one more solve on the base factor per unit); method and constants: ``include/gns_powerflow.h``, "DC optimal power
    flow".

    Returns ``DcOpfResult(pg, theta, line_flow, lmp, mu_line, mu_pmax, mu_pmin, objective, converged, iterations)`` on the inputs'
    device: ``pg`` float64 ``[Bt,Gn]``; ``theta`` ``[Bt,N]`` and ``line_flow`` ``[Bt,E]`` as ``dc_power_flow`` defines them at ``pg``
    (kept in float64); ``lmp`` ``[Bt,N]``, the derivative of the optimal cost with respect to ``Pd`` at each bus (energy plus
    congestion); ``mu_line`` ``[Bt,E]``, the multiplier of a line's upper limit minus that of its lower; ``mu_pmax``, ``mu_pmin``
    ``[Bt,Gn]`` ``>= 0``; ``objective`` ``[Bt]``, the cost at ``pg``; ``converged`` bool ``[Bt]``; ``iterations`` int32 ``[Bt]``.
    A grid that reaches ``max_iter`` (or meets a pivot that is not positive) keeps its last finite iterate with ``converged`` False.
    A grid is not solved (``iterations`` -1, NaN outputs) when its base factor fails, its data are not finite, some unit has
    ``Pmin >= Pmax`` or its demand lies outside ``[sum Pmin, sum Pmax]``; the other grids are unaffected, and every grid's result is
    bit-identical alone, in any batch, in any order and from run to run.  There is no host synchronisation after the analysis of
    the topology.  This call ignores ``requires_grad``; ``dc_optimal_power_flow_differentiable`` is the same call with a backward."""
    return _dc_opf(buses, lines, generators, B, L, G, cost, rating, slack_bus, tol, max_iter, False)


_DCOPF_ADJOINT_LDS_FORMULA = ("8 * (nnz_lu_p + dim_p + N + 3 E + 2 dim_p) + 32 Gn + 8 * (3 Gn + E + ceil((2 Gn + E) / 2) + n ((n + 1) | 1)) "
                              "bytes per workgroup: the DC N-1 screen's image at W = 1 and a generator block of zeros for the network "
                              "solves, the cotangents, and the dense KKT system of order n = free units + 1 + active lines with "
                              "its right-hand side, here with n = 0")


def _dc_opf(buses, lines, generators, B, L, G, cost, rating, slack_bus, tol, max_iter, differentiable):
    """``dc_optimal_power_flow`` and its differentiable twin: one set-up, the same launches."""
    _check_iteration(tol, max_iter)
    if differentiable and isinstance(lines, torch.Tensor) and lines.requires_grad:
        raise ValueError('dc_optimal_power_flow_differentiable does not differentiate with respect to lines (x, tau, shift): '
                         'detach them (their derivative is not zero, so it is not returned as zero)')
    grad = differentiable and torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                              for t in (buses, generators, cost, rating))
    with torch.no_grad():
        # the shapes first, so that a bad cost or rating is refused where no device is visible too
        single, shaped, shaped_lines, shaped_gens = _as_batch(buses, lines, generators, B, L, G)
        Bt, E, Gn = shaped.shape[0], shaped_lines.shape[1], shaped_gens.shape[1]
        if Gn == 0:
            raise ValueError('dc_optimal_power_flow needs at least one generator')
        cost_g, rating_g = (t if grad and isinstance(t, torch.Tensor) and t.requires_grad else None for t in (cost, rating))
        cost = _dcopf_cost(cost, Bt, Gn, single).detach()
        rating = _dcopf_rating(rating, Bt, E, single)
        rating = None if rating is None else rating.detach()
    with torch.set_grad_enabled(grad):
        if not grad:
            buses, generators = buses.detach(), generators.detach()
        single, in_dev, buses, lines, generators, _, _ = _inputs(buses, lines.detach(), generators, B, L, G, None, None, tol, max_iter,
                                                                 False)
        lib = load_library()
        N, dev = buses.shape[1], buses.device
        cfg = PfConfig(N, E, Gn, int(max_iter), float(tol))
        plain = (buses.detach(), lines, generators.detach())
        topo = _analysed(_FD, *_topology_key(*plain, slack_bus, 'dc_optimal_power_flow'), dev)
        lds = lambda: _screen_lds_bytes('gns_dcopf_lds_bytes', topo.host)[0]     # noqa: E731
        adjoint_lds = lambda: _screen_lds_bytes('gns_dcopf_adjoint_lds_bytes', topo.host)[0]     # noqa: E731
        cost, rating = cost.to(dev).contiguous(), None if rating is None else rating.to(dev).contiguous()

        def data():                      # (a closure, used as late as the backward: it keeps cost and rating alive)
            return cost.data_ptr(), int(cost.dim() == 3), _ptr(rating), int(rating is not None and rating.dim() == 2)

        f64 = dict(dtype=torch.float64, device=dev)

        def solve(bu, ge):
            pg, mu_pmax, mu_pmin = (torch.empty(Bt, Gn, **f64) for _ in range(3))
            theta, lmp = (torch.empty(Bt, N, **f64) for _ in range(2))
            flow, mu_line = (torch.empty(Bt, E, **f64) for _ in range(2))
            objective = torch.empty(Bt, **f64)
            conv, iters = torch.empty(Bt, dtype=torch.uint8, device=dev), torch.empty(Bt, dtype=torch.int32, device=dev)
            ws = _gns._workspace(_size_query(lib.gns_dcopf_workspace_bytes, 'gns_dcopf_workspace_bytes',
                                             (ctypes.byref(cfg), topo.host.ctypes.data, Bt), lds, _DCOPF.formula), dev)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                _check(lib.gns_dcopf_solve(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), lines.data_ptr(),
                                           ge.data_ptr(), Bt, *data(),
                                           *map(_ptr, (pg, theta, flow, lmp, mu_line, mu_pmax, mu_pmin, objective, conv, iters)),
                                           ws.data_ptr(), ws.numel(), stream), 'gns_dcopf_solve', lds, _DCOPF.formula)
            return [pg, theta, flow, lmp, mu_line, mu_pmax, mu_pmin, objective, conv.bool(), iters], conv

        def adjoint_workspace_bytes():
            return _size_query(lib.gns_dcopf_adjoint_workspace_bytes, 'gns_dcopf_adjoint_workspace_bytes',
                               (ctypes.byref(cfg), topo.host.ctypes.data, Bt), adjoint_lds, _DCOPF_ADJOINT_LDS_FORMULA)

        def adjoint(bu, ge, out, conv, incoming, need):
            gin = [torch.empty_like(bu) if need[0] else None, torch.empty_like(ge) if need[1] else None,
                   torch.empty(Bt, Gn, 2, **f64) if need[2] else None, torch.empty(Bt, E, **f64) if need[3] else None]
            incoming = [None if g is None else g.to(**f64).contiguous() for g in incoming]
            ws = _gns._workspace(adjoint_workspace_bytes(), dev)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                _check(lib.gns_dcopf_adjoint(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(),
                                             lines.data_ptr(), ge.data_ptr(), Bt, *data(), *map(_ptr, out[:8]), conv.data_ptr(),
                                             out[9].data_ptr(), *map(_ptr, incoming), *map(_ptr, gin), ws.data_ptr(), ws.numel(), stream),
                       'gns_dcopf_adjoint', adjoint_lds, _DCOPF_ADJOINT_LDS_FORMULA)
            return gin

        if grad:
            # the backward's own refusal comes before anything is launched; a shared cost or rating is expanded to per-grid form
            # here, so that autograd sums its gradient over the grids
            adjoint_workspace_bytes()
            if cost_g is not None:
                cost_g = cost_g.to(dev).reshape(cost.shape).expand(Bt, Gn, 2)
            if rating_g is not None:
                rating_g = rating_g.to(dev).reshape(rating.shape).expand(Bt, E)
            out = list(_DCOPFFunction.apply(solve, adjoint, buses, generators, cost_g, rating_g))
        else:
            out = solve(plain[0], plain[2])[0]
        if in_dev != dev:
            out = [t.to(in_dev) for t in out]
        if single:
            out = [t[0] for t in out]
        return DcOpfResult(*out)


class _DCOPFFunction(torch.autograd.Function):
    """``dc_optimal_power_flow_differentiable`` when an input requires grad: the forward is the plain call's launches, the backward one
    ``gns_dcopf_adjoint`` call on the forward's topology, inputs and returned tensors.  ``cost`` ``[Bt,Gn,2]`` and ``rating``
    ``[Bt,E]`` (None: no gradient wanted) are on the graph for their gradients alone: the kernels read the values the set-up
    uploaded."""

    @staticmethod
    def forward(ctx, solve, adjoint, buses, gens, cost, rating):
        out, conv = solve(buses, gens)
        ctx.mark_non_differentiable(out[8], out[9])
        ctx.set_materialize_grads(False)
        ctx.adjoint = adjoint
        ctx.save_for_backward(buses, gens, conv, *out)
        return tuple(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gout):
        buses, gens, conv, *out = ctx.saved_tensors
        return (None, None, *ctx.adjoint(buses, gens, out, conv, gout[:8], ctx.needs_input_grad[2:6]))


def dc_optimal_power_flow_differentiable(buses, lines, generators, B=None, L=None, G=None, *, cost, rating=None, slack_bus=None,
                                         tol=1e-8, max_iter=150):
    """``dc_optimal_power_flow`` with gradients: the same arguments, the same ``DcOpfResult`` with every output bit-identical to that
    call's (its forward is that call's launches), and a backward on the device: for a model trained against dispatch cost, a loss
    on locational prices, or the sensitivity of a dispatch to a load or a rating.

    With grad mode on and ``requires_grad`` on ``buses``, ``generators``, ``cost`` or ``rating``, the outputs ``pg``, ``theta``,
    ``line_flow``, ``lmp``, ``mu_line``, ``mu_pmax``, ``mu_pmin`` and ``objective`` are differentiable through one
    ``gns_dcopf_adjoint`` call on the forward's analysed topology, inputs and returned tensors (nothing else is saved, nothing is
    optimised again, the host is not synchronised): the optimum is differentiated by the implicit-function theorem on its KKT
    conditions, with the active rows held as equalities.  Per grid: the shift factors again (the forward's factor kernel), three
    solves on the base factor, and one dense LU with partial pivoting of order ``free units + 1 + active lines <= 2 Gn`` in LDS,
    exact for linear programs (``c2 == 0``) too.  Otherwise it is the plain call and returns plain tensors.

    The derivative is exact with respect to ``buses`` columns ``Pd`` (2) and ``Gs`` (4), ``generators`` columns ``Pmax`` (1) and
    ``Pmin`` (2) (every other column gets 0, the ignored ``Pg`` included), ``cost`` (``c2``, ``c1``) and ``rating`` (0 at ``+inf``);
    a shared ``cost [Gn,2]`` or ``rating [E]`` receives the sum over the grids.  ``lines`` are not differentiated: the call raises
    ``ValueError`` when ``lines.requires_grad`` rather than return zeros for a derivative that is not zero.  ``converged`` and
    ``iterations`` are not differentiable.

    A row is active when its multiplier exceeds its slack (``mu_line > max(rating - line_flow, 0)`` and so on), read from the returned
    tensors.  Near a degenerate optimum, where a row's slack and multiplier are both small, the optimum has no derivative: the
    gradient returned is that of the active set as classified, finite and not reliable.  A grid with ``iterations == -1``,
    ``converged`` False or a NaN output gets NaN gradient rows, and so does one whose KKT system exceeds the order the LDS image
    holds or meets a zero pivot; a grid whose incoming gradients are all zero (a loss that indexes it out) gets zero rows.  Other
    grids are unaffected, and a grid's gradient is bit-identical alone, in any batch, in any order and from run to run.

    Out of scope: gradients with respect to ``lines``, second derivatives, mixed topologies.
    Contract: ``include/gns_powerflow.h``, "DC optimal power flow: adjoint"."""
    return _dc_opf(buses, lines, generators, B, L, G, cost, rating, slack_bus, tol, max_iter, True)


_DCSCOPF_LDS_FORMULA = ("max(8 * (nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)) + 32 Gn, 8 * (Gn (Gn + 1) / 2 + 14 Gn + 10 E + 10 R + "
                        "ceil(E / 2))) bytes per workgroup: the DC optimal power flow's images with ten doubles per row slot and a flag "
                        "per line behind the iterate")


def _dcscopf_rows(rows, Bt, E, single):
    """The row list as an int tensor ``[R,2]`` or ``[Bt,R,2]`` of ``(l, k)``: the dtype and the shape, which need no device and no
    topology.  The rows themselves are ``_dcscopf_check_rows``'s."""
    if rows is None:
        raise ValueError('rows is required: int [R,2] or [Bt,R,2] of (monitored line, outaged line), (-1, -1) an empty slot')
    r = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows))
    if r.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'rows must hold integers (0-based (monitored line, outaged line) pairs), got dtype {r.dtype}')
    if single and r.dim() == 3 and r.shape[0] == 1:
        r = r[0]
    if r.dim() not in (2, 3) or r.shape[-1] != 2 or r.shape[-2] < 1 or (r.dim() == 3 and r.shape[0] != Bt):
        raise ValueError(f'rows must be [R,2] or [{Bt},R,2] with R >= 1, got {tuple(r.shape)}')
    return r


def _dcscopf_check_rows(r, E, bridges):
    """A row list on the CPU (``_dcscopf_rows``' tensor) against the topology, in one pass: every row that is not ``(-1, -1)`` lies in
    range, has ``l != k`` and does not outage a bridge (``bridges``: bool ``[E]``).  The first row that does not is named.  A tensor
    on a device is not looked at: the kernel's rule applies, a bad row fails its grid."""
    if r.device.type != 'cpu':
        return
    a = r.numpy().reshape(-1, 2)
    l, k = a[:, 0], a[:, 1]
    in_range = (l >= 0) & (l < E) & (k >= 0) & (k < E)
    bridge = np.zeros(a.shape[0], dtype=bool)
    bridge[in_range] = np.asarray(bridges, dtype=bool)[k[in_range]]
    bad = np.flatnonzero(((l != -1) | (k != -1)) & (~in_range | (l == k) | bridge))
    if bad.size == 0:
        return
    i = int(bad[0])
    where = f'rows{[i] if r.dim() == 2 else [i // r.shape[1], i % r.shape[1]]} = ({int(l[i])}, {int(k[i])})'
    if not in_range[i]:
        raise ValueError(f'{where}: both must lie in 0..{E - 1} (0-based line indices; (-1, -1) is an empty slot)')
    if l[i] == k[i]:
        raise ValueError(f'{where}: the monitored line is the outaged line')
    raise ValueError(f'{where}: the outage of line {int(k[i])} disconnects the grid (it is a bridge of the topology)')


def dc_security_constrained_opf(buses, lines, generators, B=None, L=None, G=None, *, cost, rows, rating=None, contingency_rating=None,
                                slack_bus=None, tol=1e-8, max_iter=150):
    """``dc_optimal_power_flow`` with contingency rows: the cheapest dispatch within the units' bounds, the lines' ratings and, for
    every listed row ``(l, k)``, the limit on line ``l``'s flow after the outage of line ``k``, on the device.

    Inputs, ``cost``, ``rating``, ``tol`` and ``max_iter`` are ``dc_optimal_power_flow``'s.  ``rows``: an int tensor or array ``[R,2]``
    (one list for the batch) or ``[Bt,R,2]`` (a list per grid) of 0-based ``(monitored line, outaged line)``; ``(-1, -1)`` is an empty
    slot, ``R >= 1``.  A list on the CPU is checked here (range, ``l != k``, ``k`` not a bridge of the topology) and refused with a
    ``ValueError`` that names the row; a tensor on the device is passed through without a synchronisation, and a bad row then fails
    its grid alone.  ``contingency_rating``: the post-outage (emergency) rating of the monitored line, float64 ``[E]`` / ``[Bt,E]``,
    positive, ``+inf``: rows on that line constrain nothing; None: ``rating`` is used.

    Per row ``|F_l + L_r F_k| <= contingency_rating_l`` with ``F`` the base flows and ``L_r = b_l (z_k[f_l] - z_k[t_l]) /
    (1 - b_k d_k)`` the line-outage factor of ``dc_contingency_screen``: a row is a combination of two rows of the shift-factor
    matrix, so the interior point still works on a ``Gn x Gn`` matrix.  Method and constants are ``dc_optimal_power_flow``'s; the
    rows follow the lines' rows (``include/gns_powerflow.h``, "Security-constrained DC optimal power flow").

    Returns ``DcScopfResult``: ``DcOpfResult``'s ten fields, ``mu_row`` ``[Bt,R]`` (the multiplier of a row's upper side minus that of
    its lower, 0 in an empty slot) and ``row_flow`` ``[Bt,R]`` (the post-outage flow at ``pg``, NaN in an empty slot).  ``lmp`` stays
    the derivative of the optimal cost with respect to ``Pd``, the rows' congestion included.  With every slot empty the ten fields
    are ``dc_optimal_power_flow``'s bit for bit.  A grid is not solved (``iterations`` -1, NaN outputs) under
    ``dc_optimal_power_flow``'s rules or when a row of a device list is out of range, has ``l == k``, outages a bridge, or has a
    zero or non-finite denominator; the other grids are unaffected, and a grid's result is bit-identical alone, in any batch, with
    ``rows`` and the ratings shared or per grid, and from run to run.  Gradients, mixed topologies, generator outages as
    constraints and corrective re-dispatch are out of scope."""
    _check_iteration(tol, max_iter)
    with torch.no_grad():
        single, shaped, shaped_lines, shaped_gens = _as_batch(buses, lines, generators, B, L, G)
        Bt, E, Gn = shaped.shape[0], shaped_lines.shape[1], shaped_gens.shape[1]
        if Gn == 0:
            raise ValueError('dc_security_constrained_opf needs at least one generator')
        # the shapes first, so that a bad cost, rating or row list is refused where no device is visible too
        cost = _dcopf_cost(cost, Bt, Gn, single).detach()
        rating = _dcopf_rating(rating, Bt, E, single)
        rating_c = _dcopf_rating(contingency_rating, Bt, E, single)
        rows = _dcscopf_rows(rows, Bt, E, single)
        single, in_dev, buses, lines, generators, _, _ = _inputs(buses.detach(), lines.detach(), generators.detach(), B, L, G, None, None,
                                                                 tol, max_iter, False)
        lib = load_library()
        N, dev = buses.shape[1], buses.device
        cfg = PfConfig(N, E, Gn, int(max_iter), float(tol))
        key, args = _topology_key(buses, lines, generators, slack_bus, 'dc_security_constrained_opf')
        topo = _analysed(_FD, key, args, dev)
        bridges = _topology_bridges(topo, args)
        _dcscopf_check_rows(rows, E, bridges)
        rows = rows.to(device=dev, dtype=torch.int32).contiguous()
        R = rows.shape[-2]
        if getattr(topo, 'bridges_dev', None) is None:
            topo.bridges_dev = torch.from_numpy(bridges.astype(np.uint8)).to(dev)
        cost = cost.to(dev).contiguous()
        rating, rating_c = (None if t is None else t.detach().to(dev).contiguous() for t in (rating, rating_c))

        def lds():
            b = ctypes.c_int64()
            _check(lib.gns_dcscopf_lds_bytes(topo.host.ctypes.data, R, ctypes.byref(b), None), 'gns_dcscopf_lds_bytes')
            return b.value

        f64 = dict(dtype=torch.float64, device=dev)
        pg, mu_pmax, mu_pmin = (torch.empty(Bt, Gn, **f64) for _ in range(3))
        theta, lmp = (torch.empty(Bt, N, **f64) for _ in range(2))
        flow, mu_line = (torch.empty(Bt, E, **f64) for _ in range(2))
        mu_row, row_flow = (torch.empty(Bt, R, **f64) for _ in range(2))
        objective = torch.empty(Bt, **f64)
        conv, iters = torch.empty(Bt, dtype=torch.uint8, device=dev), torch.empty(Bt, dtype=torch.int32, device=dev)
        ws = _gns._workspace(_size_query(lib.gns_dcscopf_workspace_bytes, 'gns_dcscopf_workspace_bytes',
                                         (ctypes.byref(cfg), topo.host.ctypes.data, Bt, R), lds, _DCSCOPF_LDS_FORMULA), dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib.gns_dcscopf_solve(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), buses.data_ptr(),
                                         lines.data_ptr(), generators.data_ptr(), Bt, cost.data_ptr(), int(cost.dim() == 3),
                                         _ptr(rating), int(rating is not None and rating.dim() == 2), rows.data_ptr(),
                                         int(rows.dim() == 3), R, _ptr(rating_c), int(rating_c is not None and rating_c.dim() == 2),
                                         topo.bridges_dev.data_ptr(),
                                         *map(_ptr, (pg, theta, flow, lmp, mu_line, mu_pmax, mu_pmin, objective, conv, iters, mu_row,
                                                     row_flow)), ws.data_ptr(), ws.numel(), stream),
                   'gns_dcscopf_solve', lds, _DCSCOPF_LDS_FORMULA)
        out = [pg, theta, flow, lmp, mu_line, mu_pmax, mu_pmin, objective, conv.bool(), iters, mu_row, row_flow]
        if in_dev != dev:
            out = [t.to(in_dev) for t in out]
        if single:
            out = [t[0] for t in out]
        return DcScopfResult(*out)


def dc_secure_dispatch(buses, lines, generators, B=None, L=None, G=None, *, cost, rating=None, contingency_rating=None, outages=None,
                       rounds=4, rows_per_round=8, violation_tol=1e-5, slack_bus=None, tol=1e-8, max_iter=150):
    """The cheapest dispatch that survives every single-line outage of ``outages``: constraint generation around
    ``dc_security_constrained_opf`` and ``dc_contingency_screen`` with static shapes, on the device.

    ``R = rounds * rows_per_round`` row slots per grid start empty.  Each of the ``rounds`` rounds solves with the rows listed so
    far, writes the dispatch into the generators' ``Pg`` column, screens the outages, forms the loading ``|flow| /
    contingency_rating`` of every (monitored line, outage) pair (the outaged line itself, islanding outages, lines without a rating
    and the pairs already listed masked), takes the ``rows_per_round`` worst per grid and writes those above ``1 + violation_tol`` into
    the round's slots; the others stay ``(-1, -1)``.  A last solve takes all the rows, and a last screen gives ``worst_loading`` ``[Bt]``
    over all outages and ``secure = worst_loading <= 1 + violation_tol``.  ``outages``: as ``dc_contingency_screen``'s, None: every
    line that is not a bridge (the bridges are never launched).  ``contingency_rating``: as ``dc_security_constrained_opf``'s (None: ``rating``; one of the two is needed).

    The screen reads the dispatch rounded to float32 (the generator rows are float32), so its loadings carry that rounding:
    ``violation_tol`` is the caller's overload tolerance and must sit above it (the default 1e-5 does for per-unit flows of order
    1).  A grid that is secure from the start keeps every slot empty and returns ``dc_optimal_power_flow``'s bits.  A grid that is still
    insecure after the last round has ``secure`` False: give it more rounds or rows.  The driver's own steps (the
    write of ``Pg``, the loadings, the masks, ``topk``, the slots) read nothing back to the host; each solve and each screen makes
    the one synchronisation of its topology lookup (the id columns against the cached analysis), as every call of this module does.
    Gradients of the secure dispatch are out of scope.

    Returns ``DcSecureDispatch(result, rows, worst_loading, secure)``: the last solve's ``DcScopfResult``, ``rows`` int32 ``[Bt,R,2]``,
    ``worst_loading`` float64 ``[Bt]`` and ``secure`` bool ``[Bt]``."""
    for name, v in (('rounds', rounds), ('rows_per_round', rows_per_round)):
        if not (isinstance(v, (int, np.integer)) and v >= 1):
            raise ValueError(f'{name} must be a positive integer, got {v!r}')
    if not float(violation_tol) >= 0.0:
        raise ValueError(f'violation_tol must be >= 0, got {violation_tol!r}')
    with torch.no_grad():
        single, in_dev, buses, lines, generators, _, _ = _inputs(buses.detach(), lines.detach(), generators.detach(), B, L, G, None, None,
                                                                 tol, max_iter, False)
        Bt, E, dev = buses.shape[0], lines.shape[1], buses.device
        rc = _dcopf_rating(contingency_rating if contingency_rating is not None else rating, Bt, E, single)
        if rc is None:
            raise ValueError('dc_secure_dispatch needs contingency_rating or rating: without one no outage can overload a line')
        rc = rc.detach().to(dev).reshape(-1, 1, E)                    # [1 or Bt, 1, E]
        R = int(rounds) * int(rows_per_round)
        rows = torch.full((Bt, R, 2), -1, dtype=torch.int32, device=dev)
        gens = generators.clone()
        if outages is None:
            key, args = _topology_key(buses, lines, generators, slack_bus, 'dc_secure_dispatch')
            outages = np.flatnonzero(~_topology_bridges(_analysed(_FD, key, args, dev), args))
            if outages.size == 0:
                raise ValueError('dc_secure_dispatch: every line is a bridge of the topology, no outage can be screened')
        listed = lines_t = isl = None
        thr = 1.0 + float(violation_tol)

        def solve():
            return dc_security_constrained_opf(buses, lines, generators, cost=cost, rows=rows, rating=rating,
                                               contingency_rating=contingency_rating, slack_bus=slack_bus, tol=tol, max_iter=max_iter)

        def loading(res):
            """[Bt,K,E]: the loading of every pair at the dispatch of res, -1 where the pair cannot be a row"""
            nonlocal lines_t, isl
            gens[..., 6] = res.pg.float()
            sc = dc_contingency_screen(buses, lines, gens, slack_bus=slack_bus, outages=outages, flows=True)
            if lines_t is None:
                lines_t, isl = sc.outages.to(dev), sc.islanding.to(dev)
                if rows_per_round > lines_t.numel() * E:
                    raise ValueError(f'rows_per_round {rows_per_round} exceeds the {lines_t.numel() * E} (line, outage) pairs')
            load = sc.line_flow.abs() / rc
            own = torch.arange(E, device=dev).reshape(1, 1, E) == lines_t.reshape(1, -1, 1)
            return torch.where(own | isl.reshape(1, -1, 1) | torch.isinf(rc), load.new_full((), -1.0), load)

        for i in range(int(rounds)):
            load = loading(solve())
            if listed is None:
                listed = torch.zeros(Bt, lines_t.numel() * E, dtype=torch.bool, device=dev)
            val, idx = torch.topk(torch.where(listed, load.new_full((), -1.0), load.reshape(Bt, -1)), int(rows_per_round), dim=1)
            above = val > thr
            pair = torch.stack([idx % E, lines_t[idx // E]], dim=-1).to(torch.int32)
            rows[:, i * rows_per_round:(i + 1) * rows_per_round] = torch.where(above.unsqueeze(-1), pair, pair.new_full((), -1))
            listed.scatter_(1, idx, above | listed.gather(1, idx))
        res = solve()
        load = loading(res).reshape(Bt, -1)
        # (a NaN loading, of a grid without a dispatch, is the worst of all)
        worst = torch.where(torch.isnan(load).any(dim=1), load.new_full((), float('nan')), load.amax(dim=1))
        secure = worst <= thr
        out_rows = rows
        if in_dev != dev:
            res = DcScopfResult(*(t.to(in_dev) for t in res))
            out_rows, worst, secure = out_rows.to(in_dev), worst.to(in_dev), secure.to(in_dev)
        if single:
            res = DcScopfResult(*(t[0] for t in res))
            out_rows, worst, secure = out_rows[0], worst[0], secure[0]
        return DcSecureDispatch(res, out_rows, worst, secure)


def _dcn1_lds_bytes(host):
    """``(LDS image, W)`` of the DC contingency screen (``gns_dcn1_lds_bytes``) on the FD blob ``host``: W outages side by side, the
    largest power of two up to 64 whose image fits (W = 1's image when none does)."""
    return _screen_lds_bytes('gns_dcn1_lds_bytes', host)


def _screen_lds_bytes(query, host):
    """``(LDS image, W)`` as the entry point ``query`` gives them for the FD blob ``host``."""
    lds, lanes = ctypes.c_int64(), ctypes.c_int32()
    _check(getattr(load_library(), query)(host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)), query)
    return lds.value, lanes.value


def _bridges(n_bus, f_bus, t_bus):
    """bool ``[E]``: the lines (0-based ends) whose removal disconnects the graph they span.  One depth-first search with low
    points (linear time); the line a bus was reached by is skipped by index, so a parallel line is never a bridge, and a line from
    a bus to itself is not in the graph."""
    f, t = np.asarray(f_bus).tolist(), np.asarray(t_bus).tolist()
    adj = [[] for _ in range(n_bus)]
    for e, (a, b) in enumerate(zip(f, t)):
        if a != b:
            adj[a].append((b, e))
            adj[b].append((a, e))
    bridge = np.zeros(len(f), dtype=bool)
    disc, low = [-1] * n_bus, [0] * n_bus
    clock = 0
    for root in range(n_bus):
        if disc[root] >= 0:
            continue
        disc[root] = low[root] = clock
        clock += 1
        stack = [(root, -1, iter(adj[root]))]
        while stack:
            i, via, it = stack[-1]
            for k, e in it:
                if e == via:
                    continue
                if disc[k] >= 0:
                    low[i] = min(low[i], disc[k])
                    continue
                disc[k] = low[k] = clock
                clock += 1
                stack.append((k, e, iter(adj[k])))
                break
            else:
                stack.pop()
                if stack:
                    parent = stack[-1][0]
                    low[parent] = min(low[parent], low[i])
                    if low[i] > disc[parent]:
                        bridge[via] = True
    return bridge


def _topology_bridges(topo, args):
    """The bridges of an analysed topology (``_bridges``), found once and kept with it.  The analysis has shown the topology
    connected, so these are exactly the lines whose outage leaves a bus without a path to the slack (``_islanded``)."""
    if getattr(topo, 'bridges', None) is None:
        n_bus, f_bus, t_bus = args[0], args[1], args[2]
        topo.bridges = _bridges(int(n_bus), f_bus.astype(np.int64) - 1, t_bus.astype(np.int64) - 1)
    return topo.bridges


def _outage_list(outages, E):
    """The checked outage list as an int64 numpy array ``[K]``."""
    if outages is None:
        return np.arange(E, dtype=np.int64)
    o = outages.detach().cpu().numpy() if isinstance(outages, torch.Tensor) else np.asarray(list(outages) if isinstance(outages, range)
                                                                                            else outages)
    if o.ndim != 1:
        raise ValueError(f'outages must be a 1-D sequence of line indices, got shape {tuple(o.shape)}')
    if o.size == 0:
        raise ValueError('outages is empty: give at least one line index (None: every line)')
    if o.dtype == np.bool_ or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f'outages must hold integers (0-based line indices), got dtype {o.dtype}')
    if o.min() < 0 or o.max() > E - 1:
        raise ValueError(f'outages must lie in 0..{E - 1} (0-based line indices), got {int(o.min())}..{int(o.max())}')
    return o.astype(np.int64)


def _rating(rating, Bt, E, single):
    """The checked rating: None, or float64 ``[E]`` / ``[Bt,E]``."""
    if rating is None:
        return None
    r = torch.as_tensor(rating).to(torch.float64)
    if single and r.dim() == 2 and r.shape[0] == 1:
        r = r[0]
    if tuple(r.shape) not in ((E,), (Bt, E)):
        raise ValueError(f'rating must be [{E}] or [{Bt},{E}], got {tuple(r.shape)}')
    if not bool((torch.isfinite(r) & (r > 0)).all()):
        raise ValueError('rating must be positive and finite')
    return r


def _dcn1_adjoint_lds_bytes(host):
    """``(LDS image, W)`` of the screen's adjoint (``gns_dcn1_adjoint_lds_bytes``) on the FD blob ``host``, as ``_dcn1_lds_bytes``."""
    return _screen_lds_bytes('gns_dcn1_adjoint_lds_bytes', host)


def _screen_setup(name, solver, buses, lines, generators, B, L, G, slack_bus, rows, rating, flags, differentiable, tol=0.0,
                  max_iter=0, pickup=None):
    """What the contingency screens do before their own launches, in the order their refusals are raised: the bool ``flags``
    (a dict by name), ``tol`` / ``max_iter`` (the DC screens' never fail) and ``differentiable`` (False from a screen without
    gradients); whether the call is differentiated (``grad``); the shapes, the list ``rows`` (outages, pairs for a screen named
    ``*_n2_*``, or (generator, line) rows for one named ``*_generator_*``, which also takes ``pickup``) and the rating, checked where
    no device is visible too; ``_inputs``; ``solver``'s cached analysis of the one topology; the islanding mask of the list, on the
    host (``isl_np``) and uploaded (``isl_dev``).  Returns a namespace of these and of the shapes, the configuration ``cfg`` and the
    detached inputs ``plain``.  The caller goes on under ``torch.set_grad_enabled(s.grad)``."""
    for flag, value in flags.items():
        if not isinstance(value, bool):
            raise ValueError(f'{flag} must be a bool, got {value!r}')
    _check_iteration(tol, max_iter)                  # (_inputs' checks, here before a device is needed)
    if not isinstance(differentiable, bool):
        raise ValueError(f'differentiable must be a bool, got {differentiable!r}')
    s = SimpleNamespace()
    s.grad = differentiable and torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                                for t in (buses, lines, generators, pickup))
    pairs, generator = '_n2_' in name, '_generator_' in name
    with torch.no_grad():
        # the shapes first, so that a bad list or rating is refused where no device is visible too
        single, shaped, shaped_lines, shaped_gens = _as_batch(buses, lines, generators, B, L, G)
        E = shaped_lines.shape[1]
        if generator:
            s.rows = _generator_contingency_list(rows, shaped_gens.shape[1], E)
            pickup = _pickup(pickup, shaped_gens, single)
        else:
            s.rows = _pair_list(rows, E, name.replace('_n2', '')) if pairs else _outage_list(rows, E)
        rating = _rating(rating, shaped.shape[0], E, single)
    with torch.set_grad_enabled(s.grad):
        if not s.grad:
            buses, lines, generators = buses.detach(), lines.detach(), generators.detach()
        s.single, s.in_dev, s.buses, s.lines, s.generators, _, _ = _inputs(buses, lines, generators, B, L, G, None, None, tol, max_iter,
                                                                           False)
        s.lib = load_library()
        s.Bt, s.N, s.E, s.dev = s.buses.shape[0], s.buses.shape[1], s.lines.shape[1], s.buses.device
        s.rating = None if rating is None else rating.to(s.dev).contiguous()
        s.pickup = None if pickup is None else pickup.to(s.dev).contiguous()
        s.cfg = PfConfig(s.N, s.E, s.generators.shape[1], int(max_iter), float(tol))
        s.plain = (s.buses.detach(), s.lines.detach(), s.generators.detach())
        key, args = s.topo_key, s.topo_args = _topology_key(*s.plain, slack_bus, name)
        s.topo = _analysed(solver, key, args, s.dev)
        if generator:
            s.isl_np = _generator_islanding(_topology_bridges(s.topo, args), s.rows)
        else:
            s.isl_np = _topology_pair_islanding(s.topo, args, s.rows) if pairs else _topology_bridges(s.topo, args)[s.rows]
        s.isl_dev = torch.from_numpy(s.isl_np.astype(np.uint8)).to(s.dev)
    return s


def _upload32(a, dev):
    """An index list as the C calls take it: contiguous int32 on the host, and its copy on the device."""
    host = np.ascontiguousarray(a.astype(np.int32))
    return host, torch.from_numpy(host).to(dev)


def _shared_args(s, *lists):
    """``shared()`` gives what every C call of a screen takes between Bt and its own arguments: each of ``lists`` (``_upload32``'s
    pairs) on the host and on the device with its length, the islanding mask, the rating and whether it is per grid.  (A closure,
    used as late as the backward: it keeps their owners alive.)"""
    def shared():
        return (*(x for host, dev in lists for x in (host.ctypes.data, dev.data_ptr(), host.shape[0])), s.isl_dev.data_ptr(),
                _ptr(s.rating), int(s.rating is not None and s.rating.dim() == 2))
    return shared


def _screen_workspace_bytes(s, query, counts, lds, formula):
    """The bytes the workspace query ``query`` of a screen asks for: it takes the configuration, the host blob, Bt and ``counts``."""
    return _size_query(getattr(s.lib, query), query, (ctypes.byref(s.cfg), s.topo.host.ctypes.data, s.Bt, *counts), lds, formula)


def _screen_results(s, base, res, conv_at):
    """The tail of a screen: ``(base, list, res, islanding)`` on the input device, ``res[conv_at]`` (``converged``, uint8) as bool, and
    without the batch dimension for a single grid.  ``res`` holds ``[Bt, ...]`` tensors or None."""
    res[conv_at] = res[conv_at].bool()
    rows_t, islanding = torch.from_numpy(s.rows).to(s.dev), torch.from_numpy(s.isl_np.copy()).to(s.dev)
    if s.in_dev != s.dev:
        base = [t.to(s.in_dev) for t in base]
        res = [None if t is None else t.to(s.in_dev) for t in res]
        rows_t, islanding = rows_t.to(s.in_dev), islanding.to(s.in_dev)
    if s.single:
        base = [t[0] for t in base]
        res = [None if t is None else t[0] for t in res]
    return base, rows_t, res, islanding


def _dc_screen(s, solver, shared, n_rows, counts, adjoint_counts, adjoint_lds_bytes, adjoint_formula, flows, pickup_grad=False,
               weights=None):
    """The DC screens after ``_screen_setup``: ``solver``'s screen launch (with its adjoint through ``_DCN1Function`` when the call is
    differentiated) and the base case.  ``shared``: ``_shared_args``'s closure; ``n_rows``: the rows per grid; ``counts`` /
    ``adjoint_counts``: what the two workspace queries take after Bt; ``adjoint_lds_bytes`` / ``adjoint_formula``: the adjoint's LDS
    query and the formula its refusal names (None for a screen without gradients: the call is then never differentiated);
    ``pickup_grad``: the adjoint has a fourth output after the three inputs', the generator screen's ``grad_pickup`` ``[Bt,Gn]``
    float64; ``weights``: the pickup weights ``[Gn]`` / ``[Bt,Gn]`` float64 on the autograd graph when they take that gradient
    (``grad_pickup`` is NULL otherwise).  Returns ``(base, [line_flow, worst_loading, worst_line, converged])``."""
    lib, cfg, topo, Bt, dev = s.lib, s.cfg, s.topo, s.Bt, s.dev
    lds = lambda: _dcn1_lds_bytes(topo.host)[0]                              # noqa: E731
    adjoint_lds = lambda: adjoint_lds_bytes(topo.host)[0]                    # noqa: E731
    name, adjoint_name = solver.prefix + '_screen', solver.prefix + '_adjoint'

    def adjoint_workspace_bytes():
        return _screen_workspace_bytes(s, adjoint_name + '_workspace_bytes', adjoint_counts, adjoint_lds, adjoint_formula)

    def screen(bu, li, ge):
        flow = torch.empty(Bt, n_rows, s.E, dtype=torch.float64, device=dev) if flows else None
        worst = torch.empty(Bt, n_rows, dtype=torch.float64, device=dev)
        worst_line = torch.empty(Bt, n_rows, dtype=torch.int32, device=dev)
        conv = torch.empty(Bt, dtype=torch.uint8, device=dev)
        ws = _gns._workspace(_screen_workspace_bytes(s, solver.prefix + '_workspace_bytes', counts, lds, solver.formula), dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(getattr(lib, name)(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                      ge.data_ptr(), Bt, *shared(), _ptr(flow), worst.data_ptr(), worst_line.data_ptr(),
                                      conv.data_ptr(), ws.data_ptr(), ws.numel(), stream), name, lds, solver.formula)
        return flow, worst, worst_line, conv

    def adjoint(bu, li, ge, worst_line, conv, incoming, need):
        gin = [torch.empty_like(t) if n else None for t, n in zip((bu, li, ge), need)]
        if pickup_grad:                                      # the generator screen: dl/d(pickup), float64, a row per grid
            gin.append(torch.empty(Bt, ge.shape[1], dtype=torch.float64, device=dev) if need[3] else None)
        gflow, gworst = (None if g is None else g.to(device=dev, dtype=torch.float64).contiguous() for g in incoming)
        ws = _gns._workspace(adjoint_workspace_bytes(), dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(getattr(lib, adjoint_name)(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(),
                                              li.data_ptr(), ge.data_ptr(), Bt, *shared(), worst_line.data_ptr(), conv.data_ptr(),
                                              _ptr(gflow), _ptr(gworst), *map(_ptr, gin), ws.data_ptr(), ws.numel(),
                                              stream), adjoint_name, adjoint_lds, adjoint_formula)
        return gin

    base_target = _one_topology(topo)._replace(lds=_dc_lds_bytes(topo.host))
    if s.grad:
        # the backward's own refusal (its LDS image is the largest of the call) comes before anything is launched
        adjoint_workspace_bytes()
        res = _DCN1Function.apply(screen, adjoint, s.buses, s.lines, s.generators, weights)
        base = list(_DCFunction.apply(lambda *a: _dc_solve(lib, cfg, base_target, *a),
                                      lambda *a: _dc_adjoint(lib, cfg, base_target, *a), s.buses, s.lines, s.generators))
    else:
        res = screen(*s.plain)
        # the base case as dc_power_flow solves it (after the screen, whose larger LDS image is the one a refusal names)
        base = _dc_solve(lib, cfg, base_target, *s.plain)
    return [torch.ones(Bt, s.N, dtype=torch.float64, device=dev), *base], list(res)


def _ac_screen_outputs(s, n_rows, keep_state, flows):
    """The fifteen outputs of an AC screen launch in ``gns_acn1_screen``'s order, uninitialised (the kernel writes every element):
    ``v`` and ``theta`` are None unless ``keep_state``, the four flows unless ``flows``."""
    Bt, dev = s.Bt, s.dev

    def rows(n, dtype):
        return [torch.empty(Bt, n_rows, dtype=dtype, device=dev) for _ in range(n)]

    state = [torch.empty(Bt, n_rows, s.N, dtype=torch.float64, device=dev) for _ in range(2)] if keep_state else [None, None]
    flow = [torch.empty(Bt, n_rows, s.E, dtype=torch.float64, device=dev) for _ in range(4)] if flows else [None] * 4
    worst, v_min, v_max, mismatch = rows(4, torch.float64)
    worst_line, v_min_bus, v_max_bus, iterations = rows(4, torch.int32)
    conv, = rows(1, torch.uint8)
    return [*state, *flow, worst, worst_line, v_min, v_min_bus, v_max, v_max_bus, conv, iterations, mismatch]


def _ac_screen_launch(s, solver, shared, n_rows, base_state, keep_state, flows, bu, li, ge):
    """One ``gns_acn1_screen`` / ``gns_acn2_screen`` launch (``solver``): the fifteen outputs in its order (``converged`` as uint8),
    every row warm-started from ``base_state`` (the base ``v``, ``theta`` and ``converged`` as uint8).  ``v`` and ``theta`` are None
    unless ``keep_state``, the four flows unless ``flows``."""
    lib, cfg, topo, Bt, dev = s.lib, s.cfg, s.topo, s.Bt, s.dev
    lds, name = topo.info['lds_bytes'], solver.prefix + '_screen'
    out = _ac_screen_outputs(s, n_rows, keep_state, flows)
    ws = _gns._workspace(_screen_workspace_bytes(s, solver.prefix + '_workspace_bytes', (n_rows,), lds, solver.formula), dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(getattr(lib, name)(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                  ge.data_ptr(), Bt, *shared(), *(t.data_ptr() for t in base_state), *map(_ptr, out), ws.data_ptr(),
                                  ws.numel(), stream), name, lds, solver.formula)
    return out


class _DCN1Function(torch.autograd.Function):
    """A DC screen's differentiable call when an input requires grad, as ``_DCFunction``: the forward is the screen's launch, the
    backward one call of its adjoint (``gns_dcn1_adjoint``, ``gns_dcn2_adjoint``, ``gns_dcg1_adjoint``) on the forward's topology and
    lists.  ``line_flow`` is not saved: the adjoint recomputes each row's state from the inputs, the forward's ``worst_line`` and
    ``converged``.  ``weights`` (None, or the generator screen's pickup weights ``[Gn]`` / ``[Bt,Gn]`` float64) is on the graph for
    its gradient alone, the adjoint's fourth output: the kernels read the values the forward uploaded.  A ``[Gn]`` tensor gets the
    sum over the grids."""

    @staticmethod
    def forward(ctx, screen, adjoint, buses, lines, gens, weights):
        flow, worst, worst_line, conv = screen(buses, lines, gens)
        ctx.mark_non_differentiable(worst_line, conv)
        ctx.set_materialize_grads(False)
        ctx.adjoint = adjoint
        ctx.shared_weights = weights is not None and weights.dim() == 1
        ctx.save_for_backward(buses, lines, gens, worst_line, conv)
        return flow, worst, worst_line, conv

    @staticmethod
    @once_differentiable
    def backward(ctx, gfl, gwl, _gwi, _gconv):
        buses, lines, gens, worst_line, conv = ctx.saved_tensors
        gb, gl, gg, *gp = ctx.adjoint(buses, lines, gens, worst_line, conv, (gfl, gwl), ctx.needs_input_grad[2:6])
        gp = gp[0] if gp else None
        if gp is not None and ctx.shared_weights:
            gp = gp.sum(dim=0)
        return (None, None, gb, gl, gg, gp)


def dc_contingency_screen(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, outages=None, rating=None,
                          flows=True, differentiable=False):
    """DC N-1 contingency screening of every grid of a batch, on the device: the exact post-outage DC flows of each single-line
    outage of ``outages`` from the base factorisation and one more solve per outage (line-outage distribution factors), not from
    one factorisation per ``(grid, outage)`` as ``dc_power_flow(mixed_topologies=True)`` on the expanded batch does.

    Inputs, column maps, the slack and the device handling are those of ``dc_power_flow``; the whole batch shares one topology
    (``mixed_topologies`` is out of scope here).  ``outages``: a 1-D sequence or tensor of 0-based line indices (the convention of
    ``synth.contingency_grids``), default every line; duplicates are independent rows.  ``rating``: None (1: the loading is
    ``|flow|``), ``[E]`` or ``[Bt,E]``, positive and finite, used in float64.

    Returns ``DcContingencyResult(base, outages, line_flow, worst_loading, worst_line, islanding, converged)``:
      base           the ``DcPowerFlowResult`` of ``dc_power_flow`` on the same inputs, bit for bit
      outages        ``[K]`` int64
      line_flow      ``[Bt,K,E]`` float64, the flows with the line out, 0 at the outaged line; None with ``flows=False`` (the tensor is
                     ``8 Bt K E`` bytes: the kernel then writes the summaries alone)
      worst_loading  ``[Bt,K]`` float64, ``max_l |line_flow| / rating``;  worst_line ``[Bt,K]`` int32, the line that attains it (the
                     lowest of equals)
      islanding      ``[K]`` bool: the outage disconnects the grid (the line is a bridge of the topology, found on the host once per
                     topology, never from a numeric threshold).  Those rows are NaN / -1 in every grid.
      converged      ``[Bt]`` bool, the base solve's.  A grid whose base solve fails has NaN / -1 in every row; a row whose update is
                     not finite has NaN / -1 alone.
    Every ``(grid, outage)`` row is bit-identical alone, in any batch, for any outage list or order that holds the outage and from
    run to run.  With a 2-D single grid the batch dimension is dropped.

    The analysis is ``fast_decoupled``'s and ``dc_power_flow``'s: a batch either has seen is not analysed again.

    Gradients: by default the outputs are not differentiable (the call runs as under ``torch.no_grad()``).  With
    ``differentiable=True``, grad mode on and ``requires_grad`` on an input, ``line_flow`` and ``worst_loading`` are differentiable
    through one ``gns_dcn1_adjoint`` call on the forward's topology (per outage a second solve on the base factor and a
    Sherman-Morrison correction; nothing is factored per outage, and ``line_flow`` is not kept for the backward), and ``base.theta``,
    ``base.line_flow`` and ``base.slack_p`` through ``dc_power_flow``'s adjoint.  The derivative is exact with respect to ``Pd``,
    ``Gs``, the lines' ``x``, ``tau``, ``shift`` and the generators' ``Pg``; every other column gets 0, and row ``k`` gives exactly 0
    to line ``k``'s own columns.  ``rating`` is a constant; a tie in the worst loading sends the gradient to ``worst_line``;
    ``worst_line``, ``islanding``, ``converged`` and ``outages`` are not differentiable.  A row that is NaN / -1 (an islanding
    outage, a non-finite update) contributes nothing when its incoming gradients are exactly zero or absent (a loss that indexes
    ``~islanding``); otherwise, and for a grid that is not solved, the grid's three gradient rows are NaN (zero rows for an
    unsolved grid whose incoming gradients are all zero).  The forward outputs are bit-identical with and without gradients.  A
    grid's gradient is bit-identical alone, in any batch and from run to run for the same outage list; the order of the list may
    change its last bits.  Mixed topologies are out of scope; double outages are ``dc_n2_contingency_screen``, the AC screen is
    ``ac_contingency_screen``.
    Contract: ``include/gns_powerflow.h``, "DC contingency screening"."""
    s = _screen_setup('dc_contingency_screen', _FD, buses, lines, generators, B, L, G, slack_bus, outages, rating, dict(flows=flows),
                      differentiable)
    with torch.set_grad_enabled(s.grad):
        K = s.rows.size
        base, res = _dc_screen(s, _DCN1, _shared_args(s, _upload32(s.rows, s.dev)), K, (K,), (K,), _dcn1_adjoint_lds_bytes,
                               _DCN1_ADJOINT_LDS_FORMULA, flows)
        base, outages_t, res, islanding = _screen_results(s, base, res, 3)
        return DcContingencyResult(DcPowerFlowResult(*base), outages_t, res[0], res[1], res[2], islanding, res[3])


def _pair_list(pairs, E, single='dc_contingency_screen'):
    """The checked list of line pairs as an int64 numpy array ``[P,2]``; None: every ``j < k`` in lexicographic order.  ``single``:
    the single-outage call a pair of twice the same line is sent to."""
    if pairs is None:
        if E < 2:
            raise ValueError(f'pairs: a grid with {E} line(s) has no pair of lines to take out')
        j, k = np.triu_indices(E, 1)
        return np.stack([j, k], axis=1).astype(np.int64)
    o = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if o.size == 0:
        raise ValueError('pairs is empty: give at least one pair of line indices (None: every pair)')
    if o.ndim != 2 or o.shape[1] != 2:
        raise ValueError(f'pairs must be a [P,2] sequence of line indices, got shape {tuple(o.shape)}')
    if o.dtype == np.bool_ or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f'pairs must hold integers (0-based line indices), got dtype {o.dtype}')
    if o.min() < 0 or o.max() > E - 1:
        raise ValueError(f'pairs must lie in 0..{E - 1} (0-based line indices), got {int(o.min())}..{int(o.max())}')
    o = o.astype(np.int64)
    same = np.flatnonzero(o[:, 0] == o[:, 1])
    if same.size:
        raise ValueError(f'pairs must name two different lines, got ({int(o[same[0], 0])}, {int(o[same[0], 1])}) at row {int(same[0])}: '
                         f'a single outage is {single}\'s')
    return o


def _pair_islanding(n_bus, f_bus, t_bus, pairs, bridges=None, cache=None):
    """bool ``[P]``: the pairs of lines (0-based ends, ``pairs`` ``[P,2]``) whose removal disconnects the graph the lines span:
    ``j`` is a bridge, or ``k`` is a bridge of the graph without line ``j``.  The relation is symmetric, so the lower line of a pair
    is taken as ``j``: one more search (``_bridges``) per distinct lower line that is not itself a bridge, kept in ``cache`` (a dict
    line -> bool ``[E]``, the bridges of the graph without that line)."""
    f, t = np.asarray(f_bus), np.asarray(t_bus)
    bridges = _bridges(n_bus, f, t) if bridges is None else bridges
    cache = {} if cache is None else cache
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    out = bridges[lo] | bridges[hi]
    todo = np.flatnonzero(~out)
    order = todo[np.argsort(lo[todo], kind='stable')]
    starts = np.flatnonzero(np.r_[True, lo[order][1:] != lo[order][:-1]]) if order.size else np.zeros(0, dtype=np.int64)
    for a, b in zip(starts.tolist(), starts.tolist()[1:] + [order.size]):
        j = int(lo[order[a]])
        row = cache.get(j)
        if row is None:
            row = cache[j] = np.insert(_bridges(n_bus, np.delete(f, j), np.delete(t, j)), j, False)
        idx = order[a:b]
        out[idx] = row[hi[idx]]
    return out


def _topology_pair_islanding(topo, args, pairs):
    """The islanding pairs of an analysed topology (``_pair_islanding``); the bridges of the graph without a line are found once
    per line and kept with the topology, as ``_topology_bridges`` keeps the bridges."""
    if getattr(topo, 'bridges_without', None) is None:
        topo.bridges_without = {}
    n_bus, f_bus, t_bus = args[0], args[1], args[2]
    return _pair_islanding(int(n_bus), f_bus.astype(np.int64) - 1, t_bus.astype(np.int64) - 1, pairs, _topology_bridges(topo, args),
                           topo.bridges_without)


def _dcn2_adjoint_lds_bytes(host):
    """``(LDS image, W)`` of the N-2 screen's adjoint (``gns_dcn2_adjoint_lds_bytes``) on the FD blob ``host``, as
    ``_dcn1_adjoint_lds_bytes``: W columns side by side in its solve kernel."""
    return _screen_lds_bytes('gns_dcn2_adjoint_lds_bytes', host)


def dc_n2_contingency_screen(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, pairs=None, rating=None,
                             flows=False, differentiable=False):
    """DC N-2 contingency screening of every grid of a batch, on the device: the exact post-outage DC flows of each double-line
    outage of ``pairs``.  Two lines out are a rank-2 change of the DC matrix: the single-outage solves on the base factor (one per
    distinct line of the list, the ones ``dc_contingency_screen`` makes) and a 2x2 system per pair give the flows, not one
    factorisation per ``(grid, pair)`` as ``dc_power_flow(mixed_topologies=True)`` on the expanded batch does.

    Inputs, column maps, the slack, the device handling and ``rating`` are those of ``dc_contingency_screen``; the whole batch
    shares one topology.  ``pairs``: a ``[P,2]`` integer tensor, array or sequence of 0-based line indices, default every ``j < k`` in
    lexicographic order (``E (E - 1) / 2`` rows).  The two lines of a pair differ; duplicate pairs and both orders of a pair are
    allowed and are independent rows.

    Returns ``DcN2ContingencyResult(base, pairs, line_flow, worst_loading, worst_line, islanding, converged)``:
      base           the ``DcPowerFlowResult`` of ``dc_power_flow`` on the same inputs, bit for bit
      pairs          ``[P,2]`` int64, as given
      line_flow      None by default; with ``flows=True`` ``[Bt,P,E]`` float64, the flows with both lines out, 0 at the two outaged
                     lines.  The default is the opposite of ``dc_contingency_screen``'s: the tensor is ``8 Bt P E`` bytes (1.6 GB for
                     one case300 grid and every pair), and the kernel writes the summaries alone without it.
      worst_loading  ``[Bt,P]`` float64, ``max_l |line_flow| / rating``;  worst_line ``[Bt,P]`` int32, the line that attains it (the
                     lowest of equals)
      islanding      ``[P]`` bool: the pair disconnects the grid (one line is a bridge of the topology, or the second is a bridge of
                     the graph without the first; found on the host and kept with the topology, never from a numeric threshold).
                     Those rows are NaN / -1 in every grid.
      converged      ``[Bt]`` bool, the base solve's.  A grid whose base solve fails has NaN / -1 in every row; a pair whose update
                     is not finite (a singular 2x2 system included) has NaN / -1 alone.
    Every ``(grid, pair)`` row is bit-identical alone, in any batch, in any pair list or order that holds it, in either order of
    its two lines, and from run to run.  With a 2-D single grid the batch dimension is dropped.

    Gradients: by default the outputs are not differentiable (the call runs as under ``torch.no_grad()``).  With
    ``differentiable=True``, grad mode on and ``requires_grad`` on an input, ``worst_loading`` (and ``line_flow`` with
    ``flows=True``) is differentiable through one ``gns_dcn2_adjoint`` call on the forward's topology and pair list (per pair a
    2x2 system again, per distinct line of the list one more solve on the base factor and one for the whole list; nothing is
    factored or solved per pair, ``line_flow`` is not kept for the backward, and with ``flows=False`` no ``[Bt,P,E]`` tensor is
    formed), and ``base.theta``, ``base.line_flow`` and ``base.slack_p`` through ``dc_power_flow``'s adjoint.  The derivative is
    exact with respect to ``Pd``, ``Gs``, the lines' ``x``, ``tau``, ``shift`` and the generators' ``Pg``; every other column gets
    0, and row ``(j,k)`` gives exactly 0 to the own columns of lines ``j`` and ``k`` (a line that every contributing row holds has
    exact zeros; next to other rows' contributions the row's own cancels to rounding in the shared solves).  ``rating`` is a constant; a tie in the worst loading
    sends the gradient to ``worst_line``; ``worst_line``, ``islanding``, ``converged`` and ``pairs`` are not differentiable.  A row
    that is NaN / -1 (an islanding pair, a non-finite 2x2 update) contributes nothing when its incoming gradients are exactly zero
    or absent (a loss that indexes ``~islanding``); otherwise, and for a grid that is not solved, the grid's three gradient rows
    are NaN (zero rows for an unsolved grid whose incoming gradients are all zero).  The forward outputs are bit-identical with and
    without gradients.  A grid's gradient is bit-identical alone, in any batch and from run to run for the same pair list, and a
    list that holds ``(k,j)`` where another holds ``(j,k)`` gives the same bits; the order of the list may change its last bits.
    Mixed topologies and second derivatives are out of scope; generator outages, alone or with a line, are
    ``dc_generator_contingency_screen``; the AC solve of chosen pairs is
    ``ac_n2_contingency_screen``.
    Contract: ``include/gns_powerflow.h``, "DC N-2 contingency screening"."""
    s = _screen_setup('dc_n2_contingency_screen', _FD, buses, lines, generators, B, L, G, slack_bus, pairs, rating, dict(flows=flows),
                      differentiable)
    with torch.set_grad_enabled(s.grad):
        # the distinct lines of the list, ascending, and each pair as two positions into them
        P = s.rows.shape[0]
        cand_np, cols_np = np.unique(s.rows, return_inverse=True)
        shared = _shared_args(s, _upload32(cand_np, s.dev), _upload32(cols_np.reshape(P, 2), s.dev))
        n_cand = cand_np.size
        base, res = _dc_screen(s, _DCN2, shared, P, (n_cand,), (n_cand, P), _dcn2_adjoint_lds_bytes, _DCN2_ADJOINT_LDS_FORMULA, flows)
        base, pairs_t, res, islanding = _screen_results(s, base, res, 3)
        return DcN2ContingencyResult(DcPowerFlowResult(*base), pairs_t, res[0], res[1], res[2], islanding, res[3])


def _generator_contingency_list(rows, Gn, E):
    """The checked list of generator contingencies as an int64 numpy array ``[P,2]`` of ``(generator, line or -1)``; None: for each
    generator in order, ``(g,-1), (g,0), ..., (g,E-1)``."""
    if rows is None:
        g = np.repeat(np.arange(Gn, dtype=np.int64), E + 1)
        k = np.tile(np.arange(-1, E, dtype=np.int64), Gn)
        return np.stack([g, k], axis=1)
    o = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    if o.size == 0:
        raise ValueError('contingencies is empty: give at least one (generator, line or -1) row (None: every generator alone and with '
                         'every line)')
    if o.ndim != 2 or o.shape[1] != 2:
        raise ValueError(f'contingencies must be a [P,2] sequence of (generator, line or -1), got shape {tuple(o.shape)}')
    if o.dtype == np.bool_ or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f'contingencies must hold integers (0-based generator rows and line indices), got dtype {o.dtype}')
    o = o.astype(np.int64)
    if o[:, 0].min() < 0 or o[:, 0].max() > Gn - 1:
        raise ValueError(f'contingencies must name generators in 0..{Gn - 1} (0-based generator rows), got '
                         f'{int(o[:, 0].min())}..{int(o[:, 0].max())}')
    if o[:, 1].min() < -1 or o[:, 1].max() > E - 1:
        raise ValueError(f'contingencies must name lines in -1..{E - 1} (0-based line indices, -1: no line out), got '
                         f'{int(o[:, 1].min())}..{int(o[:, 1].max())}')
    return o


def _generator_islanding(bridges, rows):
    """bool ``[P]``: the rows ``(generator, line or -1)`` that disconnect the grid.  A generator outage never does, so it is the rows
    whose line is one of ``bridges`` (bool ``[E]``, ``_bridges``)."""
    k = rows[:, 1]
    return bridges[np.maximum(k, 0)] & (k >= 0)


def _pickup(pickup, generators, single):
    """The checked pickup weights of ``generators`` ``[Bt,Gn,7]``: None (the slack picks up), or float64 ``[Gn]`` / ``[Bt,Gn]``
    (``'pmax'``: the generators' column 1)."""
    if pickup is None:
        return None
    Bt, Gn = generators.shape[0], generators.shape[1]
    if isinstance(pickup, str):
        if pickup != 'pmax':
            raise ValueError(f"pickup must be None, 'pmax' or weights [{Gn}] or [{Bt},{Gn}], got {pickup!r}")
        w = generators[:, :, 1].to(torch.float64)
    else:
        w = torch.as_tensor(pickup).to(torch.float64)
        if single and w.dim() == 2 and w.shape[0] == 1:
            w = w[0]
    if tuple(w.shape) not in ((Gn,), (Bt, Gn)):
        raise ValueError(f'pickup must be [{Gn}] or [{Bt},{Gn}], got {tuple(w.shape)}')
    if not bool((torch.isfinite(w) & (w >= 0)).all()):
        raise ValueError('pickup must be non-negative and finite')
    return w


def dc_generator_contingency_screen(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, contingencies=None,
                                    pickup=None, rating=None, flows=False):
    """DC generator contingency screening of every grid of a batch, on the device: the exact post-outage DC flows of each row of
    ``contingencies``, a generator out alone or with a line out as well (the combined N-1 set of a planner).  A generator outage
    changes the injections alone: one more solve on the base factor per distinct generator of the list gives its flows, and the
    line on top of it is the rank-1 update ``dc_contingency_screen`` makes, from one more solve per distinct line.  Nothing is
    factored per row, as ``dc_power_flow`` on the expanded batch (with ``mixed_topologies=True`` for the rows with a line) would.

    Inputs, column maps, the slack, the device handling and ``rating`` are those of ``dc_contingency_screen``; the whole batch
    shares one topology.  ``contingencies``: a ``[P,2]`` integer tensor, array or sequence of ``(generator, line)``, 0-based
    generator rows and line indices, line -1 for "no line out"; default, for each generator in order, ``(g,-1), (g,0), ...,
    (g,E-1)`` (``Gn (E + 1)`` rows).  Duplicates are independent rows.

    The outaged generator's ``Pg`` leaves its bus.  ``pickup`` says who replaces it: None, the slack (what ``dcpf`` does with a unit
    whose ``Pg`` is set to 0); ``'pmax'``, the other generators in proportion to their column 1; or weights ``[Gn]`` / ``[Bt,Gn]``,
    non-negative and finite, used in float64: generator ``h != g`` gains ``Pg_g w_h / W_g`` with ``W_g`` the sum of the others'
    weights, and when that sum is exactly zero the slack picks up.  No Pmax or Pmin limit is enforced on the units that pick up.

    Returns ``DcGeneratorContingencyResult(base, contingencies, line_flow, worst_loading, worst_line, islanding, converged)``:
      base           the ``DcPowerFlowResult`` of ``dc_power_flow`` on the same inputs, bit for bit
      contingencies  ``[P,2]`` int64, as given
      line_flow      None by default; with ``flows=True`` ``[Bt,P,E]`` float64, the flows with the generator (and the line) out, 0 at
                     the outaged line
      worst_loading  ``[Bt,P]`` float64, ``max_l |line_flow| / rating``;  worst_line ``[Bt,P]`` int32, the line that attains it (the
                     lowest of equals)
      islanding      ``[P]`` bool: the row's line is a bridge of the topology (found on the host and kept with the topology, never
                     from a numeric threshold); a generator outage alone never islands.  Those rows are NaN / -1 in every grid.
      converged      ``[Bt]`` bool, the base solve's.  A grid whose base solve fails has NaN / -1 in every row; a row whose update
                     is not finite has NaN / -1 alone.
    Every ``(grid, row)`` is bit-identical alone, in any batch, in any list or order that holds it, and from run to run.  Where
    ``Pg_g`` is exactly 0, or the generator sits on the slack bus and ``pickup`` is None, row ``(g,-1)`` is ``base.line_flow`` and row
    ``(g,k)`` is row ``k`` of ``dc_contingency_screen``, bit for bit.  With a 2-D single grid the batch dimension is dropped.

    The outputs are not differentiable (the call runs as under ``torch.no_grad()``, whatever requires grad): the same call with a
    backward on the device is ``dc_generator_contingency_screen_differentiable``.  The AC check of the same rows is
    ``ac_generator_contingency_screen``.  Mixed topologies, limits on the pickup and a generator with two lines are out of scope.
    Contract: ``include/gns_powerflow.h``, "DC generator contingency screening"."""
    return _dc_generator_screen(buses, lines, generators, B, L, G, slack_bus, contingencies, pickup, rating, flows, False)


def _dcg1_adjoint_lds_bytes(host):
    """``(LDS image, W)`` of the generator screen's adjoint (``gns_dcg1_adjoint_lds_bytes``) on the FD blob ``host``, as
    ``_dcn2_adjoint_lds_bytes``."""
    return _screen_lds_bytes('gns_dcg1_adjoint_lds_bytes', host)


def _dc_generator_screen(buses, lines, generators, B, L, G, slack_bus, contingencies, pickup, rating, flows, differentiable):
    """``dc_generator_contingency_screen`` and its differentiable twin: one set-up, one launch."""
    s = _screen_setup('dc_generator_contingency_screen', _FD, buses, lines, generators, B, L, G, slack_bus, contingencies, rating,
                      dict(flows=flows), differentiable, pickup=pickup)
    with torch.set_grad_enabled(s.grad):
        # the distinct lines and generators of the list, ascending, and each row as two positions into them (-1: no line)
        P = s.rows.shape[0]
        gen_np, gen_col = np.unique(s.rows[:, 0], return_inverse=True)
        k = s.rows[:, 1]
        line_np = np.unique(k[k >= 0])
        cols_np = np.stack([gen_col.reshape(P), np.where(k >= 0, np.searchsorted(line_np, k), -1)], axis=1)
        lists = _shared_args(s, _upload32(line_np, s.dev), _upload32(gen_np, s.dev), _upload32(cols_np, s.dev))

        def shared():
            return (*lists(), _ptr(s.pickup), int(s.pickup is not None and s.pickup.dim() == 2))

        # the weights as the graph sees them: column 1 of the canonical generators for 'pmax', the caller's tensor when it requires
        # grad; anything else takes no gradient (grad_pickup is then NULL)
        weights = None
        if s.grad and isinstance(pickup, str):
            weights = s.generators[:, :, 1].to(torch.float64)
        elif s.grad and isinstance(pickup, torch.Tensor) and pickup.requires_grad:
            weights = pickup.to(device=s.dev, dtype=torch.float64).reshape(s.pickup.shape)
        base, res = _dc_screen(s, _DCG1, shared, P, (line_np.size, gen_np.size), (line_np.size, gen_np.size, P),
                               _dcg1_adjoint_lds_bytes, _DCG1_ADJOINT_LDS_FORMULA, flows, True, weights)
        base, rows_t, res, islanding = _screen_results(s, base, res, 3)
        return DcGeneratorContingencyResult(DcPowerFlowResult(*base), rows_t, res[0], res[1], res[2], islanding, res[3])


def dc_generator_contingency_screen_differentiable(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None,
                                                   contingencies=None, pickup=None, rating=None, flows=False):
    """``dc_generator_contingency_screen`` with gradients: the same arguments, the same ``DcGeneratorContingencyResult`` with every
    forward output and ``base.*`` bit-identical to that call's, and a backward on the device, for a security-constrained loss
    over the combined N-1 set (a unit trips, the others pick its output up) or a sensitivity study of the dispatch and the
    participation factors.

    With grad mode on and ``requires_grad`` on an input (or on a tensor ``pickup``), ``worst_loading`` (and ``line_flow`` with
    ``flows=True``) is differentiable through one ``gns_dcg1_adjoint`` call on the forward's topology and lists: per row the
    single-outage update again, per distinct line and per distinct generator of the list one more solve on the base factor and
    one for the whole list; nothing is factored or solved per row, ``line_flow`` is not kept for the backward, and with
    ``flows=False`` no ``[Bt,P,E]`` tensor is formed in either direction.  ``base.theta``, ``base.line_flow`` and ``base.slack_p``
    are differentiable through ``dc_power_flow``'s adjoint.  Otherwise it is the plain call and returns plain tensors.

    The derivative is exact with respect to ``Pd``, ``Gs``, the lines' ``x``, ``tau``, ``shift`` and the generators' ``Pg`` (the
    outaged unit's own ``Pg`` included); every other column gets 0.  The pickup weights: with ``pickup='pmax'`` their gradient is
    added into the generators' column 1, which joins the contract for this pickup only; a tensor ``pickup`` that requires grad
    receives it in its own dtype, a ``[Gn]`` tensor the sum over the grids; otherwise it is not computed.  The branch in which a
    unit's remaining weights sum to exactly zero (the slack picks up) is not differentiated: it gives the weights 0.  Row
    ``(g,k)`` gives 0 to line ``k``'s own columns (exact when every contributing row of the grid holds ``k``, else the row's own
    part cancels to rounding in the shared solves).  ``rating`` is a constant; a tie in the worst loading sends the gradient to
    ``worst_line``; ``worst_line``, ``islanding``, ``converged`` and ``contingencies`` are not differentiable.

    A row that is NaN / -1 (an islanding row, a non-finite update) contributes nothing when its incoming gradients are exactly
    zero or absent (a loss that indexes ``~islanding``); otherwise, and for a grid that is not solved, the grid's gradient rows
    (the weights' included) are NaN, zero rows for an unsolved grid whose incoming gradients are all zero.  Other grids are
    unaffected.  A grid's gradient is bit-identical alone, in any batch and from run to run for the same list; another order of
    the list may change its last bits.

    Out of scope: mixed topologies, limits on the pickup, a generator with two lines, second derivatives.  AC generator outages:
    ``ac_generator_contingency_screen`` (with gradients: ``ac_generator_contingency_screen_differentiable``).
    Contract: ``include/gns_powerflow.h``, "Gradients of the DC generator screen"."""
    return _dc_generator_screen(buses, lines, generators, B, L, G, slack_bus, contingencies, pickup, rating, flows, True)


class _ACN1Function(torch.autograd.Function):
    """``ac_contingency_screen(differentiable=True)`` and ``ac_n2_contingency_screen_differentiable`` when an input requires grad, as
    ``_DCN1Function``: the forward is the screen's launch (``screen`` returns the fifteen outputs in ``gns_acn1_screen``'s order,
    ``v`` and ``theta`` always there), the backward one ``gns_acn1_adjoint`` / ``gns_acn2_adjoint`` call (``adjoint``, ``_ac_screen``'s)
    on the forward's topology, list and state.  Newton is not run again."""

    @staticmethod
    def forward(ctx, screen, adjoint, buses, lines, gens):
        out = screen(buses, lines, gens)
        v, theta, _, _, _, _, _, worst_line, _, v_min_bus, _, v_max_bus, conv, iters, mis = out
        ctx.mark_non_differentiable(worst_line, v_min_bus, v_max_bus, conv, iters, mis)
        ctx.set_materialize_grads(False)
        ctx.adjoint = adjoint
        ctx.save_for_backward(buses, lines, gens, v, theta, conv, worst_line, v_min_bus, v_max_bus)
        return tuple(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, gv, gth, gpf, gqf, gpt, gqt, gwl, _gwi, gvmin, _gi0, gvmax, _gi1, _gconv, _giters, _gmis):
        buses, lines, gens, *state = ctx.saved_tensors
        grads = ctx.adjoint(buses, lines, gens, state, (gv, gth, gpf, gqf, gpt, gqt, gwl, gvmin, gvmax), ctx.needs_input_grad[2:5])
        return (None, None, *grads)


def ac_contingency_screen(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, outages=None, rating=None,
                          tol=1e-8, max_iter=10, flows=True, states=True, differentiable=False):
    """AC N-1 contingency screening of every grid of a batch, on the device: Newton-Raphson on each ``(grid, outage)`` pair of the
    single-line outages of ``outages``, with the post-outage voltages, the apparent-power flows at both ends of every line, the
    worst loading and the voltage extremes.  An outage removes the line's four Y-bus stamps and nothing else, so the Jacobian of
    every pair has a subset of the base sparsity: the one analysis of the base topology (``newton_raphson``'s, cached) serves every
    outage, where ``newton_raphson(mixed_topologies=True)`` on the expanded batch analyses one topology per outage and holds a copy
    of the inputs per pair.

    Inputs, column maps, the slack and the device handling are those of ``newton_raphson``; the whole batch shares one topology.
    ``outages``: a 1-D sequence or tensor of 0-based line indices, default every line; duplicates are independent rows.
    ``rating``: None (1: the loading is ``max(|S_from|, |S_to|)``), ``[E]`` or ``[Bt,E]``, positive and finite, used in float64.
    ``tol``, ``max_iter``: Newton-Raphson's, for the base solve and for every pair.

    Row ``(g, k)`` is Newton-Raphson on grid ``g`` with line ``outages[k]`` out of service: the Y-bus from the line stamps without
    that line's, the injections, bus roles and ``vg`` set points unchanged, warm-started from ``base.v[g]``, ``base.theta[g]``; the
    convergence test, update, failure rules and float64 arithmetic of ``include/gns_powerflow.h``.

    Returns ``AcContingencyResult``:
      base           the ``PowerFlowResult`` of ``newton_raphson`` on the same inputs with the same ``tol`` and ``max_iter``, bit for bit
      outages        ``[K]`` int64
      v, theta       ``[Bt,K,N]`` float64, the post-outage state; None with ``states=False``
      p_from, q_from, p_to, q_to   ``[Bt,K,E]`` float64, MATPOWER's branch model on the makeYbus quantities: ``S_f = V_f conj(Y_ff V_f +
                     Y_ft V_t)``, ``S_t = V_t conj(Y_tf V_f + Y_tt V_t)``; all four 0 at the outaged line; None with ``flows=False``
      worst_loading  ``[Bt,K]`` float64, ``max_l max(|S_f|, |S_t|) / rating_l``;  worst_line ``[Bt,K]`` int32, the lowest of equals
      v_min, v_max   ``[Bt,K]`` float64 with v_min_bus, v_max_bus ``[Bt,K]`` int32 (0-based, the lowest of equals)
      converged, iterations, mismatch   ``[Bt,K]`` bool / int32 / float64, Newton-Raphson's own meaning per row
      islanding      ``[K]`` bool: the outage disconnects the grid (a bridge of the topology, found on the host once per topology)
    An islanding outage has NaN / -1 / ``converged`` False / ``iterations`` -1 in every grid; so has every row of a grid whose base
    solve did not converge.  A row that does not converge keeps its last finite iterate with ``converged`` False, as
    ``newton_raphson`` does, and its flows and summaries are computed from that iterate.  Every row is bit-identical alone, in any
    batch, in any list or order that holds the outage and from run to run.  With a 2-D single grid the batch dimension is dropped.

    Gradients: by default the outputs are not differentiable (the call runs as under ``torch.no_grad()``).  With
    ``differentiable=True``, grad mode on and ``requires_grad`` on an input, ``v``, ``theta``, the four flows, ``worst_loading``,
    ``v_min`` and ``v_max`` are differentiable through one ``gns_acn1_adjoint`` call on the forward's topology, outage list and state
    (per row the implicit function theorem on the grid without the line: one factorisation of the row's Jacobian on the base
    analysis and one transposed solve; Newton is not run again), and ``base.v`` / ``base.theta`` through ``newton_raphson``'s adjoint.
    The derivative is exact at the returned state with respect to ``newton_raphson``'s columns (``Pd, Qd, Gs, Bs``; the lines'
    ``r, x, b, tau, shift``; ``Pg`` and the ``vg`` of the first generator on a PV / slack bus); every other column gets 0, and row
    ``k`` gives exactly 0 to line ``k``'s own columns.  ``rating`` is a constant and the warm start is not differentiated (a
    converged row does not depend on it).  ``worst_loading`` sends its gradient to ``worst_line``, at the end that attains the
    maximum (the from end on equality), ``v_min`` / ``v_max`` to the buses reported; the index outputs, ``converged``,
    ``iterations``, ``mismatch``, ``islanding`` and ``outages`` are not differentiable.  With ``states=False`` / ``flows=False`` the
    summaries stay differentiable (``v`` and ``theta`` are then kept for the backward, ``16 Bt K N`` bytes, and not returned).  A row
    whose incoming gradients are all exactly zero or absent is skipped, never multiplied by zero (a loss that indexes ``converged``
    rows); a non-zero gradient into a row that is not converged (an islanding outage, a stopped iteration), a zero or non-finite
    pivot or a non-finite lambda makes the grid's three gradient rows NaN; a grid without a base solution gets NaN rows, zero rows
    when all its incoming gradients are zero.  Other grids are unaffected.  The forward outputs are bit-identical with and without
    gradients; a grid's gradient is bit-identical alone, in any batch and from run to run for the same outage list (another order
    of the list may change its last bits).

    Out of scope: batches that mix topologies and generator reactive limits.  Double outages: ``ac_n2_contingency_screen``;
    generator outages, alone or with a line: ``ac_generator_contingency_screen``.
    Contract: ``include/gns_powerflow.h``, "AC contingency screening"."""
    s = _screen_setup('ac_contingency_screen', _NR, buses, lines, generators, B, L, G, slack_bus, outages, rating,
                      dict(flows=flows, states=states), differentiable, tol, max_iter)
    base, outages_t, res, islanding = _ac_screen(s, _ACN1, states, flows)
    return AcContingencyResult(PowerFlowResult(*base), outages_t, *res, islanding)


def _ac_screen(s, solver, states, flows):
    """Both AC screens after ``_screen_setup``: the base case as ``newton_raphson`` solves it, ``solver``'s screen launch
    (``_ac_screen_launch``) on the list ``s.rows`` and, when the call is differentiated, the two through ``_NRFunction`` and
    ``_ACN1Function`` with ``solver``'s adjoint entry point as the screen's backward.  Returns ``_screen_results``' tuple."""
    with torch.set_grad_enabled(s.grad):
        lib, cfg, topo, Bt, dev, grad = s.lib, s.cfg, s.topo, s.Bt, s.dev, s.grad
        n_rows = s.rows.shape[0]
        shared = _shared_args(s, _upload32(s.rows, dev))
        lds = topo.info['lds_bytes']
        target = _one_topology(topo)
        adjoint_name = solver.prefix + '_adjoint'

        def adjoint_workspace_bytes():
            return _screen_workspace_bytes(s, adjoint_name + '_workspace_bytes', (n_rows,), lds, solver.formula)

        # the base case as newton_raphson solves it (its refusals come first, then the backward's own, before anything is launched)
        if grad:
            adjoint_workspace_bytes()
            base = list(_NRFunction.apply(lambda *a: _solve(lib, _NR, cfg, target, *a, None, None),
                                          lambda *a: _adjoint(lib, cfg, target, *a), s.buses, s.lines, s.generators))
        else:
            base = _solve(lib, _NR, cfg, target, *s.plain, None, None)
        base_conv = base[2].to(torch.uint8)
        base_state = (base[0].detach(), base[1].detach(), base_conv)      # the warm start is not differentiated

        def screen(bu, li, ge):
            return _ac_screen_launch(s, solver, shared, n_rows, base_state, states or grad, flows, bu, li, ge)

        def adjoint(bu, li, ge, state, incoming, need):
            """One adjoint call at the forward's ``state`` (v, theta, converged, worst_line, v_min_bus, v_max_bus)."""
            gin = [torch.empty_like(t) if n else None for t, n in zip((bu, li, ge), need)]
            incoming = [None if g is None else g.to(device=dev, dtype=torch.float64).contiguous() for g in incoming]
            ws = _gns._workspace(adjoint_workspace_bytes(), dev)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                _check(getattr(lib, adjoint_name)(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(),
                                                  li.data_ptr(), ge.data_ptr(), Bt, *shared(), *(t.data_ptr() for t in state),
                                                  base_conv.data_ptr(), *map(_ptr, incoming), *map(_ptr, gin), ws.data_ptr(),
                                                  ws.numel(), stream), adjoint_name, lds, solver.formula)
            return gin

        res = list(_ACN1Function.apply(screen, adjoint, s.buses, s.lines, s.generators)) if grad else screen(*s.plain)
        if not states:
            res[0] = res[1] = None
        return _screen_results(s, base, res, 12)


def ac_n2_contingency_screen(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, pairs=None, rating=None,
                             tol=1e-8, max_iter=10, flows=False, states=False):
    """AC N-2 contingency screening of every grid of a batch, on the device: Newton-Raphson on each ``(grid, pair)`` of the
    double-line outages of ``pairs``, with the outputs of ``ac_contingency_screen`` per pair.  Two outages remove eight Y-bus stamps
    and nothing else, so the one analysis of the base topology (``newton_raphson``'s, cached) serves every pair, where
    ``newton_raphson(mixed_topologies=True)`` on the expanded batch analyses one topology per distinct pair and holds a copy of the
    inputs per row.  It is the AC check of the pairs a linear screen ranked worst: ``dc_n2_contingency_screen`` over every pair,
    the few hundred highest ``worst_loading``, then this call with ``pairs=`` those.

    Inputs, column maps, the slack, the device handling, ``rating``, ``tol`` and ``max_iter`` are those of
    ``ac_contingency_screen``; the whole batch shares one topology.  ``pairs``: a ``[P,2]`` integer tensor, array or sequence of
    0-based line indices, default every ``j < k`` in lexicographic order (``E (E - 1) / 2`` rows).  The two lines of a pair differ
    (a single outage is ``ac_contingency_screen``'s); duplicate pairs and both orders of a pair are allowed and are independent rows.

    Row ``(g, p)`` is Newton-Raphson on grid ``g`` with both lines of ``pairs[p]`` out of service: the Y-bus from the line stamps
    without those two lines', the injections, bus roles and ``vg`` set points unchanged, warm-started from ``base.v[g]``,
    ``base.theta[g]``; the convergence test, update, failure rules and float64 arithmetic of ``include/gns_powerflow.h``.  The lines
    may share a bus, be parallel, or run from a bus to itself.

    Returns ``AcN2ContingencyResult``, ``AcContingencyResult``'s fields with ``pairs`` in place of ``outages``:
      base           the ``PowerFlowResult`` of ``newton_raphson`` on the same inputs with the same ``tol`` and ``max_iter``, bit for bit
      pairs          ``[P,2]`` int64, as given
      v, theta       None by default; with ``states=True`` ``[Bt,P,N]`` float64, the post-outage state
      p_from, q_from, p_to, q_to   None by default; with ``flows=True`` ``[Bt,P,E]`` float64, ``ac_contingency_screen``'s branch flows,
                     all four 0 at both outaged lines.  The defaults are the opposite of ``ac_contingency_screen``'s: at every pair
                     of case118 the four flow tensors are 102 MB per grid, and the kernel writes the summaries alone without them.
      worst_loading  ``[Bt,P]`` float64, ``max_l max(|S_f|, |S_t|) / rating_l``;  worst_line ``[Bt,P]`` int32, the lowest of equals
      v_min, v_max   ``[Bt,P]`` float64 with v_min_bus, v_max_bus ``[Bt,P]`` int32 (0-based, the lowest of equals)
      converged, iterations, mismatch   ``[Bt,P]`` bool / int32 / float64, Newton-Raphson's own meaning per row
      islanding      ``[P]`` bool: the pair disconnects the grid (one line is a bridge of the topology, or the second is a bridge of
                     the graph without the first; found on the host and kept with the topology, never from a numeric threshold)
    An islanding pair has NaN / -1 / ``converged`` False / ``iterations`` -1 in every grid; so has every row of a grid whose base
    solve did not converge.  A row that does not converge keeps its last finite iterate with ``converged`` False, as
    ``ac_contingency_screen`` does, and its flows and summaries are computed from that iterate.  Every row is bit-identical alone,
    in any batch, in any pair list or order that holds it, in either order of its two lines, and from run to run.  With a 2-D single
    grid the batch dimension is dropped.

    This call runs as under ``torch.no_grad()``, and ``requires_grad`` on an input is ignored without an error; the same screen with
    gradients is ``ac_n2_contingency_screen_differentiable``.
    Out of scope: batches that mix topologies, a generator with two lines and generator reactive limits.  A generator with one
    line: ``ac_generator_contingency_screen``.
    Contract: ``include/gns_powerflow.h``, "AC N-2 contingency screening"."""
    return _ac_n2_screen(buses, lines, generators, B, L, G, slack_bus, pairs, rating, tol, max_iter, flows, states, False)


def _ac_n2_screen(buses, lines, generators, B, L, G, slack_bus, pairs, rating, tol, max_iter, flows, states, differentiable):
    """``ac_n2_contingency_screen`` (``differentiable`` False) and ``ac_n2_contingency_screen_differentiable`` (True)."""
    s = _screen_setup('ac_n2_contingency_screen', _NR, buses, lines, generators, B, L, G, slack_bus, pairs, rating,
                      dict(flows=flows, states=states), differentiable, tol, max_iter)
    base, pairs_t, res, islanding = _ac_screen(s, _ACN2, states, flows)
    return AcN2ContingencyResult(PowerFlowResult(*base), pairs_t, *res, islanding)


def ac_n2_contingency_screen_differentiable(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, pairs=None,
                                            rating=None, tol=1e-8, max_iter=10, flows=False, states=False):
    """``ac_n2_contingency_screen`` with gradients: the same arguments, the same ``AcN2ContingencyResult`` with every forward output
    bit-identical to that call's, and a backward on the device, as ``ac_contingency_screen(differentiable=True)`` has one.  It is
    the last step of the workflow the plain call names (``dc_n2_contingency_screen`` over every pair, the few hundred worst, the AC
    check of those) for a security-constrained loss or a sensitivity study of the worst double outages.

    With grad mode on and ``requires_grad`` on an input, ``v``, ``theta``, the four flows, ``worst_loading``, ``v_min`` and ``v_max``
    are differentiable through one ``gns_acn2_adjoint`` call on the forward's topology, pair list and state (per row the implicit
    function theorem on the grid without both lines: one factorisation of the row's Jacobian on the base analysis and one
    transposed solve; Newton is not run again), and ``base.v`` / ``base.theta`` through ``newton_raphson``'s adjoint.  Otherwise
    (grad mode off, no input requires grad) it is the plain call and returns plain tensors.

    The derivative is exact at the returned state with respect to ``newton_raphson``'s columns (``Pd, Qd, Gs, Bs``; the lines'
    ``r, x, b, tau, shift``; ``Pg`` and the ``vg`` of the first generator on a PV / slack bus); every other column gets 0, and row
    ``(j,k)`` gives exactly 0 to the own columns of lines ``j`` and ``k``, whose flows are the constant 0.  ``rating`` is a constant
    and the warm start is not differentiated (a converged row does not depend on it).  ``worst_loading`` sends its gradient to
    ``worst_line``, at the end that attains the maximum (the from end on equality), ``v_min`` / ``v_max`` to the buses reported; the
    index outputs, ``converged``, ``iterations``, ``mismatch``, ``islanding`` and ``pairs`` are not differentiable.

    With ``states=False`` (the default) the summaries and the flows stay differentiable: ``v`` and ``theta`` are then kept for the
    backward and not returned.  That costs ``16 Bt P N`` bytes until the backward has run: 32 MB per grid at every pair of case118
    (P = 17 205, N = 118), 15 MB for 64 case118 grids and a list of 128 pairs.

    A row whose incoming gradients are all exactly zero or absent is skipped, never multiplied by zero (a loss that indexes
    ``converged`` rows); a non-zero gradient into a row that is not converged (an islanding pair, a stopped iteration), a zero or
    non-finite pivot or a non-finite lambda makes the grid's three gradient rows NaN; a grid without a base solution gets NaN rows,
    zero rows when all its incoming gradients are zero.  Other grids are unaffected.  A grid's gradient is bit-identical alone, in
    any batch, from run to run and with the two lines of any pair swapped, for the same pair list (another order of the list may
    change its last bits).

    Out of scope: batches that mix topologies, a generator with two lines, generator reactive limits and second derivatives (a
    generator with one line: ``ac_generator_contingency_screen_differentiable``).
    Contract: ``include/gns_powerflow.h``, "Gradients of the AC N-2 screen"."""
    return _ac_n2_screen(buses, lines, generators, B, L, G, slack_bus, pairs, rating, tol, max_iter, flows, states, True)


def _analysed_without(key, args, device, g):
    """The cached Newton-Raphson analysis of the topology ``_topology_key`` gave ``key`` and ``args`` for, without generator row
    ``g``: the analysis cache's entry of that topology and ``out_gen``."""
    cache = _analysis(_NR)[0]
    topo = cache.get(key + (g,))
    if topo is None:
        topo = cache[key + (g,)] = analyse_topology(*args, device=device, out_gen=g)
    return topo


def ac_generator_contingency_screen(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None, contingencies=None,
                                    pickup=None, rating=None, tol=1e-8, max_iter=10, flows=False, states=False):
    """AC generator contingency screening of every grid of a batch, on the device: Newton-Raphson on each ``(grid, row)`` of
    ``contingencies``, a generator out alone or with a line out as well (the combined N-1 set of a planner), with the outputs of
    ``ac_contingency_screen`` per row.  It is the AC check of the rows ``dc_generator_contingency_screen`` ranks: a unit trip takes
    the voltage support of its bus away, which the DC screen (``|V| = 1`` everywhere) cannot see.

    A generator outage leaves the Y-bus alone and may change the unknowns: the bus of a sole unit turns from PV to PQ, and on a bus
    with several units the set point may move.  Both depend on the topology and the unit alone, so the topology is analysed once per
    distinct generator of the list (``analyse_topology(..., out_gen=g)``, cached with the other analyses) and never per row or per
    grid; the line on top of the unit is ``ac_contingency_screen``'s Y-bus view on that analysis.  ``newton_raphson(
    mixed_topologies=True)`` on the expanded batch would analyse one topology per distinct row and hold a copy of the inputs per row.

    Inputs, column maps, the slack, the device handling, ``rating``, ``tol`` and ``max_iter`` are those of
    ``ac_contingency_screen``; the whole batch shares one topology.  ``contingencies`` and ``pickup`` are those of
    ``dc_generator_contingency_screen``: a ``[P,2]`` integer tensor, array or sequence of ``(generator, line)``, 0-based generator
    rows and line indices, line -1 for "no line out"; default, for each generator in order, ``(g,-1), (g,0), ..., (g,E-1)``
    (``Gn (E + 1)`` rows, so the two screens line up row for row).  Duplicates are independent rows.

    Row ``(grid, (g, k))`` is Newton-Raphson on the grid with generator row ``g`` deleted and, when ``k >= 0``, line ``k`` out of
    service, which is what ``newton_raphson`` computes on those inputs:
      roles       the slack stays the slack; the bus of ``g`` stays PV when another generator is listed on it, otherwise it becomes a
                  PQ bus (``|V|`` an unknown, the Q equation solved with ``Qsp = -Qd``)
      set points  ``|V|`` at a PV or slack bus is ``vg`` of the first remaining generator listed on it (the outage of the first-listed
                  unit of a shared bus moves the set point to the next unit's); a slack with none left takes 1
      injections  ``Psp_i`` = the sum of ``Pg`` over the remaining generators of bus ``i``, plus their pickup, minus ``Pd_i``.
                  ``pickup``: None, the slack picks the lost ``Pg_g`` up; ``'pmax'`` or weights ``[Gn]`` / ``[Bt,Gn]`` (non-negative,
                  finite, float64), generator ``h != g`` injects ``Pg_g w_h / W_g`` more, ``W_g`` the sum of the others' weights in
                  generator-row order; when ``W_g`` is exactly 0 the slack picks up.  No Pmax or Pmin limit is enforced, and in AC the
                  slack also takes the change of the losses, whatever the pickup.
      start       ``|V|`` at the row's PQ buses from ``base.v`` (a freed bus starts at its old set point), ``theta = base.theta -
                  base.theta[slack]``, ``|V|`` at PV and slack buses from the row's set points
    The convergence test, the update, ``max_iter``, the failure rules, the branch flows (all four exactly 0 at line ``k``), the
    summaries and their order (the lowest index among equals, NaN first) are ``ac_contingency_screen``'s.

    Returns ``AcGeneratorContingencyResult``, ``AcContingencyResult``'s fields with ``contingencies`` in place of ``outages``:
      base           the ``PowerFlowResult`` of ``newton_raphson`` on the same inputs with the same ``tol`` and ``max_iter``, bit for bit
      contingencies  ``[P,2]`` int64, as given
      v, theta       None by default; with ``states=True`` ``[Bt,P,N]`` float64, the post-outage state
      p_from, q_from, p_to, q_to   None by default; with ``flows=True`` ``[Bt,P,E]`` float64
      worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus, converged, iterations, mismatch   ``[Bt,P]``, as
                     ``ac_contingency_screen`` returns them
      islanding      ``[P]`` bool: the row's line is a bridge of the topology (found on the host and kept with the topology); a generator
                     outage alone never islands
    An islanding row has NaN / -1 / ``converged`` False / ``iterations`` -1 in every grid; so has every row of a grid whose base
    solve did not converge.  A row that does not converge keeps its last finite iterate with ``converged`` False.  Every row is
    bit-identical alone, in any batch, in any list or order that holds it, with any of ``flows`` / ``states``, and from run to run.
    With a 2-D single grid the batch dimension is dropped.

    The outputs are not differentiable: the call runs as under ``torch.no_grad()``, and ``requires_grad`` on an input is ignored
    without an error; the same call with a backward on the device is ``ac_generator_contingency_screen_differentiable``.
    Out of scope: reactive limits on the remaining units, Pmax / Pmin limits on the pickup, batches that mix topologies, a generator
    with two lines.  Contract: ``include/gns_powerflow.h``, "AC generator contingency screening"."""
    return _ac_generator_screen(buses, lines, generators, B, L, G, slack_bus, contingencies, pickup, rating, tol, max_iter, flows,
                                states, False)


class _ACG1Function(torch.autograd.Function):
    """``ac_generator_contingency_screen_differentiable`` when an input requires grad: ``_ACN1Function`` with the pickup weights as
    ``_DCN1Function`` takes them.  The forward is the screen's launch (the fifteen outputs in ``gns_acg1_screen``'s order, ``v`` and
    ``theta`` always there), the backward one ``gns_acg1_adjoint`` call on the forward's set of analyses, lists and state.
    ``weights`` (None, or the pickup weights ``[Gn]`` / ``[Bt,Gn]`` float64) is on the graph for its gradient alone, the adjoint's
    fourth output: the kernels read the values the forward uploaded.  A ``[Gn]`` tensor gets the sum over the grids."""

    @staticmethod
    def forward(ctx, screen, adjoint, buses, lines, gens, weights):
        out = screen(buses, lines, gens)
        v, theta, _, _, _, _, _, worst_line, _, v_min_bus, _, v_max_bus, conv, iters, mis = out
        ctx.mark_non_differentiable(worst_line, v_min_bus, v_max_bus, conv, iters, mis)
        ctx.set_materialize_grads(False)
        ctx.adjoint = adjoint
        ctx.shared_weights = weights is not None and weights.dim() == 1
        ctx.save_for_backward(buses, lines, gens, v, theta, conv, worst_line, v_min_bus, v_max_bus)
        return tuple(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, gv, gth, gpf, gqf, gpt, gqt, gwl, _gwi, gvmin, _gi0, gvmax, _gi1, _gconv, _giters, _gmis):
        buses, lines, gens, *state = ctx.saved_tensors
        gb, gl, gg, gp = ctx.adjoint(buses, lines, gens, state, (gv, gth, gpf, gqf, gpt, gqt, gwl, gvmin, gvmax),
                                     ctx.needs_input_grad[2:6])
        if gp is not None and ctx.shared_weights:
            gp = gp.sum(dim=0)
        return (None, None, gb, gl, gg, gp)


def _ac_generator_screen(buses, lines, generators, B, L, G, slack_bus, contingencies, pickup, rating, tol, max_iter, flows, states,
                         differentiable):
    """``ac_generator_contingency_screen`` (``differentiable`` False) and ``ac_generator_contingency_screen_differentiable`` (True):
    one set-up, one set of analyses, one launch."""
    s = _screen_setup('ac_generator_contingency_screen', _NR, buses, lines, generators, B, L, G, slack_bus, contingencies, rating,
                      dict(flows=flows, states=states), differentiable, tol, max_iter, pickup=pickup)
    with torch.set_grad_enabled(s.grad):
        lib, cfg, Bt, dev, grad = s.lib, s.cfg, s.Bt, s.dev, s.grad
        target = _one_topology(s.topo)
        # the base case as newton_raphson solves it: its refusals come first, before any other analysis is made (a differentiated
        # call solves it below, after the backward's own refusal)
        base = None if grad else _solve(lib, _NR, cfg, target, *s.plain, None, None)
        # the distinct generators of the list, ascending, each with its analysis in the topology's set of them; a row as a
        # position into the generators and its line (-1: none)
        P = s.rows.shape[0]
        gen_np, gen_col = np.unique(s.rows[:, 0], return_inverse=True)
        set_cache = _analysis(_NR)[1]
        set_key = s.topo_key + ('out_gen',)
        members = set_cache.get(set_key)
        if members is None:
            members = set_cache[set_key] = _PfTopologySet(dev)
        off_np = np.array([members.add(s.topo_key + (g,), _analysed_without(s.topo_key, s.topo_args, dev, g)) for g in gen_np.tolist()])
        members.sync()
        (off_host, off_dev), (gen_host, gen_dev) = _upload32(off_np, dev), _upload32(gen_np, dev)
        cols_host, cols_dev = _upload32(np.stack([gen_col.reshape(P), s.rows[:, 1]], axis=1), dev)
        set_host, set_blob = members.host, members.blob          # this call's: a later call may grow the set
        lds = lambda: _set_lds_bytes(set_host, off_host)                         # noqa: E731

        def workspace_bytes(query):
            return _size_query(getattr(lib, query), query, (ctypes.byref(cfg), set_host.ctypes.data, set_host.size,
                                                            off_host.ctypes.data, off_host.size, Bt, P), lds, _ACG1.formula)

        def call(name, bu, li, ge, rest, ws):
            """One C call of the screen: the set, the inputs, the lists, the rating and the pickup, then ``rest``."""
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                _check(getattr(lib, name)(ctypes.byref(cfg), set_host.ctypes.data, set_blob.data_ptr(), set_host.size,
                                          off_host.ctypes.data, off_dev.data_ptr(), off_host.size, bu.data_ptr(), li.data_ptr(),
                                          ge.data_ptr(), Bt, gen_host.ctypes.data, gen_dev.data_ptr(), cols_host.ctypes.data,
                                          cols_dev.data_ptr(), P, s.isl_dev.data_ptr(), _ptr(s.rating),
                                          int(s.rating is not None and s.rating.dim() == 2), _ptr(s.pickup),
                                          int(s.pickup is not None and s.pickup.dim() == 2), *rest, ws.data_ptr(), ws.numel(), stream),
                       name, lds, _ACG1.formula)

        if grad:
            # the backward's own refusal (an oversize image, by name) comes before anything is launched
            workspace_bytes('gns_acg1_adjoint_workspace_bytes')
            base = list(_NRFunction.apply(lambda *a: _solve(lib, _NR, cfg, target, *a, None, None),
                                          lambda *a: _adjoint(lib, cfg, target, *a), s.buses, s.lines, s.generators))
        base_conv = base[2].to(torch.uint8)
        base_state = (base[0].detach(), base[1].detach(), base_conv)      # the warm start is not differentiated

        def screen(bu, li, ge):
            ws = _gns._workspace(workspace_bytes('gns_acg1_workspace_bytes'), dev)
            out = _ac_screen_outputs(s, P, states or grad, flows)
            call('gns_acg1_screen', bu, li, ge, (*(t.data_ptr() for t in base_state), *map(_ptr, out)), ws)
            return out

        def adjoint(bu, li, ge, state, incoming, need):
            """One adjoint call at the forward's ``state`` (v, theta, converged, worst_line, v_min_bus, v_max_bus)."""
            gin = [torch.empty_like(t) if n else None for t, n in zip((bu, li, ge), need)]
            gin.append(torch.empty(Bt, ge.shape[1], dtype=torch.float64, device=dev) if need[3] else None)
            incoming = [None if g is None else g.to(device=dev, dtype=torch.float64).contiguous() for g in incoming]
            ws = _gns._workspace(workspace_bytes('gns_acg1_adjoint_workspace_bytes'), dev)
            call('gns_acg1_adjoint', bu, li, ge, (*(t.data_ptr() for t in state), base_conv.data_ptr(), *map(_ptr, incoming),
                                                  *map(_ptr, gin)), ws)
            return gin

        if grad:
            # the weights as the graph sees them: column 1 of the canonical generators for 'pmax', the caller's tensor when it
            # requires grad; anything else takes no gradient (grad_pickup is then NULL)
            weights = None
            if isinstance(pickup, str):
                weights = s.generators[:, :, 1].to(torch.float64)
            elif isinstance(pickup, torch.Tensor) and pickup.requires_grad:
                weights = pickup.to(device=dev, dtype=torch.float64).reshape(s.pickup.shape)
            res = list(_ACG1Function.apply(screen, adjoint, s.buses, s.lines, s.generators, weights))
            if not states:
                res[0] = res[1] = None
        else:
            res = screen(*s.plain)
        base, rows_t, res, islanding = _screen_results(s, base, res, 12)
        return AcGeneratorContingencyResult(PowerFlowResult(*base), rows_t, *res, islanding)


def ac_generator_contingency_screen_differentiable(buses, lines, generators, B=None, L=None, G=None, *, slack_bus=None,
                                                   contingencies=None, pickup=None, rating=None, tol=1e-8, max_iter=10, flows=False,
                                                   states=False):
    """``ac_generator_contingency_screen`` with gradients: the same arguments, the same ``AcGeneratorContingencyResult`` with every
    forward output and ``base.*`` bit-identical to that call's, and a backward on the device, as
    ``ac_n2_contingency_screen_differentiable`` and ``dc_generator_contingency_screen_differentiable`` have one.  It is the last step
    of the planner's workflow for unit trips (``dc_generator_contingency_screen`` over the combined N-1 set, the worst rows checked
    in AC here) for a security-constrained loss or a sensitivity study of the dispatch, the set points and the participation factors.

    With grad mode on and ``requires_grad`` on an input (or on a tensor ``pickup``), ``v``, ``theta``, the four flows,
    ``worst_loading``, ``v_min`` and ``v_max`` are differentiable through one ``gns_acg1_adjoint`` call on the forward's set of
    analyses, lists and state (per row the implicit function theorem on the grid without the generator row and the line, on that
    generator's own analysis: one factorisation of the row's Jacobian and one transposed solve; Newton is not run again), and
    ``base.v`` / ``base.theta`` through ``newton_raphson``'s adjoint.  Otherwise it is the plain call and returns plain tensors.

    The derivative is exact at the returned state with respect to ``newton_raphson``'s columns (``Pd, Qd, Gs, Bs``; the lines'
    ``r, x, b, tau, shift``; ``Pg`` and ``vg``); every other column gets 0, and row ``(g,k)`` gives exactly 0 to line ``k``'s own
    columns.  What the lost unit changes:
      roles    the unknowns are the row's: a freed sole-unit bus is PQ, so its ``Qd`` and ``Bs`` take a gradient and no ``vg`` does;
               its start value, the old set point, is not differentiated
      vg       goes to the first remaining unit listed on a PV or slack bus (the next unit of a shared bus when the first is out);
               the lost unit's ``vg`` gets exactly 0, and a slack with no unit left has the constant ``|V| = 1``
      Pg       a remaining unit gets ``mu_h``, the multiplier of its bus's P equation (0 at the slack); the lost unit gets
               ``sum_{h != g} mu_h w_h / W_g``, what its output does through the units that pick it up, and exactly 0 when the slack
               picks up (``pickup=None``, or ``W_g`` exactly 0)
      weights  ``dl/dw_h = Pg_g (mu_h - M) / W_g`` for ``h != g`` with ``M`` that weighted mean, 0 for ``h = g``.  With
               ``pickup='pmax'`` it is added into the generators' column 1, which joins the contract for this pickup only; a tensor
               ``pickup`` that requires grad receives it in its own dtype, a ``[Gn]`` tensor the sum over the grids; otherwise it is
               not computed.  The ``W_g == 0`` branch is not differentiated: it gives the weights 0.
    ``rating`` is a constant and the warm start is not differentiated.  ``worst_loading`` sends its gradient to ``worst_line``, at
    the end that attains the maximum (the from end on equality), ``v_min`` / ``v_max`` to the buses reported; the index outputs,
    ``converged``, ``iterations``, ``mismatch``, ``islanding`` and ``contingencies`` are not differentiable.

    With ``states=False`` (the default) the summaries and the flows stay differentiable: ``v`` and ``theta`` are then kept for the
    backward (``16 Bt P N`` bytes until it has run) and not returned.

    A row whose incoming gradients are all exactly zero or absent is skipped, never multiplied by zero (a loss that indexes
    ``converged`` rows); a non-zero gradient into a row that is not converged (an islanding row, a stopped iteration), a zero or
    non-finite pivot or a non-finite lambda makes the grid's gradient rows NaN, the weights' row included; a grid without a base
    solution gets NaN rows, zero rows when all its incoming gradients are zero.  Other grids are unaffected.  A grid's gradient is
    bit-identical alone, in any batch and from run to run for the same list (another order of the list may change its last bits).

    Out of scope: batches that mix topologies, reactive limits on the remaining units, Pmax / Pmin limits on the pickup, a generator
    with two lines, second derivatives.  Contract: ``include/gns_powerflow.h``, "Gradients of the AC generator screen"."""
    return _ac_generator_screen(buses, lines, generators, B, L, G, slack_bus, contingencies, pickup, rating, tol, max_iter, flows,
                                states, True)


_PFS_LDS_FORMULA = '40 N bytes per grid: five bus vectors'
_PFS = _Solver('gns_pfs', PowerFlowTopology, _PFS_LDS_FORMULA)   # the solved case: Newton-Raphson's analysis, its own small LDS image

# the [Bt,E] / [Bt,N] / [Bt,Gn] float64 outputs of gns_pfs_evaluate in its order, then its [Bt] outputs with their dtypes
_PFS_ROWS = (('p_from', 'E'), ('q_from', 'E'), ('p_to', 'E'), ('q_to', 'E'), ('p_inj', 'N'), ('q_inj', 'N'), ('gen_p', 'Gn'),
             ('gen_q', 'Gn'))
_PFS_SCALARS = (('mismatch', torch.float64), ('slack_p', torch.float64), ('worst_loading', torch.float64), ('worst_line', torch.int32),
                ('v_min', torch.float64), ('v_min_bus', torch.int32), ('v_max', torch.float64), ('v_max_bus', torch.int32))
_PFS_C_ORDER = tuple(n for n, _ in _PFS_ROWS) + tuple(n for n, _ in _PFS_SCALARS)
# the differentiable outputs in the order gns_pfs_adjoint takes their incoming gradients
_PFS_DIFF = ('p_from', 'q_from', 'p_to', 'q_to', 'p_inj', 'q_inj', 'gen_p', 'gen_q', 'slack_p', 'worst_loading', 'v_min', 'v_max')


def solved_case(buses, lines, generators, v, theta, B=None, L=None, G=None, *, slack_bus=None, rating=None):
    """The solved case of an AC power flow at a given state, on the device: what PYPOWER's ``runpf`` returns next to the voltages
    (its ``pfsoln`` step) and the base row of the AC contingency screens, for every grid of a batch that shares one topology.  The
    state may be a solver's (``solved_case(b, l, g, *newton_raphson(b, l, g)[:2])``) or any other, such as a GNS prediction, which then
    gets the solver's own ``||F||_inf`` and the branch-model loadings.  The call evaluates at the state given and iterates nothing.

    ``buses``, ``lines``, ``generators``, the column maps ``B, L, G``, ``slack_bus`` and the device handling are ``newton_raphson``'s
    (one topology per call, analysed and cached as there; a batch whose id columns differ raises).  ``v``, ``theta``: ``[Bt,N]`` of
    any float dtype, used as float64 and as given (``theta`` is not shifted); with a 2-D single grid ``[N]`` is accepted.
    ``rating``: None (1), ``[E]`` or ``[Bt,E]``, positive and finite, as the AC screens take it.

    Returns ``SolvedCase``, float64 unless said, on the inputs' device:
      p_from, q_from, p_to, q_to   ``[Bt,E]``: the screens' branch flows on the line's own makeYbus stamps, ``S_f = V_f conj(Y_ff V_f +
                     Y_ft V_t)``, ``S_t = V_t conj(Y_tf V_f + Y_tt V_t)``; NaN at a line whose id columns are not buses of the grid
      p_inj, q_inj   ``[Bt,N]``: what each bus injects into the network, ``V_i conj(sum_k Y_ik V_k)`` on the Y-bus with its shunts
      mismatch       ``[Bt]``: Newton-Raphson's ``||F||_inf`` at this state (``|p_inj - Psp|`` at PV and PQ buses, ``|q_inj - Qsp|`` at PQ
                     buses), NaN when a term is not finite; at ``newton_raphson``'s result it is that call's ``mismatch`` bit for bit
      gen_p, gen_q   ``[Bt,Gn]``: a bus with n listed units produces ``q_inj + Qd``, shared equally among them (no limit ranges); ``gen_p``
                     is every unit's ``Pg`` as given, but the first unit listed on the slack, which carries ``p_inj + Pd`` of the
                     slack less the other slack units' ``Pg``.  The ``qg`` column is not read
      slack_p        ``[Bt]``: ``p_inj + Pd`` of the slack less the ``Pg`` listed there: what the slack produces beyond its listed dispatch
                     (``dc_power_flow``'s ``slack_p``); defined for a slack without a unit too
      worst_loading  ``[Bt]``, ``max_l max(|S_f|, |S_t|) / rating_l``, with worst_line ``[Bt]`` int32
      v_min, v_max   ``[Bt]`` with v_min_bus, v_max_bus ``[Bt]`` int32 (0-based)
    The summaries have the AC screens' definitions and tie rules: the lowest index among equals, a NaN wins at the lowest index that
    holds one.  A grid's outputs are bit-identical alone, in any batch and from run to run; a NaN in a grid's state gives that grid
    NaN outputs and leaves the others alone.  With a 2-D single grid the batch dimension is dropped.

    Gradients: with grad mode on and ``requires_grad`` on any of ``buses`` / ``lines`` / ``generators`` / ``v`` / ``theta``, the four
    flows, ``p_inj``, ``q_inj``, ``gen_p``, ``gen_q``, ``slack_p``, ``worst_loading``, ``v_min`` and ``v_max`` are differentiable through one
    ``gns_pfs_adjoint`` launch (no linear solve: every term reduces to cotangents at the line ends and the bus shunts): ``v`` and
    ``theta`` at every bus, the slack included; ``Pd, Qd, Gs, Bs``; the lines' ``r, x, b, tau, shift``; the generators' ``Pg``.  Every
    other column gets 0 (``vg`` is not read by the forward); a line whose id columns are not buses gets a NaN row.  ``mismatch`` and
    the indices are not differentiable and ``rating`` is a constant.  ``worst_loading`` sends its gradient to ``worst_line`` at the end
    that attains the maximum (the from end on equality), ``v_min`` / ``v_max`` to the buses reported.  Because ``v`` and ``theta`` are
    ordinary inputs, a state that came from ``newton_raphson`` with ``requires_grad`` inputs backpropagates the total derivative
    through ``gns_pf_adjoint`` by autograd's chain.  A grid whose incoming gradients are all exactly zero gets exactly zero rows
    whatever its state (it is skipped, never multiplied by zero).  The forward's bits are the same with and without gradients; a
    grid's gradient is bit-identical alone, in any batch and from run to run.

    Out of scope: batches that mix topologies, second derivatives, reactive limits.
    Contract: ``include/gns_powerflow.h``, "The solved case"."""
    state_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (v, theta))
    with torch.no_grad():                    # the shapes first, so that a bad state or rating is refused where no device is visible too
        single, shaped, shaped_lines, _ = _as_batch(buses, lines, generators, B, L, G)
        Bt, N, E = shaped.shape[0], shaped.shape[1], shaped_lines.shape[1]
        rating = _rating(rating, Bt, E, single)
    v, theta = (torch.as_tensor(x) for x in (v, theta))
    state = []
    for name, x in (('v', v), ('theta', theta)):
        if not x.is_floating_point():
            raise ValueError(f'{name} must be a float tensor, got {x.dtype}')
        x = x.unsqueeze(0) if (single and x.dim() == 1) else x
        if tuple(x.shape) != (Bt, N):
            raise ValueError(f'v / theta must be [{Bt},{N}], got {tuple(x.shape)}')
        state.append(x)
    single, in_dev, buses, lines, generators, _, _ = _inputs(buses, lines, generators, B, L, G, None, None, 0.0, 0, False)
    dev = buses.device
    v, theta = (x.to(device=dev, dtype=torch.float64).contiguous() for x in state)
    rating = None if rating is None else rating.to(dev).contiguous()
    Gn = generators.shape[1]
    lib = load_library()
    cfg = PfConfig(N, E, Gn, 0, 0.0)
    plain = (buses.detach(), lines.detach(), generators.detach())
    topo = _topology(*plain, slack_bus)
    lds = 40 * N
    per_grid = int(rating is not None and rating.dim() == 2)
    head = (ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr())

    def evaluate(bu, li, ge, vv, th):
        out = {n: torch.empty(Bt, dict(E=E, N=N, Gn=Gn)[d], dtype=torch.float64, device=dev) for n, d in _PFS_ROWS}
        out.update({n: torch.empty(Bt, dtype=dt, device=dev) for n, dt in _PFS_SCALARS})
        ws = _gns._workspace(_size_query(lib.gns_pfs_workspace_bytes, 'gns_pfs_workspace_bytes', (*head[:2], Bt), lds, _PFS.formula), dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib.gns_pfs_evaluate(*head, bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt, vv.data_ptr(), th.data_ptr(),
                                        _ptr(rating), per_grid, *(out[n].data_ptr() for n in _PFS_C_ORDER), ws.data_ptr(), ws.numel(),
                                        stream), 'gns_pfs_evaluate', lds, _PFS.formula)
        return tuple(out[n] for n in SolvedCase._fields)

    def adjoint(bu, li, ge, vv, th, indices, incoming, need):
        """One adjoint call at the forward's state and indices (worst_line, v_min_bus, v_max_bus); ``need``: which of buses, lines,
        generators, v, theta want a gradient."""
        gb, gl, gg, gv, gth = (torch.empty_like(t) if n else None for t, n in zip((bu, li, ge, vv, th), need))
        incoming = [None if g is None else g.to(device=dev, dtype=torch.float64).contiguous() for g in incoming]
        nbytes = _size_query(lib.gns_pfs_adjoint_workspace_bytes, 'gns_pfs_adjoint_workspace_bytes', (*head[:2], Bt), lds, _PFS.formula)
        ws = _gns._workspace(nbytes, dev) if nbytes else None
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(lib.gns_pfs_adjoint(*head, bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt, vv.data_ptr(), th.data_ptr(), _ptr(rating),
                                       per_grid, *(t.data_ptr() for t in indices), *map(_ptr, incoming), *map(_ptr, (gv, gth, gb, gl, gg)),
                                       _ptr(ws), nbytes, stream), 'gns_pfs_adjoint', lds, _PFS.formula)
        return gb, gl, gg, gv, gth

    grad = torch.is_grad_enabled() and (state_grad or any(t.requires_grad for t in (buses, lines, generators)))
    if grad:
        out = list(_PFSFunction.apply(evaluate, adjoint, buses, lines, generators, v, theta))
    else:
        out = list(evaluate(*plain, v.detach(), theta.detach()))
    if in_dev != dev:
        out = [t.to(in_dev) for t in out]
    if single:
        out = [t[0] for t in out]
    return SolvedCase(*out)


class _PFSFunction(torch.autograd.Function):
    """``solved_case`` when an input or the state requires grad: the forward is the evaluation itself (``evaluate`` returns
    ``SolvedCase``'s fields in order), the backward one ``gns_pfs_adjoint`` call (``adjoint``) at the forward's state and indices."""

    @staticmethod
    def forward(ctx, evaluate, adjoint, buses, lines, gens, v, theta):
        out = evaluate(buses, lines, gens, v, theta)
        res = SolvedCase(*out)
        ctx.mark_non_differentiable(res.mismatch, res.worst_line, res.v_min_bus, res.v_max_bus)
        ctx.set_materialize_grads(False)
        ctx.adjoint = adjoint
        ctx.save_for_backward(buses, lines, gens, v, theta, res.worst_line, res.v_min_bus, res.v_max_bus)
        return tuple(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gout):
        buses, lines, gens, v, theta, *indices = ctx.saved_tensors
        g = SolvedCase(*gout)
        grads = ctx.adjoint(buses, lines, gens, v, theta, indices, [getattr(g, n) for n in _PFS_DIFF], ctx.needs_input_grad[2:7])
        return (None, None, *grads)


def _not_solved(Bt, N, dev):
    """The outputs of a batch none of whose topologies can be solved (each islands a bus)."""
    nan = float('nan')
    return [torch.full((Bt, N), nan, dtype=torch.float64, device=dev), torch.full((Bt, N), nan, dtype=torch.float64, device=dev),
            torch.zeros(Bt, dtype=torch.bool, device=dev), torch.full((Bt,), -1, dtype=torch.int32, device=dev),
            torch.full((Bt,), nan, dtype=torch.float64, device=dev)]


class _NRFunction(torch.autograd.Function):
    """``newton_raphson`` when an input requires grad: the forward is the solve itself (``solve``: the plain or the mixed launch, with
    its topology or ``MixedPlan`` already made), the backward one adjoint launch on the same analysis (``adjoint``:
    ``gns_pf_adjoint`` / ``gns_pf_adjoint_set``, include/gns_powerflow.h "Gradients").  It sees the canonical device tensors after
    ``_as_batch``: autograd routes the gradients back through the column maps, ``unsqueeze`` and ``.to``."""

    @staticmethod
    def forward(ctx, solve, adjoint, buses, lines, gens):
        v, theta, conv, iters, mis = solve(buses, lines, gens)
        ctx.mark_non_differentiable(conv, iters, mis)
        ctx.set_materialize_grads(False)
        ctx.adjoint = adjoint
        ctx.save_for_backward(buses, lines, gens, v, theta, conv)
        return v, theta, conv, iters, mis

    @staticmethod
    @once_differentiable
    def backward(ctx, gv, gth, _gconv, _giters, _gmis):
        buses, lines, gens, v, theta, conv = ctx.saved_tensors
        grads = ctx.adjoint(buses, lines, gens, v, theta, conv, gv, gth, ctx.needs_input_grad[2:5])
        return (None, None, *grads)


def _adjoint_args(buses, lines, gens, gv, gth, need):
    """The gradient outputs asked for (every element is written by the kernel) and the incoming gradients, contiguous."""
    gin = [torch.empty_like(t) if n else None for t, n in zip((buses, lines, gens), need)]
    gv, gth = (None if g is None else g.to(device=buses.device, dtype=torch.float64).contiguous() for g in (gv, gth))
    return gin, gv, gth


def _ptr(t):
    return None if t is None else t.data_ptr()


# Where a call launches: the suffix of its entry points, the arguments that name the blob(s) to the workspace query and to the
# launch itself (between cfg and the input tensors), the LDS image a refusal names (``_check``), and ``keep``.  The arguments are
# raw addresses, used as late as the backward: ``keep`` is never read, it holds their owners so that they outlive the target.
_Target = namedtuple('_Target', ['suffix', 'ws_args', 'args', 'lds', 'keep'])


def _one_topology(topo):
    """The target of a plain call: ``gns_*_solve`` / ``gns_pf_adjoint`` on the batch's one topology."""
    host = topo.host.ctypes.data
    return _Target('', (host,), (host, topo.blob.data_ptr()), topo.info['lds_bytes'], topo)


def _set_members(plan, set_bufs, cls=PowerFlowTopology):
    """The target of a mixed call: ``gns_*_solve_set`` / ``gns_pf_adjoint_set`` over ``plan`` (a ``MixedPlan`` of ``cls`` blobs) in
    the set as ``set_bufs = (host, blob)`` holds it.  None when every grid's topology islands a bus: there is nothing to launch."""
    host, blob = set_bufs
    members = plan.member_off
    if members.size == 0:
        return None
    ws_args = (host.ctypes.data, host.size, members.ctypes.data, members.size)
    return _Target('_set', ws_args, (ws_args[0], blob.data_ptr(), *ws_args[1:], plan.grid_off.data_ptr(), plan.order.data_ptr()),
                   lambda: _set_lds_bytes(host, members, cls), (plan, set_bufs))


def _launch(lib, solver, op, cfg, target, inputs, rest):
    """One launch of ``solver``'s entry point ``op`` on ``target``: the workspace its query asks for, then ``(cfg, the target's
    blobs, inputs, Bt, rest, workspace, stream)`` with the tensors by pointer (None: NULL), on the inputs' device and its current
    stream.  The library launches on the current device, so that is the inputs' for the length of the call."""
    Bt, dev = inputs[0].shape[0], inputs[0].device
    ws_name, ws_fn, name, fn = _entry_points(lib, solver.prefix, op, target.suffix)
    ws = _gns._workspace(_size_query(ws_fn, ws_name, (ctypes.byref(cfg), *target.ws_args, Bt), target.lds, solver.formula), dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(fn(ctypes.byref(cfg), *target.args, *map(_ptr, inputs), Bt, *map(_ptr, rest), ws.data_ptr(), ws.numel(), stream),
               name, target.lds, solver.formula)


def _size_query(fn, name, args, lds, formula):
    """The bytes a workspace query ``fn`` (``name``) answers for ``args``, its ``size_t`` out-parameter; ``lds`` and ``formula`` are
    what a refusal names (``_check``)."""
    nbytes = ctypes.c_size_t()
    _check(fn(*args, ctypes.byref(nbytes)), name, lds, formula)
    return nbytes.value


@functools.lru_cache(maxsize=None)
def _entry_points(lib, prefix, op, suffix):
    """Names and functions of the workspace query and of entry point ``op`` (resolved once, not per launch)."""
    ws_name, name = f'{prefix}_workspace_bytes{suffix}', f'{prefix}_{op}{suffix}'
    return ws_name, getattr(lib, ws_name), name, getattr(lib, name)


def _solve(lib, solver, cfg, target, buses, lines, generators, v0, theta0):
    """One solve launch (``gns_{pf,fd}_solve[_set]``) on ``target``; returns the five outputs as ``newton_raphson`` does."""
    Bt, N, dev = buses.shape[0], buses.shape[1], buses.device
    if target is None:
        return _not_solved(Bt, N, dev)
    out = _outputs(Bt, N, dev)
    _launch(lib, solver, 'solve', cfg, target, (buses, lines, generators), (v0, theta0, *out))
    v, theta, conv, iters, mis = out
    return [v, theta, conv.bool(), iters, mis]


def _adjoint(lib, cfg, target, buses, lines, gens, v, theta, conv, gv, gth, need):
    """One adjoint launch (``gns_pf_adjoint[_set]``) on the forward's ``target`` (no second analysis or classification), on the
    forward's device and stream; returns the gradients of the inputs ``need`` asks for."""
    Bt, dev = buses.shape[0], buses.device
    gin, gv, gth = _adjoint_args(buses, lines, gens, gv, gth, need)
    if target is None:
        return _unsolved_grads(gin, (gv, gth), Bt, dev)
    _launch(lib, _NR, 'adjoint', cfg, target, (buses, lines, gens), (v, theta, conv, gv, gth, *gin))
    return gin


def _unsolved_grads(gin, incoming, Bt, dev):
    """The gradients ``gin`` of a batch none of whose grids is solved: NaN rows, zero rows for a grid whose ``incoming`` gradients
    (``[Bt, ...]`` or None) are all zero."""
    zero = torch.ones(Bt, dtype=torch.bool, device=dev)
    for g in incoming:
        if g is not None:
            zero &= (g.reshape(Bt, -1) == 0).all(dim=1)
    fill = torch.where(zero, 0.0, float('nan')).to(torch.float32)
    for t in gin:
        if t is not None:
            t.copy_(fill.view(Bt, 1, 1).expand_as(t))
    return gin


def _adjoint_mixed(lib, cfg, plan, set_bufs, *args):
    """``_adjoint`` over a ``MixedPlan`` of Newton-Raphson blobs."""
    return _adjoint(lib, cfg, _set_members(plan, set_bufs), *args)


def _outputs(Bt, N, dev):
    v = torch.empty(Bt, N, dtype=torch.float64, device=dev)
    return (v, torch.empty_like(v), torch.empty(Bt, dtype=torch.uint8, device=dev), torch.empty(Bt, dtype=torch.int32, device=dev),
            torch.empty(Bt, dtype=torch.float64, device=dev))
