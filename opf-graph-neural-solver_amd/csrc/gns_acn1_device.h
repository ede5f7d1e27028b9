// What the AC contingency screens share, gns_acn1.hip (single outages and their adjoint) and gns_acn2.hip (double outages).  Device:
// the Y-bus view of a row (AcnYbus<M>: the base values but for the entries its M lines touch, with the predicate "line l is out"),
// an entry of the Y-bus without the view's lines, the prologue of a row (acn_view: the decision that the row is solved and its
// view, which the forward and the adjoint kernels both call), the outputs of a call with the writer of a row that is not solved,
// the row routine (acn_solve_row: Newton-Raphson, the extremes, the flows, the worst loading), the row kernel (gns_acn_kernel<M>:
// acn_view, then acn_solve_row) and the kernel that writes the base Y-bus of every grid.  Host: the workspace query and a screen
// call (acn_screen_call<Rows>) on the screen's trait.  Both screens are this code at M = 1 and M = 2.  gns_acg1.hip (generator
// outages, alone or with a line) has a kernel and an entry point of its own on a set of blobs and runs acn_view at M = 1 and
// acn_solve_row from here.
// What the solver and the solved case compute too is not written here: a line's stamp, its ends and the pattern search are
// gns_pf_device.h's; the Jacobian row on a view, a line's flows and loading, the total order of the reductions and the voltage
// extremes are gns_ac_device.h's.  Only Newton-Raphson's loop is restated (see acn_solve_row).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_ac_device.h"

namespace {

// The Y-bus of a row with M lines out: the grid's base values, but for the entries at p[0..4M-1] (ff, tt, ft, tf of the lowest
// line, then of the next; all one entry for a line from a bus to itself), which read y[0..4M-1].  Entries two lines share (the
// diagonal of a common bus, all four of parallel lines) appear more than once and hold the same value each time: the entry without
// every line of the row.  The same in every lane.  out and at unroll to M and 4M compare-selects.
template <int M>
struct AcnYbus {
  const double2* base;
  int k[M];               // the outaged lines, ascending
  int p[4 * M];
  double2 y[4 * M];
  __device__ __forceinline__ bool out(const int l) const {
    bool o = l == k[0];
#pragma unroll
    for (int u = 1; u < M; ++u) o = o || l == k[u];
    return o;
  }
  __device__ __forceinline__ double2 at(const int q) const {
    double2 v = base[q];
#pragma unroll
    for (int u = 0; u < 4 * M; ++u)
      if (q == p[u]) v = y[u];
    return v;
  }
};

// Entry p of row i of the Y-bus without the line(s) of the view Y (Y.out): pf_ybus_row's sum over the entry's stamps in their order,
// the outaged lines' skipped
template <class YB>   // an AcnYbus<M>
__device__ __forceinline__ double2 acn_entry_without(const int i, const int p, const YB& Y, const int32_t* y_diag,
                                                     const int32_t* st_ptr, const int32_t* st, const float* bus, const float* line) {
  double yr = 0.0, yi = 0.0;
  if (p == y_diag[i]) { yr = (double)bus[i * 6 + 4]; yi = (double)bus[i * 6 + 5]; }
  for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
    const int e = st[q] >> 2;
    if (Y.out(e)) continue;
    const double2 a = pf_stamp(line, e, st[q] & 3);
    yr += a.x; yi += a.y;
  }
  return make_double2(yr, yi);
}

// The prologue of a row, once for both screens and their adjoints: the view Y of grid `base` without the M lines that row `pos` of
// the list names, or false for a row that is not solved.  ok is what only the caller knows (no islanding row, a base solution; in
// the adjoint a converged row); the builder refuses a line that is not one of the grid's (its index, or its id columns against the
// blob's pattern) and, of a pair, twice the same line.  It orders a pair itself, so (j, k) and (k, j) are the same row bit for bit.
// line[] is read behind the index check, y_diag[] behind the ends' check, y[] filled only in a row that is solved: the lower
// line's ff, tt, ft, tf, then the higher line's.  The same decision in every lane.
template <int M>
__device__ __forceinline__ bool acn_view(bool ok, const int32_t* __restrict__ topo, const float* bus, const float* line,
                                         const int32_t* __restrict__ list, const int pos, const double2* base, AcnYbus<M>& Y) {
  static_assert(M == 1 || M == 2, "a row names one line or a pair");
  const int N = topo[PH_N], E = topo[PH_E];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];
  Y.base = base;
  if constexpr (M == 1) Y.k[0] = list[pos];
  else {
    Y.k[0] = min(list[2 * pos], list[2 * pos + 1]);
    Y.k[1] = max(list[2 * pos], list[2 * pos + 1]);
    ok = ok && Y.k[0] != Y.k[1];
  }
  ok = ok && Y.k[0] >= 0 && Y.k[M - 1] < E;
  int f[M] = {}, t[M] = {};
#pragma unroll
  for (int u = 0; u < M; ++u) ok = ok && pf_line_ends(line, Y.k[u], N, f[u], t[u]);
  if (ok) {
#pragma unroll
    for (int u = 0; u < M; ++u) {
      Y.p[4 * u] = y_diag[f[u]];
      Y.p[4 * u + 1] = y_diag[t[u]];
      Y.p[4 * u + 2] = pf_find_entry(y_ptr, y_col, f[u], t[u]);
      Y.p[4 * u + 3] = pf_find_entry(y_ptr, y_col, t[u], f[u]);
      ok = ok && Y.p[4 * u + 2] >= 0 && Y.p[4 * u + 3] >= 0;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int u = 0; u < M; ++u) {
    Y.y[4 * u] = acn_entry_without(f[u], Y.p[4 * u], Y, y_diag, st_ptr, st, bus, line);
    Y.y[4 * u + 1] = acn_entry_without(t[u], Y.p[4 * u + 1], Y, y_diag, st_ptr, st, bus, line);
    Y.y[4 * u + 2] = acn_entry_without(f[u], Y.p[4 * u + 2], Y, y_diag, st_ptr, st, bus, line);
    Y.y[4 * u + 3] = acn_entry_without(t[u], Y.p[4 * u + 3], Y, y_diag, st_ptr, st, bus, line);
  }
  return true;
}

// The outputs of a call: rows [Bt * K] of the (grid, outage) pairs.  v, theta and each of the four flows may be NULL: not written.
struct Acn1Out {
  double* v;            // [Bt,K,N]
  double* theta;
  double* p_from;       // [Bt,K,E]
  double* q_from;
  double* p_to;
  double* q_to;
  double* worst;        // [Bt,K]
  int32_t* worst_line;
  double* v_min;
  int32_t* v_min_bus;
  double* v_max;
  int32_t* v_max_bus;
  uint8_t* conv;
  int32_t* iters;
  double* mis;
};

// NaN / -1 / converged 0 / iterations -1 in row `row`
__device__ __forceinline__ void acn1_row_not_solved(const Acn1Out& o, const size_t row, const int N, const int E) {
  const double nan = __builtin_nan("");
  const int lane = threadIdx.x;
  for (int i = lane; i < N; i += PF_THREADS) {
    if (o.v) o.v[row * N + i] = nan;
    if (o.theta) o.theta[row * N + i] = nan;
  }
  for (int l = lane; l < E; l += PF_THREADS) {
    if (o.p_from) o.p_from[row * E + l] = nan;
    if (o.q_from) o.q_from[row * E + l] = nan;
    if (o.p_to) o.p_to[row * E + l] = nan;
    if (o.q_to) o.q_to[row * E + l] = nan;
  }
  if (lane == 0) {
    o.worst[row] = nan; o.worst_line[row] = -1;
    o.v_min[row] = nan; o.v_min_bus[row] = -1;
    o.v_max[row] = nan; o.v_max_bus[row] = -1;
    o.conv[row] = 0; o.iters[row] = -1; o.mis[row] = nan;
  }
}

// A row of either AC screen after its kernel's prologue (the row decode, the decision that the row is solved, the Y-bus view Y of
// the grid without the row's line or lines): Newton-Raphson on gns_pf_kernel's LDS image from the base solution v0, th0 of grid g,
// then the state, the voltage extremes, the branch flows and the worst loading of the iterate into row `row` of o.  gns_pf_kernel's
// loop is restated here, once for both screens, rather than shared with it: pf_solve_grid stays as it is (its comments record what
// sharing cost).  The bus roles, the unknowns, the by-bus generator lists and the program are those of the blob at topo, whichever
// it is: the base topology's in the line screens, the analysis without the row's generator in gns_acg1.hip, whose pickup is the one
// hook here (Extra: what a bus's specified P gains on top of its generators' Pg; AcnNoExtra compiles to nothing).
struct AcnNoExtra {};

template <class YB, class Extra = AcnNoExtra>   // an AcnYbus<M>; a functor (bus, gen_ptr, gen_idx) -> double, or AcnNoExtra
__device__ __forceinline__ void acn_solve_row(const int32_t* __restrict__ topo, const float* bus, const float* line, const float* gen,
                                              const int g, const size_t row, const YB& Y, const double* __restrict__ rating,
                                              const int rating_per_grid, const double* __restrict__ v0,
                                              const double* __restrict__ th0, const int max_iter, const double tol, const Acn1Out& o,
                                              const Extra& extra = Extra()) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], slack = topo[PH_SLACK], dim = topo[PH_DIM];
  const int nnzLU = topo[PH_NNZLU], nsteps = topo[PH_NSTEPS];
  const int32_t* role = topo + topo[PH_ROLE];
  const int32_t* th_idx = topo + topo[PH_TH_IDX];
  const int32_t* vm_idx = topo + topo[PH_VM_IDX];
  const int32_t* gen_ptr = topo + topo[PH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[PH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* jslot = topo + topo[PH_JSLOT];
  const int32_t* pivot = topo + topo[PH_PIVOT];
  const int32_t* step_ptr = topo + topo[PH_STEP_PTR];
  const int2* ops = reinterpret_cast<const int2*>(topo + topo[PH_OPS]);

  double* F = lds;                       // [nnzLU] factor, then [dim] right-hand side / Newton step: gns_pf_kernel's image
  double* rhs = lds + nnzLU;
  double* Vm = rhs + dim;
  double* Va = Vm + N;
  double* Vr = Va + N;
  double* Vi = Vr + N;
  double* Ir = Vi + N;
  double* Ii = Ir + N;
  double* Psp = Ii + N;
  double* Qsp = Psp + N;

  // specified injections, bus roles and set points as in the base case; the warm start from the base solution
  for (int i = lane; i < N; i += PF_THREADS) {
    double pg = 0.0;
    for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) pg += (double)gen[gen_idx[q] * 7 + 6];
    if constexpr (!std::is_same_v<Extra, AcnNoExtra>) pg += extra(i, gen_ptr, gen_idx);
    Psp[i] = pg - (double)bus[i * 6 + 2];
    Qsp[i] = -(double)bus[i * 6 + 3];
    const int ro = role[i];
    double vm = 1.0, va = 0.0;
    if (ro != 0 && gen_ptr[i + 1] > gen_ptr[i]) vm = (double)gen[gen_idx[gen_ptr[i]] * 7 + 4];
    if (ro == 0) vm = v0[(size_t)g * N + i];
    if (ro != 2) va = th0[(size_t)g * N + i] - th0[(size_t)g * N + slack];
    Vm[i] = vm; Va[i] = va;
  }
  __syncthreads();

  int it = 0;
  bool conv = false;
  double mis = 0.0;
  for (;;) {
    for (int i = lane; i < N; i += PF_THREADS) { Vr[i] = Vm[i] * cos(Va[i]); Vi[i] = Vm[i] * sin(Va[i]); }
    __syncthreads();
    // mismatch F = [Re(V conj(YV)) - P ; Im(...) - Q] into the right-hand side, and its infinity norm
    double nrm = 0.0;
    bool bad = false;
    for (int i = lane; i < N; i += PF_THREADS) {
      double ir = 0.0, ii = 0.0;                 // I_i = sum_k Y_ik V_k: pf_row_current's sum on the pair's Y-bus
      for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
        const int c = y_col[p];
        const double2 y = Y.at(p);
        ir += y.x * Vr[c] - y.y * Vi[c];
        ii += y.x * Vi[c] + y.y * Vr[c];
      }
      Ir[i] = ir; Ii[i] = ii;
      if (th_idx[i] >= 0) {
        const double fp = (Vr[i] * ir + Vi[i] * ii) - Psp[i];
        rhs[th_idx[i]] = fp;
        nrm = fmax(nrm, fabs(fp));
        bad |= !pf_finite(fp);
      }
      if (vm_idx[i] >= 0) {
        const double fq = (Vi[i] * ir - Vr[i] * ii) - Qsp[i];
        rhs[vm_idx[i]] = fq;
        nrm = fmax(nrm, fabs(fq));
        bad |= !pf_finite(fq);
      }
    }
    nrm = pf_wave_max(nrm);
    if (__ballot(bad)) { mis = __builtin_nan(""); break; }
    mis = nrm;
    if (nrm < tol) { conv = true; break; }
    if (it >= max_iter) break;

    // Jacobian into its factor slots; fill slots, and the entries that lost their only line(s), are zeros
    for (int s = lane; s < nnzLU; s += PF_THREADS) F[s] = 0.0;
    __syncthreads();
    for (int i = lane; i < N; i += PF_THREADS)
      if (i != slack) ac_jacobian_row(i, slack, y_ptr, y_col, jslot, Y, Vm, Vr, Vi, Ir, Ii, F);
    __syncthreads();

    // the base topology's program: LU factorisation and both triangular solves
    pf_run_program(nsteps, step_ptr, ops, F, lane);

    // the update, only if every pivot is a finite non-zero and the new iterate is finite
    bad = pf_bad_pivot(dim, pivot, F, lane);
    for (int i = lane; i < N; i += PF_THREADS) {
      if (th_idx[i] >= 0) bad |= !pf_finite(Va[i] - rhs[th_idx[i]]);
      if (vm_idx[i] >= 0) bad |= !pf_finite(Vm[i] - rhs[vm_idx[i]]);
    }
    if (__ballot(bad)) break;
    for (int i = lane; i < N; i += PF_THREADS) {
      if (th_idx[i] >= 0) Va[i] -= rhs[th_idx[i]];
      if (vm_idx[i] >= 0) Vm[i] -= rhs[vm_idx[i]];
    }
    __syncthreads();
    ++it;
  }
  // every exit leaves Vr, Vi at the iterate Vm, Va hold: the state the flows and the summaries are computed from

  // the state and the voltage extremes, a bus per lane (the lowest of equal buses)
  const AcExtremes ex = ac_voltage_extremes(N, Vm, lane, [&](const int i, const double vm) {
    if (o.v) o.v[row * N + i] = vm;
    if (o.theta) o.theta[row * N + i] = Va[i];
  });

  // the branch flows, a line per lane, on the line's own stamps: zeros at the outaged line(s); NaN at a line whose id columns are
  // not buses of the grid
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  double best = -1.0;
  int bi = INT32_MAX;
  for (int l = lane; l < E; l += PF_THREADS) {
    AcFlows s = {0.0, 0.0, 0.0, 0.0};
    int a, b;
    if (!pf_line_ends(line, l, N, a, b)) s.pf = s.qf = s.pt = s.qt = __builtin_nan("");
    else if (!Y.out(l)) s = ac_line_flows(line, l, a, b, Vr, Vi);
    if (o.p_from) o.p_from[row * E + l] = s.pf;
    if (o.q_from) o.q_from[row * E + l] = s.qf;
    if (o.p_to) o.p_to[row * E + l] = s.pt;
    if (o.q_to) o.q_to[row * E + l] = s.qt;
    const double load = ac_loading(s, rt, l);
    if (ac_before(load, l, best, bi)) { best = load; bi = l; }
  }
  ac_wave_first(best, bi);

  if (lane == 0) {
    o.worst[row] = best; o.worst_line[row] = bi;
    o.v_min[row] = -ex.lo; o.v_min_bus[row] = ex.lo_i;
    o.v_max[row] = ex.hi; o.v_max_bus[row] = ex.hi_i;
    o.conv[row] = conv ? 1 : 0; o.iters[row] = it; o.mis[row] = mis;
  }
}

// The row kernel of both screens, M lines out per row: workgroup blockIdx.x = grid * K + position in the list (M ints per row)
template <int M>
__global__ __launch_bounds__(PF_THREADS) void gns_acn_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                             const float* __restrict__ lines, const float* __restrict__ gens,
                                                             const int32_t* __restrict__ list, const int K,
                                                             const uint8_t* __restrict__ islanding,
                                                             const double* __restrict__ rating, const int rating_per_grid,
                                                             const double* __restrict__ v0, const double* __restrict__ th0,
                                                             const uint8_t* __restrict__ conv0,
                                                             const double2* __restrict__ ybus_ws, const int max_iter,
                                                             const double tol, const Acn1Out o) {
  const size_t row = blockIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)K), pos = (int)(blockIdx.x % (unsigned)K);
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], nnzY = topo[PH_NNZY];
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;

  // the row's Y-bus, or a row that is not solved: an islanding row, a grid without a base solution, what acn_view refuses
  AcnYbus<M> Y;
  if (!acn_view(!islanding[pos] && conv0[g] != 0, topo, bus, line, list, pos, ybus_ws + (size_t)g * nnzY, Y)) {
    acn1_row_not_solved(o, row, N, E);
    return;
  }
  acn_solve_row(topo, bus, line, gen, g, row, Y, rating, rating_per_grid, v0, th0, max_iter, tol, o);
}

// The base Y-bus of every grid into the workspace: a wave per grid, a row per lane (what gns_pf_kernel writes for itself)
__global__ __launch_bounds__(PF_THREADS) void gns_acn1_ybus_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                   const float* __restrict__ lines, double2* __restrict__ ybus_ws) {
  const int g = blockIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], nnzY = topo[PH_NNZY];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  double2* Y = ybus_ws + (size_t)g * nnzY;
  for (int i = threadIdx.x; i < N; i += PF_THREADS) pf_ybus_row(i, y_ptr, y_diag, st_ptr, st, bus, line, Y);
}

// ---- host: what gns_acn1_screen and gns_acn2_screen (and their workspace queries) do alike

// The workspace of either screen: one base Y-bus per grid, whatever the number of rows
inline int acn_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_row, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_row <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h)) return GNS_EINVAL;
  *bytes = pf_ws_bytes_nnzy(h[PH_NNZY], Bt);
  return GNS_OK;
}

// A screen call, in the order the codes win: the arguments, the blob's header, the list (Rows::list_ok: the screen's own check of
// its n_row outages or pairs against the blob at h), a workgroup per (grid, row) in one launch, the workspace and the LDS image
// (pf_check_topology); then two launches: the base Y-bus of every grid into the workspace, and the row kernel at Rows::M lines out.
// Rows is the screen's trait (Acn1Rows in gns_acn1.hip, Acn2Pairs in gns_acn2.hip): M, list_ok and the adjoint's chunk rule.
template <class Rows>
int acn_screen_call(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev, const float* buses, const float* lines,
                    const float* generators, int64_t Bt, const int32_t* list_host, const int32_t* list_dev, int32_t n_row,
                    const uint8_t* islanding, const double* rating, int32_t rating_per_grid, const double* base_v,
                    const double* base_theta, const uint8_t* base_converged, double* v, double* theta, double* p_from,
                    double* q_from, double* p_to, double* q_to, double* worst_loading, int32_t* worst_line, double* v_min,
                    int32_t* v_min_bus, double* v_max, int32_t* v_max_bus, uint8_t* converged, int32_t* iterations,
                    double* mismatch, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pf_config_ok(cfg) || !topo_host || !topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF ||
      !list_host || !list_dev || n_row <= 0 || !islanding || (rating_per_grid != 0 && rating_per_grid != 1) || !base_v ||
      !base_theta || !base_converged || !worst_loading || !worst_line || !v_min || !v_min_bus || !v_max || !v_max_bus || !converged ||
      !iterations || !mismatch || !workspace)
    return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h) || !Rows::list_ok(h, list_host, n_row)) return GNS_EINVAL;
  int64_t rows = 0, lds = 0;
  if (!pf_chunks(n_row, 1, Bt, &rows)) return GNS_EINVAL;
  const int rc = pf_check_topology<PfBlobKind>(cfg, h, Bt, workspace_bytes, &lds);
  if (rc != GNS_OK) return rc;
  const Acn1Out out = {v, theta, p_from, q_from, p_to, q_to, worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus,
                       converged, iterations, mismatch};
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  const int rc0 = pf_launch<gns_acn1_ybus_kernel>(Bt, 0, stream, topo, buses, lines, static_cast<double2*>(workspace));
  if (rc0 != GNS_OK) return rc0;
  return pf_launch<gns_acn_kernel<Rows::M>>(Bt * n_row, lds, stream, topo, buses, lines, generators, list_dev, (int)n_row, islanding,
                                            rating, (int)rating_per_grid, base_v, base_theta, base_converged,
                                            static_cast<const double2*>(workspace), cfg->max_iter, cfg->tol, out);
}

}  // namespace
