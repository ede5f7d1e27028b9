// The device helpers of the AC contingency screens that gns_acn1.hip (single outages and their adjoint) and gns_acn2.hip (double
// outages) share: a line's Y-bus stamps, an entry of the Y-bus without one or two lines, the Y-bus view of a pair (the base values
// but for the entries its lines touch), the Jacobian row on such a view, the total order of the reductions, the outputs of a call
// with the writer of a row that is not solved, and the kernel that writes the base Y-bus of every grid.  Both screens run this
// code, so a row of the double-outage screen is computed with the single-outage screen's arithmetic, expression for expression.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"

namespace {
// Stamp `kind` (0 ff, 1 tt, 2 ft, 3 tf) of line e as (Re, Im): pf_ybus_row's arithmetic, expression for expression
__device__ __forceinline__ double2 acn1_stamp(const float* line, const int e, const int kind) {
  const double r = line[e * 7 + 2], x = line[e * 7 + 3], b = line[e * 7 + 4], tau = line[e * 7 + 5], sh = line[e * 7 + 6];
  const double den = r * r + x * x;
  const double ysr = r / den, ysi = -x / den;
  double ar, ai;
  if (kind == 0) { ar = ysr / (tau * tau); ai = (ysi + 0.5 * b) / (tau * tau); }
  else if (kind == 1) { ar = ysr; ai = ysi + 0.5 * b; }
  else {
    const double c = cos(sh), s = kind == 2 ? sin(sh) : -sin(sh);   // -y_s e^{+-j shift} / tau
    ar = -(ysr * c - ysi * s) / tau;
    ai = -(ysr * s + ysi * c) / tau;
  }
  return make_double2(ar, ai);
}

// Entry p of row i of the Y-bus without line k: pf_ybus_row's sum over the entry's stamps in their order, line k's skipped
__device__ __forceinline__ double2 acn1_entry_without(const int i, const int p, const int k, const int32_t* y_diag,
                                                      const int32_t* st_ptr, const int32_t* st, const float* bus, const float* line) {
  double yr = 0.0, yi = 0.0;
  if (p == y_diag[i]) { yr = (double)bus[i * 6 + 4]; yi = (double)bus[i * 6 + 5]; }
  for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
    const int e = st[q] >> 2;
    if (e == k) continue;
    const double2 a = acn1_stamp(line, e, st[q] & 3);
    yr += a.x; yi += a.y;
  }
  return make_double2(yr, yi);
}

// Entry p of row i of the Y-bus without lines j and k: the same sum with both lines' stamps skipped
__device__ __forceinline__ double2 acn2_entry_without(const int i, const int p, const int j, const int k, const int32_t* y_diag,
                                                      const int32_t* st_ptr, const int32_t* st, const float* bus, const float* line) {
  double yr = 0.0, yi = 0.0;
  if (p == y_diag[i]) { yr = (double)bus[i * 6 + 4]; yi = (double)bus[i * 6 + 5]; }
  for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
    const int e = st[q] >> 2;
    if (e == j || e == k) continue;
    const double2 a = acn1_stamp(line, e, st[q] & 3);
    yr += a.x; yi += a.y;
  }
  return make_double2(yr, yi);
}

// The Y-bus entry (i, k) of the blob's CSR pattern (columns ascending), -1 if it is not there
__device__ __forceinline__ int acn1_find_entry(const int32_t* y_ptr, const int32_t* y_col, const int i, const int k) {
  int lo = y_ptr[i], hi = y_ptr[i + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (y_col[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo < y_ptr[i + 1] && y_col[lo] == k ? lo : -1;
}

// The 0-based ends of line e from its id columns (those the blob was prepared from); false unless both are buses of the grid
__device__ __forceinline__ bool acn1_line_ends(const float* line, const int e, const int N, int& f, int& t) {
  const float ff = line[e * 7 + 0], ft = line[e * 7 + 1];
  f = (int)ff - 1; t = (int)ft - 1;
  return ff == (float)(f + 1) && ft == (float)(t + 1) && f >= 0 && f < N && t >= 0 && t < N;
}

// The Y-bus of a pair: the grid's base values, but for the entries at p[0..3] (the outaged line's ff, tt, ft, tf; all one entry for
// a line from a bus to itself), which read y[0..3].  The same in every lane.
struct Acn1Ybus {
  const double2* base;
  int p[4];
  double2 y[4];
  __device__ __forceinline__ double2 at(const int q) const {
    double2 v = base[q];
    if (q == p[0]) v = y[0];
    if (q == p[1]) v = y[1];
    if (q == p[2]) v = y[2];
    if (q == p[3]) v = y[3];
    return v;
  }
};

// The Y-bus of a double outage: the base values, but for the entries at p[0..7] (ff, tt, ft, tf of the lower line, then of the
// higher), which read y[0..7].  Entries the two lines share (the diagonal of a common bus, all four of parallel lines) appear more
// than once and hold the same value each time: the entry without both lines.  The same in every lane.
struct Acn2Ybus {
  const double2* base;
  int p[8];
  double2 y[8];
  __device__ __forceinline__ double2 at(const int q) const {
    double2 v = base[q];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (q == p[u]) v = y[u];
    return v;
  }
};

// Row i (not the slack) of the Jacobian into its factor slots: gns_powerflow.hip's pf_jacobian_row on the pair's Y-bus
template <class YB>   // Acn1Ybus or Acn2Ybus
__device__ __forceinline__ void acn1_jacobian_row(const int i, const int slack, const int32_t* y_ptr, const int32_t* y_col,
                                                  const int32_t* jslot, const YB& Y, const double* Vm, const double* Vr,
                                                  const double* Vi, const double* Ir, const double* Ii, double* F) {
  const double vri = Vr[i], vii = Vi[i];
  for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
    const int k = y_col[p];
    if (k == slack) continue;
    const double2 y = Y.at(p);
    const double a = y.x * Vr[k] - y.y * Vi[k], b = y.x * Vi[k] + y.y * Vr[k];   // Y_ik V_k
    const double cr = vri * a + vii * b, ci = vii * a - vri * b;                 // V_i conj(Y_ik V_k)
    double dar = ci, dai = -cr;                                                  // dS_i / dtheta_k
    double dmr = cr, dmi = ci;                                                   // |V_k| dS_i / d|V_k|
    if (k == i) {
      const double P = vri * Ir[i] + vii * Ii[i], Q = vii * Ir[i] - vri * Ii[i];
      dar -= Q; dai += P;
      dmr += P; dmi += Q;
    }
    dmr /= Vm[k]; dmi /= Vm[k];
    const int s0 = jslot[4 * p], s1 = jslot[4 * p + 1], s2 = jslot[4 * p + 2], s3 = jslot[4 * p + 3];
    if (s0 >= 0) F[s0] = dar;
    if (s1 >= 0) F[s1] = dmr;
    if (s2 >= 0) F[s2] = dai;
    if (s3 >= 0) F[s3] = dmi;
  }
}

// Whether v at index i comes before the best so far (at index bi): larger, or equal at a lower index; NaN comes before everything
__device__ __forceinline__ bool acn1_before(const double v, const int i, const double best, const int bi) {
  if (v != v) return best == best || i < bi;
  if (best != best) return false;
  return v > best || (v == best && i < bi);
}

// The first of the wave's (best, bi) in acn1_before's order, in every lane: a total order, so the tree's shape does not matter
__device__ __forceinline__ void acn1_wave_first(double& best, int& bi) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (acn1_before(ov, oi, best, bi)) { best = ov; bi = oi; }
  }
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

}  // namespace
