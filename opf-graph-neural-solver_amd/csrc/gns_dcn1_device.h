// The device helpers of the DC contingency screens that gns_dcn1.hip (single outages and their adjoint), gns_dcn2.hip (double
// outages) and gns_dcg1.hip (generator and generator-plus-line outages) share: the LDS image of a screen workgroup, the base case of
// a grid as gns_dc_kernel solves it, a lane's own solve of z_k on the base factor, the post-outage flow of a line and the total order
// of the worst-loading reductions.  Every screen runs this code, so z_k and the base flows of the
// other screens are the single-outage screen's bit for bit.  At the end, what the adjoints share: the worst line's term, the scan for
// non-zero incoming gradients, the status of a chunk's partial, and the kernel that reduces the partials, applies the contract and
// writes the fp32 gradient rows (and its parts, for the generator screen's own reduce kernel).  What only the screens with a factor
// kernel and a streaming row kernel share is in gns_dcn2_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"

namespace {

constexpr int DCN1_PREFETCH = 8;   // operations of the solve program a lane fetches ahead of running them

// The B' solve program of the blob on one lane's own right-hand side zc[slot * ld], in the blob's order (steps in order, the
// operations of a step are independent), the factor F read-only.  In a solve program dst and b are right-hand-side slots
// (nnz1 + position) and a is a factor slot (SymLU::solve_ops).
__device__ __forceinline__ void dcn1_lane_solve(const int nops, const int2* ops, const double* F, const int nnz1, double* zc,
                                                const int ld) {
  for (int q0 = 0; q0 < nops; q0 += DCN1_PREFETCH) {
    int2 op[DCN1_PREFETCH];
#pragma unroll
    for (int u = 0; u < DCN1_PREFETCH; ++u) op[u] = ops[min(q0 + u, nops - 1)];
#pragma unroll
    for (int u = 0; u < DCN1_PREFETCH; ++u) {
      if (q0 + u >= nops) break;
      const int dst = ((op[u].x & 0xFFFF) - nnz1) * ld, a = (int)((uint32_t)op[u].x >> 16);
      if (op[u].y < 0) zc[dst] = zc[dst] / F[a];
      else zc[dst] -= F[a] * zc[(op[u].y - nnz1) * ld];
    }
  }
}

// Whether loading v at line i is worse than the worst so far (best at line bi): larger, or equal at a lower line; NaN is worst of all
__device__ __forceinline__ bool dcn1_worse(const double v, const int i, const double best, const int bi) {
  if (v != v) return best == best || i < bi;
  if (best != best) return false;
  return v > best || (v == best && i < bi);
}

// NaN / -1 in the rows of outages k0 .. k0 + nk of grid g
__device__ __forceinline__ void dcn1_rows_not_solved(const int g, const int K, const int E, const int k0, const int nk, double* fl_out,
                                                     double* wl_out, int32_t* wi_out) {
  const double nan = __builtin_nan("");
  for (int j = 0; j < nk; ++j) {
    const size_t row = (size_t)g * K + k0 + j;
    if (fl_out) for (int l = threadIdx.x; l < E; l += PF_THREADS) fl_out[row * E + l] = nan;
    if (threadIdx.x == 0) { wl_out[row] = nan; wi_out[row] = -1; }
  }
}

// The LDS image of a screen workgroup (dcn1_lds_bytes); the adjoint's arrays follow Z
struct Dcn1Image {
  double* F;      // [nnz1] factor of Bbus[r, r]
  double* rhs;    // [d1] right-hand side / theta_r of the base case
  double* th;     // [N] base theta by bus
  double* lb;     // [E] b_l
  double* lF;     // [E] base flow
  int2* ends;     // [E] B' positions of the line's ends, -1 at the slack
  double* Z;      // [d1][ld] right-hand sides / z_k of the chunk's outages
};

__device__ __forceinline__ Dcn1Image dcn1_image(const int32_t* topo, double* lds) {
  const int N = topo[FH_N], E = topo[FH_E], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  Dcn1Image m;
  m.F = lds;
  m.rhs = m.F + nnz1;
  m.th = m.rhs + d1;
  m.lb = m.th + N;
  m.lF = m.lb + E;
  m.ends = reinterpret_cast<int2*>(m.lF + E);
  m.Z = m.lF + 2 * E;
  return m;
}

// The base case of one grid, as gns_dc_kernel solves it, into the image: the factor, theta, and per line b_l, the base flow and the
// ends.  False (for the whole wave) when the base solve fails; the line arrays are not filled then.
__device__ __forceinline__ bool dcn1_base_case(const int32_t* topo, const float* bus, const float* line, const float* gen,
                                               const Dcn1Image& m, const int lane) {
  const int N = topo[FH_N], E = topo[FH_E], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[FH_Y_PTR];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int32_t* bslot = topo + topo[FH_BSLOT];
  const int2* ops_s = reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]);
  double* F = m.F;
  double* rhs = m.rhs;
  double* th = m.th;

  for (int s = lane; s < nnz1; s += PF_THREADS) F[s] = 0.0;
  __syncthreads();
  dc_matrix(N, y_ptr, st_ptr, st, bslot, line, F, lane);
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_F1], topo + topo[FH_STEP_F1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_F1]), F, lane);
  bool bad = pf_bad_pivot(d1, topo + topo[FH_PIVOT1], F, lane);
  for (int i = lane; i < N; i += PF_THREADS)
    if (p_idx[i] >= 0) rhs[p_idx[i]] = dc_injection(i, y_diag, st_ptr, st, gen_ptr, gen_idx, bus, line, gen);
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, F, lane);
  for (int i = lane; i < N; i += PF_THREADS) {
    const double x = p_idx[i] >= 0 ? rhs[p_idx[i]] : 0.0;
    th[i] = x;
    bad |= !pf_finite(x);
  }
  __syncthreads();
  if (__ballot(bad)) return false;
  for (int e = lane; e < E; e += PF_THREADS) {
    int f, t;
    const bool ok = pf_line_ends(line, e, N, f, t);
    const double b = dc_line_b(line, e);
    m.lb[e] = b;
    m.lF[e] = ok ? b * (th[f] - th[t]) + (0.0 - b * (double)line[e * 7 + 6]) : __builtin_nan("");
    m.ends[e] = ok ? make_int2(p_idx[f], p_idx[t]) : make_int2(-1, -1);
  }
  __syncthreads();
  return true;
}

// Lane j's own solve for line e: z = A^-1 m_e on the base factor into column zc of Z (m_e = 0 for a line from a bus to itself, which
// changes nothing).  Returns whether every entry of z is finite; en gets the B' positions of the line's ends.
__device__ __forceinline__ bool dcn1_lane_z(const int32_t* topo, const Dcn1Image& m, const int e, double* zc, const int ld, int2& en) {
  const int d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  for (int s = 0; s < d1; ++s) zc[s * ld] = 0.0;
  en = m.ends[e];
  if (en.x != en.y) {                                   // (a line from a bus to itself changes nothing: a = 0)
    if (en.x >= 0) zc[en.x * ld] = 1.0;
    if (en.y >= 0) zc[en.y * ld] = -1.0;
  }
  dcn1_lane_solve(topo[FH_NOPS_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), m.F, nnz1, zc, ld);
  bool fin = true;
  for (int s = 0; s < d1; ++s) fin &= pf_finite(zc[s * ld]);
  return fin;
}

// Lane j's own outage (line e, not islanding): z on the base factor into column zc of Z, then den = 1 - b_k (z_f - z_t) and
// alpha = F_k / den.  Returns the line, or -1 for a row that is not solved: a non-finite z, denominator or alpha.
__device__ __forceinline__ int dcn1_lane_outage(const int32_t* topo, const Dcn1Image& m, const int e, double* zc, const int ld,
                                                double& den, double& alpha) {
  int2 en;
  const bool fin = dcn1_lane_z(topo, m, e, zc, ld, en);
  const double d = (en.x >= 0 ? zc[en.x * ld] : 0.0) - (en.y >= 0 ? zc[en.y * ld] : 0.0);
  den = 1.0 - m.lb[e] * d;
  alpha = m.lF[e] / den;
  return fin && pf_finite(den) && den != 0.0 && pf_finite(alpha) ? e : -1;
}

// Post-outage flow of line l for the outage whose z is column j of Z: F_l + b_l (z_f - z_t) alpha (the caller puts 0 at l = k)
__device__ __forceinline__ double dcn1_flow(const Dcn1Image& m, const int l, const int ld, const int j, const double alpha) {
  const int2 en = m.ends[l];
  const double zf = en.x >= 0 ? m.Z[en.x * ld + j] : 0.0, zt = en.y >= 0 ? m.Z[en.y * ld + j] : 0.0;
  return m.lF[l] + m.lb[l] * (zf - zt) * alpha;
}

// ---- what the adjoints of the screens share (gns_dcn1_adjoint, gns_dcn2_adjoint, gns_dcg1_adjoint)

// What grad_worst_loading gw adds to a row's gradient at the line the forward found worst, fw its post-outage flow and rt its
// rating: d|F'_w| / rating_w is the sign of the flow over the rating
__device__ __forceinline__ double dcn1_worst_term(const double gw, const double fw, const double rt) {
  return gw * (fw > 0.0 ? 1.0 : fw < 0.0 ? -1.0 : 0.0) / rt;
}

// Whether one of the rows row0 + j of the incoming gradients, j a set bit of rows, holds a value that is not exactly zero (NaN
// counts).  The whole wave scans each row with a line per lane; the answer is the same in every lane.
__device__ __forceinline__ bool dcn1_rows_nonzero(unsigned long long rows, const size_t row0, const int E, const double* gfl,
                                                  const double* gwl) {
  bool nz = false;
  for (; rows; rows &= rows - 1) {
    const size_t row = row0 + (__ffsll((long long)rows) - 1);
    if (gwl && threadIdx.x == 0) nz |= gwl[row] != 0.0;
    if (gfl) for (int l = threadIdx.x; l < E; l += PF_THREADS) nz |= gfl[row * E + l] != 0.0;
  }
  return __ballot(nz) != 0;
}

// The status of a chunk's partial: its sums are valid; the grid's gradient is NaN; the grid is not solved and the chunk's incoming
// gradients are zero (the sums are zeros; when every chunk says so the grid gets zero rows, whatever its inputs hold)
constexpr double DCN1_PART_OK = 0.0, DCN1_PART_NAN = 1.0, DCN1_PART_UNSOLVED_ZERO = 2.0;

// The partial of a chunk that adds nothing: zeros and the status
__device__ __forceinline__ void dcn1_partial_none(double* part, const int n, const double status) {
  for (int q = threadIdx.x; q < n - 1; q += PF_THREADS) part[q] = 0.0;
  if (threadIdx.x == 0) part[n - 1] = status;
}

// The status of a grid from its chunks' partials, the same in every lane: DCN1_PART_OK, DCN1_PART_NAN (a chunk says NaN) or
// DCN1_PART_UNSOLVED_ZERO (every chunk says so)
__device__ __forceinline__ double dcn1_reduce_status(const double* part, const int nchunks, const int np) {
  bool bad = false, solved = false;
  for (int c = threadIdx.x; c < nchunks; c += PF_THREADS) {
    const double status = part[(size_t)c * np + np - 1];
    bad |= status != DCN1_PART_OK && status != DCN1_PART_UNSOLVED_ZERO;
    solved |= status != DCN1_PART_UNSOLVED_ZERO;
  }
  return __ballot(bad) ? DCN1_PART_NAN : __ballot(solved) ? DCN1_PART_OK : DCN1_PART_UNSOLVED_ZERO;
}

// The bus and line rows of grid g from its partials: the chunks summed in order, the contract applied, every element written
__device__ __forceinline__ void dcn1_reduce_buses_lines(const int32_t* topo, const float* line, const int nchunks, const double* part,
                                                        const int g, float* gb_out, float* gl_out) {
  const int lane = threadIdx.x;
  const int N = topo[FH_N], E = topo[FH_E];
  const int np = (int)dcn1_adjoint_partial(topo);
  // (0.0 - x rather than -x: an exact zero stays +0)
  if (gb_out)
    for (int i = lane; i < N; i += PF_THREADS) {
      double dp = 0.0;
      for (int c = 0; c < nchunks; ++c) dp += part[(size_t)c * np + i];
      float* row = gb_out + ((size_t)g * N + i) * 6;
      const float d = (float)(0.0 - dp);
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = d;                              // Pd
      row[3] = 0.0f;
      row[4] = d;                              // Gs
      row[5] = 0.0f;
    }
  if (gl_out)
    for (int e = lane; e < E; e += PF_THREADS) {
      float* row = gl_out + ((size_t)g * E + e) * 7;
      int f, t;
      if (!pf_line_ends(line, e, N, f, t)) {
        for (int c = 0; c < 7; ++c) row[c] = __builtin_nanf("");
        continue;
      }
      double d_b = 0.0, sw = 0.0;
      for (int c = 0; c < nchunks; ++c) {
        d_b += part[(size_t)c * np + N + e];
        sw += part[(size_t)c * np + N + E + e];
      }
      const double x = line[e * 7 + 3], tau = line[e * 7 + 5];
      const double b = dc_line_b(line, e);
      row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f;
      row[3] = (float)(0.0 - d_b * b / x);             // x: db/dx = -b / x
      row[4] = 0.0f;
      row[5] = (float)(0.0 - d_b * b / tau);           // tau: db/dtau = -b / tau
      row[6] = (float)(0.0 - b * sw);                  // shift
    }
}

// dl/dP at bus b: the chunks' partials summed in order
__device__ __forceinline__ double dcn1_reduce_dp(const double* part, const int nchunks, const int np, const int b) {
  double dp = 0.0;
  for (int c = 0; c < nchunks; ++c) dp += part[(size_t)c * np + b];
  return dp;
}

// A wave per grid: the chunks' partials summed in order, the contract applied, every element of the three gradient rows written
__global__ __launch_bounds__(PF_THREADS) void gns_dcn1_adjoint_reduce_kernel(const int32_t* __restrict__ topo,
                                                                             const float* __restrict__ lines, const int nchunks,
                                                                             const double* __restrict__ partials,
                                                                             float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                             float* __restrict__ gg_out) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int np = (int)dcn1_adjoint_partial(topo);
  const double* part = partials + (size_t)g * nchunks * np;

  const double status = dcn1_reduce_status(part, nchunks, np);
  if (status == DCN1_PART_NAN) { pf_adjoint_fill(g, N, E, Gn, __builtin_nanf(""), gb_out, gl_out, gg_out); return; }
  if (status == DCN1_PART_UNSOLVED_ZERO) { pf_adjoint_fill(g, N, E, Gn, 0.0f, gb_out, gl_out, gg_out); return; }

  dcn1_reduce_buses_lines(topo, lines + (size_t)g * E * 7, nchunks, part, g, gb_out, gl_out);
  if (gg_out)
    for (int q = lane; q < Gn; q += PF_THREADS) {      // a lane per generator, in the blob's by-bus order
      float* row = gg_out + ((size_t)g * Gn + gen_idx[q]) * 7;
      for (int c = 0; c < 6; ++c) row[c] = 0.0f;
      row[6] = (float)dcn1_reduce_dp(part, nchunks, np, pf_slot_bus(gen_ptr, N, q));   // Pg
    }
}

}  // namespace
