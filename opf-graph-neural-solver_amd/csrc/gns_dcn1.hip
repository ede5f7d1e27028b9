// Batched DC N-1 contingency screening (include/gns_powerflow.h, "DC contingency screening") on the fast-decoupled blob.  A
// single-line outage is a rank-1 change of Bbus[r, r], so the post-outage flows of outage k come from one more solve on the base
// factor: z_k = Bbus[r, r]^-1 (e_f - e_t)_r, the line-outage distribution factors.
//
// Mapping: one wave per (grid, chunk of W outages).  The wave builds and factors Bbus[r, r] once and solves the base case as
// gns_dc_kernel does, on 64 lanes with a barrier per step.  Then lane j owns outage j of the chunk: it runs the whole B' solve program
// on its own right-hand side, with no barrier, against the shared read-only factor.  The right-hand sides sit in LDS as
// Z[slot][W + 1]: the lanes of one operation read consecutive doubles (no bank conflict), and the padding column spreads the
// transposed reads of the flow pass (one outage, a line per lane) over the banks.  The flow pass walks the chunk's outages in order
// with a line per lane, so the stores of line_flow are contiguous, and reduces the worst loading over the wave with a comparison
// that does not depend on the order (the largest value, the lowest line among equals).  No atomics, no workspace.
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

__global__ __launch_bounds__(PF_THREADS) void gns_dcn1_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                              const float* __restrict__ lines, const float* __restrict__ gens,
                                                              const int32_t* __restrict__ outages, const int K,
                                                              const uint8_t* __restrict__ islanding,
                                                              const double* __restrict__ rating, const int rating_per_grid,
                                                              const int W, const int nchunks, double* __restrict__ fl_out,
                                                              double* __restrict__ wl_out, int32_t* __restrict__ wi_out,
                                                              uint8_t* __restrict__ conv_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, K - k0);
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[FH_Y_PTR];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int32_t* bslot = topo + topo[FH_BSLOT];
  const int2* ops_s = reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]);

  double* F = lds;                       // [nnz1] factor of Bbus[r, r], then [d1] right-hand side / theta_r of the base case
  double* rhs = F + nnz1;
  double* th = rhs + d1;                 // [N] base theta by bus
  double* lb = th + N;                   // [E] b_l
  double* lF = lb + E;                   // [E] base flow
  int2* ends = reinterpret_cast<int2*>(lF + E);   // [E] B' positions of the line's ends, -1 at the slack
  const int ld = W + 1;
  double* Z = lF + 2 * E;                // [d1][ld] right-hand sides / z_k of the chunk's outages
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;

  // the base case, as gns_dc_kernel solves it
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
  if (__ballot(bad)) {
    dcn1_rows_not_solved(g, K, E, k0, nk, fl_out, wl_out, wi_out);
    if (k0 == 0 && lane == 0) conv_out[g] = 0;
    return;
  }
  for (int e = lane; e < E; e += PF_THREADS) {
    int f, t;
    const bool ok = dc_line_ends(line, e, N, f, t);
    const double b = dc_line_b(line, e);
    lb[e] = b;
    lF[e] = ok ? b * (th[f] - th[t]) + (0.0 - b * (double)line[e * 7 + 6]) : __builtin_nan("");
    ends[e] = ok ? make_int2(p_idx[f], p_idx[t]) : make_int2(-1, -1);
  }
  __syncthreads();

  // lane j: z of outage k0 + j on the base factor, then alpha = F_k / (1 - b_k (z_f - z_t)).  e_k stays -1 for a row that is not
  // solved: an islanding outage, a line index outside the grid, a non-finite z, denominator or alpha.
  int e_k = -1;
  double alpha = __builtin_nan("");
  if (lane < nk) {
    const int e = outages[k0 + lane];
    if (e >= 0 && e < E && !islanding[k0 + lane]) {
      double* zc = Z + lane;
      for (int s = 0; s < d1; ++s) zc[s * ld] = 0.0;
      const int2 en = ends[e];
      if (en.x != en.y) {                                   // (a line from a bus to itself changes nothing: a = 0)
        if (en.x >= 0) zc[en.x * ld] = 1.0;
        if (en.y >= 0) zc[en.y * ld] = -1.0;
      }
      dcn1_lane_solve(topo[FH_NOPS_S1], ops_s, F, nnz1, zc, ld);
      bool fin = true;
      for (int s = 0; s < d1; ++s) fin &= pf_finite(zc[s * ld]);
      const double d = (en.x >= 0 ? zc[en.x * ld] : 0.0) - (en.y >= 0 ? zc[en.y * ld] : 0.0);
      const double den = 1.0 - lb[e] * d;
      const double a = lF[e] / den;
      if (fin && pf_finite(den) && den != 0.0 && pf_finite(a)) { alpha = a; e_k = e; }
    }
  }
  __syncthreads();

  // the chunk's outages in order, a line per lane: F'_l = F_l + b_l (z_f - z_t) alpha, 0 at the outaged line
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  for (int j = 0; j < nk; ++j) {
    const double al = __shfl(alpha, j);
    const int ek = __shfl(e_k, j);
    if (ek < 0) { dcn1_rows_not_solved(g, K, E, k0 + j, 1, fl_out, wl_out, wi_out); continue; }
    const size_t row = (size_t)g * K + k0 + j;
    double best = -1.0;
    int bi = INT32_MAX;
    for (int l = lane; l < E; l += PF_THREADS) {
      const int2 en = ends[l];
      const double zf = en.x >= 0 ? Z[en.x * ld + j] : 0.0, zt = en.y >= 0 ? Z[en.y * ld + j] : 0.0;
      const double fl = l == ek ? 0.0 : lF[l] + lb[l] * (zf - zt) * al;
      if (fl_out) fl_out[row * E + l] = fl;
      const double v = rt ? fabs(fl) / rt[l] : fabs(fl);
      if (dcn1_worse(v, l, best, bi)) { best = v; bi = l; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (dcn1_worse(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { wl_out[row] = best; wi_out[row] = bi; }
  }
  if (k0 == 0 && lane == 0) conv_out[g] = 1;
}

// ---- host

// One blob and one outage list: GNS_EINVAL unless it is an FD blob of cfg's shape and every outage is a line of it; lanes and lds are
// the chunk width and the LDS image of the launch
int dcn1_check(const gns_pf_config* cfg, const void* topo_host, const int32_t* outages_host, int32_t n_outage, int* lanes,
               int64_t* lds) {
  if (!cfg || !topo_host || !outages_host || n_outage <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  for (int32_t k = 0; k < n_outage; ++k)
    if (outages_host[k] < 0 || outages_host[k] >= h[FH_E]) return GNS_EINVAL;
  *lanes = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  *lds = dcn1_lds_bytes(h, *lanes);
  return GNS_OK;
}

}  // namespace

extern "C" int gns_dcn1_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  if (!topo_host || !bytes) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  const int w = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  *bytes = dcn1_lds_bytes(h, w);
  if (lanes) *lanes = w;
  return GNS_OK;
}

extern "C" int gns_dcn1_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_outage <= 0) return GNS_EINVAL;
  if (!pf_header_ok<DcBlobKind>(cfg, static_cast<const int32_t*>(topo_host))) return GNS_EINVAL;
  *bytes = 0;
  return GNS_OK;
}

extern "C" int gns_dcn1_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid,
                               double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || !outages_dev || !islanding || !worst_loading || !worst_line ||
      !converged || (rating_per_grid != 0 && rating_per_grid != 1))
    return GNS_EINVAL;
  int lanes = 0;
  int64_t lds = 0;
  const int rc = dcn1_check(cfg, topo_host, outages_host, n_outage, &lanes, &lds);
  if (rc != GNS_OK) return rc;
  const int64_t nchunks = ((int64_t)n_outage + lanes - 1) / lanes;
  if (Bt > 0x7FFFFFFF / nchunks) return GNS_EINVAL;           // a workgroup per (grid, chunk) in one launch
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  return pf_launch<gns_dcn1_kernel>(Bt * nchunks, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators,
                                    outages_dev, (int)n_outage, islanding, rating, (int)rating_per_grid, lanes, (int)nchunks,
                                    line_flow, worst_loading, worst_line, converged);
}
