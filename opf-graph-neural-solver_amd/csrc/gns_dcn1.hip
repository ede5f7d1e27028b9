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
//
// The adjoint (gns_dcn1_adjoint) has the same mapping on a wider image: the prologue and lane j's z_k are the screen's own code, so
// the row's state is the forward's bit for bit; lane j then builds the adjoint right-hand side q_k of its outage into a second
// [slot][W + 1] array, solves it on the base factor and corrects it to lambda_k (Sherman-Morrison); a last pass with a line per lane
// and a bus per lane sums the chunk's outages in order into the chunk's partial of the workspace, and a second kernel with a wave
// per grid sums the chunks in order, applies the contract and writes the fp32 gradient rows.  No atomics anywhere.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"

namespace {

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
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;

  if (!dcn1_base_case(topo, buses + (size_t)g * N * 6, lines + (size_t)g * E * 7, gens + (size_t)g * Gn * 7, m, lane)) {
    dcn1_rows_not_solved(g, K, E, k0, nk, fl_out, wl_out, wi_out);
    if (k0 == 0 && lane == 0) conv_out[g] = 0;
    return;
  }

  // lane j: z of outage k0 + j on the base factor, then alpha = F_k / (1 - b_k (z_f - z_t)).  e_k stays -1 for a row that is not
  // solved: an islanding outage, a line index outside the grid, a non-finite z, denominator or alpha.
  int e_k = -1;
  double alpha = __builtin_nan("");
  if (lane < nk) {
    const int e = outages[k0 + lane];
    if (e >= 0 && e < E && !islanding[k0 + lane]) {
      double den, a;
      e_k = dcn1_lane_outage(topo, m, e, m.Z + lane, ld, den, a);
      if (e_k >= 0) alpha = a;
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
      const double fl = l == ek ? 0.0 : dcn1_flow(m, l, ld, j, al);
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

// ---- the adjoint (gns_dcn1_adjoint; include/gns_powerflow.h, "DC contingency screening", gradients)

constexpr int DCN1_GRAD_PREFETCH = 8;   // incoming gradients of its row a lane fetches ahead of adding them to its right-hand side

__global__ __launch_bounds__(PF_THREADS) void gns_dcn1_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const float* __restrict__ gens,
                                                                      const int32_t* __restrict__ outages, const int K,
                                                                      const uint8_t* __restrict__ islanding,
                                                                      const double* __restrict__ rating, const int rating_per_grid,
                                                                      const int32_t* __restrict__ wi_in,
                                                                      const uint8_t* __restrict__ conv_in,
                                                                      const double* __restrict__ gfl, const double* __restrict__ gwl,
                                                                      const int W, const int nchunks, double* __restrict__ partials) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, K - k0);
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;
  double* U = m.Z + d1 * ld;                         // [d1][ld] adjoint right-hand sides q_k, then u_k, then lambda_k
  double* o_alpha = U + d1 * ld;                     // [W] alpha_k
  double* o_gw = o_alpha + W;                        // [W] what grad_worst_loading adds to the row's gradient at its worst line
  int2* o_line = reinterpret_cast<int2*>(o_gw + W);  // [W] (k, worst line or -1), k = -1 for a row that contributes nothing
  const int np = (int)dcn1_adjoint_partial(topo);
  double* part = partials + (size_t)blockIdx.x * np; // [N] dl/dP, [E] dl/db, [E] sum of w, the status
  const float* line = lines + (size_t)g * E * 7;
  const size_t row0 = (size_t)g * K + k0;

  // a grid that is not solved: nothing to add; its gradient is NaN unless every incoming gradient of the chunk is zero
  if (!conv_in[g] || !dcn1_base_case(topo, buses + (size_t)g * N * 6, line, gens + (size_t)g * Gn * 7, m, lane)) {
    const bool nz = dcn1_rows_nonzero(__ballot(lane < nk), row0, E, gfl, gwl);
    dcn1_partial_none(part, np, nz ? DCN1_PART_NAN : DCN1_PART_UNSOLVED_ZERO);
    return;
  }

  // lane j: the forward's state of outage k0 + j, then its adjoint right-hand side q = sum_{l != k} G_l b_l m_l, u = A^-1 q on the
  // base factor and lambda = u + z b_k (m_k^T u) / den
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  bool bad = false, unsolved = false;
  int e_k = -1, wl = -1;
  double alpha = 0.0, gterm = 0.0;
  if (lane < nk) {
    const size_t row = row0 + lane;
    const int e = outages[k0 + lane];
    double den = 0.0;
    if (e >= 0 && e < E && !islanding[k0 + lane]) e_k = dcn1_lane_outage(topo, m, e, m.Z + lane, ld, den, alpha);
    unsolved = e_k < 0;                               // a row the forward left NaN / -1: skipped, never multiplied by zero
    if (!unsolved) {
      double* uc = U + lane;
      for (int s = 0; s < d1; ++s) uc[s * ld] = 0.0;
      const double gw = gwl ? gwl[row] : 0.0;
      const int w = wi_in[row];
      if (gw != 0.0 && w >= 0 && w < E && w != e_k) {  // d|F'_w| / rating_w: the sign of the flow the forward found worst
        gterm = dcn1_worst_term(gw, dcn1_flow(m, w, ld, lane, alpha), rt ? rt[w] : 1.0);
        wl = w;
      }
      bool has = false;
      const double* grow = gfl ? gfl + row * E : nullptr;
      for (int l0 = grow ? 0 : max(wl, 0); l0 < (grow ? E : wl + 1); l0 += DCN1_GRAD_PREFETCH) {
        double gv[DCN1_GRAD_PREFETCH];
#pragma unroll
        for (int u = 0; u < DCN1_GRAD_PREFETCH; ++u) gv[u] = grow ? grow[min(l0 + u, E - 1)] : 0.0;
#pragma unroll
        for (int u = 0; u < DCN1_GRAD_PREFETCH; ++u) {
          const int l = l0 + u;
          if (l >= E || l == e_k) continue;
          const double G = l == wl ? gv[u] + gterm : gv[u];
          if (G == 0.0) continue;
          has = true;
          const int2 en = m.ends[l];
          if (en.x == en.y) continue;                   // m_l = 0
          const double x = G * m.lb[l];
          if (en.x >= 0) uc[en.x * ld] += x;
          if (en.y >= 0) uc[en.y * ld] -= x;
        }
      }
      if (!has) {
        e_k = -1;                                       // a zero incoming gradient: the row adds nothing
      } else {
        dcn1_lane_solve(topo[FH_NOPS_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), m.F, nnz1, uc, ld);
        const int2 en = m.ends[e_k];
        const double mu = (en.x >= 0 ? uc[en.x * ld] : 0.0) - (en.y >= 0 ? uc[en.y * ld] : 0.0);
        const double c = m.lb[e_k] * mu / den;
        const double* zc = m.Z + lane;
        bool fin = true;
        for (int s = 0; s < d1; ++s) {
          const double x = uc[s * ld] + zc[s * ld] * c;
          uc[s * ld] = x;
          fin &= pf_finite(x);
        }
        bad = !fin;
      }
    }
  }
  if (lane < W) {
    o_alpha[lane] = alpha;
    o_gw[lane] = gterm;
    o_line[lane] = make_int2(e_k, wl);
  }
  __syncthreads();
  // an unsolved row with a non-zero incoming gradient, or a lambda that is not finite: the grid's gradient is NaN
  if (__ballot(bad) || dcn1_rows_nonzero(__ballot(unsolved), row0, E, gfl, gwl)) { dcn1_partial_none(part, np, DCN1_PART_NAN); return; }

  // the chunk's outages in order, a line per lane: w = G - (lambda_f - lambda_t); dl/db += w (theta'_f - theta'_t - shift) with
  // theta' = theta + alpha z; the sum of w gives dl/dshift = -b sum w.  The outaged line's own entry is skipped.
  for (int l = lane; l < E; l += PF_THREADS) {
    const int2 en = m.ends[l];
    const double thf = en.x >= 0 ? m.rhs[en.x] : 0.0, tht = en.y >= 0 ? m.rhs[en.y] : 0.0;
    const double sh = (double)line[l * 7 + 6];
    double d_b = 0.0, sw = 0.0;
    for (int j = 0; j < nk; ++j) {
      const int2 o = o_line[j];
      if (o.x < 0 || o.x == l) continue;
      const double g0 = gfl ? gfl[(row0 + j) * E + l] : 0.0;
      const double G = l == o.y ? g0 + o_gw[j] : g0;
      const double lf = en.x >= 0 ? U[en.x * ld + j] : 0.0, lt = en.y >= 0 ? U[en.y * ld + j] : 0.0;
      const double zf = en.x >= 0 ? m.Z[en.x * ld + j] : 0.0, zt = en.y >= 0 ? m.Z[en.y * ld + j] : 0.0;
      const double w = G - (lf - lt);
      const double al = o_alpha[j];
      d_b += w * (((thf + al * zf) - (tht + al * zt)) - sh);
      sw += w;
    }
    part[N + l] = d_b;
    part[N + E + l] = sw;
  }
  // a bus per lane: dl/dP_i = sum_k lambda_k[i], 0 at the slack
  for (int i = lane; i < N; i += PF_THREADS) {
    const int p = p_idx[i];
    double dp = 0.0;
    if (p >= 0)
      for (int j = 0; j < nk; ++j)
        if (o_line[j].x >= 0) dp += U[p * ld + j];
    part[i] = dp;
  }
  if (lane == 0) part[np - 1] = DCN1_PART_OK;
}

// ---- host

// One blob and one outage list: GNS_EINVAL unless it is an FD blob of cfg's shape and every outage is a line of it; lanes and lds are
// the chunk width and the LDS image of the launch
int dcn1_check(const gns_pf_config* cfg, const void* topo_host, const int32_t* outages_host, int32_t n_outage, int* lanes,
               int64_t* lds) {
  if (!cfg || !topo_host || !outages_host || n_outage <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (!pf_lines_ok(h, outages_host, n_outage)) return GNS_EINVAL;
  *lanes = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  *lds = dcn1_lds_bytes(h, *lanes);
  return GNS_OK;
}

// Workspace of the adjoint: a partial per (grid, chunk), rounded up to 256 bytes
size_t dcn1_adjoint_ws_bytes(const int32_t* h, int64_t Bt, int64_t nchunks) {
  return ((size_t)Bt * nchunks * dcn1_adjoint_partial(h) * sizeof(double) + 255) & ~(size_t)255;
}

}  // namespace

extern "C" int gns_dcn1_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return pf_fd_lds_query(topo_host, bytes, lanes, dcn1_lanes, dcn1_lds_bytes);
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
  int64_t nchunks = 0;
  if (!pf_chunks(n_outage, lanes, Bt, &nchunks)) return GNS_EINVAL;
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  return pf_launch<gns_dcn1_kernel>(Bt * nchunks, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators,
                                    outages_dev, (int)n_outage, islanding, rating, (int)rating_per_grid, lanes, (int)nchunks,
                                    line_flow, worst_loading, worst_line, converged);
}

extern "C" int gns_dcn1_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return pf_fd_lds_query(topo_host, bytes, lanes, dcn1_adjoint_lanes, dcn1_adjoint_lds_bytes);
}

extern "C" int gns_dcn1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage,
                                                size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_outage <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  const int w = dcn1_adjoint_lanes(h, GNS_PF_LDS_MAX_BYTES);
  int64_t nchunks = 0;
  if (!pf_chunks(n_outage, w, Bt, &nchunks)) return GNS_EINVAL;
  if (dcn1_adjoint_lds_bytes(h, w) > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  *bytes = dcn1_adjoint_ws_bytes(h, Bt, nchunks);
  return GNS_OK;
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.
extern "C" int gns_dcn1_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid,
                                const int32_t* worst_line, const uint8_t* converged,
                                const double* grad_line_flow, const double* grad_worst_loading,
                                float* grad_buses, float* grad_lines, float* grad_generators,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || !outages_dev || !islanding || !worst_line || !converged ||
      (rating_per_grid != 0 && rating_per_grid != 1))
    return GNS_EINVAL;
  int lanes = 0;
  int64_t lds = 0;
  const int rc = dcn1_check(cfg, topo_host, outages_host, n_outage, &lanes, &lds);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  lanes = dcn1_adjoint_lanes(h, GNS_PF_LDS_MAX_BYTES);
  lds = dcn1_adjoint_lds_bytes(h, lanes);
  int64_t nchunks = 0;
  if (!pf_chunks(n_outage, lanes, Bt, &nchunks)) return GNS_EINVAL;
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  if (!workspace) return GNS_EINVAL;
  if (workspace_bytes < dcn1_adjoint_ws_bytes(h, Bt, nchunks)) return GNS_ESIZE;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  double* partials = static_cast<double*>(workspace);
  const int rc1 = pf_launch<gns_dcn1_adjoint_kernel>(Bt * nchunks, lds, stream, topo, buses, lines, generators, outages_dev,
                                                     (int)n_outage, islanding, rating, (int)rating_per_grid, worst_line, converged,
                                                     grad_line_flow, grad_worst_loading, lanes, (int)nchunks, partials);
  if (rc1 != GNS_OK) return rc1;
  return pf_launch<gns_dcn1_adjoint_reduce_kernel>(Bt, 0, stream, topo, lines, (int)nchunks, (const double*)partials, grad_buses,
                                                   grad_lines, grad_generators);
}
