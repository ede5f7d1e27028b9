// Batched DC generator contingency screening (include/gns_powerflow.h, "DC generator contingency screening") on the fast-decoupled
// blob: the post-outage DC flows of a list of rows (generator g out, with line k out as well or no line).  A generator outage changes
// the injections alone, so it is one more solve u_g on the base factor; the line on top of it is the rank-1 update of the N-1
// screen, from the single-line solve z_k that screen makes.  Per grid that is one solve per distinct generator and per distinct
// line of the list, not one factorisation per row.
//
// The kernels, the workspace and the host code after the checks are gns_dcn2_device.h's, shared with gns_dcn2.hip: the factor kernel
// over the list's lines followed by its generators (H_k for a line, D_g for a generator), then the row kernel over the rows; the
// adjoint (gns_dcg1_adjoint) runs the factor kernel again, the adjoint's row, gather and solve kernels, and its own reduce kernel
// below.  Here: the row as a row model (Dcg1Rows: den and alpha of the N-1 screen on top of D_g, v = ga / den), the list check, the
// reduce kernel with the generators' own terms and the entry points.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn2_device.h"

namespace {

constexpr int DCG1_GEN = 3;   // doubles the reduce kernel keeps per listed generator: Pg_g / W_g (0: nothing shared), s_g, c_g^T y_g

// The lists of a call: the lines and the generators as the factor kernel's candidates (the lines first), and per row the generator's
// and the line's position (-1: no line)
struct Dcg1Rows {
  static constexpr int NOUT = 1;
  static constexpr int REC = 4;   // doubles of a (grid, row) record: alpha, v, the worst-line term, (contributes, worst line)
  const int32_t* line_list;
  int n_line, n_gen;
  const int32_t* cols;

  __device__ __forceinline__ int n_cand() const { return n_line + n_gen; }

  struct Row : DcrowOut<1> {
    using Sums = DcrowSums<1>;
    int cg, ck;
    const double* Dg;
    const double* Hk;
    double den, alpha;

    __device__ __forceinline__ bool place(const Dcg1Rows& s, const int p) {
      cg = s.cols[2 * (size_t)p];
      ck = s.cols[2 * (size_t)p + 1];
      return cg >= 0 && cg < s.n_gen && ck >= -1 && ck < s.n_line;
    }
    // the same scalars on every lane: the flow of line k with the generator out, then the N-1 screen's den and alpha
    __device__ __forceinline__ bool solve(const Dcg1Rows& s, const DcrowBase& g) {
      e[0] = -1;
      den = 1.0;
      alpha = 0.0;
      Dg = g.H + (size_t)(s.n_line + cg) * g.E;
      Hk = g.H;
      if (g.fin[s.n_line + cg] == 0.0) return false;
      if (ck < 0) return true;
      const int ek = s.line_list[ck];
      e[0] = ek;
      Hk += (size_t)ck * g.E;
      const double fgk = g.F[ek] + g.b[ek] * Dg[ek];
      den = 1.0 - g.b[ek] * Hk[ek];
      alpha = fgk / den;
      return g.fin[ck] != 0.0 && pf_finite(den) && den != 0.0 && pf_finite(alpha);
    }
    __device__ __forceinline__ double flow(const DcrowBase& g, const int l) const {
      const double fg = g.F[l] + g.b[l] * Dg[l];
      return e[0] < 0 ? fg : fg + (g.b[l] * Hk[l]) * alpha;
    }
    // ga = sum_l G_l b_l H_k[l]; nothing without a line
    __device__ __forceinline__ Sums ga_term(const DcrowBase&, const double x, const int l) const { return {{e[0] >= 0 ? x * Hk[l] : 0.0}}; }
    // v = ga / den: dl/dFg at the outaged line
    __device__ __forceinline__ void close(const Sums& ga) { v[0] = e[0] >= 0 ? ga.s[0] / den : 0.0; }
    __device__ __forceinline__ void record(double* rec) const { rec[0] = alpha; rec[1] = v[0]; }
  };

  // candidate c is a line (a position of the rows' second column) or, from n_line on, a generator (of the first)
  __device__ __forceinline__ bool holds(const int p, const int c) const {
    return c < n_line ? cols[2 * (size_t)p + 1] == c : cols[2 * (size_t)p] == c - n_line;
  }
  // T_k takes G alpha, S_g takes G; the outaged line's own entry: v alpha (the derivative of den) for T_k, v for S_g
  __device__ __forceinline__ DcrowHeld<1> held(const int p, const int c, const double* rec) const {
    const int ck = cols[2 * (size_t)p + 1];
    DcrowHeld<1> h;
    h.e[0] = ck >= 0 ? line_list[ck] : -1;
    h.v[0] = rec[1];
    h.a_c = c < n_line ? rec[0] : 1.0;
    return h;
  }
};

// One blob, the two candidate lists and one row list: GNS_EINVAL unless it is an FD blob of cfg's shape, the lines and the generators
// are indices of it, ascending and distinct (the line list may be empty), and every row holds a position into the generators and a
// position into the lines or -1
int dcg1_check(const gns_pf_config* cfg, const void* topo_host, const int32_t* line_host, int32_t n_line, const int32_t* gen_host,
               int32_t n_gen, const int32_t* row_cols_host, int32_t n_row) {
  if (!cfg || !topo_host || n_line < 0 || (n_line > 0 && !line_host) || !gen_host || n_gen <= 0 || !row_cols_host || n_row <= 0)
    return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (n_line > h[FH_E] || n_gen > h[FH_GN]) return GNS_EINVAL;
  if (!dcg1_list_ok(line_host, n_line, h[FH_E]) || !dcg1_list_ok(gen_host, n_gen, h[FH_GN])) return GNS_EINVAL;
  for (int64_t p = 0; p < n_row; ++p) {
    const int32_t a = row_cols_host[2 * p], b = row_cols_host[2 * p + 1];
    if (a < 0 || a >= n_gen || b < -1 || b >= n_line) return GNS_EINVAL;
  }
  return GNS_OK;
}

// The adjoint's own blocks of the workspace after the shared ones (DcrowAdjointWorkspace::own): the generators' y by bus
// [Bt][n_gen][N], which the solve kernel writes, then three doubles per listed generator [Bt][n_gen][3]
int64_t dcg1_adjoint_own(int64_t N, int64_t n_gen) { return n_gen * N + n_gen * DCG1_GEN; }

// A wave per grid: gns_dcn1_adjoint_reduce_kernel's sums and contract, with the generators' own terms.  y_g by bus is the solve
// kernel's; dl/dPg_g += c_g^T y_g, and dl/dw_h sums (Pg_g / W_g) (y_g[m_h] - s_g) over the listed g != h that share, s_g the
// shared mean sum_{h != g} (w_h / W_g) y_g[m_h].
__global__ __launch_bounds__(PF_THREADS) void gns_dcg1_adjoint_reduce_kernel(const int32_t* __restrict__ topo, const float* __restrict__ lines,
                                                                             const float* __restrict__ gens,
                                                                             const int32_t* __restrict__ gen_list, const int n_gen,
                                                                             const double* __restrict__ pickup, const int pickup_per_grid,
                                                                             const int nchunks, const double* __restrict__ partials,
                                                                             const double* __restrict__ ycols, double* __restrict__ gen_ws,
                                                                             float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                             float* __restrict__ gg_out, double* __restrict__ gp_out) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int np = (int)dcn1_adjoint_partial(topo);
  const double* part = partials + (size_t)g * nchunks * np;

  const double status = dcn1_reduce_status(part, nchunks, np);
  if (status != DCN1_PART_OK) {
    const bool nan = status == DCN1_PART_NAN;
    pf_adjoint_fill(g, N, E, Gn, nan ? __builtin_nanf("") : 0.0f, gb_out, gl_out, gg_out);
    if (gp_out) for (int h = lane; h < Gn; h += PF_THREADS) gp_out[(size_t)g * Gn + h] = nan ? __builtin_nan("") : 0.0;
    return;
  }
  dcn1_reduce_buses_lines(topo, lines + (size_t)g * E * 7, nchunks, part, g, gb_out, gl_out);
  if (!gg_out && !gp_out) return;

  // a lane per listed generator: W_g in generator-index order as the forward sums it, then s_g and y_g at its own bus in the blob's
  // by-bus order
  const float* gen = gens + (size_t)g * Gn * 7;
  const double* wg = pickup ? pickup + (pickup_per_grid ? (size_t)g * Gn : 0) : nullptr;
  const double* yg = ycols + (size_t)g * n_gen * N;
  double* gw = gen_ws + (size_t)g * n_gen * DCG1_GEN;
  for (int c = lane; c < n_gen; c += PF_THREADS) {
    const int gi = gen_list[c];
    const double* y = yg + (size_t)c * N;
    double W = 0.0;
    if (wg)
      for (int h = 0; h < Gn; ++h)
        if (h != gi) W += wg[h];
    const bool shared = W > 0.0;
    double s = 0.0, own = 0.0;
    for (int i = 0; i < N; ++i)
      for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) {
        const int h = gen_idx[q];
        if (h == gi) own = y[i];
        else if (shared) s += (wg[h] / W) * y[i];
      }
    gw[c * DCG1_GEN] = shared ? (double)gen[gi * 7 + 6] / W : 0.0;
    gw[c * DCG1_GEN + 1] = s;
    gw[c * DCG1_GEN + 2] = s - own;
  }
  __threadfence_block();
  __syncthreads();

  for (int q = lane; q < Gn; q += PF_THREADS) {        // a lane per generator, in the blob's by-bus order
    const int bus = pf_slot_bus(gen_ptr, N, q), h = gen_idx[q];
    double dpg = dcn1_reduce_dp(part, nchunks, np, bus), dw = 0.0;
    for (int c = 0; c < n_gen; ++c) {                  // the listed generators in list order
      const double coef = gw[c * DCG1_GEN];
      if (gen_list[c] == h) dpg += gw[c * DCG1_GEN + 2];
      else if (coef != 0.0) dw += coef * (yg[(size_t)c * N + bus] - gw[c * DCG1_GEN + 1]);
    }
    if (gg_out) {
      float* row = gg_out + ((size_t)g * Gn + h) * 7;
      for (int c = 0; c < 6; ++c) row[c] = 0.0f;
      row[6] = (float)dpg;                             // Pg
    }
    if (gp_out) gp_out[(size_t)g * Gn + h] = dw;
  }
}
}  // namespace

extern "C" int gns_dcg1_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return gns_dcn1_lds_bytes(topo_host, bytes, lanes);
}

extern "C" int gns_dcg1_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_line, int32_t n_gen,
                                        size_t* bytes) {
  return dcrow_ws_query(cfg, topo_host, bytes && Bt > 0 && n_line >= 0 && n_gen > 0, Bt, n_line, n_gen, bytes);
}

extern "C" int gns_dcg1_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* line_host, const int32_t* line_dev, int32_t n_line,
                               const int32_t* gen_host, const int32_t* gen_dev, int32_t n_gen,
                               const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                               double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || (n_line > 0 && !line_dev) || !gen_dev ||
      !row_cols_dev || !islanding || !worst_loading || !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1) ||
      (pickup_per_grid != 0 && pickup_per_grid != 1))
    return GNS_EINVAL;
  const int rc = dcg1_check(cfg, topo_host, line_host, n_line, gen_host, n_gen, row_cols_host, n_row);
  if (rc != GNS_OK) return rc;
  const DcrowCall call = {static_cast<const int32_t*>(topo_dev), buses, lines, generators, Bt, islanding, rating, (int)rating_per_grid, stream};
  return dcrow_screen(static_cast<const int32_t*>(topo_host), call,
                      DcrowCands{line_dev, (int)n_line, gen_dev, (int)n_gen, pickup, (int)pickup_per_grid},
                      Dcg1Rows{line_dev, (int)n_line, (int)n_gen, row_cols_dev}, n_row, line_flow, worst_loading, worst_line, converged,
                      workspace, workspace_bytes);
}

extern "C" int gns_dcg1_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return dcrow_adjoint_lds_query(topo_host, bytes, lanes);
}

extern "C" int gns_dcg1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_line,
                                                int32_t n_gen, int32_t n_row, size_t* bytes) {
  const bool args_ok = bytes && Bt > 0 && n_line >= 0 && n_gen > 0 && n_row > 0;
  return dcrow_adjoint_ws_query(cfg, topo_host, args_ok, Bt, n_line, n_gen, n_row, Dcg1Rows::REC,
                                cfg ? dcg1_adjoint_own(cfg->n_bus, n_gen) : 0, bytes);
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.  The reduce launch: the
// chunks in order, the contract, every element written; a lane per listed generator forms W_g, the shared mean of y_g and
// c_g^T y_g, then a lane per generator adds the Pg term and sums the gradient of the weights in list order.
extern "C" int gns_dcg1_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* line_host, const int32_t* line_dev, int32_t n_line,
                                const int32_t* gen_host, const int32_t* gen_dev, int32_t n_gen,
                                const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                                const int32_t* worst_line, const uint8_t* converged,
                                const double* grad_line_flow, const double* grad_worst_loading,
                                float* grad_buses, float* grad_lines, float* grad_generators, double* grad_pickup,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || (n_line > 0 && !line_dev) || !gen_dev ||
      !row_cols_dev || !islanding || !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1) ||
      (pickup_per_grid != 0 && pickup_per_grid != 1))
    return GNS_EINVAL;
  const int rc = dcg1_check(cfg, topo_host, line_host, n_line, gen_host, n_gen, row_cols_host, n_row);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const DcrowCall call = {static_cast<const int32_t*>(topo_dev), buses, lines, generators, Bt, islanding, rating, (int)rating_per_grid, stream};
  DcrowAdjointShape s;
  DcrowAdjointWorkspace a;
  const int rl = dcrow_adjoint_launch(h, call, DcrowCands{line_dev, (int)n_line, gen_dev, (int)n_gen, pickup, (int)pickup_per_grid},
                                      Dcg1Rows{line_dev, (int)n_line, (int)n_gen, row_cols_dev}, n_row, dcg1_adjoint_own(h[FH_N], n_gen),
                                      grad_buses || grad_lines || grad_generators || grad_pickup, worst_line, converged, grad_line_flow,
                                      grad_worst_loading, workspace, workspace_bytes, &s, &a);
  if (rl != GNS_OK || !a.T) return rl;
  const double* ycols = a.own;
  double* gen_ws = a.own + Bt * n_gen * h[FH_N];
  return pf_launch<gns_dcg1_adjoint_reduce_kernel>(Bt, 0, stream, call.topo, lines, generators, gen_dev, (int)n_gen, pickup,
                                                   (int)pickup_per_grid, (int)s.chunks_a, (const double*)a.part, ycols, gen_ws,
                                                   grad_buses, grad_lines, grad_generators, grad_pickup);
}
