// Batched DC N-2 contingency screening (include/gns_powerflow.h, "DC N-2 contingency screening") on the fast-decoupled blob.  A
// double-line outage is a rank-2 change of Bbus[r, r], so the post-outage flows of the pair (j, k) come from the two single-line
// solves z_j, z_k on the base factor (what gns_dcn1.hip makes per outage) and a 2x2 system per pair.  Per grid that is one solve per
// distinct line of the pair list, not one factorisation per pair.
//
// The kernels, the workspace and the host code after the checks are gns_dcn2_device.h's, shared with gns_dcg1.hip: the factor kernel
// over the candidate lines (no generators), so z_c is the N-1 screen's bit for bit, then the row kernel over the pairs; the adjoint
// (gns_dcn2_adjoint) runs the factor kernel again, the adjoint's row, gather and solve kernels, and gns_dcn1_adjoint_reduce_kernel.
// Here: the pair as a row model (Dcn2Pairs: the 2x2 system, F'_l from the two H rows, v = M^-T ga), the list check and the entry
// points.  The row orders the two lines of a pair itself, so (k, j) gives the bits of (j, k).
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn2_device.h"

namespace {

// The lists of a call: the candidate lines, ascending (no generators), and per pair two positions into them
struct Dcn2Pairs {
  static constexpr int NOUT = 2;
  static constexpr int REC = 6;   // doubles of a (grid, pair) record: a_j, a_k, v_j, v_k, the worst-line term, (contributes, worst line)
  const int32_t* line_list;
  int n_line, n_gen;
  const int32_t* cols;

  __device__ __forceinline__ int n_cand() const { return n_line; }

  // The two candidates of pair p, the lower first: cand ascends, so the lower line first, whatever the pair's order
  __device__ __forceinline__ int2 pair(const int p) const {
    const int cj = cols[2 * (size_t)p], ck = cols[2 * (size_t)p + 1];
    return cj > ck ? make_int2(ck, cj) : make_int2(cj, ck);
  }

  struct Row : DcrowOut<2> {
    using Sums = DcrowSums<2>;
    int2 c;
    const double* Hj;
    const double* Hk;
    double m11, m12, m21, m22, det, a_j, a_k;

    __device__ __forceinline__ bool place(const Dcn2Pairs& s, const int p) {
      c = s.pair(p);
      return c.x >= 0 && c.y < s.n_line && c.x != c.y;
    }
    // (I - diag(b) M^T Z) a = F_S: the same six scalars on every lane
    __device__ __forceinline__ bool solve(const Dcn2Pairs& s, const DcrowBase& g) {
      const int ej = s.line_list[c.x], ek = s.line_list[c.y];
      e[0] = ej;
      e[1] = ek;
      Hj = g.H + (size_t)c.x * g.E;
      Hk = g.H + (size_t)c.y * g.E;
      m11 = 1.0 - g.b[ej] * Hj[ej]; m12 = 0.0 - g.b[ej] * Hk[ej];
      m21 = 0.0 - g.b[ek] * Hj[ek]; m22 = 1.0 - g.b[ek] * Hk[ek];
      det = m11 * m22 - m12 * m21;
      a_j = (g.F[ej] * m22 - m12 * g.F[ek]) / det;
      a_k = (m11 * g.F[ek] - m21 * g.F[ej]) / det;
      return g.fin[c.x] != 0.0 && g.fin[c.y] != 0.0 && pf_finite(det) && det != 0.0 && pf_finite(a_j) && pf_finite(a_k);
    }
    __device__ __forceinline__ double flow(const DcrowBase& g, const int l) const {
      return g.F[l] + g.b[l] * (Hj[l] * a_j + Hk[l] * a_k);
    }
    // ga = sum_l G_l b_l (H_j[l], H_k[l])
    __device__ __forceinline__ Sums ga_term(const DcrowBase&, const double x, const int l) const { return {{x * Hj[l], x * Hk[l]}}; }
    // v = M^-T ga
    __device__ __forceinline__ void close(const Sums& ga) {
      v[0] = (ga.s[0] * m22 - m21 * ga.s[1]) / det;
      v[1] = (m11 * ga.s[1] - m12 * ga.s[0]) / det;
    }
    __device__ __forceinline__ void record(double* rec) const { rec[0] = a_j; rec[1] = a_k; rec[2] = v[0]; rec[3] = v[1]; }
  };

  __device__ __forceinline__ bool holds(const int p, const int c) const {
    return cols[2 * (size_t)p] == c || cols[2 * (size_t)p + 1] == c;
  }
  // T'_c takes G a_pc, and the 2x2 terms -gM[r][c] = v_r a_pc at the two outaged lines
  __device__ __forceinline__ DcrowHeld<2> held(const int p, const int c, const double* rec) const {
    const int2 cc = pair(p);
    DcrowHeld<2> h;
    h.e[0] = line_list[cc.x];
    h.e[1] = line_list[cc.y];
    h.v[0] = rec[2];
    h.v[1] = rec[3];
    h.a_c = cc.x == c ? rec[0] : rec[1];
    return h;
  }
};

// One blob, one candidate list and one pair list: GNS_EINVAL unless it is an FD blob of cfg's shape, the candidates are lines of it,
// ascending and distinct, and every pair holds two different positions into them
int dcn2_check(const gns_pf_config* cfg, const void* topo_host, const int32_t* cand_host, int32_t n_cand,
               const int32_t* pair_cols_host, int32_t n_pair) {
  if (!cfg || !topo_host || !cand_host || n_cand <= 0 || !pair_cols_host || n_pair <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (!dcg1_list_ok(cand_host, n_cand, h[FH_E])) return GNS_EINVAL;
  for (int64_t p = 0; p < n_pair; ++p) {
    const int32_t a = pair_cols_host[2 * p], b = pair_cols_host[2 * p + 1];
    if (a < 0 || a >= n_cand || b < 0 || b >= n_cand || a == b) return GNS_EINVAL;
  }
  return GNS_OK;
}

}  // namespace

extern "C" int gns_dcn2_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return gns_dcn1_lds_bytes(topo_host, bytes, lanes);
}

extern "C" int gns_dcn2_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_cand, size_t* bytes) {
  return dcrow_ws_query(cfg, topo_host, bytes && Bt > 0 && n_cand > 0, Bt, n_cand, 0, bytes);
}

extern "C" int gns_dcn2_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* cand_host, const int32_t* cand_dev, int32_t n_cand,
                               const int32_t* pair_cols_host, const int32_t* pair_cols_dev, int32_t n_pair, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid,
                               double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cand_dev || !pair_cols_dev || !islanding || !worst_loading || !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1))
    return GNS_EINVAL;
  const int rc = dcn2_check(cfg, topo_host, cand_host, n_cand, pair_cols_host, n_pair);
  if (rc != GNS_OK) return rc;
  const DcrowCall call = {static_cast<const int32_t*>(topo_dev), buses, lines, generators, Bt, islanding, rating, (int)rating_per_grid, stream};
  return dcrow_screen(static_cast<const int32_t*>(topo_host), call, DcrowCands{cand_dev, (int)n_cand, nullptr, 0, nullptr, 0},
                      Dcn2Pairs{cand_dev, (int)n_cand, 0, pair_cols_dev}, n_pair, line_flow, worst_loading, worst_line, converged, workspace,
                      workspace_bytes);
}

extern "C" int gns_dcn2_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return dcrow_adjoint_lds_query(topo_host, bytes, lanes);
}

extern "C" int gns_dcn2_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_cand,
                                                int32_t n_pair, size_t* bytes) {
  return dcrow_adjoint_ws_query(cfg, topo_host, bytes && Bt > 0 && n_cand > 0 && n_pair > 0, Bt, n_cand, 0, n_pair, Dcn2Pairs::REC, 0, bytes);
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.
extern "C" int gns_dcn2_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* cand_host, const int32_t* cand_dev, int32_t n_cand,
                                const int32_t* pair_cols_host, const int32_t* pair_cols_dev, int32_t n_pair, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid,
                                const int32_t* worst_line, const uint8_t* converged,
                                const double* grad_line_flow, const double* grad_worst_loading,
                                float* grad_buses, float* grad_lines, float* grad_generators,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cand_dev || !pair_cols_dev || !islanding ||
      !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1))
    return GNS_EINVAL;
  const int rc = dcn2_check(cfg, topo_host, cand_host, n_cand, pair_cols_host, n_pair);
  if (rc != GNS_OK) return rc;
  const DcrowCall call = {static_cast<const int32_t*>(topo_dev), buses, lines, generators, Bt, islanding, rating, (int)rating_per_grid, stream};
  DcrowAdjointShape s;
  DcrowAdjointWorkspace a;
  const int rl = dcrow_adjoint_launch(static_cast<const int32_t*>(topo_host), call, DcrowCands{cand_dev, (int)n_cand, nullptr, 0, nullptr, 0},
                                      Dcn2Pairs{cand_dev, (int)n_cand, 0, pair_cols_dev}, n_pair, 0, grad_buses || grad_lines || grad_generators,
                                      worst_line, converged, grad_line_flow, grad_worst_loading, workspace, workspace_bytes, &s, &a);
  if (rl != GNS_OK || !a.T) return rl;
  return pf_launch<gns_dcn1_adjoint_reduce_kernel>(Bt, 0, stream, call.topo, lines, (int)s.chunks_a, (const double*)a.part, grad_buses,
                                                   grad_lines, grad_generators);
}
