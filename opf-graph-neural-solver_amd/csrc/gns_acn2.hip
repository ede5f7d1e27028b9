// Batched AC N-2 contingency screening (include/gns_powerflow.h, "AC N-2 contingency screening") on the Newton-Raphson blob: the
// AC N-1 screen (gns_acn1.hip) with two lines out per row.  Two outages remove eight Y-bus stamps and nothing else, so the base
// analysis, its factor slots and its elimination program serve every pair, as they serve every single outage; the caller passes
// the pairs that island a bus.
//
// Mapping: one wave per (grid, pair) on the N-1 screen's LDS image and iteration, warm-started from the base solution.  The
// N-1 screen's pre-kernel (gns_acn1_ybus_kernel, gns_acn1_device.h) writes the base Y-bus of every grid to the workspace once; a
// pair reads its grid's base values and replaces the at most eight entries its lines touch (ff, tt, ft, tf of the lower line,
// then of the higher) by values the wave holds in registers, wave-uniform.  Each is recomputed from the entry's stamps with both
// lines skipped, in stamp order: a sum in a fixed order, never a subtraction, the bits a solve of the grid without the two lines
// computes.  An entry both lines touch (the diagonal of a shared bus, all four entries of parallel lines, the one entry of a line
// from a bus to itself) sits in the set more than once with the same value, so which copy a read meets does not matter.  The
// prologue (acn_view) orders the two lines itself: (k, j) and (j, k) are the same row bit for bit.  Flows and reductions are the N-1 screen's;
// no atomics.
//
// Not chosen: the pair's whole Y-bus in the workspace (16 nnz(Y) bytes per pair: 1.3 GB at 64 case118 grids and 2 000 pairs);
// subtracting the two lines' stamps from the base entries (other bits than a solve without the lines); the N-1 rows of the two
// lines as a start (a second screen before this one, for an iteration or so saved).
//
// The kernels are the N-1 screen's at M = 2 (gns_acn_kernel<2> of gns_acn1_device.h, gns_acn_adjoint_kernel<2> of
// gns_acn_adjoint_device.h), the host bodies acn_screen_call and acn_adjoint_call: a row here is computed with the single-outage
// screen's code, not a copy of it.  This file is the screen's trait (M = 2, the list check, the chunk rule) and its entry points.
//
// The adjoint (gns_acn2_adjoint): gns_acn1_adjoint per solved row (grid, p) on the grid without both lines of the pair, at the
// forward's state.  One wave per (grid, chunk of C consecutive pairs) on the same LDS image; after the prologue a row is
// acn_adjoint_row (gns_acn_adjoint_device.h) on AcnYbus<2>: the Jacobian of the pair on the
// base analysis, one transposed solve, flows and flow cotangents skipped at both lines, exactly 0 into both lines' own columns.
// The partial layout and the kernel that sums a grid's partials are the N-1 adjoint's.  C = max(1, ceil(P / 64)) from the list's
// length alone, never Bt: a wave per row up to 64 pairs, at most 64 chunks per grid after that, whatever the length (the N-1
// adjoint's cap of 8 rows per wave would ask for 1.6 GB of partials at 64 case118 grids and all 17 205 pairs; this rule asks for
// 48 MB there).  Not chosen: a partial per pair; one chunk per grid (P factorisations in a row on one CU for a single grid).
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_acn1_device.h"
#include "gns_acn_adjoint_device.h"

namespace {

// The double-outage screen's rows: a pair of lines per row
struct Acn2Pairs {
  static constexpr int M = 2;
  static constexpr int CHUNKS = 64;        // chunks per grid at most

  // Every pair of the list: two different lines of the blob at h
  static bool list_ok(const int32_t* h, const int32_t* pairs_host, int32_t n_pair) {
    if (!pf_lines_ok(h, pairs_host, 2 * (int64_t)n_pair)) return false;
    for (int32_t p = 0; p < n_pair; ++p)
      if (pairs_host[2 * p] == pairs_host[2 * p + 1]) return false;
    return true;
  }

  // Rows of the pair list a wave of the adjoint walks: 1 up to CHUNKS pairs (a wave per row), then ceil(P / CHUNKS), without a cap:
  // the partials of a grid are bounded, the rows a wave walks are not.  From the list's length alone, never the batch size.
  static int chunk(const int P) {
    const int c = (P + CHUNKS - 1) / CHUNKS;
    return c < 1 ? 1 : c;
  }
};

}  // namespace

extern "C" int gns_acn2_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_pair, size_t* bytes) {
  return acn_workspace_bytes(cfg, topo_host, Bt, n_pair, bytes);
}

extern "C" int gns_acn2_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pair, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid,
                               const double* base_v, const double* base_theta, const uint8_t* base_converged,
                               double* v, double* theta, double* p_from, double* q_from, double* p_to, double* q_to,
                               double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus, double* v_max,
                               int32_t* v_max_bus, uint8_t* converged, int32_t* iterations, double* mismatch,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return acn_screen_call<Acn2Pairs>(cfg, topo_host, topo_dev, buses, lines, generators, Bt, pairs_host, pairs_dev, n_pair, islanding,
                                    rating, rating_per_grid, base_v, base_theta, base_converged, v, theta, p_from, q_from, p_to, q_to,
                                    worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus, converged, iterations, mismatch,
                                    workspace, workspace_bytes, stream);
}

extern "C" int gns_acn2_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_pair,
                                                size_t* bytes) {
  return acn_adjoint_workspace_bytes<Acn2Pairs>(cfg, topo_host, Bt, n_pair, bytes);
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.
extern "C" int gns_acn2_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pair, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid,
                                const double* v, const double* theta, const uint8_t* converged, const int32_t* worst_line,
                                const int32_t* v_min_bus, const int32_t* v_max_bus, const uint8_t* base_converged,
                                const double* grad_v, const double* grad_theta, const double* grad_p_from, const double* grad_q_from,
                                const double* grad_p_to, const double* grad_q_to, const double* grad_worst_loading,
                                const double* grad_v_min, const double* grad_v_max,
                                float* grad_buses, float* grad_lines, float* grad_generators,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return acn_adjoint_call<Acn2Pairs>(
      cfg, topo_host, topo_dev, buses, lines, generators, Bt, pairs_host, pairs_dev, n_pair, islanding, rating, rating_per_grid, v, theta,
      converged, worst_line, v_min_bus, v_max_bus, base_converged,
      {grad_v, grad_theta, grad_p_from, grad_q_from, grad_p_to, grad_q_to, grad_worst_loading, grad_v_min, grad_v_max}, grad_buses,
      grad_lines, grad_generators, workspace, workspace_bytes, stream);
}
