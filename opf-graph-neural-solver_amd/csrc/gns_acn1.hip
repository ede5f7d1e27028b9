// Batched AC N-1 contingency screening (include/gns_powerflow.h, "AC contingency screening") on the Newton-Raphson blob.  The outage
// of a line removes its four Y-bus stamps and nothing else, so the Jacobian of the grid without the line has a subset of the base
// pattern: the base analysis, its factor slots and its elimination program serve every outage; entries that lose their only line
// are numeric zeros.  There is no pivoting to upset, and the caller passes the outages that island a bus (the bridges).
//
// Mapping: one wave per (grid, outage) pair with Newton-Raphson's LDS image (factor, right-hand side, eight bus vectors) and its
// iteration, warm-started from the base solution.  The Y-bus: a pre-kernel with a wave per grid writes the base Y-bus of every grid
// to the workspace once (pf_ybus_row, 16 nnz(Y) bytes per grid); a pair reads its grid's base values and replaces the at most four
// entries its line touches (ff, tt, ft, tf) by values the wave holds in registers, each recomputed from the entry's stamps without
// the line, in stamp order: a sum in a fixed order, never a subtraction, the bits a solve of the grid without the line computes.
// After the iteration a line per lane computes the four branch flows from the line's own stamps (contiguous stores), and the worst
// loading and the voltage extremes are reduced over the wave with a comparison that does not depend on the order (the extreme
// value, the lowest index among equals).  No atomics.
//
// Not chosen: the pair's whole Y-bus in the workspace (16 nnz(Y) bytes per pair: 0.3 GB at 256 case118 grids and 166 outages, and
// the wrapper would slice the outage list); it would let the iteration read Y without the four compares per entry.
//
// The adjoint (gns_acn1_adjoint): per solved row the implicit function theorem on the grid without the line at the forward's state
// (v, theta are inputs: Newton is not run again).  One wave per (grid, chunk of C consecutive outages) on the same LDS image, lambda
// in the Psp / Qsp vectors; J_k from ac_jacobian_row (gns_ac_device.h) on the pair's Y-bus, factored by the leading factor steps of the blob's
// program, then the transposed program, as pf_adjoint_grid does.  The flow cotangents reach dl/dx by a gather with a bus per lane
// over the stamps of its diagonal entry (no scatter, no atomics).  The wave walks its rows in order and every lane adds into the
// addresses it alone owns of the chunk's fp64 partial in the workspace (4 N + 5 E + Gn + 1 doubles); a second kernel, a wave per
// grid, sums the chunks in order, applies the contract and rounds once to fp32.  C = min(8, max(1, ceil(K / 32))) from the list's
// length alone, never Bt: a wave per row up to 32 outages, about 32 chunks per grid after that.  Workspace: the base Y-bus plus
// Bt ceil(K / C) partials.  Not chosen: C = 1 always (a partial per pair, 0.5 GB at 256 case118 grids x 166 outages); one chunk per
// grid (K factorisations in a row on one CU for a single grid); atomics (no fixed order of the sums); rows side by side in one
// wave as gns_dcn1.hip does (each row has its own factor here: nnz(L+U) doubles of LDS per row).
//
// The kernels are in the two headers, once for both screens: gns_acn_kernel<M> (gns_acn1_device.h: the prologue acn_view, then
// acn_solve_row) and gns_acn_adjoint_kernel<M> (gns_acn_adjoint_device.h: the same prologue, then acn_adjoint_row, over a chunk's
// rows), with the host's acn_screen_call and acn_adjoint_call.  This file is the screen's trait (M = 1, the list check, the chunk
// rule) and its four entry points; gns_acn2.hip is the same at M = 2.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_acn1_device.h"
#include "gns_acn_adjoint_device.h"

namespace {

// The single-outage screen's rows: a line per row
struct Acn1Rows {
  static constexpr int M = 1;
  static constexpr int CHUNK_MAX = 8;      // rows a wave of the adjoint walks at most
  static constexpr int CHUNKS = 32;        // chunks per grid a list is cut into before the chunks grow

  // Every outage of the list: a line of the blob at h
  static bool list_ok(const int32_t* h, const int32_t* outages_host, int32_t n_outage) { return pf_lines_ok(h, outages_host, n_outage); }

  // Rows of the outage list a wave of the adjoint walks: 1 up to CHUNKS outages (a wave per row), then ceil(K / CHUNKS), at most
  // CHUNK_MAX: the rows a wave walks are bounded, the partials of a grid are not.  From the list's length alone, never the batch
  // size: the order of a grid's sums does not depend on its batch.
  static int chunk(const int K) {
    const int c = (K + CHUNKS - 1) / CHUNKS;
    return c < 1 ? 1 : c > CHUNK_MAX ? CHUNK_MAX : c;
  }
};

}  // namespace

extern "C" int gns_acn1_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage, size_t* bytes) {
  return acn_workspace_bytes(cfg, topo_host, Bt, n_outage, bytes);
}

extern "C" int gns_acn1_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid,
                               const double* base_v, const double* base_theta, const uint8_t* base_converged,
                               double* v, double* theta, double* p_from, double* q_from, double* p_to, double* q_to,
                               double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus, double* v_max,
                               int32_t* v_max_bus, uint8_t* converged, int32_t* iterations, double* mismatch,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return acn_screen_call<Acn1Rows>(cfg, topo_host, topo_dev, buses, lines, generators, Bt, outages_host, outages_dev, n_outage, islanding,
                                   rating, rating_per_grid, base_v, base_theta, base_converged, v, theta, p_from, q_from, p_to, q_to,
                                   worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus, converged, iterations, mismatch,
                                   workspace, workspace_bytes, stream);
}

extern "C" int gns_acn1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage,
                                                size_t* bytes) {
  return acn_adjoint_workspace_bytes<Acn1Rows>(cfg, topo_host, Bt, n_outage, bytes);
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.
extern "C" int gns_acn1_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid,
                                const double* v, const double* theta, const uint8_t* converged, const int32_t* worst_line,
                                const int32_t* v_min_bus, const int32_t* v_max_bus, const uint8_t* base_converged,
                                const double* grad_v, const double* grad_theta, const double* grad_p_from, const double* grad_q_from,
                                const double* grad_p_to, const double* grad_q_to, const double* grad_worst_loading,
                                const double* grad_v_min, const double* grad_v_max,
                                float* grad_buses, float* grad_lines, float* grad_generators,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return acn_adjoint_call<Acn1Rows>(
      cfg, topo_host, topo_dev, buses, lines, generators, Bt, outages_host, outages_dev, n_outage, islanding, rating, rating_per_grid, v,
      theta, converged, worst_line, v_min_bus, v_max_bus, base_converged,
      {grad_v, grad_theta, grad_p_from, grad_q_from, grad_p_to, grad_q_to, grad_worst_loading, grad_v_min, grad_v_max}, grad_buses,
      grad_lines, grad_generators, workspace, workspace_bytes, stream);
}
