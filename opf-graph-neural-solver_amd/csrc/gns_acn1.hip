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
// in the Psp / Qsp vectors; J_k from acn1_jacobian_row on the pair's Y-bus, factored by the leading factor steps of the blob's
// program, then the transposed program, as pf_adjoint_grid does.  The flow cotangents reach dl/dx by a gather with a bus per lane
// over the stamps of its diagonal entry (no scatter, no atomics).  The wave walks its rows in order and every lane adds into the
// addresses it alone owns of the chunk's fp64 partial in the workspace (4 N + 5 E + Gn + 1 doubles); a second kernel, a wave per
// grid, sums the chunks in order, applies the contract and rounds once to fp32.  C = min(8, max(1, ceil(K / 32))) from the list's
// length alone, never Bt: a wave per row up to 32 outages, about 32 chunks per grid after that.  Workspace: the base Y-bus plus
// Bt ceil(K / C) partials.  Not chosen: C = 1 always (a partial per pair, 0.5 GB at 256 case118 grids x 166 outages); one chunk per
// grid (K factorisations in a row on one CU for a single grid); atomics (no fixed order of the sums); rows side by side in one
// wave as gns_dcn1.hip does (each row has its own factor here: nnz(L+U) doubles of LDS per row).
//
// A row after the kernel's prologue (Newton-Raphson, the extremes, the flows, the worst loading) is acn_solve_row of
// gns_acn1_device.h, which the double-outage screen (gns_acn2.hip) runs too on its own Y-bus view; the other helpers both screens
// run, the kernel that writes the base Y-bus and what the two entry points check alike are there as well.  A solved row of the
// adjoint after its prologue is acn_adjoint_row of gns_acn_adjoint_device.h, which the double-outage adjoint runs too; the kernel
// that sums the partials and what the two adjoint entry points do alike are in that header.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_acn1_device.h"
#include "gns_acn_adjoint_device.h"

namespace {

// Pair blockIdx.x = grid * K + position in the outage list
__global__ __launch_bounds__(PF_THREADS) void gns_acn1_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                              const float* __restrict__ lines, const float* __restrict__ gens,
                                                              const int32_t* __restrict__ outages, const int K,
                                                              const uint8_t* __restrict__ islanding,
                                                              const double* __restrict__ rating, const int rating_per_grid,
                                                              const double* __restrict__ v0, const double* __restrict__ th0,
                                                              const uint8_t* __restrict__ conv0,
                                                              const double2* __restrict__ ybus_ws, const int max_iter,
                                                              const double tol, const Acn1Out o) {
  const size_t row = blockIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)K), j = (int)(blockIdx.x % (unsigned)K);
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], nnzY = topo[PH_NNZY];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;

  // the pair's Y-bus, or a row that is not solved: an islanding outage, a grid without a base solution, a line that is not one of
  // the grid's (its index, or its id columns against the blob's pattern).  The same decision in every lane.
  const int k = outages[j];
  int f = 0, t = 0;
  bool ok = k >= 0 && k < E && !islanding[j] && conv0[g] != 0;
  ok = ok && acn1_line_ends(line, k, N, f, t);
  Acn1Ybus Y;
  Y.base = ybus_ws + (size_t)g * nnzY;
  Y.k = k;
  if (ok) {
    Y.p[0] = y_diag[f];
    Y.p[1] = y_diag[t];
    Y.p[2] = acn1_find_entry(y_ptr, y_col, f, t);
    Y.p[3] = acn1_find_entry(y_ptr, y_col, t, f);
    ok = Y.p[2] >= 0 && Y.p[3] >= 0;
  }
  if (!ok) { acn1_row_not_solved(o, row, N, E); return; }
  Y.y[0] = acn_entry_without(f, Y.p[0], Y, y_diag, st_ptr, st, bus, line);
  Y.y[1] = acn_entry_without(t, Y.p[1], Y, y_diag, st_ptr, st, bus, line);
  Y.y[2] = acn_entry_without(f, Y.p[2], Y, y_diag, st_ptr, st, bus, line);
  Y.y[3] = acn_entry_without(t, Y.p[3], Y, y_diag, st_ptr, st, bus, line);

  acn_solve_row(topo, bus, line, gen, g, row, Y, rating, rating_per_grid, v0, th0, max_iter, tol, o);
}

// ---- the adjoint (gns_acn1_adjoint): gradients of a loss of the screen's nine fp64 outputs, per solved row by the implicit function
// theorem on the grid without the row's line: J_k^T lambda = dl/dx at the forward's state, dl/dp = direct - lambda^T dF_k/dp.  The row
// itself is acn_adjoint_row of gns_acn_adjoint_device.h, which the double-outage adjoint (gns_acn2.hip) runs too.

constexpr int ACN1_ADJ_CHUNK_MAX = 8;      // rows a wave walks at most
constexpr int ACN1_ADJ_CHUNKS = 32;        // chunks per grid a list is cut into before the chunks grow

// Rows of the outage list a wave walks: 1 up to ACN1_ADJ_CHUNKS outages (a wave per row), then ceil(K / ACN1_ADJ_CHUNKS), at most
// ACN1_ADJ_CHUNK_MAX.  From the list's length alone, never the batch size: the order of a grid's sums does not depend on its batch.
__device__ __host__ inline int acn1_adjoint_chunk(const int K) {
  const int c = (K + ACN1_ADJ_CHUNKS - 1) / ACN1_ADJ_CHUNKS;
  return c < 1 ? 1 : c > ACN1_ADJ_CHUNK_MAX ? ACN1_ADJ_CHUNK_MAX : c;
}

// Workgroup blockIdx.x = grid * nchunks + chunk: rows k0 .. k0 + C of the grid, in order, each lane adding into the addresses of
// the chunk's partial it alone owns (a bus, a line or a generator slot per lane)
__global__ __launch_bounds__(PF_THREADS) void gns_acn1_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const float* __restrict__ gens,
                                                                      const int32_t* __restrict__ outages, const int K,
                                                                      const uint8_t* __restrict__ islanding,
                                                                      const double* __restrict__ rating, const int rating_per_grid,
                                                                      const double* __restrict__ v_in, const double* __restrict__ th_in,
                                                                      const uint8_t* __restrict__ conv_in,
                                                                      const int32_t* __restrict__ wl_in, const int32_t* __restrict__ lo_in,
                                                                      const int32_t* __restrict__ hi_in,
                                                                      const uint8_t* __restrict__ conv0, const Acn1Grad gr,
                                                                      const double2* __restrict__ ybus_ws, const int C, const int nchunks,
                                                                      double* __restrict__ partials) {
  const int lane = threadIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)nchunks), k0 = (int)(blockIdx.x % (unsigned)nchunks) * C;
  const int nk = min(C, K - k0);
  const int N = topo[PH_N], E = topo[PH_E], nnzY = topo[PH_NNZY];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  const int np = (int)acn1_adjoint_partial(topo);
  double* part = partials + (size_t)blockIdx.x * np;

  for (int q = lane; q < np - 1; q += PF_THREADS) part[q] = 0.0;   // bus i's, line l's and slot q's doubles all sit at lane + 64 m
  bool solved_row = false;

  for (int j = 0; j < nk; ++j) {
    const size_t row = (size_t)g * K + k0 + j;
    // a row whose incoming gradients are all exactly zero or NULL is skipped, never multiplied by zero
    if (!acn1_row_nonzero(gr, row, N, E)) continue;
    // a row without a solution (no base solution, an islanding outage, a stopped or unconverged iteration): the grid's gradient is NaN
    const int k = outages[k0 + j];
    int f = 0, t = 0;
    bool ok = conv0[g] != 0 && conv_in[row] != 0 && k >= 0 && k < E && !islanding[k0 + j] && acn1_line_ends(line, k, N, f, t);
    Acn1Ybus Y;
    Y.base = ybus_ws + (size_t)g * nnzY;
    Y.k = k;
    if (ok) {
      Y.p[0] = y_diag[f];
      Y.p[1] = y_diag[t];
      Y.p[2] = acn1_find_entry(y_ptr, y_col, f, t);
      Y.p[3] = acn1_find_entry(y_ptr, y_col, t, f);
      ok = Y.p[2] >= 0 && Y.p[3] >= 0;
    }
    if (!ok) { acn1_partial_status(part, np, ACN1_PART_NAN); return; }
    Y.y[0] = acn_entry_without(f, Y.p[0], Y, y_diag, st_ptr, st, bus, line);
    Y.y[1] = acn_entry_without(t, Y.p[1], Y, y_diag, st_ptr, st, bus, line);
    Y.y[2] = acn_entry_without(f, Y.p[2], Y, y_diag, st_ptr, st, bus, line);
    Y.y[3] = acn_entry_without(t, Y.p[3], Y, y_diag, st_ptr, st, bus, line);

    if (!acn_adjoint_row(topo, line, row, Y, rt, gr, v_in, th_in, wl_in, lo_in, hi_in, part)) {
      acn1_partial_status(part, np, ACN1_PART_NAN);
      return;
    }
    solved_row = true;
  }
  // a grid without a base solution whose chunk asked for nothing: zero rows when every chunk says so
  acn1_partial_status(part, np, !solved_row && conv0[g] == 0 ? ACN1_PART_UNSOLVED_ZERO : ACN1_PART_OK);
}

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
  int64_t lds = 0;
  Acn1Out out;
  const int rc = acn_screen_begin(cfg, topo_host, topo_dev, buses, lines, generators, Bt, outages_host, outages_dev, n_outage, islanding,
                                  rating_per_grid, base_v, base_theta, base_converged, v, theta, p_from, q_from, p_to, q_to,
                                  worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus, converged, iterations, mismatch,
                                  workspace, workspace_bytes, stream,
                                  [&](const int32_t* h) { return pf_lines_ok(h, outages_host, n_outage); }, &lds, &out);
  if (rc != GNS_OK) return rc;
  return pf_launch<gns_acn1_kernel>(Bt * n_outage, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators,
                                    outages_dev, (int)n_outage, islanding, rating, (int)rating_per_grid, base_v, base_theta,
                                    base_converged, static_cast<const double2*>(workspace), cfg->max_iter, cfg->tol, out);
}

extern "C" int gns_acn1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage,
                                                size_t* bytes) {
  return acn_adjoint_workspace_bytes(cfg, topo_host, Bt, n_outage, acn1_adjoint_chunk(n_outage), bytes);
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
  const int C = acn1_adjoint_chunk(n_outage);
  const Acn1Grad gr = {grad_v, grad_theta, grad_p_from, grad_q_from, grad_p_to, grad_q_to, grad_worst_loading, grad_v_min, grad_v_max};
  return acn_adjoint_call(
      cfg, topo_host, topo_dev, buses, lines, generators, Bt, outages_host, outages_dev, n_outage, islanding, rating_per_grid, v,
      theta, converged, worst_line, v_min_bus, v_max_bus, base_converged, grad_buses, grad_lines, grad_generators, workspace,
      workspace_bytes, stream, C, [&](const int32_t* h) { return pf_lines_ok(h, outages_host, n_outage); },
      [&](int64_t lds, int64_t nchunks, const double2* ybus, double* partials) {
        return pf_launch<gns_acn1_adjoint_kernel>(Bt * nchunks, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines,
                                                  generators, outages_dev, (int)n_outage, islanding, rating, (int)rating_per_grid, v,
                                                  theta, converged, worst_line, v_min_bus, v_max_bus, base_converged, gr, ybus, C,
                                                  (int)nchunks, partials);
      });
}
