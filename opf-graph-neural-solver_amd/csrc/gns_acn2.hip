// Batched AC N-2 contingency screening (include/gns_powerflow.h, "AC N-2 contingency screening") on the Newton-Raphson blob: the
// AC N-1 screen (gns_acn1.hip) with two lines out per row.  Two outages remove eight Y-bus stamps and nothing else, so the base
// analysis, its factor slots and its elimination program serve every pair, as they serve every single outage; the caller passes
// the pairs that island a bus.
//
// Mapping: one wave per (grid, pair) on gns_acn1_kernel's LDS image and iteration, warm-started from the base solution.  The
// N-1 screen's pre-kernel (gns_acn1_ybus_kernel, gns_acn1_device.h) writes the base Y-bus of every grid to the workspace once; a
// pair reads its grid's base values and replaces the at most eight entries its lines touch (ff, tt, ft, tf of the lower line,
// then of the higher) by values the wave holds in registers, wave-uniform.  Each is recomputed from the entry's stamps with both
// lines skipped, in stamp order: a sum in a fixed order, never a subtraction, the bits a solve of the grid without the two lines
// computes.  An entry both lines touch (the diagonal of a shared bus, all four entries of parallel lines, the one entry of a line
// from a bus to itself) sits in the set more than once with the same value, so which copy a read meets does not matter.  The
// kernel orders the two lines itself: (k, j) and (j, k) are the same row bit for bit.  Flows and reductions are the N-1 screen's;
// no atomics.
//
// Not chosen: the pair's whole Y-bus in the workspace (16 nnz(Y) bytes per pair: 1.3 GB at 64 case118 grids and 2 000 pairs);
// subtracting the two lines' stamps from the base entries (other bits than a solve without the lines); the N-1 rows of the two
// lines as a start (a second screen before this one, for an iteration or so saved).
//
// A row after the prologue is acn_solve_row (gns_acn1_device.h), the routine gns_acn1_kernel runs, on this screen's Y-bus view: a
// row here is computed with the single-outage screen's code, not a copy of it.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_acn1_device.h"

namespace {

// Row blockIdx.x = grid * P + position in the pair list
__global__ __launch_bounds__(PF_THREADS) void gns_acn2_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                              const float* __restrict__ lines, const float* __restrict__ gens,
                                                              const int32_t* __restrict__ pairs, const int P,
                                                              const uint8_t* __restrict__ islanding,
                                                              const double* __restrict__ rating, const int rating_per_grid,
                                                              const double* __restrict__ v0, const double* __restrict__ th0,
                                                              const uint8_t* __restrict__ conv0,
                                                              const double2* __restrict__ ybus_ws, const int max_iter,
                                                              const double tol, const Acn1Out o) {
  const size_t row = blockIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)P), pi = (int)(blockIdx.x % (unsigned)P);
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], nnzY = topo[PH_NNZY];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;

  // the pair's Y-bus, or a row that is not solved: an islanding pair, a grid without a base solution, a line that is not one of
  // the grid's (its index, or its id columns against the blob's pattern), twice the same line.  The same decision in every lane.
  const int j = min(pairs[2 * pi], pairs[2 * pi + 1]), k = max(pairs[2 * pi], pairs[2 * pi + 1]);
  int fj = 0, tj = 0, fk = 0, tk = 0;
  bool ok = j >= 0 && k < E && j != k && !islanding[pi] && conv0[g] != 0;
  ok = ok && acn1_line_ends(line, j, N, fj, tj) && acn1_line_ends(line, k, N, fk, tk);
  Acn2Ybus Y;
  Y.base = ybus_ws + (size_t)g * nnzY;
  Y.j = j; Y.k = k;
  if (ok) {
    Y.p[0] = y_diag[fj];
    Y.p[1] = y_diag[tj];
    Y.p[2] = acn1_find_entry(y_ptr, y_col, fj, tj);
    Y.p[3] = acn1_find_entry(y_ptr, y_col, tj, fj);
    Y.p[4] = y_diag[fk];
    Y.p[5] = y_diag[tk];
    Y.p[6] = acn1_find_entry(y_ptr, y_col, fk, tk);
    Y.p[7] = acn1_find_entry(y_ptr, y_col, tk, fk);
    ok = Y.p[2] >= 0 && Y.p[3] >= 0 && Y.p[6] >= 0 && Y.p[7] >= 0;
  }
  if (!ok) { acn1_row_not_solved(o, row, N, E); return; }
  Y.y[0] = acn_entry_without(fj, Y.p[0], Y, y_diag, st_ptr, st, bus, line);
  Y.y[1] = acn_entry_without(tj, Y.p[1], Y, y_diag, st_ptr, st, bus, line);
  Y.y[2] = acn_entry_without(fj, Y.p[2], Y, y_diag, st_ptr, st, bus, line);
  Y.y[3] = acn_entry_without(tj, Y.p[3], Y, y_diag, st_ptr, st, bus, line);
  Y.y[4] = acn_entry_without(fk, Y.p[4], Y, y_diag, st_ptr, st, bus, line);
  Y.y[5] = acn_entry_without(tk, Y.p[5], Y, y_diag, st_ptr, st, bus, line);
  Y.y[6] = acn_entry_without(fk, Y.p[6], Y, y_diag, st_ptr, st, bus, line);
  Y.y[7] = acn_entry_without(tk, Y.p[7], Y, y_diag, st_ptr, st, bus, line);

  acn_solve_row(topo, bus, line, gen, g, row, Y, rating, rating_per_grid, v0, th0, max_iter, tol, o);
}

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
  // every pair: two different lines of the blob
  const auto pairs_ok = [&](const int32_t* h) {
    if (!pf_lines_ok(h, pairs_host, 2 * (int64_t)n_pair)) return false;
    for (int32_t p = 0; p < n_pair; ++p)
      if (pairs_host[2 * p] == pairs_host[2 * p + 1]) return false;
    return true;
  };
  int64_t lds = 0;
  Acn1Out out;
  const int rc = acn_screen_begin(cfg, topo_host, topo_dev, buses, lines, generators, Bt, pairs_host, pairs_dev, n_pair, islanding,
                                  rating_per_grid, base_v, base_theta, base_converged, v, theta, p_from, q_from, p_to, q_to,
                                  worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus, converged, iterations, mismatch,
                                  workspace, workspace_bytes, stream, pairs_ok, &lds, &out);
  if (rc != GNS_OK) return rc;
  return pf_launch<gns_acn2_kernel>(Bt * n_pair, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators,
                                    pairs_dev, (int)n_pair, islanding, rating, (int)rating_per_grid, base_v, base_theta,
                                    base_converged, static_cast<const double2*>(workspace), cfg->max_iter, cfg->tol, out);
}
