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
//
// The adjoint (gns_acn2_adjoint): gns_acn1_adjoint per solved row (grid, p) on the grid without both lines of the pair, at the
// forward's state.  One wave per (grid, chunk of C consecutive pairs) on the same LDS image; after the prologue a row is
// acn_adjoint_row (gns_acn_adjoint_device.h), the routine gns_acn1_adjoint_kernel runs, on Acn2Ybus: the Jacobian of the pair on the
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

// ---- the adjoint (gns_acn2_adjoint)

constexpr int ACN2_ADJ_CHUNKS = 64;        // chunks per grid at most

// Rows of the pair list a wave walks: 1 up to ACN2_ADJ_CHUNKS pairs (a wave per row), then ceil(P / ACN2_ADJ_CHUNKS), without a cap:
// the partials of a grid are bounded, the rows a wave walks are not.  From the list's length alone, never the batch size.
__device__ __host__ inline int acn2_adjoint_chunk(const int P) {
  const int c = (P + ACN2_ADJ_CHUNKS - 1) / ACN2_ADJ_CHUNKS;
  return c < 1 ? 1 : c;
}

// Workgroup blockIdx.x = grid * nchunks + chunk: rows p0 .. p0 + C of the grid, in order, as gns_acn1_adjoint_kernel walks its rows
__global__ __launch_bounds__(PF_THREADS) void gns_acn2_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const float* __restrict__ gens,
                                                                      const int32_t* __restrict__ pairs, const int P,
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
  const int g = (int)(blockIdx.x / (unsigned)nchunks), p0 = (int)(blockIdx.x % (unsigned)nchunks) * C;
  const int nrow = min(C, P - p0);
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

  for (int r = 0; r < nrow; ++r) {
    const int pi = p0 + r;
    const size_t row = (size_t)g * P + pi;
    // a row whose incoming gradients are all exactly zero or NULL is skipped, never multiplied by zero
    if (!acn1_row_nonzero(gr, row, N, E)) continue;
    // a row without a solution (no base solution, an islanding pair, a stopped or unconverged iteration): the grid's gradient is
    // NaN.  The view is gns_acn2_kernel's: the lower line first, whichever order the list names them in.
    const int j = min(pairs[2 * pi], pairs[2 * pi + 1]), k = max(pairs[2 * pi], pairs[2 * pi + 1]);
    int fj = 0, tj = 0, fk = 0, tk = 0;
    bool ok = conv0[g] != 0 && conv_in[row] != 0 && j >= 0 && k < E && j != k && !islanding[pi];
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
    if (!ok) { acn1_partial_status(part, np, ACN1_PART_NAN); return; }
    Y.y[0] = acn_entry_without(fj, Y.p[0], Y, y_diag, st_ptr, st, bus, line);
    Y.y[1] = acn_entry_without(tj, Y.p[1], Y, y_diag, st_ptr, st, bus, line);
    Y.y[2] = acn_entry_without(fj, Y.p[2], Y, y_diag, st_ptr, st, bus, line);
    Y.y[3] = acn_entry_without(tj, Y.p[3], Y, y_diag, st_ptr, st, bus, line);
    Y.y[4] = acn_entry_without(fk, Y.p[4], Y, y_diag, st_ptr, st, bus, line);
    Y.y[5] = acn_entry_without(tk, Y.p[5], Y, y_diag, st_ptr, st, bus, line);
    Y.y[6] = acn_entry_without(fk, Y.p[6], Y, y_diag, st_ptr, st, bus, line);
    Y.y[7] = acn_entry_without(tk, Y.p[7], Y, y_diag, st_ptr, st, bus, line);

    if (!acn_adjoint_row(topo, line, row, Y, rt, gr, v_in, th_in, wl_in, lo_in, hi_in, part)) {
      acn1_partial_status(part, np, ACN1_PART_NAN);
      return;
    }
    solved_row = true;
  }
  // a grid without a base solution whose chunk asked for nothing: zero rows when every chunk says so
  acn1_partial_status(part, np, !solved_row && conv0[g] == 0 ? ACN1_PART_UNSOLVED_ZERO : ACN1_PART_OK);
}

// Every pair of the list: two different lines of the blob at h
bool acn2_pairs_ok(const int32_t* h, const int32_t* pairs_host, int32_t n_pair) {
  if (!pf_lines_ok(h, pairs_host, 2 * (int64_t)n_pair)) return false;
  for (int32_t p = 0; p < n_pair; ++p)
    if (pairs_host[2 * p] == pairs_host[2 * p + 1]) return false;
  return true;
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
  const auto pairs_ok = [&](const int32_t* h) { return acn2_pairs_ok(h, pairs_host, n_pair); };
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

extern "C" int gns_acn2_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_pair,
                                                size_t* bytes) {
  return acn_adjoint_workspace_bytes(cfg, topo_host, Bt, n_pair, acn2_adjoint_chunk(n_pair), bytes);
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
  const int C = acn2_adjoint_chunk(n_pair);
  const Acn1Grad gr = {grad_v, grad_theta, grad_p_from, grad_q_from, grad_p_to, grad_q_to, grad_worst_loading, grad_v_min, grad_v_max};
  return acn_adjoint_call(
      cfg, topo_host, topo_dev, buses, lines, generators, Bt, pairs_host, pairs_dev, n_pair, islanding, rating_per_grid, v, theta,
      converged, worst_line, v_min_bus, v_max_bus, base_converged, grad_buses, grad_lines, grad_generators, workspace,
      workspace_bytes, stream, C, [&](const int32_t* h) { return acn2_pairs_ok(h, pairs_host, n_pair); },
      [&](int64_t lds, int64_t nchunks, const double2* ybus, double* partials) {
        return pf_launch<gns_acn2_adjoint_kernel>(Bt * nchunks, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines,
                                                  generators, pairs_dev, (int)n_pair, islanding, rating, (int)rating_per_grid, v,
                                                  theta, converged, worst_line, v_min_bus, v_max_bus, base_converged, gr, ybus, C,
                                                  (int)nchunks, partials);
      });
}
