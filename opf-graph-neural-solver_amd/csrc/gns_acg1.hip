// Batched AC generator contingency screening (include/gns_powerflow.h, "AC generator contingency screening") on Newton-Raphson
// blobs: Newton-Raphson on every (grid, row) of a list of rows (generator g out, with line k out as well or no line), warm-started
// from the base solution, with the outputs of the AC line screens per row.
//
// What changes with the unit.  A line outage removes Y-bus stamps and leaves the unknowns alone, so the base analysis serves every
// row of gns_acn1.hip.  A generator outage leaves the Y-bus alone and may change the unknowns: the bus of a sole unit turns from PV
// to PQ (|V| becomes an unknown, the Q equation joins the system), and on a shared bus the set point moves to the next unit's vg.
// Both are facts of the topology and of g alone, so the host analyses the topology once per distinct generator of the list with that
// generator's row left out of the roles and of the by-bus lists (gns_pf_prepare_topology_out_gen): the roles, th_idx / vm_idx, the
// by-bus lists (original row numbers), the factor slots and the program of such a blob are those of gns_pf_solve on the grid with
// the generator row deleted.  Nothing is analysed per row, and the line on top of the unit is gns_acn1.hip's Y-bus view on that
// blob: the Y-bus pattern and its stamps come from the lines alone and are the same words in every member, so the members share
// the one base Y-bus per grid that gns_acn1_ybus_kernel writes.
//
// Mapping: one wave per (grid, row) on gns_pf_solve's LDS image; the launch asks for the largest member's.  The row decodes
// (position into the generator list, line or -1), takes its blob at set + member_off[position] after pf_set_member's checks (a bad
// offset indexes nothing outside the set), builds the view with acn_view (k >= 0) or a view with nothing out (k = -1), and runs the
// row routine the line screens run (acn_solve_row, gns_acn1_device.h).  The pickup is that routine's one hook: what a bus's
// specified P gains on top of its remaining generators' Pg, the DC generator screen's expression (gns_dcn2_device.h, dcg1_lane_u):
// W_g summed in generator-row order, Pg_g * (w_h / W_g) per remaining unit in the by-bus order, fp64.
//
// Not chosen: one superset analysis in which every PV bus carries a |V| unknown with a pinned row, so that one blob serves every
// generator: every row would pay a Jacobian of dimension 2 (N - 1) (234 against 181 at case118) and a larger LDS image.  Sharing one
// blob among the generators whose removal changes no role (units on a shared bus with equal consequences): it saves host and device
// memory and changes no result; left for when the blobs' memory is measured to matter.
//
// The adjoint (gns_acg1_adjoint, "Gradients of the AC generator screen"): gns_acn1_adjoint per solved row (grid, (g, k)) on the
// grid without generator row g and line k, at the forward's state.  One wave per (grid, chunk of C consecutive rows) on the same
// LDS image; a row picks its blob, builds its view and sums W_g as gns_acg1_kernel does, then runs acn_adjoint_row
// (gns_acn_adjoint_device.h) on that blob: its unknowns and roles decide where lambda_Q exists (a freed bus is PQ) and which unit's
// vg is a set point.  What a line row cannot do is the generator part: the by-bus slot order differs from member to member, and Pg
// differs per generator per row, so the partial holds four doubles per ORIGINAL generator row (dl/dvg, dl/dPg, dl/dw and the
// bus's lambda_P of the row in hand) and acn_adjoint_row's hook (Acg1Gen) fills them: a remaining unit h gets mu_h = lambda_P of
// its bus (0 at the slack); with W_g > 0 the lost unit gets M = sum_{h != g} mu_h (w_h / W_g), in generator-row order, and the
// weight of h gets Pg_g (mu_h - M) / W_g.  With W_g == 0 (no weights, or all the others' zero) the slack picks up: the lost unit
// and the weights get exactly 0, and that branch is not differentiated.  The reduce kernel here sums the chunks in order with the
// line adjoints' pieces for the buses and the lines, and writes vg, Pg and the weights by generator row.  C = max(1, ceil(n_row /
// 64)), the N-2 adjoint's rule: at most 64 partials per grid however long the list.  The default list is generator-major, so a
// chunk mostly stays on one blob; nothing depends on that.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_acn1_device.h"
#include "gns_acn_adjoint_device.h"

namespace {

// acn_solve_row's hook: the share of the lost unit's Pg that the remaining generators of bus i pick up.  W is W_g, 0 where the
// slack picks up (no weights, or every remaining weight exactly zero); the blob's by-bus lists do not hold the lost unit.
struct Acg1Pickup {
  const double* w;   // the grid's weights by generator row; not read when W is 0
  double pg, W;
  __device__ __forceinline__ double operator()(const int i, const int32_t* gen_ptr, const int32_t* gen_idx) const {
    double dp = 0.0;
    if (W > 0.0)
      for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) dp += pg * (w[gen_idx[q]] / W);
    return dp;
  }
};

// Workgroup blockIdx.x = grid * K + position in the row list.  N, E, Gn are the call's shape (every member's, checked here again),
// lds_bytes the launch's image and nnzY the members' common nnz(Y).
__global__ __launch_bounds__(PF_THREADS) void gns_acg1_kernel(const int32_t* __restrict__ set, const int64_t set_words,
                                                              const int32_t* __restrict__ member_off, const int n_member, const int N,
                                                              const int E, const int Gn, const int64_t lds_bytes, const int nnzY,
                                                              const float* __restrict__ buses, const float* __restrict__ lines,
                                                              const float* __restrict__ gens, const int32_t* __restrict__ gen_list,
                                                              const int32_t* __restrict__ row_cols, const int K,
                                                              const uint8_t* __restrict__ islanding,
                                                              const double* __restrict__ rating, const int rating_per_grid,
                                                              const double* __restrict__ pickup, const int pickup_per_grid,
                                                              const double* __restrict__ v0, const double* __restrict__ th0,
                                                              const uint8_t* __restrict__ conv0,
                                                              const double2* __restrict__ ybus_ws, const int max_iter,
                                                              const double tol, const Acn1Out o) {
  const size_t row = blockIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)K), pos = (int)(blockIdx.x % (unsigned)K);
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;

  // the row's blob: the analysis without generator gen_list[cg].  The same decisions in every lane.
  const int cg = row_cols[2 * (size_t)pos], ck = row_cols[2 * (size_t)pos + 1];
  const int32_t* topo = set;
  int gi = -1;
  bool ok = cg >= 0 && cg < n_member && ck >= -1 && !islanding[pos] && conv0[g] != 0;
  if (ok) {
    ok = pf_set_member<PfBlobKind>(set, set_words, member_off[cg], N, E, Gn, lds_bytes, nnzY, topo) && topo[PH_NNZY] == nnzY;
    gi = gen_list[cg];
    ok = ok && gi >= 0 && gi < Gn;
  }

  // the row's Y-bus: the view without line ck (acn_view refuses a line that is not the grid's), or with nothing out
  AcnYbus<1> Y;
  if (ok && ck >= 0) ok = acn_view(true, topo, bus, line, row_cols + 2 * (size_t)pos + 1, 0, ybus_ws + (size_t)g * nnzY, Y);
  else {
    Y.base = ybus_ws + (size_t)g * nnzY;
    Y.k[0] = -1;
#pragma unroll
    for (int u = 0; u < 4; ++u) { Y.p[u] = -1; Y.y[u] = make_double2(0.0, 0.0); }
  }
  if (!ok) {
    acn1_row_not_solved(o, row, N, E);
    return;
  }

  // W_g in generator-row order, as the DC generator screen sums it
  Acg1Pickup extra = {nullptr, 0.0, 0.0};
  if (pickup) {
    const double* w = pickup + (pickup_per_grid ? (size_t)g * Gn : 0);
    double W = 0.0;
    for (int h = 0; h < Gn; ++h)
      if (h != gi) W += w[h];
    extra = {w, (double)gen[gi * 7 + 6], W};
  }
  acn_solve_row(topo, bus, line, gen, g, row, Y, rating, rating_per_grid, v0, th0, max_iter, tol, o, extra);
}

// ---- the adjoint

// The generator part of a partial by ORIGINAL generator row, four doubles per generator: [Gn] dl/dvg, [Gn] dl/dPg, [Gn] dl/dw, and
// [Gn] the bus's lambda_P of each remaining unit in the row in hand (kept from unit() for lost(); the reduce kernel does not read it)
struct Acg1Partial {
  static constexpr int GEN = 4;
};

// acn_adjoint_row's hook for a row with generator row gi out: the pickup as the forward held it (w by generator row, not read when W
// is 0; pg = Pg_gi; W = W_gi, 0 where the slack picks up), whether the weights' gradient is asked for, and Gn.
struct Acg1Gen {
  const double* w;
  double pg, W;
  int gi, Gn;
  bool want_w;
  // a remaining unit h, on a bus whose lambda_P is mu (0 at the slack): dl/dPg_h = mu.  The lane of h's slot alone writes row h.
  __device__ __forceinline__ void unit(double* part_gen, const int h, const double mu) const {
    part_gen[Gn + h] += mu;
    if (W > 0.0) part_gen[3 * Gn + h] = mu;
  }
  // after every unit(): the lost unit's dl/dPg = M = sum_{h != gi} mu_h (w_h / W) in generator-row order, and dl/dw_h = pg (mu_h -
  // M) / W for h != gi; nothing where the slack picks up.  The same branch in every lane (W is the wave's); a lane per row.
  __device__ __forceinline__ void lost(double* part_gen) const {
    if (!(W > 0.0)) return;
    __threadfence_block();
    __syncthreads();                       // every unit()'s mu is written
    const double* mu = part_gen + 3 * Gn;
    double M = 0.0;
    for (int h = 0; h < Gn; ++h)
      if (h != gi) M += mu[h] * (w[h] / W);
    for (int h = threadIdx.x; h < Gn; h += PF_THREADS) {
      if (h == gi) part_gen[Gn + h] += M;
      else if (want_w) part_gen[2 * Gn + h] += pg * (mu[h] - M) / W;
    }
  }
};

// Rows of the list a wave of the adjoint walks: the N-2 adjoint's rule.  1 up to 64 rows (a wave per row), then ceil(n_row / 64):
// at most 64 partials per grid however long the list.  From the list's length alone, never the batch size.
constexpr int ACG1_CHUNKS = 64;
int acg1_chunk(const int n_row) {
  const int c = (n_row + ACG1_CHUNKS - 1) / ACG1_CHUNKS;
  return c < 1 ? 1 : c;
}

// The row kernel of the adjoint: workgroup blockIdx.x = grid * nchunks + chunk walks rows k0 .. k0 + C of the list in order, each lane
// adding into the addresses of the chunk's partial it alone owns (a bus, a line, a generator row per lane).  The row's blob, its view
// and W_g are gns_acg1_kernel's, expression for expression; every decision is the same in all lanes.
__global__ __launch_bounds__(PF_THREADS) void gns_acg1_adjoint_kernel(const int32_t* __restrict__ set, const int64_t set_words,
                                                                      const int32_t* __restrict__ member_off, const int n_member,
                                                                      const int N, const int E, const int Gn, const int64_t lds_bytes,
                                                                      const int nnzY, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const float* __restrict__ gens,
                                                                      const int32_t* __restrict__ gen_list,
                                                                      const int32_t* __restrict__ row_cols, const int K,
                                                                      const uint8_t* __restrict__ islanding,
                                                                      const double* __restrict__ rating, const int rating_per_grid,
                                                                      const double* __restrict__ pickup, const int pickup_per_grid,
                                                                      const double* __restrict__ v_in, const double* __restrict__ th_in,
                                                                      const uint8_t* __restrict__ conv_in,
                                                                      const int32_t* __restrict__ wl_in, const int32_t* __restrict__ lo_in,
                                                                      const int32_t* __restrict__ hi_in,
                                                                      const uint8_t* __restrict__ conv0, const Acn1Grad gr,
                                                                      const int want_w, const double2* __restrict__ ybus_ws, const int C,
                                                                      const int nchunks, const int np, double* __restrict__ partials) {
  const int lane = threadIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)nchunks), k0 = (int)(blockIdx.x % (unsigned)nchunks) * C;
  const int nk = min(C, K - k0);
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  double* part = partials + (size_t)blockIdx.x * np;

  for (int q = lane; q < np - 1; q += PF_THREADS) part[q] = 0.0;   // bus i's, line l's and generator h's doubles all sit at lane + 64 m
  bool solved_row = false;

  for (int j = 0; j < nk; ++j) {
    const int pos = k0 + j;
    const size_t row = (size_t)g * K + pos;
    // a row whose incoming gradients are all exactly zero or NULL is skipped, never multiplied by zero
    if (!acn1_row_nonzero(gr, row, N, E)) continue;

    // the row's blob, as in gns_acg1_kernel; a row without a solution (no base solution, an islanding row, a stopped or unconverged
    // iteration, a blob or a line that is refused): the grid's gradient is NaN
    const int cg = row_cols[2 * (size_t)pos], ck = row_cols[2 * (size_t)pos + 1];
    const int32_t* topo = set;
    int gi = -1;
    bool ok = cg >= 0 && cg < n_member && ck >= -1 && !islanding[pos] && conv0[g] != 0 && conv_in[row] != 0;
    if (ok) {
      ok = pf_set_member<PfBlobKind>(set, set_words, member_off[cg], N, E, Gn, lds_bytes, nnzY, topo) && topo[PH_NNZY] == nnzY;
      gi = gen_list[cg];
      ok = ok && gi >= 0 && gi < Gn;
    }
    AcnYbus<1> Y;
    if (ok && ck >= 0) ok = acn_view(true, topo, bus, line, row_cols + 2 * (size_t)pos + 1, 0, ybus_ws + (size_t)g * nnzY, Y);
    else {
      Y.base = ybus_ws + (size_t)g * nnzY;
      Y.k[0] = -1;
#pragma unroll
      for (int u = 0; u < 4; ++u) { Y.p[u] = -1; Y.y[u] = make_double2(0.0, 0.0); }
    }
    if (!ok) {
      acn1_partial_status(part, np, ACN1_PART_NAN);
      return;
    }

    // W_g in generator-row order, as the forward sums it
    Acg1Gen hook = {nullptr, 0.0, 0.0, gi, Gn, want_w != 0};
    if (pickup) {
      const double* w = pickup + (pickup_per_grid ? (size_t)g * Gn : 0);
      double W = 0.0;
      for (int h = 0; h < Gn; ++h)
        if (h != gi) W += w[h];
      hook.w = w; hook.pg = (double)gen[gi * 7 + 6]; hook.W = W;
    }
    if (!acn_adjoint_row(topo, line, row, Y, rt, gr, v_in, th_in, wl_in, lo_in, hi_in, part, hook)) {
      acn1_partial_status(part, np, ACN1_PART_NAN);
      return;
    }
    solved_row = true;
  }
  // a grid without a base solution whose chunk asked for nothing: zero rows when every chunk says so
  acn1_partial_status(part, np, !solved_row && conv0[g] == 0 ? ACN1_PART_UNSOLVED_ZERO : ACN1_PART_OK);
}

// A wave per grid: the chunks' partials summed in order, the contract applied, every element of the gradient rows written; vg, Pg
// and the weights by original generator row, a row per lane
__global__ __launch_bounds__(PF_THREADS) void gns_acg1_adjoint_reduce_kernel(const int N, const int E, const int Gn,
                                                                             const float* __restrict__ lines, const int nchunks,
                                                                             const int np, const double* __restrict__ partials,
                                                                             float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                             float* __restrict__ gg_out, double* __restrict__ gp_out) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const double* part = partials + (size_t)g * nchunks * np;

  bool bad, solved;
  acn1_reduce_status(part, nchunks, np, bad, solved);
  if (bad || !solved) {
    pf_adjoint_fill(g, N, E, Gn, bad ? __builtin_nanf("") : 0.0f, gb_out, gl_out, gg_out);
    if (gp_out) for (int h = lane; h < Gn; h += PF_THREADS) gp_out[(size_t)g * Gn + h] = bad ? __builtin_nan("") : 0.0;
    return;
  }
  if (gb_out) acn1_reduce_buses(g, N, nchunks, np, part, gb_out);
  if (gg_out || gp_out)
    for (int h = lane; h < Gn; h += PF_THREADS) {
      double dvg = 0.0, dpg = 0.0, dw = 0.0;
      for (int c = 0; c < nchunks; ++c) {
        const double* pg = part + (size_t)c * np + 4 * N + 5 * E;
        dvg += pg[h]; dpg += pg[Gn + h]; dw += pg[2 * Gn + h];
      }
      if (gg_out) {
        float* row = gg_out + ((size_t)g * Gn + h) * 7;
        row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f; row[3] = 0.0f;
        row[4] = (float)dvg;                   // vg
        row[5] = 0.0f;
        row[6] = (float)dpg;                   // Pg
      }
      if (gp_out) gp_out[(size_t)g * Gn + h] = dw;
    }
  if (gl_out) acn1_reduce_lines(g, N, E, lines + (size_t)g * E * 7, nchunks, np, part, gl_out);
}

// Whether the blob at h (its header checked) is an analysis without generator row g: its by-bus lists inside the blob, Gn - 1
// entries, none of them g
bool acg1_member_without(const int32_t* h, const int32_t g) {
  const int64_t N = h[PH_N], Gn = h[PH_GN], total = h[PH_TOTAL], gp = h[PH_GEN_PTR], gx = h[PH_GEN_IDX];
  if (gp < PF_HDR_WORDS || gp + N + 1 > total || gx < PF_HDR_WORDS || gx + (Gn > 1 ? Gn : 1) > total) return false;
  if (h[gp + N] != Gn - 1) return false;
  for (int64_t q = 0; q < Gn - 1; ++q)
    if (h[gx + q] == g) return false;
  return true;
}

// Whether the by-bus lists of the blob at h (acg1_member_without's checks passed) name generator rows alone: the adjoint writes
// its partial at them
bool acg1_member_rows_ok(const int32_t* h) {
  const int64_t Gn = h[PH_GN], gx = h[PH_GEN_IDX];
  for (int64_t q = 0; q < Gn - 1; ++q)
    if (h[gx + q] < 0 || h[gx + q] >= Gn) return false;
  return true;
}

// The members of a call's set: pf_scan_set's checks, and one nnz(Y) in all of them (they share the base Y-bus of a grid).
// GNS_OK, GNS_EINVAL, or GNS_EUNSUPPORTED with nnzy and lds written all the same.
int acg1_scan_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off, int32_t n_member,
                  int32_t* nnzy, int64_t* lds) {
  const int rc = pf_scan_set<PfBlobKind>(cfg, set_host, set_words, member_off, n_member, nnzy, lds);
  if (rc == GNS_EINVAL) return rc;
  const int32_t* set = static_cast<const int32_t*>(set_host);
  for (int32_t m = 0; m < n_member; ++m)
    if (set[member_off[m] + PH_NNZY] != *nnzy) return GNS_EINVAL;
  return rc;
}

}  // namespace

extern "C" int gns_acg1_workspace_bytes(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                                        int32_t n_member, int64_t Bt, int32_t n_row, size_t* bytes) {
  if (!bytes || Bt <= 0 || n_row <= 0) return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  if (acg1_scan_set(cfg, set_host, set_words, member_off, n_member, &nnzy, &lds) == GNS_EINVAL) return GNS_EINVAL;
  *bytes = pf_ws_bytes_nnzy(nnzy, Bt);
  return GNS_OK;
}

extern "C" int gns_acg1_screen(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                               const int32_t* member_off_host, const int32_t* member_off_dev, int32_t n_member,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* gen_host, const int32_t* gen_dev,
                               const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                               const double* base_v, const double* base_theta, const uint8_t* base_converged,
                               double* v, double* theta, double* p_from, double* q_from, double* p_to, double* q_to,
                               double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus, double* v_max,
                               int32_t* v_max_bus, uint8_t* converged, int32_t* iterations, double* mismatch,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!pf_config_ok(cfg) || !set_host || !set_dev || !member_off_host || !member_off_dev || n_member <= 0 || !buses || !lines ||
      !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !gen_host || !gen_dev || !row_cols_host || !row_cols_dev || n_row <= 0 ||
      !islanding || (rating_per_grid != 0 && rating_per_grid != 1) || (pickup_per_grid != 0 && pickup_per_grid != 1) || !base_v ||
      !base_theta || !base_converged || !worst_loading || !worst_line || !v_min || !v_min_bus || !v_max || !v_max_bus || !converged ||
      !iterations || !mismatch || !workspace)
    return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = acg1_scan_set(cfg, set_host, set_words, member_off_host, n_member, &nnzy, &lds);
  if (rc == GNS_EINVAL) return rc;
  // the generators: rows of the grid, ascending and distinct, each with its own analysis; the rows: positions into them, lines or -1
  const int32_t* set = static_cast<const int32_t*>(set_host);
  if (n_member > cfg->n_gen || !dcg1_list_ok(gen_host, n_member, cfg->n_gen)) return GNS_EINVAL;
  for (int32_t m = 0; m < n_member; ++m)
    if (!acg1_member_without(set + member_off_host[m], gen_host[m])) return GNS_EINVAL;
  for (int64_t p = 0; p < n_row; ++p) {
    const int32_t a = row_cols_host[2 * p], b = row_cols_host[2 * p + 1];
    if (a < 0 || a >= n_member || b < -1 || b >= cfg->n_line) return GNS_EINVAL;
  }
  int64_t rows = 0;
  if (!pf_chunks(n_row, 1, Bt, &rows)) return GNS_EINVAL;
  if (workspace_bytes < pf_ws_bytes_nnzy(nnzy, Bt)) return GNS_ESIZE;
  if (rc != GNS_OK) return rc;

  const Acn1Out out = {v, theta, p_from, q_from, p_to, q_to, worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus,
                       converged, iterations, mismatch};
  // the base Y-bus of every grid, once: the pattern and the stamps are the same words in every member, so the first serves
  const int32_t* sdev = static_cast<const int32_t*>(set_dev);
  const int rc0 = pf_launch<gns_acn1_ybus_kernel>(Bt, 0, stream, sdev + member_off_host[0], buses, lines, static_cast<double2*>(workspace));
  if (rc0 != GNS_OK) return rc0;
  return pf_launch<gns_acg1_kernel>(Bt * n_row, lds, stream, sdev, (int64_t)set_words, member_off_dev, (int)n_member, (int)cfg->n_bus,
                                    (int)cfg->n_line, (int)cfg->n_gen, lds, (int)nnzy, buses, lines, generators, gen_dev, row_cols_dev,
                                    (int)n_row, islanding, rating, (int)rating_per_grid, pickup, (int)pickup_per_grid, base_v,
                                    base_theta, base_converged, static_cast<const double2*>(workspace), cfg->max_iter, cfg->tol, out);
}

// The workspace of the adjoint: the base Y-bus of every grid, then a partial per (grid, chunk of acg1_chunk(n_row) rows of the list)
extern "C" int gns_acg1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* set_host, size_t set_words,
                                                const int32_t* member_off, int32_t n_member, int64_t Bt, int32_t n_row, size_t* bytes) {
  if (!bytes || Bt <= 0 || n_row <= 0) return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0, nchunks = 0;
  const int rc = acg1_scan_set(cfg, set_host, set_words, member_off, n_member, &nnzy, &lds);
  if (rc == GNS_EINVAL) return rc;
  if (!pf_chunks(n_row, acg1_chunk(n_row), Bt, &nchunks)) return GNS_EINVAL;
  if (rc != GNS_OK) return rc;
  const int32_t* first = static_cast<const int32_t*>(set_host) + member_off[0];
  *bytes = pf_ws_bytes_nnzy(nnzy, Bt) + acn1_adjoint_partial_bytes<Acg1Partial>(first, Bt, nchunks);
  return GNS_OK;
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.  Three launches: the base
// Y-bus of every grid from the first member's pattern, the row kernel (a workgroup per (grid, chunk)) with the largest member's
// LDS image, the sum of each grid's partials.
extern "C" int gns_acg1_adjoint(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                                const int32_t* member_off_host, const int32_t* member_off_dev, int32_t n_member,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* gen_host, const int32_t* gen_dev,
                                const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                                const double* v, const double* theta, const uint8_t* converged, const int32_t* worst_line,
                                const int32_t* v_min_bus, const int32_t* v_max_bus, const uint8_t* base_converged,
                                const double* grad_v, const double* grad_theta, const double* grad_p_from, const double* grad_q_from,
                                const double* grad_p_to, const double* grad_q_to, const double* grad_worst_loading,
                                const double* grad_v_min, const double* grad_v_max,
                                float* grad_buses, float* grad_lines, float* grad_generators, double* grad_pickup,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!pf_config_ok(cfg) || !set_host || !set_dev || !member_off_host || !member_off_dev || n_member <= 0 || !buses || !lines ||
      !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !gen_host || !gen_dev || !row_cols_host || !row_cols_dev || n_row <= 0 ||
      !islanding || (rating_per_grid != 0 && rating_per_grid != 1) || (pickup_per_grid != 0 && pickup_per_grid != 1) || !v || !theta ||
      !converged || !worst_line || !v_min_bus || !v_max_bus || !base_converged)
    return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = acg1_scan_set(cfg, set_host, set_words, member_off_host, n_member, &nnzy, &lds);
  if (rc == GNS_EINVAL) return rc;
  // the lists, as gns_acg1_screen checks them; the members' by-bus lists name generator rows
  const int32_t* set = static_cast<const int32_t*>(set_host);
  if (n_member > cfg->n_gen || !dcg1_list_ok(gen_host, n_member, cfg->n_gen)) return GNS_EINVAL;
  for (int32_t m = 0; m < n_member; ++m)
    if (!acg1_member_without(set + member_off_host[m], gen_host[m]) || !acg1_member_rows_ok(set + member_off_host[m])) return GNS_EINVAL;
  for (int64_t p = 0; p < n_row; ++p) {
    const int32_t a = row_cols_host[2 * p], b = row_cols_host[2 * p + 1];
    if (a < 0 || a >= n_member || b < -1 || b >= cfg->n_line) return GNS_EINVAL;
  }
  const int C = acg1_chunk(n_row);
  int64_t nchunks = 0;
  if (!pf_chunks(n_row, C, Bt, &nchunks)) return GNS_EINVAL;
  if (rc != GNS_OK) return rc;
  if (!grad_buses && !grad_lines && !grad_generators && !grad_pickup) return GNS_OK;
  if (!workspace) return GNS_EINVAL;
  const int32_t* first = set + member_off_host[0];
  const size_t ybytes = pf_ws_bytes_nnzy(nnzy, Bt);
  if (workspace_bytes < ybytes + acn1_adjoint_partial_bytes<Acg1Partial>(first, Bt, nchunks)) return GNS_ESIZE;

  const int np = (int)acn1_adjoint_partial<Acg1Partial>(first);
  const int32_t* sdev = static_cast<const int32_t*>(set_dev);
  double2* ybus = static_cast<double2*>(workspace);
  double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + ybytes);
  const Acn1Grad gr = {grad_v, grad_theta, grad_p_from, grad_q_from, grad_p_to, grad_q_to, grad_worst_loading, grad_v_min, grad_v_max};
  const int rc0 = pf_launch<gns_acn1_ybus_kernel>(Bt, 0, stream, sdev + member_off_host[0], buses, lines, ybus);
  if (rc0 != GNS_OK) return rc0;
  const int rc1 = pf_launch<gns_acg1_adjoint_kernel>(Bt * nchunks, lds, stream, sdev, (int64_t)set_words, member_off_dev, (int)n_member,
                                                     (int)cfg->n_bus, (int)cfg->n_line, (int)cfg->n_gen, lds, (int)nnzy, buses, lines,
                                                     generators, gen_dev, row_cols_dev, (int)n_row, islanding, rating,
                                                     (int)rating_per_grid, pickup, (int)pickup_per_grid, v, theta, converged, worst_line,
                                                     v_min_bus, v_max_bus, base_converged, gr, (int)(grad_pickup != nullptr),
                                                     (const double2*)ybus, C, (int)nchunks, np, partials);
  if (rc1 != GNS_OK) return rc1;
  return pf_launch<gns_acg1_adjoint_reduce_kernel>(Bt, 0, stream, (int)cfg->n_bus, (int)cfg->n_line, (int)cfg->n_gen, lines,
                                                   (int)nchunks, np, (const double*)partials, grad_buses, grad_lines, grad_generators,
                                                   grad_pickup);
}
