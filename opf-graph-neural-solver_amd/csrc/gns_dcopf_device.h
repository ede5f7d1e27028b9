// What the DC optimal power flow (gns_dcopf.hip) and its adjoint (gns_dcopf_adjoint.hip) share: the workspace of a call as the
// factor kernel fills it, the generator block of zeros behind the screens' image, the factor kernel's chunk width and LDS image, the
// wave's sum, the host check of a call's blob, and the launches of the factor and the finish kernel, which live in gns_dcopf.hip.
// Then what gns_dcopf.hip shares with the security-constrained call (gns_dcscopf.hip): the interior point itself, dcopf_ipm.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dcn1_device.h"

// The factor kernel of gns_dcopf.hip on Bt grids of the blob (h on the host, topo_dev on the device) into the workspace ws, laid out
// by dcopf_workspace: S, f0, the units' finite flags and the grids' status.  The caller has checked the blob, Bt and the chunk count.
int gns_dcopf_launch_factor(const int32_t* h, const void* topo_dev, const float* buses, const float* lines, const float* generators,
                            int64_t Bt, double* ws, void* stream);

// The finish kernel of gns_dcopf.hip on the same workspace once the iteration has left lambda and the solved flags there: theta and
// line_flow at pg, and lmp = -lambda - A^-1 sum_l b_l mu_l (e_f - e_t) for the per-line multipliers mu [Bt][E] the caller hands over
int gns_dcopf_launch_finish(const int32_t* h, const void* topo_dev, const float* buses, const float* lines, int64_t Bt, const double* ws,
                            const double* pg, const double* mu, double* theta, double* line_flow, double* lmp, void* stream);

namespace {

// The workspace of one call, all doubles: S [Bt][E][Gn], f0 [Bt][E], the units' finite flags [Bt][Gn], the base case's status [Bt]
// (1: solved), then what the iteration leaves for the finish: lambda [Bt] and whether the grid has a dispatch [Bt]
struct DcopfWorkspace {
  double* S;
  double* f0;
  double* fin;
  double* status;
  double* lam;
  double* solved;
};

__host__ __device__ inline DcopfWorkspace dcopf_workspace(double* ws, const int64_t Bt, const int64_t Gn, const int64_t E) {
  DcopfWorkspace w;
  w.S = ws;
  w.f0 = w.S + Bt * E * Gn;
  w.fin = w.f0 + Bt * E;
  w.status = w.fin + Bt * Gn;
  w.lam = w.status + Bt;
  w.solved = w.lam + Bt;
  return w;
}

inline size_t dcopf_ws_bytes(const int32_t* h, int64_t Bt) {
  const int64_t E = h[FH_E], Gn = h[FH_GN];
  return ((size_t)Bt * (size_t)(E * Gn + E + Gn + 3) * sizeof(double) + 255) & ~(size_t)255;
}

// The factor and the finish kernel keep a generator block of zeros behind the screens' image (four doubles per unit hold its seven
// floats): the base case is the one without generation, whatever Pg the rows list
inline int64_t dcopf_zero_gens_bytes(const int32_t* h) { return 32 * (int64_t)h[FH_GN]; }

// Units a workgroup of the factor kernel takes side by side: dcn1_lanes on what the zeros leave
inline int dcopf_lanes(const int32_t* h) { return dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES - dcopf_zero_gens_bytes(h)); }

inline int64_t dcopf_factor_lds(const int32_t* h, int lanes) { return dcn1_lds_bytes(h, lanes) + dcopf_zero_gens_bytes(h); }

__device__ __forceinline__ double dcopf_wave_sum(double x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// The zeros a base case without generation reads as its generator rows
__device__ __forceinline__ const float* dcopf_zero_gens(double* at, const int Gn, const int lane) {
  float* z = reinterpret_cast<float*>(at);
  for (int q = lane; q < Gn * 7; q += PF_THREADS) z[q] = 0.0f;
  __syncthreads();
  return z;
}

// The host checks of a call on the blob at topo_host: GNS_EINVAL unless it is an FD blob of cfg's shape with a unit
inline int dcopf_check(const gns_pf_config* cfg, const void* topo_host) {
  if (!pf_config_ok(cfg) || !topo_host) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h) || h[FH_GN] <= 0) return GNS_EINVAL;
  return GNS_OK;
}

// ---- the interior point, shared by gns_dcopf_ipm_kernel (ROWS false) and the security-constrained gns_dcscopf_ipm_kernel (ROWS
// true): one body, so that with every row slot empty the second runs the first's arithmetic operation for operation

constexpr double DCOPF_XI = 0.99995;     // fraction to the boundary
constexpr double DCOPF_SIGMA = 0.1;      // centring
constexpr double DCOPF_DELTA = 1e-14;    // the normal matrix's diagonal gets DELTA trace(M) / Gn
constexpr int DCOPF_TILE = 4;            // a lane forms DCOPF_TILE x DCOPF_TILE entries of the normal matrix at a time

__device__ __forceinline__ double dcopf_wave_min(double x) {
  for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o));
  return x;
}

// The LDS image of the iteration (dcopf_lds_bytes)
struct DcopfImage {
  double* M;                                   // [Gn (Gn + 1) / 2] lower triangle by rows, then its Cholesky factor
  double *x, *q2, *c1, *pmin, *pmax;           // [Gn] the dispatch, 2 c2, c1 and the bounds
  double *zbu, *zbd, *mbu, *mbd;               // [Gn] slacks and multipliers of p <= Pmax (u) and p >= Pmin (d)
  double *Lx, *w, *u, *dx, *dg;                // [Gn] L_x, the two solves, the step, the box rows' diagonal
  double *f0, *rt, *fl;                        // [E] flows without generation, the rating, the flows
  double *zu, *zd, *mu, *md;                   // [E] slacks and multipliers of f <= rating (u) and -f <= rating (d)
  double *d, *va, *vb;                         // [E] the weights mu / z, and the two vectors S^T is applied to (then S dx)
};

__device__ __forceinline__ DcopfImage dcopf_image(double* lds, const int Gn, const int E) {
  DcopfImage m;
  m.M = lds;
  double* gv = m.M + (size_t)Gn * (Gn + 1) / 2;              // the fourteen unit vectors
  m.x = gv; m.q2 = gv + Gn; m.c1 = gv + 2 * Gn; m.pmin = gv + 3 * Gn; m.pmax = gv + 4 * Gn;
  m.zbu = gv + 5 * Gn; m.zbd = gv + 6 * Gn; m.mbu = gv + 7 * Gn; m.mbd = gv + 8 * Gn;
  m.Lx = gv + 9 * Gn; m.w = gv + 10 * Gn; m.u = gv + 11 * Gn; m.dx = gv + 12 * Gn; m.dg = gv + 13 * Gn;
  double* ev = gv + 14 * Gn;                                  // the ten line vectors
  m.f0 = ev; m.rt = ev + E; m.fl = ev + 2 * E; m.zu = ev + 3 * E; m.zd = ev + 4 * E;
  m.mu = ev + 5 * E; m.md = ev + 6 * E; m.d = ev + 7 * E; m.va = ev + 8 * E; m.vb = ev + 9 * E;
  return m;
}

// The contingency rows of one grid as the security-constrained call hands them to the iteration (ROWS true; unused otherwise), and
// their image behind DcopfImage's: ten doubles per slot and a flag per line.  The rows that are not empty sit at the front of the
// image's arrays in list order (the empty slots are left out once, after the data are read)
struct DcopfRows {
  int R;                       // slots
  const int32_t* ids;          // [R][2] (l, k) of the grid
  const double* rc;            // [E] the contingency rating of the grid, NULL: no line has one
  const double* L;             // [R] L_r from the row-factor kernel
  const double* st;            // [R] its status: DCSCOPF_ROW_EMPTY, _OK or _FAILED
  double* mu_row;              // [R] out: the upper multiplier minus the lower, 0 in an empty slot
  double* mu_eff;              // [E] out: what the finish's right-hand side takes per line
};

constexpr double DCSCOPF_ROW_EMPTY = 0.0, DCSCOPF_ROW_OK = 1.0, DCSCOPF_ROW_FAILED = 2.0;

struct DcopfRowImage {
  double *L, *rt;                              // [R] L_r and the monitored line's contingency rating
  double *zu, *zd, *mu, *md;                   // [R] slacks and multipliers of the two sides
  double *d, *va, *vb;                         // [R] the weight and the row's entries of the two vectors A_in^T takes
  int2* id;                                    // [R] (l, k)
  int32_t* tch;                                // [E] whether a row names the line: S^T must not skip it
};

__device__ __forceinline__ DcopfRowImage dcopf_row_image(double* at, const int R) {
  DcopfRowImage r;
  r.L = at; r.rt = at + R; r.zu = at + 2 * R; r.zd = at + 3 * R; r.mu = at + 4 * R; r.md = at + 5 * R;
  r.d = at + 6 * R; r.va = at + 7 * R; r.vb = at + 8 * R;
  r.id = reinterpret_cast<int2*>(at + 9 * R);
  r.tch = reinterpret_cast<int32_t*>(at + 10 * R);
  return r;
}

// The step of one inequality row with slack z, multiplier mu, value h and A dx = adx: dz = -h - z - A dx, dmu = -mu + (gamma - mu dz) / z
__device__ __forceinline__ void dcopf_row_step(const double h, const double z, const double mu, const double gamma, const double adx,
                                               double& dz, double& dmu) {
  dz = 0.0 - h - z - adx;
  dmu = (gamma - mu * dz) / z - mu;
}

// The largest steps that keep z and mu positive: min over dz < 0 of z / -dz, and likewise for mu
__device__ __forceinline__ void dcopf_row_ratio(const double z, const double mu, const double dz, const double dmu, double& rp, double& rd) {
  if (dz < 0.0) rp = fmin(rp, z / (0.0 - dz));
  if (dmu < 0.0) rd = fmin(rd, mu / (0.0 - dmu));
}

// Entry (i, j), j <= i, of the packed lower triangle
__device__ __forceinline__ int dcopf_tri(const int i, const int j) { return i * (i + 1) / 2 + j; }

// Cholesky of the packed lower triangle in place, a column at a time.  False (for the whole wave) at a pivot that is not positive
// or not finite.
__device__ __forceinline__ bool dcopf_cholesky(double* M, const int n, const int lane) {
  for (int k = 0; k < n; ++k) {
    const double p = M[dcopf_tri(k, k)];
    if (!(p > 0.0) || !pf_finite(p)) return false;
    const double s = sqrt(p);
    __syncthreads();
    for (int i = k + 1 + lane; i < n; i += PF_THREADS) M[dcopf_tri(i, k)] = M[dcopf_tri(i, k)] / s;
    if (lane == 0) M[dcopf_tri(k, k)] = s;
    __syncthreads();
    for (int i = k + 1 + lane; i < n; i += PF_THREADS) {      // a row per lane
      const double lik = M[dcopf_tri(i, k)];
      double* row = M + dcopf_tri(i, 0);
      for (int j = k + 1; j <= i; ++j) row[j] -= lik * M[dcopf_tri(j, k)];
    }
    __syncthreads();
  }
  return true;
}

// L L^T a = a and L L^T b = b in place
__device__ __forceinline__ void dcopf_solve2(const double* L, const int n, double* a, double* b, const int lane) {
  for (int k = 0; k < n; ++k) {
    const double lkk = L[dcopf_tri(k, k)];
    const double ak = a[k] / lkk, bk = b[k] / lkk;
    __syncthreads();
    if (lane == 0) { a[k] = ak; b[k] = bk; }
    for (int i = k + 1 + lane; i < n; i += PF_THREADS) {
      const double lik = L[dcopf_tri(i, k)];
      a[i] -= lik * ak;
      b[i] -= lik * bk;
    }
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {
    const double lkk = L[dcopf_tri(k, k)];
    const double ak = a[k] / lkk, bk = b[k] / lkk;
    __syncthreads();
    if (lane == 0) { a[k] = ak; b[k] = bk; }
    for (int i = lane; i < k; i += PF_THREADS) {
      const double lki = L[dcopf_tri(k, i)];
      a[i] -= lki * ak;
      b[i] -= lki * bk;
    }
    __syncthreads();
  }
}

// out[l] = base[l] + sum_g S[l][g] v[g], a line per lane, the units in order (base NULL: 0)
__device__ __forceinline__ void dcopf_apply_s(const double* __restrict__ S, const int E, const int Gn, const double* base, const double* v,
                                              double* out, const int lane) {
  for (int l = lane; l < E; l += PF_THREADS) {
    const double* row = S + (size_t)l * Gn;
    double s = base ? base[l] : 0.0;
    for (int q = 0; q < Gn; ++q) s += row[q] * v[q];
    out[l] = s;
  }
}

// A grid without a dispatch: NaN in its rows, iterations -1
__device__ __forceinline__ void dcopf_not_solved(const int g, const int E, const int Gn, double* pg, double* mu_line, double* mu_pmax,
                                                 double* mu_pmin, double* objective, uint8_t* converged, int32_t* iterations) {
  const double nan = __builtin_nan("");
  for (int q = threadIdx.x; q < Gn; q += PF_THREADS) {
    pg[(size_t)g * Gn + q] = nan;
    mu_pmax[(size_t)g * Gn + q] = nan;
    mu_pmin[(size_t)g * Gn + q] = nan;
  }
  for (int l = threadIdx.x; l < E; l += PF_THREADS) mu_line[(size_t)g * E + l] = nan;
  if (threadIdx.x == 0) { objective[g] = nan; converged[g] = 0; iterations[g] = -1; }
}

// The same with the rows' multipliers (NaN in every slot: the grid has none)
template <bool ROWS>
__device__ __forceinline__ void dcopf_refuse(const int g, const int E, const int Gn, const DcopfRows& rows, double* pg, double* mu_line,
                                             double* mu_pmax, double* mu_pmin, double* objective, uint8_t* converged,
                                             int32_t* iterations) {
  dcopf_not_solved(g, E, Gn, pg, mu_line, mu_pmax, mu_pmin, objective, converged, iterations);
  if constexpr (ROWS)
    for (int r = threadIdx.x; r < rows.R; r += PF_THREADS) rows.mu_row[r] = __builtin_nan("");
}

// Where the row of this lane goes in the image: behind the nR rows placed so far and the live rows of the lanes below it
__device__ __forceinline__ int dcopf_row_place(const int nR, const unsigned long long live, const int lane) {
  return nR + __popcll(live & ((1ull << lane) - 1ull));
}

// The value of row r = (l, k) on the line vector v: v[l] + L_r v[k]
__device__ __forceinline__ double dcopf_row_value(const DcopfRowImage& rm, const int r, const double* v) {
  const int2 id = rm.id[r];
  return v[id.x] + rm.L[r] * v[id.y];
}

// One grid's interior point on the factor kernel's workspace, the whole wave.  With ROWS the contingency rows join A_in after the
// line rows and before the box rows; every statement the rows add sits behind `if constexpr (ROWS)`.
template <bool ROWS>
__device__ __forceinline__ void dcopf_ipm(double* lds, const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                          const float* __restrict__ gens, const double* __restrict__ cost, const int cost_per_grid,
                                          const double* __restrict__ rating, const int rating_per_grid, const int Bt, const double tol,
                                          const int max_iter, double* __restrict__ ws, const DcopfRows rows,
                                          double* __restrict__ pg_out, double* __restrict__ mu_line_out,
                                          double* __restrict__ mu_pmax_out, double* __restrict__ mu_pmin_out,
                                          double* __restrict__ objective_out, uint8_t* __restrict__ conv_out,
                                          int32_t* __restrict__ iter_out) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const int R = ROWS ? rows.R : 0;
  const DcopfWorkspace w = dcopf_workspace(ws, Bt, Gn, E);
  const DcopfImage m = dcopf_image(lds, Gn, E);
  const DcopfRowImage rm = dcopf_row_image(m.vb + E, R);
  const double* __restrict__ S = w.S + (size_t)g * E * Gn;
  const float* bus = buses + (size_t)g * N * 6;
  const float* gen = gens + (size_t)g * Gn * 7;
  const double* cg = cost + (cost_per_grid ? (size_t)g * Gn * 2 : 0);
  const double* rt_in = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  const double inf = __builtin_inf();

  // ---- the data: refused unless the base case and every unit's solve are finite, the data are finite, Pmin < Pmax at every unit,
  // c2 >= 0, the ratings are positive and the demand lies within the units' range
  bool bad = w.status[g] == 0.0;
  if (bad) {                                     // (nothing else of the grid's workspace is written then)
    if (lane == 0) w.solved[g] = 0.0;
    dcopf_refuse<ROWS>(g, E, Gn, rows, pg_out, mu_line_out, mu_pmax_out, mu_pmin_out, objective_out, conv_out, iter_out);
    return;
  }
  double s_lo = 0.0, s_hi = 0.0, dem = 0.0;
  for (int q = lane; q < Gn; q += PF_THREADS) {
    const double pmax = gen[q * 7 + 1], pmin = gen[q * 7 + 2], c2 = cg[2 * q], c1 = cg[2 * q + 1];
    bad |= w.fin[(size_t)g * Gn + q] == 0.0 || !pf_finite(pmax) || !pf_finite(pmin) || !pf_finite(c2) || !pf_finite(c1) ||
           !(pmin < pmax) || c2 < 0.0;
    m.pmax[q] = pmax; m.pmin[q] = pmin; m.q2[q] = 2.0 * c2; m.c1[q] = c1;
    m.x[q] = 0.5 * (pmin + pmax);
    s_lo += pmin; s_hi += pmax;
  }
  int nlim = 0;
  for (int l = lane; l < E; l += PF_THREADS) {
    const double r = rt_in ? rt_in[l] : inf, f0 = w.f0[(size_t)g * E + l];
    bad |= !(r > 0.0) || !pf_finite(f0);
    m.rt[l] = r; m.f0[l] = f0;
    nlim += r < inf;
  }
  int nR = 0;                                    // the rows that are not empty: they sit side by side in the image, in list order
  if constexpr (ROWS) {
    // a row the row-factor kernel refused refuses the grid; the empty slots are left out here once, so that no loop of the
    // iteration walks them
    for (int r0 = 0; r0 < R; r0 += PF_THREADS) {
      const int r = r0 + lane;
      const double st = r < R ? rows.st[r] : DCSCOPF_ROW_EMPTY;
      bad |= st != DCSCOPF_ROW_EMPTY && st != DCSCOPF_ROW_OK;
      const unsigned long long live = __ballot(st == DCSCOPF_ROW_OK);
      if (st == DCSCOPF_ROW_OK) {
        const int at = dcopf_row_place(nR, live, lane);
        const int2 id = make_int2(rows.ids[2 * r], rows.ids[2 * r + 1]);
        const double rc = rows.rc[id.x];
        bad |= !(rc > 0.0) || !pf_finite(rows.L[r]);
        nlim += 1;
        rm.id[at] = id; rm.rt[at] = rc; rm.L[at] = rows.L[r];
      }
      nR += __popcll(live);
    }
  }
  for (int i = lane; i < N; i += PF_THREADS) dem += (double)bus[i * 6 + 2] + (double)bus[i * 6 + 4];
  s_lo = dcopf_wave_sum(s_lo); s_hi = dcopf_wave_sum(s_hi); dem = dcopf_wave_sum(dem);
  for (int o = 32; o > 0; o >>= 1) nlim += __shfl_xor(nlim, o);
  bad |= !(dem >= s_lo && dem <= s_hi);
  if (__ballot(bad)) {
    if (lane == 0) w.solved[g] = 0.0;
    dcopf_refuse<ROWS>(g, E, Gn, rows, pg_out, mu_line_out, mu_pmax_out, mu_pmin_out, objective_out, conv_out, iter_out);
    return;
  }
  const double n_ineq = 2.0 * nlim + 2.0 * Gn;
  __syncthreads();
  if constexpr (ROWS) {
    for (int l = lane; l < E; l += PF_THREADS) {
      int t = 0;
      for (int r = 0; r < nR; ++r) t |= rm.id[r].x == l || rm.id[r].y == l;
      rm.tch[l] = t;
    }
  }

  // ---- the start: the midpoint, z = max(1, -h), mu = gamma / z with gamma = 1, lambda = 0
  dcopf_apply_s(S, E, Gn, m.f0, m.x, m.fl, lane);
  for (int l = lane; l < E; l += PF_THREADS) {
    const bool lim = m.rt[l] < inf;
    const double hu = m.fl[l] - m.rt[l], hd = 0.0 - m.fl[l] - m.rt[l];
    const double zu = lim && 0.0 - hu > 1.0 ? 0.0 - hu : 1.0, zd = lim && 0.0 - hd > 1.0 ? 0.0 - hd : 1.0;
    m.zu[l] = zu; m.zd[l] = zd;
    m.mu[l] = lim ? 1.0 / zu : 0.0; m.md[l] = lim ? 1.0 / zd : 0.0;
  }
  if constexpr (ROWS) {
    __syncthreads();
    for (int r = lane; r < nR; r += PF_THREADS) {
      const double f = dcopf_row_value(rm, r, m.fl);
      const double hu = f - rm.rt[r], hd = 0.0 - f - rm.rt[r];
      const double zu = 0.0 - hu > 1.0 ? 0.0 - hu : 1.0, zd = 0.0 - hd > 1.0 ? 0.0 - hd : 1.0;
      rm.zu[r] = zu; rm.zd[r] = zd;
      rm.mu[r] = 1.0 / zu; rm.md[r] = 1.0 / zd;
    }
  }
  for (int q = lane; q < Gn; q += PF_THREADS) {
    const double hu = m.x[q] - m.pmax[q], hd = m.pmin[q] - m.x[q];
    const double zu = 0.0 - hu > 1.0 ? 0.0 - hu : 1.0, zd = 0.0 - hd > 1.0 ? 0.0 - hd : 1.0;
    m.zbu[q] = zu; m.zbd[q] = zd;
    m.mbu[q] = 1.0 / zu; m.mbd[q] = 1.0 / zd;
  }
  double gamma = 1.0, lam = 0.0;
  int it = 0;
  bool converged = false;
  __syncthreads();

  for (;; ++it) {
    // the flows, then per limited line the weights and the two vectors S^T takes; the lines' share of the termination figures
    dcopf_apply_s(S, E, Gn, m.f0, m.x, m.fl, lane);
    double max_h = -inf, max_z = 0.0, max_mu = 0.0, zmu = 0.0;
    for (int l = lane; l < E; l += PF_THREADS) {
      if (!(m.rt[l] < inf)) { m.d[l] = 0.0; m.va[l] = 0.0; m.vb[l] = 0.0; continue; }
      const double hu = m.fl[l] - m.rt[l], hd = 0.0 - m.fl[l] - m.rt[l];
      const double zu = m.zu[l], zd = m.zd[l], mu = m.mu[l], md = m.md[l];
      m.d[l] = mu / zu + md / zd;
      m.va[l] = mu - md;
      m.vb[l] = (gamma + mu * hu) / zu - (gamma + md * hd) / zd;
      max_h = fmax(max_h, fmax(hu, hd));
      max_z = fmax(max_z, fmax(zu, zd));
      max_mu = fmax(max_mu, fmax(mu, md));
      zmu += zu * mu + zd * md;
    }
    if constexpr (ROWS) {
      // the rows likewise, a slot per lane; then a line per lane gathers its rows' entries in list order: v_r at l, L_r v_r at k
      __syncthreads();
      for (int r = lane; r < nR; r += PF_THREADS) {
        const double f = dcopf_row_value(rm, r, m.fl);
        const double hu = f - rm.rt[r], hd = 0.0 - f - rm.rt[r];
        const double zu = rm.zu[r], zd = rm.zd[r], mu = rm.mu[r], md = rm.md[r];
        rm.d[r] = mu / zu + md / zd;
        rm.va[r] = mu - md;
        rm.vb[r] = (gamma + mu * hu) / zu - (gamma + md * hd) / zd;
        max_h = fmax(max_h, fmax(hu, hd));
        max_z = fmax(max_z, fmax(zu, zd));
        max_mu = fmax(max_mu, fmax(mu, md));
        zmu += zu * mu + zd * md;
      }
      __syncthreads();
      for (int l = lane; l < E; l += PF_THREADS) {
        if (!rm.tch[l]) continue;
        double a = m.va[l], b = m.vb[l];
        for (int r = 0; r < nR; ++r) {
          const int2 id = rm.id[r];
          if (id.x == l) { a += rm.va[r]; b += rm.vb[r]; }
          if (id.y == l) { a += rm.L[r] * rm.va[r]; b += rm.L[r] * rm.vb[r]; }
        }
        m.va[l] = a; m.vb[l] = b;
      }
    }
    __syncthreads();

    // a unit per lane: L_x, the reduced gradient, the box rows' diagonal and the units' share of the figures
    double max_x = 0.0, max_lx = 0.0, sum_x = 0.0;
    for (int q = lane; q < Gn; q += PF_THREADS) {
      double a = 0.0, b = 0.0;
      for (int l = 0; l < E; ++l) {
        if (m.d[l] == 0.0) {
          if constexpr (ROWS) { if (!rm.tch[l]) continue; }
          else continue;
        }
        const double s = S[(size_t)l * Gn + q];
        a += s * m.va[l];
        b += s * m.vb[l];
      }
      const double x = m.x[q], zu = m.zbu[q], zd = m.zbd[q], mu = m.mbu[q], md = m.mbd[q];
      const double hu = x - m.pmax[q], hd = m.pmin[q] - x;
      const double lx = m.q2[q] * x + m.c1[q] + lam + a + (mu - md);
      m.Lx[q] = lx;
      m.w[q] = 0.0 - (lx + b + ((gamma + mu * hu) / zu - (gamma + md * hd) / zd));
      m.u[q] = 1.0;
      m.dg[q] = m.q2[q] + mu / zu + md / zd;
      max_h = fmax(max_h, fmax(hu, hd));
      max_z = fmax(max_z, fmax(zu, zd));
      max_mu = fmax(max_mu, fmax(mu, md));
      zmu += zu * mu + zd * md;
      max_x = fmax(max_x, fabs(x));
      max_lx = fmax(max_lx, fabs(lx));
      sum_x += x;
    }
    max_h = pf_wave_max(max_h); max_z = pf_wave_max(max_z); max_mu = pf_wave_max(max_mu);
    max_x = pf_wave_max(max_x); max_lx = pf_wave_max(max_lx);
    zmu = dcopf_wave_sum(zmu); sum_x = dcopf_wave_sum(sum_x);
    const double gcon = sum_x - dem;
    const double feas = fmax(fabs(gcon), max_h) / (1.0 + fmax(max_x, max_z));
    const double grad = max_lx / (1.0 + fmax(fabs(lam), max_mu));
    const double comp = zmu / (1.0 + max_x);
    if (feas < tol && grad < tol && comp < tol) { converged = true; break; }
    if (it >= max_iter) break;

    // M = diag(2 c2 + the box rows) + S^T diag(d) S over the limited lines in order, then the rows' d_r a_r a_r^T in list order with
    // a_r = S[l] + L_r S[k]: a lane owns tiles of the lower triangle
    {
      const int nt = (Gn + DCOPF_TILE - 1) / DCOPF_TILE, ntiles = nt * (nt + 1) / 2;
      for (int t = lane; t < ntiles; t += PF_THREADS) {
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        const int tj = t - ti * (ti + 1) / 2;
        const int i0 = ti * DCOPF_TILE, j0 = tj * DCOPF_TILE;
        int ri[DCOPF_TILE], cj[DCOPF_TILE];
#pragma unroll
        for (int r = 0; r < DCOPF_TILE; ++r) { ri[r] = min(i0 + r, Gn - 1); cj[r] = min(j0 + r, Gn - 1); }
        double acc[DCOPF_TILE][DCOPF_TILE] = {};
        for (int l = 0; l < E; ++l) {
          const double d = m.d[l];
          if (d == 0.0) continue;
          const double* row = S + (size_t)l * Gn;
          double a[DCOPF_TILE], b[DCOPF_TILE];
#pragma unroll
          for (int r = 0; r < DCOPF_TILE; ++r) { a[r] = d * row[ri[r]]; b[r] = row[cj[r]]; }
#pragma unroll
          for (int r = 0; r < DCOPF_TILE; ++r)
#pragma unroll
            for (int c = 0; c < DCOPF_TILE; ++c) acc[r][c] += a[r] * b[c];
        }
        if constexpr (ROWS) {
          for (int s = 0; s < nR; ++s) {
            const int2 id = rm.id[s];
            const double d = rm.d[s], Lr = rm.L[s];
            const double* rl = S + (size_t)id.x * Gn;
            const double* rk = S + (size_t)id.y * Gn;
            double a[DCOPF_TILE], b[DCOPF_TILE];
#pragma unroll
            for (int r = 0; r < DCOPF_TILE; ++r) { a[r] = d * (rl[ri[r]] + Lr * rk[ri[r]]); b[r] = rl[cj[r]] + Lr * rk[cj[r]]; }
#pragma unroll
            for (int r = 0; r < DCOPF_TILE; ++r)
#pragma unroll
              for (int c = 0; c < DCOPF_TILE; ++c) acc[r][c] += a[r] * b[c];
          }
        }
#pragma unroll
        for (int r = 0; r < DCOPF_TILE; ++r)
#pragma unroll
          for (int c = 0; c < DCOPF_TILE; ++c) {
            const int i = i0 + r, j = j0 + c;
            if (i < Gn && j <= i) m.M[dcopf_tri(i, j)] = acc[r][c];
          }
      }
    }
    __syncthreads();
    double tr = 0.0;
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const double v = m.M[dcopf_tri(q, q)] + m.dg[q];
      m.M[dcopf_tri(q, q)] = v;
      tr += v;
    }
    tr = dcopf_wave_sum(tr);
    const double shift = DCOPF_DELTA * tr / (double)Gn;
    for (int q = lane; q < Gn; q += PF_THREADS) m.M[dcopf_tri(q, q)] += shift;
    __syncthreads();

    if (!dcopf_cholesky(m.M, Gn, lane)) break;
    dcopf_solve2(m.M, Gn, m.w, m.u, lane);

    // the equality's multiplier and the step in p
    double sw = 0.0, su = 0.0;
    for (int q = lane; q < Gn; q += PF_THREADS) { sw += m.w[q]; su += m.u[q]; }
    sw = dcopf_wave_sum(sw); su = dcopf_wave_sum(su);
    const double dlam = (sw + gcon) / su;
    bool nf = !pf_finite(dlam);
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const double dx = m.w[q] - dlam * m.u[q];
      m.dx[q] = dx;
      nf |= !pf_finite(dx);
    }
    __syncthreads();
    dcopf_apply_s(S, E, Gn, nullptr, m.dx, m.vb, lane);       // S dx
    if constexpr (ROWS) __syncthreads();

    // the step lengths
    double rp = inf, rd = inf;
    for (int l = lane; l < E; l += PF_THREADS) {
      if (!(m.rt[l] < inf)) continue;
      const double hu = m.fl[l] - m.rt[l], hd = 0.0 - m.fl[l] - m.rt[l], sdx = m.vb[l];
      double dz, dmu;
      dcopf_row_step(hu, m.zu[l], m.mu[l], gamma, sdx, dz, dmu);
      dcopf_row_ratio(m.zu[l], m.mu[l], dz, dmu, rp, rd);
      nf |= !pf_finite(dz) || !pf_finite(dmu);
      dcopf_row_step(hd, m.zd[l], m.md[l], gamma, 0.0 - sdx, dz, dmu);
      dcopf_row_ratio(m.zd[l], m.md[l], dz, dmu, rp, rd);
      nf |= !pf_finite(dz) || !pf_finite(dmu);
    }
    if constexpr (ROWS) {
      for (int r = lane; r < nR; r += PF_THREADS) {
        const double f = dcopf_row_value(rm, r, m.fl), sdx = dcopf_row_value(rm, r, m.vb);
        const double hu = f - rm.rt[r], hd = 0.0 - f - rm.rt[r];
        double dz, dmu;
        dcopf_row_step(hu, rm.zu[r], rm.mu[r], gamma, sdx, dz, dmu);
        dcopf_row_ratio(rm.zu[r], rm.mu[r], dz, dmu, rp, rd);
        nf |= !pf_finite(dz) || !pf_finite(dmu);
        dcopf_row_step(hd, rm.zd[r], rm.md[r], gamma, 0.0 - sdx, dz, dmu);
        dcopf_row_ratio(rm.zd[r], rm.md[r], dz, dmu, rp, rd);
        nf |= !pf_finite(dz) || !pf_finite(dmu);
      }
    }
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const double x = m.x[q], dx = m.dx[q];
      double dz, dmu;
      dcopf_row_step(x - m.pmax[q], m.zbu[q], m.mbu[q], gamma, dx, dz, dmu);
      dcopf_row_ratio(m.zbu[q], m.mbu[q], dz, dmu, rp, rd);
      nf |= !pf_finite(dz) || !pf_finite(dmu);
      dcopf_row_step(m.pmin[q] - x, m.zbd[q], m.mbd[q], gamma, 0.0 - dx, dz, dmu);
      dcopf_row_ratio(m.zbd[q], m.mbd[q], dz, dmu, rp, rd);
      nf |= !pf_finite(dz) || !pf_finite(dmu);
    }
    if (__ballot(nf)) break;                                  // a step that is not finite: the last iterate stays
    rp = dcopf_wave_min(rp); rd = dcopf_wave_min(rd);
    const double ap = fmin(DCOPF_XI * rp, 1.0), ad = fmin(DCOPF_XI * rd, 1.0);

    // the update, and gamma from the new z . mu
    double zm = 0.0;
    for (int l = lane; l < E; l += PF_THREADS) {
      if (!(m.rt[l] < inf)) continue;
      const double hu = m.fl[l] - m.rt[l], hd = 0.0 - m.fl[l] - m.rt[l], sdx = m.vb[l];
      double dz, dmu;
      dcopf_row_step(hu, m.zu[l], m.mu[l], gamma, sdx, dz, dmu);
      m.zu[l] += ap * dz; m.mu[l] += ad * dmu;
      dcopf_row_step(hd, m.zd[l], m.md[l], gamma, 0.0 - sdx, dz, dmu);
      m.zd[l] += ap * dz; m.md[l] += ad * dmu;
      zm += m.zu[l] * m.mu[l] + m.zd[l] * m.md[l];
    }
    if constexpr (ROWS) {
      for (int r = lane; r < nR; r += PF_THREADS) {
        const double f = dcopf_row_value(rm, r, m.fl), sdx = dcopf_row_value(rm, r, m.vb);
        const double hu = f - rm.rt[r], hd = 0.0 - f - rm.rt[r];
        double dz, dmu;
        dcopf_row_step(hu, rm.zu[r], rm.mu[r], gamma, sdx, dz, dmu);
        rm.zu[r] += ap * dz; rm.mu[r] += ad * dmu;
        dcopf_row_step(hd, rm.zd[r], rm.md[r], gamma, 0.0 - sdx, dz, dmu);
        rm.zd[r] += ap * dz; rm.md[r] += ad * dmu;
        zm += rm.zu[r] * rm.mu[r] + rm.zd[r] * rm.md[r];
      }
    }
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const double x = m.x[q], dx = m.dx[q];
      double dz, dmu;
      dcopf_row_step(x - m.pmax[q], m.zbu[q], m.mbu[q], gamma, dx, dz, dmu);
      m.zbu[q] += ap * dz; m.mbu[q] += ad * dmu;
      dcopf_row_step(m.pmin[q] - x, m.zbd[q], m.mbd[q], gamma, 0.0 - dx, dz, dmu);
      m.zbd[q] += ap * dz; m.mbd[q] += ad * dmu;
      m.x[q] = x + ap * dx;
      zm += m.zbu[q] * m.mbu[q] + m.zbd[q] * m.mbd[q];
    }
    lam += ad * dlam;
    gamma = DCOPF_SIGMA * dcopf_wave_sum(zm) / n_ineq;
    __syncthreads();
  }

  // ---- the last iterate: the dispatch, the multipliers, the cost; lambda and the flag for the finish
  double obj = 0.0;
  for (int q = lane; q < Gn; q += PF_THREADS) {
    const double x = m.x[q];
    pg_out[(size_t)g * Gn + q] = x;
    mu_pmax_out[(size_t)g * Gn + q] = m.mbu[q];
    mu_pmin_out[(size_t)g * Gn + q] = m.mbd[q];
    obj += (0.5 * m.q2[q] * x + m.c1[q]) * x;
  }
  obj = dcopf_wave_sum(obj);
  for (int l = lane; l < E; l += PF_THREADS) mu_line_out[(size_t)g * E + l] = m.rt[l] < inf ? m.mu[l] - m.md[l] : 0.0;
  if constexpr (ROWS) {
    // the rows' multipliers, and per line what the finish's right-hand side takes: mu_line_l + sum_r mu_r at l, L_r mu_r at k
    int done = 0;
    for (int r0 = 0; r0 < R; r0 += PF_THREADS) {                // (the data phase's walk again: slot r's row is at its place)
      const int r = r0 + lane;
      const bool is = r < R && rows.st[r] == DCSCOPF_ROW_OK;
      const unsigned long long live = __ballot(is);
      const int at = dcopf_row_place(done, live, lane);
      if (r < R) rows.mu_row[r] = is ? rm.mu[at] - rm.md[at] : 0.0;
      done += __popcll(live);
    }
    for (int l = lane; l < E; l += PF_THREADS) {
      double v = m.rt[l] < inf ? m.mu[l] - m.md[l] : 0.0;
      if (rm.tch[l])
        for (int r = 0; r < nR; ++r) {
          const int2 id = rm.id[r];
          if (id.x == l) v += rm.mu[r] - rm.md[r];
          if (id.y == l) v += rm.L[r] * (rm.mu[r] - rm.md[r]);
        }
      rows.mu_eff[l] = v;
    }
  }
  if (lane == 0) {
    objective_out[g] = obj;
    conv_out[g] = converged ? 1 : 0;
    iter_out[g] = it;
    w.lam[g] = lam;
    w.solved[g] = 1.0;
  }
}

}  // namespace
