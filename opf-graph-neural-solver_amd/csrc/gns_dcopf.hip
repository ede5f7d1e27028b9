// Batched DC optimal power flow (include/gns_powerflow.h, "DC optimal power flow") on the fast-decoupled blob: the cheapest dispatch
// within the units' bounds and the lines' ratings, with the multipliers and the locational marginal prices.  The problem is reduced
// to the dispatch p by generator shift factors: one solve z_g = A^-1 e_bus(g) per unit on the base factor gives the row
// S_g[l] = b_l (z_g[f_l] - z_g[t_l]), the flows are f0 + S p with f0 the flows without generation, and the one equality left is the
// balance sum p = sum (Pd + Gs).  A primal-dual interior point with PIPS's steps then works on a Gn x Gn normal matrix per grid.
//
// Three launches:
//   gns_dcopf_factor_kernel  a wave per (grid, chunk of W units) on the DC screens' image: the base case without generation, a lane
//                            per unit for its solve, S into the workspace as [E][Gn] per grid (a line's row contiguous: that is how
//                            the normal matrix reads it), f0, the units' finite flags and the grid's status
//   gns_dcopf_ipm_kernel     a wave per grid: the iteration, everything but S in LDS (dcopf_lds_bytes)
//   gns_dcopf_finish_kernel  a wave per grid on the DC image again: theta and the flows from the optimal injections in fp64, and the
//                            prices from one more solve on the symmetric factor
// No atomics, every sum in a fixed order (a lane's terms in index order, then the wave's xor tree).
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"
#include "gns_dcopf_device.h"

namespace {

constexpr double DCOPF_XI = 0.99995;     // fraction to the boundary
constexpr double DCOPF_SIGMA = 0.1;      // centring
constexpr double DCOPF_DELTA = 1e-14;    // the normal matrix's diagonal gets DELTA trace(M) / Gn
constexpr int DCOPF_TILE = 4;            // a lane forms DCOPF_TILE x DCOPF_TILE entries of the normal matrix at a time

// The largest image of the three kernels (the finish runs on the factor kernel's image at width 1)
int64_t dcopf_call_lds(const int32_t* h, int lanes) {
  const int64_t a = dcopf_factor_lds(h, lanes), b = dcopf_lds_bytes(h);
  return a > b ? a : b;
}

__device__ __forceinline__ double dcopf_wave_min(double x) {
  for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o));
  return x;
}

// ---- the factor kernel
__global__ __launch_bounds__(PF_THREADS) void gns_dcopf_factor_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const float* __restrict__ gens,
                                                                      const int Bt, const int W, const int nchunks,
                                                                      double* __restrict__ ws) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, Gn - k0);
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;
  const DcopfWorkspace w = dcopf_workspace(ws, Bt, Gn, E);
  const float* gen = gens + (size_t)g * Gn * 7;
  const float* zero = dcopf_zero_gens(m.Z + (size_t)d1 * ld, Gn, lane);

  if (!dcn1_base_case(topo, buses + (size_t)g * N * 6, lines + (size_t)g * E * 7, zero, m, lane)) {
    if (k0 == 0 && lane == 0) w.status[g] = 0.0;
    return;
  }

  // lane j: z = A^-1 e_bus on the base factor for unit k0 + j (nothing at the slack: its column of S is zero)
  bool fin = false;
  if (lane < nk) {
    const float fb = gen[(k0 + lane) * 7];
    const int bus = (int)fb - 1;
    if (fb == (float)(bus + 1) && bus >= 0 && bus < N) {
      double* zc = m.Z + lane;
      for (int s = 0; s < d1; ++s) zc[s * ld] = 0.0;
      if (p_idx[bus] >= 0) zc[p_idx[bus] * ld] = 1.0;
      dcn1_lane_solve(topo[FH_NOPS_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), m.F, nnz1, zc, ld);
      fin = true;
      for (int s = 0; s < d1; ++s) fin &= pf_finite(zc[s * ld]);
    }
  }
  __syncthreads();

  // the chunk's units in order, a line per lane: S_g[l] = b_l (z_g[f_l] - z_g[t_l]), z = 0 at the slack
  double* S = w.S + (size_t)g * E * Gn;
  for (int j = 0; j < nk; ++j) {
    const int ok = __shfl((int)fin, j);
    for (int l = lane; l < E; l += PF_THREADS) {
      const int2 en = m.ends[l];
      const double zf = en.x >= 0 ? m.Z[en.x * ld + j] : 0.0, zt = en.y >= 0 ? m.Z[en.y * ld + j] : 0.0;
      S[(size_t)l * Gn + k0 + j] = ok ? m.lb[l] * (zf - zt) : __builtin_nan("");
    }
    if (lane == 0) w.fin[(size_t)g * Gn + k0 + j] = ok ? 1.0 : 0.0;
  }
  if (k0 == 0) {
    for (int l = lane; l < E; l += PF_THREADS) w.f0[(size_t)g * E + l] = m.lF[l];
    if (lane == 0) w.status[g] = 1.0;
  }
}

// ---- the interior point

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

__global__ __launch_bounds__(PF_THREADS) void gns_dcopf_ipm_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                   const float* __restrict__ gens, const double* __restrict__ cost,
                                                                   const int cost_per_grid, const double* __restrict__ rating,
                                                                   const int rating_per_grid, const int Bt, const double tol,
                                                                   const int max_iter, double* __restrict__ ws,
                                                                   double* __restrict__ pg_out, double* __restrict__ mu_line_out,
                                                                   double* __restrict__ mu_pmax_out, double* __restrict__ mu_pmin_out,
                                                                   double* __restrict__ objective_out, uint8_t* __restrict__ conv_out,
                                                                   int32_t* __restrict__ iter_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const DcopfWorkspace w = dcopf_workspace(ws, Bt, Gn, E);
  const DcopfImage m = dcopf_image(lds, Gn, E);
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
    dcopf_not_solved(g, E, Gn, pg_out, mu_line_out, mu_pmax_out, mu_pmin_out, objective_out, conv_out, iter_out);
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
  for (int i = lane; i < N; i += PF_THREADS) dem += (double)bus[i * 6 + 2] + (double)bus[i * 6 + 4];
  s_lo = dcopf_wave_sum(s_lo); s_hi = dcopf_wave_sum(s_hi); dem = dcopf_wave_sum(dem);
  for (int o = 32; o > 0; o >>= 1) nlim += __shfl_xor(nlim, o);
  bad |= !(dem >= s_lo && dem <= s_hi);
  if (__ballot(bad)) {
    if (lane == 0) w.solved[g] = 0.0;
    dcopf_not_solved(g, E, Gn, pg_out, mu_line_out, mu_pmax_out, mu_pmin_out, objective_out, conv_out, iter_out);
    return;
  }
  const double n_ineq = 2.0 * nlim + 2.0 * Gn;
  __syncthreads();

  // ---- the start: the midpoint, z = max(1, -h), mu = gamma / z with gamma = 1, lambda = 0
  dcopf_apply_s(S, E, Gn, m.f0, m.x, m.fl, lane);
  for (int l = lane; l < E; l += PF_THREADS) {
    const bool lim = m.rt[l] < inf;
    const double hu = m.fl[l] - m.rt[l], hd = 0.0 - m.fl[l] - m.rt[l];
    const double zu = lim && 0.0 - hu > 1.0 ? 0.0 - hu : 1.0, zd = lim && 0.0 - hd > 1.0 ? 0.0 - hd : 1.0;
    m.zu[l] = zu; m.zd[l] = zd;
    m.mu[l] = lim ? 1.0 / zu : 0.0; m.md[l] = lim ? 1.0 / zd : 0.0;
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
    __syncthreads();

    // a unit per lane: L_x, the reduced gradient, the box rows' diagonal and the units' share of the figures
    double max_x = 0.0, max_lx = 0.0, sum_x = 0.0;
    for (int q = lane; q < Gn; q += PF_THREADS) {
      double a = 0.0, b = 0.0;
      for (int l = 0; l < E; ++l) {
        if (m.d[l] == 0.0) continue;
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

    // M = diag(2 c2 + the box rows) + S^T diag(d) S over the limited lines in order: a lane owns tiles of the lower triangle
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
  if (lane == 0) {
    objective_out[g] = obj;
    conv_out[g] = converged ? 1 : 0;
    iter_out[g] = it;
    w.lam[g] = lam;
    w.solved[g] = 1.0;
  }
}

// ---- the finish: theta and the flows at the returned dispatch as gns_dc_kernel defines them, the injections in fp64; then
// lmp = -lambda - A^-1 sum_l b_l mu_line_l (e_f - e_t) on the same factor (0 at the slack), a bus walking its diagonal's stamps
__global__ __launch_bounds__(PF_THREADS) void gns_dcopf_finish_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const int Bt,
                                                                      const double* __restrict__ ws, const double* __restrict__ pg,
                                                                      const double* __restrict__ mu_line, double* __restrict__ theta_out,
                                                                      double* __restrict__ flow_out, double* __restrict__ lmp_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int2* ops_s = reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]);
  const DcopfWorkspace w = dcopf_workspace(const_cast<double*>(ws), Bt, Gn, E);
  const Dcn1Image m = dcn1_image(topo, lds);
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const double* p = pg + (size_t)g * Gn;
  const double* ml = mu_line + (size_t)g * E;
  const float* zero = dcopf_zero_gens(m.Z + (size_t)d1 * 2, Gn, lane);

  if (w.status[g] == 0.0 || w.solved[g] == 0.0 || !dcn1_base_case(topo, bus, line, zero, m, lane)) {
    const double nan = __builtin_nan("");
    for (int i = lane; i < N; i += PF_THREADS) { theta_out[(size_t)g * N + i] = nan; lmp_out[(size_t)g * N + i] = nan; }
    for (int l = lane; l < E; l += PF_THREADS) flow_out[(size_t)g * E + l] = nan;
    return;
  }
  for (int i = lane; i < N; i += PF_THREADS) {
    if (p_idx[i] < 0) continue;
    double inj = dc_injection(i, y_diag, st_ptr, st, gen_ptr, gen_idx, bus, line, zero);
    for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) inj += p[gen_idx[q]];
    m.rhs[p_idx[i]] = inj;
  }
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, m.F, lane);
  for (int i = lane; i < N; i += PF_THREADS) {
    const double x = p_idx[i] >= 0 ? m.rhs[p_idx[i]] : 0.0;
    m.th[i] = x;
    theta_out[(size_t)g * N + i] = x;
  }
  __syncthreads();
  for (int e = lane; e < E; e += PF_THREADS) {
    int f, t;
    const bool ok = pf_line_ends(line, e, N, f, t);
    const double b = m.lb[e];
    flow_out[(size_t)g * E + e] = ok ? b * (m.th[f] - m.th[t]) + (0.0 - b * (double)line[e * 7 + 6]) : __builtin_nan("");
  }
  for (int i = lane; i < N; i += PF_THREADS) {
    if (p_idx[i] < 0) continue;
    double r = 0.0;
    const int d = y_diag[i];
    for (int q = st_ptr[d]; q < st_ptr[d + 1]; ++q) {
      const int e = st[q] >> 2, kind = st[q] & 3;
      if (kind >= 2) continue;
      const double x = m.lb[e] * ml[e];
      r += kind == 0 ? x : 0.0 - x;
    }
    m.rhs[p_idx[i]] = r;
  }
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, m.F, lane);
  const double lam = w.lam[g];
  for (int i = lane; i < N; i += PF_THREADS) lmp_out[(size_t)g * N + i] = 0.0 - lam - (p_idx[i] >= 0 ? m.rhs[p_idx[i]] : 0.0);
}

}  // namespace

int gns_dcopf_launch_factor(const int32_t* h, const void* topo_dev, const float* buses, const float* lines, const float* generators,
                            int64_t Bt, double* ws, void* stream) {
  const int lanes = dcopf_lanes(h);
  const int64_t nchunks = (h[FH_GN] + lanes - 1) / lanes;
  return pf_launch<gns_dcopf_factor_kernel>(Bt * nchunks, dcopf_factor_lds(h, lanes), stream, static_cast<const int32_t*>(topo_dev), buses,
                                            lines, generators, (int)Bt, lanes, (int)nchunks, ws);
}

extern "C" int gns_dcopf_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  if (!topo_host || !bytes) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  const int w = dcopf_lanes(h);
  *bytes = dcopf_call_lds(h, w);
  if (lanes) *lanes = w;
  return GNS_OK;
}

extern "C" int gns_dcopf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  *bytes = dcopf_ws_bytes(static_cast<const int32_t*>(topo_host), Bt);
  return GNS_OK;
}

extern "C" int gns_dcopf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const double* cost, int32_t cost_per_grid, const double* rating, int32_t rating_per_grid,
                               double* pg, double* theta, double* line_flow, double* lmp, double* mu_line, double* mu_pmax,
                               double* mu_pmin, double* objective, uint8_t* converged, int32_t* iterations,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cost || (cost_per_grid != 0 && cost_per_grid != 1) ||
      (rating_per_grid != 0 && rating_per_grid != 1) || !pg || !theta || !line_flow || !lmp || !mu_line || !mu_pmax || !mu_pmin ||
      !objective || !converged || !iterations || !workspace)
    return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const int lanes = dcopf_lanes(h);
  int64_t nchunks = 0;
  if (!pf_chunks(h[FH_GN], lanes, Bt, &nchunks)) return GNS_EINVAL;
  if (workspace_bytes < dcopf_ws_bytes(h, Bt)) return GNS_ESIZE;
  if (dcopf_call_lds(h, lanes) > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  double* ws = static_cast<double*>(workspace);
  int rl = gns_dcopf_launch_factor(h, topo_dev, buses, lines, generators, Bt, ws, stream);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcopf_ipm_kernel>(Bt, dcopf_lds_bytes(h), stream, topo, buses, generators, cost, (int)cost_per_grid, rating,
                                       (int)rating_per_grid, (int)Bt, cfg->tol, (int)cfg->max_iter, ws, pg, mu_line, mu_pmax, mu_pmin,
                                       objective, converged, iterations);
  if (rl != GNS_OK) return rl;
  return pf_launch<gns_dcopf_finish_kernel>(Bt, dcopf_factor_lds(h, 1), stream, topo, buses, lines, (int)Bt, (const double*)ws,
                                            (const double*)pg, (const double*)mu_line, theta, line_flow, lmp);
}
