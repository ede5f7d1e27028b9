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
// gns_acn1_kernel's loop is restated here rather than shared, as that kernel restates gns_pf_kernel's (gns_acn1.hip says why).
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
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const size_t row = blockIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)P), pi = (int)(blockIdx.x % (unsigned)P);
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], slack = topo[PH_SLACK], dim = topo[PH_DIM];
  const int nnzLU = topo[PH_NNZLU], nnzY = topo[PH_NNZY], nsteps = topo[PH_NSTEPS];
  const int32_t* role = topo + topo[PH_ROLE];
  const int32_t* th_idx = topo + topo[PH_TH_IDX];
  const int32_t* vm_idx = topo + topo[PH_VM_IDX];
  const int32_t* gen_ptr = topo + topo[PH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[PH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];
  const int32_t* jslot = topo + topo[PH_JSLOT];
  const int32_t* pivot = topo + topo[PH_PIVOT];
  const int32_t* step_ptr = topo + topo[PH_STEP_PTR];
  const int2* ops = reinterpret_cast<const int2*>(topo + topo[PH_OPS]);
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
  Y.y[0] = acn2_entry_without(fj, Y.p[0], j, k, y_diag, st_ptr, st, bus, line);
  Y.y[1] = acn2_entry_without(tj, Y.p[1], j, k, y_diag, st_ptr, st, bus, line);
  Y.y[2] = acn2_entry_without(fj, Y.p[2], j, k, y_diag, st_ptr, st, bus, line);
  Y.y[3] = acn2_entry_without(tj, Y.p[3], j, k, y_diag, st_ptr, st, bus, line);
  Y.y[4] = acn2_entry_without(fk, Y.p[4], j, k, y_diag, st_ptr, st, bus, line);
  Y.y[5] = acn2_entry_without(tk, Y.p[5], j, k, y_diag, st_ptr, st, bus, line);
  Y.y[6] = acn2_entry_without(fk, Y.p[6], j, k, y_diag, st_ptr, st, bus, line);
  Y.y[7] = acn2_entry_without(tk, Y.p[7], j, k, y_diag, st_ptr, st, bus, line);

  double* F = lds;                       // [nnzLU] factor, then [dim] right-hand side / Newton step: gns_acn1_kernel's image
  double* rhs = lds + nnzLU;
  double* Vm = rhs + dim;
  double* Va = Vm + N;
  double* Vr = Va + N;
  double* Vi = Vr + N;
  double* Ir = Vi + N;
  double* Ii = Ir + N;
  double* Psp = Ii + N;
  double* Qsp = Psp + N;

  // specified injections, bus roles and set points as in the base case; the warm start from the base solution
  for (int i = lane; i < N; i += PF_THREADS) {
    double pg = 0.0;
    for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) pg += (double)gen[gen_idx[q] * 7 + 6];
    Psp[i] = pg - (double)bus[i * 6 + 2];
    Qsp[i] = -(double)bus[i * 6 + 3];
    const int ro = role[i];
    double vm = 1.0, va = 0.0;
    if (ro != 0 && gen_ptr[i + 1] > gen_ptr[i]) vm = (double)gen[gen_idx[gen_ptr[i]] * 7 + 4];
    if (ro == 0) vm = v0[(size_t)g * N + i];
    if (ro != 2) va = th0[(size_t)g * N + i] - th0[(size_t)g * N + slack];
    Vm[i] = vm; Va[i] = va;
  }
  __syncthreads();

  int it = 0;
  bool conv = false;
  double mis = 0.0;
  for (;;) {
    for (int i = lane; i < N; i += PF_THREADS) { Vr[i] = Vm[i] * cos(Va[i]); Vi[i] = Vm[i] * sin(Va[i]); }
    __syncthreads();
    // mismatch F = [Re(V conj(YV)) - P ; Im(...) - Q] into the right-hand side, and its infinity norm
    double nrm = 0.0;
    bool bad = false;
    for (int i = lane; i < N; i += PF_THREADS) {
      double ir = 0.0, ii = 0.0;                 // I_i = sum_k Y_ik V_k: pf_row_current's sum on the pair's Y-bus
      for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
        const int c = y_col[p];
        const double2 y = Y.at(p);
        ir += y.x * Vr[c] - y.y * Vi[c];
        ii += y.x * Vi[c] + y.y * Vr[c];
      }
      Ir[i] = ir; Ii[i] = ii;
      if (th_idx[i] >= 0) {
        const double fp = (Vr[i] * ir + Vi[i] * ii) - Psp[i];
        rhs[th_idx[i]] = fp;
        nrm = fmax(nrm, fabs(fp));
        bad |= !pf_finite(fp);
      }
      if (vm_idx[i] >= 0) {
        const double fq = (Vi[i] * ir - Vr[i] * ii) - Qsp[i];
        rhs[vm_idx[i]] = fq;
        nrm = fmax(nrm, fabs(fq));
        bad |= !pf_finite(fq);
      }
    }
    nrm = pf_wave_max(nrm);
    if (__ballot(bad)) { mis = __builtin_nan(""); break; }
    mis = nrm;
    if (nrm < tol) { conv = true; break; }
    if (it >= max_iter) break;

    // Jacobian into its factor slots; fill slots, and the entries that lost their only lines, are zeros
    for (int s = lane; s < nnzLU; s += PF_THREADS) F[s] = 0.0;
    __syncthreads();
    for (int i = lane; i < N; i += PF_THREADS)
      if (i != slack) acn1_jacobian_row(i, slack, y_ptr, y_col, jslot, Y, Vm, Vr, Vi, Ir, Ii, F);
    __syncthreads();

    // the base topology's program: LU factorisation and both triangular solves
    pf_run_program(nsteps, step_ptr, ops, F, lane);

    // the update, only if every pivot is a finite non-zero and the new iterate is finite
    bad = pf_bad_pivot(dim, pivot, F, lane);
    for (int i = lane; i < N; i += PF_THREADS) {
      if (th_idx[i] >= 0) bad |= !pf_finite(Va[i] - rhs[th_idx[i]]);
      if (vm_idx[i] >= 0) bad |= !pf_finite(Vm[i] - rhs[vm_idx[i]]);
    }
    if (__ballot(bad)) break;
    for (int i = lane; i < N; i += PF_THREADS) {
      if (th_idx[i] >= 0) Va[i] -= rhs[th_idx[i]];
      if (vm_idx[i] >= 0) Vm[i] -= rhs[vm_idx[i]];
    }
    __syncthreads();
    ++it;
  }
  // every exit leaves Vr, Vi at the iterate Vm, Va hold: the state the flows and the summaries are computed from

  // the state and the voltage extremes, a bus per lane (the lowest of equal buses)
  const double inf = __builtin_inf();
  double lo = -inf, hi = -inf;             // lo holds -|V|: the smallest |V| is the first in acn1_before's order of the negated values
  int lo_i = INT32_MAX, hi_i = INT32_MAX;
  for (int i = lane; i < N; i += PF_THREADS) {
    const double vm = Vm[i];
    if (o.v) o.v[row * N + i] = vm;
    if (o.theta) o.theta[row * N + i] = Va[i];
    if (acn1_before(-vm, i, lo, lo_i)) { lo = -vm; lo_i = i; }
    if (acn1_before(vm, i, hi, hi_i)) { hi = vm; hi_i = i; }
  }
  acn1_wave_first(lo, lo_i);
  acn1_wave_first(hi, hi_i);

  // the branch flows, a line per lane: S_f = V_f conj(Y_ff V_f + Y_ft V_t), S_t = V_t conj(Y_tf V_f + Y_tt V_t) on the line's own
  // stamps; zeros at the two outaged lines; NaN at a line whose id columns are not buses of the grid
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  double best = -1.0;
  int bi = INT32_MAX;
  for (int l = lane; l < E; l += PF_THREADS) {
    double pf = 0.0, qf = 0.0, pt = 0.0, qt = 0.0;
    int a, b;
    if (!acn1_line_ends(line, l, N, a, b)) pf = qf = pt = qt = __builtin_nan("");
    else if (l != j && l != k) {
      const double2 yff = acn1_stamp(line, l, 0), ytt = acn1_stamp(line, l, 1), yft = acn1_stamp(line, l, 2), ytf = acn1_stamp(line, l, 3);
      const double far = Vr[a], fai = Vi[a], tor = Vr[b], toi = Vi[b];
      const double ifr = (yff.x * far - yff.y * fai) + (yft.x * tor - yft.y * toi);
      const double ifi = (yff.x * fai + yff.y * far) + (yft.x * toi + yft.y * tor);
      const double itr = (ytf.x * far - ytf.y * fai) + (ytt.x * tor - ytt.y * toi);
      const double iti = (ytf.x * fai + ytf.y * far) + (ytt.x * toi + ytt.y * tor);
      pf = far * ifr + fai * ifi; qf = fai * ifr - far * ifi;
      pt = tor * itr + toi * iti; qt = toi * itr - tor * iti;
    }
    if (o.p_from) o.p_from[row * E + l] = pf;
    if (o.q_from) o.q_from[row * E + l] = qf;
    if (o.p_to) o.p_to[row * E + l] = pt;
    if (o.q_to) o.q_to[row * E + l] = qt;
    const double sf = sqrt(pf * pf + qf * qf), s_t = sqrt(pt * pt + qt * qt);
    const double s = sf != sf ? sf : s_t != s_t ? s_t : fmax(sf, s_t);   // NaN from either end
    const double load = rt ? s / rt[l] : s;
    if (acn1_before(load, l, best, bi)) { best = load; bi = l; }
  }
  acn1_wave_first(best, bi);

  if (lane == 0) {
    o.worst[row] = best; o.worst_line[row] = bi;
    o.v_min[row] = -lo; o.v_min_bus[row] = lo_i;
    o.v_max[row] = hi; o.v_max_bus[row] = hi_i;
    o.conv[row] = conv ? 1 : 0; o.iters[row] = it; o.mis[row] = mis;
  }
}

}  // namespace

extern "C" int gns_acn2_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_pair, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_pair <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h)) return GNS_EINVAL;
  *bytes = pf_ws_bytes_nnzy(h[PH_NNZY], Bt);          // one base Y-bus per grid, whatever the number of pairs
  return GNS_OK;
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
  if (!pf_config_ok(cfg) || !topo_host || !topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF ||
      !pairs_host || !pairs_dev || n_pair <= 0 || !islanding || (rating_per_grid != 0 && rating_per_grid != 1) || !base_v ||
      !base_theta || !base_converged || !worst_loading || !worst_line || !v_min || !v_min_bus || !v_max || !v_max_bus || !converged ||
      !iterations || !mismatch || !workspace)
    return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h)) return GNS_EINVAL;
  for (int32_t p = 0; p < n_pair; ++p) {
    const int32_t j = pairs_host[2 * p], k = pairs_host[2 * p + 1];
    if (j < 0 || j >= h[PH_E] || k < 0 || k >= h[PH_E] || j == k) return GNS_EINVAL;
  }
  if (Bt > 0x7FFFFFFF / (int64_t)n_pair) return GNS_EINVAL;             // a workgroup per (grid, pair) in one launch
  int64_t lds = 0;
  const int rc = pf_check_topology<PfBlobKind>(cfg, h, Bt, workspace_bytes, &lds);
  if (rc != GNS_OK) return rc;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  double2* ybus = static_cast<double2*>(workspace);
  const int rc0 = pf_launch<gns_acn1_ybus_kernel>(Bt, 0, stream, topo, buses, lines, ybus);
  if (rc0 != GNS_OK) return rc0;
  const Acn1Out out = {v, theta, p_from, q_from, p_to, q_to, worst_loading, worst_line, v_min, v_min_bus, v_max, v_max_bus,
                       converged, iterations, mismatch};
  return pf_launch<gns_acn2_kernel>(Bt * n_pair, lds, stream, topo, buses, lines, generators, pairs_dev, (int)n_pair, islanding,
                                    rating, (int)rating_per_grid, base_v, base_theta, base_converged, (const double2*)ybus,
                                    cfg->max_iter, cfg->tol, out);
}
