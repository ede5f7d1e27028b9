// The AC line and bus arithmetic, written once for its consumers: Newton-Raphson and its adjoint (gns_powerflow.hip), the row
// skeleton of the AC screens and of their adjoints (gns_acn1_device.h, gns_acn_adjoint_device.h) and the solved case (gns_pfs.hip).
// The Jacobian row and dl/dvg on any Y-bus accessor (AcPlainYbus: the values as they lie in the workspace; AcnYbus<M>: a screen's
// view), the branch flows of a line on its own four stamps and its loading, the total order of the reductions and the voltage
// extremes, the flow terms, the worst-loading cotangent, the gather of the line-end cotangents to the buses, and the cotangent
// algebra of a line row.  The build has -ffp-contract=off, so one expression order gives every caller the same bits: the solved
// case equals newton_raphson's mismatch and the screens' rows bit for bit because it runs this code, not a copy of it.
#pragma once
#include "gns_pf_device.h"

namespace {

// The Y-bus values of a grid as an accessor, what a screen's view (AcnYbus<M>) is for a row with lines out
struct AcPlainYbus {
  const double2* base;
  __device__ __forceinline__ double2 at(const int p) const { return base[p]; }
};

// Row i (not the slack) of the Jacobian (MATPOWER dSbus_dV, polar) into its factor slots, at V = Vr + j Vi with I = Ir + j Ii = Y V
template <class YB>   // AcPlainYbus or an AcnYbus<M>
__device__ __forceinline__ void ac_jacobian_row(const int i, const int slack, const int32_t* y_ptr, const int32_t* y_col,
                                                const int32_t* jslot, const YB& Y, const double* Vm, const double* Vr,
                                                const double* Vi, const double* Ir, const double* Ii, double* F) {
  const double vri = Vr[i], vii = Vi[i];
  for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
    const int k = y_col[p];
    if (k == slack) continue;
    const double2 y = Y.at(p);
    const double a = y.x * Vr[k] - y.y * Vi[k], b = y.x * Vi[k] + y.y * Vr[k];   // Y_ik V_k
    const double cr = vri * a + vii * b, ci = vii * a - vri * b;                 // V_i conj(Y_ik V_k)
    double dar = ci, dai = -cr;                                                  // dS_i / dtheta_k
    double dmr = cr, dmi = ci;                                                   // |V_k| dS_i / d|V_k|
    if (k == i) {
      const double P = vri * Ir[i] + vii * Ii[i], Q = vii * Ir[i] - vri * Ii[i];
      dar -= Q; dai += P;
      dmr += P; dmi += Q;
    }
    dmr /= Vm[k]; dmi /= Vm[k];
    const int s0 = jslot[4 * p], s1 = jslot[4 * p + 1], s2 = jslot[4 * p + 2], s3 = jslot[4 * p + 3];
    if (s0 >= 0) F[s0] = dar;
    if (s1 >= 0) F[s1] = dmr;
    if (s2 >= 0) F[s2] = dai;
    if (s3 >= 0) F[s3] = dmi;
  }
}

// lambda^T dF/d|V_b| over column b of the Y-bus, what dl/dvg of the first unit of a PV / slack bus b subtracts.  (uc, us) is
// e^{j theta_b} as the caller has it: cos and sin of the angle in the solver's adjoint, Vr / Vm and Vi / Vm in a screen's row.
// Those are not the same bits, so the unit vector is an argument.
template <class YB>
__device__ __forceinline__ double ac_vg_column(const int b, const double uc, const double us, const int32_t* y_ptr,
                                               const int32_t* y_col, const YB& Y, const double* Vr, const double* Vi,
                                               const double* Ir, const double* Ii, const double* lamP, const double* lamQ) {
  double acc = 0.0;
  for (int p = y_ptr[b]; p < y_ptr[b + 1]; ++p) {
    const int k = y_col[p];
    const int r = pf_find_entry(y_ptr, y_col, k, b);   // Y_kb (the pattern is structurally symmetric)
    if (r < 0) continue;
    const double2 y = Y.at(r);
    const double wr = y.x * uc - y.y * us, wi = y.x * us + y.y * uc;   // Y_kb e^{j theta_b}
    double dr = Vr[k] * wr + Vi[k] * wi, di = Vi[k] * wr - Vr[k] * wi;  // dS_k / d|V_b| = V_k conj(Y_kb e^{j theta_b}) ...
    if (k == b) { dr += uc * Ir[b] + us * Ii[b]; di += us * Ir[b] - uc * Ii[b]; }   // ... + e^{j theta_b} conj(I_b) at k = b
    acc += lamP[k] * dr + lamQ[k] * di;
  }
  return acc;
}

// The branch flows of line l between buses a and b: S_f = V_f conj(Y_ff V_f + Y_ft V_t), S_t = V_t conj(Y_tf V_f + Y_tt V_t) on
// the line's own stamps
struct AcFlows {
  double pf, qf, pt, qt;
};

__device__ __forceinline__ AcFlows ac_line_flows(const float* line, const int l, const int a, const int b, const double* Vr,
                                                 const double* Vi) {
  const double2 yff = pf_stamp(line, l, 0), ytt = pf_stamp(line, l, 1), yft = pf_stamp(line, l, 2), ytf = pf_stamp(line, l, 3);
  const double far = Vr[a], fai = Vi[a], tor = Vr[b], toi = Vi[b];
  const double ifr = (yff.x * far - yff.y * fai) + (yft.x * tor - yft.y * toi);
  const double ifi = (yff.x * fai + yff.y * far) + (yft.x * toi + yft.y * tor);
  const double itr = (ytf.x * far - ytf.y * fai) + (ytt.x * tor - ytt.y * toi);
  const double iti = (ytf.x * fai + ytf.y * far) + (ytt.x * toi + ytt.y * tor);
  return {far * ifr + fai * ifi, fai * ifr - far * ifi, tor * itr + toi * iti, toi * itr - tor * iti};
}

// The loading of line l at those flows: the larger |S| of its two ends, NaN from either end, over its rating (rt NULL: |S| itself)
__device__ __forceinline__ double ac_loading(const AcFlows& s, const double* rt, const int l) {
  const double sf = sqrt(s.pf * s.pf + s.qf * s.qf), s_t = sqrt(s.pt * s.pt + s.qt * s.qt);
  const double m = sf != sf ? sf : s_t != s_t ? s_t : fmax(sf, s_t);
  return rt ? m / rt[l] : m;
}

// Whether v at index i comes before the best so far (at index bi): larger, or equal at a lower index; NaN comes before everything
__device__ __forceinline__ bool ac_before(const double v, const int i, const double best, const int bi) {
  if (v != v) return best == best || i < bi;
  if (best != best) return false;
  return v > best || (v == best && i < bi);
}

// The first of the wave's (best, bi) in ac_before's order, in every lane: a total order, so the tree's shape does not matter
__device__ __forceinline__ void ac_wave_first(double& best, int& bi) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ac_before(ov, oi, best, bi)) { best = ov; bi = oi; }
  }
}

// The voltage extremes of a grid, a bus per lane (the lowest of equal buses), in every lane after the wave reduction.  lo is
// -min|V|: the smallest |V| is the first in ac_before's order of the negated values.  per_bus(i, |V_i|) is the rest of the caller's
// loop over the buses (the store of a row's state, the injections of the solved case) and runs before bus i is compared.
struct AcExtremes {
  double lo, hi;
  int lo_i, hi_i;
};

template <class PerBus>
__device__ __forceinline__ AcExtremes ac_voltage_extremes(const int N, const double* Vm, const int lane, const PerBus& per_bus) {
  const double inf = __builtin_inf();
  double lo = -inf, hi = -inf;
  int lo_i = INT32_MAX, hi_i = INT32_MAX;
  for (int i = lane; i < N; i += PF_THREADS) {
    const double vm = Vm[i];
    per_bus(i, vm);
    if (ac_before(-vm, i, lo, lo_i)) { lo = -vm; lo_i = i; }
    if (ac_before(vm, i, hi, hi_i)) { hi = vm; hi_i = i; }
  }
  ac_wave_first(lo, lo_i);
  ac_wave_first(hi, hi_i);
  return {lo, hi, lo_i, hi_i};
}

// The four terms of the flows of line l between buses a and b at V: A = V_a conj(Y_ft V_b), D = |V_a|^2 conj(Y_ff) (S_f = D + A),
// B = V_b conj(Y_tf V_a), C = |V_b|^2 conj(Y_tt) (S_t = C + B), on the line's own stamps
__device__ __forceinline__ void ac_flow_terms(const float* line, const int l, const int a, const int b, const double* Vm,
                                              const double* Vr, const double* Vi, double2& A, double2& D, double2& B, double2& C) {
  const double2 yff = pf_stamp(line, l, 0), ytt = pf_stamp(line, l, 1), yft = pf_stamp(line, l, 2), ytf = pf_stamp(line, l, 3);
  const double far = Vr[a], fai = Vi[a], tor = Vr[b], toi = Vi[b];
  const double xr = yft.x * tor - yft.y * toi, xi = yft.x * toi + yft.y * tor;   // Y_ft V_t
  A = make_double2(far * xr + fai * xi, fai * xr - far * xi);
  const double zr = ytf.x * far - ytf.y * fai, zi = ytf.x * fai + ytf.y * far;   // Y_tf V_f
  B = make_double2(tor * zr + toi * zi, toi * zr - tor * zi);
  const double mf = Vm[a] * Vm[a], mt = Vm[b] * Vm[b];
  D = make_double2(mf * yff.x, 0.0 - mf * yff.y);
  C = make_double2(mt * ytt.x, 0.0 - mt * ytt.y);
}

// What grad_worst_loading gw adds to the line-end cotangents cot (its wf, wt and w): it goes to the end of line w that attains the
// maximum (the from end on equality) as S / |S| / rating, nothing at |S| = 0, nothing for a w that is no line with buses at its ends
template <class Cot>   // Acn1Cot<YB>, PfsCot
__device__ __forceinline__ void ac_worst_cot(Cot& cot, const double gw, const int w, const int N, const int E, const double* rt,
                                             const float* line, const double* Vm, const double* Vr, const double* Vi) {
  int wa = 0, wb = 0;
  if (gw != 0.0 && w >= 0 && w < E && pf_line_ends(line, w, N, wa, wb)) {
    double2 A, D, B, Cc;
    ac_flow_terms(line, w, wa, wb, Vm, Vr, Vi, A, D, B, Cc);
    const double pf = D.x + A.x, qf = D.y + A.y, pt = Cc.x + B.x, qt = Cc.y + B.y;
    const double sf = sqrt(pf * pf + qf * qf), s_t = sqrt(pt * pt + qt * qt);
    const double r = rt ? rt[w] : 1.0;
    double2 wf = cot.wf, wt = cot.wt;   // the choice is made on locals: a store to one of two members of cot keeps cot in scratch
    if (sf >= s_t) { if (sf > 0.0) wf = make_double2(gw * (pf / sf) / r, gw * (qf / sf) / r); }
    else wt = make_double2(gw * (pt / s_t) / r, gw * (qt / s_t) / r);
    cot.wf = wf; cot.wt = wt; cot.w = w;
  }
}

// What the line-end cotangents add to dl/dtheta_i and dl/d|V_i|: a gather.  Bus i walks the stamps of its diagonal entry, where kind 0
// names every line it is the from end of and kind 1 every line it is the to end of (a line from a bus to itself: once per end).
//   dS_f/dtheta_f = jA = -dS_f/dtheta_t,  dS_t/dtheta_t = jB = -dS_t/dtheta_f,
//   |V_f| dS_f/d|V_f| = 2D + A,  |V_t| dS_f/d|V_t| = A,  |V_t| dS_t/d|V_t| = 2C + B,  |V_f| dS_t/d|V_f| = B;  dl = Re(conj(W) dS)
// cot.at(l, a, b, Wf, Wt) gives the cotangents of line l between buses a and b.  The two early-outs only skip work.
template <class Cot>
__device__ __forceinline__ void ac_flow_cot_bus(const int i, const int N, const int32_t* y_diag, const int32_t* st_ptr,
                                                const int32_t* st, const float* line, const Cot& cot, const double* Vm,
                                                const double* Vr, const double* Vi, double& dth, double& dvm) {
  const int p = y_diag[i];
  for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
    const int e = st[q] >> 2, kind = st[q] & 3;
    if (kind > 1) continue;
    int a, b;
    if (!pf_line_ends(line, e, N, a, b)) continue;       // NaN flows: the line's own gradient row is NaN
    double2 Wf, Wt;
    cot.at(e, a, b, Wf, Wt);
    if (Wf.x == 0.0 && Wf.y == 0.0 && Wt.x == 0.0 && Wt.y == 0.0) continue;
    double2 A, D, B, C;
    ac_flow_terms(line, e, a, b, Vm, Vr, Vi, A, D, B, C);
    const double tf = Wf.y * A.x - Wf.x * A.y, tt = Wt.y * B.x - Wt.x * B.y;   // Re(conj(W_f) jA), Re(conj(W_t) jB)
    if (kind == 0) {
      dth += tf - tt;
      dvm += ((Wf.x * (2.0 * D.x + A.x) + Wf.y * (2.0 * D.y + A.y)) + (Wt.x * B.x + Wt.y * B.y)) / Vm[a];
    } else {
      dth += tt - tf;
      dvm += ((Wt.x * (2.0 * C.x + B.x) + Wt.y * (2.0 * C.y + B.y)) + (Wf.x * A.x + Wf.y * A.y)) / Vm[b];
    }
  }
}

// dl/d(r, x, b, tau, shift) of line e between buses f and t, over its four stamps, from the cotangents (lpf + j lqf) at its from
// end and (lpt + j lqt) at its to end: Lambda of the mismatches in the solver's adjoint, Lambda - W in a screen's row, -W in the
// solved case.  A real parameter that moves Y_ik by c moves S_i by V_i conj(V_k) conj(c), so dl/dp = Re(conj(c) G_ik) with
// G_ik = -V_i conj(V_k) conj(Lambda_i).  (0.0 - x rather than -x: an exact zero stays +0.)
struct AcLineCot {
  double r, x, b, tau, sh;
};

__device__ __forceinline__ AcLineCot ac_line_row_cot(const float* line, const int e, const int f, const int t, const double* Vm,
                                                     const double* Vr, const double* Vi, const double lpf, const double lqf,
                                                     const double lpt, const double lqt) {
  const double r = line[e * 7 + 2], x = line[e * 7 + 3], b = line[e * 7 + 4], tau = line[e * 7 + 5], sh = line[e * 7 + 6];
  const double den = r * r + x * x;
  const double ysr = r / den, ysi = -x / den, t2 = tau * tau;
  const double cs = cos(sh), sn = sin(sh);
  // G of the four entries: V_i conj(V_k) conj(Lambda_i), negated
  const double mf = Vm[f] * Vm[f], mt = Vm[t] * Vm[t];
  const double gffr = 0.0 - mf * lpf, gffi = mf * lqf;
  const double gttr = 0.0 - mt * lpt, gtti = mt * lqt;
  const double pr = Vr[f] * Vr[t] + Vi[f] * Vi[t], pi = Vi[f] * Vr[t] - Vr[f] * Vi[t];   // V_f conj(V_t)
  const double gftr = 0.0 - (pr * lpf + pi * lqf), gfti = 0.0 - (pi * lpf - pr * lqf);
  const double gtfr = 0.0 - (pr * lpt - pi * lqt), gtfi = 0.0 - (0.0 - pi * lpt - pr * lqt);
  // through y_s: Gamma = G_ff / tau^2 + G_tt - e^{-j shift} G_ft / tau - e^{j shift} G_tf / tau; dy_s/dr = -y_s^2, dy_s/dx = -j y_s^2
  const double gmr = gffr / t2 + gttr - ((cs * gftr + sn * gfti) + (cs * gtfr - sn * gtfi)) / tau;
  const double gmi = gffi / t2 + gtti - ((cs * gfti - sn * gftr) + (cs * gtfi + sn * gtfr)) / tau;
  const double y2r = ysr * ysr - ysi * ysi, y2i = 2.0 * ysr * ysi;
  const double qr = y2r * gmr + y2i * gmi, qi = y2r * gmi - y2i * gmr;   // conj(y_s^2) Gamma
  // the stamps A_ff = (y_s + jb/2) / tau^2, A_ft = -y_s e^{j shift} / tau, A_tf = -y_s e^{-j shift} / tau
  const double a0r = ysr / t2, a0i = (ysi + 0.5 * b) / t2;
  const double a2r = -(ysr * cs - ysi * sn) / tau, a2i = -(ysr * sn + ysi * cs) / tau;
  const double a3r = -(ysr * cs + ysi * sn) / tau, a3i = -(ysi * cs - ysr * sn) / tau;
  const double d_tau = 0.0 - (2.0 * (a0r * gffr + a0i * gffi) + (a2r * gftr + a2i * gfti) + (a3r * gtfr + a3i * gtfi)) / tau;
  const double d_sh = (a2r * gfti - a2i * gftr) - (a3r * gtfi - a3i * gtfr);
  return {0.0 - qr, 0.0 - qi, 0.5 * gffi / t2 + 0.5 * gtti, d_tau, d_sh};   // b: c = j/2 on Y_ff / tau^2 and Y_tt
}

}  // namespace
