// The hand-derived reverse of the line physics (global_active_compensation / local_power_imbalance, GNS/main.py:34-104), ONCE, for
// every backward kernel: the persistent kernel (gns_backward.hip), the split backward's phys and input-gradient kernels
// (gns_backward_split.hip) and the grid-per-workgroup backward (gns_gridwg_bwd.hip).  Plus the small helpers the grid-per-workgroup
// pair (gns_gridwg.hip, gns_gridwg_bwd.hip) shares.
//
// Everything here works on values: the kernels keep their own loads, LDS planes, slot layout and stores.  The library is built with
// -ffp-contract=off, so an expression tree IS its result: the trees below are the ones every copy carried, and must stay as they are.
//
// A line e = (s -> t) contributes, with the reference's bus-id-as-line-index quirk (y_s, tau_s, sh_s are gathered at LINE NUMBER s,
// y_t, tau_t, sh_t at line number t; dl = theta[a] - theta[b] and dl2 = theta[d] - theta[c] are the angle differences of those lines):
//   p_from = v_s v_t y_s / tau_s sin(angA) + (v_s / tau_s)^2 y_s sin(dl)                     -> dp[t]   (main.py:91,94)   adjoint Fb
//   p_to   = v_t v_s y_t / tau_t sin(angC) + v_t^2 y_t sin(dl2)                              -> dp[s]   (main.py:92,95)   adjoint Tb
//   |msg|  = |v_s v_t y_s / tau_s (sin(angA) + sin(angB)) + (v_s / tau_s^2 + v_t^2) y_s sin(dl)|  -> p_joule (main.py:41) adjoint pgbar
//   angA = th_s - th_t - dl - sh_s,  angB = th_t - th_s - dl + sh_s,  angC = th_t - th_s - dl2 - sh_t
#pragma once
#include "gns_device.h"

// ---- helpers of the grid-per-workgroup kernels -------------------------------------------------------------------------------
struct __attribute__((packed, aligned(4))) GwU4 { float x, y, z, w; };
struct __attribute__((packed, aligned(4))) GwU2 { float x, y; };
// four / two floats of the caller's tensors, which start at any dword
__device__ __forceinline__ f4 ld4(const float* p) { const GwU4 u = *reinterpret_cast<const GwU4*>(p); return f4{u.x, u.y, u.z, u.w}; }
__device__ __forceinline__ f2 ld2(const float* p) { const GwU2 u = *reinterpret_cast<const GwU2*>(p); return f2{u.x, u.y}; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// main.py:38: 1 / sqrt(r^2 + x^2), each op rounded like torch does
__device__ __forceinline__ float yof(float r, float x) {
  return __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(__fmul_rn(r, r), __fmul_rn(x, x))));
}

template <int NF>
__device__ __forceinline__ void read_row(const float* row, f2 (&dst)[NF / 2]) {
#pragma unroll
  for (int i = 0; i < NF / 2; ++i) dst[i] = reinterpret_cast<const f2*>(row)[i];
}
template <int NF>
__device__ __forceinline__ void write_row(float* row, const f2 (&src)[NF / 2]) {
#pragma unroll
  for (int i = 0; i < NF / 2; ++i) reinterpret_cast<f2*>(row)[i] = src[i];
}

// sin / cos on |x| <= pi/4 without range reduction (Cephes single-precision kernels, < 1 ulp); the caller votes
// wave-wide that every angle is in range and otherwise takes the library path.
__device__ __forceinline__ void sincos_small(float x, float& s, float& c) {
  const float z = x * x;
  const float ps = __builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
  s = __builtin_fmaf(ps * z, x, x);
  const float pc = __builtin_fmaf(__builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
  c = __builtin_fmaf(pc * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
}
__device__ __forceinline__ float sin_small(float x) {
  const float z = x * x;
  const float ps = __builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
  return __builtin_fmaf(ps * z, x, x);
}

// ---- 1. trig of a line --------------------------------------------------------------------------------------------------------
struct LineTrig { float sA, cA, sB, cB, sD, cD, sC, cC, sD2, cD2; };
// VOTE = false: the library's sincosf.  VOTE = true (grid-per-workgroup backward, where the angles of a converging solve are small):
// when every angle of the WAVE lies within pi/4 the range reduction is skipped; the vote keeps the branch wave-uniform.
template <bool VOTE>
__device__ __forceinline__ LineTrig line_trig(float ths, float tht, float tha, float thb, float thc, float thd, float shs, float sht) {
  const float dl = tha - thb, dl2 = thd - thc;
  const float angA = ths - tht - dl - shs, angB = tht - ths - dl + shs, angC = tht - ths - dl2 - sht;
  LineTrig T;
  if constexpr (VOTE) {
    const float amax = fmaxf(fmaxf(fmaxf(fabsf(angA), fabsf(angB)), fmaxf(fabsf(angC), fabsf(dl))), fabsf(dl2));
    if (__builtin_amdgcn_ballot_w64(!(amax <= 0.785f)) == 0) {     // every angle of the wave within pi/4: no range reduction
      sincos_small(angA, T.sA, T.cA); sincos_small(angB, T.sB, T.cB); sincos_small(dl, T.sD, T.cD);
      sincos_small(angC, T.sC, T.cC); sincos_small(dl2, T.sD2, T.cD2);
      return T;
    }
  }
  sincosf(angA, &T.sA, &T.cA);
  sincosf(angB, &T.sB, &T.cB);
  sincosf(dl, &T.sD, &T.cD);
  sincosf(angC, &T.sC, &T.cC);
  sincosf(dl2, &T.sD2, &T.cD2);
  return T;
}

// ---- the prologue the state and the parameter adjoints share --------------------------------------------------------------------
// Jb: adjoint of the signed argument of |msg| (pgbar = d total / d p_global: every line's joule term enters p_global, main.py:42-45)
struct LinePro { float yot, yot2, base, kJ, Jb, yot_t, base2; };
__device__ __forceinline__ LinePro line_prologue(const LineTrig& T, float vs, float vt, float ys, float taus, float yt, float taut, float pgbar) {
  LinePro Q;
  // "from" expressions: p_from (main.py:91) and |msg| of the joule loss (main.py:41)
  Q.yot = ys / taus; Q.yot2 = ys / (taus * taus);
  Q.base = vs * vt * Q.yot;
  Q.kJ = vs * Q.yot2 + vt * vt * ys;
  const float inner = Q.base * (T.sA + T.sB) + Q.kJ * T.sD;
  Q.Jb = pgbar * (inner > 0.f ? 1.f : (inner < 0.f ? -1.f : 0.f));
  // "to" expression: p_to (main.py:92)
  Q.yot_t = yt / taut;
  Q.base2 = vt * vs * Q.yot_t;
  return Q;
}

// ---- 2. state adjoint of a line -----------------------------------------------------------------------------------------------
// dvs, dvt: d/dv of the two ends;  dths, dtht: d/dtheta of the two ends (dtht == -dths bit for bit: Bb - Ab + Cb against
// Ab - Bb - Cb, so the lane-per-grid kernels store dths alone and their gather negates it);  dbar, dbar2: d/d(dl), d/d(dl2), which
// the gather hands to the four buses of the two angle differences with the signs of its incidence list.
struct LineAdj { float dvs, dvt, dths, dtht, dbar, dbar2; };
__device__ __forceinline__ LineAdj line_state_adjoint(const LineTrig& T, const LinePro& Q, float vs, float vt, float ys, float yt, float Fb, float Tb) {
  const float yot = Q.yot, yot2 = Q.yot2, base = Q.base, kJ = Q.kJ, Jb = Q.Jb, yot_t = Q.yot_t, base2 = Q.base2;
  float dvs = Fb * (vt * yot * T.sA + 2.f * vs * yot2 * T.sD) + Jb * (vt * yot * (T.sA + T.sB) + yot2 * T.sD);
  float dvt = Fb * (vs * yot * T.sA) + Jb * (vs * yot * (T.sA + T.sB) + 2.f * vt * ys * T.sD);
  const float Ab = (Fb + Jb) * base * T.cA, Bb = Jb * base * T.cB;
  const float dbar = Fb * (vs * vs * yot2) * T.cD + Jb * kJ * T.cD - Ab - Bb;
  float dths = Ab - Bb, dtht = Bb - Ab;
  dvt += Tb * (vs * yot_t * T.sC + 2.f * vt * yt * T.sD2);
  dvs += Tb * (vt * yot_t * T.sC);
  const float Cb = Tb * base2 * T.cC;
  const float dbar2 = Tb * vt * vt * yt * T.cD2 - Cb;
  dtht += Cb; dths -= Cb;
  return LineAdj{dvs, dvt, dths, dtht, dbar, dbar2};
}
__device__ __forceinline__ LineAdj line_state_adjoint(const LineTrig& T, float vs, float vt, float ys, float taus, float yt, float taut,
                                                      float Fb, float Tb, float pgbar) {
  return line_state_adjoint(T, line_prologue(T, vs, vt, ys, taus, yt, taut, pgbar), vs, vt, ys, yt, Fb, Tb);
}

// ---- 3. parameter adjoint of a line ---------------------------------------------------------------------------------------------
// d/d(y_s, tau_s, sh_s) of p_from and |msg|, d/d(y_t, tau_t, sh_t) of p_to: what the input gradients need
struct LineParAdj { float ybs, tbs, sbs, ybt, tbt, sbt; };
__device__ __forceinline__ LineParAdj line_param_adjoint(const LineTrig& T, const LinePro& Q, float vs, float vt, float taus, float taut, float Fb, float Tb) {
  const float yot2 = Q.yot2, base = Q.base, Jb = Q.Jb, base2 = Q.base2;
  LineParAdj R;
  R.ybs = Fb * (vs * vt / taus * T.sA + vs * vs / (taus * taus) * T.sD) + Jb * (vs * vt / taus * (T.sA + T.sB) + (vs / (taus * taus) + vt * vt) * T.sD);
  R.tbs = -(Fb * (base * T.sA + 2.f * vs * vs * yot2 * T.sD) + Jb * (base * (T.sA + T.sB) + 2.f * vs * yot2 * T.sD)) / taus;
  R.sbs = Jb * base * T.cB - (Fb + Jb) * base * T.cA;
  R.ybt = Tb * (vt * vs / taut * T.sC + vt * vt * T.sD2);
  R.tbt = -Tb * base2 * T.sC / taut;
  R.sbt = -Tb * base2 * T.cC;
  return R;
}
