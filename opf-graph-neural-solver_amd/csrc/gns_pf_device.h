// What the power-flow kernels and their entry points share (gns_powerflow.hip: Newton-Raphson and its adjoint; gns_fdpf.hip:
// fast-decoupled).  Device: one wave per grid, the Y-bus of a grid from its line stamps, I = Y V, the pivot test, the interpreter of
// the blobs' op programs and the grid and member checks of a set kernel; and what every kind of kernel asks of a grid, AC or DC: the
// ends of a line, the bus of a generator slot, an entry of the CSR pattern, the fill of the three gradient rows.  Host: the checks of a call's
// arguments, of one blob and of a set of blobs, and the launch; for the contingency screens (gns_dcn1.hip, gns_dcn2.hip, gns_acn1.hip,
// gns_acn2.hip, gns_acg1.hip) the check of a list of lines, the chunk count of a launch and the body of their LDS queries.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"

namespace {

constexpr int PF_THREADS = 64;   // one wave

__device__ inline bool pf_finite(double x) { return __builtin_isfinite(x); }

__device__ inline double pf_wave_max(double x) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

// Stamp `kind` (0 ff, 1 tt, 2 ft, 3 tf) of line e as (Re, Im)
__device__ __forceinline__ double2 pf_stamp(const float* line, const int e, const int kind) {
  const double r = line[e * 7 + 2], x = line[e * 7 + 3], b = line[e * 7 + 4], tau = line[e * 7 + 5], sh = line[e * 7 + 6];
  const double den = r * r + x * x;
  const double ysr = r / den, ysi = -x / den;
  double ar, ai;
  if (kind == 0) { ar = ysr / (tau * tau); ai = (ysi + 0.5 * b) / (tau * tau); }
  else if (kind == 1) { ar = ysr; ai = ysi + 0.5 * b; }
  else {
    const double c = cos(sh), s = kind == 2 ? sin(sh) : -sin(sh);   // -y_s e^{+-j shift} / tau
    ar = -(ysr * c - ysi * s) / tau;
    ai = -(ysr * s + ysi * c) / tau;
  }
  return make_double2(ar, ai);
}

// Y-bus values of row i (makeYbus) into Y[y_ptr[i] .. y_ptr[i+1]): the line stamps of every entry, Gs + jBs on the diagonal
__device__ __forceinline__ void pf_ybus_row(const int i, const int32_t* y_ptr, const int32_t* y_diag, const int32_t* st_ptr,
                                            const int32_t* st, const float* bus, const float* line, double2* Y) {
  for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
    double yr = 0.0, yi = 0.0;
    if (p == y_diag[i]) { yr = (double)bus[i * 6 + 4]; yi = (double)bus[i * 6 + 5]; }
    for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
      const double2 a = pf_stamp(line, st[q] >> 2, st[q] & 3);
      yr += a.x; yi += a.y;
    }
    Y[p] = make_double2(yr, yi);
  }
}

// The 0-based ends of line e from its id columns (those the blob was prepared from); false unless both are buses of the grid
__device__ __forceinline__ bool pf_line_ends(const float* line, const int e, const int N, int& f, int& t) {
  const float ff = line[e * 7 + 0], ft = line[e * 7 + 1];
  f = (int)ff - 1; t = (int)ft - 1;
  return ff == (float)(f + 1) && ft == (float)(t + 1) && f >= 0 && f < N && t >= 0 && t < N;
}

// The bus of generator slot q of the blob's by-bus lists: gen_ptr[b] <= q < gen_ptr[b + 1]
__device__ __forceinline__ int pf_slot_bus(const int32_t* gen_ptr, const int N, const int q) {
  int b = 0, hi = N;
  while (hi - b > 1) {
    const int mid = (b + hi) >> 1;
    if (gen_ptr[mid] <= q) b = mid;
    else hi = mid;
  }
  return b;
}

// The Y-bus entry (i, k) of the blob's CSR pattern (columns ascending), -1 if it is not there
__device__ __forceinline__ int pf_find_entry(const int32_t* y_ptr, const int32_t* y_col, const int i, const int k) {
  int lo = y_ptr[i], hi = y_ptr[i + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (y_col[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo < y_ptr[i + 1] && y_col[lo] == k ? lo : -1;
}

// Every element of grid g's three gradient rows set to x
__device__ __forceinline__ void pf_adjoint_fill(const int g, const int N, const int E, const int Gn, const float x, float* gb_out,
                                                float* gl_out, float* gg_out) {
  const int lane = threadIdx.x;
  if (gb_out) for (int q = lane; q < N * 6; q += PF_THREADS) gb_out[(size_t)g * N * 6 + q] = x;
  if (gl_out) for (int q = lane; q < E * 7; q += PF_THREADS) gl_out[(size_t)g * E * 7 + q] = x;
  if (gg_out) for (int q = lane; q < Gn * 7; q += PF_THREADS) gg_out[(size_t)g * Gn * 7 + q] = x;
}

// I_i = sum_k Y_ik V_k over row i of the Y-bus, as (Re, Im)
__device__ __forceinline__ double2 pf_row_current(const int i, const int32_t* y_ptr, const int32_t* y_col, const double2* Y,
                                                  const double* Vr, const double* Vi) {
  double ir = 0.0, ii = 0.0;
  for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
    const int k = y_col[p];
    const double2 y = Y[p];
    ir += y.x * Vr[k] - y.y * Vi[k];
    ii += y.x * Vi[k] + y.y * Vr[k];
  }
  return make_double2(ir, ii);
}

// Whether one of this lane's pivots of a factor (F at the slots pivot[0 .. dim) names) is zero or not finite
__device__ __forceinline__ bool pf_bad_pivot(const int dim, const int32_t* pivot, const double* F, const int lane) {
  bool bad = false;
  for (int k = lane; k < dim; k += PF_THREADS) {
    const double pv = F[pivot[k]];
    bad |= pv == 0.0 || !pf_finite(pv);
  }
  return bad;
}

// One op program of the blob (PH_STEP_PTR / PH_OPS, or the transposed PH_T_*): F[dst] -= F[a] F[b] or F[dst] /= F[a],
// independent within a step, a barrier after each step
__device__ __forceinline__ void pf_run_program(const int nsteps, const int32_t* step_ptr, const int2* ops, double* F, const int lane) {
  for (int s = 0; s < nsteps; ++s) {
    const int q1 = step_ptr[s + 1];
    for (int q = step_ptr[s] + lane; q < q1; q += PF_THREADS) {
      const int2 op = ops[q];
      const int dst = op.x & 0xFFFF, a = (int)((uint32_t)op.x >> 16);
      if (op.y < 0) F[dst] = F[dst] / F[a];
      else F[dst] -= F[a] * F[op.y];
    }
    __syncthreads();
  }
}

// A set kernel's workgroup to its grid and blob, in two steps (the adjoint answers a zero incoming gradient between them).
// The grid of this workgroup: order ? order[w] : w.  The caller returns, writing nothing, unless it is a grid of the batch.
__device__ __forceinline__ int64_t pf_set_grid(const int32_t* order) {
  const int64_t w = blockIdx.x;
  return order ? (int64_t)order[w] : w;
}

// The blob of a grid whose grid_off is off, into topo.  False for a grid without a usable blob: off is -1, misaligned or outside
// the set, or not at a blob of this kind and shape that lies inside the set and whose Y-bus and LDS image fit the launch.  Nothing
// past the set's first header is read then: this is what keeps a bad offset from indexing outside the set.
template <class Kind>
__device__ __forceinline__ bool pf_set_member(const int32_t* set, const int64_t set_words, const int64_t off, const int N,
                                              const int E, const int Gn, const int64_t lds_bytes, const int nnzy_max,
                                              const int32_t*& topo) {
  bool ok = off >= 0 && off % PF_SET_ALIGN_WORDS == 0 && off + Kind::HDR_WORDS <= set_words;
  topo = set + (ok ? off : 0);
  if (ok) {
    ok = topo[PH_MAGIC] == Kind::MAGIC && topo[PH_N] == N && topo[PH_E] == E && topo[PH_GN] == Gn &&
         topo[PH_TOTAL] >= Kind::HDR_WORDS && topo[PH_TOTAL] <= set_words - off && topo[Kind::NNZY] >= 0 &&
         topo[Kind::NNZY] <= nnzy_max && Kind::lds_bytes(topo) <= lds_bytes;
  }
  return ok;
}

// Device workspace of Bt grids: their Y-bus values, 16 bytes per entry, rounded up to 256 bytes
inline size_t pf_ws_bytes_nnzy(int64_t nnzy, int64_t Bt) { return (((size_t)Bt * nnzy * sizeof(double2)) + 255) & ~(size_t)255; }

// ---- host: what the entry points (include/gns_powerflow.h) check before a launch.  shape is the gns_pf_config that holds
// n_bus, n_line and n_gen (a gns_fd_config's pf).

inline bool pf_config_ok(const gns_pf_config* cfg) { return cfg && cfg->max_iter >= 0 && cfg->tol >= 0.0; }

// The arguments of a solve call, but for its configuration and host blob(s): the device blob or set, the inputs, a batch one launch
// takes, a warm start with both parts or neither, every output, the workspace
inline bool pf_solve_args_ok(const void* blob_dev, const float* buses, const float* lines, const float* gens, int64_t Bt,
                             const double* v0, const double* theta0, const double* v, const double* theta, const uint8_t* converged,
                             const int32_t* iterations, const double* mismatch, const void* workspace) {
  return blob_dev && buses && lines && gens && Bt > 0 && Bt <= 0x7FFFFFFF && (v0 == nullptr) == (theta0 == nullptr) && v && theta &&
         converged && iterations && mismatch && workspace;
}

// The arguments of an adjoint call, but for its configuration and host blob(s).  Unlike a solve's, any of its outputs may be NULL.
inline bool pf_adjoint_args_ok(const void* blob_dev, const float* buses, const float* lines, const float* gens, int64_t Bt,
                               const double* v, const double* theta, const uint8_t* converged, const void* workspace) {
  return blob_dev && buses && lines && gens && Bt > 0 && Bt <= 0x7FFFFFFF && v && theta && converged && workspace;
}

template <class Kind>
bool pf_header_ok(const gns_pf_config* shape, const int32_t* h) {
  return h[PH_MAGIC] == Kind::MAGIC && h[PH_N] == shape->n_bus && h[PH_E] == shape->n_line && h[PH_GN] == shape->n_gen;
}

// Whether every one of the n indices at list is a line of the blob at h (an outage list, or a pair list as 2 P indices)
inline bool pf_lines_ok(const int32_t* h, const int32_t* list, int64_t n) {
  for (int64_t k = 0; k < n; ++k)
    if (list[k] < 0 || list[k] >= h[PH_E]) return false;
  return true;
}

// Whether the n entries of list are indices below bound, ascending and distinct (the candidate lists of the N-2 and the generator
// screen)
inline bool dcg1_list_ok(const int32_t* list, int32_t n, int32_t bound) {
  for (int32_t c = 0; c < n; ++c)
    if (list[c] < 0 || list[c] >= bound || (c > 0 && list[c] <= list[c - 1])) return false;
  return true;
}

// The chunks of `width` a list of n items is cut into; false when Bt grids of that many chunks are more workgroups than one launch
// takes (a workgroup per (grid, chunk))
inline bool pf_chunks(int64_t n, int64_t width, int64_t Bt, int64_t* nchunks) {
  *nchunks = (n + width - 1) / width;
  return Bt <= 0x7FFFFFFF / *nchunks;
}

// The body of a contingency screen's *_lds_bytes query on an FD blob: the chunk width lanes_of gives under the limit, and the LDS
// image bytes_of gives at that width
template <class Lanes, class Bytes>
int pf_fd_lds_query(const void* topo_host, int64_t* bytes, int32_t* lanes, Lanes lanes_of, Bytes bytes_of) {
  if (!topo_host || !bytes) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  const int w = lanes_of(h, GNS_PF_LDS_MAX_BYTES);
  *bytes = bytes_of(h, w);
  if (lanes) *lanes = w;
  return GNS_OK;
}

// Host check of a call on the one blob at h, in the order its codes win: GNS_EINVAL unless it is a blob of this kind and shape,
// GNS_ESIZE for a workspace that does not hold the Y-bus of Bt grids, GNS_EUNSUPPORTED for an LDS image above the limit.
template <class Kind>
int pf_check_topology(const gns_pf_config* shape, const int32_t* h, int64_t Bt, size_t workspace_bytes, int64_t* lds) {
  if (!pf_header_ok<Kind>(shape, h)) return GNS_EINVAL;
  if (workspace_bytes < pf_ws_bytes_nnzy(h[Kind::NNZY], Bt)) return GNS_ESIZE;
  *lds = Kind::lds_bytes(h);
  return *lds > GNS_PF_LDS_MAX_BYTES ? GNS_EUNSUPPORTED : GNS_OK;
}

// Host check of the members of a set: each at an aligned word offset with its whole blob inside set_words, a blob of this kind and
// shape.  Returns GNS_OK, GNS_EINVAL, or GNS_EUNSUPPORTED when a member's LDS image is too large (GNS_EINVAL wins over it whichever
// member comes first); unless it is GNS_EINVAL the largest nnz(Y) and LDS image are written.
template <class Kind>
int pf_scan_set(const gns_pf_config* shape, const void* set_host, size_t set_words, const int32_t* member_off, int32_t n_member,
                int32_t* nnzy_max, int64_t* lds_max) {
  if (!shape || !set_host || !member_off || n_member <= 0 || set_words > (size_t)INT32_MAX) return GNS_EINVAL;
  const int32_t* set = static_cast<const int32_t*>(set_host);
  int32_t ny = 0;
  int64_t lds = 0;
  bool too_big = false;
  for (int32_t m = 0; m < n_member; ++m) {
    const int64_t off = member_off[m];
    if (off < 0 || off % PF_SET_ALIGN_WORDS != 0 || off + Kind::HDR_WORDS > (int64_t)set_words) return GNS_EINVAL;
    const int32_t* h = set + off;
    if (!pf_header_ok<Kind>(shape, h) || h[PH_TOTAL] < Kind::HDR_WORDS || h[PH_TOTAL] > (int64_t)set_words - off || h[Kind::NNZY] < 0)
      return GNS_EINVAL;
    ny = h[Kind::NNZY] > ny ? h[Kind::NNZY] : ny;
    const int64_t b = Kind::lds_bytes(h);
    lds = b > lds ? b : lds;
    too_big |= b > GNS_PF_LDS_MAX_BYTES;
  }
  *nnzy_max = ny;
  *lds_max = lds;
  return too_big ? GNS_EUNSUPPORTED : GNS_OK;
}

// Launches Kernel with a workgroup per grid and lds_bytes of dynamic LDS.  Before the first launch the kernel's dynamic-LDS limit
// is raised to GNS_PF_LDS_MAX_BYTES, once per process, on the device that is current then.  The flag belongs to the instantiation
// (kernel and argument types): that is one per kernel only because each kernel is launched from one entry point; a second call
// site with other argument types would get a flag of its own.  State per device would change what a second device sees; it would
// be added here alone.
template <auto Kernel, class... Args>
int pf_launch(int64_t Bt, int64_t lds_bytes, void* stream, Args... args) {
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            GNS_PF_LDS_MAX_BYTES) != hipSuccess)
      return GNS_ELAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(Kernel, dim3((unsigned)Bt), dim3(PF_THREADS), (size_t)lds_bytes, (hipStream_t)stream, args...);
  return hipGetLastError() == hipSuccess ? GNS_OK : GNS_ELAUNCH;
}

}  // namespace
