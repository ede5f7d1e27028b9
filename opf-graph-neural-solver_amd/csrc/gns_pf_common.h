// Layout of the power-flow topology blob (include/gns_powerflow.h): a header of PF_HDR_WORDS int32 words, then int32 arrays at
// the word offsets the header names.  Written by gns_pf_topology.cpp, read by gns_powerflow.hip.
#pragma once
#include <stdint.h>

#define GNS_PF_MAGIC 0x47504631   // "GPF1"

enum {
  PH_MAGIC = 0, PH_TOTAL, PH_N, PH_E, PH_GN, PH_SLACK, PH_NPV, PH_NPQ, PH_DIM, PH_NNZJ, PH_NNZLU, PH_NNZY, PH_NOPS, PH_NSTEPS,
  // word offsets of the arrays
  PH_ROLE,       // [N]      0 PQ, 1 PV, 2 slack
  PH_TH_IDX,     // [N]      position of the bus's theta unknown in the ordered system, -1 at the slack
  PH_VM_IDX,     // [N]      position of its |V| unknown, -1 unless PQ
  PH_GEN_PTR,    // [N+1]    generators of each bus ...
  PH_GEN_IDX,    // [max(Gn,1)] ... in listing order
  PH_Y_PTR,      // [N+1]    Y-bus rows (CSR, columns ascending, diagonal included)
  PH_Y_COL,      // [nnzY]
  PH_Y_DIAG,     // [N]      entry of the diagonal of each row
  PH_ST_PTR,     // [nnzY+1] stamps adding into each entry ...
  PH_ST,         // [4E]     ... as line * 4 + kind (0 ff, 1 tt, 2 ft, 3 tf), in line order
  PH_JSLOT,      // [4 nnzY] factor slot of (dP/dtheta_k, dP/d|V|_k, dQ/dtheta_k, dQ/d|V|_k) of entry (i, k), -1 if not in J
  PH_PIVOT,      // [dim]    factor slot of each pivot
  PH_STEP_PTR,   // [nsteps+1] operations of each step ...
  PH_OPS,        // [2 nops] ... as (dst | a << 16, b): F[dst] -= F[a] * F[b], or F[dst] /= F[a] when b == -1 (8-byte aligned)
  // the transposed-solve program of the adjoint (gns_pf_adjoint): J^T x = rhs on the factor PH_OPS leaves in the slots, as U^T y = rhs
  // then L^T x = y, in the format and schedule of PH_OPS.  The solve kernel reads none of it.
  PH_T_NOPS,     // operations of the transposed program
  PH_T_NSTEPS,   // its barrier-separated steps
  PH_T_STEP_PTR, // [t_nsteps+2] operations of each step ..., then the number of leading steps of PH_STEP_PTR that hold every
                 //   factor operation (the adjoint factors J with those; the solve operations among them see a zero rhs)
  PH_T_OPS,      // [2 t_nops] ... as in PH_OPS (8-byte aligned)
  PF_HDR_WORDS = 32,
  PF_SET_ALIGN_WORDS = 16   // blobs of a set (gns_pf_solve_set) start at multiples of 16 words (64 bytes)
};

static_assert(PH_T_OPS < PF_HDR_WORDS, "the header holds every word offset");

#if defined(__HIPCC__)
#define PF_HOST_DEVICE __host__ __device__
#else
#define PF_HOST_DEVICE
#endif

// LDS image of one grid (gns_pf_info.lds_bytes): the factor, the right-hand side and eight bus vectors, in doubles
PF_HOST_DEVICE inline int64_t pf_lds_bytes(const int32_t* h) {
  return 8 * ((int64_t)h[PH_NNZLU] + h[PH_DIM] + 8 * (int64_t)h[PH_N]);
}

// Layout of the fast-decoupled topology blob (gns_fd_prepare_topology): a header of FD_HDR_WORDS int32 words, then int32 arrays at
// the word offsets the header names.  Roles, generators, the Y-bus pattern and its stamps as in the Newton-Raphson blob; B' (rows
// and columns of the PV+PQ buses) and B'' (the PQ buses) each have their own minimum-degree ordering, symbolic LU and two programs
// in the format of PH_OPS: the factorisation, run once per grid, and the triangular solve, run every half-iteration.  Each program
// addresses its own factor's slots: nnz(L+U) factor slots, then dim right-hand-side / solution slots.
#define GNS_FD_MAGIC 0x44504631   // "1FPD"

enum {
  FH_MAGIC = 0, FH_TOTAL, FH_N, FH_E, FH_GN, FH_SLACK, FH_NPV, FH_NPQ, FH_NNZY,
  FH_DIM1, FH_NNZLU1, FH_DIM2, FH_NNZLU2,   // B' (dim N - 1) and B'' (dim n_pq)
  FH_NOPS_F1, FH_NSTEPS_F1, FH_NOPS_S1, FH_NSTEPS_S1, FH_NOPS_F2, FH_NSTEPS_F2, FH_NOPS_S2, FH_NSTEPS_S2,
  // word offsets of the arrays
  FH_ROLE,       // [N]      0 PQ, 1 PV, 2 slack
  FH_P_IDX,      // [N]      position of the bus in B' (its theta), -1 at the slack
  FH_Q_IDX,      // [N]      position of the bus in B'' (its |V|), -1 unless PQ
  FH_GEN_PTR,    // [N+1]
  FH_GEN_IDX,    // [max(Gn,1)]
  FH_Y_PTR,      // [N+1]    the Y-bus pattern and stamps of PH_Y_PTR .. PH_ST
  FH_Y_COL,      // [nnzY]
  FH_Y_DIAG,     // [N]
  FH_ST_PTR,     // [nnzY+1]
  FH_ST,         // [4E]
  FH_BSLOT,      // [2 nnzY] slot in B' and slot in B'' of Y-bus entry p, -1 where the entry is not in that matrix
  FH_PIVOT1,     // [dim1]   B' factor slot of each pivot
  FH_PIVOT2,     // [dim2]
  FH_STEP_F1, FH_OPS_F1,   // B' factorisation: [nsteps+1] step pointers, [2 nops] operations (8-byte aligned)
  FH_STEP_S1, FH_OPS_S1,   // B' solve
  FH_STEP_F2, FH_OPS_F2,   // B'' factorisation
  FH_STEP_S2, FH_OPS_S2,   // B'' solve
  FD_HDR_WORDS = 48
};

static_assert(FH_OPS_S2 < FD_HDR_WORDS, "the header holds every word offset");

// LDS image of one grid (gns_fd_info.lds_bytes): both factors with their right-hand sides and six bus vectors, in doubles
PF_HOST_DEVICE inline int64_t fd_lds_bytes(const int32_t* h) {
  return 8 * ((int64_t)h[FH_NNZLU1] + h[FH_DIM1] + h[FH_NNZLU2] + h[FH_DIM2] + 6 * (int64_t)h[FH_N]);
}

// LDS image of one grid of the DC power flow (gns_dc_lds_bytes), which runs on the FD blob: the B' factor with its right-hand side
// and one bus vector, in doubles
PF_HOST_DEVICE inline int64_t dc_lds_bytes(const int32_t* h) {
  return 8 * ((int64_t)h[FH_NNZLU1] + h[FH_DIM1] + (int64_t)h[FH_N]);
}

// LDS image of one workgroup of the DC contingency screen (gns_dcn1_lds_bytes), which runs on the FD blob with `lanes` outages side
// by side: the DC image, three doubles per line (b_l, the base flow, the two ends' B' positions) and the right-hand sides of the
// outages as [dim_p][lanes + 1] doubles (a row per B' slot, a column per outage, one column of padding)
PF_HOST_DEVICE inline int64_t dcn1_lds_bytes(const int32_t* h, int lanes) {
  return dc_lds_bytes(h) + 8 * (3 * (int64_t)h[FH_E] + (int64_t)h[FH_DIM1] * (lanes + 1));
}

// Outages a workgroup of the screen takes side by side: the largest power of two up to 64 whose image fits max_bytes (1 if none does)
PF_HOST_DEVICE inline int dcn1_lanes(const int32_t* h, int64_t max_bytes) {
  int lanes = 64;
  while (lanes > 1 && dcn1_lds_bytes(h, lanes) > max_bytes) lanes >>= 1;
  return lanes;
}

// LDS image of one workgroup of the screen's adjoint (gns_dcn1_adjoint_lds_bytes) with `lanes` outages side by side: the screen's
// image at that width, a second [dim_p][lanes + 1] array (the adjoint right-hand sides, then lambda_k) and three doubles per outage
// (alpha_k, the worst-loading term of its incoming gradient, its line and its worst line)
PF_HOST_DEVICE inline int64_t dcn1_adjoint_lds_bytes(const int32_t* h, int lanes) {
  return dcn1_lds_bytes(h, lanes) + 8 * ((int64_t)h[FH_DIM1] * (lanes + 1) + 3 * (int64_t)lanes);
}

// Outages a workgroup of the adjoint takes side by side: as dcn1_lanes, on the adjoint's image
PF_HOST_DEVICE inline int dcn1_adjoint_lanes(const int32_t* h, int64_t max_bytes) {
  int lanes = 64;
  while (lanes > 1 && dcn1_adjoint_lds_bytes(h, lanes) > max_bytes) lanes >>= 1;
  return lanes;
}

// Doubles of one (grid, chunk) partial of the adjoint's workspace: dl/dP by bus, dl/db and the sum of w by line, then the chunk's status
PF_HOST_DEVICE inline int64_t dcn1_adjoint_partial(const int32_t* h) { return (int64_t)h[FH_N] + 2 * (int64_t)h[FH_E] + 1; }

// LDS image of one workgroup of the DC optimal power flow's interior-point kernel (gns_dcopf_lds_bytes), one grid per workgroup:
// the packed lower triangle of the Gn x Gn normal matrix, fourteen doubles per generator (the dispatch, its bounds and costs, the
// box rows' slacks and multipliers, the gradients, the two right-hand sides and the step) and ten per line (f0, the rating, the flow,
// the limit rows' slacks and multipliers, their weights and the two vectors S^T is applied to)
PF_HOST_DEVICE inline int64_t dcopf_lds_bytes(const int32_t* h) {
  const int64_t Gn = h[FH_GN];
  return 8 * (Gn * (Gn + 1) / 2 + 14 * Gn + 10 * (int64_t)h[FH_E]);
}

// LDS image of one workgroup of the DC optimal power flow's adjoint (gns_dcopf_adjoint_lds_bytes), one grid per workgroup, at KKT
// order n: the DC N-1 screen's image at width 1 with the 32 Gn bytes of generator zeros (the network solves), three doubles per unit
// and one per line (the cotangents and the adjoint of the dispatch and of the line multipliers), two int32 per unit and one per line
// (each unit's row state, the free units and the active lines in order), and the dense KKT matrix with its right-hand side as
// [n][(n + 1) | 1] doubles (an odd row length: a column walks every bank)
PF_HOST_DEVICE inline int64_t dcopf_adjoint_lds_bytes(const int32_t* h, int64_t n) {
  const int64_t Gn = h[FH_GN], E = h[FH_E];
  return dcn1_lds_bytes(h, 1) + 32 * Gn + 8 * (3 * Gn + E + (2 * Gn + E + 1) / 2 + n * ((n + 1) | 1));
}

// The largest KKT order the adjoint's image holds within max_bytes: up to 2 Gn, the worst case (Gn free units, Gn - 1 active lines
// and the balance); 0 when even the network-solve part does not fit
PF_HOST_DEVICE inline int dcopf_adjoint_order(const int32_t* h, int64_t max_bytes) {
  int n = 2 * h[FH_GN];
  while (n > 0 && dcopf_adjoint_lds_bytes(h, n) > max_bytes) --n;
  return n;
}

// What the code that handles either kind of blob (the set checks on the host and in the set kernels) needs to know of a kind.
// The magic, the total, N, E and Gn sit at the same header words in both.
static_assert(FH_MAGIC == PH_MAGIC && FH_TOTAL == PH_TOTAL && FH_N == PH_N && FH_E == PH_E && FH_GN == PH_GN, "shared header words");

struct PfBlobKind {
  static constexpr int32_t MAGIC = GNS_PF_MAGIC;
  static constexpr int HDR_WORDS = PF_HDR_WORDS, NNZY = PH_NNZY;
  PF_HOST_DEVICE static int64_t lds_bytes(const int32_t* h) { return pf_lds_bytes(h); }
};

struct FdBlobKind {
  static constexpr int32_t MAGIC = GNS_FD_MAGIC;
  static constexpr int HDR_WORDS = FD_HDR_WORDS, NNZY = FH_NNZY;
  PF_HOST_DEVICE static int64_t lds_bytes(const int32_t* h) { return fd_lds_bytes(h); }
};

// The FD blob as the DC power flow uses it: the same blob, its own LDS image
struct DcBlobKind : FdBlobKind {
  PF_HOST_DEVICE static int64_t lds_bytes(const int32_t* h) { return dc_lds_bytes(h); }
};
