/* C-ABI of the batched Newton-Raphson AC power-flow solver (libgns_hip.so).
 *
 * The reference evaluates a trained GNS against PYPOWER's runpf(PF_ALG=1) (GNS/evaluate.py:24-40), one grid at a time on the
 * CPU.  This solver produces that baseline on the device for a whole batch that shares one topology: the sparse structure of the
 * Jacobian and of its LU factor is analysed ONCE on the host (gns_pf_prepare_topology), and every grid then runs the same
 * elimination program; only the values differ.  A batch that mixes topologies runs in one launch over a set of such analyses
 * (gns_pf_solve_set, at the end of this file), each grid on its own.  Conventions are those of gns_hip.h: plain pointers, caller-owned device memory,
 * GNS_E* return codes (the enum of gns_hip.h), work enqueued on the caller's stream, no allocation and no host synchronisation
 * inside gns_pf_solve.
 *
 * Semantics
 *   Inputs: buses [Bt,N,6], lines [Bt,E,7], generators [Bt,Gn,7], fp32, the layout GNS.forward takes (GNS/utils.py:4-13): powers in
 *   per unit, the line shift in radians, tau used as given.  The id columns are those the topology was prepared from.
 *   Bus roles: the slack is given to the analysis; PV = every other bus with at least one generator; PQ = every remaining bus.
 *   Y-bus (MATPOWER makeYbus): per line (f, t, r, x, b, tau, phi), y_s = 1/(r + jx), a = tau e^{j phi}:
 *     Y_ff += (y_s + jb/2)/tau^2,  Y_tt += y_s + jb/2,  Y_ft += -y_s/conj(a),  Y_tf += -y_s/a;  parallel lines add;
 *     Y_ii += Gs + jBs.
 *   Specified injections: S_i = sum of Pg (generator column 6) on bus i - Pd_i - j Qd_i (generator qg is not used).
 *   Newton-Raphson in polar form (MATPOWER newtonpf): unknowns theta at PV+PQ, |V| at PQ;
 *     F = [Re(V conj(YV) - S) at PV+PQ ; Im(...) at PQ].
 *   Start: |V| = vg of the first generator listed on each PV / slack bus (1 on a slack without generators), 1 at PQ buses, theta 0.
 *   Warm start (v0, theta0 [Bt,N] fp64, both or neither): |V| at PQ buses from v0, theta = theta0 - theta0[slack].
 *   ||F||_inf < tol is tested before every update; iterations = updates applied, at most max_iter.  theta_slack stays 0.
 *   Arithmetic: fp64 throughout (Y-bus, mismatch, Jacobian, factorisation, update).
 *   Failure is per grid: a zero or non-finite pivot, a non-finite mismatch or a non-finite iterate stops that grid with
 *   converged = 0; v / theta then hold its last finite iterate and mismatch the norm there (NaN when the mismatch itself is not
 *   finite).  No float atomics: a grid's results are bit-identical alone or in any batch, and from run to run.
 *
 * Outputs: v, theta [Bt,N] fp64; converged [Bt] uint8 (0/1); iterations [Bt] int32; mismatch [Bt] fp64 (the final ||F||_inf).
 *
 * Kernel: one wave per grid, the grid's LU factor, right-hand side and bus state in LDS (gns_powerflow.hip).  A topology whose
 * LDS image (gns_pf_info.lds_bytes = 8 * (nnz(L+U) + dim + 8 N) bytes) exceeds GNS_PF_LDS_MAX_BYTES is refused by gns_pf_solve
 * with GNS_EUNSUPPORTED.
 */
#ifndef GNS_POWERFLOW_H
#define GNS_POWERFLOW_H
#include <stddef.h>
#include <stdint.h>

#include "gns_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The LDS one workgroup may use on gfx950 (160 KiB): the limit of a topology's LDS image. */
#define GNS_PF_LDS_MAX_BYTES 163840
/* The most slots (nnz(L+U) + dim) a program may address: its operands are 16-bit.  The analysis refuses a topology whose factor
 * needs more with GNS_EUNSUPPORTED. */
#define GNS_PF_MAX_SLOTS 65535

typedef struct gns_pf_config {
  int32_t n_bus;     /* N  */
  int32_t n_line;    /* E  */
  int32_t n_gen;     /* Gn */
  int32_t max_iter;  /* Newton updates at most (MATPOWER: 10)  */
  double  tol;       /* ||F||_inf convergence bound (MATPOWER: 1e-8) */
} gns_pf_config;

/* What the analysis of a topology found (read from a HOST copy of the blob). */
typedef struct gns_pf_info {
  int32_t n_bus, n_line, n_gen;
  int32_t slack;      /* 0-based */
  int32_t n_pv, n_pq;
  int32_t dim;        /* Jacobian dimension = (N - 1) + n_pq */
  int32_t nnz_jac;    /* structural nonzeros of the Jacobian */
  int32_t nnz_lu;     /* nonzeros of L + U (unit diagonal of L not stored) under the fill-reducing ordering */
  int32_t nnz_ybus;   /* structural nonzeros of the Y-bus */
  int32_t n_ops;      /* elimination + triangular-solve operations per Newton iteration */
  int32_t n_steps;    /* barrier-separated steps those operations are scheduled into */
  int64_t lds_bytes;  /* LDS image of one grid; > GNS_PF_LDS_MAX_BYTES: gns_pf_solve returns GNS_EUNSUPPORTED */
  int32_t n_adj_ops;      /* operations of the transposed-solve program of gns_pf_adjoint (J^T x = b on the factor) */
  int32_t n_adj_steps;    /* barrier-separated steps of that program */
  int32_t n_factor_steps; /* leading steps of the solve program that hold every factorisation operation: gns_pf_adjoint
                             factors J with these (0 when J is diagonal) */
} gns_pf_info;

/* Host analysis.  From 0-based f_bus / t_bus [E], generator bus [Gn] HOST arrays and the 0-based slack bus: bus roles, the Y-bus
 * pattern with every line's four stamps, a minimum-degree ordering on the bus graph (the theta and |V| of a PQ bus kept together),
 * the symbolic LU (structurally symmetric, no pivoting), the map of Jacobian entries to factor slots and the elimination +
 * triangular-solve program in barrier-separated steps, in one relocatable int32 blob of gns_pf_topology_bytes() bytes.
 * GNS_ETOPOLOGY: a bus id out of range, a slack that is not a bus, or a bus with no path of lines to the slack (an island: its
 * theta is undetermined and the Jacobian structurally singular).  The program's length depends on the ids, so
 * gns_pf_topology_bytes runs the analysis and reports the blob's exact size.  GNS_EUNSUPPORTED: the factor needs more than
 * GNS_PF_MAX_SLOTS slots; gns_pf_topology_slots then reports how many (and the count of an accepted topology too; its errors are
 * otherwise those of the analysis). */
int gns_pf_topology_bytes(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                          const int32_t* gen_bus, int32_t slack, size_t* bytes);
int gns_pf_prepare_topology(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                            const int32_t* gen_bus, int32_t slack, void* topo_host_out, size_t topo_bytes);
int gns_pf_topology_info(const void* topo_host, gns_pf_info* info);
int gns_pf_topology_slots(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                          const int32_t* gen_bus, int32_t slack, int64_t* slots);

/* The same analysis with generator row out_gen (0-based) out of service: the blob a row of gns_acg1_screen ("AC generator
 * contingency screening", below) is solved on.  The row gives its bus no role (a sole unit's bus that is not the slack becomes a PQ
 * bus and gains a |V| unknown: dim is the plain analysis' plus one exactly then) and is left off the by-bus generator lists, which
 * hold the other Gn - 1 rows under their original numbers; the header's n_gen stays Gn, so the header checks of every entry point
 * and the indexing of generators [Bt,Gn,7] are untouched.  The Y-bus pattern and its stamps come from the lines alone: the same
 * words whatever out_gen is.  out_gen = -1 gives gns_pf_prepare_topology's blob byte for byte; GNS_EINVAL for an out_gen outside
 * -1 .. n_gen-1; otherwise the arguments and errors of the three entry points above. */
int gns_pf_topology_bytes_out_gen(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                  const int32_t* gen_bus, int32_t slack, int32_t out_gen, size_t* bytes);
int gns_pf_prepare_topology_out_gen(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                    const int32_t* gen_bus, int32_t slack, int32_t out_gen, void* topo_host_out, size_t topo_bytes);
int gns_pf_topology_slots_out_gen(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                  const int32_t* gen_bus, int32_t slack, int32_t out_gen, int64_t* slots);

/* Device workspace of a solve of Bt grids (the Y-bus values, 16 bytes per structural nonzero and grid). */
int gns_pf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes);

/* Solve Bt grids.  topo_host: the host blob (sizes are read from it on the host); topo_dev: the same bytes on the device.
 * v0 / theta0: NULL (flat start) or both [Bt,N] fp64.  stream: a hipStream_t passed as void*.
 * GNS_EINVAL: a NULL pointer or a config that does not match the blob; GNS_ESIZE: workspace too small; GNS_EUNSUPPORTED: the
 * topology's LDS image exceeds GNS_PF_LDS_MAX_BYTES. */
int gns_pf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                 const float* buses, const float* lines, const float* generators, int64_t Bt,
                 const double* v0, const double* theta0,
                 double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Batches that mix topologies (an N-1 contingency set).  A SET is topology blobs of one (N, E, Gn) concatenated in one int32 buffer
 * of set_words words, each starting at a word offset that is a multiple of 16 (64 bytes; blobs are relocatable, and their
 * operation records need 8-byte alignment).  set_host and set_dev hold the same words.  member_off [n_member] (host) lists the
 * offsets of the blobs this call may use; the host checks every member before launching: aligned, its whole blob inside
 * set_words, a blob whose N, E and Gn are cfg's (GNS_EINVAL otherwise), and its LDS image <= GNS_PF_LDS_MAX_BYTES
 * (GNS_EUNSUPPORTED for the whole call otherwise).  The launch uses the largest member's LDS image.
 * Workspace: Bt x (the largest nnz(Y) of the members) Y-bus entries of 16 bytes, rounded up to 256 bytes. */
int gns_pf_workspace_bytes_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                               int32_t n_member, int64_t Bt, size_t* bytes);

/* Solve Bt grids, each on its own blob of the set.  grid_off [Bt] (device): word offset in the set of grid g's blob, or -1 for
 * "not solved" (a topology that islands a bus).  order [Bt] (device, or NULL for 0..Bt-1): workgroup w solves grid order[w]; a
 * permutation of 0..Bt-1 that groups the grids of one topology keeps that blob in L2 (entries outside 0..Bt-1 are skipped).
 * Outputs go to grid g's rows whatever the order, and a grid's results do not depend on its batch, its position or the order:
 * they are bit-identical to gns_pf_solve on its blob.  A grid whose offset is -1, misaligned, outside the set, or not at a blob of
 * cfg's shape that fits the launch (checked on the device before the blob is indexed; the set is never read out of bounds) gets
 * v = theta = NaN, converged = 0, iterations = -1, mismatch = NaN.
 * Errors as gns_pf_solve: GNS_EINVAL for a NULL pointer, a config or member that does not match, GNS_ESIZE for a short
 * workspace, GNS_EUNSUPPORTED for a member's LDS image above the limit. */
int gns_pf_solve_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                     const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const double* v0, const double* theta0,
                     double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Gradients (the adjoint).  gns_pf_adjoint takes the inputs of a gns_pf_solve call (cfg, blob, buses, lines, generators, Bt; not
 * the warm start), that call's outputs v, theta [Bt,N] fp64 and converged [Bt] uint8, and the incoming gradients grad_v,
 * grad_theta [Bt,N] fp64 of a loss l(v, theta) (either may be NULL: zero).  It writes dl/d(input) into grad_buses [Bt,N,6],
 * grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32, each of which may be NULL (not computed).  Every element of each non-NULL
 * output is written (overwritten, not accumulated).
 *
 * Method: the implicit function theorem at the solution F(x*, p) = 0, x = [theta at PV+PQ ; |V| at PQ]:
 *   J^T lambda = dl/dx = [grad_theta at PV+PQ ; grad_v at PQ],   dl/dp = -(dF/dp)^T lambda  (+ the direct grad_v of a set |V|),
 * with J the Newton Jacobian at (v, theta), factored by the leading n_factor_steps steps of the blob's solve program (on a zero
 * right-hand side), and lambda from its transposed-solve program (U^T y = g, then L^T lambda = y; gns_pf_info.n_adj_ops /
 * n_adj_steps).  One wave per grid, the solve's
 * LDS image (lambda_P, lambda_Q in the injection vectors): every topology the solve accepts, the adjoint accepts.  Workspace: the
 * Y-bus values only, so gns_pf_workspace_bytes / gns_pf_workspace_bytes_set give its size.  fp64 throughout, rounded once to fp32.
 * No atomics: a grid's gradient is bit-identical alone, in any batch, in any order and from run to run.
 *
 * Contract (lambda_P at PV+PQ buses, lambda_Q at PQ buses, both 0 elsewhere; signs follow F = Re/Im(V conj(YV)) - S_spec,
 * S_spec = sum Pg - Pd - j Qd):
 *   buses      col 2 Pd: -lambda_P;  col 3 Qd: -lambda_Q;  col 4 Gs: -|V|^2 lambda_P;  col 5 Bs: +|V|^2 lambda_Q.  All 0 at the
 *              slack; Qd and Bs 0 at PV buses.  Cols 0, 1 (id, type): 0.
 *   lines      cols 2-6 (r, x, b, tau, shift): -lambda^T dF/dp through the line's four Y-bus stamps (ff, tt, ft, tf of makeYbus);
 *              parallel lines each get their own.  Cols 0, 1 (ids): 0.  The line's buses are read from its id columns, which must
 *              be those the blob was prepared from (a line whose ids are not buses of the grid gets a NaN row).
 *   generators col 6 Pg: +lambda_P at its bus.  Col 4 vg: for the first generator listed on a PV or slack bus only (its vg is
 *              that bus's |V|), grad_v of the bus plus -lambda^T dF/d|V_bus|; 0 for every other generator.  Cols 0-3, 5 (bus,
 *              Pmax, Pmin, Pg_set, qg): 0.
 *   The slack's theta is constant: its incoming gradient is ignored.  Warm starts are not differentiated.
 *   A grid whose incoming grad_v and grad_theta rows are all exactly zero gets zero rows, whatever its convergence.  Otherwise a
 *   grid with converged == 0, or whose factor has a zero or non-finite pivot, gets NaN in all three rows.
 *
 * Errors as gns_pf_solve: GNS_EINVAL for a NULL cfg / blob / input / v / theta / converged / workspace or a config that does not
 * match the blob, GNS_ESIZE for a short workspace, GNS_EUNSUPPORTED for an LDS image above the limit.  With all three outputs
 * NULL nothing is launched. */
int gns_pf_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                   const float* buses, const float* lines, const float* generators, int64_t Bt,
                   const double* v, const double* theta, const uint8_t* converged,
                   const double* grad_v, const double* grad_theta,
                   float* grad_buses, float* grad_lines, float* grad_generators,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The adjoint of a gns_pf_solve_set call: its set, members, grid_off and order (grid g's rows whatever the order), then the
 * arguments of gns_pf_adjoint.  Each grid's blob is checked on the device as gns_pf_solve_set does; a grid without a usable blob
 * (an islanding topology: grid_off -1) gets NaN rows, or zero rows when its incoming gradient is zero.  Results are bit-identical
 * to gns_pf_adjoint on the grid's blob.  Errors as gns_pf_solve_set. */
int gns_pf_adjoint_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                       const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                       const float* buses, const float* lines, const float* generators, int64_t Bt,
                       const double* v, const double* theta, const uint8_t* converged,
                       const double* grad_v, const double* grad_theta,
                       float* grad_buses, float* grad_lines, float* grad_generators,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Fast-decoupled power flow (PYPOWER runpf with PF_ALG = 2, XB, or 3, BX: makeB + fdpf), the classical cheap iterative
 * baseline a trained GNS is compared with next to Newton-Raphson (GNS/evaluate.py:42-58).
 *
 * Semantics
 *   Inputs, bus roles, Y-bus, specified injections, start and warm start: those of the Newton-Raphson section above.
 *   B' and B'' (makeB) are -Im(Y) of modified copies of the grid, with per-unit shunts as above:
 *     B':  bus Bs = 0, line b = 0, tau = 1, shift kept; XB also sets r = 0.  Rows and columns of the PV+PQ buses.
 *     B'': shift = 0, everything else as given;        BX also sets r = 0.  Rows and columns of the PQ buses.
 *   Both share the Y-bus pattern, so one analysis serves both variants: the variant is gns_fd_config.alg, a launch argument.
 *   Iteration (fdpf): mis = (V conj(YV) - S) / |V|, P = Re(mis) at PV+PQ, Q = Im(mis) at PQ.  max(||P||_inf, ||Q||_inf) < tol is
 *   tested at the start; then, at most max_iter times:
 *     P half-step: dtheta = -B'^-1 P, theta += dtheta, recompute the mismatch, test;
 *     Q half-step: d|V| = -B''^-1 Q, |V| += d|V|, recompute the mismatch, test.
 *   iterations = the P half-steps taken.  mismatch = the norm the last test read: the SCALED max(||P||_inf, ||Q||_inf) of mis / |V|,
 *   not Newton-Raphson's unscaled ||F||_inf.  n_pq = 0: the Q half-step is empty and ||Q|| = 0.
 *   Both factors are computed once per grid (fp64, no pivoting, the minimum-degree orderings of the analysis).
 *   Failure is per grid: a grid that meets the test at its start is converged with 0 iterations, whatever its factors; otherwise a
 *   zero or non-finite pivot in either factor stops it at its start point (converged 0, iterations 0).  A non-finite step stops
 *   it before that update; a non-finite mismatch stops it with mismatch NaN; v / theta keep the last finite iterate.  No atomics:
 *   a grid's results are bit-identical alone, in any batch and from run to run.
 *   PYPOWER's defaults: tol 1e-8, max_iter 30 (PF_MAX_IT_FD).
 *
 * Kernel: one wave per grid; both factors, both right-hand sides and six bus vectors in LDS (gns_fd_info.lds_bytes =
 * 8 * (nnz_lu_p + dim_p + nnz_lu_pp + dim_pp + 6 N) bytes); the Y-bus values go to the workspace once.  Workspace: that of
 * gns_pf_workspace_bytes (16 bytes per Y-bus entry and grid).  The two factorisation programs run once, the two solve programs
 * once per half-step.
 *
 * Gradients: FD solves the same equations F = 0 as Newton-Raphson, so the implicit-function gradient at its solution is the
 * Newton-Raphson adjoint: call gns_pf_adjoint / gns_pf_adjoint_set on the Newton-Raphson analysis of the topology with FD's v,
 * theta and converged ("Gradients" above). */

typedef struct gns_fd_config {
  gns_pf_config pf;  /* n_bus, n_line, n_gen, max_iter (P half-steps at most; PYPOWER: 30), tol (scaled mismatch bound: 1e-8) */
  int32_t alg;       /* 2: XB, 3: BX (PYPOWER's PF_ALG) */
} gns_fd_config;

typedef struct gns_fd_info {
  int32_t n_bus, n_line, n_gen;
  int32_t slack;                          /* 0-based */
  int32_t n_pv, n_pq;
  int32_t nnz_ybus;
  int32_t dim_p, nnz_lu_p;                /* B': N - 1, nonzeros of its L + U (unit diagonal of L not stored) */
  int32_t dim_pp, nnz_lu_pp;              /* B'': n_pq, nonzeros of its L + U */
  int32_t factor_p_ops, factor_p_steps;   /* operations and barrier-separated steps of the B' factorisation (once per grid) */
  int32_t solve_p_ops, solve_p_steps;     /* ... of the B' solve (every P half-step) */
  int32_t factor_pp_ops, factor_pp_steps; /* ... of the B'' factorisation */
  int32_t solve_pp_ops, solve_pp_steps;   /* ... of the B'' solve (every Q half-step) */
  int64_t lds_bytes;                      /* LDS image of one grid; > GNS_PF_LDS_MAX_BYTES: gns_fd_solve returns GNS_EUNSUPPORTED */
} gns_fd_info;

/* Host analysis, arguments and errors as gns_pf_topology_bytes / gns_pf_prepare_topology / gns_pf_topology_slots (GNS_ETOPOLOGY
 * for an island; GNS_EUNSUPPORTED when a factor needs more than GNS_PF_MAX_SLOTS slots, nnz(L+U) + dim, and gns_fd_topology_slots
 * then reports the larger of the two).  B' gets a minimum-degree ordering of the bus graph without the slack, B'' one of the
 * subgraph the PQ buses induce. */
int gns_fd_topology_bytes(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                          const int32_t* gen_bus, int32_t slack, size_t* bytes);
int gns_fd_prepare_topology(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                            const int32_t* gen_bus, int32_t slack, void* topo_host_out, size_t topo_bytes);
int gns_fd_topology_info(const void* topo_host, gns_fd_info* info);
int gns_fd_topology_slots(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                          const int32_t* gen_bus, int32_t slack, int64_t* slots);

/* Solve, arguments and errors as gns_pf_workspace_bytes / gns_pf_solve on an FD blob (GNS_EINVAL also for alg not 2 or 3). */
int gns_fd_workspace_bytes(const gns_fd_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes);
int gns_fd_solve(const gns_fd_config* cfg, const void* topo_host, const void* topo_dev,
                 const float* buses, const float* lines, const float* generators, int64_t Bt,
                 const double* v0, const double* theta0,
                 double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Mixed topologies: gns_pf_workspace_bytes_set / gns_pf_solve_set on a set of FD blobs (the same set layout, member checks,
 * grid_off = -1 semantics and device-side blob checks); results are bit-identical to gns_fd_solve on each grid's blob. */
int gns_fd_workspace_bytes_set(const gns_fd_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                               int32_t n_member, int64_t Bt, size_t* bytes);
int gns_fd_solve_set(const gns_fd_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                     const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const double* v0, const double* theta0,
                     double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                     void* workspace, size_t workspace_bytes, void* stream);

/* DC power flow (PYPOWER makeBdc + dcpf and the DC branch of runpf), the linear baseline a trained GNS is compared with
 * (GNS/evaluate.py:13, 42-58), with the per-line active flows and the slack's balancing power, and its adjoint.
 *
 * Semantics
 *   Inputs and the slack: those of the Newton-Raphson section above; PV and PQ buses are treated alike; every line is in service.
 *   Per line (f, t, r, x, b, tau, shift): b_l = 1 / (x tau) (tau as given), Pfinj_l = -b_l shift.  r, the line charging b and the
 *   bus Bs are not used.
 *   Bbus (makeBdc): ff += b_l, tt += b_l, ft -= b_l, tf -= b_l; parallel lines add.
 *   P_i = sum of Pg (generator column 6) on bus i - Pd_i - Gs_i - Pbusinj_i, with Pbusinj_f += Pfinj_l, Pbusinj_t -= Pfinj_l.
 *   theta_slack = 0; theta at the other buses r solves Bbus[r, r] theta_r = P_r.
 *   line_flow_l = b_l (theta_f - theta_t) + Pfinj_l: the active flow at the from end (the to end carries its negative).
 *   slack_p = Bbus[slack, :] theta - P_slack: what the slack generates beyond its listed Pg (runpf adds it to the slack generator).
 *   |V| = 1 at every bus: not an output.
 *   Arithmetic: fp64 throughout.  Bbus[r, r] is factored once per grid (no pivoting, the B' ordering of the analysis).
 *   Failure is per grid: a zero or non-finite pivot or a non-finite theta gives converged = 0 and NaN in theta, line_flow and
 *   slack_p of that grid; the other grids are unaffected.  No atomics: a grid's results are bit-identical alone, in any batch, in
 *   any order and from run to run.
 *
 * Outputs: theta [Bt,N], line_flow [Bt,E], slack_p [Bt] fp64; converged [Bt] uint8 (0/1: solved).
 *
 * Analysis: Bbus[r, r] has the sparsity of the fast-decoupled B', so the calls take an FD blob (gns_fd_prepare_topology) and use its B'
 * ordering, factor slots and two B' programs; there is no DC analysis.  Configuration: a gns_pf_config for n_bus, n_line and n_gen;
 * max_iter and tol are not read.
 *
 * Kernel: one wave per grid (gns_dcpf.hip): Bbus from the line rows into the B' factor slots, the B' factorisation program once, the
 * B' solve program once, then the flows and the slack's row.  LDS image (gns_dc_lds_bytes): 8 * (nnz_lu_p + dim_p + N) bytes, the B'
 * factor with its right-hand side and one bus vector; smaller than the fast-decoupled image, so every topology gns_fd_solve accepts
 * is accepted.  No workspace: the queries report 0 bytes, and workspace may be NULL.
 *
 * Errors: GNS_EINVAL for a NULL cfg, blob, input or output, a blob that is not an FD blob or whose N, E, Gn are not cfg's;
 * GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES.  Nothing is allocated and the host is not synchronised. */
int gns_dc_lds_bytes(const void* topo_host, int64_t* bytes);
int gns_dc_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes);
int gns_dc_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                 const float* buses, const float* lines, const float* generators, int64_t Bt,
                 double* theta, double* line_flow, double* slack_p, uint8_t* converged,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Mixed topologies: the set, members, grid_off and order of gns_fd_solve_set (a set of FD blobs), with its host and device-side
 * checks against DC's LDS image.  A grid without a usable blob (grid_off -1: a topology that islands a bus) gets converged = 0 and
 * NaN in theta, line_flow and slack_p.  Results are bit-identical to gns_dc_solve on each grid's blob. */
int gns_dc_workspace_bytes_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                               int32_t n_member, int64_t Bt, size_t* bytes);
int gns_dc_solve_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                     const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     double* theta, double* line_flow, double* slack_p, uint8_t* converged,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Gradients.  gns_dc_adjoint takes the inputs of a gns_dc_solve call, its outputs theta and converged, and the incoming gradients
 * grad_theta [Bt,N], grad_line_flow [Bt,E], grad_slack_p [Bt] fp64 of a loss l(theta, line_flow, slack_p) (each may be NULL: zero).
 * It writes dl/d(input) into grad_buses [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32, each of which may be NULL (not
 * computed; with all three NULL nothing is launched).  Every element of each non-NULL output is written (overwritten, not accumulated).
 *
 * Method: the map is linear in P with a symmetric matrix, so with g_r = grad_theta_r + sum_l grad_line_flow_l b_l (e_f - e_t)_r the
 * adjoint is Bbus[r, r] lambda_r = g_r on the same factor with the same B' solve program, lambda_slack = 0.  One wave per grid, the
 * solve's LDS image.  fp64 throughout, rounded once to fp32; no atomics: bit-identical alone, in any batch, in any order.
 *
 * Contract (the exact derivative of the map above; w_l = grad_line_flow_l - (lambda_f - lambda_t)):
 *   buses      col 2 Pd and col 4 Gs: -(lambda_i - grad_slack_p), at the slack too (slack_p = -sum_i P_i: Bbus has zero column sums).
 *              Every other column: 0.
 *   lines      dl/db_l = w_l (theta_f - theta_t - shift_l);  col 3 x: -dl/db_l b_l / x;  col 5 tau: -dl/db_l b_l / tau;
 *              col 6 shift: -b_l w_l.  Cols 0, 1, 2, 4 (ids, r, b): 0.  The line's buses are read from its id columns, which must be
 *              those the blob was prepared from (a line whose ids are not buses of the grid gets a NaN row, and a NaN line_flow).
 *   generators col 6 Pg: lambda_bus - grad_slack_p.  Every other column: 0.
 *   A grid whose incoming gradients are all exactly zero gets zero rows, whatever its state.  Otherwise a grid with converged == 0,
 *   or whose factor has a zero or non-finite pivot, gets NaN in all three rows.
 * Errors as gns_dc_solve (theta and converged must not be NULL).  gns_dc_adjoint_set is the adjoint of a gns_dc_solve_set call: a
 * grid without a usable blob gets NaN rows, or zero rows when its incoming gradients are zero. */
int gns_dc_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                   const float* buses, const float* lines, const float* generators, int64_t Bt,
                   const double* theta, const uint8_t* converged,
                   const double* grad_theta, const double* grad_line_flow, const double* grad_slack_p,
                   float* grad_buses, float* grad_lines, float* grad_generators,
                   void* workspace, size_t workspace_bytes, void* stream);
int gns_dc_adjoint_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                       const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                       const float* buses, const float* lines, const float* generators, int64_t Bt,
                       const double* theta, const uint8_t* converged,
                       const double* grad_theta, const double* grad_line_flow, const double* grad_slack_p,
                       float* grad_buses, float* grad_lines, float* grad_generators,
                       void* workspace, size_t workspace_bytes, void* stream);

/* DC contingency screening: the post-outage DC flows of a list of single-line outages (an N-1 set) of every grid of a batch, from
 * the base factorisation alone (line-outage distribution factors).
 *
 * Semantics (the DC power flow above is the base case: theta, F_l = line_flow_l, b_l, Bbus; fp64 throughout)
 *   The outage of line k with ends f, t removes its four Bbus stamps and its Pfinj, a rank-1 change of Bbus[r, r]:
 *   a_k = (e_f - e_t) restricted to the non-slack buses; Bbus[r, r] z_k = a_k on the base factor, z_k = 0 at the slack;
 *   d_k = z_k[f] - z_k[t];  alpha_k = F_k / (1 - b_k d_k);  theta' = theta + alpha_k z_k;
 *   F'_l = F_l + b_l (z_k[f_l] - z_k[t_l]) alpha_k for l != k, F'_k = 0.  A line from a bus to itself has a_k = 0 and changes nothing.
 *   worst_loading = max_l |F'_l| / rating_l (rating NULL: 1) and worst_line the 0-based line that attains it, the lowest of equals.
 *   Islanding: an outage that disconnects the graph (a bridge) has 1 - b_k d_k = 0 in exact arithmetic.  The kernel does not decide
 *   that numerically: the caller finds the bridges of the topology and passes islanding[n_outage] (1: bridge).  Those rows get NaN
 *   in line_flow and worst_loading and -1 in worst_line, in every grid.
 *   Failure: a grid whose base solve fails (converged = 0, as gns_dc_solve decides it) gets NaN / -1 in every row; a row whose z_k,
 *   denominator or alpha_k is not finite (or whose denominator is zero) gets NaN / -1 alone.  Other rows are unaffected.
 *   Every (grid, outage) row is bit-identical alone, in any batch, for any outage list or order that holds the outage (duplicates
 *   are independent rows), and from run to run: no atomics, the reductions in a fixed order.
 *
 * Inputs: outages as 0-based line indices, on the host (checked before the launch) and on the device (read by the kernel), both
 * [n_outage] int32; islanding [n_outage] uint8 on the device; rating NULL, [E] (rating_per_grid 0) or [Bt,E] (1) fp64 on the device.
 * Outputs: line_flow [Bt,n_outage,E] fp64, or NULL for the summaries alone (8 Bt n_outage E bytes not written);
 * worst_loading [Bt,n_outage] fp64; worst_line [Bt,n_outage] int32; converged [Bt] uint8, the base solve's.
 *
 * Kernel (gns_dcn1.hip): one wave per (grid, chunk of W outages), on the FD blob.  The wave builds and factors Bbus[r, r] once and
 * solves the base case; then lane j runs the B' solve program on the right-hand side of outage j of its chunk, with no barrier,
 * against the shared factor; then the chunk's outages are written one after the other with a line per lane.  LDS image
 * (gns_dcn1_lds_bytes): 8 * (nnz_lu_p + dim_p + N + 3 E + dim_p (W + 1)) bytes, the DC image, three doubles per line and the
 * right-hand sides [dim_p][W + 1]; W is the largest power of two up to 64 whose image fits GNS_PF_LDS_MAX_BYTES (1 when none
 * does: the image reported is then W = 1's).  No workspace: the query reports 0 bytes, and workspace may be NULL.
 *
 * Errors: GNS_EINVAL for a NULL cfg, blob, input, outage list, islanding mask or output other than line_flow, a blob that is not an
 * FD blob or whose N, E, Gn are not cfg's, n_outage <= 0, an outage outside 0 .. E-1, rating_per_grid outside {0, 1}, or
 * Bt * ceil(n_outage / W) above 2^31 - 1; GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES.  Every refusal comes before
 * any launch; nothing is allocated and the host is not synchronised. */
int gns_dcn1_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes /* W; may be NULL */);
int gns_dcn1_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage, size_t* bytes);
int gns_dcn1_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                    const double* rating, int32_t rating_per_grid,
                    double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Gradients of the screen.  gns_dcn1_adjoint takes the inputs of a gns_dcn1_screen call (the same outage list, islanding mask and
 * rating), its outputs worst_line and converged, and the incoming gradients grad_line_flow [Bt,n_outage,E] and grad_worst_loading
 * [Bt,n_outage] fp64 of a loss l(line_flow, worst_loading) (each may be NULL: zero).  It writes dl/d(input) into grad_buses
 * [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32, each of which may be NULL (not computed; with all three NULL
 * nothing is launched).  Every element of each non-NULL output is written (overwritten, not accumulated).  line_flow is not an
 * input: each row's state is recomputed with the forward's own arithmetic.
 *
 * Method (A = Bbus[r, r], m_l = (e_f - e_t)_r of line l, z_k, d_k, den_k = 1 - b_k d_k, alpha_k, theta'_k as above).  For a solved
 * row (grid, k): G_k = grad_line_flow of the row, plus grad_worst_loading sign(F'_{k,w}) / rating_w at w = worst_line (so a tie
 * sends the gradient to the lowest of equals); its entry at l = k is ignored, F'_{k,k} being the constant 0.
 *   q_k = sum_{l != k} G_{k,l} b_l m_l;  A u_k = q_k on the base factor with the B' solve program;
 *   lambda_k = u_k + z_k b_k (m_k^T u_k) / den_k  (Sherman-Morrison: the DC adjoint of the grid without line k), 0 at the slack;
 *   w_{k,l} = G_{k,l} - (lambda_k[f_l] - lambda_k[t_l]) for l != k, 0 for l = k.
 * Summed over the outages of the list:  dl/dP_i = sum_k lambda_k[i];  dl/db_l = sum_k w_{k,l} (theta'_k[f_l] - theta'_k[t_l] -
 * shift_l);  dl/dshift_l = -b_l sum_k w_{k,l}.  Two solves on the base factor per outage; nothing is factored per outage.
 *
 * Contract (gns_dc_adjoint's columns):
 *   buses      col 2 Pd and col 4 Gs: -dl/dP_i.  Every other column: 0.
 *   lines      col 3 x: -dl/db_l b_l / x;  col 5 tau: -dl/db_l b_l / tau;  col 6 shift: dl/dshift_l.  Cols 0, 1, 2, 4: 0.  Row k
 *              of the screen contributes exactly 0 to line k's own columns.  A line whose ids are not buses of the grid gets a NaN row.
 *   generators col 6 Pg: dl/dP at its bus.  Every other column: 0.
 *   rating is a constant.  A solved row whose incoming gradients are all exactly zero is skipped.
 *   Failure: a row the forward left NaN / -1 (an islanding outage, a non-finite update) contributes nothing when its incoming
 *   gradients are all exactly zero or NULL; it is skipped, never multiplied by zero.  Otherwise, or when a lambda_k is not finite,
 *   all three gradient rows of that grid are NaN.  A grid with converged == 0 (or whose base solve fails here) gets NaN rows unless
 *   all its incoming gradients are exactly zero, and zero rows then.  Other grids are unaffected.
 *   fp64 throughout, rounded once to fp32.  No atomics, every sum in a fixed order: a grid's gradient is bit-identical alone, in
 *   any batch and from run to run for the same outage list.  The order and the chunking of the list set the order of the sums
 *   over outages, so another order of the same outages may change the last bits.
 *
 * Kernels (gns_dcn1.hip): one wave per (grid, chunk of Wa outages) with the screen's prologue; lane j solves z_k as the screen
 * does, fills q_k into its own column of a second right-hand-side array in line order, solves u_k and forms lambda_k; a last pass
 * walks the chunk's outages in order with a line per lane (dl/db, sum of w) and a bus per lane (dl/dP) and stores the chunk's
 * partial.  A second kernel, a wave per grid, sums the chunks' partials in order, applies the contract and writes the outputs.
 * LDS image (gns_dcn1_adjoint_lds_bytes): 8 * (nnz_lu_p + dim_p + N + 3 E + 2 dim_p (Wa + 1) + 3 Wa) bytes, the screen's image at
 * width Wa, the second array [dim_p][Wa + 1] and three doubles per outage; Wa is the largest power of two up to 64 whose image fits
 * GNS_PF_LDS_MAX_BYTES (1 when none does: the image reported is then Wa = 1's).  Workspace (gns_dcn1_adjoint_workspace_bytes):
 * Bt * ceil(n_outage / Wa) partials of N + 2 E + 1 doubles (dl/dP, dl/db, the sum of w, a status), rounded up to 256 bytes.
 *
 * Errors: as gns_dcn1_screen, with worst_line and converged in place of its outputs (GNS_EINVAL when NULL) and Wa in place of W;
 * GNS_EUNSUPPORTED for an adjoint LDS image above GNS_PF_LDS_MAX_BYTES (from the workspace query too); then, when an output is
 * asked for, GNS_EINVAL for a NULL workspace and GNS_ESIZE for a short one.  Every refusal comes before any launch; nothing is
 * allocated and the host is not synchronised. */
int gns_dcn1_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes /* Wa; may be NULL */);
int gns_dcn1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage, size_t* bytes);
int gns_dcn1_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                     const double* rating, int32_t rating_per_grid,
                     const int32_t* worst_line, const uint8_t* converged,
                     const double* grad_line_flow, const double* grad_worst_loading,
                     float* grad_buses, float* grad_lines, float* grad_generators,
                     void* workspace, size_t workspace_bytes, void* stream);

/* DC N-2 contingency screening: the post-outage DC flows of a list of double-line outages (an N-2 set) of every grid of a batch,
 * from the base factorisation alone.  Two lines out are a rank-2 change of Bbus[r, r]: the single-line solves of "DC contingency
 * screening" above, one per distinct line of the list, and a 2x2 system per pair give the exact flows.
 *
 * Semantics (notation of "DC contingency screening": A = Bbus[r, r]; m_l = (e_f - e_t)_r; A z_c = m_c on the base factor; F_l the
 * base flow; fp64 throughout).  Let H_c[l] = z_c[f_l] - z_c[t_l], with z taken as 0 at the slack.  For a pair of lines j < k (the
 * kernel orders the two lines itself, so (k, j) gives the same bits as (j, k)):
 *   m11 = 1 - b_j H_j[j]      m12 = -b_j H_k[j]
 *   m21 = -b_k H_j[k]         m22 = 1 - b_k H_k[k]
 *   det = m11 m22 - m12 m21
 *   a_j = (F_j m22 - m12 F_k) / det
 *   a_k = (m11 F_k - m21 F_j) / det
 *   F'_l = F_l + b_l (H_j[l] a_j + H_k[l] a_k)   for l not in {j, k};   F'_j = F'_k = 0
 *   (with theta' = theta + Z a, Z = [z_j z_k], the flows of the two lines must vanish: (I - diag(b) M^T Z) a = F_S).  A line from
 *   a bus to itself has m = 0 and changes nothing.
 *   worst_loading = max_l |F'_l| / rating_l (rating NULL: 1) and worst_line the 0-based line that attains it, the lowest of equals,
 *   by the total order of the N-1 screen's reduction (NaN is worst of all).
 *   Islanding: a pair that disconnects the graph has det = 0 in exact arithmetic.  The kernel does not decide that numerically: the
 *   caller passes islanding[n_pair] (1: j is a bridge, or k is a bridge of the graph without j).  Those rows get NaN in line_flow
 *   and worst_loading and -1 in worst_line, in every grid.
 *   Failure: a grid whose base solve fails (converged = 0, as gns_dc_solve decides it) gets NaN / -1 in every row; a pair one of
 *   whose z_c is not finite, or whose det, a_j or a_k is not finite (or whose det is zero) gets NaN / -1 alone.
 *   Every (grid, pair) row is bit-identical alone, in any batch, in any pair list or order that holds it (duplicates are independent
 *   rows), in either order of its two lines, and from run to run: no atomics, the reductions in a fixed order.
 *
 * Inputs: cand [n_cand] int32, the distinct lines that occur in the pairs, ascending, on the host (checked before the launch) and
 * on the device; pair_cols [n_pair,2] int32, each pair as two positions into cand, on the host and on the device; islanding [n_pair]
 * uint8 on the device; rating NULL, [E] (rating_per_grid 0) or [Bt,E] (1) fp64 on the device.
 * Outputs: line_flow [Bt,n_pair,E] fp64, or NULL for the summaries alone (8 Bt n_pair E bytes not written); worst_loading
 * [Bt,n_pair] fp64; worst_line [Bt,n_pair] int32; converged [Bt] uint8, the base solve's.
 *
 * Kernels (gns_dcn2_device.h, the pair as gns_dcn2.hip's row model).  Factor: one wave per (grid, chunk of W candidate lines) with the N-1 screen's prologue, LDS image and
 * lane solve (gns_dcn1_device.h), so z_c is that screen's bit for bit; a pass with a line per lane then stores H_c[0 .. E)
 * contiguously into the workspace with a finite flag per candidate, and chunk 0 also stores F_l, b_l and the grid's status.  Its LDS
 * image and W are gns_dcn1_lds_bytes' (gns_dcn2_lds_bytes reports them).  Pair: one wave per (grid, chunk of Q consecutive pairs), F,
 * b and the rating in LDS (24 E bytes); per pair the six scalars above are computed identically on every lane, a line per lane
 * forms F'_l from the two H rows, and the wave reduction of the N-1 screen finishes the row.  Q comes from n_pair alone (32 from
 * 8192 pairs on, else 8).  Workspace (gns_dcn2_workspace_bytes): Bt * (n_cand * E + 2 E + n_cand + 1) doubles (H, F, b, the flags,
 * the status), rounded up to 256 bytes.
 *
 * Errors: GNS_EINVAL for a NULL cfg, blob, input, cand, pair_cols, islanding mask, output other than line_flow or workspace, a blob
 * that is not an FD blob or whose N, E, Gn are not cfg's, n_cand <= 0 or n_pair <= 0, a candidate outside 0 .. E-1, cand not
 * ascending or not distinct, a column outside 0 .. n_cand-1, a pair with equal columns, rating_per_grid outside {0, 1}, or Bt, or
 * Bt times the chunks of either kernel, above 2^31 - 1; GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES; GNS_ESIZE
 * for a short workspace.  GNS_EINVAL wins over GNS_EUNSUPPORTED, which wins over GNS_ESIZE (a NULL workspace is looked at with its
 * size).  Every refusal comes before any launch; nothing is allocated and the host is not synchronised.
 * Gradients: gns_dcn2_adjoint, below.  The AC solve of chosen pairs: gns_acn2_screen.  Generator outages, alone or with a line:
 * "DC generator contingency screening", below.  Not here: batches that mix topologies. */
int gns_dcn2_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes /* W; may be NULL */);
int gns_dcn2_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_cand, size_t* bytes);
int gns_dcn2_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const int32_t* cand_host, const int32_t* cand_dev, int32_t n_cand,
                    const int32_t* pair_cols_host, const int32_t* pair_cols_dev, int32_t n_pair, const uint8_t* islanding,
                    const double* rating, int32_t rating_per_grid,
                    double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Gradients of the N-2 screen.  gns_dcn2_adjoint takes the inputs of a gns_dcn2_screen call (the same candidate and pair lists,
 * islanding mask and rating), its outputs worst_line [Bt,n_pair] and converged [Bt], and the incoming gradients of a loss of its two
 * fp64 outputs: grad_line_flow [Bt,n_pair,E] and grad_worst_loading [Bt,n_pair] (each may be NULL: zero).  It writes dl/d(input)
 * into grad_buses [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32, each of which may be NULL (not computed; with all
 * three NULL nothing is launched).  Every element of each non-NULL output is written (overwritten, not accumulated).  The row state is
 * recomputed from the inputs, not kept by the forward.
 *
 * Method, per grid, with A = Bbus[r, r], z_c = A^-1 m_c and H_c[l] = m_l^T z_c of candidate c (the forward's rows), and per pair
 * S = (j, k) the forward's M = I - diag(b_S) H[S,S], a = M^-1 F_S and F'_l = F_l + b_l (H_j[l] a_j + H_k[l] a_k):
 *   G_l = grad_line_flow[l] plus, at l = worst_line, grad_worst_loading sign(F'_w) / rating_w; G_j = G_k = 0.
 *   Per pair: gF_l += G_l;  ga = sum_l G_l b_l (H_j[l], H_k[l]);  v = M^-T ga;  gF_j += v_j, gF_k += v_k;
 *   T'_c[l] += G_l a_c for c in S, and T'_c[e_r] += v_r a_c at the two outaged lines e_r (the derivative of M).
 *   Per grid: y_0 = A^-1 sum_l gF_l b_l m_l and y_c = A^-1 sum_l b_l T'_c[l] m_l, one solve on the base factor per candidate and
 *   one more;  w_l = gF_l - m_l^T y_0;  dl/db_l = w_l (theta_f - theta_t - shift_l) + sum_c H_c[l] (T'_c[l] - m_l^T y_c);
 *   dl/dP = y_0;  dl/dshift_l = -b_l w_l.  At most n_cand + 1 solves for the gradient and the n_cand solves and the base case that
 *   recompute the forward's state; nothing is factored or solved per pair, and with grad_line_flow NULL a pair is O(1) work.
 *
 * Contract (gns_dcn1_adjoint's): buses cols 2, 4 (Pd, Gs); lines cols 3, 5, 6 (x, tau, shift); generators col 6 (Pg); every other
 *   column exactly 0.  rating is a constant; a tie in the worst loading goes to the worst_line the forward reported.  A row the
 *   forward left NaN / -1 (an islanding pair, a non-finite 2x2 update) is skipped when its incoming gradients are exactly zero or
 *   NULL, never multiplied by zero; with a non-zero incoming gradient, or a non-finite solve, the grid's three gradient rows are NaN.
 *   A grid with converged == 0 gets NaN rows when an incoming gradient of it is non-zero, zero rows otherwise.  Other grids are
 *   unaffected.  Row (j, k) contributes 0 to the own columns of lines j and k.  The sums over pairs run through shared solves, in
 *   which a row's contribution to its own two lines cancels to rounding (of the order of 1e-16 of the row's other entries); the
 *   columns of a line are therefore the sum over the contributing rows that do not hold it plus that rounding, and a line that every
 *   contributing row of the grid holds (the sum over the others is empty: a single row, rows that share a line) gets exactly 0.
 *   fp64 throughout, rounded once to fp32.  No atomics, every sum in a fixed order: a grid's gradient is bit-identical alone, in any
 *   batch and from run to run for the same pair list, and (k, j) gives the bits of (j, k); another order of the list may change the
 *   last bits.
 *
 * Kernels (gns_dcn2_device.h), five launches: the forward's factor kernel again, into the adjoint's own workspace (the pool is reused
 * between forward and backward, so nothing of the forward's is read); a pair kernel, one wave per (grid, chunk of Q pairs, the
 * forward's Q), 32 E bytes of LDS, which writes a record of 6 doubles per (grid, pair) (a, v, the worst-line term, whether the row
 * contributes and its worst line) and the chunk's partial of gF; a gather kernel, one wave per (grid, candidate), 8 E bytes of LDS,
 * which scans the pair list 64 pairs at a time and sums T'_c over the pairs that hold its candidate in list order, lane l mod 64
 * owning line l, and counts the contributing pairs that do not hold it; a solve kernel, one wave per (grid, chunk of W columns: column 0 is y_0, column c + 1 candidate c) on the N-1
 * adjoint's LDS image and width (gns_dcn1_adjoint_lds_bytes; gns_dcn2_adjoint_lds_bytes reports the larger of that image and
 * 32 E), lane j running the solve program on its column; and gns_dcn1_adjoint's reduce kernel over the chunks' partials.
 * Workspace (gns_dcn2_adjoint_workspace_bytes): gns_dcn2_workspace_bytes' figure, plus
 * Bt * (n_cand * E + 6 n_pair + ceil(n_pair / Q) * (E + 1) + E + n_cand + ceil((n_cand + 1) / W) * (N + 2 E + 1)) doubles and Bt bytes,
 * rounded up to 256 bytes.
 *
 * Errors, in order (gns_dcn1_adjoint's): GNS_EINVAL for what gns_dcn2_screen refuses with it, a NULL worst_line or converged, or
 * Bt times the chunks of any kernel, or Bt * n_cand, above 2^31 - 1; then GNS_EUNSUPPORTED for an LDS image above
 * GNS_PF_LDS_MAX_BYTES (from the workspace query too); then, when an output is asked for, GNS_EINVAL for a NULL workspace and
 * GNS_ESIZE for a short one.  Every refusal comes before any launch; nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, second derivatives.  Generator outages: "DC generator contingency screening", below. */
int gns_dcn2_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes /* W; may be NULL */);
int gns_dcn2_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_cand, int32_t n_pair,
                                     size_t* bytes);
int gns_dcn2_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const int32_t* cand_host, const int32_t* cand_dev, int32_t n_cand,
                     const int32_t* pair_cols_host, const int32_t* pair_cols_dev, int32_t n_pair, const uint8_t* islanding,
                     const double* rating, int32_t rating_per_grid,
                     const int32_t* worst_line, const uint8_t* converged,
                     const double* grad_line_flow, const double* grad_worst_loading,
                     float* grad_buses, float* grad_lines, float* grad_generators,
                     void* workspace, size_t workspace_bytes, void* stream);

/* DC generator contingency screening: the post-outage DC flows of a list of generator outages, each alone or with one line out as
 * well (the combined N-1 set: a unit out plus a line out), of every grid of a batch, from the base factorisation alone.  A generator
 * outage changes the injections, not the matrix: it is one more solve on the base factor per distinct generator of the list.  The
 * line on top of it is the rank-1 update of "DC contingency screening" above, from one single-line solve per distinct line.
 *
 * Semantics (the base case of "DC power flow": theta, F_l, b_l, Bbus; notation of "DC contingency screening": A = Bbus[r, r],
 * A z_k = m_k on the base factor; fp64 throughout).  A row is (g, k): g a 0-based generator row, k a 0-based line or -1 for "no
 * line out".
 *   Generator g out: its Pg_g (column 6) leaves its bus m_g.  With pickup weights w_h >= 0 (per grid or shared) and W_g the sum of
 *   w_h over h != g in generator-index order, every other generator h gains Pg_g * (w_h / W_g) at its bus when W_g > 0; when
 *   W_g == 0 (every remaining weight exactly zero) or pickup is NULL nothing is redistributed and the slack picks the loss up, which
 *   is what dcpf does with a unit whose Pg is set to 0.  dP is the resulting change of the bus injections: -Pg_g at m_g first, then
 *   the shares in generator-index order.  No Pmax or Pmin limit is enforced on the units that pick up.
 *     A u_g = dP_r on the base factor, u_g = 0 at the slack
 *     D_g[l] = u_g[f_l] - u_g[t_l]
 *     Fg_l = F_l + b_l * D_g[l]
 *   Row (g, -1): F'_l = Fg_l.
 *   Row (g, k), with H_k[l] = z_k[f_l] - z_k[t_l] and z_k exactly as the N-1 and N-2 screens make it:
 *     den = 1 - b_k * H_k[k]
 *     alpha = Fg_k / den
 *     F'_l = Fg_l + (b_l * H_k[l]) * alpha   for l != k;   F'_k = 0
 *   with exactly this association of the operations (the build has -ffp-contract=off, so the bits are determined).  A line from a
 *   bus to itself has m = 0 and changes nothing.
 *   worst_loading = max_l |F'_l| / rating_l (rating NULL: 1) and worst_line the 0-based line that attains it, the lowest of equals,
 *   by the total order of the N-1 screen's reduction (NaN is worst of all).
 *   Islanding: a generator outage never islands; row (g, k) islands exactly when k is a bridge.  The kernel does not decide that
 *   numerically: the caller passes islanding[n_row].  Those rows get NaN in line_flow and worst_loading and -1 in worst_line, in
 *   every grid.
 *   Failure: a grid whose base solve fails (converged = 0, as gns_dc_solve decides it) gets NaN / -1 in every row; a row whose u_g,
 *   z_k, den or alpha is not finite, or whose den is zero, gets NaN / -1 alone.
 *   Every (grid, row) is bit-identical alone, in any batch, in any list or order that holds it (duplicates are independent rows) and
 *   from run to run: no atomics, the reductions in a fixed order.
 *   From the definition: where Pg_g is exactly 0, or g sits on the slack bus and pickup is NULL, dP_r is zero, so row (g, -1) is the
 *   base line_flow and row (g, k) is row k of gns_dcn1_screen, bit for bit.
 *
 * Inputs: line_list [n_line] int32, the distinct lines of the rows, ascending (n_line may be 0: then the two pointers may be NULL),
 * and gen_list [n_gen] int32, the distinct generators of the rows, ascending, each on the host (checked before the launch) and on
 * the device; row_cols [n_row,2] int32, each row as a position into gen_list and a position into line_list or -1, on the host and
 * on the device; islanding [n_row] uint8 on the device; rating NULL, [E] (rating_per_grid 0) or [Bt,E] (1) fp64 on the device;
 * pickup NULL, [Gn] (pickup_per_grid 0) or [Bt,Gn] (1) fp64 on the device, by generator row (not by position into gen_list).
 * Outputs: line_flow [Bt,n_row,E] fp64, or NULL for the summaries alone (8 Bt n_row E bytes not written); worst_loading [Bt,n_row]
 * fp64; worst_line [Bt,n_row] int32; converged [Bt] uint8, the base solve's.
 *
 * Kernels (gns_dcn2_device.h, the two kernels of the N-2 screen with gns_dcg1.hip's row model).  Factor: one wave per (grid, chunk of W candidates), the candidates
 * being line_list followed by gen_list (n_cand = n_line + n_gen), with the N-1 screen's prologue, LDS image and lane solve
 * (gns_dcn1_device.h): a line lane solves z_k as that screen does, bit for bit; a generator lane zeroes its column, writes dP_r (the
 * bus of a generator from the blob's by-bus generator lists) and runs the same solve program.  A pass with a line per lane then
 * stores z[f_l] - z[t_l] of every candidate (H_k, D_g) contiguously into the workspace with a finite flag per candidate, and chunk 0
 * also stores F_l, b_l and the grid's status.  Its LDS image and W are gns_dcn1_lds_bytes' (gns_dcg1_lds_bytes reports them).  Row:
 * one wave per (grid, chunk of Q consecutive rows), F, b and the rating in LDS (24 E bytes); per row den and alpha are computed
 * identically on every lane, a line per lane forms F'_l from the two contiguous workspace rows, and the wave reduction of the N-1
 * screen finishes the row.  Q comes from n_row alone (32 from 8192 rows on, else 8).  Workspace (gns_dcg1_workspace_bytes), the N-2
 * screen's layout: Bt * (n_cand * E + 2 E + n_cand + 1) doubles (the candidates' rows, F, b, the flags, the status), rounded up to
 * 256 bytes.
 *
 * Errors: GNS_EINVAL for a NULL cfg, blob, input, gen_list, row_cols, islanding mask, output other than line_flow or workspace, a
 * NULL line_list with n_line > 0, a blob that is not an FD blob or whose N, E, Gn are not cfg's, n_line < 0 or above E, n_gen <= 0
 * or above Gn, n_row <= 0, a line outside 0 .. E-1 or a generator outside 0 .. Gn-1, a list not ascending or not distinct, a
 * generator column outside 0 .. n_gen-1, a line column outside -1 .. n_line-1, rating_per_grid or pickup_per_grid outside {0, 1}, or
 * Bt, or Bt times the chunks of either kernel, above 2^31 - 1; GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES;
 * GNS_ESIZE for a short workspace.  GNS_EINVAL wins over GNS_EUNSUPPORTED, which wins over GNS_ESIZE (a NULL workspace is looked at
 * with its size).  Every refusal comes before any launch; nothing is allocated and the host is not synchronised.  The values of
 * pickup are the caller's to check (non-negative, finite): the kernel reads them as they are.
 * Gradients: gns_dcg1_adjoint, below.  The AC screen of the same rows: gns_acg1_screen, "AC generator contingency screening" below.
 * Not here: limits on the units that pick up, batches that mix topologies, a generator plus two lines. */
int gns_dcg1_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes /* W; may be NULL */);
int gns_dcg1_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_line, int32_t n_gen, size_t* bytes);
int gns_dcg1_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const int32_t* line_host, const int32_t* line_dev, int32_t n_line,
                    const int32_t* gen_host, const int32_t* gen_dev, int32_t n_gen,
                    const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                    const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                    double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Gradients of the DC generator screen.  gns_dcg1_adjoint takes the inputs of a gns_dcg1_screen call (the same three lists,
 * islanding mask, rating and pickup), its outputs worst_line [Bt,n_row] and converged [Bt], and the incoming gradients of a loss
 * of its two fp64 outputs: grad_line_flow [Bt,n_row,E] and grad_worst_loading [Bt,n_row] (each may be NULL: zero).  It writes
 * dl/d(input) into grad_buses [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32 and dl/d(pickup) into grad_pickup
 * [Bt,Gn] fp64 (per grid also when pickup is shared: the caller sums), each of which may be NULL (not computed; with all four NULL
 * nothing is launched).  Every element of each non-NULL output is written (overwritten, not accumulated).  The row state is
 * recomputed from the inputs, not kept by the forward.
 *
 * Method, per grid, in the notation of "DC generator contingency screening": row (g, k) is the N-1 screen's row k at the
 * injections P + dP_g, dP_g = Pg_g c_g with c_g = -e_{m_g} + sum_{h != g} (w_h / W_g) e_{m_h} on the non-slack buses (the sum only
 * with a pickup and W_g > 0).
 *   G_l = grad_line_flow[l] plus, at l = worst_line, grad_worst_loading sign(F'_w) / rating_w; G_k = 0.
 *   Row (g, -1): gFg_l = G_l.  Row (g, k): ga = sum_l G_l b_l H_k[l], v = ga / den, gFg_l = G_l for l != k and gFg_k = v;
 *   T_k[l] += G_l alpha for l != k and T_k[k] += v alpha (the derivative of den).  Every row: gF_l += gFg_l and S_g[l] += gFg_l.
 *   Per grid: y_0 = A^-1 sum_l gF_l b_l m_l, y_k = A^-1 sum_l b_l T_k[l] m_l per distinct line and y_g = A^-1 sum_l b_l S_g[l] m_l
 *   per distinct generator: n_line + n_gen + 1 solves on the base factor, and the n_line + n_gen solves and the base case that
 *   recompute the forward's state; nothing is factored or solved per row, and with grad_line_flow NULL a row is O(1) work.
 *   w_l = gF_l - m_l^T y_0;  dl/db_l = w_l (theta_f - theta_t - shift_l) + sum_k H_k[l] (T_k[l] - m_l^T y_k)
 *   + sum_g D_g[l] (S_g[l] - m_l^T y_g);  dl/dshift_l = -b_l w_l;  dl/dP = y_0, sent to Pd, Gs and Pg as gns_dcn1_adjoint sends it;
 *   dl/dPg_g += c_g^T y_g for each generator of the list;  dl/dw_h = sum over the listed g != h with W_g > 0 of
 *   (Pg_g / W_g) (y_g[m_h] - sum_{h' != g} (w_h' / W_g) y_g[m_h']), y_g = 0 at the slack bus.  The branch W_g == 0 (the slack
 *   picks up) is not differentiated: it gives exactly 0 to the weights.
 *
 * Contract (gns_dcn2_adjoint's): buses cols 2, 4 (Pd, Gs); lines cols 3, 5, 6 (x, tau, shift); generators col 6 (Pg); every other
 *   column exactly 0.  rating is a constant; a tie in the worst loading goes to the worst_line the forward reported.  A row the
 *   forward left NaN / -1 is skipped when its incoming gradients are exactly zero or NULL, never multiplied by zero; with a
 *   non-zero incoming gradient, or a non-finite solve, the grid's gradient rows are NaN, grad_pickup's row included.  A grid with
 *   converged == 0 gets NaN rows when an incoming gradient of it is non-zero, zero rows otherwise.  Other grids are unaffected.
 *   Row (g, k) contributes 0 to the own columns of line k: exactly when every contributing row of the grid holds k, else the row's
 *   own part cancels to rounding in the shared solves.  fp64 throughout, rounded once to fp32; grad_pickup stays fp64.  No
 *   atomics, every sum in a fixed order: a grid's gradient is bit-identical alone, in any batch and from run to run for the same
 *   list; another order of the list may change the last bits.
 *
 * Kernels (gns_dcn2_device.h and gns_dcg1.hip), five launches, those of gns_dcn2_adjoint but for the last: the forward's factor kernel again, into the adjoint's own
 * workspace; a row kernel, one wave per (grid, chunk of Q rows, the forward's Q), 32 E bytes of LDS, which writes a record of 4
 * doubles per (grid, row) (alpha, v, the worst-line term, whether the row contributes and its worst line) and the chunk's partial
 * of gF; a gather kernel, one wave per (grid, candidate), 8 E bytes of LDS, which scans the row list 64 rows at a time and sums T_k
 * or S_g over the rows that hold its candidate in list order, lane l mod 64 owning line l; the N-2 adjoint's solve kernel
 * (gns_dcn2_device.h), one wave per (grid, chunk of W columns: y_0, the lines, the generators) on the N-1 adjoint's LDS image and
 * width, which also stores y_g by bus; and a reduce kernel, gns_dcn1_adjoint's sums and contract with the Pg and w terms of the
 * generators.  LDS (gns_dcg1_adjoint_lds_bytes): max(8 * (nnz_lu_p + dim_p + N + 3 E + 2 dim_p (W + 1) + 3 W), 32 E) bytes.
 * Workspace (gns_dcg1_adjoint_workspace_bytes): gns_dcg1_workspace_bytes' figure, plus, with n_cand = n_line + n_gen,
 * Bt * (n_cand * E + 4 n_row + ceil(n_row / Q) * (E + 1) + E + n_cand + ceil((n_cand + 1) / W) * (N + 2 E + 1) + n_gen * N + 3 n_gen)
 * doubles and Bt bytes, rounded up to 256 bytes.
 *
 * Errors, in order (gns_dcn2_adjoint's): GNS_EINVAL for what gns_dcg1_screen refuses with it, a NULL worst_line or converged, or
 * Bt times the chunks of any kernel, or Bt * n_cand, above 2^31 - 1; then GNS_EUNSUPPORTED for an LDS image above
 * GNS_PF_LDS_MAX_BYTES (from the workspace query too); then, when an output is asked for, GNS_EINVAL for a NULL workspace and
 * GNS_ESIZE for a short one.  Every refusal comes before any launch; nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, limits on the pickup, a generator with two lines, second derivatives. */
int gns_dcg1_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes /* W; may be NULL */);
int gns_dcg1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_line, int32_t n_gen,
                                     int32_t n_row, size_t* bytes);
int gns_dcg1_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const int32_t* line_host, const int32_t* line_dev, int32_t n_line,
                     const int32_t* gen_host, const int32_t* gen_dev, int32_t n_gen,
                     const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                     const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                     const int32_t* worst_line, const uint8_t* converged,
                     const double* grad_line_flow, const double* grad_worst_loading,
                     float* grad_buses, float* grad_lines, float* grad_generators, double* grad_pickup,
                     void* workspace, size_t workspace_bytes, void* stream);

/* AC contingency screening: Newton-Raphson on every grid of a batch with each single line of a list out of service (an N-1 set),
 * with the post-outage state, the branch flows at both ends of every line and their summaries, from the base analysis alone.
 *
 * Semantics (the Newton-Raphson section at the top of this file is the base case: inputs, bus roles, Y-bus, injections, fp64)
 *   Row (grid, k) is Newton-Raphson on the grid without line outages[k]: its Y-bus is the sum of the line stamps with that line's
 *   four skipped (each entry a sum in stamp order, never a subtraction: the values gns_pf_solve computes on the grid with the line
 *   row deleted); injections, bus roles and the vg set points are the base case's.  The outage removes entries from the Jacobian
 *   and adds none, so the blob of the base topology serves every row: its factor slots and its program, with numeric zeros where an
 *   entry lost its only line.  Nothing is analysed or allocated per outage.
 *   Start: the warm start of gns_pf_solve from base_v, base_theta (the outputs of gns_pf_solve on the same inputs): |V| at PQ buses
 *   from base_v, theta = base_theta - base_theta[slack]; |V| at PV / slack buses from vg.  The convergence test (||F||_inf < tol
 *   before every update), the update, max_iter and the failure rules are gns_pf_solve's, per row: a row that does not converge, or
 *   stops at a zero or non-finite pivot, mismatch or iterate, has converged = 0 and keeps its last finite iterate (mismatch NaN
 *   when the mismatch itself is not finite); its flows and summaries are computed from that iterate.
 *   Branch flows (MATPOWER's branch model on the stamps of makeYbus, Y_ff = (y_s + jb/2)/tau^2, Y_tt = y_s + jb/2,
 *   Y_ft = -y_s/conj(a), Y_tf = -y_s/a of the line alone):  S_f = V_f conj(Y_ff V_f + Y_ft V_t),  S_t = V_t conj(Y_tf V_f + Y_tt V_t);
 *   p_from + j q_from = S_f, p_to + j q_to = S_t, all four exactly 0 at the outaged line.  The line's buses are read from its id
 *   columns, which must be those the blob was prepared from (a line whose ids are not buses of the grid gets NaN flows).
 *   worst_loading = max_l max(|S_f|, |S_t|) / rating_l (rating NULL: 1) and worst_line the 0-based line that attains it; v_min, v_max
 *   the extremes of |V| over the buses and v_min_bus, v_max_bus the 0-based buses that attain them; the lowest index among equals.
 *   A NaN loading or voltage wins its summary, at the lowest index that holds one: the value is NaN, the index that line or bus.
 *   Islanding: the caller finds the outages that disconnect the graph (the bridges of the topology) and passes islanding[n_outage]
 *   (1: bridge); the kernel does not decide that numerically.  Those rows get NaN in every fp64 output, -1 in worst_line, v_min_bus,
 *   v_max_bus and iterations, and converged = 0, in every grid.  So does every row of a grid with base_converged = 0, and a row
 *   whose line's id columns do not name an entry of the blob's Y-bus pattern.  Other rows are unaffected.
 *   Every (grid, outage) row is bit-identical alone, in any batch, for any outage list or order that holds the outage (duplicates
 *   are independent rows), and from run to run: no atomics, the reductions by a total order.
 *   Gradients: gns_acn1_adjoint, below.  Double outages: gns_acn2_screen, "AC N-2 contingency screening" below.  Generator outages,
 *   alone or with a line: gns_acg1_screen, "AC generator contingency screening" below.  Not here: batches that mix topologies (one
 *   blob per call), generator reactive limits.
 *
 * Inputs: outages as 0-based line indices, on the host (checked before the launch) and on the device (read by the kernel), both
 * [n_outage] int32; islanding [n_outage] uint8 on the device; rating NULL, [E] (rating_per_grid 0) or [Bt,E] (1) fp64 on the device;
 * base_v, base_theta [Bt,N] fp64 and base_converged [Bt] uint8 on the device.  cfg: max_iter and tol as in gns_pf_solve.
 * Outputs (row r = grid * n_outage + position in the list): v, theta [Bt,n_outage,N] and p_from, q_from, p_to, q_to
 * [Bt,n_outage,E] fp64, each of which may be NULL (not written); worst_loading, v_min, v_max, mismatch fp64, worst_line, v_min_bus,
 * v_max_bus, iterations int32, converged uint8 (0/1), all [Bt,n_outage].
 *
 * Kernels (gns_acn1.hip): a wave per grid writes the base Y-bus of every grid to the workspace once; then one wave per (grid,
 * outage) with gns_pf_solve's LDS image (gns_pf_info.lds_bytes) reads its grid's base Y-bus and holds the at most four entries its
 * line touches (ff, tt, ft, tf) in registers, recomputed from their stamps without the line.  After the iteration a line per lane
 * computes the flows and the summaries are reduced over the wave.  Workspace (gns_acn1_workspace_bytes): the base Y-bus, 16 bytes
 * per structural nonzero and GRID (gns_pf_workspace_bytes' figure, whatever n_outage is).
 *
 * Errors: GNS_EINVAL for a NULL cfg, blob, input, outage list, islanding mask, base_v, base_theta, base_converged, workspace or
 * output other than v, theta and the four flows, a negative max_iter or tol, a blob that is not a Newton-Raphson blob or whose N, E,
 * Gn are not cfg's, n_outage <= 0, an outage outside 0 .. E-1, rating_per_grid outside {0, 1}, or Bt * n_outage above 2^31 - 1;
 * then GNS_ESIZE for a short workspace; then GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES.  Every refusal comes
 * before any launch; nothing is allocated and the host is not synchronised. */
int gns_acn1_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage, size_t* bytes);
int gns_acn1_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                    const double* rating, int32_t rating_per_grid,
                    const double* base_v, const double* base_theta, const uint8_t* base_converged,
                    double* v, double* theta, double* p_from, double* q_from, double* p_to, double* q_to,
                    double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus, double* v_max,
                    int32_t* v_max_bus, uint8_t* converged, int32_t* iterations, double* mismatch,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Gradients of the AC screen.  gns_acn1_adjoint takes the inputs of a gns_acn1_screen call (the same outage list, islanding mask and
 * rating), its outputs v, theta [Bt,n_outage,N], converged, worst_line, v_min_bus, v_max_bus [Bt,n_outage] and the base_converged
 * [Bt] it was given, and the incoming gradients of a loss of its nine fp64 outputs: grad_v, grad_theta [Bt,n_outage,N], grad_p_from,
 * grad_q_from, grad_p_to, grad_q_to [Bt,n_outage,E], grad_worst_loading, grad_v_min, grad_v_max [Bt,n_outage] (each may be NULL:
 * zero).  It writes dl/d(input) into grad_buses [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32, each of which may be
 * NULL (not computed; with all three NULL nothing is launched).  Every element of each non-NULL output is written (overwritten,
 * not accumulated).  The state is the forward's: Newton-Raphson is not run again, and the warm start is not differentiated (a
 * converged row does not depend on it).
 *
 * Method, per solved row (grid, k): the implicit function theorem on the grid without line k, F_k(x, p) = 0 with the unknowns x of
 * "Gradients" above (theta at PV+PQ, |V| at PQ) and J_k = dF_k/dx on the row's Y-bus.
 *   Effective cotangents: W_f,l = grad_p_from + j grad_q_from and W_t,l = grad_p_to + j grad_q_to of line l != k (line k's flows are
 *   the constant 0: its entries are ignored); grad_worst_loading adds (p + jq) / |S| / rating_w at w = worst_line to the end of the
 *   line that attains the maximum (the from end on equality; nothing at |S| = 0); grad_v_min and grad_v_max add to grad_v at
 *   v_min_bus and v_max_bus (a tie goes to the index the forward reported).
 *   Right-hand side: dl/dx = the theta and |V| cotangents at the unknowns plus the flows' derivatives, with A = V_f conj(Y_ft V_t),
 *   D = |V_f|^2 conj(Y_ff), B = V_t conj(Y_tf V_f), C = |V_t|^2 conj(Y_tt) (S_f = D + A, S_t = C + B) and dl = Re(conj(W) dS):
 *   dS_f/dtheta_f = jA = -dS_f/dtheta_t, dS_t/dtheta_t = jB = -dS_t/dtheta_f, |V_f| dS_f/d|V_f| = 2D + A, |V_t| dS_f/d|V_t| = A,
 *   |V_t| dS_t/d|V_t| = 2C + B, |V_f| dS_t/d|V_f| = B.
 *   Solve: J_k^T lambda = dl/dx; J_k is factored by the leading factor steps of the blob's program, then the transposed program
 *   (PH_T_*) runs, exactly as in gns_pf_adjoint.  One factorisation and one transposed solve per row.
 *   Gradients: dl/dp = direct - lambda^T dF_k/dp.  The line columns reuse gns_pf_adjoint's stamp algebra with Lambda_f - W_f,l and
 *   Lambda_t - W_t,l in place of Lambda_f, Lambda_t of line l (the flow term is +Re(conj(W) S) on the line's own stamps where the
 *   mismatch term is -Re(conj(Lambda) S)); vg gets the total direct dl/d|V_b| (the state cotangent plus the flows' dependence on
 *   |V_b|) minus lambda^T dF_k/d|V_b|.  Summed over the rows of the list.
 *
 * Contract (gns_pf_adjoint's columns): buses cols 2-5 (Pd, Qd, Gs, Bs); lines cols 2-6 (r, x, b, tau, shift); generators col 6 Pg
 *   and col 4 vg of the first generator listed on a PV / slack bus.  Every other column: 0.  Row k of the screen contributes
 *   exactly 0 to line k's own columns.  A line whose id columns are not buses of the grid gets a NaN row.  rating is a constant.
 *   Failure: a row whose incoming gradients are all exactly zero or NULL is skipped, never multiplied by zero (so a loss may mask
 *   out islanding and unconverged rows by indexing).  A row with converged == 0 (an islanding outage, a stopped or unconverged
 *   iteration, NaN / -1) and a non-zero incoming gradient, a zero or non-finite pivot, or a non-finite lambda: all three gradient
 *   rows of that grid are NaN.  A grid with base_converged == 0 gets NaN rows when an incoming gradient of it is non-zero, zero rows
 *   otherwise.  Other grids are unaffected.
 *   fp64 throughout, rounded once to fp32.  No atomics, every sum in a fixed order: a grid's gradient is bit-identical alone, in
 *   any batch and from run to run for the same outage list.  The order and the chunking of the list set the order of the sums
 *   over rows, so another order of the same outages may change the last bits.
 *
 * Kernels (gns_acn1.hip): the pre-kernel of the screen writes the base Y-bus per grid; then one wave per (grid, chunk of C consecutive
 * outages of the list) with gns_pf_solve's LDS image (gns_pf_info.lds_bytes; lambda in the Psp / Qsp vectors, the direct dl/d|V| in
 * the theta vector), so every topology the screen accepts the adjoint accepts.  The flow cotangents reach dl/dx by a gather with a
 * bus per lane: each bus walks the stamps of its diagonal entry, whose kinds 0 and 1 name every incident line and the end it
 * touches (a line from a bus to itself: once per end); no scatter.  The wave walks its chunk's rows in order and every lane adds
 * into the addresses it alone owns (a bus, a line or a generator per lane) of the chunk's fp64 partial in the workspace.  A second
 * kernel, a wave per grid, sums the chunks' partials in order, applies the contract, rounds once and writes every element.
 * C = min(8, max(1, ceil(n_outage / 32))): from the list's length alone, never from Bt.  Workspace
 * (gns_acn1_adjoint_workspace_bytes): the base Y-bus (gns_acn1_workspace_bytes' figure) plus Bt * ceil(n_outage / C) partials of
 * 4 N + 5 E + Gn + 1 doubles (per bus the sums of lambda_P, lambda_Q, |V|^2 lambda_P, |V|^2 lambda_Q; per line its five columns; per
 * generator dl/dvg; a status), each part rounded up to 256 bytes.
 *
 * Errors, in order: GNS_EINVAL for a NULL cfg, blob, input, outage list, islanding mask, v, theta, converged, worst_line, v_min_bus,
 * v_max_bus or base_converged, a negative max_iter or tol, a blob that is not a Newton-Raphson blob or whose N, E, Gn are not cfg's,
 * n_outage <= 0, an outage outside 0 .. E-1, rating_per_grid outside {0, 1}, or Bt * ceil(n_outage / C) above 2^31 - 1; then
 * GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES (from the workspace query too); then, when an output is asked for,
 * GNS_EINVAL for a NULL workspace and GNS_ESIZE for a short one.  Every refusal comes before any launch; nothing is allocated and
 * the host is not synchronised. */
int gns_acn1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_outage, size_t* bytes);
int gns_acn1_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const int32_t* outages_host, const int32_t* outages_dev, int32_t n_outage, const uint8_t* islanding,
                     const double* rating, int32_t rating_per_grid,
                     const double* v, const double* theta, const uint8_t* converged, const int32_t* worst_line,
                     const int32_t* v_min_bus, const int32_t* v_max_bus, const uint8_t* base_converged,
                     const double* grad_v, const double* grad_theta, const double* grad_p_from, const double* grad_q_from,
                     const double* grad_p_to, const double* grad_q_to, const double* grad_worst_loading,
                     const double* grad_v_min, const double* grad_v_max,
                     float* grad_buses, float* grad_lines, float* grad_generators,
                     void* workspace, size_t workspace_bytes, void* stream);

/* AC N-2 contingency screening: Newton-Raphson on every grid of a batch with each PAIR of lines of a list out of service at once (an
 * N-2 set), with the outputs of "AC contingency screening" above per (grid, pair), from the base analysis alone.
 *
 * Semantics: those of gns_acn1_screen with two lines out.  Row (grid, p) is Newton-Raphson on the grid without the lines
 *   pairs[p][0] and pairs[p][1]: its Y-bus is the sum of the line stamps with those two lines' eight skipped (each entry a sum in
 *   stamp order, never a subtraction: the values gns_pf_solve computes on the grid with both line rows deleted); injections, bus
 *   roles and the vg set points are the base case's.  Two outages remove entries from the Jacobian and add none, so the blob of the
 *   base topology serves every row, with numeric zeros where an entry lost its only lines (two parallel lines with no third).
 *   Nothing is analysed or allocated per pair.  The warm start from base_v, base_theta, the convergence test, the update, max_iter,
 *   the failure rules, the branch flows (all four exactly 0 at BOTH outaged lines), worst_loading / worst_line, v_min / v_max and
 *   their buses, and the order of the summaries (the lowest index among equals, NaN first) are gns_acn1_screen's, word for word.
 *   The two lines of a pair differ; either order of them is the same row bit for bit (the kernel orders them itself), and duplicate
 *   pairs are independent rows.  Lines may share a bus, be parallel, or run from a bus to itself.
 *   Islanding: the caller finds the pairs that disconnect the graph (one line a bridge of the topology, or the second a bridge of
 *   the graph without the first) and passes islanding[n_pair] (1: islanding); the kernel does not decide that numerically.  Those
 *   rows get NaN in every fp64 output, -1 in worst_line, v_min_bus, v_max_bus and iterations, and converged = 0, in every grid.  So
 *   does every row of a grid with base_converged = 0, and a row one of whose lines has id columns that do not name an entry of the
 *   blob's Y-bus pattern (nothing is read out of bounds for it).  Other rows are unaffected.
 *   Every (grid, pair) row is bit-identical alone, in any batch, for any pair list or order that holds the pair, in either order of
 *   its two lines, and from run to run: no atomics, the reductions by a total order.
 *   Gradients: gns_acn2_adjoint, below.  A generator with one line: gns_acg1_screen, "AC generator contingency screening" below.
 *   Not here: batches that mix topologies (one blob per call), a generator plus two lines, generator reactive limits.
 *
 * Inputs: gns_acn1_screen's, but for the list: pairs as 0-based line indices [n_pair,2] int32, on the host (checked before the
 * launch) and on the device (read by the kernel); islanding [n_pair] uint8 on the device.
 * Outputs (row r = grid * n_pair + position in the list): v, theta [Bt,n_pair,N] and p_from, q_from, p_to, q_to [Bt,n_pair,E] fp64,
 * each of which may be NULL (not written); worst_loading, v_min, v_max, mismatch fp64, worst_line, v_min_bus, v_max_bus, iterations
 * int32, converged uint8 (0/1), all [Bt,n_pair].
 *
 * Kernels (gns_acn2.hip): gns_acn1_screen's pre-kernel writes the base Y-bus of every grid to the workspace once; then one wave per
 * (grid, pair) with gns_pf_solve's LDS image (gns_pf_info.lds_bytes: every topology gns_acn1_screen accepts this call accepts) reads
 * its grid's base Y-bus and holds the at most eight entries its lines touch (ff, tt, ft, tf of each) in registers, the same in every
 * lane, each recomputed from its stamps without both lines; an entry both lines touch is held more than once with the same value.
 * Workspace (gns_acn2_workspace_bytes): the base Y-bus, gns_acn1_workspace_bytes' figure for the same Bt, whatever n_pair is.
 *
 * Errors: GNS_EINVAL for a NULL cfg, blob, input, pair list, islanding mask, base_v, base_theta, base_converged, workspace or
 * output other than v, theta and the four flows, a negative max_iter or tol, a blob that is not a Newton-Raphson blob or whose N, E,
 * Gn are not cfg's, n_pair <= 0, a line outside 0 .. E-1, a pair of twice the same line, rating_per_grid outside {0, 1}, or
 * Bt * n_pair above 2^31 - 1; then GNS_ESIZE for a short workspace; then GNS_EUNSUPPORTED for an LDS image above
 * GNS_PF_LDS_MAX_BYTES.  Every refusal comes before any launch; nothing is allocated and the host is not synchronised. */
int gns_acn2_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_pair, size_t* bytes);
int gns_acn2_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pair, const uint8_t* islanding,
                    const double* rating, int32_t rating_per_grid,
                    const double* base_v, const double* base_theta, const uint8_t* base_converged,
                    double* v, double* theta, double* p_from, double* q_from, double* p_to, double* q_to,
                    double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus, double* v_max,
                    int32_t* v_max_bus, uint8_t* converged, int32_t* iterations, double* mismatch,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Gradients of the AC N-2 screen.  gns_acn2_adjoint is gns_acn1_adjoint ("Gradients of the AC screen" above) with two lines out per
 * row.  It takes the inputs of a gns_acn2_screen call (the same pair list, islanding mask and rating), its outputs v, theta
 * [Bt,n_pair,N], converged, worst_line, v_min_bus, v_max_bus [Bt,n_pair] and the base_converged [Bt] it was given, and the incoming
 * gradients of a loss of its nine fp64 outputs: grad_v, grad_theta [Bt,n_pair,N], grad_p_from, grad_q_from, grad_p_to, grad_q_to
 * [Bt,n_pair,E], grad_worst_loading, grad_v_min, grad_v_max [Bt,n_pair] (each may be NULL: zero).  It writes dl/d(input) into
 * grad_buses [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32, each of which may be NULL (not computed; with all three
 * NULL nothing is launched).  Every element of each non-NULL output is written (overwritten, not accumulated).  The state is the
 * forward's: Newton-Raphson is not run again, and the warm start is not differentiated.
 *
 * Method, per solved row (grid, p) with j = min(pairs[p]), k = max(pairs[p]): gns_acn1_adjoint's, word for word, on the grid without
 * lines j and k: F_jk(x, p) = 0, J_jk = dF_jk/dx on the row's Y-bus (gns_acn2_screen's: each of the at most eight entries the lines
 * touch recomputed from its stamps without both lines), factored on the base analysis, one transposed solve.  What differs for two
 * lines: the flows of BOTH lines are the constant 0, so the entries of the four flow gradients at lines j and k are ignored, a
 * worst_line that is j or k (a forward's never is) gets nothing, and the row adds exactly 0 to the own columns of lines j and k.
 * Two parallel lines that are both out leave numeric zeros in the pattern; a line from a bus to itself and two lines that share a
 * bus are handled as in the forward.  The kernel orders the two lines itself: (k, j) and (j, k) give the same row contribution bit
 * for bit.
 *
 * Contract, failure rules and arithmetic: gns_acn1_adjoint's, with "pair" for "outage": gns_pf_adjoint's columns, every other column
 *   0; a line whose id columns are not buses of the grid gets a NaN row; rating is a constant.  A row whose incoming gradients are
 *   all exactly zero or NULL is skipped, never multiplied by zero.  A row with converged == 0 (an islanding pair, a stopped or
 *   unconverged iteration, NaN / -1) and a non-zero incoming gradient, a zero or non-finite pivot, or a non-finite lambda: all three
 *   gradient rows of that grid are NaN.  A grid with base_converged == 0 gets NaN rows when an incoming gradient of it is non-zero,
 *   zero rows otherwise.  Other grids are unaffected.  fp64 throughout, rounded once to fp32.  No atomics, every sum in a fixed
 *   order: a grid's gradient is bit-identical alone, in any batch, from run to run and with the two lines of any pair swapped, for
 *   the same pair list.  The order and the chunking of the list set the order of the sums over rows, so another order of the same
 *   pairs may change the last bits.
 *
 * Kernels (gns_acn2.hip): the screen's pre-kernel writes the base Y-bus per grid; then one wave per (grid, chunk of C consecutive
 * pairs of the list) with gns_pf_solve's LDS image, so every topology the screen accepts the adjoint accepts.  After the row's
 * prologue (its Y-bus view) the wave runs the routine gns_acn1_adjoint's kernel runs (acn_adjoint_row, gns_acn_adjoint_device.h), and
 * gns_acn1_adjoint's second kernel sums the chunks' partials (the same layout) in order.  C = max(1, ceil(n_pair / 64)): from the
 * list's length alone, never from Bt, and without gns_acn1_adjoint's cap of 8 rows per wave, so that a grid has at most 64 partials
 * however long the list (pair lists are long: every pair of case118 is 17 205 rows).  Workspace
 * (gns_acn2_adjoint_workspace_bytes): the base Y-bus (gns_acn2_workspace_bytes' figure) plus Bt * ceil(n_pair / C) partials of
 * 4 N + 5 E + Gn + 1 doubles, each part rounded up to 256 bytes.
 *
 * Errors, in order: GNS_EINVAL for a NULL cfg, blob, input, pair list, islanding mask, v, theta, converged, worst_line, v_min_bus,
 * v_max_bus or base_converged, a negative max_iter or tol, a blob that is not a Newton-Raphson blob or whose N, E, Gn are not cfg's,
 * n_pair <= 0, a line outside 0 .. E-1, a pair of twice the same line, rating_per_grid outside {0, 1}, or Bt * ceil(n_pair / C)
 * above 2^31 - 1; then GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES (from the workspace query too); then, when an
 * output is asked for, GNS_EINVAL for a NULL workspace and GNS_ESIZE for a short one.  Every refusal comes before any launch;
 * nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, a generator plus two lines (a generator with one line: "AC generator contingency
 * screening" below, with gns_acg1_adjoint), generator reactive limits, second derivatives. */
int gns_acn2_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_pair, size_t* bytes);
int gns_acn2_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const int32_t* pairs_host, const int32_t* pairs_dev, int32_t n_pair, const uint8_t* islanding,
                     const double* rating, int32_t rating_per_grid,
                     const double* v, const double* theta, const uint8_t* converged, const int32_t* worst_line,
                     const int32_t* v_min_bus, const int32_t* v_max_bus, const uint8_t* base_converged,
                     const double* grad_v, const double* grad_theta, const double* grad_p_from, const double* grad_q_from,
                     const double* grad_p_to, const double* grad_q_to, const double* grad_worst_loading,
                     const double* grad_v_min, const double* grad_v_max,
                     float* grad_buses, float* grad_lines, float* grad_generators,
                     void* workspace, size_t workspace_bytes, void* stream);

/* AC generator contingency screening: Newton-Raphson on every grid of a batch with each generator of a list out of service, alone or
 * with one line out as well (the combined N-1 set: a unit out plus a line out; the rows of "DC generator contingency screening"),
 * with the outputs of "AC contingency screening" above per (grid, row).  One host analysis per distinct generator of the list, none
 * per row or per grid.
 *
 * Semantics.  A row is (g, k): g a 0-based generator row, k a 0-based line or -1 for "no line out".  Row (grid, (g, k)) is
 *   Newton-Raphson on the grid with generator row g deleted and, when k >= 0, line k out of service: what gns_pf_solve computes on
 *   those inputs, warm-started from the base solution.  Everything not named here is gns_acn1_screen's, word for word: the
 *   convergence test, the update, max_iter and the failure rules; the branch flows, all four exactly 0 at line k; worst_loading /
 *   worst_line, v_min / v_max and their buses; a NaN wins its summary, the lowest index among equals; no atomics; fp64.
 *   Bus roles: the slack stays the slack.  The bus of g stays PV when another generator is listed on it; otherwise it becomes a PQ
 *   bus: |V| is an unknown there and the Q equation is solved with Qsp = -Qd.
 *   Set points: |V| at a PV or slack bus is vg of the first REMAINING generator listed on it, so the outage of the first-listed unit
 *   of a shared bus moves the set point to the next unit's vg; a slack with none left takes 1, as in gns_pf_solve.
 *   Injections: Psp_i = (sum of Pg_h over the remaining generators h of bus i, in row order) + (sum of their pickup shares, in row
 *   order) - Pd_i, with exactly this association.  pickup has the meaning and the arithmetic of "DC generator contingency
 *   screening": NULL, the slack picks the lost Pg_g up and nothing is added; weights w_h >= 0 (per grid or shared), W_g the sum of
 *   w_h over h != g in generator-row order: the share of h != g is Pg_g * (w_h / W_g) when W_g > 0, and when W_g == 0 the slack
 *   picks up.  No Pmax or Pmin limit is enforced.  In AC the slack also takes the change of the losses, whatever the pickup.
 *   Start: |V| at the row's PQ buses from base_v (a freed bus starts at its old set point), theta = base_theta - base_theta[slack],
 *   |V| at PV and slack buses from the row's set points.
 *   Islanding: a generator outage never islands; row (g, k) islands exactly when k is a bridge.  The kernel does not decide that
 *   numerically: the caller passes islanding[n_row].  Those rows, every row of a grid with base_converged = 0, and a row whose line's
 *   id columns do not name an entry of the Y-bus pattern get NaN in every fp64 output, -1 in worst_line, v_min_bus, v_max_bus and
 *   iterations, and converged = 0.  Other rows are unaffected.
 *   Every (grid, row) is bit-identical alone, in any batch, in any list or order that holds it (duplicates are independent rows),
 *   with any of the optional outputs NULL, and from run to run.
 *   From the definition: where Pg_g is exactly 0 and g is not the first generator listed on its bus (nor the only one), the row's
 *   system is the base case's, so row (g, -1) starts converged at the base state with 0 iterations.
 *
 * The set.  The call takes one Newton-Raphson blob per distinct generator of the list, gns_pf_prepare_topology_out_gen's with
 * out_gen = gen_list[m], in the set layout of gns_pf_solve_set: set_host / set_dev, set_words int32 words, member m at the word
 * offset member_off[m], a multiple of 16 (64 bytes), its whole blob inside the set.  Every member has cfg's N, E, Gn and the same
 * nnz(Y) (the pattern comes from the lines alone), and the members share ONE base Y-bus per grid in the workspace.
 * Inputs: gns_acn1_screen's buses, lines, generators, rating, base_v, base_theta, base_converged and cfg; the set, with member_off
 * [n_member] int32 on the host (checked before the launch) and on the device (read by the kernel); gen_list [n_member] int32,
 * ascending and distinct, on the host and on the device; row_cols [n_row,2] int32, each row as a position into gen_list and a
 * 0-based line or -1, on the host and on the device; islanding [n_row] uint8 on the device; pickup NULL, [Gn] (pickup_per_grid 0)
 * or [Bt,Gn] (1) fp64 on the device, by generator row (not by position into gen_list); its values are the caller's to check
 * (non-negative, finite).
 * Outputs (row r = grid * n_row + position in the list): gns_acn1_screen's fifteen, shaped [Bt,n_row,...]; v, theta and the four
 * flows may be NULL (not written).
 *
 * Kernels (gns_acg1.hip): gns_acn1_screen's pre-kernel writes the base Y-bus of every grid to the workspace once, from the first
 * member's pattern; then one wave per (grid, row) with gns_pf_solve's LDS image, the launch asking for the largest member's.  The
 * row takes its blob at set + member_off[position] after the member checks of gns_pf_solve_set's kernel (an offset that is
 * negative, misaligned or outside the set, or a blob of another shape, nnz(Y) or a larger image: the row is not solved and nothing
 * outside the set is indexed), builds gns_acn1_screen's Y-bus view for k >= 0 or a view with nothing out for k = -1, and runs the
 * row routine of the AC line screens on that blob's roles, unknowns, by-bus generator lists and program, with the pickup added to
 * the specified P.  Workspace (gns_acg1_workspace_bytes): gns_acn1_workspace_bytes' figure, the base Y-bus, 16 bytes per structural
 * nonzero and GRID, whatever n_row and n_member are.
 *
 * Errors, in order: GNS_EINVAL for a NULL cfg, set, member_off, input, gen_list, row_cols, islanding mask, base_v, base_theta,
 * base_converged, workspace or output other than v, theta and the four flows, a negative max_iter or tol, n_member <= 0 or above
 * Gn, n_row <= 0, set_words above 2^31 - 1, a member offset that is negative, misaligned or whose blob does not lie inside the set,
 * a member that is not a Newton-Raphson blob of cfg's N, E, Gn, members whose nnz(Y) differ, a gen_list entry outside 0 .. Gn-1 or a
 * gen_list not ascending or not distinct, a member m whose by-bus lists are not the Gn - 1 rows without gen_list[m], a generator
 * column outside 0 .. n_member-1, a line column outside -1 .. E-1, rating_per_grid or pickup_per_grid outside {0, 1}, or Bt or
 * Bt * n_row above 2^31 - 1; then GNS_ESIZE for a short workspace; then GNS_EUNSUPPORTED, for the whole call, when any member's LDS
 * image is above GNS_PF_LDS_MAX_BYTES.  gns_acg1_workspace_bytes: GNS_EINVAL for a NULL bytes, Bt <= 0, n_row <= 0 and what the
 * call refuses of the set; it does not refuse a large image.  Every refusal comes before any launch; nothing is allocated and the
 * host is not synchronised.
 * Gradients: gns_acg1_adjoint, below.  Not here: reactive limits on the remaining units, Pmax / Pmin limits on the pickup, batches
 * that mix topologies, a generator plus two lines. */
int gns_acg1_workspace_bytes(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                             int32_t n_member, int64_t Bt, int32_t n_row, size_t* bytes);
int gns_acg1_screen(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                    const int32_t* member_off_host, const int32_t* member_off_dev, int32_t n_member,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const int32_t* gen_host, const int32_t* gen_dev,
                    const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                    const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                    const double* base_v, const double* base_theta, const uint8_t* base_converged,
                    double* v, double* theta, double* p_from, double* q_from, double* p_to, double* q_to,
                    double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus, double* v_max,
                    int32_t* v_max_bus, uint8_t* converged, int32_t* iterations, double* mismatch,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Gradients of the AC generator screen.  gns_acg1_adjoint is gns_acn1_adjoint ("Gradients of the AC screen" above) per row of a
 * gns_acg1_screen call.  It takes the arguments of that call up to pickup_per_grid (the same set, lists, islanding mask, rating and
 * pickup), its outputs v, theta [Bt,n_row,N], converged, worst_line, v_min_bus, v_max_bus [Bt,n_row] and the base_converged [Bt] it
 * was given, and the incoming gradients of a loss of its nine fp64 outputs: grad_v, grad_theta [Bt,n_row,N], grad_p_from,
 * grad_q_from, grad_p_to, grad_q_to [Bt,n_row,E], grad_worst_loading, grad_v_min, grad_v_max [Bt,n_row] (each may be NULL: zero).
 * It writes dl/d(input) into grad_buses [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32 and dl/d(pickup weights) into
 * grad_pickup [Bt,Gn] fp64, a row per grid whether the weights are per grid or shared; each may be NULL (not computed; with all four
 * NULL nothing is launched).  Every element of each non-NULL output is written (overwritten, not accumulated).  The state is the
 * forward's: Newton-Raphson is not run again, and the warm start (a freed bus's old set point included) is not differentiated.
 *
 * Method, per solved row (grid, (g, k)): the implicit function theorem on the grid with generator row g deleted and line k out, at
 * the forward's state, on the row's own blob (the member without g) and gns_acn1_screen's Y-bus view: one factorisation of the
 * row's Jacobian, one transposed solve, gns_acn1_adjoint's bus and line algebra unchanged (row (g, k) adds exactly 0 to line k's
 * own columns).  What the generator brings:
 *   unknowns and roles are the member's.  A freed sole-unit bus is PQ: its lambda_Q feeds Qd and Bs, and it gives no vg gradient.
 *   vg goes to the first REMAINING unit listed on a PV or slack bus of the member, at that unit's original generator row; the lost
 *   unit's vg gets exactly 0; a slack with no unit left has |V| = 1, a constant.
 *   Pg.  mu_h = lambda_P of the bus of h, 0 at the slack, in the sign gns_acn1_adjoint gives Pg.  A remaining unit h != g gets
 *   dl/dPg_h = mu_h.  With W = W_g > 0 as the forward sums it, the lost unit gets dl/dPg_g = M = sum_{h != g} mu_h (w_h / W), summed
 *   in generator-row order; when the slack picks up (pickup NULL, or W exactly 0) it gets exactly 0.
 *   Weights.  For h != g, dl/dw_h = Pg_g (mu_h - M) / W, and dl/dw_g = 0.  The W == 0 branch is not differentiated: it gives the
 *   weights 0.  A caller whose weights are a column of the generators ('pmax': column 1) adds grad_pickup into that column.
 *
 * Contract, failure rules and arithmetic: gns_acn1_adjoint's, with "row" for "outage": gns_pf_adjoint's columns (Pd, Qd, Gs, Bs; r,
 *   x, b, tau, shift; Pg, vg), every other column 0; a line whose id columns are not buses of the grid gets a NaN row; rating is a
 *   constant.  A row whose incoming gradients are all exactly zero or NULL is skipped, never multiplied by zero.  A row with
 *   converged == 0 (an islanding row, a stopped or unconverged iteration, NaN / -1) and a non-zero incoming gradient, a zero or
 *   non-finite pivot, or a non-finite lambda: all gradient rows of that grid, grad_pickup's included, are NaN.  A grid with
 *   base_converged == 0 gets NaN rows when an incoming gradient of it is non-zero, zero rows otherwise.  Other grids are unaffected.
 *   fp64 throughout, the three input gradients rounded once to fp32.  No atomics, every sum in a fixed order: a grid's gradient is
 *   bit-identical alone, in any batch and from run to run for the same list.  The order and the chunking of the list set the order
 *   of the sums over rows, so another order of the same rows may change the last bits.
 *
 * Kernels (gns_acg1.hip), three launches: the base Y-bus of every grid from the first member's pattern; one wave per (grid, chunk of
 * C consecutive rows of the list) with gns_pf_solve's LDS image, the launch asking for the largest member's; one wave per grid that
 * sums the chunks' partials in order, applies the contract and writes vg, Pg and the weights by original generator row.  Each row
 * takes its blob after gns_acg1_screen's member checks, builds the same view and sums W_g the same way, then runs the routine of the
 * line adjoints (acn_adjoint_row, gns_acn_adjoint_device.h) with the generator part of the partial laid out by generator row.
 * C = max(1, ceil(n_row / 64)): from the list's length alone, never from Bt; a grid has at most 64 partials however long the list.
 * Workspace (gns_acg1_adjoint_workspace_bytes): the base Y-bus (gns_acg1_workspace_bytes' figure) plus Bt * ceil(n_row / C) partials
 * of 4 N + 5 E + 4 Gn + 1 doubles, each part rounded up to 256 bytes.
 *
 * Errors, in order: GNS_EINVAL for what gns_acg1_screen refuses of cfg, the set, the inputs, the lists, the islanding mask,
 * rating_per_grid, pickup_per_grid and Bt, for a NULL v, theta, converged, worst_line, v_min_bus, v_max_bus or base_converged, for
 * a member whose by-bus lists name something that is not a generator row, or for Bt * ceil(n_row / C) above 2^31 - 1; then
 * GNS_EUNSUPPORTED, for the whole call, when any member's LDS image is above GNS_PF_LDS_MAX_BYTES (from the workspace query too,
 * unlike gns_acg1_workspace_bytes); then, when an output is asked for, GNS_EINVAL for a NULL workspace and GNS_ESIZE for a short one.
 * Every refusal comes before any launch; nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, reactive limits on the remaining units, Pmax / Pmin limits on the pickup, a generator
 * plus two lines, second derivatives. */
int gns_acg1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                                     int32_t n_member, int64_t Bt, int32_t n_row, size_t* bytes);
int gns_acg1_adjoint(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
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
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- The solved case -------------------------------------------------------------------------------------------------------------
 * What PYPOWER's runpf returns next to the voltages (its pfsoln step), for every grid of a batch at a GIVEN state (v, theta): a
 * solver's result, a warm start or a model's prediction.  Nothing is iterated or solved.  One Newton-Raphson blob per call
 * (gns_pf_prepare_topology); buses, lines, generators and cfg (max_iter and tol are checked as gns_pf_solve checks them and not
 * used) as in gns_pf_solve; v, theta [Bt,N] fp64 are used as given (theta is not shifted); rating NULL (1), [E]
 * (rating_per_grid = 0) or [Bt,E] (1) fp64 as in gns_acn1_screen.
 *
 * Semantics.  V_i = v_i e^{j theta_i}; Y the makeYbus matrix gns_pf_solve builds (shunts included).
 *   p_from, q_from, p_to, q_to [Bt,E]: gns_acn1_screen's branch flows on the line's own four stamps, S_f = V_f conj(Y_ff V_f +
 *     Y_ft V_t), S_t = V_t conj(Y_tf V_f + Y_tt V_t), in its expression order; NaN at a line whose id columns are not buses of the
 *     grid; a line from a bus to itself and parallel lines as there.
 *   p_inj, q_inj [Bt,N]: Re and Im of V_i conj(sum_k Y_ik V_k), the row product and the power in gns_pf_solve's expression order.
 *   mismatch [Bt]: gns_pf_solve's ||F||_inf at this state: the largest of |p_inj - Psp| at PV and PQ buses and |q_inj - Qsp| at PQ
 *     buses (Psp = sum of the bus's Pg in listing order - Pd, Qsp = -Qd), NaN when a term is not finite.  At the v, theta that
 *     gns_pf_solve returns it is that call's mismatch bit for bit.
 *   gen_q [Bt,Gn]: a bus with n >= 1 listed units produces q_inj + Qd, each unit (q_inj + Qd) / n (pfsoln without limit ranges).
 *   gen_p [Bt,Gn]: every unit's Pg (column 6) as given, but the first unit listed on the slack, which carries p_inj[slack] +
 *     Pd[slack] - (the sum, in listing order, of Pg of the other units on the slack).
 *   slack_p [Bt] = p_inj[slack] + Pd[slack] - (the sum, in listing order, of Pg on the slack): what the slack produces beyond its
 *     listed dispatch (gns_dc_solve's slack_p), defined for a slack without a unit too.  Column 5 (qg) is not read, nor is vg.
 *   worst_loading [Bt] = max_l max(|S_f|, |S_t|) / rating_l with worst_line [Bt]; v_min, v_max [Bt] with v_min_bus, v_max_bus:
 *     gns_acn1_screen's definitions, total order and tie rules (a NaN wins at the lowest index that holds one, the lowest index
 *     among equals).
 *   Each of the [Bt,E], [Bt,N] and [Bt,Gn] outputs may be NULL: not written.  No atomics, every sum in a fixed order: a grid's
 *   outputs are bit-identical alone, in any batch, with any optional output NULL and from run to run; a NaN in a grid's state makes
 *   that grid's outputs NaN and leaves the others alone.
 *
 * Kernel (gns_pfs.hip): one wave per grid; the state and the injections in LDS, 40 N bytes per grid (below gns_pf_solve's image on
 * every topology); the grid's Y-bus values go to the workspace, gns_pf_workspace_bytes' figure (gns_pfs_workspace_bytes).
 *
 * Errors, in order: GNS_EINVAL for a NULL cfg (or one gns_pf_solve refuses), blob, input, v, theta, [Bt] output or workspace, for
 * rating_per_grid outside {0, 1}, for Bt <= 0 or above 2^31 - 1, for a blob that is not a Newton-Raphson blob or whose N, E, Gn are
 * not cfg's; then GNS_ESIZE for a short workspace; then GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES.  Every
 * refusal comes before any launch; nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, reactive limits, second derivatives. */
int gns_pfs_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes);
int gns_pfs_evaluate(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                     const float* buses, const float* lines, const float* generators, int64_t Bt,
                     const double* v, const double* theta, const double* rating, int32_t rating_per_grid,
                     double* p_from, double* q_from, double* p_to, double* q_to, double* p_inj, double* q_inj,
                     double* gen_p, double* gen_q, double* mismatch, double* slack_p,
                     double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus, double* v_max, int32_t* v_max_bus,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- Gradients of the solved case ------------------------------------------------------------------------------------------------
 * gns_pfs_adjoint: the gradients of a loss l of gns_pfs_evaluate's differentiable outputs (the four flows, p_inj, q_inj, gen_p,
 * gen_q, slack_p, worst_loading, v_min, v_max) with respect to the state and the inputs, at the state the forward was given.  The
 * incoming gradients grad_<output> have the outputs' shapes, fp64; each may be NULL (zero).  worst_line, v_min_bus, v_max_bus are
 * the forward's.  mismatch and the indices are not differentiable, rating is a constant.
 * Outputs, each may be NULL (with all five NULL nothing is launched), every element written: grad_v, grad_theta [Bt,N] fp64 at
 * every bus, the slack included; grad_buses [Bt,N,6], grad_lines [Bt,E,7], grad_generators [Bt,Gn,7] fp32.
 *
 * Method: no linear solve.  The bus cotangent Lambda_i = grad_p_inj_i + j grad_q_inj_i, whose real part at the slack also takes
 * grad_slack_p + grad_gen_p[first slack unit] and whose imaginary part at a bus with n_i >= 1 units also takes (sum_u grad_gen_q_u)
 * / n_i, joins the flows' cotangents at the line ends: W_f,l = grad_p_from_l + j grad_q_from_l + Lambda_{f_l}, W_t,l likewise
 * (S_i is the sum of the flows that leave bus i plus |V_i|^2 conj(Gs_i + j Bs_i)).  grad_worst_loading adds (p + jq) / |S| /
 * rating_w to the end of worst_line that attains the maximum, as gns_acn1_adjoint does (the from end on equality, nothing at
 * |S| = 0).
 *   grad_theta, grad_v: gns_acn1_adjoint's gather of the flow cotangents with these W (a bus walks its diagonal's stamps, no
 *     scatter), plus the shunt term 2 |V_i| (Gs Re Lambda_i - Bs Im Lambda_i), plus grad_v_min / grad_v_max at their buses.
 *   lines, columns 2-6 (r, x, b, tau, shift): gns_pf_adjoint's stamp algebra with +W where the mismatch term has -Lambda; parallel
 *     lines each get their own row; a line whose id columns are not buses of the grid gets a NaN row.  Columns 0, 1: 0.
 *   buses: Pd = grad_slack_p + grad_gen_p[first slack unit] at the slack, 0 elsewhere; Qd = (sum_u grad_gen_q_u) / n_i; Gs = |V|^2
 *     Re Lambda; Bs = -|V|^2 Im Lambda; columns 0, 1: 0.
 *   generators, column 6 (Pg): a unit off the slack gets grad_gen_p_u; the first slack unit -grad_slack_p; every other slack unit
 *     grad_gen_p_u - grad_slack_p - grad_gen_p[first slack unit] (its own gen_p is its Pg, and its Pg leaves both slack_p and the
 *     first unit's gen_p).  Every other column 0 (the forward reads neither vg nor qg).
 *   A grid whose incoming gradients are all exactly zero or NULL gets exactly zero rows whatever its state: it is skipped, never
 *   multiplied by zero.  fp64 throughout, the three input gradients rounded once to fp32.  No atomics, every sum in a fixed order:
 *   a grid's gradient is bit-identical alone, in any batch and from run to run.
 *
 * Kernel (gns_pfs.hip): one wave per grid, the forward's LDS image (40 N bytes).  It reads no Y-bus, so it needs no workspace:
 * gns_pfs_adjoint_workspace_bytes answers 0 and workspace may be NULL.
 * Errors, in order: GNS_EINVAL for what gns_pfs_evaluate refuses of cfg, the blob, the inputs, v, theta, rating_per_grid and Bt and
 * for a NULL worst_line, v_min_bus or v_max_bus; then GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES.  Before any
 * launch, with no allocation and no host synchronisation.
 * Not here: batches that mix topologies, second derivatives. */
int gns_pfs_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes);
int gns_pfs_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const double* v, const double* theta, const double* rating, int32_t rating_per_grid,
                    const int32_t* worst_line, const int32_t* v_min_bus, const int32_t* v_max_bus,
                    const double* grad_p_from, const double* grad_q_from, const double* grad_p_to, const double* grad_q_to,
                    const double* grad_p_inj, const double* grad_q_inj, const double* grad_gen_p, const double* grad_gen_q,
                    const double* grad_slack_p, const double* grad_worst_loading, const double* grad_v_min, const double* grad_v_max,
                    double* grad_v, double* grad_theta, float* grad_buses, float* grad_lines, float* grad_generators,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- DC optimal power flow -------------------------------------------------------------------------------------------------------
 * PYPOWER's DC OPF (dcopf / dcopf_solver) without piecewise-linear costs, for every grid of a batch: the dispatch of every listed
 * unit that is cheapest within the units' bounds and the lines' ratings, its multipliers and the locational marginal prices.  One
 * fast-decoupled blob per call (gns_fd_prepare_topology); buses, lines, generators as in gns_dc_solve.  cfg: n_bus, n_line, n_gen,
 * max_iter (iterations allowed) and tol (the termination tolerance).
 *
 * Problem, per grid, fp64:  min sum_g c2_g p_g^2 + c1_g p_g  subject to  Bbus[r, r] theta_r = P_r(p),  theta_slack = 0,
 *   |b_l (theta_f - theta_t) + Pfinj_l| <= rating_l,  Pmin_g <= p_g <= Pmax_g,
 * with b, Pfinj, Pbusinj and P = sum p - Pd - Gs - Pbusinj exactly gns_dc_solve's; the slack's balance is the one equality left once
 * theta is eliminated: sum_g p_g = sum_i (Pd_i + Gs_i).  The listed Pg (column 6) is not read; Pmax and Pmin are columns 1 and 2.
 *   cost    [Gn,2] (cost_per_grid = 0) or [Bt,Gn,2] (1) fp64: (c2, c1) per unit, in per-unit p; c2 >= 0 (all zero: a linear program).
 *   rating  NULL (no line has a limit), [E] (rating_per_grid = 0) or [Bt,E] (1) fp64: positive; +inf: that line has no limit.
 *
 * Method.  Shift factors: one solve z_g = A^-1 e_bus(g) per unit on the factor of A = Bbus[r, r] gives S_g[l] = b_l (z_g[f_l] -
 * z_g[t_l]) (a zero column for a unit on the slack); f0 is the flow without generation; the inequalities are f0 + S p <= rating,
 * -(f0 + S p) <= rating, p <= Pmax, -p <= -Pmin (h <= 0, rows of A_in).  A primal-dual interior point with PIPS's scheme on p, the
 * slacks z > 0 and the multipliers mu > 0 and lambda:
 *   start     p the midpoint of the bounds, z = max(1, -h), gamma = 1, mu = gamma / z, lambda = 0
 *   test      before every update, all three below tol:  max(|g|, max h) / (1 + max(|p|_inf, |z|_inf)),
 *             |L_x|_inf / (1 + max(|lambda|, |mu|_inf)),  z.mu / (1 + |p|_inf);   g = sum p - demand,
 *             L_x = 2 c2 p + c1 + lambda + A_in^T mu
 *   matrix    M = diag(2 c2) + A_in^T diag(mu / z) A_in, Gn x Gn, plus delta trace(M) / Gn on its diagonal, delta = 1e-14; dense
 *             Cholesky in LDS; a pivot that is not positive or not finite ends the grid with its last iterate, converged 0
 *   step      M w = -(L_x + A_in^T ((gamma + mu h) / z)), M u = 1, dlambda = (sum w + g) / sum u, dp = w - dlambda u,
 *             dz = -h - z - A_in dp, dmu = -mu + (gamma - mu dz) / z; separate primal and dual lengths min(xi min(z / -dz), 1) and
 *             min(xi min(mu / -dmu), 1) with xi = 0.99995; then gamma = sigma z.mu / n_ineq, sigma = 0.1.  A step that is not
 *             finite is not taken: the grid ends with its last iterate, converged 0.
 * Outputs, every element written:
 *   pg [Bt,Gn]; theta [Bt,N] and line_flow [Bt,E]: gns_dc_solve's definitions at the injections of pg, formed and solved in fp64
 *   (pg is never rounded to fp32); mu_line [Bt,E]: the multiplier of the upper limit minus that of the lower (0 at a line without a
 *   limit); mu_pmax, mu_pmin [Bt,Gn] >= 0; lmp [Bt,N] = -lambda - PTDF^T mu_line, the derivative of the optimal cost with respect
 *   to Pd at each bus, from one more solve on the symmetric factor with right-hand side sum_l b_l mu_line_l (e_f - e_t) (no [E,N]
 *   matrix is formed); objective [Bt]: the cost at pg; converged [Bt] u8; iterations [Bt] i32: the updates made.
 *   A grid that reaches max_iter keeps its last finite iterate with converged 0.  A grid is not solved (iterations -1, NaN in every
 *   fp64 output, converged 0) when its base factor or a unit's solve fails, its data (Pd, Gs, the lines, Pmin, Pmax, cost, rating)
 *   are not finite (a rating of +inf aside), a rating is not positive, a c2 is negative, some unit has Pmin >= Pmax, or its demand
 *   lies outside [sum Pmin, sum Pmax]; the other grids are unaffected.  No atomics, every sum in a fixed order: a grid's result is
 *   bit-identical alone, in any batch, in any order, with cost and rating shared or per grid, and from run to run.
 *
 * Kernels (gns_dcopf.hip), three launches, a wave per workgroup:
 *   factor  per (grid, chunk of W units) on gns_dcn1_screen's LDS image at width W plus 32 Gn bytes (generator rows of zeros: the
 *           base case is the one without generation): S as [E][Gn] per grid, f0, the units' finite flags and the grid's status
 *   ipm     per grid; LDS 8 (Gn (Gn + 1) / 2 + 14 Gn + 10 E) bytes: the packed triangle of M and the iterate; S streams from
 *           the workspace
 *   finish  per grid on the factor kernel's image at width 1: theta, line_flow, lmp
 * gns_dcopf_lds_bytes: the largest of these images, and W (NULL: not wanted), the largest power of two up to 64 whose factor image
 * fits.  gns_dcopf_workspace_bytes: 8 Bt (E Gn + E + Gn + 3) bytes rounded up to 256.
 *
 * Errors, in order: GNS_EINVAL for a NULL device blob, input, cost, output or workspace, for cost_per_grid or rating_per_grid outside
 * {0, 1}, for Bt <= 0 or above 2^31 - 1, for a NULL cfg or one gns_pf_solve refuses, a NULL host blob, a blob that is not a
 * fast-decoupled blob or whose N, E, Gn are not cfg's, for Gn = 0, and for more workgroups than a launch takes; then GNS_ESIZE for
 * a short workspace; then GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES.  Every refusal comes before any launch;
 * nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, gradients of the optimum (the adjoint below), AC OPF, units with Pmin = Pmax, piecewise-linear costs,
 * contingency constraints (gns_dcscopf_solve below). */
int gns_dcopf_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes);
int gns_dcopf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes);
int gns_dcopf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                    const float* buses, const float* lines, const float* generators, int64_t Bt,
                    const double* cost, int32_t cost_per_grid, const double* rating, int32_t rating_per_grid,
                    double* pg, double* theta, double* line_flow, double* lmp, double* mu_line, double* mu_pmax, double* mu_pmin,
                    double* objective, uint8_t* converged, int32_t* iterations,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- DC optimal power flow: adjoint ----------------------------------------------------------------------------------------------
 * The gradient of a loss on the eight fp64 outputs of gns_dcopf_solve with respect to the data of the problem, for every grid of the
 * batch, from the forward's inputs and returned tensors alone (the forward saves nothing else).  The optimum is differentiated by
 * the implicit-function theorem on its KKT conditions with the active rows held as equalities and the multipliers of the others
 * as constants; there is no second optimisation.
 *   inputs   buses, lines, generators, cost, rating and their flags: the forward call's.  pg .. iterations: what it returned.
 *   incoming grad_pg [Bt,Gn], grad_theta [Bt,N], grad_line_flow [Bt,E], grad_lmp [Bt,N], grad_mu_line [Bt,E], grad_mu_pmax,
 *            grad_mu_pmin [Bt,Gn], grad_objective [Bt], fp64; NULL: zero.
 *   outputs  (NULL: not wanted; every element written) grad_buses [Bt,N,6] fp32: Pd (2) and Gs (4), the other columns 0;
 *            grad_generators [Bt,Gn,7] fp32: Pmax (1) and Pmin (2), the other columns 0, the listed Pg included; grad_cost
 *            [Bt,Gn,2] fp64 (c2, c1), per grid whatever cost_per_grid says (a shared cost's gradient is the sum over the grids);
 *            grad_rating [Bt,E] fp64, likewise, 0 at a rating of +inf.  The lines' x, tau and shift are not differentiated.
 *
 * Method, per grid.  S as the forward forms it (its factor kernel, unchanged, into this call's workspace).  Active set from the
 * outputs: with the slacks z = rating -+ line_flow, Pmax - pg, pg - Pmin, a line's upper row is active when mu_line > max(z, 0), its
 * lower one when -mu_line > max(z, 0), a unit's rows likewise with mu_pmax and mu_pmin; F is the set of units without an active
 * row, k the number of active lines.  The cotangents are pulled back to (p, lambda, mu_line, nu): theta and line_flow through
 * t = A^-1 (g_theta_r + B_f,r^T g_flow) on the base factor (A = Bbus[r, r] is symmetric), C_g^T t to p and -t to Pd and Gs; lmp
 * through y = A^-1 g_lmp_r, -sum g_lmp to lambda and -b_l (y_f - y_t) to mu_line_l; objective gives g (2 c2 p + c1) to p, g p^2 to
 * c2 and g p to c1; the cotangent of a multiplier whose row is not active is dropped (its derivative is 0).  Then
 *     [ diag(2 c2_F)  1    S_aF^T ] [a_p     ]   [g_p     ]
 *     [ 1^T           0    0      ] [a_lambda] = [g_lambda]
 *     [ S_aF          0    0      ] [a_mu    ]   [g_mu    ]
 * of order n = |F| + 1 + k <= 2 Gn, the units on a bound substituted (a_p there is the cotangent of the unit's own multiplier, a_nu
 * follows from its stationarity row), is solved by dense LU with partial pivoting in LDS: exact for c2 = 0, no regularisation, no
 * S Q^-1 S^T, and not the forward's normal matrix, which is conditioned 1e14 and worse on a linear program.  The gradients are
 * -a^T dF/d(data): c1 -a_p, c2 -2 p a_p, every bus's Pd and Gs +a_lambda and, through f0, +A^-1 B_f,r^T a_mu (a third solve), an
 * active line's rating +-a_mu by the sign of its row, Pmax or Pmin +a_nu.  Three network solves and one dense solve per grid.
 * Rows.  A grid whose incoming gradients are all exactly zero (or NULL) gets zero rows.  Otherwise a grid with iterations -1,
 * converged 0 or an output that is not finite gets NaN in every element of its rows, and so does a grid whose n exceeds the
 * order the image holds or whose LU meets a pivot that is zero or not finite; the other grids are unaffected.  Near a degenerate
 * optimum (a row whose slack and multiplier are both small) the gradient is that of the active set as classified: finite, and not
 * reliable.  No atomics, every sum in a fixed order: a grid's rows are bit-identical alone, in any batch, in any order and from
 * run to run.
 *
 * Kernels (gns_dcopf_adjoint.hip), a wave per workgroup: gns_dcopf.hip's factor kernel, then the adjoint kernel, one grid each.
 * gns_dcopf_adjoint_lds_bytes: the adjoint kernel's image at the largest order n_max <= 2 Gn that fits GNS_PF_LDS_MAX_BYTES, and
 * n_max (NULL: not wanted): 8 (nnz_lu_p + dim_p + N + 3 E + 2 dim_p) + 32 Gn bytes for the network solves, then
 * 8 (3 Gn + E + ceil((2 Gn + E) / 2) + n_max ((n_max + 1) | 1)) bytes.  gns_dcopf_adjoint_workspace_bytes: gns_dcopf_workspace_bytes'
 * (GNS_EUNSUPPORTED from the query too).
 *
 * Errors, in order: gns_dcopf_solve's GNS_EINVAL cases (the forward's outputs count as inputs here; the incoming gradients and
 * the gradient outputs may be NULL); then GNS_ESIZE for a short workspace; then GNS_EUNSUPPORTED when the network-solve part of
 * the image (n = 0) alone is above GNS_PF_LDS_MAX_BYTES.  With no gradient output asked for the call returns GNS_OK without a
 * launch, after every other check.  Every refusal comes before any launch; nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, gradients with respect to the lines, second derivatives. */
int gns_dcopf_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* order);
int gns_dcopf_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes);
int gns_dcopf_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                      const float* buses, const float* lines, const float* generators, int64_t Bt,
                      const double* cost, int32_t cost_per_grid, const double* rating, int32_t rating_per_grid,
                      const double* pg, const double* theta, const double* line_flow, const double* lmp,
                      const double* mu_line, const double* mu_pmax, const double* mu_pmin, const double* objective,
                      const uint8_t* converged, const int32_t* iterations,
                      const double* grad_pg, const double* grad_theta, const double* grad_line_flow, const double* grad_lmp,
                      const double* grad_mu_line, const double* grad_mu_pmax, const double* grad_mu_pmin, const double* grad_objective,
                      float* grad_buses, float* grad_generators, double* grad_cost, double* grad_rating,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- Security-constrained DC optimal power flow ----------------------------------------------------------------------------------
 * gns_dcopf_solve's problem with contingency rows: the cheapest dispatch within the units' bounds, the lines' ratings and, for every
 * listed row, the limit on a monitored line's flow after the outage of another line.  Blob, buses, lines, generators, cfg, cost,
 * rating and their flags are gns_dcopf_solve's.  Additional inputs:
 *   rows      int32 on the device, [R,2] (rows_per_grid = 0) or [Bt,R,2] (1), R = n_row >= 1: (l, k), line l monitored after the
 *             outage of line k, 0-based; (-1, -1) is an empty slot.  Duplicates are independent rows.
 *   rating_c  fp64 [E] (rating_c_per_grid = 0) or [Bt,E] (1), positive: the post-outage (emergency) rating of the monitored line;
 *             NULL: rating with its flag is used (both NULL: no row constrains anything).  A row whose monitored line has a rating
 *             of +inf constrains nothing and is treated as an empty slot.
 *   bridge    u8 [E] on the device: the host's bridge flags of the topology (what the screens take per outage as `islanding`).
 *
 * Problem.  gns_dcopf_solve's, plus for every row r = (l, k) that is not empty:  |F_l + L_r F_k| <= rating_c_l,  with F = f0 + S p
 * the base flows and L_r = b_l (z_k[f_l] - z_k[t_l]) / (1 - b_k d_k), z_k and d_k as gns_dcn1_screen defines them ("Semantics"): the
 * post-outage flow of line l.  A line k from a bus to itself gives L_r = 0.  A row is a combination of two rows of S, so the normal
 * matrix stays Gn x Gn however many rows are listed.
 *
 * Method.  gns_dcopf_solve's, constant for constant (start, xi, sigma, delta, the three termination figures, separate step lengths,
 * the not-finite-step rule); both calls run one body.  The rows join A_in after the line rows and before the box rows:
 * z = max(1, -h), mu = gamma / z at the start; n_ineq counts two per row that is not empty.  A row's value is fl[l] + L_r fl[k] from
 * the current flows and A_r dp is (S dp)[l] + L_r (S dp)[k]; A_in^T v adds v_r at l and L_r v_r at k, the rows in list order, before
 * the one S^T product; M gains sum_r d_r a_r a_r^T with a_r = S[l] + L_r S[k] after the lines' terms, the rows in list order.
 *
 * Outputs, every element written: gns_dcopf_solve's ten, and
 *   mu_row [Bt,R]    the multiplier of the row's upper side minus that of its lower; 0 in an empty slot
 *   row_flow [Bt,R]  line_flow_l + L_r line_flow_k at the returned dispatch; NaN in an empty slot
 * lmp stays the derivative of the optimal cost with respect to Pd: the finish's right-hand side takes mu_line_l + sum_r mu_r at
 * line l and L_r mu_r at line k.  With every slot empty the ten outputs are gns_dcopf_solve's bit for bit.
 *   A grid is not solved (iterations -1, NaN in every fp64 output, mu_row and row_flow included in every slot, converged 0) under
 *   gns_dcopf_solve's rules (rating_c read like rating, at the monitored lines of the rows), or when a row that is not (-1, -1) has
 *   l or k outside 0 .. E - 1, has l = k, has bridge[k] != 0 (unless its rating_c is +inf: it is an empty slot), or has a z_k or a
 *   denominator that is zero or not finite; the other grids are unaffected.  No atomics, every sum in a fixed order: a grid's
 *   result is bit-identical alone, in any batch, in any order, with rows, cost and the ratings shared or per grid, and from run to
 *   run.
 *
 * Kernels (gns_dcscopf.hip and gns_dcopf.hip), five launches, a wave per workgroup:
 *   factor    gns_dcopf_solve's, unchanged
 *   rows      per (grid, chunk of W slots) on the factor kernel's image: the base factor, a lane per slot for its own solve z_k (a
 *             solve per slot, duplicates of k included), L_r and the slot's status into the workspace
 *   ipm       per grid; gns_dcopf_solve's image plus 8 (10 R + ceil(E / 2)) bytes: per slot L_r, the rating, the two slacks and
 *             multipliers, the weight, the row's entries of the two vectors A_in^T takes and (l, k); per line an int32, whether a
 *             row names it
 *   finish    gns_dcopf_solve's, unchanged, on the per-line multipliers above
 *   row_flow  a thread per slot
 * gns_dcscopf_lds_bytes: the larger of the factor image at W and the ipm image for n_row, and W (NULL: not wanted), as
 * gns_dcopf_lds_bytes.  gns_dcscopf_workspace_bytes: gns_dcopf_workspace_bytes' plus 8 Bt (2 R + E) bytes rounded up to 256.
 *
 * Errors, in gns_dcopf_solve's order: GNS_EINVAL for its cases and for NULL rows, bridge, mu_row or row_flow, n_row <= 0, a flag
 * outside {0, 1} and more workgroups than a launch takes (the units' chunks, the slots' chunks or the row_flow blocks); then
 * GNS_ESIZE for a short workspace; then GNS_EUNSUPPORTED for an LDS image above GNS_PF_LDS_MAX_BYTES.  Every refusal comes before
 * any launch; nothing is allocated and the host is not synchronised.
 * Not here: batches that mix topologies, gradients of the secure dispatch, generator outages as constraints, corrective
 * re-dispatch after an outage, double outages. */
int gns_dcscopf_lds_bytes(const void* topo_host, int32_t n_row, int64_t* bytes, int32_t* lanes);
int gns_dcscopf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_row, size_t* bytes);
int gns_dcscopf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                      const float* buses, const float* lines, const float* generators, int64_t Bt,
                      const double* cost, int32_t cost_per_grid, const double* rating, int32_t rating_per_grid,
                      const int32_t* rows, int32_t rows_per_grid, int32_t n_row,
                      const double* rating_c, int32_t rating_c_per_grid, const uint8_t* bridge,
                      double* pg, double* theta, double* line_flow, double* lmp, double* mu_line, double* mu_pmax, double* mu_pmin,
                      double* objective, uint8_t* converged, int32_t* iterations, double* mu_row, double* row_flow,
                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNS_POWERFLOW_H */
