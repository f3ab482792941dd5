/*
 * pddp_hip.h - C ABI of libpddp_hip.so, the MI355X (gfx950) implementation of
 * the PDDP / iLQR data-parallel hot path.
 *
 * The reference (anassinator/pddp) is pure Python on torch 0.4.1 and has NO
 * native boundary; this ABI is what a native extension
 * of the reference would bind for its hot path.  Each entry point names the
 * reference function it replaces.  The Python plugin API on top
 * (pddp_amd.controllers / costs / models) mirrors the reference's classes and
 * calls these through ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless marked "host";
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered,
 *     nothing allocates, nothing synchronises the host, nothing throws;
 *   - return value: 0 on success, <0 PDDP_E_* for argument errors, >0 a
 *     hipError_t from the launch;
 *   - numerical failures the reference signals with RuntimeError
 *     (ilqr.py:608,639,653 and potrf at :595) are reported per trajectory in
 *     `status[b]` (PDDP_BWD_* of pddp_problem.h);
 *   - B independent trajectories (the batch axis the reference does not have:
 *     every trajectory is one reference controller call), N horizon,
 *     n encoded state size, m action size;
 *   - _f32 / _f64 suffix = arithmetic type of the whole path.
 *
 * Record layout (the HBM format the backward sweep streams; one record per
 * trajectory and time step, trajectory-major, N+1 records per trajectory, the
 * last one holding the terminal L_z, L_zz of ilqr.py:471-473):
 *
 *   rec[b][t][ F_z n*n | L_zz n*n | F_u n*m | L_uz m*n | L_z n | L_uu m*m |
 *              L_u m | U m | pad ]          stride = roundup4(total) scalars
 *
 * (cartpole n=4,m=1: 47 -> 48 floats = 192 B.)  `U` is the un-clamped nominal
 * action (ilqr.py:602,647 read it for the BoxQP bounds).  Gains come back as
 *
 *   gains[b][t][ k m | K m*n ]              (ilqr.py:581-582 k, K)
 */
#ifndef PDDP_HIP_H
#define PDDP_HIP_H

#include <stdint.h>

#include "pddp_problem.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  PDDP_E_BADARG = -1,      /* null pointer / non-positive size */
  PDDP_E_UNSUPPORTED = -2, /* (n, m, model, encoding) not built */
  PDDP_E_NODEVICE = -3
};

typedef struct pddp_record_layout {
  int n, m;
  int o_Fz, o_Lzz, o_Fu, o_Luz, o_Lz, o_Luu, o_Lu, o_U;
  int stride;      /* scalars per record */
  int gain_stride; /* m + m*n */
} pddp_record_layout;

/* Library / device probes (host). */
int pddp_hip_abi_version(void);
int pddp_hip_device_count(void);
const char* pddp_hip_arch(void); /* "gfx950" */
int pddp_record_layout_of(int n, int m, pddp_record_layout* out /* host */);

/* ---- ilqr.py:529-674 backward(): the Riccati sweep --------------------- */
/* rec    [B][N+1][stride]   records (see above)
 * u_min, u_max [m] or both NULL -> branch A/C (no BoxQP), else B/D
 * reg    [B] per-trajectory mu (ilqr.py:135 passes self._mu), host-side type
 *        double like the reference's python float
 * branch PDDP_BRANCH_EIG (controller default, V_zz_reg=False) or _CHOLESKY
 * active [B] nullable; trajectories with active[b]==0 are skipped: their
 *        status is left untouched, their gains rows are unspecified
 * gains  [B][N][m + m*n] out (unspecified from the failing step on when
 *        status[b] != 0, like the reference which raises)
 * status [B] out (PDDP_BWD_*) */
int pddp_riccati_backward_f32(int B, int N, int n, int m, const float* rec,
                              const float* u_min, const float* u_max,
                              const double* reg, int branch,
                              const uint8_t* active, float* gains,
                              int32_t* status, void* stream);
int pddp_riccati_backward_f64(int B, int N, int n, int m, const double* rec,
                              const double* u_min, const double* u_max,
                              const double* reg, int branch,
                              const uint8_t* active, double* gains,
                              int32_t* status, void* stream);

/* The same sweep through a chosen kernel variant (A/B measurements):
 * 0 auto (what the entry points above use), 1 generic kernel (one wavefront
 * per trajectory, any n <= 32, m <= 4; larger n: four wavefronts), and for
 * n = 4, m = 1:
 *   6 / 7   sixteen lanes per trajectory, BoxQP in closed form with the
 *           reference's loop as fall-back (IEEE division / v_rcp + v_sqrt,
 *           f32 only for the odd numbers throughout);
 *   16 / 17 four lanes per trajectory, sixteen trajectories per wavefront
 *           (all four branches); 18 = 16 with every BoxQP through the
 *           reference's loop (bounded branches);
 * 14 / 15: the matrix-core kernels for n <= 30, m = 1 (IEEE / approximate
 * division; auto for those shapes other than n = 4); f64: n <= 14 on the f64
 * matrix cores, variant 14 only (15 and n > 14: PDDP_E_UNSUPPORTED; auto then
 * takes the generic kernel).
 * 26 / 27 (IEEE / approximate division): 15 <= n <= 30, m = 1, f32, eig-clamp
 * branches with one trajectory's step split over two wavefronts; auto for
 * those shapes and branches: 27.
 * Auto for n = 4, m = 1: f32 from 12288 trajectories on -> 17, otherwise 7
 * (f32) / 6 (f64).  Any other number: PDDP_E_BADARG (rounds 1-4 carried 2 / 3,
 * 8 - 13, 20 - 25: other formulations of the n = 4 sweep ON RECORDS, retired
 * once the cartpole's rounds took their sweep from the nominal,
 * pddp_sweep_nominal_* / pddp_round_nominal_f32). */
int pddp_riccati_backward_variant_f32(int B, int N, int n, int m,
                                      const float* rec, const float* u_min,
                                      const float* u_max, const double* reg,
                                      int branch, const uint8_t* active,
                                      float* gains, int32_t* status,
                                      void* stream, int variant);
int pddp_riccati_backward_variant_f64(int B, int N, int n, int m,
                                      const double* rec, const double* u_min,
                                      const double* u_max, const double* reg,
                                      int branch, const uint8_t* active,
                                      double* gains, int32_t* status,
                                      void* stream, int variant);

/* ---- utils/constraint.py:150-266 boxqp() for one action dimension -------- */
/* `count` independent scalar QPs  min 0.5 Q x^2 + c x  s.t. lower <= x <= upper,
 * warm-started at x0: the projected-Newton loop of the reference with its
 * exit codes (`result`, constraint.py:23-32) and its `free` flag, exactly the
 * device routine the sweep calls.  All arrays [count]. */
int pddp_boxqp_m1_f32(int count, const float* x0, const float* Q,
                      const float* c, const float* lower, const float* upper,
                      float* x, int32_t* result, uint8_t* free_mask,
                      void* stream);
int pddp_boxqp_m1_f64(int count, const double* x0, const double* Q,
                      const double* c, const double* lower,
                      const double* upper, double* x, int32_t* result,
                      uint8_t* free_mask, void* stream);

/* The scalar BoxQP AS THE BENCHED SWEEP RUNS IT (csrc/riccati_n4_elem.hpp
 * elem_gains: ilqr.py:633-634 e = (Quu < 0 ? 1e-12 : Quu) + reg, then
 * constraint.py:150-266 on (x0, e, Qu, lower, upper) in the lean closed form
 * with v_rcp_f32: every exit test of the loop's two passes and its `free`
 * flag; not its Armijo back-tracking, which for one action returns the same
 * clamped Newton point in exact arithmetic - riccati_n4_elem.hpp QpLean1 has
 * the argument and the measured agreement; a curvature that is not positive
 * and finite goes to the closed form of pddp_boxqp_m1_* and the reference's
 * loop behind it): x = the feed-forward gain,
 * free_mask = 1 where the feedback row is not zeroed (the reference's possibly
 * stale `free`), status = PDDP_BWD_OK / _NAN / _BOXQP_FAILED; coeffs, nullable,
 * [count][3] = {s, c, w}: 1 / e or 0, and the two coefficients of the rank-one
 * value update V' = sym(Qzz) + c Quz Quz^T, V_z' = Qz + w Quz (ilqr.py:664-672
 * with K = -s Quz).  The unit-test entry of that routine. */
int pddp_boxqp_m1_lean_f32(int count, const float* x0, const float* Quu,
                           const float* Qu, const float* reg,
                           const float* lower, const float* upper, float* x,
                           uint8_t* free_mask, int32_t* status, float* coeffs,
                           void* stream);

/* ---- utils/constraint.py:150-266 boxqp() for m <= 4 action dimensions ------ */
/* `count` independent QPs  min 0.5 x^T Q x + c^T x  s.t. lower <= x <= upper,
 * warm-started at x0; the routine the generic sweep calls (csrc/gains.hpp),
 * one lane per problem.  x0, c, lower, upper, x [count][m]; Q [count][m][m];
 * result [count] (constraint.py:23-32); free_mask [count][m] (1 = free, the
 * possibly stale set of constraint.py:191-204); Ufree [count][m][m] = upper
 * Cholesky factor of the free block with identity rows / columns in place of
 * the clamped dimensions (the reference returns the compacted block).
 * PDDP_E_UNSUPPORTED for m > 4. */
int pddp_boxqp_f32(int count, int m, const float* x0, const float* Q,
                   const float* c, const float* lower, const float* upper,
                   float* x, int32_t* result, float* Ufree,
                   uint8_t* free_mask, void* stream);
int pddp_boxqp_f64(int count, int m, const double* x0, const double* Q,
                   const double* c, const double* lower, const double* upper,
                   double* x, int32_t* result, double* Ufree,
                   uint8_t* free_mask, void* stream);

/* Packs reference-layout tensors (what ilqr.py:393-486 forward() returns,
 * with a leading batch axis) into records, for plugin models whose
 * derivatives come from elsewhere.  F_z [B][N][n][n], F_u [B][N][n][m],
 * L_z [B][N+1][n], L_u [B][N][m], L_zz [B][N+1][n][n], L_uz [B][N][m][n],
 * L_uu [B][N][m][m], U [B][N][m] (nullable -> zeros). */
int pddp_pack_records_f32(int B, int N, int n, int m, const float* F_z,
                          const float* F_u, const float* L_z, const float* L_u,
                          const float* L_zz, const float* L_uz,
                          const float* L_uu, const float* U, float* rec,
                          void* stream);
int pddp_pack_records_f64(int B, int N, int n, int m, const double* F_z,
                          const double* F_u, const double* L_z,
                          const double* L_u, const double* L_zz,
                          const double* L_uz, const double* L_uu,
                          const double* U, double* rec, void* stream);

/* Trajectory cost J[b] = sum_t L[b][t] (ilqr.py:484 `L.sum()`), summed in t
 * order by one lane per trajectory: the result does not depend on the
 * trajectory's position in the batch.  L [B][count], J [B]. */
int pddp_sum_stage_costs_f32(int B, int count, const float* L, float* J,
                             void* stream);
int pddp_sum_stage_costs_f64(int B, int count, const double* L, double* J,
                             void* stream);

/* ---- ilqr.py:393-486 forward(): derivative rollout for the sample
 * problems (analytic; replaces utils/evaluation.py:134-288 autograd) ------ */
/* Nominal rollout Z[b][0] = z0[b], Z[b][t+1] = model(Z[b][t], clamp(U[b][t]))
 * (ilqr.py:457-468).  problem: host pointer, copied by value into the launch.
 * z0 [B][n]; U [B][N][m]; u_min/u_max [m] nullable (ilqr.py:461-462);
 * mask [B] nullable (0 -> trajectory skipped); Z [B][N+1][n] out. */
int pddp_nominal_rollout_f32(const pddp_problem* problem, int B, int N,
                             const float* z0, const float* U,
                             const float* u_min, const float* u_max,
                             const uint8_t* mask, float* Z, void* stream);
int pddp_nominal_rollout_f64(const pddp_problem* problem, int B, int N,
                             const double* z0, const double* U,
                             const double* u_min, const double* u_max,
                             const uint8_t* mask, double* Z, void* stream);

/* Derivative records along a given nominal (Z, U): F_z, F_u, L_z .. L_uu at
 * every (b, t) (ilqr.py:464-473), parallel over b AND t.
 * rec [B][N+1][stride] out; L [B][N+1] out; J [B] out = L.sum() (ilqr.py:209);
 * state [B] nullable: set to UNDEFINED for computed trajectories
 * (ilqr.py:212). */
int pddp_derivs_f32(const pddp_problem* problem, int B, int N, const float* Z,
                    const float* U, const float* u_min, const float* u_max,
                    const uint8_t* mask, float* rec, float* L, float* J,
                    int32_t* state, void* stream);
int pddp_derivs_f64(const pddp_problem* problem, int B, int N, const double* Z,
                    const double* U, const double* u_min, const double* u_max,
                    const uint8_t* mask, double* rec, double* L, double* J,
                    int32_t* state, void* stream);

/* ---- ilqr.py:677-723 _control_law() + :764-791 _trajectory_cost() ------- */
/* A candidate step sizes per trajectory.  Z [B][N+1][n], U [B][N][m] nominal;
 * gains [B][N][m+m*n]; alphas [A]; bwd_status [B] nullable (non-zero ->
 * skipped, the reference never reaches the line search then, ilqr.py:140-145);
 * Zc [B][N+1][A][n], Uc [B][N][A][m] candidates out (time-major, the
 * reference's Z_new / U_new per trajectory: the A rollouts of a trajectory
 * write one contiguous segment per step), Jc [B][A] out. */
int pddp_line_search_f32(const pddp_problem* problem, int B, int N, int A,
                         const float* Z, const float* U, const float* gains,
                         const float* alphas, const float* u_min,
                         const float* u_max, const uint8_t* active,
                         const int32_t* bwd_status, float* Zc, float* Uc,
                         float* Jc, void* stream);
int pddp_line_search_f64(const pddp_problem* problem, int B, int N, int A,
                         const double* Z, const double* U, const double* gains,
                         const double* alphas, const double* u_min,
                         const double* u_max, const uint8_t* active,
                         const int32_t* bwd_status, double* Zc, double* Uc,
                         double* Jc, void* stream);

/* ---- the same three operations with a PER-TRAJECTORY problem -------------
 * (the batch_* kernels of csrc/problem_kernels.hip).  `table`
 * [B][PDDP_BATCH_ROW], device memory of the run's dtype: row b holds
 * trajectory b's model parameters and goals,
 *   [PDDP_BATCH_PARAMS .. +7]  params  (pddp_problem.params order: dt first,
 *                                       then the model's constants)
 *   [PDDP_BATCH_X_GOAL .. +7]  x_goal  (augmented coordinates, PDDP_MAX_AUG)
 *   [PDDP_BATCH_U_GOAL .. +3]  u_goal  (PDDP_MAX_ACTION)
 * Entries beyond the model's sizes are ignored.  Q, Q_term, R, the model, the
 * encoding and the action bounds are shared: those of `problem`, whose own
 * params / x_goal / u_goal are not read by the kernels.  An f32 row is 80
 * bytes, an f64 row 160: rows are 16-byte aligned when the base is.
 * Every other argument is its uniform namesake's.  Domain: the four sample
 * models under PDDP_ENC_IGNORE_UNCERTAINTY (PDDP_E_UNSUPPORTED for any other
 * encoding); table == NULL: PDDP_E_BADARG.  The line search takes any A. */
#define PDDP_BATCH_ROW 20
#define PDDP_BATCH_PARAMS 0
#define PDDP_BATCH_X_GOAL 8
#define PDDP_BATCH_U_GOAL 16
int pddp_nominal_rollout_batch_f32(const pddp_problem* problem,
                                   const float* table, int B, int N,
                                   const float* z0, const float* U,
                                   const float* u_min, const float* u_max,
                                   const uint8_t* mask, float* Z, void* stream);
int pddp_nominal_rollout_batch_f64(const pddp_problem* problem,
                                   const double* table, int B, int N,
                                   const double* z0, const double* U,
                                   const double* u_min, const double* u_max,
                                   const uint8_t* mask, double* Z,
                                   void* stream);
int pddp_derivs_batch_f32(const pddp_problem* problem, const float* table,
                          int B, int N, const float* Z, const float* U,
                          const float* u_min, const float* u_max,
                          const uint8_t* mask, float* rec, float* L, float* J,
                          int32_t* state, void* stream);
int pddp_derivs_batch_f64(const pddp_problem* problem, const double* table,
                          int B, int N, const double* Z, const double* U,
                          const double* u_min, const double* u_max,
                          const uint8_t* mask, double* rec, double* L,
                          double* J, int32_t* state, void* stream);
int pddp_line_search_batch_f32(const pddp_problem* problem, const float* table,
                               int B, int N, int A, const float* Z,
                               const float* U, const float* gains,
                               const float* alphas, const float* u_min,
                               const float* u_max, const uint8_t* active,
                               const int32_t* bwd_status, float* Zc, float* Uc,
                               float* Jc, void* stream);
int pddp_line_search_batch_f64(const pddp_problem* problem,
                               const double* table, int B, int N, int A,
                               const double* Z, const double* U,
                               const double* gains, const double* alphas,
                               const double* u_min, const double* u_max,
                               const uint8_t* active,
                               const int32_t* bwd_status, double* Zc,
                               double* Uc, double* Jc, void* stream);

/* ---- pddp.py:209-245 _apply_controller() with ilqr.py:318-355 forward() as
 * the controller, batched and with the sample models as the plant: S
 * closed-loop rollouts of every trajectory's policy (Z, U, K), each from its
 * own initial state on its own plant (csrc/closed_loop.hip).  Rollout (b, s):
 *
 *   x_0 = z0s[b][s]                      (z0s == NULL: Z[b][0])
 *   u_t = clamp(U[b][t] + K[b][t] (x_t - Z[b][t]))     t = 0 .. N-1
 *         (gains == NULL: the open-loop action tensor form, u_t = clamp(U[b][t]);
 *          bounds NULL together: no clamp; the clamped action is what is applied,
 *          recorded and costed, as in pddp_line_search_*)
 *   J += l(x_t, u_t);  x_{t+1} = plant_{b,s}(x_t, u_t);  J += l_f(x_N)
 *
 * Z [B][N+1][n], U [B][N][m] the nominal; gains [B][N][m + m n] in the sweep's
 * layout (the K part only is read; gains_acc of pddp_accept_* is the
 * reference's self._K); z0s [B][S][n]; plant [B][S][PDDP_BATCH_ROW], rows in
 * the table's layout above (params | x_goal | u_goal): the dynamics AND the
 * cost of rollout (b, s) are that row's; plant == NULL: every rollout runs
 * `problem`'s own params and goals.  Q, Q_term, R, the model and the encoding
 * are `problem`'s, as for the _batch_ entry points.
 * Xc [B][N+1][S][n], Uc [B][N][S][m] out, time-major like Zc / Uc of the line
 * search (the rollouts of a trajectory write one contiguous segment per step);
 * both or neither: with NULL nothing but costs leaves the chip.  Jc [B][S]
 * out, required.  stats [B][4] out, nullable: {mean, min, max of the finite
 * costs, number of finite costs} of trajectory b, reduced inside the launch in
 * an order that depends on S alone (the same controller gives the same bits
 * wherever it sits in the batch); no finite cost: mean = min = max = +inf,
 * count 0.  active [B] nullable: trajectories with active[b] == 0 are skipped,
 * nothing of theirs is read or written.
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY, any
 * B, N, S >= 1.  PDDP_E_BADARG: a null required pointer, a non-positive size,
 * exactly one of Xc / Uc; PDDP_E_UNSUPPORTED: any other encoding; both before
 * any HIP call. */
int pddp_closed_loop_f32(const pddp_problem* problem, int B, int N, int S,
                         const float* Z, const float* U, const float* gains,
                         const float* z0s, const float* plant,
                         const float* u_min, const float* u_max,
                         const uint8_t* active, float* Xc, float* Uc,
                         float* Jc, float* stats, void* stream);
int pddp_closed_loop_f64(const pddp_problem* problem, int B, int N, int S,
                         const double* Z, const double* U, const double* gains,
                         const double* z0s, const double* plant,
                         const double* u_min, const double* u_max,
                         const uint8_t* active, double* Xc, double* Uc,
                         double* Jc, double* stats, void* stream);

/* ---- pddp_closed_loop_* under process and measurement noise drawn on the
 * device (csrc/closed_loop.hip; the reference has no counterpart).
 * Rollout (b, s), t = 0 .. N-1, in this order:
 *
 *   y   = x_t + v_std (.) v_t                (v_std == NULL: y = x_t)
 *   u_t = clamp(U[b][t] + K[b][t] (y - Z[b][t]))  (gains == NULL: clamp(U[b][t]))
 *   record x_t, u_t;  J += l(x_t, u_t)       (the true state, the applied
 *                                             action, the plant row's goals)
 *   x_{t+1} = plant_{b,s}(x_t, u_t) + w_std (.) w_t    (w_std == NULL: + 0)
 *
 * then J += l_f(x_N).  w_std, v_std [n], the launch's, of the run's type, not
 * both NULL.  Every other argument, the output layout, the statistics and
 * their order are pddp_closed_loop_*'s.
 *
 * w_t (stream 0) and v_t (stream 1) are n unit normals each, a pure function
 * of (seed, rollout, step, stream, component) - no generator state, no noise
 * tensor; the same seed gives the same noise to another controller:
 *   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter
 *     r = sample_offset + b S + s  (uint64);
 *     (c0, c1, c2, c3) = (r & 0xffffffff, r >> 32, t, (stream << 16) | k);
 *   _f32: call k gives components 4k .. 4k+3: u(x) = ((x >> 9) + 0.5) 2^-23,
 *     (z0, z1) = sqrt(-2 ln u(x0)) (cos, sin)(2 pi u(x1)), (z2, z3) likewise
 *     from (x2, x3);
 *   _f64: call k gives components 2k, 2k+1:
 *     u(hi, lo) = (((hi << 20) | (lo >> 12)) + 0.5) 2^-52,
 *     (z0, z1) = sqrt(-2 ln u(x0, x1)) (cos, sin)(2 pi u(x2, x3));
 *   components beyond n are discarded.  `sample_offset` places a launch's
 *   rollouts in a longer sequence: trajectories b0.. of a batch, run alone with
 *   sample_offset + b0 S, see the noise they saw in the batch.
 *
 * pddp_closed_loop_draws_* writes those unit normals, W [B][N][S][n]
 * (time-major like Xc), `which` 0 = w, 1 = v, through the rollouts' own device
 * function: for tests, and to replay one rollout's noise elsewhere (e.g. as
 * pddp_mpc_advance_*'s disturbance).
 * PDDP_E_BADARG: what pddp_closed_loop_* refuses; w_std == v_std == NULL;
 * draws: a null W, a non-positive size, which not 0 or 1, n > PDDP_MAX_STATE.
 * PDDP_E_UNSUPPORTED: any encoding but PDDP_ENC_IGNORE_UNCERTAINTY.  All
 * before any HIP call. */
int pddp_closed_loop_noisy_f32(const pddp_problem* problem, int B, int N, int S,
                               const float* Z, const float* U,
                               const float* gains, const float* z0s,
                               const float* plant, const float* u_min,
                               const float* u_max, const float* w_std,
                               const float* v_std, uint64_t seed,
                               uint64_t sample_offset, const uint8_t* active,
                               float* Xc, float* Uc, float* Jc, float* stats,
                               void* stream);
int pddp_closed_loop_noisy_f64(const pddp_problem* problem, int B, int N, int S,
                               const double* Z, const double* U,
                               const double* gains, const double* z0s,
                               const double* plant, const double* u_min,
                               const double* u_max, const double* w_std,
                               const double* v_std, uint64_t seed,
                               uint64_t sample_offset, const uint8_t* active,
                               double* Xc, double* Uc, double* Jc,
                               double* stats, void* stream);
int pddp_closed_loop_draws_f32(int B, int N, int S, int n, int which,
                               uint64_t seed, uint64_t sample_offset,
                               float* W /* [B][N][S][n] */, void* stream);
int pddp_closed_loop_draws_f64(int B, int N, int S, int n, int which,
                               uint64_t seed, uint64_t sample_offset,
                               double* W /* [B][N][S][n] */, void* stream);

/* ---- sampled shooting: S perturbed copies of every trajectory's action
 * sequence rolled out open loop, the cheapest found inside the launch and only
 * its states and actions written (csrc/shoot.hip; the reference has no
 * counterpart).  Candidate (b, s), with r = sample_offset + b S + s (uint64)
 * and t = 0 .. N-1:
 *
 *   x_0  = z0[b]
 *   xi_t = the m unit normals of (seed, r, t, stream 2): the draws of
 *          pddp_closed_loop_noisy_* above with counter
 *          (r & 0xffffffff, r >> 32, t, (2 << 16) | k), components beyond m
 *          discarded
 *   e_0  = xi_0;  e_t = fma(beta, e_{t-1}, gamma xi_t)     (AR(1), unit variance)
 *          beta = smooth, gamma = sqrt(1 - beta^2) formed on the host in double,
 *          both then cast to the run's type; gamma xi_t is rounded, then ONE fma
 *   u_t  = clamp(fma(a_std, e_t, U[b][t]))     s >= 1
 *   u_t  = clamp(U[b][t])                      s == 0: the base sequence is a
 *          candidate, so the result is never worse than where it started
 *   J += l(x_t, u_t);  x_{t+1} = f_b(x_t, u_t);  then J += l_f(x_N)
 *
 * The clamped action is what is applied, costed and written (bounds NULL
 * together: no clamp).  pddp_shoot_batch_* takes `table` [B][PDDP_BATCH_ROW]:
 * trajectory b runs row b's parameters and goals, as pddp_line_search_batch_*.
 * z0 [B][n]; U [B][N][m] the base sequence; a_std [m], of the run's type,
 * entries >= 0 the caller's business; smooth in [0, 1).
 *
 * Jc [B][S] out: every candidate's cost.  best [B] out: the s of the lowest
 * FINITE Jc[b][s], ties to the lower s; no finite cost: best[b] = -1,
 * J_best[b] = +inf and row b of Z_out / U_out is not written.  J_best [B] out,
 * nullable: the bits of Jc[b][best[b]].  Z_out [B][N+1][n], U_out [B][N][m]
 * out, both or neither: the winner's states and applied actions - the winner
 * is rolled out a second time inside the launch by the instructions that
 * summed its cost, with their stores enabled; no [B][N][S][.] tensor exists.
 * The argmin meets in an order that depends on S alone (the lane's own
 * candidates in s order, a butterfly over its lane group comparing (J, s)
 * lexicographically, then the wavefronts in their order; no atomics): a
 * trajectory gets the same bits wherever it sits in the batch, and run alone
 * with sample_offset + b S it gets the draws it had in the batch.
 * active [B] nullable: trajectories with active[b] == 0 are skipped, nothing of
 * theirs is read or written.
 *
 * pddp_shoot_draws_* writes the unit normals xi, E [B][N][S][m], through the
 * rollouts' own device function: for tests and to replay a candidate.
 * (pddp_closed_loop_draws_* keeps to streams 0 and 1.)
 *
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: a null required pointer (problem, z0, U, a_std, Jc, best; the
 * table of _batch_); non-positive B, N or S; B S > 0x7fffffff; exactly one of
 * Z_out / U_out; U_out == U or Z_out == z0 (the caller owns a second buffer);
 * smooth outside [0, 1) or NaN; draws: a null E, a non-positive size,
 * m > PDDP_MAX_ACTION.  PDDP_E_UNSUPPORTED: any other encoding.  All before
 * any HIP call. */
int pddp_shoot_f32(const pddp_problem* problem, int B, int N, int S,
                   const float* z0, const float* U, const float* u_min,
                   const float* u_max, const float* a_std, double smooth,
                   uint64_t seed, uint64_t sample_offset,
                   const uint8_t* active, float* Jc, int32_t* best,
                   float* J_best, float* Z_out, float* U_out, void* stream);
int pddp_shoot_f64(const pddp_problem* problem, int B, int N, int S,
                   const double* z0, const double* U, const double* u_min,
                   const double* u_max, const double* a_std, double smooth,
                   uint64_t seed, uint64_t sample_offset,
                   const uint8_t* active, double* Jc, int32_t* best,
                   double* J_best, double* Z_out, double* U_out, void* stream);
int pddp_shoot_batch_f32(const pddp_problem* problem, const float* table,
                         int B, int N, int S, const float* z0, const float* U,
                         const float* u_min, const float* u_max,
                         const float* a_std, double smooth, uint64_t seed,
                         uint64_t sample_offset, const uint8_t* active,
                         float* Jc, int32_t* best, float* J_best, float* Z_out,
                         float* U_out, void* stream);
int pddp_shoot_batch_f64(const pddp_problem* problem, const double* table,
                         int B, int N, int S, const double* z0,
                         const double* U, const double* u_min,
                         const double* u_max, const double* a_std,
                         double smooth, uint64_t seed, uint64_t sample_offset,
                         const uint8_t* active, double* Jc, int32_t* best,
                         double* J_best, double* Z_out, double* U_out,
                         void* stream);
int pddp_shoot_draws_f32(int B, int N, int S, int m, uint64_t seed,
                         uint64_t sample_offset, float* E /* [B][N][S][m] */,
                         void* stream);
int pddp_shoot_draws_f64(int B, int N, int S, int m, uint64_t seed,
                         uint64_t sample_offset, double* E /* [B][N][S][m] */,
                         void* stream);

/* ---- sampled shooting with a softmin-weighted (MPPI) update: the candidates
 * of pddp_shoot_* above, and instead of the cheapest one the weighted mean of
 * all their perturbations added to the base sequence, that sequence rolled out
 * and costed inside the launch (csrc/mppi.hip; the reference has no
 * counterpart).  Trajectory b, candidate s, r = sample_offset + b S + s:
 *
 *   Jc[b][s], best[b], J_best[b]   pddp_shoot_*'s law, word for word (stream 2,
 *                                  the AR(1) with explicit fmas, candidate 0 the
 *                                  base, the clamp, the lowest finite cost, ties
 *                                  to the lower s)
 *   a_s   = (Jc[b][s] - J_best[b]) / lam[b]    (the difference, then the quotient)
 *   w_s   = exp(-a_s) where Jc[b][s] is finite, else 0     (w_best = 1: eta >= 1)
 *   eta   = sum_s w_s;   W[b][s] = w_s / eta
 *   ebar_t = (sum_{s>=1} w_s e_{s,t}) / eta    e_{s,t}: the RAW AR(1) value,
 *                                  before a_std and the clamp; every product is
 *                                  rounded before it is summed; candidate 0 adds
 *                                  w_0 to eta and nothing to the sum
 *   Uw[b][t] = clamp(fma(a_std, ebar_t, U[b][t]))
 *   Zw[b]    = the open-loop rollout of Uw[b] from z0[b] under f_b;  J_w[b] = its
 *              cost (stage costs in t order, then the terminal one)
 *
 * The order of every sum depends on S alone, never on b or B.  With G the lane
 * group of S (pddp_closed_loop_*'s mapping: S rounded up to a power of two up to
 * 64, then to whole wavefronts up to 256) lane l of the group holds the
 * candidates s = l, l + G, ... ("turns").  eta: a lane's own weights in s order,
 * then the group.  sum_s w_s e_{s,t}, per step t and component: the group's sum
 * of turn 0, then that of turn 1 added to it, and so on.  A sum over the group
 * is a butterfly over its lanes of a wavefront with partner distances 1, 2, 4,
 * ... (both partners form the same sum; lanes without a candidate, and
 * candidates whose weight is 0, add +0), then the wavefronts in their order.
 * No atomics: a trajectory's outputs are the same bits wherever it sits in the
 * batch, and with sample_offset + b0 S they are the same bits when trajectories
 * b0.. run alone.
 *
 * Arguments beside pddp_shoot_*'s: lam [B], one temperature per trajectory in
 * cost units; lam[b] <= 0 or NaN is treated as "no finite candidate".  W [B][S]
 * out, nullable.  J_w [B] out.  Z_out [B][N+1][n] / U_out [B][N][m], both or
 * neither, receive Zw / Uw (shoot's aliasing rules); with S > 256 the running
 * sum over a lane's turns is kept in U_out, so both are required then.  Without
 * a finite candidate: best[b] = -1, J_best[b] = J_w[b] = +inf, row b of W is
 * zeros and row b of Z_out / U_out is not written (Jc[b] is).  active [B]
 * nullable: nothing of a skipped trajectory is read or written.
 *
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: pddp_shoot_*'s list; a null lam or J_w; S > 256 without
 * Z_out / U_out.  PDDP_E_UNSUPPORTED: any other encoding.  All before any HIP
 * call. */
int pddp_mppi_f32(const pddp_problem* problem, int B, int N, int S,
                  const float* z0, const float* U, const float* u_min,
                  const float* u_max, const float* a_std, const float* lam,
                  double smooth, uint64_t seed, uint64_t sample_offset,
                  const uint8_t* active, float* Jc, int32_t* best,
                  float* J_best, float* W, float* J_w, float* Z_out,
                  float* U_out, void* stream);
int pddp_mppi_f64(const pddp_problem* problem, int B, int N, int S,
                  const double* z0, const double* U, const double* u_min,
                  const double* u_max, const double* a_std, const double* lam,
                  double smooth, uint64_t seed, uint64_t sample_offset,
                  const uint8_t* active, double* Jc, int32_t* best,
                  double* J_best, double* W, double* J_w, double* Z_out,
                  double* U_out, void* stream);
int pddp_mppi_batch_f32(const pddp_problem* problem, const float* table,
                        int B, int N, int S, const float* z0, const float* U,
                        const float* u_min, const float* u_max,
                        const float* a_std, const float* lam, double smooth,
                        uint64_t seed, uint64_t sample_offset,
                        const uint8_t* active, float* Jc, int32_t* best,
                        float* J_best, float* W, float* J_w, float* Z_out,
                        float* U_out, void* stream);
int pddp_mppi_batch_f64(const pddp_problem* problem, const double* table,
                        int B, int N, int S, const double* z0,
                        const double* U, const double* u_min,
                        const double* u_max, const double* a_std,
                        const double* lam, double smooth, uint64_t seed,
                        uint64_t sample_offset, const uint8_t* active,
                        double* Jc, int32_t* best, double* J_best, double* W,
                        double* J_w, double* Z_out, double* U_out,
                        void* stream);

/* ---- sampled shooting with a cross-entropy (CEM) refit: the candidates of
 * pddp_shoot_* above drawn with a width per time step and action component
 * around the mean U, the K cheapest ("elites") ranked out inside the launch,
 * and the mean AND the width refitted to them; the new mean rolled out and
 * costed inside the launch (csrc/cem.hip; the reference has no counterpart).
 * Trajectory b, candidate s, r = sample_offset + b S + s:
 *
 *   e_{s,t}          pddp_shoot_*'s draws and AR(1), word for word (stream 2,
 *                    explicit fmas)
 *   u_{s,t}[j]     = clamp(fma(sigma[b][t][j], e_{s,t}[j], U[b][t][j]))    s >= 1
 *   u_{0,t}        = clamp(U[b][t])                  the mean is a candidate
 *   Jc[b][s]         the open-loop cost, as pddp_shoot_*
 *   rank[b][s]     = #{ s' : Jc[b][s'] finite and (Jc[b][s'], s') <
 *                    (Jc[b][s], s) lexicographically } where Jc[b][s] is
 *                    finite, else -1
 *   Ke[b]          = min(K, number of finite costs)
 *   elite(s)      <=> 0 <= rank[b][s] < K
 *   best[b]        = the s of rank 0 (-1 without a finite cost);
 *   J_best[b]      = the bits of Jc[b][best[b]]
 *   s1_t[j]        = sum over elites s >= 1 of e_{s,t}[j]
 *   s2_t[j]        = sum over elites s >= 1 of fma(e, e, 0)   (each term rounded
 *                    before it meets a sum; candidate 0 counts in Ke and adds
 *                    nothing)
 *   ebar           = s1 / Ke
 *   V              = Ke > 1 ? max(fma(-ebar, ebar, s2 / Ke), 0) : 0
 *   g              = step * sigma[b][t][j]          (rounded)
 *   Um[b][t][j]    = clamp(fma(g, ebar, U[b][t][j]))
 *   sd             = sigma[b][t][j] * sqrt(V)       (rounded)
 *   Sm[b][t][j]    = max(fma(step, sd - sigma[b][t][j], sigma[b][t][j]),
 *                        std_min[j])
 *   Zm[b], J_m[b]    the open-loop rollout of Um[b] from z0[b] under f_b, and
 *                    its cost (stage costs in t order, then the terminal one)
 *
 * The refit is in the raw AR(1) values e, as pddp_mppi_*'s mean is: they are
 * of unit scale whatever the width has become, so the variance does not cancel
 * badly when the distribution narrows.  step = 1 - mix, formed on the host in
 * double and then cast to the run's type: mix = 0 replaces the distribution by
 * the elites' fit, mix towards 1 keeps more of the old one.
 *
 * Arguments beside pddp_shoot_*'s: K, 1 <= K <= S, after S; sigma [B][N][m] in
 * a_std's place, entries >= 0 the caller's business; std_min [m] behind it,
 * nullable: zeros; mix in [0, 1) next to smooth.  Jc [B][S] out.  rank [B][S]
 * int32 out, nullable.  best [B] out.  J_best [B] out, nullable.  n_elite [B]
 * int32 out: Ke.  J_m [B] out.  Z_out [B][N+1][n], U_out [B][N][m], S_out
 * [B][N][m] out, all three or none, receive Zm, Um, Sm (shoot's aliasing
 * rules, S_out against sigma as U_out against U); with S > 256 the running
 * sums over a lane's turns are kept in U_out (s1) and S_out (s2), so the three
 * are required then.  Without a finite cost: best[b] = -1, J_best[b] = J_m[b]
 * = +inf, n_elite[b] = 0, the ranks are -1 and row b of Z_out / U_out / S_out
 * is not written (Jc[b] is).  active [B] nullable: nothing of a skipped
 * trajectory is read or written.  pddp_cem_batch_* takes `table`
 * [B][PDDP_BATCH_ROW] as pddp_mppi_batch_*.
 *
 * The order of every sum and of the ranking depends on S alone, never on b or
 * B.  The ranking is exact integer work on (Jc, s).  s1 and s2, per step and
 * component, with G and the turns as pddp_mppi_*'s: the group's sum of turn 0,
 * then that of turn 1 added to it, and so on; a sum over the group is the
 * butterfly with partner distances 1, 2, 4, ... (lanes without an elite add
 * +0), then the wavefronts in their order.  No atomics: a trajectory's outputs
 * are the same bits wherever it sits in the batch, and with sample_offset +
 * b0 S they are the same bits when trajectories b0.. run alone.
 *
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: pddp_shoot_*'s list, with sigma in a_std's place; a null
 * n_elite or J_m; K < 1 or K > S; mix outside [0, 1) or NaN; some but not all
 * of Z_out / U_out / S_out; U_out == U, S_out == sigma or Z_out == z0; S > 256
 * without the rows.  PDDP_E_UNSUPPORTED: any other encoding.  All before any
 * HIP call. */
int pddp_cem_f32(const pddp_problem* problem, int B, int N, int S, int K,
                 const float* z0, const float* U, const float* u_min,
                 const float* u_max, const float* sigma, const float* std_min,
                 double smooth, double mix, uint64_t seed,
                 uint64_t sample_offset, const uint8_t* active, float* Jc,
                 int32_t* rank, int32_t* best, float* J_best, int32_t* n_elite,
                 float* J_m, float* Z_out, float* U_out, float* S_out,
                 void* stream);
int pddp_cem_f64(const pddp_problem* problem, int B, int N, int S, int K,
                 const double* z0, const double* U, const double* u_min,
                 const double* u_max, const double* sigma,
                 const double* std_min, double smooth, double mix,
                 uint64_t seed, uint64_t sample_offset, const uint8_t* active,
                 double* Jc, int32_t* rank, int32_t* best, double* J_best,
                 int32_t* n_elite, double* J_m, double* Z_out, double* U_out,
                 double* S_out, void* stream);
int pddp_cem_batch_f32(const pddp_problem* problem, const float* table, int B,
                       int N, int S, int K, const float* z0, const float* U,
                       const float* u_min, const float* u_max,
                       const float* sigma, const float* std_min, double smooth,
                       double mix, uint64_t seed, uint64_t sample_offset,
                       const uint8_t* active, float* Jc, int32_t* rank,
                       int32_t* best, float* J_best, int32_t* n_elite,
                       float* J_m, float* Z_out, float* U_out, float* S_out,
                       void* stream);
int pddp_cem_batch_f64(const pddp_problem* problem, const double* table, int B,
                       int N, int S, int K, const double* z0, const double* U,
                       const double* u_min, const double* u_max,
                       const double* sigma, const double* std_min,
                       double smooth, double mix, uint64_t seed,
                       uint64_t sample_offset, const uint8_t* active,
                       double* Jc, int32_t* rank, int32_t* best,
                       double* J_best, int32_t* n_elite, double* J_m,
                       double* Z_out, double* U_out, double* S_out,
                       void* stream);

/* ---- a receding-horizon MPPI trial, every control step inside ONE launch:
 * plan by K iterations of pddp_mppi_*'s law around the plan U, apply the first
 * action to the plant, observe, shift the plan (csrc/mppi_trial.hip; the
 * reference has no counterpart).  Trajectory b is live when active is NULL or
 * active[b] != 0; control step c runs over t0 .. t0 + count - 1 of TT:
 *
 *   1. plan.  For k = 0 .. K-1: pddp_mppi_*'s law above, word for word, from
 *      x_0 = z0[b] under the controller's model (the shared problem with row b
 *      of `table` written over it), the base U[b], candidate (b, s) rollout
 *        r = cand_offset + (c K + k) iter_stride + b S + s          (uint64)
 *      of stream 2: Jc, best, J_best, eta, the weights, Uw (into U_work) and
 *      J_w.  J0_log[b][c][k] = Jc[b][0]; Jw_log[b][c][k] = J_w;
 *      took = isfinite(J_w) && J_w <= Jc[b][0]; where it holds U[b] = Uw, else
 *      U[b] stays (no finite candidate, or lam[b] not positive: J_w = +inf).
 *      ess_log[b][c] = eta^2 / sum_s w_s^2 of the last iteration (w and w^2
 *      summed together, in eta's order), 0 without a finite candidate;
 *      plan_log[b][c] = U[b] after the K iterations.
 *   2. apply (pddp_mpc_advance_noisy_*'s steps 2 - 4).  x = x_true[b] with
 *      v_std, else z0[b]; u = clamp(U[b][0]); Xlog[b][c] = x; Ulog[b][c] = u;
 *      Jcl[b] (read if c > 0, else 0) += l(x, u) under the plant row's goals;
 *      x' = f_plant(x, u) + disturbance[b][c], then with w_std
 *      x' = fma(w_std, w(seed, rollout_offset + b, step_offset + c, stream 0),
 *      x') per component; at c == TT-1: Xlog[b][TT] = x', Jcl[b] += l_f(x').
 *   3. observe.  With v_std: x_true[b] = x', y' = fma(v_std, v(seed,
 *      rollout_offset + b, step_offset + c + 1, stream 1), x'),
 *      Ylog[b][c+1] = y'.  z0[b] = y', or x' without v_std.
 *   4. shift.  U[b][i] = U[b][i+1], the last row repeated: plain copies of
 *      unclamped words.
 *
 * After the last control step of the launch Z[b] is the rollout of the shifted
 * U[b], clamped, from z0[b] under the controller's model (the advance's step
 * 6).  No iLQR controller state is an argument.
 *
 * iter_stride: a solver passes B S, so that iteration (c, k) draws what
 * pddp_mppi_* draws with sample_offset = cand_offset + (c K + k) B S.  A run
 * of trajectories b0.. alone passes the ORIGINAL B S, cand_offset + b0 S and
 * rollout_offset + b0 and gets the same bits; so do count control steps in
 * one launch and in several (t0 advanced; z0, U, x_true, Jcl carried).
 *
 * Arguments, in this order:
 *   problem, table, plant     [B][PDDP_BATCH_ROW] or NULL each (plant NULL: the
 *                             controller's model)
 *   B, N, S, K, TT, t0, count
 *   z0 [B][n]                 in: what the controller sees at step t0; out: at
 *                             step t0 + count
 *   U [B][N][m]               in: the plan (unclamped words); out: shifted
 *   Z [B][N+1][n]             out, written once
 *   U_work [B][N][m]          workspace: the weighted sequence of an iteration
 *                             (S > 256: also the running sum of a lane's turns)
 *   u_min, u_max, a_std [m], lam [B], smooth      pddp_mppi_*'s
 *   seed                      ONE key: stream 2 the candidates, 0 / 1 the noises
 *   cand_offset, iter_stride  (uint64)
 *   disturbance [B][TT][n], w_std [n], v_std [n]  nullable each
 *   rollout_offset (uint64), step_offset, x_true [B][n]
 *                             pddp_mpc_advance_noisy_*'s, same meaning
 *   active [B]                nullable: nothing of a skipped trajectory is read
 *                             or written
 *   Jc, log_costs             Jc workspace [B][S]; log_costs != 0:
 *                             [B][TT][K][S], every iteration's costs kept
 *   Xlog [B][TT+1][n], Ulog [B][TT][m], Jcl [B]
 *   Ylog [B][TT+1][n]         nullable, written with v_std only (rows c + 1)
 *   J0_log [B][TT][K], Jw_log [B][TT][K], ess_log [B][TT],
 *   plan_log [B][TT][N][m]    nullable each
 *   stream
 *
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: pddp_mppi_*'s list (a null problem, z0, U, a_std, lam or Jc;
 * non-positive B, N or S; B S > 0x7fffffff; smooth outside [0, 1) or NaN);
 * K < 1, TT < 1, t0 < 0, count < 1, t0 + count > TT; a null Z, U_work, Xlog,
 * Ulog or Jcl; U_work == U; v_std without x_true; step_offset < 0 or
 * step_offset + TT beyond an int.  PDDP_E_UNSUPPORTED: any other encoding.  All
 * before any HIP call. */
int pddp_mppi_trial_f32(
    const pddp_problem* problem, const float* table, const float* plant, int B,
    int N, int S, int K, int TT, int t0, int count, float* z0, float* U,
    float* Z, float* U_work, const float* u_min, const float* u_max,
    const float* a_std, const float* lam, double smooth, uint64_t seed,
    uint64_t cand_offset, uint64_t iter_stride, const float* disturbance,
    const float* w_std, const float* v_std, uint64_t rollout_offset,
    int step_offset, float* x_true, const uint8_t* active, float* Jc,
    int log_costs, float* Xlog, float* Ulog, float* Jcl, float* Ylog,
    float* J0_log, float* Jw_log, float* ess_log, float* plan_log,
    void* stream);
int pddp_mppi_trial_f64(
    const pddp_problem* problem, const double* table, const double* plant,
    int B, int N, int S, int K, int TT, int t0, int count, double* z0,
    double* U, double* Z, double* U_work, const double* u_min,
    const double* u_max, const double* a_std, const double* lam, double smooth,
    uint64_t seed, uint64_t cand_offset, uint64_t iter_stride,
    const double* disturbance, const double* w_std, const double* v_std,
    uint64_t rollout_offset, int step_offset, double* x_true,
    const uint8_t* active, double* Jc, int log_costs, double* Xlog,
    double* Ulog, double* Jcl, double* Ylog, double* J0_log, double* Jw_log,
    double* ess_log, double* plan_log, void* stream);

/* ---- a receding-horizon CEM trial, every control step inside ONE launch:
 * plan by I iterations of pddp_cem_*'s law around a mean and a width, apply
 * the incumbent's first action to the plant, observe, shift the plan and the
 * width (csrc/cem_trial.hip; the reference has no counterpart).  The plain
 * objective only: the shared Q, Q_term, R, one goal per trajectory.
 * Trajectory b is live when active is NULL or active[b] != 0 and carries two
 * things between control steps, both in/out: the plan U[b] and the width
 * sigma[b] its next control step starts from.  Control step c runs over
 * t0 .. t0 + count - 1 of TT, from what the controller sees, y = z0[b]:
 *
 *   1. mean = U[b], width = sigma[b], incumbent = U[b].
 *   2. plan.  For k = 0 .. I-1: pddp_cem_*'s law above, word for word, from
 *      x_0 = y under the controller's model (the shared problem with row b of
 *      `table` written over it), with `mean` as U[b] and `width` as sigma[b],
 *      candidate (b, s) rollout
 *        r = cand_offset + (c I + k) iter_stride + b S + s          (uint64)
 *      of stream 2: Jc[b][.], the ranks, Ke, Um, Sm and J_m (+inf without a
 *      finite cost; Um, Sm are then not written).
 *        at k = 0: J_inc = Jc[b][0]  (the mean is candidate 0 and, at k = 0,
 *                  the incumbent);  Jtrace_log[b][c][0] = J_inc
 *        Jm_log[b][c][k] = J_m;  nelite_log[b][c][k] = Ke
 *        better = isfinite(J_m) && J_m <= J_inc: incumbent = Um, J_inc = J_m
 *        moved  = Ke > 0:                        mean = Um, width = Sm
 *        Jtrace_log[b][c][k+1] = J_inc
 *      - the selects ILQRSolver.cem makes on the host between its launches.
 *   3. apply, observe.  plan_log[b][c] = incumbent; std_log[b][c] = width (the
 *      one after the last iteration, before step 5); u = clamp(incumbent[0]);
 *      then pddp_mppi_trial_*'s steps 2 and 3 word for word: Xlog, Ulog, Jcl,
 *      the disturbance, w and v of streams 0 / 1 at (seed, rollout_offset + b,
 *      step_offset + c [+ 1]), the terminal cost at c == TT-1, x_true, Ylog,
 *      z0[b].
 *   4. U[b][i] = incumbent[i+1], the last row repeated: plain copies of
 *      unclamped words.
 *   5. sigma[b] = sigma0[b] where sigma0 is given: every control step restarts
 *      from the caller's width.  Else sigma[b][i] = width[i+1], the last row
 *      repeated: the refitted width is carried; it is >= std_min.
 *
 * After the last control step of the launch Z[b] is the rollout of the shifted
 * U[b], clamped, from z0[b] under the controller's model.  The trial keeps no
 * rank array: the ranks follow exactly from the logged costs.
 *
 * iter_stride, a run of trajectories b0.. alone and count control steps in one
 * launch or in several: as pddp_mppi_trial_* (z0, U, sigma, x_true, Jcl
 * carried; the work buffers carry nothing between launches).
 *
 * Arguments, in this order:
 *   problem, table, plant     pddp_mppi_trial_*'s
 *   B, N, S, K, I, TT, t0, count      K: the elites, 1 <= K <= S; I >= 1
 *   z0 [B][n], U [B][N][m], Z [B][N+1][n]       pddp_mppi_trial_*'s
 *   mean, width, Um, Sm       [B][N][m] each, workspace: the distribution
 *                             inside a control step and an iteration's refit
 *                             (S > 256: Um, Sm also hold the running sums of a
 *                             lane's turns - the rows always exist here)
 *   u_min, u_max              pddp_cem_*'s
 *   sigma [B][N][m]           in: the width control step t0 starts from; out:
 *                             the one step t0 + count would start from
 *   sigma0 [B][N][m]          nullable, const
 *   std_min [m]               nullable: zeros
 *   smooth, mix               pddp_cem_*'s
 *   seed, cand_offset, iter_stride, disturbance, w_std, v_std,
 *   rollout_offset, step_offset, x_true, active
 *                             pddp_mppi_trial_*'s
 *   Jc, log_costs             Jc workspace [B][S]; log_costs != 0:
 *                             [B][TT][I][S], every iteration's costs kept
 *   Xlog, Ulog, Jcl, Ylog     pddp_mppi_trial_*'s
 *   Jtrace_log [B][TT][I+1], Jm_log [B][TT][I], nelite_log [B][TT][I] int32,
 *   plan_log [B][TT][N][m], std_log [B][TT][N][m]       nullable each
 *   stream
 *
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: what pddp_mppi_trial_* refuses (a null problem, z0, U or Jc;
 * non-positive B, N or S; B S > 0x7fffffff; smooth outside [0, 1) or NaN;
 * TT < 1, t0 < 0, count < 1, t0 + count > TT; a null Z, Xlog, Ulog or Jcl;
 * v_std without x_true; step_offset < 0 or step_offset + TT beyond an int);
 * K < 1 or K > S; I < 1; mix outside [0, 1) or NaN; a null sigma; a work
 * buffer (mean, width, Um, Sm) that is null or is another buffer of the call.
 * PDDP_E_UNSUPPORTED: any other encoding.  All before any HIP call. */
int pddp_cem_trial_f32(
    const pddp_problem* problem, const float* table, const float* plant, int B,
    int N, int S, int K, int I, int TT, int t0, int count, float* z0, float* U,
    float* Z, float* mean, float* width, float* Um, float* Sm,
    const float* u_min, const float* u_max, float* sigma, const float* sigma0,
    const float* std_min, double smooth, double mix, uint64_t seed,
    uint64_t cand_offset, uint64_t iter_stride, const float* disturbance,
    const float* w_std, const float* v_std, uint64_t rollout_offset,
    int step_offset, float* x_true, const uint8_t* active, float* Jc,
    int log_costs, float* Xlog, float* Ulog, float* Jcl, float* Ylog,
    float* Jtrace_log, float* Jm_log, int32_t* nelite_log, float* plan_log,
    float* std_log, void* stream);
int pddp_cem_trial_f64(
    const pddp_problem* problem, const double* table, const double* plant,
    int B, int N, int S, int K, int I, int TT, int t0, int count, double* z0,
    double* U, double* Z, double* mean, double* width, double* Um, double* Sm,
    const double* u_min, const double* u_max, double* sigma,
    const double* sigma0, const double* std_min, double smooth, double mix,
    uint64_t seed, uint64_t cand_offset, uint64_t iter_stride,
    const double* disturbance, const double* w_std, const double* v_std,
    uint64_t rollout_offset, int step_offset, double* x_true,
    const uint8_t* active, double* Jc, int log_costs, double* Xlog,
    double* Ulog, double* Jcl, double* Ylog, double* Jtrace_log,
    double* Jm_log, int32_t* nelite_log, double* plan_log, double* std_log,
    void* stream);

/* ---- the sampling planners under the line search's objective: pddp_shoot_*,
 * pddp_mppi_*, pddp_cem_* and pddp_mppi_trial_* above along a reference (a
 * goal per time step, pddp_line_search_track_*) and / or under per-trajectory
 * cost weights (pddp_line_search_weighted_*) (the *_goals_kernel of
 * csrc/shoot.hip, mppi.hip, cem.hip, mppi_trial.hip; the reference has no
 * counterpart).  Nothing changes in how candidates are drawn, clamped,
 * selected, ranked, weighted or summed: the four laws above hold word for
 * word.  Only the cost every rollout is summed under changes - the
 * candidates', the winner's second pass in shoot, the weighted sequence's in
 * mppi and the trial, the refitted mean's in cem:
 *
 *   P_b = the shared problem, the parameters of row b of `table` where one is
 *         given (with a reference the table's goal fields are NOT read), then,
 *         where weights are given, row b of `weights` [B][PDDP_WEIGHT_ROW]
 *         written over the diagonals of Q, Q_term, R
 *   J += l(x_t, u_t)  under row min(ref_t0 + t, ref_len - 1) of `ref`
 *                     [B][ref_len][PDDP_REF_ROW], trajectory b, t = 0 .. N-1
 *   J += l_f(x_N)     under row min(ref_t0 + N, ref_len - 1), x_goal only
 *
 * Without a reference the goals are the table's or the shared problem's.  The
 * cost is evaluated under the full mask: a weight may make a row live that
 * the shared Q leaves dead.  The S candidates of a trajectory share its
 * reference and its weights row.  With every reference row equal to the
 * table's goals and every weights row equal to the shared diagonals the
 * results agree with the _batch siblings' to rounding (another kernel), not to
 * the bit.
 *
 * Leading arguments, then the sibling's parameter list unchanged; `table` may
 * be NULL:
 *   _track_            (problem, table, ref, ref_len, ref_t0, ...)
 *   _weighted_         (problem, table, weights, ...)
 *   _track_weighted_   (problem, table, ref, ref_len, ref_t0, weights, ...)
 *
 * pddp_cem_track_*, pddp_cem_weighted_*, pddp_cem_track_weighted_*:
 * pddp_cem_*'s word for word, every rollout - the candidates' and the refitted
 * mean's - costed along the reference and / or under the weights.  The ranks,
 * the elites and both moments are pddp_cem_*'s on these costs; Um's step t is
 * costed under row min(ref_t0 + t, ref_len - 1), the terminal term of J_m
 * under row min(ref_t0 + N, ref_len - 1).
 *
 * pddp_mppi_trial_goals_* takes pddp_mppi_trial_*'s parameters with `ref,
 * ref_len, ref_t0, weights` after `plant`; both additions are nullable, at
 * least one of them is given.  Control step c (absolute in TT, as for the
 * noise) plans under the window that starts at row min(ref_t0 + c,
 * ref_len - 1).  The applied step is logged as pddp_mpc_advance_track_* logs
 * it, on the common yardstick: Jcl[b] += l(x, u) under row ref_t0 + c and the
 * SHARED Q, R; at c == TT-1 l_f(x') under row ref_t0 + c + 1 (both clamped)
 * and the shared Q_term; with a reference the plant row supplies parameters
 * only.  The weights affect planning only.  The final Z reads no goal.
 *
 * PDDP_E_BADARG: everything the sibling refuses; a null `weights` where the
 * name promises weights; a null `ref`, ref_len < 1 or ref_t0 < 0 where it
 * promises a reference; the trial: neither a reference nor weights, or (with
 * a reference) ref_len < 1, ref_t0 < 0, ref_t0 + TT beyond an int.  All before
 * any HIP call. */
#define PDDP_SHOOT_REST(T)                                                     \
  int B, int N, int S, const T* z0, const T* U, const T* u_min,                \
      const T* u_max, const T* a_std, double smooth, uint64_t seed,            \
      uint64_t sample_offset, const uint8_t* active, T* Jc, int32_t* best,     \
      T* J_best, T* Z_out, T* U_out, void* stream
#define PDDP_MPPI_REST(T)                                                      \
  int B, int N, int S, const T* z0, const T* U, const T* u_min,                \
      const T* u_max, const T* a_std, const T* lam, double smooth,             \
      uint64_t seed, uint64_t sample_offset, const uint8_t* active, T* Jc,     \
      int32_t* best, T* J_best, T* W, T* J_w, T* Z_out, T* U_out, void* stream
int pddp_shoot_track_f32(const pddp_problem* problem, const float* table,
                         const float* ref, int ref_len, int ref_t0,
                         PDDP_SHOOT_REST(float));
int pddp_shoot_track_f64(const pddp_problem* problem, const double* table,
                         const double* ref, int ref_len, int ref_t0,
                         PDDP_SHOOT_REST(double));
int pddp_shoot_weighted_f32(const pddp_problem* problem, const float* table,
                            const float* weights, PDDP_SHOOT_REST(float));
int pddp_shoot_weighted_f64(const pddp_problem* problem, const double* table,
                            const double* weights, PDDP_SHOOT_REST(double));
int pddp_shoot_track_weighted_f32(const pddp_problem* problem,
                                  const float* table, const float* ref,
                                  int ref_len, int ref_t0,
                                  const float* weights,
                                  PDDP_SHOOT_REST(float));
int pddp_shoot_track_weighted_f64(const pddp_problem* problem,
                                  const double* table, const double* ref,
                                  int ref_len, int ref_t0,
                                  const double* weights,
                                  PDDP_SHOOT_REST(double));
int pddp_mppi_track_f32(const pddp_problem* problem, const float* table,
                        const float* ref, int ref_len, int ref_t0,
                        PDDP_MPPI_REST(float));
int pddp_mppi_track_f64(const pddp_problem* problem, const double* table,
                        const double* ref, int ref_len, int ref_t0,
                        PDDP_MPPI_REST(double));
int pddp_mppi_weighted_f32(const pddp_problem* problem, const float* table,
                           const float* weights, PDDP_MPPI_REST(float));
int pddp_mppi_weighted_f64(const pddp_problem* problem, const double* table,
                           const double* weights, PDDP_MPPI_REST(double));
int pddp_mppi_track_weighted_f32(const pddp_problem* problem,
                                 const float* table, const float* ref,
                                 int ref_len, int ref_t0, const float* weights,
                                 PDDP_MPPI_REST(float));
int pddp_mppi_track_weighted_f64(const pddp_problem* problem,
                                 const double* table, const double* ref,
                                 int ref_len, int ref_t0,
                                 const double* weights,
                                 PDDP_MPPI_REST(double));
#define PDDP_CEM_REST(T)                                                       \
  int B, int N, int S, int K, const T* z0, const T* U, const T* u_min,         \
      const T* u_max, const T* sigma, const T* std_min, double smooth,         \
      double mix, uint64_t seed, uint64_t sample_offset,                       \
      const uint8_t* active, T* Jc, int32_t* rank, int32_t* best, T* J_best,   \
      int32_t* n_elite, T* J_m, T* Z_out, T* U_out, T* S_out, void* stream
int pddp_cem_track_f32(const pddp_problem* problem, const float* table,
                       const float* ref, int ref_len, int ref_t0,
                       PDDP_CEM_REST(float));
int pddp_cem_track_f64(const pddp_problem* problem, const double* table,
                       const double* ref, int ref_len, int ref_t0,
                       PDDP_CEM_REST(double));
int pddp_cem_weighted_f32(const pddp_problem* problem, const float* table,
                          const float* weights, PDDP_CEM_REST(float));
int pddp_cem_weighted_f64(const pddp_problem* problem, const double* table,
                          const double* weights, PDDP_CEM_REST(double));
int pddp_cem_track_weighted_f32(const pddp_problem* problem,
                                const float* table, const float* ref,
                                int ref_len, int ref_t0, const float* weights,
                                PDDP_CEM_REST(float));
int pddp_cem_track_weighted_f64(const pddp_problem* problem,
                                const double* table, const double* ref,
                                int ref_len, int ref_t0, const double* weights,
                                PDDP_CEM_REST(double));
#undef PDDP_CEM_REST
#undef PDDP_MPPI_REST
#undef PDDP_SHOOT_REST
int pddp_mppi_trial_goals_f32(
    const pddp_problem* problem, const float* table, const float* plant,
    const float* ref, int ref_len, int ref_t0, const float* weights, int B,
    int N, int S, int K, int TT, int t0, int count, float* z0, float* U,
    float* Z, float* U_work, const float* u_min, const float* u_max,
    const float* a_std, const float* lam, double smooth, uint64_t seed,
    uint64_t cand_offset, uint64_t iter_stride, const float* disturbance,
    const float* w_std, const float* v_std, uint64_t rollout_offset,
    int step_offset, float* x_true, const uint8_t* active, float* Jc,
    int log_costs, float* Xlog, float* Ulog, float* Jcl, float* Ylog,
    float* J0_log, float* Jw_log, float* ess_log, float* plan_log,
    void* stream);
int pddp_mppi_trial_goals_f64(
    const pddp_problem* problem, const double* table, const double* plant,
    const double* ref, int ref_len, int ref_t0, const double* weights, int B,
    int N, int S, int K, int TT, int t0, int count, double* z0, double* U,
    double* Z, double* U_work, const double* u_min, const double* u_max,
    const double* a_std, const double* lam, double smooth, uint64_t seed,
    uint64_t cand_offset, uint64_t iter_stride, const double* disturbance,
    const double* w_std, const double* v_std, uint64_t rollout_offset,
    int step_offset, double* x_true, const uint8_t* active, double* Jc,
    int log_costs, double* Xlog, double* Ulog, double* Jcl, double* Ylog,
    double* J0_log, double* Jw_log, double* ess_log, double* plan_log,
    void* stream);

/* ---- pddp.py:209-245 _apply_controller(mpc=True) with ilqr.py:355-362
 * forward(mpc=True) as the controller, batched and with the sample models as
 * the plant: the hand-over between two control steps of a receding-horizon
 * trial, one launch per control step AFTER that step's rounds
 * (csrc/mpc_advance.hip; one lane per trajectory).  Trajectory b at control
 * step t of T, in this order:
 *
 *   state_log[b][t] = state[b];  live_log[b][t] = active[b] != 0
 *         (as the rounds left them; live: the rounds ran out before the
 *          trajectory was accepted, converged or exhausted its regularisation)
 *   x = z0[b];  u = clamp(U[b][0])   (bounds NULL together: no clamp)
 *   Xlog[b][t] = x;  Ulog[b][t] = u;  Jcl[b] = (t == 0 ? 0 : Jcl[b]) + l(x, u)
 *   x' = plant_b(x, u) + disturbance[b][t]       (disturbance == NULL: + 0)
 *   t == T-1:  Xlog[b][T] = x';  Jcl[b] += l_f(x')
 *   U[b][i] = U[b][i+1], i < N-1; the last row stays (repeated): a plain copy
 *         of the unclamped words;  z0[b] = x'
 *   Z[b][0..N] = the rollout of the shifted U from x' with clamped actions
 *         under the CONTROLLER's model: what pddp_nominal_rollout[_batch]_*
 *         computes for (z0, U) as this launch leaves them
 *   mu = 0, delta = 2, state = UNDEFINED, iter = 1, active = 1, fresh = 1
 *         (the regularisation reset, ilqr.py:364-367, and the start of a fit
 *          loop with n_iterations = 1)
 *
 * table [B][PDDP_BATCH_ROW], nullable: the controller's model of trajectory b
 * is row b (the layout above), else `problem`'s own params and goals.  plant
 * [B][PDDP_BATCH_ROW], nullable: the plant's dynamics AND the cost of the
 * trial are that row's; NULL: the plant is the controller's model.  Q, Q_term,
 * R, the model and the encoding are `problem`'s.  z0 [B][n], U [B][N][m],
 * Z [B][N+1][n], the controller state arrays ([B], as pddp_accept_*) in / out.
 * disturbance [B][T][n].  Xlog [B][T+1][n], Ulog [B][T][m], Jcl [B],
 * state_log [B][T] int32, live_log [B][T] uint8: the trial, written at t (and
 * T); Jcl is summed in t order by the trajectory's lane, no atomics.
 * mask [B] nullable: trajectories with mask[b] == 0 are left entirely
 * untouched, nothing of theirs is read or written.  n_live
 * [PDDP_LIVE_SHARDS], nullable: zeroed by the launch whatever the mask says
 * (it belongs to no trajectory).
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY, any
 * B, N, T >= 1.  PDDP_E_BADARG: a null required pointer (everything but table,
 * plant, the bounds, disturbance, mask and n_live), a non-positive size, t
 * outside [0, T); PDDP_E_UNSUPPORTED: any other encoding or model; both before
 * any HIP call. */
int pddp_mpc_advance_f32(const pddp_problem* problem, const float* table,
                         int B, int N, int T, int t, float* z0, float* U,
                         float* Z, const float* u_min, const float* u_max,
                         const float* plant, const float* disturbance,
                         const uint8_t* mask, float* Xlog, float* Ulog,
                         float* Jcl, int32_t* state_log, uint8_t* live_log,
                         double* mu, double* delta, int32_t* state,
                         int32_t* iter, uint8_t* active, uint8_t* fresh,
                         int32_t* n_live, void* stream);
int pddp_mpc_advance_f64(const pddp_problem* problem, const double* table,
                         int B, int N, int T, int t, double* z0, double* U,
                         double* Z, const double* u_min, const double* u_max,
                         const double* plant, const double* disturbance,
                         const uint8_t* mask, double* Xlog, double* Ulog,
                         double* Jcl, int32_t* state_log, uint8_t* live_log,
                         double* mu, double* delta, int32_t* state,
                         int32_t* iter, uint8_t* active, uint8_t* fresh,
                         int32_t* n_live, void* stream);

/* ---- reference tracking: a goal PER TIME STEP (csrc/goal_kernels.hpp) -----
 * `ref` [B][ref_len][PDDP_REF_ROW], device memory of the run's dtype: row k of
 * trajectory b holds the goals of step k of its reference,
 *   [PDDP_REF_X_GOAL .. +7]  x_goal  (augmented coordinates, PDDP_MAX_AUG)
 *   [PDDP_REF_U_GOAL .. +3]  u_goal  (PDDP_MAX_ACTION)
 * (the widths of the table's fields above).  Entries beyond the model's sizes
 * are never read.  An f32 row is 48 bytes, an f64 row 96: rows are 16-byte
 * aligned when the base is.  Horizon index i = 0 .. N (N: the terminal step)
 * of trajectory b reads row min(ref_t0 + i, ref_len - 1): the last row is
 * held, a reference may be shorter than a window or a trial.  The terminal
 * step reads its row's x_goal only.
 * Q, Q_term, R, the model, the encoding and the action bounds are `problem`'s.
 * table [B][PDDP_BATCH_ROW], nullable: the model parameters of trajectory b
 * are row b's (its goal fields are not read), else `problem`'s.
 *
 * pddp_derivs_track_* / pddp_line_search_track_*: every other argument and
 * every result as pddp_derivs_batch_* / pddp_line_search_batch_* (one
 * workgroup per trajectory and one lane per time step; one lane per
 * (trajectory, step size), any A).
 * pddp_mpc_advance_track_* (csrc/mpc_advance.hip): pddp_mpc_advance_* with
 *   Jcl[b] += l(x, u) under row ref_t0;  t == T-1: += l_f(x') under row
 *   ref_t0 + 1 (both clamped to the last row)
 * plant [B][PDDP_BATCH_ROW], nullable: the plant's PARAMETERS only; its goal
 * fields are not read.  Shift, rollout and re-arm read no goal.
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: ref == NULL, ref_len < 1, ref_t0 < 0 and everything the
 * siblings answer it for; PDDP_E_UNSUPPORTED: any other encoding or model;
 * both before any HIP call. */
#define PDDP_REF_ROW 12
#define PDDP_REF_X_GOAL 0
#define PDDP_REF_U_GOAL 8
int pddp_derivs_track_f32(const pddp_problem* problem, const float* table,
                          const float* ref, int ref_len, int ref_t0, int B,
                          int N, const float* Z, const float* U,
                          const float* u_min, const float* u_max,
                          const uint8_t* mask, float* rec, float* L, float* J,
                          int32_t* state, void* stream);
int pddp_derivs_track_f64(const pddp_problem* problem, const double* table,
                          const double* ref, int ref_len, int ref_t0, int B,
                          int N, const double* Z, const double* U,
                          const double* u_min, const double* u_max,
                          const uint8_t* mask, double* rec, double* L,
                          double* J, int32_t* state, void* stream);
int pddp_line_search_track_f32(const pddp_problem* problem, const float* table,
                               const float* ref, int ref_len, int ref_t0,
                               int B, int N, int A, const float* Z,
                               const float* U, const float* gains,
                               const float* alphas, const float* u_min,
                               const float* u_max, const uint8_t* active,
                               const int32_t* bwd_status, float* Zc, float* Uc,
                               float* Jc, void* stream);
int pddp_line_search_track_f64(const pddp_problem* problem,
                               const double* table, const double* ref,
                               int ref_len, int ref_t0, int B, int N, int A,
                               const double* Z, const double* U,
                               const double* gains, const double* alphas,
                               const double* u_min, const double* u_max,
                               const uint8_t* active,
                               const int32_t* bwd_status, double* Zc,
                               double* Uc, double* Jc, void* stream);
int pddp_mpc_advance_track_f32(const pddp_problem* problem, const float* table,
                               const float* ref, int ref_len, int ref_t0,
                               int B, int N, int T, int t, float* z0, float* U,
                               float* Z, const float* u_min,
                               const float* u_max, const float* plant,
                               const float* disturbance, const uint8_t* mask,
                               float* Xlog, float* Ulog, float* Jcl,
                               int32_t* state_log, uint8_t* live_log,
                               double* mu, double* delta, int32_t* state,
                               int32_t* iter, uint8_t* active, uint8_t* fresh,
                               int32_t* n_live, void* stream);
int pddp_mpc_advance_track_f64(const pddp_problem* problem,
                               const double* table, const double* ref,
                               int ref_len, int ref_t0, int B, int N, int T,
                               int t, double* z0, double* U, double* Z,
                               const double* u_min, const double* u_max,
                               const double* plant, const double* disturbance,
                               const uint8_t* mask, double* Xlog, double* Ulog,
                               double* Jcl, int32_t* state_log,
                               uint8_t* live_log, double* mu, double* delta,
                               int32_t* state, int32_t* iter, uint8_t* active,
                               uint8_t* fresh, int32_t* n_live, void* stream);

/* ---- pddp_mpc_advance[_track]_* under process and measurement noise drawn on
 * the device (csrc/mpc_advance_noise.hip; the reference has no counterpart).
 * Trial b is rollout r = rollout_offset + b of the generator stated for
 * pddp_closed_loop_noisy_* above (its counter layout with S = 1), control step
 * t its step step_offset + t, stream 0 the process noise w and stream 1 the
 * measurement noise v: a trial sees the normals pddp_closed_loop_draws_* writes
 * for (seed, sample_offset = rollout_offset, S = 1), and a fixed policy run by
 * pddp_closed_loop_noisy_* with that seed and offset sees the same ones.
 *
 * With v_std the plant's state is x_true [B][n], in / out; z0 and Z[b][0] hold
 * what the controller sees.  Trajectory b at control step t of T, in this
 * order (everything not named is pddp_mpc_advance_*'s):
 *
 *   x = x_true[b]                              (v_std == NULL: x = z0[b])
 *   u = clamp(U[b][0]);  Xlog[b][t] = x;  Ulog[b][t] = u;  Jcl[b] += l(x, u)
 *         (the TRUE state, under the plant row's goals, or under reference row
 *          ref_t0 where ref != NULL)
 *   x' = plant_b(x, u) + disturbance[b][t] + w_std (.) w(r, step_offset + t)
 *   t == T-1:  Xlog[b][T] = x';  Jcl[b] += l_f(x')
 *   x_true[b] = x'                             (v_std == NULL: not written)
 *   y' = x' + v_std (.) v(r, step_offset + t + 1);  z0[b] = y';
 *         Ylog[b][t+1] = y' where Ylog != NULL    (v_std == NULL: y' = x',
 *                                                  Ylog is not written)
 *   shift U;  Z[b][0..N] = the rollout of the shifted U from y' under the
 *         CONTROLLER's model;  re-arm the controller
 *
 * Each noisy sum is one fused multiply-add per component, a + std * z.
 * w_std, v_std [n], the launch's, of the run's type, not both NULL (that is
 * pddp_mpc_advance[_track]_*'s launch); a launch without one of them carries
 * none of its instructions.  Ylog [B][T+1][n], nullable; row 0 is the caller's.
 * ref == NULL: no tracking, ref_len / ref_t0 are not read, table and plant
 * rows supply goals as in pddp_mpc_advance_*; ref != NULL: the goals of
 * pddp_mpc_advance_track_*.
 *
 * pddp_mpc_observe_*: y[b] = x[b] + v_std (.) v(rollout_offset + b, step), one
 * lane per trajectory, through the device function of the hand-over, so that a
 * trial's first observation obeys the law of every later one (bit for bit what
 * the hand-over writes for the same x, r and step).  x, y [B][n] (they may be
 * the same array), mask [B] nullable: trajectories with 0 are not touched.
 *
 * PDDP_E_BADARG: w_std == v_std == NULL; v_std with x_true == NULL; ref != NULL
 * with ref_len < 1 or ref_t0 < 0; step_offset < 0 (or step_offset + T beyond an
 * int); everything pddp_mpc_advance_* answers it for; observe: a null x, v_std
 * or y, B or n < 1, n > PDDP_MAX_STATE, step < 0.  PDDP_E_UNSUPPORTED: any
 * encoding but PDDP_ENC_IGNORE_UNCERTAINTY.  All before any HIP call. */
int pddp_mpc_advance_noisy_f32(
    const pddp_problem* problem, const float* table, const float* ref,
    int ref_len, int ref_t0, int B, int N, int T, int t, float* z0, float* U,
    float* Z, const float* u_min, const float* u_max, const float* plant,
    const float* disturbance, const float* w_std, const float* v_std,
    uint64_t seed, uint64_t rollout_offset, int step_offset, float* x_true,
    float* Ylog, const uint8_t* mask, float* Xlog, float* Ulog, float* Jcl,
    int32_t* state_log, uint8_t* live_log, double* mu, double* delta,
    int32_t* state, int32_t* iter, uint8_t* active, uint8_t* fresh,
    int32_t* n_live, void* stream);
int pddp_mpc_advance_noisy_f64(
    const pddp_problem* problem, const double* table, const double* ref,
    int ref_len, int ref_t0, int B, int N, int T, int t, double* z0, double* U,
    double* Z, const double* u_min, const double* u_max, const double* plant,
    const double* disturbance, const double* w_std, const double* v_std,
    uint64_t seed, uint64_t rollout_offset, int step_offset, double* x_true,
    double* Ylog, const uint8_t* mask, double* Xlog, double* Ulog, double* Jcl,
    int32_t* state_log, uint8_t* live_log, double* mu, double* delta,
    int32_t* state, int32_t* iter, uint8_t* active, uint8_t* fresh,
    int32_t* n_live, void* stream);
int pddp_mpc_observe_f32(int B, int n, const float* x, const float* v_std,
                         uint64_t seed, uint64_t rollout_offset, int step,
                         const uint8_t* mask, float* y, void* stream);
int pddp_mpc_observe_f64(int B, int n, const double* x, const double* v_std,
                         uint64_t seed, uint64_t rollout_offset, int step,
                         const uint8_t* mask, double* y, void* stream);

/* ---- per-trajectory cost weights (csrc/goal_kernels.hpp) --------------------
 * `weights` [B][PDDP_WEIGHT_ROW], device memory of the run's dtype: row b holds
 *   [PDDP_WEIGHT_Q      .. +7]  the diagonal of Q      of trajectory b
 *                               (augmented coordinates, PDDP_MAX_AUG)
 *   [PDDP_WEIGHT_Q_TERM .. +7]  the diagonal of Q_term
 *   [PDDP_WEIGHT_R      .. +3]  the diagonal of R      (PDDP_MAX_ACTION)
 * Trajectory b's cost matrices are `problem`'s with their diagonals REPLACED
 * by row b; the off-diagonal entries stay `problem`'s.  Entries of a row
 * beyond the model's aug_size / action_size are never read.  An f32 row is 80
 * bytes, an f64 row 160: rows are 16-byte aligned when the base is.  Nothing
 * checks that the matrices of a row are positive (semi-)definite:
 * ILQRSolver.set_batch_weights does, on the host.
 * table [B][PDDP_BATCH_ROW], nullable: the model parameters AND goals of
 * trajectory b are row b's (as pddp_*_batch_*), else `problem`'s.
 *
 * pddp_derivs_weighted_* / pddp_line_search_weighted_*: every other argument
 * and every result as pddp_derivs_batch_* / pddp_line_search_batch_* (one
 * workgroup per trajectory and one lane per time step; one lane per
 * (trajectory, step size), any A).  The nominal rollout reads no cost:
 * pddp_nominal_rollout[_batch]_* serves.
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: weights == NULL and everything the siblings answer it for
 * (B * A > 0x7fffffff included); PDDP_E_UNSUPPORTED: any other encoding or
 * model; both before any HIP call. */
#define PDDP_WEIGHT_ROW 20
#define PDDP_WEIGHT_Q 0
#define PDDP_WEIGHT_Q_TERM 8
#define PDDP_WEIGHT_R 16
int pddp_derivs_weighted_f32(const pddp_problem* problem, const float* table,
                             const float* weights, int B, int N,
                             const float* Z, const float* U,
                             const float* u_min, const float* u_max,
                             const uint8_t* mask, float* rec, float* L,
                             float* J, int32_t* state, void* stream);
int pddp_derivs_weighted_f64(const pddp_problem* problem, const double* table,
                             const double* weights, int B, int N,
                             const double* Z, const double* U,
                             const double* u_min, const double* u_max,
                             const uint8_t* mask, double* rec, double* L,
                             double* J, int32_t* state, void* stream);
int pddp_line_search_weighted_f32(const pddp_problem* problem,
                                  const float* table, const float* weights,
                                  int B, int N, int A, const float* Z,
                                  const float* U, const float* gains,
                                  const float* alphas, const float* u_min,
                                  const float* u_max, const uint8_t* active,
                                  const int32_t* bwd_status, float* Zc,
                                  float* Uc, float* Jc, void* stream);
int pddp_line_search_weighted_f64(const pddp_problem* problem,
                                  const double* table, const double* weights,
                                  int B, int N, int A, const double* Z,
                                  const double* U, const double* gains,
                                  const double* alphas, const double* u_min,
                                  const double* u_max, const uint8_t* active,
                                  const int32_t* bwd_status, double* Zc,
                                  double* Uc, double* Jc, void* stream);

/* ---- a reference tracked under per-trajectory cost weights
 * (csrc/goal_kernels.hpp): pddp_derivs_track_* / pddp_line_search_track_*
 * with the diagonals of Q, Q_term and R of trajectory b REPLACED by row b of
 * `weights`.  `ref`, ref_len, ref_t0 in the reference's layout and law above
 * (row min(ref_t0 + i, ref_len - 1), the last row held), `weights`
 * [B][PDDP_WEIGHT_ROW] in the weights' layout above.  table
 * [B][PDDP_BATCH_ROW], nullable: the model parameters of trajectory b are row
 * b's (its goal fields are not read), else `problem`'s.  Every other argument
 * and every result as the _track_ entry points.  The hand-over between two MPC
 * control steps and the closed-loop rollouts report under the shared matrices:
 * pddp_mpc_advance_track_* / pddp_mpc_advance_noisy_* / pddp_closed_loop_track_*
 * serve unchanged.
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY.
 * PDDP_E_BADARG: weights == NULL, ref == NULL, ref_len < 1, ref_t0 < 0 and
 * everything the siblings answer it for (B * A > 0x7fffffff included);
 * PDDP_E_UNSUPPORTED: any other encoding or model; both before any HIP
 * call. */
int pddp_derivs_track_weighted_f32(const pddp_problem* problem,
                                   const float* table, const float* ref,
                                   int ref_len, int ref_t0,
                                   const float* weights, int B, int N,
                                   const float* Z, const float* U,
                                   const float* u_min, const float* u_max,
                                   const uint8_t* mask, float* rec, float* L,
                                   float* J, int32_t* state, void* stream);
int pddp_derivs_track_weighted_f64(const pddp_problem* problem,
                                   const double* table, const double* ref,
                                   int ref_len, int ref_t0,
                                   const double* weights, int B, int N,
                                   const double* Z, const double* U,
                                   const double* u_min, const double* u_max,
                                   const uint8_t* mask, double* rec, double* L,
                                   double* J, int32_t* state, void* stream);
int pddp_line_search_track_weighted_f32(
    const pddp_problem* problem, const float* table, const float* ref,
    int ref_len, int ref_t0, const float* weights, int B, int N, int A,
    const float* Z, const float* U, const float* gains, const float* alphas,
    const float* u_min, const float* u_max, const uint8_t* active,
    const int32_t* bwd_status, float* Zc, float* Uc, float* Jc, void* stream);
int pddp_line_search_track_weighted_f64(
    const pddp_problem* problem, const double* table, const double* ref,
    int ref_len, int ref_t0, const double* weights, int B, int N, int A,
    const double* Z, const double* U, const double* gains,
    const double* alphas, const double* u_min, const double* u_max,
    const uint8_t* active, const int32_t* bwd_status, double* Zc, double* Uc,
    double* Jc, void* stream);

/* ---- pddp_closed_loop_* / pddp_closed_loop_noisy_* ALONG A REFERENCE
 * (csrc/closed_loop.hip): the same S rollouts per trajectory, costed
 * under a goal per time step.  Rollout (b, s) takes
 *
 *   J += l(x_t, u_t)  under row min(ref_t0 + t, ref_len - 1) of trajectory b,
 *                     t = 0 .. N-1
 *   J += l_f(x_N)     under row min(ref_t0 + N, ref_len - 1), x_goal only
 *
 * `ref` [B][ref_len][PDDP_REF_ROW] in the layout above; the S rollouts of a
 * trajectory share its reference.  plant [B][S][PDDP_BATCH_ROW], nullable: the
 * plant's PARAMETERS only; its goal fields are not read.  w_std, v_std, seed,
 * sample_offset: pddp_closed_loop_noisy_*'s law and draws - rollout (b, s) at
 * step t sees the normals pddp_closed_loop_draws_* writes for it;
 * w_std == v_std == NULL is the noise-free launch, valid here.  Every other
 * argument, the feedback law, the clamp, the output layout, the statistics and
 * their order are pddp_closed_loop_*'s: none of them reads a goal.
 * Domain: the four sample models under PDDP_ENC_IGNORE_UNCERTAINTY, any
 * B, N, S >= 1.  PDDP_E_BADARG: what pddp_closed_loop_* refuses; ref == NULL,
 * ref_len < 1, ref_t0 < 0; PDDP_E_UNSUPPORTED: any other encoding; both before
 * any HIP call. */
int pddp_closed_loop_track_f32(const pddp_problem* problem, const float* ref,
                               int ref_len, int ref_t0, int B, int N, int S,
                               const float* Z, const float* U,
                               const float* gains, const float* z0s,
                               const float* plant, const float* u_min,
                               const float* u_max, const float* w_std,
                               const float* v_std, uint64_t seed,
                               uint64_t sample_offset, const uint8_t* active,
                               float* Xc, float* Uc, float* Jc, float* stats,
                               void* stream);
int pddp_closed_loop_track_f64(const pddp_problem* problem, const double* ref,
                               int ref_len, int ref_t0, int B, int N, int S,
                               const double* Z, const double* U,
                               const double* gains, const double* z0s,
                               const double* plant, const double* u_min,
                               const double* u_max, const double* w_std,
                               const double* v_std, uint64_t seed,
                               uint64_t sample_offset, const uint8_t* active,
                               double* Xc, double* Uc, double* Jc,
                               double* stats, void* stream);

/* ---- ilqr.py:102-181 _step() accept / reject, :364-390 mu schedule and the
 * fit() loop bookkeeping (:298-314), per trajectory, device resident -------- */
/* Controller state arrays (all [B]):
 *   J_opt (T), mu, delta (double, the reference's python floats), state
 *   (iLQRState), iter (number of step() calls started, ilqr.py:298),
 *   active (attempted this round), fresh (needs new derivatives next round).
 * For each trajectory with active[b] != 0:
 *   bwd_status != 0 -> _increase_reg, NOT_PD / MAX_REG          (:140-145)
 *   else amin = argmin Jc[b], accept iff J_new < J_opt           (:161-166)
 *     accept: Z, U <- candidate amin; gains_acc <- gains (self._K);
 *             _decrease_reg; CONVERGED iff |dJ|/J_opt < tol      (:167-176)
 *     reject: _increase_reg, REJECTED / MAX_REG                  (:178-181)
 * then the masks of the NEXT round: retry states keep active=1, fresh=0;
 * ACCEPTED starts the next step() (iter+1, fresh=1) unless iter == n_iterations;
 * CONVERGED / MAX_REG leave the loop (:313).  n_live (device
 * int32[PDDP_LIVE_SHARDS], nullable) accumulates, sharded by b mod
 * PDDP_LIVE_SHARDS, the number of trajectories still active after this round
 * (sum the shards; one word would serialise 4096 atomics). */
#define PDDP_LIVE_SHARDS 256
int pddp_accept_f32(int B, int N, int n, int m, int A, const float* Zc,
                    const float* Uc, const float* Jc, const float* gains,
                    const int32_t* bwd_status, double tol, double max_reg,
                    int n_iterations, float* Z, float* U, float* gains_acc,
                    float* J_opt, double* mu, double* delta, int32_t* state,
                    int32_t* iter, uint8_t* active, uint8_t* fresh,
                    int32_t* n_live, void* stream);
int pddp_accept_f64(int B, int N, int n, int m, int A, const double* Zc,
                    const double* Uc, const double* Jc, const double* gains,
                    const int32_t* bwd_status, double tol, double max_reg,
                    int n_iterations, double* Z, double* U, double* gains_acc,
                    double* J_opt, double* mu, double* delta, int32_t* state,
                    int32_t* iter, uint8_t* active, uint8_t* fresh,
                    int32_t* n_live, void* stream);

/* ---- multi-GPU exchange: the record a rank contributes to the
 * all-gather of the best rollout, out[2 + nz + nu] = {J_best, offset + index,
 * Z[index][nz], U[index][nu]}, index = the first trajectory of least finite
 * J (non-finite costs count as +inf; all non-finite: index 0, J_best = inf).
 * J [B], Z [B][nz], U [B][nu]; one launch, no host synchronisation. */
int pddp_pack_best_f32(int B, int nz, int nu, const float* J, const float* Z,
                       const float* U, long long offset, float* out,
                       void* stream);
int pddp_pack_best_f64(int B, int nz, int nu, const double* J, const double* Z,
                       const double* U, long long offset, double* out,
                       void* stream);

/* ---- the backward sweep of a sample problem FROM ITS NOMINAL TRAJECTORY: the
 * derivative records (ilqr.py:464-473: F_z, F_u, L_z ... of every step) are
 * evaluated inside the sweep's workgroups, in LDS, and never written - the
 * 79 MB per launch that pddp_derivs_* / pddp_search_accept_* write and
 * pddp_riccati_backward_* reads at B = 4096, N = 100 stay on the chip.
 * Results as pddp_derivs_* followed by pddp_riccati_backward_* (auto kernel):
 * gains [B][N][5], status [B]; L [B][N+1] the stage / terminal costs of the
 * nominal (rows of ACTIVE trajectories);
 * for trajectories with fresh[b] != 0 (all, when fresh is NULL)
 * J_opt[b] = sum_t L[b][t] in t order (ilqr.py:289 L.sum()) and fresh[b] is
 * cleared.  Z [B][N+1][n], U [B][N] un-clamped nominal actions.  Under
 * IGNORE_UNCERTAINTY:
 *   cartpole          f32 and f64, both branches, bounded (u_min, u_max
 *                     non-NULL) or not (both NULL) (csrc/riccati_n4_elem.hpp;
 *                     every combination but bounded PDDP_BRANCH_EIG in the
 *                     kernels of csrc/cartpole_branches.hip.  Gains of
 *                     trajectories with active[b] == 0 are left alone there;
 *                     the bounded PDDP_BRANCH_EIG f32 kernels may overwrite
 *                     them);
 *   pendulum, double cartpole   f32 and f64, both branches, bounded or not
 *                     (csrc/riccati_mfma16_nominal.hpp: the 16 x 16
 *                     matrix-core sweep, its records generated block by block
 *                     in the wavefront);
 * PDDP_E_UNSUPPORTED otherwise (make the two calls then).  `L` of
 * pddp_search_accept_* may be NULL with this sweep. */
int pddp_sweep_nominal_f32(const pddp_problem* problem, int B, int N,
                           const float* Z, const float* U, const float* u_min,
                           const float* u_max, const double* reg, int branch,
                           const uint8_t* active, uint8_t* fresh, float* gains,
                           int32_t* status, float* L, float* J_opt,
                           void* stream);
int pddp_sweep_nominal_f64(const pddp_problem* problem, int B, int N,
                           const double* Z, const double* U, const double* u_min,
                           const double* u_max, const double* reg, int branch,
                           const uint8_t* active, uint8_t* fresh, double* gains,
                           int32_t* status, double* L, double* J_opt,
                           void* stream);

/* How pddp_sweep_nominal_f32 (csrc/riccati_n4_elem.hpp) generates its records:
 * 0 = auto (on wavefronts of their own while one workgroup per CU holds the
 * batch, inline beyond), 3 = inline, 4 = on wavefronts of their own; results
 * are bit-identical.  Other values are ignored.  Process-wide (an A/B and
 * test knob); -1 only queries.  Returns the previous choice. */
int pddp_sweep_nominal_kernel(int which);

/* What a cartpole launch of pddp_sweep_nominal_f32 / _f64 (rounds == 0) or of
 * pddp_round_nominal_f32 (rounds != 0) looks like for these arguments: the
 * plan every such launch is made from (csrc/riccati_n4_elem.hpp,
 * n4_nominal_plan).  element_size 4 or 8; has_u_min / has_u_max: whether that
 * bound is given; kernel_choice: as pddp_sweep_nominal_kernel (the sweep's;
 * the round ignores it); A is looked at for the round only.  Returns what the
 * launch returns before its first HIP call - 0, PDDP_E_BADARG, or
 * PDDP_E_UNSUPPORTED for everything the cartpole's kernels do not serve (other
 * models and encodings among it) - and with 0 writes plan[PDDP_N4_PLAN_*].
 * Host function: no HIP call. */
enum {
  PDDP_N4_PLAN_BRANCH = 0,  /* 0 eig-clamp bounded, 1 eig-clamp unbounded,
                             * 2 V_zz-regularised unbounded, 3 ... bounded */
  PDDP_N4_PLAN_SPARSE = 1,  /* stage cost on {x, sin, cos} only (else full) */
  PDDP_N4_PLAN_OVERLAP = 2, /* record generator on wavefronts of its own */
  PDDP_N4_PLAN_MULTI = 3,   /* round: several rounds per launch */
  PDDP_N4_PLAN_CARRY = 4,   /* round: the nominal's last rows stay in LDS */
  PDDP_N4_PLAN_GRID = 5,    /* workgroups */
  PDDP_N4_PLAN_THREADS = 6, /* threads per workgroup */
  PDDP_N4_PLAN_LDS = 7,     /* dynamic LDS, bytes */
  PDDP_N4_PLAN_FIELDS = 8
};
int pddp_n4_nominal_plan(const pddp_problem* problem, int element_size, int B,
                         int N, int A, int has_u_min, int has_u_max,
                         int branch, int rounds, int kernel_choice,
                         int32_t* plan);

/* ---- one launch for the rest of a round: the line search, the accept step
 * and the derivative records of the trajectories whose nominal changed and
 * whose fit goes on.  Same arguments and semantics as the three calls; Z, U, active are
 * in/out; `fresh` is cleared for the trajectories whose records were written
 * here.  Sample problems with at most 16 step sizes; returns
 * PDDP_E_UNSUPPORTED otherwise (make the three calls then).  L == NULL: no
 * records are written and `fresh` stays set - the caller's next sweep is
 * pddp_sweep_nominal_*, which needs none; `rec`, when not NULL, is then
 * scratch of at least B (N+1) n scalars: the states of every trajectory's
 * full-step candidate go there, rows next to one another, INSTEAD of
 * Zc[b][.][0][.] (the usual winner: its copy into the nominal reads whole
 * sectors there, 16 bytes out of every A n 4-byte step in Zc).  In that form
 * (L == NULL, rec given, N + 1 within the tail's short form: 128 steps for the
 * paired launch) the candidates' ACTIONS `Uc` are not written either: the
 * winner's are its control law at its states, re-evaluated bit for bit. */
/* Candidates of pddp_search_accept_* in its form without records (L == NULL,
 * rec given as scratch): 0 = auto - kept while B A (N (n + m) + n) scalars fit
 * the Infinity Cache next to the round's other traffic (200 MB), dropped
 * beyond; 1 = always kept; 2 = always dropped.  Dropped: Zc / Uc are scratch
 * (contents unspecified after the call), only the costs Jc are formed; the
 * full step's states go to `rec` as above, a winner other than the full step
 * is rolled out a second time.  Every other output is the same to rounding.
 * Process-wide (an A/B and test knob); -1 only queries.  Returns the previous
 * mode. */
int pddp_search_candidates(int mode);
/* Which form of pddp_search_accept_* runs (f32, n <= 4): 0 = auto - the paired
 * form (a helper wavefront per rollout wavefront, the nominal's 4 KB per
 * trajectory in LDS, two workgroups per CU), from 8193 to 49152 trajectories
 * the dense form (gains only in LDS, no helpers, four workgroups per CU); 1 =
 * always the paired form; 2 = the dense form wherever it is built.  Results are
 * bit-identical.  Process-wide (an A/B and test knob); -1 only queries.
 * Returns the previous mode. */
int pddp_search_form(int mode);

int pddp_search_accept_f32(const pddp_problem* problem, int B, int N, int A,
                           float* Z, float* U, const float* gains,
                           const float* alphas, const float* u_min,
                           const float* u_max, uint8_t* active,
                           const int32_t* bwd_status, float* Zc, float* Uc,
                           float* Jc, double tol, double max_reg,
                           int n_iterations, float* gains_acc, float* J_opt,
                           double* mu, double* delta, int32_t* state,
                           int32_t* iter, uint8_t* fresh, int32_t* n_live,
                           float* rec, float* L, void* stream);
int pddp_search_accept_f64(const pddp_problem* problem, int B, int N, int A,
                           double* Z, double* U, const double* gains,
                           const double* alphas, const double* u_min,
                           const double* u_max, uint8_t* active,
                           const int32_t* bwd_status, double* Zc, double* Uc,
                           double* Jc, double tol, double max_reg,
                           int n_iterations, double* gains_acc, double* J_opt,
                           double* mu, double* delta, int32_t* state,
                           int32_t* iter, uint8_t* fresh, int32_t* n_live,
                           double* rec, double* L, void* stream);

/* ---- a whole round in ONE launch: pddp_sweep_nominal_f32 followed by
 * pddp_search_accept_f32(L = NULL) for the same arguments, the workgroups
 * going straight from their sweep to their line search (csrc/round_n4.hip:
 * the gains, the nominal's rows, its cost and the sweep's status stay in LDS /
 * registers between the phases; no second launch, no second prologue).  Results
 * are the two calls' bit for bit (replaces ilqr.py:125-181 of one attempt:
 * backward, _control_law, _trajectory_cost, accept / reject, mu schedule).
 * (of the candidates, `Zc` and the costs `Jc` are written, `Uc` is NOT: the
 * winner's actions are its control law at its states, re-evaluated.)
 * `mu` is both the sweep's `reg` and the schedule's state; `scratch` as `rec`
 * of pddp_search_accept_* with L == NULL (B (N+1) n scalars).  Cartpole under
 * IGNORE_UNCERTAINTY, f32, both branches, bounded or not (u_min and u_max both
 * NULL: the search clamps to +-inf), A <= 16, N <= 127 (every branch: the LDS
 * image of a step is the same 52 words) and at most 4096 trajectories (one
 * workgroup of 16 per CU); PDDP_E_UNSUPPORTED otherwise (make the two calls
 * then).
 * `rounds` >= 1: that many attempts of every trajectory in the one launch,
 * exactly as `rounds` calls with rounds = 1 (trajectories are independent and
 * a workgroup owns its sixteen for the whole launch; one that has left the fit
 * - active[b] == 0 - is skipped, as by a later call).
 * `phase_ticks`, nullable: [ceil(B / 16)][2] counters to which every workgroup
 * ADDS the ticks of the chip's 100 MHz clock it spent in its sweeps and in its
 * searches (rocprofv3 sees one kernel; bench.py's roofline leg wants the
 * sweep's share). */
int pddp_round_nominal_f32(const pddp_problem* problem, int B, int N, int A,
                           float* Z, float* U, const float* alphas,
                           const float* u_min, const float* u_max, int branch,
                           uint8_t* active, uint8_t* fresh, float* gains,
                           int32_t* bwd_status, float* L, float* J_opt,
                           float* Zc, float* Uc, float* Jc, double tol,
                           double max_reg, int n_iterations, float* gains_acc,
                           double* mu, double* delta, int32_t* state,
                           int32_t* iter, int32_t* n_live, float* scratch,
                           int rounds, long long* phase_ticks, void* stream);

/* The variant entry with two HIP events (pddp_event_create) attached to the
 * sweep's own dispatch: elapsed(start, stop) is the kernel's duration as
 * rocprofv3 --kernel-trace reports it (bench.py's roofline leg). */
int pddp_riccati_backward_timed_f32(int B, int N, int n, int m,
                                    const float* rec, const float* u_min,
                                    const float* u_max, const double* reg,
                                    int branch, const uint8_t* active,
                                    float* gains, int32_t* status,
                                    void* stream, int variant, void* start,
                                    void* stop);
int pddp_riccati_backward_timed_f64(int B, int N, int n, int m,
                                    const double* rec, const double* u_min,
                                    const double* u_max, const double* reg,
                                    int branch, const uint8_t* active,
                                    double* gains, int32_t* status,
                                    void* stream, int variant, void* start,
                                    void* stop);

/* Arithmetic of the hidden-to-hidden contraction (layer 2) of pddp_bnn_mlp_* /
 * pddp_bnn_mlp_jvp_*: 0 = exact f32 on v_mfma_f32_32x32x2_f32 (default; bitwise
 * an fmaf chain), 3 = the bf16-split twin - weights and activations as three
 * bf16 parts, six v_mfma_f32_32x32x16_bf16 per product: f32 accuracy to
 * rounding (not bit-exact), 2.5 times fewer matrix cycles; H = 200 only, other
 * widths stay exact.  Process-wide; -1 only queries.  Returns the previous
 * mode (PDDP_MLP_BF16X3=1 in the environment makes 3 the initial one). */
int pddp_bnn_mlp_precision(int mode);

/* How the exact-f32 network kernel deals its layer-2 contraction out over a
 * workgroup's wavefronts at H = 200 (csrc/bnn_mlp.hip): 0 = every
 * block its own, 1 = round 2's balanced roles, 2 = round 5's (the last block's
 * 8 units on 16 x 16 x 4 tiles, three chunks handed over), -1 = the default:
 * 2 for inference, 1 for forward mode.  Another deal is another summation
 * order - the same numbers to rounding.  Process-wide; -2 only queries.
 * Returns the previous value (PDDP_MLP_BALANCED in the environment sets the
 * initial one). */
int pddp_bnn_mlp_deal(int deal);

/* ---- pddp/models/bnn/modules.py:774-864: the Bayesian network of the learned
 * dynamics model, fused (fc -> dropout mask -> ReLU, twice, fc_out), float:
 *   Y[r] = W3 relu(M2[p] * (W2 relu(M1[p] * (W1 X[r] + b1)) + b2)) + b3,
 * p = r % P the particle of row r (rows = states x particles, particle
 * fastest).  X [R][in_dim], W1 [H][in_dim], W2 [H][H], W3 [out_dim][H]
 * (torch.nn.Linear layout); M1, M2 [P][H] the dropout masks of the two hidden
 * layers as the framework holds them (all ones: no dropout), rows 16-byte
 * aligned (H a multiple of 4); Y [R][out_dim].  in_dim <= 15, out_dim <= 16, H in {64, 128,
 * 200}; PDDP_E_UNSUPPORTED otherwise (use the library GEMMs then). */
int pddp_bnn_mlp_f32(int R, int P, int in_dim, int H, int out_dim,
                     const float* X, const float* W1, const float* b1,
                     const float* M1, const float* W2, const float* b2,
                     const float* M2, const float* W3, const float* b3,
                     float* Y, void* stream);
/* The same on the first min(R, *live_rows) rows only (live_rows: one int32 on
 * the device, read by the kernel - no host synchronisation; nullable = R): the
 * launch is sized for R, workgroups without a tile leave at once.  The rows
 * beyond are neither read nor written.  For a line search whose live
 * candidates are packed to the front (pddp_bnn_step.slot): a round of retries
 * with three of 256 restarts alive runs the network on 3 / 256 of the rows. */
int pddp_bnn_mlp_rows_f32(int R, int P, int in_dim, int H, int out_dim,
                          const float* X, const float* W1, const float* b1,
                          const float* M1, const float* W2, const float* b2,
                          const float* M2, const float* W3, const float* b3,
                          float* Y, const int32_t* live_rows, void* stream);
/* The same network in double precision (modules.py runs in the dtype of its
 * inputs) on v_mfma_f64_16x16x4_f64, weights-stationary, four wavefronts per
 * CU (csrc/bnn_mlp_f64.hip); arguments as above with double data.  M1, M2:
 * 32-byte aligned (their rows then are: H is a multiple of 4). */
int pddp_bnn_mlp_f64(int R, int P, int in_dim, int H, int out_dim,
                     const double* X, const double* W1, const double* b1,
                     const double* M1, const double* W2, const double* b2,
                     const double* M2, const double* W3, const double* b3,
                     double* Y, void* stream);
int pddp_bnn_mlp_rows_f64(int R, int P, int in_dim, int H, int out_dim,
                          const double* X, const double* W1, const double* b1,
                          const double* M1, const double* W2, const double* b2,
                          const double* M2, const double* W3, const double* b3,
                          double* Y, const int32_t* live_rows, void* stream);

/* ---- one time step of the moment-matched line-search rollout under a BNN
 * dynamics model, everything but the network: ilqr.py:677-723 (_control_law),
 * :764-791 (_trajectory_cost), modules.py:287-386 (BNNDynamicsModel.forward:
 * particles in, particle moments out), encoding.py:99-141 (encode, DEFAULT) and
 * angular.py:47-84,161-248 (angle augmentation of the moments for the cost).
 * Called N + 1 times (t = 0 .. N) with the network (above) on F in between:
 *   t > 0:  Xp += net_out[:, :D] * dX_std + dX_mean   (the particle cloud is
 *           carried: `infer_noise_variables` re-whitens and re-colours with the
 *           same factor), z_t = encode(mean, covariance of Xp); t = 0: z_0 =
 *           Z[b][0], Xp as given (sampled by the caller, modules.py:312-330);
 *   Zc[b][t][a] = z_t;  t < N: Uc[b][t][a] = u_t = clamp(U + alpha k + K (z_t -
 *           Z)), J += l(z_t, u_t), F = network input rows of the particles;
 *   t = N:  J += l_f(z_N), Jc = J.
 * Candidate c = b * A + a; particle rows c * P + p.  DEFAULT encoding
 * (n = D + D (D + 1) / 2), D <= 8, at most two angular states, m <= 2,
 * P <= 128; the cost is a QR cost on the augmented moments. */
typedef struct pddp_bnn_step {
  int32_t B, A, P, D, m, N, t;
  int32_t n_ang, ang[2], n_non, non[8]; /* angular / non-angular state indices */
  int32_t in_dim, out_dim;              /* network: n_non + 2 n_ang + m, >= D */
  const float* Z;        /* [B][N+1][n] nominal */
  const float* U;        /* [B][N][m] */
  const float* gains;    /* [B][N][m + m n] */
  const float* alphas;   /* [A] */
  const float* u_min;    /* [m], nullable with u_max */
  const float* u_max;
  const uint8_t* active;       /* [B] nullable */
  const int32_t* bwd_status;   /* [B] nullable: non-zero -> skipped */
  const float* Q;        /* [na][na], na = n_non + 2 n_ang */
  const float* Q_term;
  const float* R;        /* [m][m] */
  const float* x_goal;   /* [na] */
  const float* u_goal;   /* [m] */
  const float* X_mean;   /* [in_dim] input normalisation (modules.py:181-186) */
  const float* X_std_inv;
  const float* dX_mean;  /* [D] output de-normalisation (modules.py:262) */
  const float* dX_std;
  const float* net_out;  /* [B A P][out_dim]: the network's output of step t-1 */
  float* Xp;             /* [B A][P][D] particles, in / out */
  float* F;              /* [B A P][in_dim] network input, out (t < N) */
  float* Zc;             /* [B][N+1][A][n] out */
  float* Uc;             /* [B][N][A][m] out */
  float* J;              /* [B A] running cost, in / out */
  float* Jc;             /* [B A] out at t = N */
  /* use_predicted_std (modules.py:242-262): the standardised normals of step
   * t - 1, [P][D]; then X_t += exp(net_out[:, D + d] + log dX_std[d]) *
   * eps_out[p][d] and out_dim >= 2 D.  NULL: the predicted std is not used. */
  const float* eps_out;
  /* [B] nullable: the rank of trajectory b among the live ones (active and
   * bwd_status == 0; anything for the others).  Given, the network-facing rows
   * - F and net_out - of candidate (b, a) are (slot[b] A + a) P + p instead of
   * (b A + a) P + p: the network then runs on the first (live count) A P rows
   * only (pddp_bnn_mlp_rows_f32).  The other arrays keep their indexing. */
  const int32_t* slot;
} pddp_bnn_step;
int pddp_bnn_moment_step_f32(const pddp_bnn_step* step, void* stream);
/* double precision: the same fields, double data */
typedef struct pddp_bnn_step_f64 {
  int32_t B, A, P, D, m, N, t;
  int32_t n_ang, ang[2], n_non, non[8];
  int32_t in_dim, out_dim;
  const double* Z;
  const double* U;
  const double* gains;
  const double* alphas;
  const double* u_min;
  const double* u_max;
  const uint8_t* active;
  const int32_t* bwd_status;
  const double* Q;
  const double* Q_term;
  const double* R;
  const double* x_goal;
  const double* u_goal;
  const double* X_mean;
  const double* X_std_inv;
  const double* dX_mean;
  const double* dX_std;
  const double* net_out;
  double* Xp;
  double* F;
  double* Zc;
  double* Uc;
  double* J;
  double* Jc;
  const double* eps_out;
  const int32_t* slot;
} pddp_bnn_step_f64;
int pddp_bnn_moment_step_f64(const pddp_bnn_step_f64* step, void* stream);

/* ---- the same network in forward mode (JVP), for the derivative rollout
 * (ilqr.py:457-468 -> utils/evaluation.py:203-235 batch_eval_dynamics, which
 * replicates the input n times and back-propagates an identity): rows come in
 * groups of `group` = 8, 16 or 32 = one (state, particle) input row followed
 * by group - 1 tangent rows d X / d direction; a tangent row passes through the
 * weights without biases and through the ReLUs linearised at its group's first
 * row.  p = (r / group) % P, R a multiple of group; everything else as
 * pddp_bnn_mlp_f32. */
int pddp_bnn_mlp_jvp_f32(int R, int P, int group, int in_dim, int H,
                         int out_dim, const float* X, const float* W1,
                         const float* b1,
                         const float* M1, const float* W2, const float* b2,
                         const float* M2, const float* W3, const float* b3,
                         float* Y, void* stream);
/* The same with only the first `live` <= group rows of every group in use (the
 * input row and the 1 + D + m - 1 tangent rows that exist): the other rows are
 * neither read nor written, and the kernel packs 32 / live whole groups into a
 * tile instead of 32 / group (group = 8, live <= 4: eight, live <= 6: five). */
int pddp_bnn_mlp_jvp_live_f32(int R, int P, int group, int live, int in_dim,
                              int H, int out_dim, const float* X,
                              const float* W1, const float* b1, const float* M1,
                              const float* W2, const float* b2, const float* M2,
                              const float* W3, const float* b3, float* Y,
                              void* stream);
/* The same on the first min(R, *live_rows) rows (a device scalar, nullable =
 * R; whole groups): see pddp_bnn_mlp_rows_f32 and pddp_bnn_jvp.slot. */
int pddp_bnn_mlp_jvp_rows_f32(int R, int P, int group, int live, int in_dim,
                              int H, int out_dim, const float* X,
                              const float* W1, const float* b1, const float* M1,
                              const float* W2, const float* b2, const float* M2,
                              const float* W3, const float* b3, float* Y,
                              const int32_t* live_rows, void* stream);
/* double precision (group = 8 or 16; 32: PDDP_E_UNSUPPORTED) */
int pddp_bnn_mlp_jvp_rows_f64(int R, int P, int group, int live, int in_dim,
                              int H, int out_dim, const double* X,
                              const double* W1, const double* b1,
                              const double* M1, const double* W2,
                              const double* b2, const double* M2,
                              const double* W3, const double* b3, double* Y,
                              const int32_t* live_rows, void* stream);

/* ---- Jacobians F_z, F_u of one moment-matched BNN step (modules.py:287-386
 * under DEFAULT encoding) in forward mode, around pddp_bnn_mlp_jvp_f32:
 *   features(t): eps = (Xp - mean_t) U_t^-1 (the detached re-whitening of
 *                modules.py:333-348), F = [B P][8][in_dim]: the input row, the
 *                D + m tangent rows for the directions (mean_d | u) at the
 *                clamped action, zero rows.  The Cholesky directions U_ab need
 *                no rows of their own: d X / d U_ab = eps[a] d X / d mean_b per
 *                particle, and the network pass is linear in the tangent;
 *   moments(t):  net_out [B P][8][out_dim] -> Xp_next (output particles =
 *                the cloud of step t + 1), Z_next = encode(mean, covariance),
 *                F_z[b][t], F_u[b][t] through the differential of the Cholesky
 *                factor.
 * pddp_bnn_jvp_group(D, m) = lanes per trajectory of the moments launch: 16
 * for D <= 4 with at most 15 directions of (z | u) (cartpole, pendulum), 32
 * for D <= 6 with at most 31 (double cartpole), 0 = PDDP_E_UNSUPPORTED (D + m >
 * 7 or more directions: the autograd path then).  The network launch in
 * between is pddp_bnn_mlp_jvp_f32 with group = 8. */
int pddp_bnn_jvp_group(int D, int m);
typedef struct pddp_bnn_jvp {
  int32_t B, P, D, m, N, t;
  int32_t n_ang, ang[2], n_non, non[8];
  int32_t in_dim, out_dim;
  const float* Z;        /* [B][N+1][n] nominal */
  const float* U;        /* [B][N][m] */
  const float* u_min;    /* [m], nullable with u_max */
  const float* u_max;
  const float* X_mean;   /* [in_dim] */
  const float* X_std_inv;
  const float* dX_mean;  /* [D] */
  const float* dX_std;
  const float* net_out;  /* [B P][8][out_dim] (moments) */
  const float* Xp;       /* [B][P][D] particles of step t */
  float* Xp_next;        /* [B][P][D] out (moments), nullable */
  float* eps;            /* [B][P][D] out (features), in (moments) */
  float* F;              /* [B P][8][in_dim] out (features) */
  float* Z_next;         /* [B][n] out (moments), nullable */
  float* F_z;            /* [B][N][n][n] out (moments) */
  float* F_u;            /* [B][N][n][m] out (moments) */
  /* use_predicted_std: standardised normals of step t, [P][D] (moments); the
   * network rows then carry 2 D outputs (mean | log std).  NULL: unused.
   * independent_noise != 0: the std is a constant of the differentiation
   * (modules.py:256-258). */
  const float* eps_out;
  int32_t independent_noise;
  /* [B] nullable: trajectories with slot[b] < 0 are skipped (nothing of theirs
   * is read or written); the others' network-facing rows - F and net_out - are
   * those of trajectory slot[b] (their rank among the ones that run), so that
   * the network launch in between covers the first (count) P 8 rows only
   * (pddp_bnn_mlp_jvp_rows_f32).  The derivative rollout of a round passes the
   * trajectories whose nominal is new. */
  const int32_t* slot;
} pddp_bnn_jvp;
int pddp_bnn_jvp_features_f32(const pddp_bnn_jvp* step, void* stream);
int pddp_bnn_jvp_moments_f32(const pddp_bnn_jvp* step, void* stream);
/* double precision: the same fields, double data */
typedef struct pddp_bnn_jvp_f64 {
  int32_t B, P, D, m, N, t;
  int32_t n_ang, ang[2], n_non, non[8];
  int32_t in_dim, out_dim;
  const double* Z;
  const double* U;
  const double* u_min;
  const double* u_max;
  const double* X_mean;
  const double* X_std_inv;
  const double* dX_mean;
  const double* dX_std;
  const double* net_out;
  const double* Xp;
  double* Xp_next;
  double* eps;
  double* F;
  double* Z_next;
  double* F_z;
  double* F_u;
  const double* eps_out;
  int32_t independent_noise;
  const int32_t* slot;
} pddp_bnn_jvp_f64;
int pddp_bnn_jvp_features_f64(const pddp_bnn_jvp_f64* step, void* stream);
int pddp_bnn_jvp_moments_f64(const pddp_bnn_jvp_f64* step, void* stream);

/* ---- value, gradient and Hessian of the QR cost on the angle-augmented
 * Gaussian state under DEFAULT encoding, every (trajectory, time step) in one
 * launch: costs/quadratic.py:60-99 on examples/cartpole/cost.py:60-87's
 * augmented state (utils/angular.py:161-248), differentiated as
 * utils/evaluation.py:238-288 batch_eval_cost does (L_z, L_u, L_zz, L_uz, L_uu
 * at the clamped action), by hyper-dual evaluation instead of autograd's double
 * backward.  Step N is the terminal state (Q_term, no action; its L_u / L_uz /
 * L_uu rows do not exist).  D in {2, 4, 6}, m <= 2, at most two angular
 * states; PDDP_E_UNSUPPORTED otherwise. */
typedef struct pddp_qr_cost {
  int32_t B, N, D, m;
  int32_t n_ang, ang[2], n_non, non[8];
  const float* Z;       /* [B][N+1][n], n = D + D (D + 1) / 2 */
  const float* U;       /* [B][N][m] */
  const float* u_min;   /* [m], nullable with u_max */
  const float* u_max;
  const float* Q;       /* [na][na], na = n_non + 2 n_ang */
  const float* Q_term;
  const float* R;       /* [m][m] */
  const float* x_goal;  /* [na] */
  const float* u_goal;  /* [m] */
  float* L;             /* [B][N+1] */
  float* L_z;           /* [B][N+1][n] */
  float* L_u;           /* [B][N][m] */
  float* L_zz;          /* [B][N+1][n][n] */
  float* L_uz;          /* [B][N][m][n] */
  float* L_uu;          /* [B][N][m][m] */
} pddp_qr_cost;
int pddp_qr_cost_derivs_f32(const pddp_qr_cost* cost, void* stream);
/* double precision: the same fields, double data */
typedef struct pddp_qr_cost_f64 {
  int32_t B, N, D, m;
  int32_t n_ang, ang[2], n_non, non[8];
  const double* Z;
  const double* U;
  const double* u_min;
  const double* u_max;
  const double* Q;
  const double* Q_term;
  const double* R;
  const double* x_goal;
  const double* u_goal;
  double* L;
  double* L_z;
  double* L_u;
  double* L_zz;
  double* L_uz;
  double* L_uu;
} pddp_qr_cost_f64;
int pddp_qr_cost_derivs_f64(const pddp_qr_cost_f64* cost, void* stream);

/* ---- pddp_amd/models/gp.py (the build's own plugin behind models/base.py:24-83
 * `DynamicsModel.forward(z, u, i, encoding)`; the reference has no GP - PARITY
 * UNPINNED): one moment-matched step of squared-exponential ARD GPs, one per
 * state increment, on the features [x_non-angular, sin a, cos a, u]:
 *   z [R][n] encoded state distributions, u [R][m] (already clamped) actions ->
 *   z_next [R][n]; with Fz [R][n][n] and Fu [R][n][m] non-NULL (both or
 *   neither) also d z_next / d z and d z_next / d u (the dynamics half of the
 *   derivative records, ilqr.py:443-470).
 * encoding: StateEncoding 1 (upper-triangular Cholesky, n = E + E(E+1)/2), 2
 * (variance), 3 (standard deviation), 4 (mean only); 0 (full covariance):
 * PDDP_E_UNSUPPORTED.  Built for (state_size, features + actions) = (2, 4),
 * (4, 6), (6, 9) - pendulum, cartpole, double cartpole; n + m <= 64.  Any
 * number of training points M, in one of two forms chosen by the entry points
 * themselves: RESIDENT while every per-point table of a row fits the
 * workgroup's 160 KB of LDS next to the inverses (double cartpole: M <= 1278
 * in f32 / 596 in f64 without the Jacobian, 890 / 208 with; the smaller
 * systems several times that), CHUNKED beyond - the per-point tables hold a
 * chunk of C points, the rows go out in consecutive launches on the stream
 * (each sized to a fraction of a second by a cost model proportional to M^2;
 * stream-ordered and capturable like one launch, same outputs).
 * PDDP_E_UNSUPPORTED: an unbuilt (state_size, d), encoding 0, n + m > 64.
 * All arrays on the device. */
typedef struct pddp_gp_model {
  int state_size;        /* E: one GP per state increment */
  int action_size;       /* m */
  int M;                 /* training points */
  int encoding;
  int n_ang, n_non;
  int ang[4], non[8];    /* angular / non-angular state indices */
  const void* Xt;        /* [M][d] training inputs, d = n_non + 2 n_ang + m */
  /* the same inputs in pairs of points, for the M^2 loop's scalar loads:
   * [MQ/2][PS], MQ = M rounded up to a multiple of 4, PS = 2 d rounded up to a
   * multiple of 4, element 2 p + h of row j = Xt[2 j + h][p]; zero beyond
   * (points M .. MQ-1 and the row padding); 16-byte aligned */
  const void* Xt_pairs;
  const void* beta;      /* [E][M]  (K_a + sn2_a I)^-1 y_a */
  const void* beta_pairs; /* [E][MQ] = beta, rows zero-padded to MQ points */
  const void* Kinv;      /* [E][M][M] (K_a + sn2_a I)^-1, symmetric */
  const void* inv_ell2;  /* [E][d]  1 / lengthscale^2 */
  const void* sf2;       /* [E] signal variances */
  const void* sn2;       /* [E] noise variances */
} pddp_gp_model;
/* Bytes of LDS a workgroup of pddp_gp_step_* needs for `M` training points
 * (inputs = n + m, element_size 4 or 8); the launch needs <= 160 KB.  -1: the
 * (state_size, d) pair is not built.  Host function. */
long long pddp_gp_step_lds_bytes(int state_size, int d, int M, int inputs, int jacobian,
                                 int element_size);
/* The form pddp_gp_step_* / _masked_* / (jacobian = 0) pddp_gp_rollout_* use for
 * these sizes: 0 resident (pddp_gp_step_lds_bytes <= 160 KB), 1 chunked, -1
 * not covered; and the points per chunk C of that launch (M for the resident
 * form, -1 when not covered).  pddp_gp_step_chunked_lds_bytes: the chunked
 * form's LDS at chunk C (-1: pair not built).  Host functions; they reflect
 * pddp_gp_step_force_chunk. */
int pddp_gp_step_form(int state_size, int d, int M, int inputs, int jacobian, int element_size);
int pddp_gp_step_chunk(int state_size, int d, int M, int inputs, int jacobian, int element_size);
long long pddp_gp_step_chunked_lds_bytes(int state_size, int d, int C, int inputs, int jacobian,
                                         int element_size);
/* For tests: C > 0 makes every later launch of this process use the chunked
 * form with chunks of (at most) C points (rounded up to an even number, and
 * never more than the LDS or M allow) also where the resident form fits; 0:
 * automatic.  pddp_gp_step_force_rows_per_launch: rows > 0 replaces the cost
 * model's rows per launch of the chunked form; 0: automatic.  Both return the
 * previous value (>= 0, never an error code; negative arguments count as 0).
 * Process-wide, not synchronised with launches in flight on other threads; a
 * hipGraph captured before a change keeps the form it was captured with. */
int pddp_gp_step_force_chunk(int C);
int pddp_gp_step_force_rows_per_launch(int rows);
int pddp_gp_step_f32(const pddp_gp_model* gp, int R, const float* z, const float* u,
                     float* z_next, float* Fz, float* Fu, void* stream);
int pddp_gp_step_f64(const pddp_gp_model* gp, int R, const double* z, const double* u,
                     double* z_next, double* Fz, double* Fu, void* stream);
/* The same with a mask over groups of `rows_per_mask` consecutive rows
 * (row_mask [ceil(R / rows_per_mask)], nullable = every row): rows of a group
 * with row_mask[group] == 0 are skipped - nothing of theirs is read or
 * written.  The derivative rollout of a round passes the trajectories whose
 * nominal is new (rows_per_mask = N): the records of the others stand
 * (ilqr.py:125-139: a rejected step retries with a larger mu on the same
 * nominal). */
int pddp_gp_step_masked_f32(const pddp_gp_model* gp, int R, const float* z, const float* u,
                            float* z_next, float* Fz, float* Fu, const uint8_t* row_mask,
                            int rows_per_mask, void* stream);
int pddp_gp_step_masked_f64(const pddp_gp_model* gp, int R, const double* z, const double* u,
                            double* z_next, double* Fz, double* Fu, const uint8_t* row_mask,
                            int rows_per_mask, void* stream);

/* ---- the GP workload's line search as a device rollout (the plugin path's
 * counterpart of pddp_line_search_*; ilqr.py:677-723 control law + rollout,
 * :764-791 trajectory cost): for every trajectory b and step size a, from
 * Z_new[0] = Z[b][0],
 *   u_t = clamp(U[b][t] + alphas[a] k[b][t] + K[b][t] (z_t - Z[b][t]))
 *   Jc[b][a] += QR cost of (z_t, u_t);  z_{t+1} = GP step of (z_t, u_t)
 * and the terminal cost of z_N: N + 1 launches of the moment-matched step's
 * kernel with nothing between them (stream-ordered, capturable).  The cost is
 * the QR cost on the angle-augmented Gaussian state (costs/quadratic.py:60-99:
 * E[(x~ - x_goal)^T Q (x~ - x_goal)] + (u - u_goal)^T R (u - u_goal), Q_term
 * at t = N) with the model's own angular / non-angular indices - its moments
 * are the step's feature moments; the covariance term enters as the encoding
 * carries it (full for 1, diagonal for 2 / 3, none for 4).  Zc [B][N+1][A][n],
 * Uc [B][N][A][m] time-major like pddp_line_search_*; Jc [B][A].  Rows of
 * inactive trajectories (active[b] == 0) and of failed sweeps
 * (bwd_status[b] != 0) are skipped (both nullable).  Same model limits as
 * pddp_gp_step_*; na = n_non + 2 n_ang <= 8, m <= 4. */
typedef struct pddp_gp_rollout {
  int32_t B, N, A;
  const void* Z;        /* [B][N+1][n] nominal states */
  const void* U;        /* [B][N][m] nominal actions (un-clamped) */
  const void* gains;    /* [B][N][m + m n]: k | K */
  const void* alphas;   /* [A] */
  const void* u_min;    /* [m], nullable with u_max */
  const void* u_max;
  const uint8_t* active;       /* [B] nullable */
  const int32_t* bwd_status;   /* [B] nullable */
  void* Zc;
  void* Uc;
  void* Jc;
  const void* Q;        /* [na][na] */
  const void* Q_term;
  const void* R;        /* [m][m] */
  const void* x_goal;   /* [na] */
  const void* u_goal;   /* [m] */
} pddp_gp_rollout;
int pddp_gp_rollout_f32(const pddp_gp_model* model, const pddp_gp_rollout* r,
                        void* stream);
int pddp_gp_rollout_f64(const pddp_gp_model* model, const pddp_gp_rollout* r,
                        void* stream);

/* Timing helper for bench.py: HIP events on `stream` (torch.cuda.Event only
 * sees torch's current stream). Host functions. */
int pddp_event_create(void** ev);
int pddp_event_record(void* ev, void* stream);
int pddp_event_elapsed_ms(void* start, void* stop, float* ms); /* syncs stop */
int pddp_event_destroy(void* ev);
/* Attaches (start, stop) to the NEXT kernel this host thread launches through
 * any pddp_* entry point: the events then time that kernel from its own start
 * to its own end (what rocprofv3 --kernel-trace reports), without the
 * stream's dispatch gaps.  One-shot; (NULL, NULL) detaches. */
int pddp_attach_events(void* start, void* stop);

#ifdef __cplusplus
}
#endif
#endif /* PDDP_HIP_H */
