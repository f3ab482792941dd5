// mpc_advance.hip - the hand-over between two control steps of a receding-
// horizon (MPC) trial: apply the first action of every trajectory's re-optimised
// nominal to its plant, log the trial, shift the warm start, roll out the new
// nominal and re-arm the controller state machine, in one launch.
//
//   the trial step of the outer loop   pddp/controllers/pddp.py:209-245
//                                      (_apply_controller, mpc=True, batched:
//                                      the sample models as the plant)
//   emit U[0], shift the nominal       ilqr.py:355-362 (forward, mpc=True)
//   the regularisation reset           ilqr.py:364-367 (_reset_reg)
//
// A translation unit of its own: it includes models.hpp and problem_args.hpp
// as they are and shares no text with problem_kernels.hip (csrc/Makefile:
// moving shared text around changes the FMA contraction of the kernels there).
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"

namespace pddp {

constexpr int kAdvanceLiveShards = PDDP_LIVE_SHARDS;

template <typename T>
struct MpcAdvanceArgs {
  int B, N, T_, t;   // control step t of T_
  const T* table;    // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  const T* plant;    // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  T* z0;             // [B][n]       in: x_t, out: x_{t+1}
  T* U;              // [B][N][m]    shifted in place (unclamped)
  T* Z;              // [B][N+1][n]  out: the rollout of the shifted nominal
  const T* u_min;
  const T* u_max;
  const T* disturbance;  // [B][T_][n] or NULL
  const uint8_t* mask;   // [B] or NULL
  T* Xlog;               // [B][T_+1][n]
  T* Ulog;               // [B][T_][m]
  T* Jcl;                // [B]
  int32_t* state_log;    // [B][T_]
  uint8_t* live_log;     // [B][T_]
  double* mu;
  double* delta;
  int32_t* state;
  int32_t* iter;
  uint8_t* active;
  uint8_t* fresh;
  int32_t* n_live;  // [PDDP_LIVE_SHARDS] or NULL
};

// `row` of the table's layout written over P's params and goals.
template <typename T, int MODEL>
PDDP_DEV void overwrite_row(ProblemT<T>& P, const T* row) {
  using D = ModelDims<MODEL>;
  P.dt = row[PDDP_BATCH_PARAMS];
#pragma unroll
  for (int i = 0; i < kModelParamCount<MODEL> - 1; ++i)
    P.p[i] = row[PDDP_BATCH_PARAMS + 1 + i];
#pragma unroll
  for (int i = 0; i < D::na; ++i) P.goal[i] = row[PDDP_BATCH_X_GOAL + i];
#pragma unroll
  for (int i = 0; i < D::m; ++i) P.ugoal[i] = row[PDDP_BATCH_U_GOAL + i];
}

// Mapping: one lane per trajectory, as nominal_rollout_kernel; everything of
// trajectory b is read and written by its lane alone, J in t order, no
// atomics.  The shards of n_live belong to no trajectory: the first workgroup
// zeroes them (the rounds before and after this launch are stream-ordered
// around it).
template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void mpc_advance_kernel(
    ProblemT<T> shared, MpcAdvanceArgs<T> a) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  if (blockIdx.x == 0 && a.n_live != nullptr) {
    for (int i = threadIdx.x; i < kAdvanceLiveShards; i += blockDim.x)
      a.n_live[i] = 0;
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  const int N = a.N, t = a.t, TT = a.T_;

  // 1. the controller as the step's rounds left it
  a.state_log[(size_t)b * TT + t] = a.state[b];
  a.live_log[(size_t)b * TT + t] = a.active[b] != 0 ? 1 : 0;

  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  T umin[m], umax[m];
#pragma unroll
  for (int r = 0; r < m; ++r) {
    umin[r] = bounded ? a.u_min[r] : T(0);
    umax[r] = bounded ? a.u_max[r] : T(0);
  }
  T* Zb = a.Z + (size_t)b * (N + 1) * n;
  T* Ub = a.U + (size_t)b * N * m;
  T* Xb = a.Xlog + (size_t)b * (TT + 1) * n;

  // the controller's model: the shared problem with row b of the table
  // written over it; Q, Qt and R are never written and stay scalar operands of
  // the kernel argument
  ProblemT<T> P = shared;
  if (a.table != nullptr)
    overwrite_row<T, MODEL>(P, a.table + (size_t)b * PDDP_BATCH_ROW);

  T z[n], zn[n], u[m], cur[m], nxt[m];
#pragma unroll
  for (int j = 0; j < n; ++j) z[j] = a.z0[(size_t)b * n + j];
#pragma unroll
  for (int j = 0; j < m; ++j) {
    u[j] = Ub[j];
    if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
  }
  // the warm start's first row, requested ahead of the plant step
  const int i1 = N > 1 ? 1 : 0;
#pragma unroll
  for (int j = 0; j < m; ++j) cur[j] = Ub[i1 * m + j];

  {
    // 2. - 4. apply u to the plant of row b, log the trial
    ProblemT<T> Pl = P;
    if (a.plant != nullptr)
      overwrite_row<T, MODEL>(Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);
    T w[n];
#pragma unroll
    for (int j = 0; j < n; ++j) w[j] = T(0);
    if (a.disturbance != nullptr) {
#pragma unroll
      for (int j = 0; j < n; ++j)
        w[j] = a.disturbance[((size_t)b * TT + t) * n + j];
    }
    T J = T(0);
    if (t > 0) J = a.Jcl[b];
#pragma unroll
    for (int j = 0; j < n; ++j) Xb[(size_t)t * n + j] = z[j];
#pragma unroll
    for (int j = 0; j < m; ++j) a.Ulog[((size_t)b * TT + t) * m + j] = u[j];
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    J += cost_value<T, MODEL>(Pl, z, u, tr, false);
    dynamics<T, MODEL, false>(Pl, z, u, tr, zn, nullptr, nullptr);
    if (a.disturbance != nullptr) {
#pragma unroll
      for (int j = 0; j < n; ++j) zn[j] = zn[j] + w[j];
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z[j] = zn[j];
    if (t == TT - 1) {
#pragma unroll
      for (int j = 0; j < n; ++j) Xb[(size_t)TT * n + j] = z[j];
      J += cost_value<T, MODEL>(Pl, z, nullptr, trig_of<T, MODEL>(z), true);
    }
    a.Jcl[b] = J;
  }

  // 5. + 6. the shift (a plain copy of unclamped words; new row i is old row
  // i + 1, the last one repeated) and the rollout of the shifted nominal from
  // x' under the controller's model, in one loop over time.  Row i + 2 is read
  // before row i is written; the last row is read for the last time in the
  // iteration before it is written.
#pragma unroll
  for (int j = 0; j < n; ++j) {
    a.z0[(size_t)b * n + j] = z[j];
    Zb[j] = z[j];
  }
  for (int i = 0; i < N; ++i) {
    const int i2 = (i + 2 < N) ? i + 2 : N - 1;
#pragma unroll
    for (int j = 0; j < m; ++j) nxt[j] = Ub[i2 * m + j];
#pragma unroll
    for (int j = 0; j < m; ++j) {
      Ub[i * m + j] = cur[j];
      u[j] = cur[j];
      if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
    }
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    dynamics<T, MODEL, false>(P, z, u, tr, zn, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = zn[j];
      Zb[(i + 1) * n + j] = z[j];
    }
#pragma unroll
    for (int j = 0; j < m; ++j) cur[j] = nxt[j];
  }

  // 7. re-arm: the words of reset_controller_state()       (ilqr.py:364-367)
  a.mu[b] = 0.0;
  a.delta[b] = 2.0;
  a.state[b] = PDDP_STATE_UNDEFINED;
  a.iter[b] = 1;
  a.active[b] = 1;
  a.fresh[b] = 1;
}

template <typename T, int MODEL>
static int launch_mpc_advance(const pddp_problem& p, MpcAdvanceArgs<T> a,
                              hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const dim3 blocks((a.B + kWave - 1) / kWave);
  PDDP_LAUNCH((mpc_advance_kernel<T, MODEL>), blocks, dim3(kWave), 0, st, P,
              a);
  return launch_status();
}

template <typename T>
static int mpc_advance_impl(const pddp_problem* p, const T* table, int B,
                            int N, int TT, int t, T* z0, T* U, T* Z,
                            const T* u_min, const T* u_max, const T* plant,
                            const T* disturbance, const uint8_t* mask, T* Xlog,
                            T* Ulog, T* Jcl, int32_t* state_log,
                            uint8_t* live_log, double* mu, double* delta,
                            int32_t* state, int32_t* iter, uint8_t* active,
                            uint8_t* fresh, int32_t* n_live, void* stream) {
  if (B <= 0 || N <= 0 || TT <= 0 || t < 0 || t >= TT || !z0 || !U || !Z ||
      !Xlog || !Ulog || !Jcl || !state_log || !live_log || !mu || !delta ||
      !state || !iter || !active || !fresh)
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  MpcAdvanceArgs<T> a{B,     N,     TT,        t,        table, plant,
                      z0,    U,     Z,         u_min,    u_max, disturbance,
                      mask,  Xlog,  Ulog,      Jcl,      state_log, live_log,
                      mu,    delta, state,     iter,     active, fresh,
                      n_live};
  PDDP_DISPATCH_MODEL(launch_mpc_advance, T, p, a, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

int pddp_mpc_advance_f32(const pddp_problem* p, const float* table, int B,
                         int N, int T, int t, float* z0, float* U, float* Z,
                         const float* u_min, const float* u_max,
                         const float* plant, const float* disturbance,
                         const uint8_t* mask, float* Xlog, float* Ulog,
                         float* Jcl, int32_t* state_log, uint8_t* live_log,
                         double* mu, double* delta, int32_t* state,
                         int32_t* iter, uint8_t* active, uint8_t* fresh,
                         int32_t* n_live, void* stream) {
  return pddp::mpc_advance_impl<float>(
      p, table, B, N, T, t, z0, U, Z, u_min, u_max, plant, disturbance, mask,
      Xlog, Ulog, Jcl, state_log, live_log, mu, delta, state, iter, active,
      fresh, n_live, stream);
}
int pddp_mpc_advance_f64(const pddp_problem* p, const double* table, int B,
                         int N, int T, int t, double* z0, double* U, double* Z,
                         const double* u_min, const double* u_max,
                         const double* plant, const double* disturbance,
                         const uint8_t* mask, double* Xlog, double* Ulog,
                         double* Jcl, int32_t* state_log, uint8_t* live_log,
                         double* mu, double* delta, int32_t* state,
                         int32_t* iter, uint8_t* active, uint8_t* fresh,
                         int32_t* n_live, void* stream) {
  return pddp::mpc_advance_impl<double>(
      p, table, B, N, T, t, z0, U, Z, u_min, u_max, plant, disturbance, mask,
      Xlog, Ulog, Jcl, state_log, live_log, mu, delta, state, iter, active,
      fresh, n_live, stream);
}

}  // extern "C"
