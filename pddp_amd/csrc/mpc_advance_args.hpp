// mpc_advance_args.hpp - what the three hand-over kernels (mpc_advance.hip:
// with one goal, along a reference; mpc_advance_noise.hip: under noise) share
// besides the kernel text (mpc_advance_body.inc) and its goal hooks
// (mpc_advance_goal_hooks.inc): the argument blocks with their test, the grid
// and the entry points' common parameters.
#pragma once

#include "pddp_common.hpp"

namespace pddp {

template <typename T>
struct MpcAdvanceArgs {
  int B, N, T_, t;   // control step t of T_
  const T* table;    // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  const T* plant;    // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  T* z0;             // [B][n]       in: x_t, out: x_{t+1}  (under measurement
                     //              noise: y_t, y_{t+1})
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

// The block of track_mpc_advance_kernel: the one above without `table` (the
// table travels in the launch's RefArgs; `plant` supplies parameters only).  A
// type of its own because the kernel's argument layout is this one.
template <typename T>
struct TrackAdvanceArgs {
  int B, N, T_, t;
  const T* plant;
  T* z0;
  T* U;
  T* Z;
  const T* u_min;
  const T* u_max;
  const T* disturbance;
  const uint8_t* mask;
  T* Xlog;
  T* Ulog;
  T* Jcl;
  int32_t* state_log;
  uint8_t* live_log;
  double* mu;
  double* delta;
  int32_t* state;
  int32_t* iter;
  uint8_t* active;
  uint8_t* fresh;
  int32_t* n_live;
};

// Host side of the three entry points: the argument test of either block (in
// the style of args_ok, problem_args.hpp) and the grid, one lane per
// trajectory.
template <typename Args>
inline bool advance_args_ok(const Args& a) {
  return !(a.B <= 0 || a.N <= 0 || a.T_ <= 0 || a.t < 0 || a.t >= a.T_ ||
           !a.z0 || !a.U || !a.Z || !a.Xlog || !a.Ulog || !a.Jcl ||
           !a.state_log || !a.live_log || !a.mu || !a.delta || !a.state ||
           !a.iter || !a.active || !a.fresh);
}
template <typename Args>
inline dim3 advance_blocks(const Args& a) {
  return dim3((a.B + kWave - 1) / kWave);
}

}  // namespace pddp

// The parameters every pddp_mpc_advance*_ entry point has, in the ABI's order
// (the noisy one's noise stands between the two groups; include/pddp_hip.h
// spells the lists out and the compiler holds these to it), and the blocks
// made of them: the *_ARGS name the parameters of the entry point that expands
// them.  Each unit undefines the four behind its entry points.
#define PDDP_ADVANCE_STEP_PARAMS(T)                                            \
  int B, int N, int TT, int t, T* z0, T* U, T* Z, const T* u_min,              \
      const T* u_max, const T* plant, const T* disturbance
#define PDDP_ADVANCE_LOG_PARAMS(T)                                             \
  const uint8_t* mask, T* Xlog, T* Ulog, T* Jcl, int32_t* state_log,           \
      uint8_t* live_log, double* mu, double* delta, int32_t* state,            \
      int32_t* iter, uint8_t* active, uint8_t* fresh, int32_t* n_live,         \
      void* stream
#define PDDP_TRACK_ADVANCE_ARGS                                                \
  B, N, TT, t, plant, z0, U, Z, u_min, u_max, disturbance, mask, Xlog, Ulog,   \
      Jcl, state_log, live_log, mu, delta, state, iter, active, fresh, n_live
#define PDDP_MPC_ADVANCE_ARGS                                                  \
  B, N, TT, t, table, plant, z0, U, Z, u_min, u_max, disturbance, mask, Xlog,  \
      Ulog, Jcl, state_log, live_log, mu, delta, state, iter, active, fresh,   \
      n_live
