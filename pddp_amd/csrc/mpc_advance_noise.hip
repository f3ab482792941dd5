// mpc_advance_noise.hip - the hand-over between two control steps of a
// receding-horizon (MPC) trial under process and measurement noise drawn on the
// device: pddp_mpc_advance_*'s launch, with or without the goal per time step
// of pddp_mpc_advance_track_* (both mpc_advance.hip), with
//
//   x_{t+1} = plant(x_t, u_t) + disturbance + w_std (.) w_t
//   y_{t+1} = x_{t+1} + v_std (.) v_{t+1}     what the controller re-plans from
//
// where w and v are the unit normals of closed_loop_draws.hpp: trial b is
// rollout `rollout_offset + b` of the generator, control step t its step
// `step_offset + t`, stream 0 process and stream 1 measurement noise - the
// draws pddp_closed_loop_noisy_* makes with S = 1, so that a fixed policy and a
// re-planning one can be run under the same noise.  With measurement noise the
// plant's state lives in `x_true`; z0 and Z[:, 0] hold what the controller
// sees.  The trial's logs and its cost are the true states'.
//
// A translation unit of its own (csrc/Makefile: FLAGS_mpc_advance_noise, whose
// scheduling flag is not mpc_advance.hip's).  The kernel is
// mpc_advance_kernel's text, mpc_advance_body.inc, and argument block, with
// the goal hooks of mpc_advance_goal_hooks.inc and the draws at the three state
// hooks; PROC / OBS / TRACK are compile-time, so that a launch carries the
// instructions of what it asked for and of nothing else.
// pddp_mpc_observe_* forms the first observation of a trial through the device
// function the hand-over forms every later one with.
#include <climits>
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_draws.hpp"
#include "mpc_advance_args.hpp"
#include "ref_args.hpp"

namespace pddp {

// the noise of one control step of a launch of trials
template <typename T>
struct TrialNoise {
  const T* w_std;  // [n]; NULL exactly when the kernel's PROC is false
  const T* v_std;  // [n]; NULL exactly when the kernel's OBS is false
  uint64_t seed, offset;
  int step;   // step_offset + t: w of this step, v of the next
  T* x_true;  // [B][n]         OBS: in x_t, out x_{t+1}
  T* Ylog;    // [B][T_+1][n]   OBS, nullable: y_{t+1} at row t + 1
};

// Mapping, ownership and the n_live shards: mpc_advance_kernel's.  The key of
// the draws (`seed`) is a kernel argument and the step a scalar: both stay in
// scalar registers; the rollout index is the lane's counter word.  The noise
// levels are the launch's (scalar loads).
template <typename T, int MODEL, bool PROC, bool OBS, bool TRACK>
__global__ __launch_bounds__(kWave) void mpc_advance_noisy_kernel(
    ProblemT<T> shared, MpcAdvanceArgs<T> a, TrialNoise<T> noise,
    RefArgs<T> goals) {
#define PDDP_TABLE a.table
#include "mpc_advance_goal_hooks.inc"
// the plant is at x_true, not at what the controller saw.  The draws of the
// step depend on no state: they are made here, ahead of the dependent chain
// and of the two problem copies, and wait as unit normals in vector registers.
#define PDDP_PLANT_STATE                                                       \
  const uint64_t roll = noise.offset + (uint64_t)b;                            \
  T wn[n], vn[n];                                                              \
  if constexpr (PROC) draw_units<T, n>(noise.seed, roll, noise.step, 0, wn);   \
  if constexpr (OBS) {                                                         \
    draw_units<T, n>(noise.seed, roll, noise.step + 1, 1, vn);                 \
    _Pragma("unroll") for (int j = 0; j < n; ++j) z[j] =                       \
        noise.x_true[(size_t)b * n + j];                                       \
  }
// x' = f(x, u) + disturbance + w_std (.) w_t
#define PDDP_PLANT_STEPPED \
  if constexpr (PROC) add_scaled<T, n>(noise.w_std, wn, zn);
// x' stays the plant's; the new nominal starts at y' = x' + v_std (.) v_{t+1}
#define PDDP_NOMINAL_START                                                     \
  if constexpr (OBS) {                                                         \
    _Pragma("unroll") for (int j = 0; j < n; ++j)                              \
        noise.x_true[(size_t)b * n + j] = z[j];                                \
    add_scaled<T, n>(noise.v_std, vn, z);                                      \
    if (noise.Ylog != nullptr) {                                               \
      _Pragma("unroll") for (int j = 0; j < n; ++j)                            \
          noise.Ylog[((size_t)b * (TT + 1) + t + 1) * n + j] = z[j];           \
    }                                                                          \
  }
#include "mpc_advance_body.inc"
#undef PDDP_NOMINAL_START
#undef PDDP_PLANT_STEPPED
#undef PDDP_PLANT_STATE
#undef PDDP_TERMINAL_GOALS
#undef PDDP_PLANT_OF_B
#undef PDDP_PROBLEM_OF_B
#undef PDDP_TABLE
}

// y = x + v_std (.) v(r, step): one lane per trajectory, the hand-over's
// device function (draw_added), so that the first observation of a trial obeys
// the law of every later one.
template <typename T>
struct ObserveArgs {
  int B, step;
  const T* x;      // [B][n]
  const T* v_std;  // [n]
  uint64_t seed, offset;
  const uint8_t* mask;  // [B] or NULL
  T* y;                 // [B][n]
};

template <typename T, int n>
__global__ __launch_bounds__(kWave) void mpc_observe_kernel(ObserveArgs<T> a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  T z[n];
#pragma unroll
  for (int j = 0; j < n; ++j) z[j] = a.x[(size_t)b * n + j];
  draw_added<T, n>(a.seed, a.offset + (uint64_t)b, a.step, 1, a.v_std, z);
#pragma unroll
  for (int j = 0; j < n; ++j) a.y[(size_t)b * n + j] = z[j];
}

template <typename T>
struct NoisyAdvanceLaunch {
  MpcAdvanceArgs<T> a;
  TrialNoise<T> noise;
  RefArgs<T> r;
  bool track;
};

template <typename T, int MODEL>
static int launch_noisy_advance(const pddp_problem& p, NoisyAdvanceLaunch<T> w,
                                hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const dim3 blocks = advance_blocks(w.a);
#define PDDP_NOISY(PROC, OBS)                                                  \
  do {                                                                         \
    if (w.track)                                                               \
      PDDP_LAUNCH((mpc_advance_noisy_kernel<T, MODEL, PROC, OBS, true>),       \
                  blocks, dim3(kWave), 0, st, P, w.a, w.noise, w.r);           \
    else                                                                       \
      PDDP_LAUNCH((mpc_advance_noisy_kernel<T, MODEL, PROC, OBS, false>),      \
                  blocks, dim3(kWave), 0, st, P, w.a, w.noise, w.r);           \
  } while (0)
  if (w.noise.w_std != nullptr && w.noise.v_std != nullptr)
    PDDP_NOISY(true, true);
  else if (w.noise.w_std != nullptr)
    PDDP_NOISY(true, false);
  else
    PDDP_NOISY(false, true);
#undef PDDP_NOISY
  return launch_status();
}

// `noise` as the entry point got it: `step` holds step_offset, x_true and Ylog
// are taken as given.
template <typename T>
static int noisy_advance_impl(const pddp_problem* p, MpcAdvanceArgs<T> a,
                              TrialNoise<T> noise, const T* ref, int ref_len,
                              int ref_t0, void* stream) {
  if (!advance_args_ok(a)) return PDDP_E_BADARG;
  // (no noise at all is pddp_mpc_advance[_track]_*'s launch)
  if (noise.w_std == nullptr && noise.v_std == nullptr) return PDDP_E_BADARG;
  if (noise.v_std != nullptr && noise.x_true == nullptr) return PDDP_E_BADARG;
  // (step_offset + t + 1 is a counter word of the draws: an int)
  if (noise.step < 0 || noise.step > INT_MAX - a.T_) return PDDP_E_BADARG;
  noise.step += a.t;
  if (noise.v_std == nullptr) noise.x_true = noise.Ylog = nullptr;
  NoisyAdvanceLaunch<T> w{a, noise, {a.table, nullptr, 1, 0}, ref != nullptr};
  if (ref != nullptr && !ref_args(a.table, ref, ref_len, ref_t0, &w.r))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_noisy_advance, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int observe_impl(int B, int n, const T* x, const T* v_std,
                        uint64_t seed, uint64_t rollout_offset, int step,
                        const uint8_t* mask, T* y, void* stream) {
  if (B <= 0 || n <= 0 || n > PDDP_MAX_STATE || step < 0 || !x || !v_std || !y)
    return PDDP_E_BADARG;
  const ObserveArgs<T> a{B, step, x, v_std, seed, rollout_offset, mask, y};
  const dim3 blocks((B + kWave - 1) / kWave);
  hipStream_t st = (hipStream_t)stream;
#define PDDP_OBSERVE(K)                                                        \
  case K:                                                                      \
    PDDP_LAUNCH((mpc_observe_kernel<T, K>), blocks, dim3(kWave), 0, st, a);    \
    break;
  switch (n) {
    PDDP_OBSERVE(1)
    PDDP_OBSERVE(2)
    PDDP_OBSERVE(3)
    PDDP_OBSERVE(4)
    PDDP_OBSERVE(5)
    PDDP_OBSERVE(6)
    PDDP_OBSERVE(7)
    default:
      PDDP_LAUNCH((mpc_observe_kernel<T, 8>), blocks, dim3(kWave), 0, st, a);
  }
#undef PDDP_OBSERVE
  return launch_status();
}

}  // namespace pddp

extern "C" {

#define PDDP_MPC_NOISE_ENTRY_POINTS(SUF, T)                                    \
  int pddp_mpc_advance_noisy_##SUF(                                            \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, PDDP_ADVANCE_STEP_PARAMS(T), const T* w_std,                 \
      const T* v_std, uint64_t seed, uint64_t rollout_offset,                  \
      int step_offset, T* x_true, T* Ylog, PDDP_ADVANCE_LOG_PARAMS(T)) {       \
    return pddp::noisy_advance_impl<T>(                                        \
        p, {PDDP_MPC_ADVANCE_ARGS},                                            \
        {w_std, v_std, seed, rollout_offset, step_offset, x_true, Ylog}, ref,  \
        ref_len, ref_t0, stream);                                              \
  }                                                                            \
  int pddp_mpc_observe_##SUF(int B, int n, const T* x, const T* v_std,         \
                             uint64_t seed, uint64_t rollout_offset, int step, \
                             const uint8_t* mask, T* y, void* stream) {        \
    return pddp::observe_impl<T>(B, n, x, v_std, seed, rollout_offset, step,   \
                                 mask, y, stream);                             \
  }

PDDP_MPC_NOISE_ENTRY_POINTS(f32, float)
PDDP_MPC_NOISE_ENTRY_POINTS(f64, double)
#undef PDDP_MPC_NOISE_ENTRY_POINTS
#undef PDDP_MPC_ADVANCE_ARGS
#undef PDDP_TRACK_ADVANCE_ARGS
#undef PDDP_ADVANCE_LOG_PARAMS
#undef PDDP_ADVANCE_STEP_PARAMS

}  // extern "C"
