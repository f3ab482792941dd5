// closed_loop.hip - closed-loop policy evaluation: S rollouts of every
// trajectory's time-varying feedback policy (Z, U, K), each from its own
// initial state on its own plant, and the statistics of a controller's costs
// (pddp_closed_loop_*); the same under process and measurement noise drawn on
// the device (pddp_closed_loop_noisy_*, the draws written out by
// pddp_closed_loop_draws_*), and, with or without that noise, costed ALONG A
// REFERENCE (pddp_closed_loop_track_*, ILQRSolver.closed_loop(track=True)).
//
//   the trial step of the outer loop   pddp/controllers/pddp.py:209-245
//                                      (_apply_controller, batched: the sample
//                                      models as the plant)
//   the feedback law                   ilqr.py:318-355 (forward, mpc=False)
//   the cost of a rollout              ilqr.py:764-791 (_trajectory_cost)
//
//   noise:  y = x_t + v_std (.) v_t          the controller sees a noisy state
//           x_{t+1} = plant(x_t, u_t) + w_std (.) w_t
//   where v_t and w_t are n unit normals each, a pure function of (seed,
//   rollout, step, stream, component): Philox4x32-10 on a counter, Box-Muller
//   on its words (closed_loop_draws.hpp).  No noise tensor exists.
//
//   `ref` [B][ref_len][PDDP_REF_ROW], the records': rollout (b, s) takes the
//   stage cost of step t under row min(ref_t0 + t, ref_len - 1) of trajectory
//   b and the terminal cost under row min(ref_t0 + N, ref_len - 1), x_goal
//   only.  The S rollouts of a trajectory share its reference; the plant row
//   supplies the model PARAMETERS only, its goal fields are not read.
//
// One translation unit (csrc/Makefile: FLAGS_closed_loop), one host path, three
// rollout kernels.  The rollout's loop resembles the line search's but is its
// own text - the feedback law and the output layout differ; the parameter count
// is model_params.hpp's, the row writer stays written out at its one call site
// (DESIGN.md 3.4f).  That text is closed_loop_body.inc, included by each kernel
// with its hooks: empty (3.4c), the draws at the noise hooks (3.4g), the goals
// of a reference row at the goal hooks as well (3.4h).  Mapping, output layout,
// the uniform `keep` branch, the statistics and their order are the text's, so
// the same for all three.  Each kernel keeps a parameter list of its own: an
// argument that is never read still re-schedules these kernels (3.4k).
#include <limits>
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"
#include "ref_args.hpp"

namespace pddp {

// The step's nominal row Z[b][t] | U[b][t] | K[b][t] is read by every lane,
// the lanes of a trajectory at the same addresses: one broadcast.  (Where a
// wavefront holds one trajectory, G >= 64, the row is wave-uniform; fetching it
// through scalar loads was built and measured slower)
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void closed_loop_kernel(
    ProblemT<T> shared, ClosedLoopArgs<T> a, const T* __restrict__ Znom,
    const T* __restrict__ Unom, const T* __restrict__ gains) {
#define PDDP_NOISE_LEVELS
#define PDDP_NOISE_OF_ROLLOUT
#define PDDP_NOISE_OF_STEP
#define PDDP_SEEN(c) z[c]
#define PDDP_NEXT(j) zn[j]
#define PDDP_GOALS_TAKE_FIRST
#define PDDP_GOALS_REQUEST_NEXT
#define PDDP_GOALS_TAKE_NEXT
#include "closed_loop_body.inc"
#undef PDDP_GOALS_TAKE_NEXT
#undef PDDP_GOALS_REQUEST_NEXT
#undef PDDP_GOALS_TAKE_FIRST
#undef PDDP_NEXT
#undef PDDP_SEEN
#undef PDDP_NOISE_OF_STEP
#undef PDDP_NOISE_OF_ROLLOUT
#undef PDDP_NOISE_LEVELS
}

// closed_loop_kernel's text with noise at its hooks.  PROC / OBS: which
// streams the launch draws - compile-time, so that a step is one basic block
// and the draws, which depend on no state, are the compiler's to place among
// the step's dependent chain.  The measurement noise of step t + 1 is drawn
// during step t (its first use is the head of the next chain; after step N - 1
// nobody reads it), the process noise of step t during step t (its one use is
// the chain's end).
template <typename T, int MODEL, bool PROC, bool OBS>
__global__ __launch_bounds__(kClosedLoopThreads) void closed_loop_noisy_kernel(
    ProblemT<T> shared, ClosedLoopArgs<T> a, NoiseArgs<T> noise,
    const T* __restrict__ Znom, const T* __restrict__ Unom,
    const T* __restrict__ gains) {
#include "closed_loop_noise_hooks.inc"
#define PDDP_GOALS_TAKE_FIRST
#define PDDP_GOALS_REQUEST_NEXT
#define PDDP_GOALS_TAKE_NEXT
#include "closed_loop_body.inc"
#undef PDDP_GOALS_TAKE_NEXT
#undef PDDP_GOALS_REQUEST_NEXT
#undef PDDP_GOALS_TAKE_FIRST
#undef PDDP_NEXT
#undef PDDP_SEEN
#undef PDDP_NOISE_OF_STEP
#undef PDDP_NOISE_OF_ROLLOUT
#undef PDDP_NOISE_LEVELS
}

// closed_loop_kernel's text with noise and goals at its hooks.  PROC / OBS as
// in closed_loop_noisy_kernel; both false is the noise-free rollout (the draws
// and `noise` are then dead text).  The goal row of step t + 1 is requested
// together with that step's nominal row and draws, ahead of the dependent
// chain, up to row N, under which the terminal cost is taken - as in
// track_line_search_kernel.  All lanes of a trajectory read the same row: one
// broadcast; the adjacent words of a row half come out as one 16-byte load.
template <typename T, int MODEL, bool PROC, bool OBS>
__global__ __launch_bounds__(kClosedLoopThreads) void closed_loop_track_kernel(
    ProblemT<T> shared, ClosedLoopArgs<T> a, NoiseArgs<T> noise,
    RefArgs<T> goals, const T* __restrict__ Znom, const T* __restrict__ Unom,
    const T* __restrict__ gains) {
#include "closed_loop_noise_hooks.inc"
#define PDDP_GOALS_TAKE_FIRST                                                  \
  const T* row0 = ref_row(goals, b, 0);                                        \
  PDDP_COPY(D::na, P.goal, row0 + PDDP_REF_X_GOAL)                             \
  PDDP_COPY(m, P.ugoal, row0 + PDDP_REF_U_GOAL)
#define PDDP_GOALS_REQUEST_NEXT                                                \
  const T* row = ref_row(goals, b, t + 1);                                     \
  T xg2[D::na], ug2[m];                                                        \
  PDDP_COPY(D::na, xg2, row + PDDP_REF_X_GOAL)                                 \
  PDDP_COPY(m, ug2, row + PDDP_REF_U_GOAL)
#define PDDP_GOALS_TAKE_NEXT                                                   \
  PDDP_COPY(m, P.ugoal, ug2)                                                   \
  PDDP_COPY(D::na, P.goal, xg2)
#include "closed_loop_body.inc"
#undef PDDP_GOALS_TAKE_NEXT
#undef PDDP_GOALS_REQUEST_NEXT
#undef PDDP_GOALS_TAKE_FIRST
#undef PDDP_NEXT
#undef PDDP_SEEN
#undef PDDP_NOISE_OF_STEP
#undef PDDP_NOISE_OF_ROLLOUT
#undef PDDP_NOISE_LEVELS
}

// ---- the draws written out (closed_loop_draws.hpp holds the draws) ---------

template <typename T>
struct DrawArgs {
  int B, N, S, n, which;
  uint64_t seed, offset;
  T* W;  // [B][N][S][n]
};

// One lane per (b, t, s), s fastest: W is time-major like Xc.
template <typename T>
__global__ __launch_bounds__(kClosedLoopThreads) void closed_loop_draws_kernel(
    DrawArgs<T> a) {
  constexpr int kPer = DrawBlock<T>::kPer;
  const size_t total = (size_t)a.B * a.N * a.S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t bt = i / a.S;
    const int s = (int)(i - bt * a.S);
    const size_t b = bt / a.N;
    const int t = (int)(bt - b * a.N);
    const uint64_t r = a.offset + (uint64_t)b * a.S + s;
    T* out = a.W + i * a.n;
    for (int k = 0; k * kPer < a.n; ++k) {
      T z[kPer];
      draw_block(a.seed, r, t, a.which, k, z);
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (k * kPer + j < a.n) out[k * kPer + j] = z[j];
    }
  }
}

// ---- the host path of the three rollouts -----------------------------------

// What a launch carries: an entry point leaves what it lacks null - no noise
// level: none of that stream is drawn; no `r.ref`: one goal per rollout.
template <typename T>
struct ClosedLoopLaunch {
  ClosedLoopArgs<T> a;
  NoiseArgs<T> noise;
  RefArgs<T> r;
  const T* Z;
  const T* U;
  const T* gains;
};

template <typename T, int MODEL>
static int launch_closed_loop(const pddp_problem& p, ClosedLoopLaunch<T> w,
                              hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  dim3 blocks;
  const int threads = closed_loop_geometry(w.a, blocks);
#define PDDP_ROLLOUT(KERNEL, ...) \
  PDDP_LAUNCH(KERNEL, blocks, dim3(threads), 0, st, P, w.a, __VA_ARGS__)
#define PDDP_DRAWING(PROC, OBS)                                                \
  do {                                                                         \
    if (w.r.ref != nullptr)                                                    \
      PDDP_ROLLOUT((closed_loop_track_kernel<T, MODEL, PROC, OBS>), w.noise,   \
                   w.r, w.Z, w.U, w.gains);                                    \
    else                                                                       \
      PDDP_ROLLOUT((closed_loop_noisy_kernel<T, MODEL, PROC, OBS>), w.noise,   \
                   w.Z, w.U, w.gains);                                         \
  } while (0)
  if (w.noise.w_std != nullptr && w.noise.v_std != nullptr)
    PDDP_DRAWING(true, true);
  else if (w.noise.w_std != nullptr)
    PDDP_DRAWING(true, false);
  else if (w.noise.v_std != nullptr)
    PDDP_DRAWING(false, true);
  else if (w.r.ref != nullptr)
    PDDP_ROLLOUT((closed_loop_track_kernel<T, MODEL, false, false>), w.noise,
                 w.r, w.Z, w.U, w.gains);
  else  // (no noise, one goal: the kernel without either argument)
    PDDP_ROLLOUT((closed_loop_kernel<T, MODEL>), w.Z, w.U, w.gains);
#undef PDDP_DRAWING
#undef PDDP_ROLLOUT
  return launch_status();
}

// (what an entry point refuses on its own account it refuses ahead of this)
template <typename T>
static int closed_loop_impl(const pddp_problem* p, ClosedLoopLaunch<T> w,
                            void* stream) {
  if (!args_ok(w.a, w.Z, w.U)) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_closed_loop, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int draws_impl(int B, int N, int S, int n, int which, uint64_t seed,
                      uint64_t sample_offset, T* W, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || n <= 0 || n > PDDP_MAX_STATE ||
      (which != 0 && which != 1) || !W)
    return PDDP_E_BADARG;
  const size_t total = (size_t)B * N * S;
  const size_t want = (total + kClosedLoopThreads - 1) / kClosedLoopThreads;
  const size_t cap = (size_t)1 << 20;  // (the kernel strides over the rest)
  const dim3 blocks((unsigned)(want < cap ? want : cap));
  PDDP_LAUNCH((closed_loop_draws_kernel<T>), blocks,
              dim3(kClosedLoopThreads), 0, (hipStream_t)stream,
              (DrawArgs<T>{B, N, S, n, which, seed, sample_offset, W}));
  return launch_status();
}

}  // namespace pddp

extern "C" {

// (the rollouts' common parameters, and the argument block made of them)
#define PDDP_ROLLOUT_PARAMS(T)                                                 \
  int B, int N, int S, const T* Z, const T* U, const T* gains, const T* z0s,   \
      const T* plant, const T* u_min, const T* u_max
#define PDDP_NOISE_PARAMS(T) \
  const T* w_std, const T* v_std, uint64_t seed, uint64_t sample_offset
#define PDDP_OUTPUT_PARAMS(T) \
  const uint8_t* active, T* Xc, T* Uc, T* Jc, T* stats, void* stream
#define PDDP_ROLLOUT_ARGS \
  {B, N, S, 0, z0s, plant, u_min, u_max, active, Xc, Uc, Jc, stats}
#define PDDP_NOISE_ARGS {w_std, v_std, seed, sample_offset}

#define PDDP_CLOSED_LOOP_ENTRY_POINTS(SUF, T)                                  \
  int pddp_closed_loop_##SUF(const pddp_problem* p, PDDP_ROLLOUT_PARAMS(T),    \
                             PDDP_OUTPUT_PARAMS(T)) {                          \
    return pddp::closed_loop_impl<T>(                                          \
        p, {PDDP_ROLLOUT_ARGS, {}, {}, Z, U, gains}, stream);                  \
  }                                                                            \
  int pddp_closed_loop_noisy_##SUF(                                            \
      const pddp_problem* p, PDDP_ROLLOUT_PARAMS(T), PDDP_NOISE_PARAMS(T),     \
      PDDP_OUTPUT_PARAMS(T)) {                                                 \
    /* (no noise at all is pddp_closed_loop_*'s launch) */                     \
    if (w_std == nullptr && v_std == nullptr) return PDDP_E_BADARG;            \
    return pddp::closed_loop_impl<T>(                                          \
        p, {PDDP_ROLLOUT_ARGS, PDDP_NOISE_ARGS, {}, Z, U, gains}, stream);     \
  }                                                                            \
  int pddp_closed_loop_track_##SUF(                                            \
      const pddp_problem* p, const T* ref, int ref_len, int ref_t0,            \
      PDDP_ROLLOUT_PARAMS(T), PDDP_NOISE_PARAMS(T), PDDP_OUTPUT_PARAMS(T)) {   \
    pddp::ClosedLoopLaunch<T> w{PDDP_ROLLOUT_ARGS, PDDP_NOISE_ARGS, {},        \
                                Z, U, gains};                                  \
    if (!pddp::ref_args<T>(nullptr, ref, ref_len, ref_t0, &w.r))               \
      return PDDP_E_BADARG;                                                    \
    return pddp::closed_loop_impl<T>(p, w, stream);                            \
  }                                                                            \
  int pddp_closed_loop_draws_##SUF(int B, int N, int S, int n, int which,      \
                                   uint64_t seed, uint64_t sample_offset,      \
                                   T* W, void* stream) {                       \
    return pddp::draws_impl<T>(B, N, S, n, which, seed, sample_offset, W,      \
                               stream);                                        \
  }

PDDP_CLOSED_LOOP_ENTRY_POINTS(f32, float)
PDDP_CLOSED_LOOP_ENTRY_POINTS(f64, double)
#undef PDDP_CLOSED_LOOP_ENTRY_POINTS
#undef PDDP_NOISE_ARGS
#undef PDDP_ROLLOUT_ARGS
#undef PDDP_OUTPUT_PARAMS
#undef PDDP_NOISE_PARAMS
#undef PDDP_ROLLOUT_PARAMS

}  // extern "C"
