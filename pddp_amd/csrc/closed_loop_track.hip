// closed_loop_track.hip - closed-loop policy evaluation ALONG A REFERENCE:
// pddp_closed_loop_*'s rollout (closed_loop.hip), with or without the noise of
// pddp_closed_loop_noisy_* (closed_loop_noise.hip), costed under a goal PER
// TIME STEP (the pddp_closed_loop_track_* entry points,
// ILQRSolver.closed_loop(track=True)).
//
//   `ref` [B][ref_len][PDDP_REF_ROW], tracking.hip's: rollout (b, s) takes the
//   stage cost of step t under row min(ref_t0 + t, ref_len - 1) of trajectory
//   b and the terminal cost under row min(ref_t0 + N, ref_len - 1), x_goal
//   only.  The S rollouts of a trajectory share its reference; the plant row
//   supplies the model PARAMETERS only, its goal fields are not read.
//
// Dynamics, the feedback law, the clamp, the draws, the outputs and the
// statistics read no goal: they are the siblings', because the kernel is their
// text, closed_loop_body.inc, with the draws at its noise hooks and the goals
// of `P` taken from a reference row at its goal hooks.
//
// A translation unit of its own (csrc/Makefile: FLAGS_closed_loop_track).
#include <limits>
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"
#include "ref_args.hpp"

namespace pddp {

// K words of a reference row copied to `dst` (tracking.hip's statement: a
// statement, not a function, for its reason).
#define PDDP_COPY(K, dst, src) \
  _Pragma("unroll") for (int i = 0; i < (K); ++i)(dst)[i] = (src)[i];

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

#undef PDDP_COPY

template <typename T>
struct TrackedLaunch {
  ClosedLoopArgs<T> a;
  NoiseArgs<T> noise;
  RefArgs<T> r;
  const T* Z;
  const T* U;
  const T* gains;
};

template <typename T, int MODEL>
static int launch_tracked(const pddp_problem& p, TrackedLaunch<T> w,
                          hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  dim3 blocks;
  const int threads = closed_loop_geometry(w.a, blocks);
#define PDDP_TRACKED(PROC, OBS)                                                \
  PDDP_LAUNCH((closed_loop_track_kernel<T, MODEL, PROC, OBS>), blocks,         \
              dim3(threads), 0, st, P, w.a, w.noise, w.r, w.Z, w.U, w.gains)
  if (w.noise.w_std != nullptr && w.noise.v_std != nullptr)
    PDDP_TRACKED(true, true);
  else if (w.noise.w_std != nullptr)
    PDDP_TRACKED(true, false);
  else if (w.noise.v_std != nullptr)
    PDDP_TRACKED(false, true);
  else
    PDDP_TRACKED(false, false);
#undef PDDP_TRACKED
  return launch_status();
}

template <typename T>
static int tracked_impl(const pddp_problem* p, const T* ref, int ref_len,
                        int ref_t0, int B, int N, int S, const T* Z,
                        const T* U, const T* gains, const T* z0s,
                        const T* plant, const T* u_min, const T* u_max,
                        const T* w_std, const T* v_std, uint64_t seed,
                        uint64_t sample_offset, const uint8_t* active, T* Xc,
                        T* Uc, T* Jc, T* stats, void* stream) {
  TrackedLaunch<T> w{{B, N, S, 0, z0s, plant, u_min, u_max, active, Xc, Uc, Jc,
                      stats},
                     {w_std, v_std, seed, sample_offset},
                     {},
                     Z, U, gains};
  if (B <= 0 || N <= 0 || S <= 0 || !Z || !U || !Jc ||
      (Xc == nullptr) != (Uc == nullptr) ||
      !ref_args<T>(nullptr, ref, ref_len, ref_t0, &w.r))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_tracked, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_CLOSED_LOOP_TRACK(SUF, T)                                         \
  int pddp_closed_loop_track_##SUF(                                            \
      const pddp_problem* p, const T* ref, int ref_len, int ref_t0, int B,     \
      int N, int S, const T* Z, const T* U, const T* gains, const T* z0s,      \
      const T* plant, const T* u_min, const T* u_max, const T* w_std,          \
      const T* v_std, uint64_t seed, uint64_t sample_offset,                   \
      const uint8_t* active, T* Xc, T* Uc, T* Jc, T* stats, void* stream) {    \
    return pddp::tracked_impl<T>(p, ref, ref_len, ref_t0, B, N, S, Z, U,       \
                                 gains, z0s, plant, u_min, u_max, w_std,       \
                                 v_std, seed, sample_offset, active, Xc, Uc,   \
                                 Jc, stats, stream);                           \
  }

PDDP_CLOSED_LOOP_TRACK(f32, float)
PDDP_CLOSED_LOOP_TRACK(f64, double)
#undef PDDP_CLOSED_LOOP_TRACK

}  // extern "C"
