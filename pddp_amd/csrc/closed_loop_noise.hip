// closed_loop_noise.hip - closed-loop policy evaluation under process and
// measurement noise drawn on the device: pddp_closed_loop_*'s rollout
// (closed_loop.hip) with
//
//   y   = x_t + v_std (.) v_t              the controller sees a noisy state
//   x_{t+1} = plant(x_t, u_t) + w_std (.) w_t
//
// where v_t and w_t are n unit normals each, a pure function of (seed,
// rollout, step, stream, component): Philox4x32-10 on a counter, Box-Muller on
// its words.  No noise tensor exists; pddp_closed_loop_draws_* writes out the
// same normals (through the same device function) for tests and replays.
//
// A translation unit of its own (csrc/Makefile: FLAGS_closed_loop_noise).  The
// rollout kernel is closed_loop_kernel's text, closed_loop_body.inc, included
// with the draws at its hooks: mapping, output layout, the uniform `keep`
// branch, the statistics and their order are that kernel's.
#include <limits>
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"

namespace pddp {

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

// ---- the rollout -----------------------------------------------------------

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

template <typename T>
struct NoisyLaunch {
  ClosedLoopArgs<T> a;
  NoiseArgs<T> noise;
  const T* Z;
  const T* U;
  const T* gains;
};

template <typename T, int MODEL>
static int launch_noisy(const pddp_problem& p, NoisyLaunch<T> w,
                        hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  dim3 blocks;
  const int threads = closed_loop_geometry(w.a, blocks);
  if (w.noise.w_std != nullptr && w.noise.v_std != nullptr)
    PDDP_LAUNCH((closed_loop_noisy_kernel<T, MODEL, true, true>), blocks,
                dim3(threads), 0, st, P, w.a, w.noise, w.Z, w.U, w.gains);
  else if (w.noise.w_std != nullptr)
    PDDP_LAUNCH((closed_loop_noisy_kernel<T, MODEL, true, false>), blocks,
                dim3(threads), 0, st, P, w.a, w.noise, w.Z, w.U, w.gains);
  else
    PDDP_LAUNCH((closed_loop_noisy_kernel<T, MODEL, false, true>), blocks,
                dim3(threads), 0, st, P, w.a, w.noise, w.Z, w.U, w.gains);
  return launch_status();
}

template <typename T>
static int noisy_impl(const pddp_problem* p, int B, int N, int S, const T* Z,
                      const T* U, const T* gains, const T* z0s, const T* plant,
                      const T* u_min, const T* u_max, const T* w_std,
                      const T* v_std, uint64_t seed, uint64_t sample_offset,
                      const uint8_t* active, T* Xc, T* Uc, T* Jc, T* stats,
                      void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || !Z || !U || !Jc ||
      (Xc == nullptr) != (Uc == nullptr))
    return PDDP_E_BADARG;
  // (no noise at all is pddp_closed_loop_*'s launch)
  if (w_std == nullptr && v_std == nullptr) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  NoisyLaunch<T> w{{B, N, S, 0, z0s, plant, u_min, u_max, active, Xc, Uc, Jc,
                    stats},
                   {w_std, v_std, seed, sample_offset},
                   Z, U, gains};
  PDDP_DISPATCH_MODEL(launch_noisy, T, p, w, (hipStream_t)stream)
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

int pddp_closed_loop_noisy_f32(const pddp_problem* p, int B, int N, int S,
                               const float* Z, const float* U,
                               const float* gains, const float* z0s,
                               const float* plant, const float* u_min,
                               const float* u_max, const float* w_std,
                               const float* v_std, uint64_t seed,
                               uint64_t sample_offset, const uint8_t* active,
                               float* Xc, float* Uc, float* Jc, float* stats,
                               void* stream) {
  return pddp::noisy_impl<float>(p, B, N, S, Z, U, gains, z0s, plant, u_min,
                                 u_max, w_std, v_std, seed, sample_offset,
                                 active, Xc, Uc, Jc, stats, stream);
}
int pddp_closed_loop_noisy_f64(const pddp_problem* p, int B, int N, int S,
                               const double* Z, const double* U,
                               const double* gains, const double* z0s,
                               const double* plant, const double* u_min,
                               const double* u_max, const double* w_std,
                               const double* v_std, uint64_t seed,
                               uint64_t sample_offset, const uint8_t* active,
                               double* Xc, double* Uc, double* Jc,
                               double* stats, void* stream) {
  return pddp::noisy_impl<double>(p, B, N, S, Z, U, gains, z0s, plant, u_min,
                                  u_max, w_std, v_std, seed, sample_offset,
                                  active, Xc, Uc, Jc, stats, stream);
}
int pddp_closed_loop_draws_f32(int B, int N, int S, int n, int which,
                               uint64_t seed, uint64_t sample_offset, float* W,
                               void* stream) {
  return pddp::draws_impl<float>(B, N, S, n, which, seed, sample_offset, W,
                                 stream);
}
int pddp_closed_loop_draws_f64(int B, int N, int S, int n, int which,
                               uint64_t seed, uint64_t sample_offset,
                               double* W, void* stream) {
  return pddp::draws_impl<double>(B, N, S, n, which, seed, sample_offset, W,
                                  stream);
}

}  // extern "C"
