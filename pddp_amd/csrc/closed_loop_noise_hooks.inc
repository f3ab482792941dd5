// closed_loop_noise_hooks.inc - closed_loop_body.inc's five noise hooks with
// the draws of closed_loop_draws.hpp at them: the text closed_loop_noisy_kernel
// and closed_loop_track_kernel (closed_loop.hip) define ahead of the body and
// undefine behind it.  The including kernel has
// `noise` (NoiseArgs) and the compile-time flags PROC / OBS: which streams the
// launch draws (DESIGN.md 3.4g).
#define PDDP_NOISE_LEVELS /* (the launch's: scalar registers) */               \
  T wstd[n], vstd[n];                                                          \
  _Pragma("unroll") for (int j = 0; j < n; ++j) {                              \
    wstd[j] = PROC ? noise.w_std[j] : T(0);                                    \
    vstd[j] = OBS ? noise.v_std[j] : T(0);                                     \
  }
#define PDDP_NOISE_OF_ROLLOUT                                                  \
  const uint64_t roll = noise.offset + (uint64_t)bs;                           \
  T v[n]; /* v_std (.) v_t of the coming step */                               \
  if (OBS) draw_scaled<T, n>(noise.seed, roll, 0, 1, vstd, v);
#define PDDP_NOISE_OF_STEP                                                     \
  T y[n], w[n];                                                                \
  _Pragma("unroll") for (int j = 0; j < n; ++j) y[j] = OBS ? z[j] + v[j]       \
                                                           : z[j];             \
  if (PROC) draw_scaled<T, n>(noise.seed, roll, t, 0, wstd, w);                \
  if (OBS) draw_scaled<T, n>(noise.seed, roll, t + 1, 1, vstd, v);
#define PDDP_SEEN(c) y[c]
#define PDDP_NEXT(j) (PROC ? zn[j] + w[j] : zn[j])
