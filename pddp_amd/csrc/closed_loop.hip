// closed_loop.hip - closed-loop policy evaluation: S rollouts of every
// trajectory's time-varying feedback policy (Z, U, K), each from its own
// initial state on its own plant, and the statistics of a controller's costs.
//
//   the trial step of the outer loop   pddp/controllers/pddp.py:209-245
//                                      (_apply_controller, batched: the sample
//                                      models as the plant)
//   the feedback law                   ilqr.py:318-355 (forward, mpc=False)
//   the cost of a rollout              ilqr.py:764-791 (_trajectory_cost)
//
// A translation unit of its own (csrc/Makefile: FLAGS_closed_loop).  Its loop
// resembles the line search's but is its own text - the feedback law and the
// output layout differ; the parameter count is model_params.hpp's, the row
// writer stays written out at its one call site.  That text
// is closed_loop_body.inc: closed_loop_noise.hip includes it too, with noise
// drawn at its hooks, and closed_loop_track.hip with the goals
// of a reference row at its goal hooks as well (3.4h); here the hooks are empty.
#include <limits>
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_args.hpp"

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

template <typename T>
struct ClosedLoopLaunch {
  ClosedLoopArgs<T> a;
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
  PDDP_LAUNCH((closed_loop_kernel<T, MODEL>), blocks, dim3(threads), 0, st, P,
              w.a, w.Z, w.U, w.gains);
  return launch_status();
}

template <typename T>
static int closed_loop_impl(const pddp_problem* p, int B, int N, int S,
                            const T* Z, const T* U, const T* gains,
                            const T* z0s, const T* plant, const T* u_min,
                            const T* u_max, const uint8_t* active, T* Xc,
                            T* Uc, T* Jc, T* stats, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || !Z || !U || !Jc ||
      (Xc == nullptr) != (Uc == nullptr))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  ClosedLoopLaunch<T> w{{B, N, S, 0, z0s, plant, u_min, u_max, active, Xc, Uc,
                         Jc, stats},
                        Z, U, gains};
  PDDP_DISPATCH_MODEL(launch_closed_loop, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

int pddp_closed_loop_f32(const pddp_problem* p, int B, int N, int S,
                         const float* Z, const float* U, const float* gains,
                         const float* z0s, const float* plant,
                         const float* u_min, const float* u_max,
                         const uint8_t* active, float* Xc, float* Uc,
                         float* Jc, float* stats, void* stream) {
  return pddp::closed_loop_impl<float>(p, B, N, S, Z, U, gains, z0s, plant,
                                       u_min, u_max, active, Xc, Uc, Jc, stats,
                                       stream);
}
int pddp_closed_loop_f64(const pddp_problem* p, int B, int N, int S,
                         const double* Z, const double* U, const double* gains,
                         const double* z0s, const double* plant,
                         const double* u_min, const double* u_max,
                         const uint8_t* active, double* Xc, double* Uc,
                         double* Jc, double* stats, void* stream) {
  return pddp::closed_loop_impl<double>(p, B, N, S, Z, U, gains, z0s, plant,
                                        u_min, u_max, active, Xc, Uc, Jc,
                                        stats, stream);
}

}  // extern "C"
