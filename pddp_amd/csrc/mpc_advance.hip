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
// A translation unit of its own (csrc/Makefile: FLAGS_mpc_advance).  The
// kernel's loop is an included text, mpc_advance_body.inc, which tracking.hip
// includes too with a goal per time step; the row writers are
// model_params.hpp's.
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"

namespace pddp {

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

// Mapping: one lane per trajectory, as nominal_rollout_kernel; everything of
// trajectory b is read and written by its lane alone, J in t order, no
// atomics.  The shards of n_live belong to no trajectory: the first workgroup
// zeroes them (the rounds before and after this launch are stream-ordered
// around it).
template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void mpc_advance_kernel(
    ProblemT<T> shared, MpcAdvanceArgs<T> a) {
#define PDDP_PROBLEM_OF_B                                                      \
  ProblemT<T> P = shared;                                                      \
  if (a.table != nullptr)                                                      \
    write_params_and_goals<T, MODEL>(P, a.table + (size_t)b * PDDP_BATCH_ROW);
#define PDDP_PLANT_OF_B                                                        \
  ProblemT<T> Pl = P;                                                          \
  if (a.plant != nullptr)                                                      \
    write_params_and_goals<T, MODEL>(Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);
#define PDDP_TERMINAL_GOALS
// (no noise: z0 is the plant's state and the controller's)
#define PDDP_PLANT_STATE
#define PDDP_PLANT_STEPPED
#define PDDP_NOMINAL_START
#include "mpc_advance_body.inc"
#undef PDDP_NOMINAL_START
#undef PDDP_PLANT_STEPPED
#undef PDDP_PLANT_STATE
#undef PDDP_TERMINAL_GOALS
#undef PDDP_PLANT_OF_B
#undef PDDP_PROBLEM_OF_B
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

#define PDDP_MPC_ADVANCE_ENTRY_POINT(SUF, T)                                   \
  int pddp_mpc_advance_##SUF(                                                  \
      const pddp_problem* p, const T* table, int B, int N, int TT, int t,      \
      T* z0, T* U, T* Z, const T* u_min, const T* u_max, const T* plant,       \
      const T* disturbance, const uint8_t* mask, T* Xlog, T* Ulog, T* Jcl,     \
      int32_t* state_log, uint8_t* live_log, double* mu, double* delta,        \
      int32_t* state, int32_t* iter, uint8_t* active, uint8_t* fresh,          \
      int32_t* n_live, void* stream) {                                         \
    return pddp::mpc_advance_impl<T>(                                          \
        p, table, B, N, TT, t, z0, U, Z, u_min, u_max, plant, disturbance,     \
        mask, Xlog, Ulog, Jcl, state_log, live_log, mu, delta, state, iter,    \
        active, fresh, n_live, stream);                                        \
  }

PDDP_MPC_ADVANCE_ENTRY_POINT(f32, float)
PDDP_MPC_ADVANCE_ENTRY_POINT(f64, double)
#undef PDDP_MPC_ADVANCE_ENTRY_POINT

}  // extern "C"
