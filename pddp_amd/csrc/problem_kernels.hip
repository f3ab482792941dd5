// problem_kernels.hip - kernels that evaluate the sample problems' dynamics and
// cost: nominal rollout, derivative records, and the batched line search.
//
//   nominal rollout   pddp/controllers/ilqr.py:457-468   (sequential in t)
//   derivative records ilqr.py:464-473 via analytic Jacobians / Hessians
//                      (parallel over trajectory AND time step)
//   line search       ilqr.py:677-723 _control_law + :764-791 _trajectory_cost
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "goal_form.hpp"
#include "goal_kernels.hpp"  // (_track, _weighted, _track_weighted)
#include "accept.hpp"
#include "riccati_n4.hpp"  // DPP helpers of the 16-lane groups
#include "line_search_lds.hpp"

namespace pddp {

// Each operation's loop is written ONCE, as a text (*_body.inc) that the
// kernels of the two forms include: the uniform kernels read the problem from
// their kernel argument `P`; the batch_* kernels (a problem PER TRAJECTORY: the
// pddp_*_batch_* entry points, ILQRSolver.set_batch_problem) declare `P` at
// PDDP_PROBLEM_OF_B as the shared problem with row b of `table`
// [B][PDDP_BATCH_ROW] written over it (include/pddp_hip.h: params, x_goal,
// u_goal).  The __global__ functions are that and nothing else; launchers,
// argument checks and the dispatch on the model are shared too.  The records'
// and the search's texts are goal_kernels.hpp's as well (a goal PER TIME STEP,
// per-trajectory cost weights, both): at their PDDP_GOALS(point) the tracked
// kernels write a reference row's goals over P's; here the hook is empty.
//
// An included text and not a device function: as a forceinline function
// <T, MODEL> (arguments by value or by reference, the problem handed in or
// asked for through a callable - all were built) the same statements reach the
// optimiser with some commutative operands the other way round, `a * b + c * d`
// is then contracted into the other FMA, and rollouts, records and candidates
// differ from the separate kernels' in their last bits
// (tests/test_problem_kernels_golden.py).  Included, every kernel is the
// instruction sequence it was.
//
// Q, Q_term, R, the model, the encoding and the action bounds stay those of the
// pddp_problem passed by value.  The row is read ONCE ahead of the time loop,
// by each lane (rollout, line search) or workgroup (records); the overwritten
// fields live in vector registers from then on (27 words for the double
// cartpole, 12 for the cartpole); Q, Qt and R are never written and stay scalar
// operands of the kernel argument.
//
// The backward sweep and the accept kernel never see the problem, so a round
// with a table is derivs(batch), backward, line_search(batch), accept.

// The shared problem with trajectory b's row written over it
// (write_params_and_goals: model_params.hpp).  Returned by value into a const
// `P`: with the two statements in the kernels' own scope the batch records and
// searches come out as other instructions.
template <typename T, int MODEL>
PDDP_DEV ProblemT<T> problem_of_row(const ProblemT<T>& shared, const T* table,
                                    int b) {
  ProblemT<T> P = shared;
  write_params_and_goals<T, MODEL>(P, table + (size_t)b * PDDP_BATCH_ROW);
  return P;
}

// --------------------------------------------------------------------------
// nominal rollout: one lane per trajectory (rollout_body.inc)
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void nominal_rollout_kernel(
    ProblemT<T> P, RolloutArgs<T> a) {
#define PDDP_PROBLEM_OF_B
#include "rollout_body.inc"
#undef PDDP_PROBLEM_OF_B
}

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void batch_rollout_kernel(
    ProblemT<T> shared, RolloutArgs<T> a, const T* table) {
#define PDDP_PROBLEM_OF_B const ProblemT<T> P = problem_of_row<T, MODEL>(shared, table, b);
#include "rollout_body.inc"
#undef PDDP_PROBLEM_OF_B
}

// --------------------------------------------------------------------------
// derivative records: one workgroup per trajectory (the row index is the
// workgroup's), one lane per time step; records are staged through LDS so the
// HBM writes are fully coalesced (derivs_body.inc).
// --------------------------------------------------------------------------
// (group_copy, store4: line_search_lds.hpp)
// (record_of: models.hpp)

// (kDerivThreads: problem_args.hpp)

template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void derivs_kernel(
    ProblemT<T> P, DerivArgs<T> a) {
#define PDDP_PROBLEM_OF_B
#define PDDP_SPLIT_TERMINAL 0
#define PDDP_GOALS(point)
#include "derivs_body.inc"
#undef PDDP_GOALS
#undef PDDP_SPLIT_TERMINAL
#undef PDDP_PROBLEM_OF_B
}

// `terminal` as a constant in each call of record_of: the cost picks its
// matrix by `terminal ? P.Qt : P.Q`, and a run-time choice between two members
// of this per-workgroup COPY would put the whole copy into scratch memory
// (1344 B in f64, 680 B in f32).  The uniform kernel indexes the kernel
// argument itself and keeps the run-time flag: its code object is the one it
// was before the two forms shared their text.
template <typename T, int MODEL>
__global__ __launch_bounds__(kDerivThreads) void batch_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, const T* table) {
#define PDDP_PROBLEM_OF_B const ProblemT<T> P = problem_of_row<T, MODEL>(shared, table, b);
#define PDDP_SPLIT_TERMINAL 1
#define PDDP_GOALS(point)
#include "derivs_body.inc"
#undef PDDP_GOALS
#undef PDDP_SPLIT_TERMINAL
#undef PDDP_PROBLEM_OF_B
}

// --------------------------------------------------------------------------
// line search: one lane per (trajectory, alpha) candidate, any A; the next
// step's nominal row and gains are requested ahead of the dependent chain
// (with a table, the lanes of a trajectory read the same row: one broadcast
// read each ahead of the loop) (line_search_body.inc)
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void line_search_kernel(
    ProblemT<T> P, LineSearchArgs<T> a) {
#define PDDP_PROBLEM_OF_B
#define PDDP_GOALS(point)
#include "line_search_body.inc"
#undef PDDP_GOALS
#undef PDDP_PROBLEM_OF_B
}

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void batch_line_search_kernel(
    ProblemT<T> shared, LineSearchArgs<T> a, const T* table) {
#define PDDP_PROBLEM_OF_B const ProblemT<T> P = problem_of_row<T, MODEL>(shared, table, b);
#define PDDP_GOALS(point)
#include "line_search_body.inc"
#undef PDDP_GOALS
#undef PDDP_PROBLEM_OF_B
}

// --------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------
// (kSparseMask, models.hpp: a cost matrix with entries outside it runs the
// full form; for a model without a sparse instantiation the dispatch below
// folds to one launch)
template <int MODEL, unsigned QM>
static bool stage_cost_on(const pddp_problem& p) {
  if (QM == kFullMask<MODEL>) return false;
  return (live_mask(p.Q, ModelDims<MODEL>::na) & ~QM) == 0;
}
// (With<Args, const T*>, problem_args.hpp: an argument block and the
// per-trajectory table of the batch entry points, nullptr from the uniform
// ones)
template <typename T, int MODEL>
static int launch_rollout(const pddp_problem& p,
                          With<RolloutArgs<T>, const T*> w, hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const dim3 blocks((w.a.B + kWave - 1) / kWave);
  if (w.x != nullptr)
    PDDP_LAUNCH((batch_rollout_kernel<T, MODEL>), blocks, dim3(kWave), 0, st,
                P, w.a, w.x);
  else
    PDDP_LAUNCH((nominal_rollout_kernel<T, MODEL>), blocks, dim3(kWave), 0, st,
                P, w.a);
  return launch_status();
}
// The records and the line search in their five forms: the kernel by what the
// form brought (FormGoals, goal_form.hpp) - a reference, weights, both, the
// table alone, nothing.
template <typename T, int MODEL>
static int launch_derivs(const pddp_problem& p,
                         With<DerivArgs<T>, FormGoals<T>> w, hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const RefArgs<T>& g = w.x.goals;
  const T* weights = w.x.weights;
  const dim3 grid(w.a.B), block(kDerivThreads);
  if (g.ref != nullptr && weights != nullptr)
    PDDP_LAUNCH((track_weighted_derivs_kernel<T, MODEL>), grid, block, 0, st,
                P, w.a, g, weights);
  else if (g.ref != nullptr)
    PDDP_LAUNCH((track_derivs_kernel<T, MODEL>), grid, block, 0, st, P, w.a,
                g);
  else if (weights != nullptr)
    PDDP_LAUNCH((weighted_derivs_kernel<T, MODEL>), grid, block, 0, st, P,
                w.a, (WeightArgs<T>{g.table, weights}));
  else if (g.table != nullptr)
    PDDP_LAUNCH((batch_derivs_kernel<T, MODEL>), grid, block, 0, st, P, w.a,
                g.table);
  else
    PDDP_LAUNCH((derivs_kernel<T, MODEL>), grid, block, 0, st, P, w.a);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_line_search(const pddp_problem& p,
                              With<LineSearchArgs<T>, FormGoals<T>> w,
                              hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const LineSearchArgs<T>& a = w.a;
  const RefArgs<T>& g = w.x.goals;
  const T* weights = w.x.weights;
  const dim3 lanes = search_lanes(a);
  if (g.ref != nullptr || weights != nullptr || g.table != nullptr) {
    // (the LDS kernels take one problem)
    if (g.ref != nullptr && weights != nullptr)
      PDDP_LAUNCH((track_weighted_line_search_kernel<T, MODEL>), lanes,
                  dim3(kWave), 0, st, P, a, g, weights);
    else if (g.ref != nullptr)
      PDDP_LAUNCH((track_line_search_kernel<T, MODEL>), lanes, dim3(kWave), 0,
                  st, P, a, g);
    else if (weights != nullptr)
      PDDP_LAUNCH((weighted_line_search_kernel<T, MODEL>), lanes, dim3(kWave),
                  0, st, P, a, (WeightArgs<T>{g.table, weights}));
    else
      PDDP_LAUNCH((batch_line_search_kernel<T, MODEL>), lanes, dim3(kWave), 0,
                  st, P, a, g.table);
    return launch_status();
  }
  using D = ModelDims<MODEL>;
  const size_t per = (size_t)(a.N + 1) * D::n + (size_t)a.N * D::m +
                     (size_t)a.N * (D::m + D::m * D::n);
  const size_t lds = 4 * per * sizeof(T);
  if (a.A <= 16 && lds <= 64 * 1024) {  // nominal data staged in LDS
    if (4 * lds <= 64 * 1024) {
      if (stage_cost_on<MODEL, kSparseMask<MODEL>>(p))
        PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, false, 4, 1,
                                            kSparseMask<MODEL>>),
                           dim3((a.B + 15) / 16), dim3(kWave * 4), 4 * lds, st,
                           P, a, AcceptArgs<T>{}, (T*)nullptr, (T*)nullptr);
      else
        PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, false, 4>),
                           dim3((a.B + 15) / 16), dim3(kWave * 4), 4 * lds, st,
                           P, a, AcceptArgs<T>{}, (T*)nullptr, (T*)nullptr);
    } else
      PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, false, 1>),
                         dim3((a.B + 3) / 4), dim3(kWave), lds, st, P, a,
                         AcceptArgs<T>{}, (T*)nullptr, (T*)nullptr);
    return launch_status();
  }
  PDDP_LAUNCH((line_search_kernel<T, MODEL>), lanes, dim3(kWave), 0, st, P,
              a);
  return launch_status();
}

// fused line search + accept + derivative records; PDDP_E_UNSUPPORTED when the
// LDS kernel does not apply (more than 16 step sizes, nominal data > 64 KB)
template <typename T>
struct SearchAcceptArgs {
  LineSearchArgs<T> ls;
  AcceptArgs<T> ac;
  T* rec;
  T* L;
};
// 0 auto (by batch), 1 the paired form always, 2 the dense form where built
inline int& search_form_choice() {
  static int choice = 0;
  return choice;
}
template <typename T, int MODEL>
static int launch_search_accept(const pddp_problem& p, SearchAcceptArgs<T> a,
                                hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  using D = ModelDims<MODEL>;
  const size_t per = (size_t)(a.ls.N + 1) * D::n + (size_t)a.ls.N * D::m +
                     (size_t)a.ls.N * (D::m + D::m * D::n);
  const size_t lds = 4 * per * sizeof(T);
  if (a.ls.A > 16 || lds > 64 * 1024) return PDDP_E_UNSUPPORTED;
  a.ac.n = D::n;
  a.ac.m = D::m;
  if constexpr (sizeof(T) == 4 && D::n <= 4) {
    // the dense form (see the kernel): from the batch on that the paired
    // form's two workgroups per CU no longer hold at once
    const int mode = search_form_choice();
    const size_t lds_dense =
        16 * (size_t)a.ls.N * (D::m + D::m * D::n) * sizeof(T);
    // (measured, tools/dbg/search_form_scan.py: 100.5 -> 90.7 us at 12288
    // trajectories, 117.8 -> 105.5 at 16384, 206.7 -> 192.1 at 32768; slower
    // at 8192 and below - 50.5 -> 60.3 - and at 65536 - 406 -> 483)
    const bool dense =
        mode == 2 || (mode == 0 && a.ls.B > 8192 && a.ls.B <= 49152);
    if (dense && 4 * lds <= 64 * 1024 && lds_dense <= 40 * 1024 &&
        a.ls.N + 1 <= 128) {
      if (stage_cost_on<MODEL, kSparseMask<MODEL>>(p))
        PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, true, 4, 1,
                                            kSparseMask<MODEL>, true>),
                    dim3((a.ls.B + 15) / 16), dim3(kWave * 4), lds_dense, st,
                    P, a.ls, a.ac, a.rec, a.L);
      else
        PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, true, 4, 1,
                                            kFullMask<MODEL>, true>),
                    dim3((a.ls.B + 15) / 16), dim3(kWave * 4), lds_dense, st,
                    P, a.ls, a.ac, a.rec, a.L);
      return launch_status();
    }
  }
  if (4 * lds <= 64 * 1024) {
    // four rollout waves (one per SIMD of a CU) + their four helpers
    if (stage_cost_on<MODEL, kSparseMask<MODEL>>(p))
      PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, true, 4, 2,
                                          kSparseMask<MODEL>>),
                         dim3((a.ls.B + 15) / 16), dim3(kWave * 8), 4 * lds, st,
                         P, a.ls, a.ac, a.rec, a.L);
    else
      PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, true, 4, 2>),
                         dim3((a.ls.B + 15) / 16), dim3(kWave * 8), 4 * lds, st,
                         P, a.ls, a.ac, a.rec, a.L);
  } else
    PDDP_LAUNCH((line_search_lds_kernel<T, MODEL, true, 1>),
                       dim3((a.ls.B + 3) / 4), dim3(kWave), lds, st, P, a.ls,
                       a.ac, a.rec, a.L);
  return launch_status();
}

// default_kernels.hip: the same three operations under the DEFAULT (upper-
// triangular Cholesky) encoding, selected by pddp_problem.encoding
template <typename T>
int default_rollout(const pddp_problem& p, RolloutArgs<T> a, hipStream_t st);
template <typename T>
int default_derivs(const pddp_problem& p, DerivArgs<T> a, hipStream_t st);
template <typename T>
int default_line_search(const pddp_problem& p, LineSearchArgs<T> a,
                        hipStream_t st);
static bool is_default_encoding(const pddp_problem* p) {
  return p != nullptr && (p->encoding == PDDP_ENC_UPPER_TRIANGULAR_CHOLESKY ||
                          p->encoding == PDDP_ENC_VARIANCE_ONLY ||
                          p->encoding == PDDP_ENC_STANDARD_DEVIATION_ONLY ||
                          p->encoding == PDDP_ENC_FULL_COVARIANCE_MATRIX);
}

// (check_problem, PDDP_DISPATCH_MODEL: problem_args.hpp)

// The nominal rollout in its two forms.  `batch`: pddp_nominal_rollout_batch_*
// - it needs its table and takes check_problem()'s domain only, the four
// sample models under IGNORE_UNCERTAINTY; the uniform one (table == nullptr)
// routes the Gaussian encodings to default_kernels.hip.
template <typename T>
static int nominal_rollout_impl(const pddp_problem* p, bool batch,
                                const T* table, int B, int N, const T* z0,
                                const T* U, const T* u_min, const T* u_max,
                                const uint8_t* mask, T* Z, void* stream) {
  if (B <= 0 || N <= 0 || (batch && !table) || !z0 || !U || !Z)
    return PDDP_E_BADARG;
  With<RolloutArgs<T>, const T*> w{{B, N, z0, U, u_min, u_max, mask, Z},
                                   table};
  if (!batch && is_default_encoding(p))
    return default_rollout<T>(*p, w.a, (hipStream_t)stream);
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_rollout, T, p, w, (hipStream_t)stream)
}

// What every form of an operation takes behind its leading arguments.
#define PDDP_DERIVS_PARAMS(T)                                                  \
  int B, int N, const T* Z, const T* U, const T* u_min, const T* u_max,        \
      const uint8_t* mask, T* rec, T* L, T* J, int32_t* state, void* stream
#define PDDP_DERIVS_ARGS \
  B, N, Z, U, u_min, u_max, mask, rec, L, J, state, stream
#define PDDP_SEARCH_PARAMS(T)                                                  \
  int B, int N, int A, const T* Z, const T* U, const T* gains,                 \
      const T* alphas, const T* u_min, const T* u_max, const uint8_t* active,  \
      const int32_t* bwd_status, T* Zc, T* Uc, T* Jc, void* stream
#define PDDP_SEARCH_ARGS                                                       \
  B, N, A, Z, U, gains, alphas, u_min, u_max, active, bwd_status, Zc, Uc, Jc,  \
      stream

// The records and the line search: one impl and one argument test for the five
// forms (goal_form.hpp).  The plain form alone (no suffix) routes the Gaussian
// encodings to default_kernels.hip, and alone does not hold B * A to an int.
template <typename T>
static bool is_plain(const GoalForm<T>& f) {
  return !f.batch && !f.goals;
}

template <typename T>
static int derivs_impl(const pddp_problem* p, const GoalForm<T>& f,
                       PDDP_DERIVS_PARAMS(T)) {
  With<DerivArgs<T>, FormGoals<T>> w{
      {B, N, Z, U, u_min, u_max, mask, rec, L, J, state}, {}};
  if (!args_ok(w.a) || !form_goals(f, &w.x)) return PDDP_E_BADARG;
  if (is_plain(f) && is_default_encoding(p))
    return default_derivs<T>(*p, w.a, (hipStream_t)stream);
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_derivs, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int line_search_impl(const pddp_problem* p, const GoalForm<T>& f,
                            PDDP_SEARCH_PARAMS(T)) {
  With<LineSearchArgs<T>, FormGoals<T>> w{
      {B, N, A, Z, U, gains, alphas, u_min, u_max, active, bwd_status, Zc, Uc,
       Jc},
      {}};
  if (!args_ok(w.a, !is_plain(f)) || !form_goals(f, &w.x))
    return PDDP_E_BADARG;
  if (is_plain(f) && is_default_encoding(p))
    return default_line_search<T>(*p, w.a, (hipStream_t)stream);
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_line_search, T, p, w, (hipStream_t)stream)
}

// 0 auto (by the size of the candidates), 1 keep them, 2 drop them
inline int& search_candidates_choice() {
  static int choice = 0;
  return choice;
}

template <typename T>
static int search_accept_impl(const pddp_problem* p, int B, int N, int A, T* Z,
                              T* U, const T* gains, const T* alphas,
                              const T* u_min, const T* u_max, uint8_t* active,
                              const int32_t* bwd_status, T* Zc, T* Uc, T* Jc,
                              double tol, double max_reg, int n_iterations,
                              T* gains_acc, T* J_opt, double* mu,
                              double* delta, int32_t* state, int32_t* iter,
                              uint8_t* fresh, int32_t* n_live, T* rec, T* L,
                              void* stream) {
  if (int rc = check_problem(p)) return rc;
  if (B <= 0 || N <= 0 || A <= 0 || !Z || !U || !gains || !alphas || !active ||
      !bwd_status || !Zc || !Uc || !Jc || !gains_acc || !J_opt || !mu ||
      !delta || !state || !iter || !fresh || (L != nullptr && !rec))
    return PDDP_E_BADARG;
  SearchAcceptArgs<T> a;
  a.ls = LineSearchArgs<T>{B, N, A, Z, U, gains, alphas, u_min, u_max, active,
                           bwd_status, Zc, Uc, Jc};
  a.ac = AcceptArgs<T>{B, N, 0, 0, A, Zc, Uc, Jc, gains, bwd_status, tol,
                       max_reg, n_iterations, Z, U, gains_acc, J_opt, mu, delta,
                       state, iter, active, fresh, n_live};
  a.rec = rec;
  a.L = L;
  // keep the candidates while they fit the Infinity Cache next to the rest of
  // the round's traffic (256 MB; a launch's candidates: 82 MB at B = 4096,
  // 164 MB at 8192: 50 us; 328 MB at 16384: 163 us kept, 97 us dropped)
  const double cand_bytes =
      (double)B * A * ((double)(N + 1) * p->encoded_size +
                       (double)N * p->action_size) * sizeof(T);
  const int mode = search_candidates_choice();
  a.ls.drop_candidates =
      (L == nullptr && rec != nullptr &&
       (mode == 2 || (mode == 0 && cand_bytes > 200e6))) ? 1 : 0;
  PDDP_DISPATCH_MODEL(launch_search_accept, T, p, a, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#ifdef PDDP_WG_TIMELINE
int pddp_debug_search_timeline(long long* out) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::g_search_timeline),
                      sizeof(long long) * 1024 * 12);
  return 0;
}
#endif

int pddp_search_form(int mode) {
  const int prev = pddp::search_form_choice();
  if (mode >= 0 && mode <= 2) pddp::search_form_choice() = mode;
  return prev;
}
int pddp_search_candidates(int mode) {
  const int prev = pddp::search_candidates_choice();
  if (mode >= 0 && mode <= 2) pddp::search_candidates_choice() = mode;
  return prev;
}

#define PDDP_PROBLEM_ENTRY_POINTS(SUF, T)                                      \
  int pddp_search_accept_##SUF(                                                \
      const pddp_problem* p, int B, int N, int A, T* Z, T* U, const T* gains,  \
      const T* alphas, const T* u_min, const T* u_max, uint8_t* active,        \
      const int32_t* bwd_status, T* Zc, T* Uc, T* Jc, double tol,              \
      double max_reg, int n_iterations, T* gains_acc, T* J_opt, double* mu,    \
      double* delta, int32_t* state, int32_t* iter, uint8_t* fresh,            \
      int32_t* n_live, T* rec, T* L, void* stream) {                           \
    return pddp::search_accept_impl<T>(                                        \
        p, B, N, A, Z, U, gains, alphas, u_min, u_max, active, bwd_status, Zc, \
        Uc, Jc, tol, max_reg, n_iterations, gains_acc, J_opt, mu, delta,       \
        state, iter, fresh, n_live, rec, L, stream);                           \
  }                                                                            \
  int pddp_nominal_rollout_##SUF(                                              \
      const pddp_problem* p, int B, int N, const T* z0, const T* U,            \
      const T* u_min, const T* u_max, const uint8_t* mask, T* Z,               \
      void* stream) {                                                          \
    return pddp::nominal_rollout_impl<T>(p, false, nullptr, B, N, z0, U,       \
                                         u_min, u_max, mask, Z, stream);       \
  }                                                                            \
  /* the same with a problem per trajectory: row b of `table` */               \
  int pddp_nominal_rollout_batch_##SUF(                                        \
      const pddp_problem* p, const T* table, int B, int N, const T* z0,        \
      const T* U, const T* u_min, const T* u_max, const uint8_t* mask, T* Z,   \
      void* stream) {                                                          \
    return pddp::nominal_rollout_impl<T>(p, true, table, B, N, z0, U, u_min,   \
                                         u_max, mask, Z, stream);              \
  }                                                                            \
  /* the records and the line search: five forms each (goal_form.hpp) */       \
  PDDP_FORM_ENTRY_POINTS(derivs, SUF, T, PDDP_DERIVS_PARAMS,                   \
                         PDDP_DERIVS_ARGS)                                     \
  PDDP_FORM_ENTRY_POINTS(line_search, SUF, T, PDDP_SEARCH_PARAMS,              \
                         PDDP_SEARCH_ARGS)

PDDP_PROBLEM_ENTRY_POINTS(f32, float)
PDDP_PROBLEM_ENTRY_POINTS(f64, double)
#undef PDDP_PROBLEM_ENTRY_POINTS

}  // extern "C"
