// riccati_nominal.hip - the sweeps that evaluate their derivative records
// themselves, from the nominal trajectory (pddp_sweep_nominal_*: one
// implementation for both types): the n = 4 sweep of riccati_n4_elem.hpp
// (cartpole; launched as n4_nominal_plan says - f32 with the generator on
// partner wavefronts or inline, f64 inline) and the 16 x 16 matrix-core sweep
// of riccati_mfma16_nominal.hpp (pendulum, double cartpole); and
// pddp_n4_nominal_plan, the host-only query of that plan.  A translation unit
// of its own: no SLP pairing (the FMAs take DPP operands, riccati_quad.hip)
// and matrix-instruction results in ordinary VGPRs.
#include "riccati_n4_elem.hpp"
#include "riccati_mfma16_nominal.hpp"

namespace pddp {

template <typename T>
static int sweep_nominal(const pddp_problem* problem, int B, int N, const T* Z,
                         const T* U, const T* u_min, const T* u_max,
                         const double* reg, int branch, const uint8_t* active,
                         uint8_t* fresh, T* gains, int32_t* status, T* L,
                         T* J_opt, void* stream) {
  if (problem == nullptr || B <= 0 || N <= 0 || Z == nullptr || U == nullptr ||
      reg == nullptr || gains == nullptr || status == nullptr ||
      L == nullptr || J_opt == nullptr)
    return PDDP_E_BADARG;
  if (branch != PDDP_BRANCH_EIG && branch != PDDP_BRANCH_CHOLESKY)
    return PDDP_E_BADARG;
  const NominalArgs<T> sw =
      nominal_args<T>(*problem, B, N, Z, U, u_min, u_max, reg, branch, active,
                      fresh, gains, status, L, J_opt);
  // cartpole: riccati_n4_elem.hpp, launched as n4_nominal_plan says (f32: its
  // record generator inline, on wavefronts of its own, or - auto - by batch;
  // f64: inline)
  if (problem->model == PDDP_MODEL_CARTPOLE)
    return launch_n4_elem(*problem, sw.a, sw.gen, (hipStream_t)stream);
  // pendulum, double cartpole: the 16 x 16 matrix-core sweep with its
  // records generated in the wavefront (riccati_mfma16_nominal.hpp)
  return launch_m16_nominal<T>(*problem, sw.a, sw.gen, (hipStream_t)stream);
}

}  // namespace pddp

extern "C" int pddp_sweep_nominal_f32(const pddp_problem* problem, int B, int N,
                                      const float* Z, const float* U,
                                      const float* u_min, const float* u_max,
                                      const double* reg, int branch,
                                      const uint8_t* active, uint8_t* fresh,
                                      float* gains, int32_t* status, float* L,
                                      float* J_opt, void* stream) {
  return pddp::sweep_nominal<float>(problem, B, N, Z, U, u_min, u_max, reg,
                                    branch, active, fresh, gains, status, L,
                                    J_opt, stream);
}
extern "C" int pddp_sweep_nominal_f64(const pddp_problem* problem, int B, int N,
                                      const double* Z, const double* U,
                                      const double* u_min, const double* u_max,
                                      const double* reg, int branch,
                                      const uint8_t* active, uint8_t* fresh,
                                      double* gains, int32_t* status, double* L,
                                      double* J_opt, void* stream) {
  return pddp::sweep_nominal<double>(problem, B, N, Z, U, u_min, u_max, reg,
                                     branch, active, fresh, gains, status, L,
                                     J_opt, stream);
}

extern "C" int pddp_n4_nominal_plan(const pddp_problem* problem,
                                    int element_size, int B, int N, int A,
                                    int has_u_min, int has_u_max, int branch,
                                    int rounds, int kernel_choice,
                                    int32_t* plan) {
  const bool round = rounds != 0;
  if (problem == nullptr || plan == nullptr || B <= 0 || N <= 0 ||
      (round && A <= 0) || (element_size != 4 && element_size != 8))
    return PDDP_E_BADARG;
  if (branch != PDDP_BRANCH_EIG && branch != PDDP_BRANCH_CHOLESKY)
    return PDDP_E_BADARG;
  pddp::N4NominalPlan pl;
  if (const int rc = pddp::n4_nominal_plan(
          *problem, (size_t)element_size, round, B, N, A, has_u_min != 0,
          has_u_max != 0, branch, rounds, kernel_choice, pl))
    return rc;
  plan[PDDP_N4_PLAN_BRANCH] = pl.br;
  plan[PDDP_N4_PLAN_SPARSE] = pl.sparse;
  plan[PDDP_N4_PLAN_OVERLAP] = pl.ovl;
  plan[PDDP_N4_PLAN_MULTI] = pl.multi;
  plan[PDDP_N4_PLAN_CARRY] = pl.use_carry;
  plan[PDDP_N4_PLAN_GRID] = (int32_t)pl.grid;
  plan[PDDP_N4_PLAN_THREADS] = (int32_t)pl.threads;
  plan[PDDP_N4_PLAN_LDS] = (int32_t)pl.lds;
  return 0;
}

namespace pddp {
namespace n4e {
// elem_gains on `count` independent scalar problems, four per wavefront as in
// the sweep (pddp_boxqp_m1_lean_f32: the unit-test entry of the benched
// sweep's BoxQP).  x = k, free_mask = (K is not zeroed), status = PDDP_BWD_*.
__global__ __launch_bounds__(kWave) void elem_gains_kernel(
    int count, const float* x0, const float* Quu, const float* Qu,
    const float* reg, const float* lo, const float* hi, float* x,
    uint8_t* free_mask, int32_t* status_out, float* coeffs) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x * kTrajW + (lane >> 4);
  const bool exists = p < count;
  const int pc = exists ? p : count - 1;
  int status = PDDP_BWD_OK;
  unsigned long long alive_m = __ballot(exists);
  const ElemGains<float> g = elem_gains<float>(
      x0[pc], Quu[pc], Qu[pc], reg[pc], lo[pc], hi[pc], lane, status, alive_m);
  if (exists && (lane & 15) == 0) {
    x[p] = g.kt;
    free_mask[p] = g.sK != 0.0f ? 1 : 0;
    status_out[p] = status;
    if (coeffs != nullptr) {
      coeffs[3 * p] = g.sK;
      coeffs[3 * p + 1] = g.c;
      coeffs[3 * p + 2] = g.wv;
    }
  }
}

}  // namespace n4e
}  // namespace pddp

extern "C" int pddp_boxqp_m1_lean_f32(int count, const float* x0,
                                      const float* Quu, const float* Qu,
                                      const float* reg, const float* lower,
                                      const float* upper, float* x,
                                      uint8_t* free_mask, int32_t* status,
                                      float* coeffs, void* stream) {
  if (count <= 0 || !x0 || !Quu || !Qu || !reg || !lower || !upper || !x ||
      !free_mask || !status)
    return PDDP_E_BADARG;
  PDDP_LAUNCH(pddp::n4e::elem_gains_kernel,
              dim3((count + pddp::n4e::kTrajW - 1) / pddp::n4e::kTrajW),
              dim3(pddp::kWave), 0, (hipStream_t)stream, count, x0, Quu, Qu,
              reg, lower, upper, x, free_mask, status, coeffs);
  return pddp::launch_status();
}

extern "C" int pddp_sweep_nominal_kernel(int which) {
  const int prev = pddp::nominal_kernel_choice();
  if (which == 0 || which == 3 || which == 4)
    pddp::nominal_kernel_choice() = which;
  return prev;
}

#ifdef PDDP_ELEM_MARKS
extern "C" int pddp_debug_elem_marks(long long* out) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::n4e::g_elem_marks), 64);
  long long z[8] = {};
  hipMemcpyToSymbol(HIP_SYMBOL(pddp::n4e::g_elem_marks), z, 64);
  return 0;
}
#endif
#ifdef PDDP_WG_TIMELINE
extern "C" int pddp_debug_elem_timeline(long long* out) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::n4e::g_elem_timeline),
                      sizeof(long long) * 1024 * 12);
  return 0;
}
#endif
