// round_n4.hip - ONE launch for a whole round of the cartpole f32 path
// (BASELINE.json configs[1]; this file: the kernels of the bounded eig-clamp
// branch and the entry point - the other three gain branches run the same
// body, round_n4_body.hpp, in the kernels of cartpole_branches.hip; what the
// launch looks like for all four is n4_nominal_plan's, riccati_n4_elem.hpp):
// the backward sweep from the nominal
// (riccati_n4_elem.hpp; ilqr.py:489-674 with the records of :393-486 evaluated
// in place) and then, in the SAME wavefronts for the same four trajectories,
// the batched line search, argmin, accept / regularisation schedule and the
// copy of the winner into the nominal (line_search_lds.hpp; ilqr.py:677-791,
// :140-181, :364-390).
//
// Why (tools/wg_timeline.py, profiles/r05_wg_timeline_*.txt):
// as two launches a round at B = 4096 was 29.3 us of sweep workgroups, 2.6 us
// of idle chip between the launches, 36.8 us of search workgroups and 2.6 us
// again before the next round - and inside the search launch every workgroup
// spent 5.4 us copying the nominal and the gains from global memory into LDS
// before its first step.  Both launches have the same shape (16 trajectories
// per workgroup, four chain wavefronts and four partner wavefronts, one
// workgroup per CU), so the workgroup simply goes on: the gains never leave
// LDS between the phases (they are still written to HBM, by the partner
// wavefront, for the API), the partner stages the nominal's rows while the
// sweep runs its last block, the nominal's cost and the sweep's status cross in
// LDS / registers, and a workgroup whose sweep ends early starts its search
// early - the round is the slowest workgroup's SUM, not the sum of the two
// slowest phases.
//
// Same code as the two launches (device functions shared with them): the
// sweep's outputs are theirs bit for bit, decisions and masks identical, the
// search's values to rounding - the same closed forms inlined into another
// kernel are contracted into FMAs differently (tests/test_gpu_parity.py::
// test_one_launch_round_equals_two_launches); R rounds per launch are R
// one-round launches bit for bit (test_rounds_in_one_launch_equal_single_
// rounds).  The search's step here differs from the stand-alone launch's in
// three places, each an A/B-measured cut: the nominal row is
// read with one 16-byte and three 8-byte LDS reads, one LDS wait per step, and
// between the rounds of a launch the nominal's last rows stay in LDS.
#include "round_n4_body.hpp"

namespace pddp {

template <unsigned QM, bool MULTI>
__global__ __launch_bounds__(2 * n4e::kWaves * kWave) void round_n4_kernel(
    RiccatiArgs<float> a, n4d::GenArgs<float> gen, ProblemT<float> prob,
    LineSearchArgs<float> ls, AcceptArgs<float> ac, float* scratch,
    int rounds, long long* phase_ticks, int use_carry) {
  round_n4_body<QM, MULTI, n4e::kBrEigBox>(a, gen, prob, ls, ac, scratch,
                                           rounds, phase_ticks, use_carry);
}

// n4_nominal_plan (riccati_n4_elem.hpp) decides the launch; here: the kernel
// instantiation it names
static int launch_round_n4(const pddp_problem& p, const RiccatiArgs<float>& a,
                           const n4d::GenArgs<float>& gen,
                           const LineSearchArgs<float>& ls,
                           const AcceptArgs<float>& ac, float* scratch,
                           int rounds, long long* phase_ticks,
                           hipStream_t st) {
  N4NominalPlan pl;
  if (const int rc = n4_nominal_plan(p, sizeof(float), true, a.B, a.N, ls.A,
                                     a.u_min != nullptr, a.u_max != nullptr,
                                     a.branch, rounds, 0, pl))
    return rc;
  // (the other gain branches: kernels of their own, cartpole_branches.hip)
  if (pl.br != n4e::kBrEigBox)
    return launch_round_n4_branches(p, pl, a, gen, ls, ac, scratch, rounds,
                                    phase_ticks, st);
#define PDDP_K(QM)                                                            \
  (pl.multi ? round_n4_kernel<QM, true> : round_n4_kernel<QM, false>)
  return launch_dyn_lds(PDDP_N4_BY_MASK(PDDP_K), dim3(pl.grid),
                        dim3(pl.threads), pl.lds, st, a, gen,
                        convert_problem<float>(p), ls, ac, scratch, rounds,
                        phase_ticks, pl.use_carry);
#undef PDDP_K
}

}  // namespace pddp

extern "C" int pddp_round_nominal_f32(
    const pddp_problem* problem, int B, int N, int A, float* Z, float* U,
    const float* alphas, const float* u_min, const float* u_max, int branch,
    uint8_t* active, uint8_t* fresh, float* gains, int32_t* bwd_status,
    float* L, float* J_opt, float* Zc, float* Uc, float* Jc, double tol,
    double max_reg, int n_iterations, float* gains_acc, double* mu,
    double* delta, int32_t* state, int32_t* iter, int32_t* n_live,
    float* scratch, int rounds, long long* phase_ticks, void* stream) {
  if (problem == nullptr || B <= 0 || N <= 0 || A <= 0 || !Z || !U || !alphas ||
      !active || !fresh || !gains || !bwd_status || !L || !J_opt || !Zc ||
      !Uc || !Jc || !gains_acc || !mu || !delta || !state || !iter || !scratch)
    return PDDP_E_BADARG;
  if (branch != PDDP_BRANCH_EIG && branch != PDDP_BRANCH_CHOLESKY)
    return PDDP_E_BADARG;
  // (mu: the sweep's regulariser and the schedule's state)
  const pddp::NominalArgs<float> sw = pddp::nominal_args<float>(
      *problem, B, N, Z, U, u_min, u_max, mu, branch, active, fresh, gains,
      bwd_status, L, J_opt);
  const pddp::LineSearchArgs<float> ls{B, N, A, Z, U, gains, alphas, u_min,
                                       u_max, active, bwd_status, Zc, Uc, Jc};
  const pddp::AcceptArgs<float> ac{
      B, N, 4, 1, A, Zc, Uc, Jc, gains, bwd_status, tol, max_reg, n_iterations,
      Z, U, gains_acc, J_opt, mu, delta, state, iter, active, fresh, n_live};
  return pddp::launch_round_n4(*problem, sw.a, sw.gen, ls, ac, scratch, rounds,
                               phase_ticks, (hipStream_t)stream);
}

#ifdef PDDP_WG_TIMELINE
// (this translation unit's copies of the marks: tools/wg_timeline.py)
extern "C" int pddp_debug_round_timeline(long long* sweep, long long* search) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(sweep, HIP_SYMBOL(pddp::n4e::g_elem_timeline),
                            sizeof(long long) * 1024 * 12);
  (void)hipMemcpyFromSymbol(search, HIP_SYMBOL(pddp::g_search_timeline),
                            sizeof(long long) * 1024 * 12);
  return 0;
}
#endif
