// cartpole_branches.hip - the cartpole's record-free sweep and one-launch
// round for the gain branches of the reference's `backward` other than the
// bounded eig-clamp one: eig-clamp without action bounds (ilqr.py:635-643) and
// V_zz-regularised with and without them (ilqr.py:587-625).  The device code
// is riccati_n4_elem.hpp (sweep; BR selects the gain step and value update)
// and line_search_lds.hpp (search) through round_n4_body.hpp - the same lane
// mapping, LDS images, generator and search as the bounded eig-clamp kernels
// of riccati_nominal.hip / round_n4.hip, which are instantiated there and not
// touched by anything here.  A translation unit of its own: kernels of other
// names (the ISA tests of the benched kernels find theirs by name), its own
// line of flags in the Makefile.  Its launchers are handed the launch's plan
// (n4_nominal_plan, riccati_n4_elem.hpp: grid, workgroup, LDS, cost mask,
// generator / rounds form) by launch_n4_elem and launch_round_n4 and only pick
// the instantiation it names.  DESIGN.md 3.1i.
#include "round_n4_body.hpp"

namespace pddp {

namespace n4e {

template <unsigned QM, bool OVL, int BR>
__global__ __launch_bounds__((OVL ? 2 : 1) * kWaves * kWave) void
sweep_n4_branch_kernel(RiccatiArgs<float> a, GenArgs<float> gen,
                       ProblemT<float> prob) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  RoundOut ro;
  elem_sweep_body<float, QM, OVL, false, BR>(a, gen, prob, smem_raw, ro);
}
template <unsigned QM, int BR>
__global__ __launch_bounds__(kWaves * kWave) void sweep_n4_branch_f64_kernel(
    RiccatiArgs<double> a, GenArgs<double> gen, ProblemT<double> prob) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  RoundOut ro;
  elem_sweep_body<double, QM, false, false, BR>(a, gen, prob, smem_raw, ro);
}

}  // namespace n4e

template <unsigned QM, bool MULTI, int BR>
__global__ __launch_bounds__(2 * n4e::kWaves * kWave) void
round_n4_branch_kernel(RiccatiArgs<float> a, n4d::GenArgs<float> gen,
                       ProblemT<float> prob, LineSearchArgs<float> ls,
                       AcceptArgs<float> ac, float* scratch, int rounds,
                       long long* phase_ticks, int use_carry) {
  round_n4_body<QM, MULTI, BR>(a, gen, prob, ls, ac, scratch, rounds,
                               phase_ticks, use_carry);
}

// PDDP_BRANCH_PICK(K): the instantiation K(cost mask, gain branch) that plan
// `pl` (n4_nominal_plan) names; the callers have kept kBrEigBox for their own
// kernels.  (Nested to the left: the compiler then meets the instantiations -
// and lays the kernels out in the code object - in the order written.)
#define PDDP_BY_BRANCH(K, QM)                                                 \
  (pl.br != n4e::kBrCholBox                                                   \
       ? (pl.br == n4e::kBrEig ? K(QM, n4e::kBrEig) : K(QM, n4e::kBrChol))    \
       : K(QM, n4e::kBrCholBox))
#define PDDP_BRANCH_PICK(K)                                                   \
  (pl.sparse ? PDDP_BY_BRANCH(K, kSparseMask<PDDP_MODEL_CARTPOLE>)            \
             : PDDP_BY_BRANCH(K, kFullMask<PDDP_MODEL_CARTPOLE>))

int launch_n4_branches(const pddp_problem& p, const N4NominalPlan& pl,
                       const RiccatiArgs<float>& a,
                       const n4d::GenArgs<float>& gen, hipStream_t st) {
#define PDDP_K(QM, BR)                                                        \
  (pl.ovl ? n4e::sweep_n4_branch_kernel<QM, true, BR>                         \
          : n4e::sweep_n4_branch_kernel<QM, false, BR>)
  return launch_dyn_lds(PDDP_BRANCH_PICK(PDDP_K), dim3(pl.grid),
                        dim3(pl.threads), pl.lds, st, a, gen,
                        convert_problem<float>(p));
#undef PDDP_K
}

int launch_n4_branches(const pddp_problem& p, const N4NominalPlan& pl,
                       const RiccatiArgs<double>& a,
                       const n4d::GenArgs<double>& gen, hipStream_t st) {
#define PDDP_K(QM, BR) n4e::sweep_n4_branch_f64_kernel<QM, BR>
  return launch_dyn_lds(PDDP_BRANCH_PICK(PDDP_K), dim3(pl.grid),
                        dim3(pl.threads), pl.lds, st, a, gen,
                        convert_problem<double>(p));
#undef PDDP_K
}

int launch_round_n4_branches(const pddp_problem& p, const N4NominalPlan& pl,
                             const RiccatiArgs<float>& a,
                             const n4d::GenArgs<float>& gen,
                             const LineSearchArgs<float>& ls,
                             const AcceptArgs<float>& ac, float* scratch,
                             int rounds, long long* phase_ticks,
                             hipStream_t st) {
#define PDDP_K(QM, BR)                                                        \
  (pl.multi ? round_n4_branch_kernel<QM, true, BR>                            \
            : round_n4_branch_kernel<QM, false, BR>)
  return launch_dyn_lds(PDDP_BRANCH_PICK(PDDP_K), dim3(pl.grid),
                        dim3(pl.threads), pl.lds, st, a, gen,
                        convert_problem<float>(p), ls, ac, scratch, rounds,
                        phase_ticks, pl.use_carry);
#undef PDDP_K
}

}  // namespace pddp
