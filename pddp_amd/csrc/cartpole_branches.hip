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
// line of flags in the Makefile.  DESIGN.md 3.1i.
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

namespace {
constexpr unsigned kSparse = 0b11001u;  // CartpoleCost: {x, sin, cos}
constexpr unsigned kFull = kFullMask<PDDP_MODEL_CARTPOLE>;
constexpr int kPer = n4e::kWaves * n4e::kTrajW;  // trajectories / workgroup
bool sparse_cost(const pddp_problem& p) {
  return (live_mask(p.Q, ModelDims<PDDP_MODEL_CARTPOLE>::na) & ~kSparse) == 0;
}
// GO(QM, BR): the launch of one instantiation; the run-time (cost matrix,
// branch) pair picks it
#define PDDP_BRANCH_DISPATCH(GO)                                              \
  do {                                                                        \
    if (sparse) {                                                             \
      if (br == n4e::kBrEig) GO(kSparse, n4e::kBrEig);                        \
      else if (br == n4e::kBrChol) GO(kSparse, n4e::kBrChol);                 \
      else GO(kSparse, n4e::kBrCholBox);                                      \
    } else {                                                                  \
      if (br == n4e::kBrEig) GO(kFull, n4e::kBrEig);                          \
      else if (br == n4e::kBrChol) GO(kFull, n4e::kBrChol);                   \
      else GO(kFull, n4e::kBrCholBox);                                        \
    }                                                                         \
  } while (0)
#define PDDP_SET_LDS(KERN, LDS)                                               \
  do {                                                                        \
    const hipError_t e = hipFuncSetAttribute(                                 \
        (const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize,        \
        (int)(LDS));                                                          \
    if (e != hipSuccess) return (int)e;                                       \
  } while (0)
bool served(int br) {
  return br == n4e::kBrEig || br == n4e::kBrChol || br == n4e::kBrCholBox;
}
}  // namespace

int launch_n4_branches(const pddp_problem& p, const RiccatiArgs<float>& a,
                       const n4d::GenArgs<float>& gen, hipStream_t st,
                       bool ovl, int br) {
  if (!served(br)) return PDDP_E_UNSUPPORTED;
  const ProblemT<float> P = convert_problem<float>(p);
  const dim3 grid((a.B + kPer - 1) / kPer);
  const bool sparse = sparse_cost(p);
  const size_t lds = (size_t)n4e::kWaves * sizeof(float) *
                     (ovl ? n4e::kPairLdsOvl : n4e::kPairLdsInl);
#define PDDP_GO(QMV, BRV)                                                     \
  do {                                                                        \
    if (ovl) {                                                                \
      auto kern = n4e::sweep_n4_branch_kernel<QMV, true, BRV>;                \
      PDDP_SET_LDS(kern, lds);                                                \
      PDDP_LAUNCH(kern, grid, dim3(2 * n4e::kWaves * kWave), lds, st, a, gen, \
                  P);                                                         \
    } else {                                                                  \
      auto kern = n4e::sweep_n4_branch_kernel<QMV, false, BRV>;               \
      PDDP_SET_LDS(kern, lds);                                                \
      PDDP_LAUNCH(kern, grid, dim3(n4e::kWaves * kWave), lds, st, a, gen, P); \
    }                                                                         \
  } while (0)
  PDDP_BRANCH_DISPATCH(PDDP_GO);
#undef PDDP_GO
  return launch_status();
}

int launch_n4_branches_f64(const pddp_problem& p, const RiccatiArgs<double>& a,
                           const n4d::GenArgs<double>& gen, hipStream_t st,
                           int br) {
  if (!served(br)) return PDDP_E_UNSUPPORTED;
  const ProblemT<double> P = convert_problem<double>(p);
  const dim3 grid((a.B + kPer - 1) / kPer);
  const bool sparse = sparse_cost(p);
  const size_t lds =
      (size_t)n4e::kWaves * sizeof(double) * n4e::kPairLdsInl;  // 106 KB
#define PDDP_GO(QMV, BRV)                                                     \
  do {                                                                        \
    auto kern = n4e::sweep_n4_branch_f64_kernel<QMV, BRV>;                    \
    PDDP_SET_LDS(kern, lds);                                                  \
    PDDP_LAUNCH(kern, grid, dim3(n4e::kWaves * kWave), lds, st, a, gen, P);   \
  } while (0)
  PDDP_BRANCH_DISPATCH(PDDP_GO);
#undef PDDP_GO
  return launch_status();
}

// (the caller, launch_round_n4, has checked model, encoding, N, A, rounds)
int launch_round_n4_branches(const pddp_problem& p, const RiccatiArgs<float>& a,
                             const n4d::GenArgs<float>& gen,
                             const LineSearchArgs<float>& ls,
                             const AcceptArgs<float>& ac, float* scratch,
                             int rounds, long long* phase_ticks, hipStream_t st,
                             int br) {
  if (!served(br)) return PDDP_E_UNSUPPORTED;
  const dim3 grid((a.B + kPer - 1) / kPer);
  // one workgroup per CU, as the bounded eig-clamp round (round_n4.hip)
  if (grid.x > 256u) return PDDP_E_UNSUPPORTED;
  int use_carry;
  const size_t lds = round_n4_lds(a.N, rounds, use_carry);
  if (lds == 0) return PDDP_E_UNSUPPORTED;
  const ProblemT<float> P = convert_problem<float>(p);
  const bool sparse = sparse_cost(p);
#define PDDP_GO(QMV, BRV)                                                     \
  do {                                                                        \
    auto kern = rounds > 1 ? round_n4_branch_kernel<QMV, true, BRV>           \
                           : round_n4_branch_kernel<QMV, false, BRV>;         \
    PDDP_SET_LDS(kern, lds);                                                  \
    PDDP_LAUNCH(kern, grid, dim3(2 * n4e::kWaves * kWave), lds, st, a, gen,   \
                P, ls, ac, scratch, rounds, phase_ticks, use_carry);          \
  } while (0)
  PDDP_BRANCH_DISPATCH(PDDP_GO);
#undef PDDP_GO
  return launch_status();
}

}  // namespace pddp
