// gp_step_chunked.hip - the kernels of the GP step's chunked form: any number
// of training points (gp_step_body.hpp, CH).  Kernels of their own, in a
// translation unit of their own, so that the resident kernels compile to what
// they did.  Nothing is launched here: gp_step.hip takes the kernels from
// chunked_step_kernel / chunked_roll_kernel and launches both forms.
#include "gp_step_body.hpp"

namespace pddp {
namespace gp {

// (no waves-per-SIMD cap on the float forward forms as the resident ones have:
// under it they would spill; these kernels spill nothing)
template <typename T, int E, int D, bool JAC>
__global__ __launch_bounds__(kThreads) void gp_step_chunked_kernel(const Args<T> A, const Chunk CK) {
  gp_step_body<T, E, D, JAC, false, true>(A, Roll<T>(), CK);
}
template <typename T, int E, int D>
__global__ __launch_bounds__(kThreads)
void gp_roll_chunked_kernel(const Args<T> A, const Roll<T> RL, const Chunk CK) {
  gp_step_body<T, E, D, false, true, true>(A, RL, CK);
}

// What the launcher (gp_step.hip) launches; instantiated here for every built
// pair, which instantiates the kernels
template <typename T, int E, int D>
ChunkedStepKernel<T> chunked_step_kernel(bool jac) {
  return jac ? gp_step_chunked_kernel<T, E, D, true> : gp_step_chunked_kernel<T, E, D, false>;
}
template <typename T, int E, int D>
ChunkedRollKernel<T> chunked_roll_kernel() {
  return gp_roll_chunked_kernel<T, E, D>;
}
#define PDDP_GP_CHUNKED_INST(E, D)                                            \
  template ChunkedStepKernel<float> chunked_step_kernel<float, E, D>(bool);   \
  template ChunkedRollKernel<float> chunked_roll_kernel<float, E, D>();       \
  template ChunkedStepKernel<double> chunked_step_kernel<double, E, D>(bool); \
  template ChunkedRollKernel<double> chunked_roll_kernel<double, E, D>();
PDDP_GP_SHAPES(PDDP_GP_CHUNKED_INST)
#undef PDDP_GP_CHUNKED_INST

}  // namespace gp
}  // namespace pddp

#ifdef PDDP_GP_MARKS
extern "C" int pddp_debug_gp_marks_chunked(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::gp::g_gp_marks), sizeof(long long) * 64);
}
#endif
