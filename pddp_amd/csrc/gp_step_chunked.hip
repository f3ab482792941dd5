// gp_step_chunked.hip - the GP step's chunked form: any number of training
// points (gp_step_body.hpp, CH).  Kernels of their own, in a translation unit
// of their own, so that the resident kernels compile to what they did.
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

// Rows per launch.  A row is one workgroup and almost all of it is B: NP pairs
// x M^2 terms at kCyclesPerTerm workgroup cycles each (measured: 3.35 M cycles
// for the float Jacobian row at M = 300, E = 6 - DESIGN.md 3.11 - is 1.8 per
// term; double: about three times that).  One launch gets the rows that 256
// CUs, a workgroup each, work off in kLaunchSeconds at kClockHz - the shared
// card is never held for seconds by one launch - and never fewer than one row
// per CU
constexpr double kCyclesPerTermF32 = 2.0, kCyclesPerTermF64 = 6.0;
constexpr double kLaunchSeconds = 0.15, kClockHz = 2.4e9;
constexpr int kCUs = 256;
template <typename T, int E>
int rows_per_launch_of(int M, int forced) {
  if (forced > 0) return forced;
  const double per_row = (sizeof(T) == 4 ? kCyclesPerTermF32 : kCyclesPerTermF64) *
                         (E * (E + 1) / 2) * (double)M * (double)M;
  const double rows = kLaunchSeconds * kClockHz * kCUs / per_row;
  return rows < kCUs ? kCUs : rows > 1e9 ? 1000000000 : (int)rows;
}

template <typename K>
int allow_lds(K kern, size_t bytes) {
  if (bytes <= 64 * 1024) return 0;
  return (int)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes);
}

template <typename T, int E, int D>
int launch_chunked(const Args<T>& a, bool jac, int C, int rows_per_launch, hipStream_t st) {
  const int K = a.n + a.m_act;
  if (K > 64 || C < 2 || (C & 1)) return PDDP_E_UNSUPPORTED;
  const size_t bytes = (size_t)chunked_words<E, D>(C, K, jac) * sizeof(T);
  if (bytes > (size_t)kGpLdsMax) return PDDP_E_UNSUPPORTED;
  auto kern = jac ? gp_step_chunked_kernel<T, E, D, true> : gp_step_chunked_kernel<T, E, D, false>;
  if (int rc = allow_lds(kern, bytes)) return rc;
  const int per = rows_per_launch_of<T, E>(a.M, rows_per_launch);
  // consecutive slices of the rows on the one stream (rows are independent)
  for (int row0 = 0; row0 < a.R; row0 += per) {
    const int rows = a.R - row0 < per ? a.R - row0 : per;
    hipLaunchKernelGGL(kern, dim3(rows), dim3(kThreads), bytes, st, a, Chunk{C, row0});
  }
  return (int)hipGetLastError();
}

template <typename T, int E, int D>
int launch_roll_chunked(Args<T> a, Roll<T> r, int C, int rows_per_launch, hipStream_t st) {
  if (a.n + a.m_act > 64 || r.na > 8 || r.na != a.n_non + 2 * a.n_ang || a.m_act > kMaxAct)
    return PDDP_E_UNSUPPORTED;
  if (C < 2 || (C & 1)) return PDDP_E_UNSUPPORTED;
  const size_t bytes = (size_t)chunked_words<E, D>(C, a.n + a.m_act, false) * sizeof(T);
  if (bytes > (size_t)kGpLdsMax) return PDDP_E_UNSUPPORTED;
  auto kern = gp_roll_chunked_kernel<T, E, D>;
  if (int rc = allow_lds(kern, bytes)) return rc;
  a.R = r.B * r.A;
  const int per = rows_per_launch_of<T, E>(a.M, rows_per_launch);
  // N steps and the terminal cost, each in slices of the rows (the terminal
  // launch has no M^2 loop: one slice)
  for (int t = 0; t <= r.N; ++t) {
    r.t = t;
    r.terminal = t == r.N ? 1 : 0;
    const int step = r.terminal ? a.R : per;
    for (int row0 = 0; row0 < a.R; row0 += step) {
      const int rows = a.R - row0 < step ? a.R - row0 : step;
      hipLaunchKernelGGL(kern, dim3(rows), dim3(kThreads), bytes, st, a, r, Chunk{C, row0});
    }
  }
  return (int)hipGetLastError();
}

#define PDDP_GP_CHUNKED_INST(T, E, D)                                                          \
  template int launch_chunked<T, E, D>(const Args<T>&, bool, int, int, hipStream_t);           \
  template int launch_roll_chunked<T, E, D>(Args<T>, Roll<T>, int, int, hipStream_t);
PDDP_GP_CHUNKED_INST(float, 2, 4)
PDDP_GP_CHUNKED_INST(float, 4, 6)
PDDP_GP_CHUNKED_INST(float, 6, 9)
PDDP_GP_CHUNKED_INST(double, 2, 4)
PDDP_GP_CHUNKED_INST(double, 4, 6)
PDDP_GP_CHUNKED_INST(double, 6, 9)

}  // namespace gp
}  // namespace pddp

#ifdef PDDP_GP_MARKS
extern "C" int pddp_debug_gp_marks_chunked(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::gp::g_gp_marks), sizeof(long long) * 64);
}
#endif
