// problem_args.hpp - kernel argument blocks of the problem kernels (shared by
// problem_kernels.hip with goal_kernels.hpp: IGNORE_UNCERTAINTY, and
// default_kernels.hip: the DEFAULT / upper-triangular Cholesky encoding).
#pragma once

#include "pddp_common.hpp"

namespace pddp {

template <typename T>
struct RolloutArgs {
  int B, N;
  const T* z0;
  const T* U;
  const T* u_min;
  const T* u_max;
  const uint8_t* mask;
  T* Z;
};

// the workgroup of the derivative records (derivs_body.inc): one lane per time
// step of a chunk
constexpr int kDerivThreads = 64;

template <typename T>
struct DerivArgs {
  int B, N;
  const T* Z;
  const T* U;
  const T* u_min;
  const T* u_max;
  const uint8_t* mask;
  T* rec;
  T* L;
  T* J;
  int32_t* state;
};

template <typename T>
struct LineSearchArgs {
  int B, N, A;
  const T* Z;
  const T* U;
  const T* gains;
  const T* alphas;
  const T* u_min;
  const T* u_max;
  const uint8_t* active;
  const int32_t* bwd_status;
  // Candidates are laid out time-major, Zc [B][N+1][A][n], Uc [B][N][A][m]:
  // the A lanes of a trajectory then write ONE contiguous segment per step
  // (160 B for cartpole) instead of A scattered 16-B pieces of A different
  // rows.  Measured on gfx950 (rocprofv3 WRITE_SIZE): candidate-major cost
  // 152 MB of HBM writes per launch for 82 MB of data and a third of the
  // kernel's time; the accept kernel's strided read of the one winning row is
  // 12x smaller than what this saves.
  T* Zc;
  T* Uc;
  T* Jc;
  // Fused launch without records (pddp_search_accept_*, L == NULL, rec given
  // as scratch) only: 1 = the candidates are NOT kept - a step size other than
  // the full step writes nothing but its cost, the full step its compact rows
  // in `rec`; a winner other than the full step (1 accepted attempt in 20) is
  // rolled out a second time.  B A N (n + m) words of candidates are 82 MB at
  // B = 4096 - absorbed by the 256 MB Infinity Cache - and 1.3 GB at B = 65536,
  // where writing them out at ~2 TB/s WAS the launch (654 of its 654 us).
  int drop_candidates = 0;
};

// Host side of every entry point that takes one of the blocks above
// (problem_kernels.hip, all five forms): the argument test, the grid of the
// per-candidate line search, and the carrier of a block together with a
// form's per-trajectory data through PDDP_DISPATCH_MODEL.
template <typename T>
inline bool args_ok(const DerivArgs<T>& a) {
  return !(a.B <= 0 || a.N <= 0 || !a.Z || !a.U || !a.rec || !a.L || !a.J);
}
// `int_lanes`: the kernel indexes its B * A lanes with an int (the forms with
// per-trajectory data; the uniform entry points never checked)
template <typename T>
inline bool args_ok(const LineSearchArgs<T>& a, bool int_lanes) {
  if (a.B <= 0 || a.N <= 0 || a.A <= 0 || !a.Z || !a.U || !a.gains ||
      !a.alphas || !a.Zc || !a.Uc || !a.Jc)
    return false;
  return !(int_lanes && (long long)a.B * a.A > 0x7fffffffLL);
}
// one lane per (trajectory, step size) candidate
template <typename T>
inline dim3 search_lanes(const LineSearchArgs<T>& a) {
  return dim3((unsigned)(((long long)a.B * a.A + kWave - 1) / kWave));
}
template <typename Args, typename Extra>
struct With {
  Args a;
  Extra x;
};

// The domain of the IGNORE_UNCERTAINTY problem kernels (problem_kernels.hip,
// both forms) and their dispatch on the model.
inline int check_problem(const pddp_problem* p) {
  if (p == nullptr) return PDDP_E_BADARG;
  if (p->encoding != PDDP_ENC_IGNORE_UNCERTAINTY) return PDDP_E_UNSUPPORTED;
  switch (p->model) {
    case PDDP_MODEL_CARTPOLE:
    case PDDP_MODEL_DOUBLE_CARTPOLE:
    case PDDP_MODEL_PENDULUM:
    case PDDP_MODEL_RENDEZVOUS:
      return 0;
  }
  return PDDP_E_UNSUPPORTED;
}

#define PDDP_DISPATCH_MODEL(FN, T, p, args, st)                                \
  switch ((p)->model) {                                                        \
    case PDDP_MODEL_CARTPOLE:                                                  \
      return FN<T, PDDP_MODEL_CARTPOLE>(*(p), args, st);                       \
    case PDDP_MODEL_DOUBLE_CARTPOLE:                                           \
      return FN<T, PDDP_MODEL_DOUBLE_CARTPOLE>(*(p), args, st);                \
    case PDDP_MODEL_PENDULUM:                                                  \
      return FN<T, PDDP_MODEL_PENDULUM>(*(p), args, st);                       \
    default:                                                                   \
      return FN<T, PDDP_MODEL_RENDEZVOUS>(*(p), args, st);                     \
  }

}  // namespace pddp
