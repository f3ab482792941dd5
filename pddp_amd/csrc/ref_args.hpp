// ref_args.hpp - where the kernels with a goal PER TIME STEP take their goals
// from: what goal_kernels.hpp, closed_loop.hip, mpc_advance.hip and
// mpc_advance_noise.hip share.  The layout of `ref` is include/pddp_hip.h's
// (PDDP_REF_*); DESIGN.md 3.4e.
#pragma once

#include "pddp_common.hpp"

namespace pddp {

// where the goals come from; ref_t0 arrives clamped to ref_len - 1, so that
// `ref_t0 + min(i, hold)` neither leaves the reference nor overflows
template <typename T>
struct RefArgs {
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the model parameters
  const T* ref;    // [B][ref_len][PDDP_REF_ROW]
  int ref_len, ref_t0;
};

// A statement, not a function (problem_kernels.hip's note: the same statements
// inlined from a function reach the optimiser in another order - here too, the
// kernels then differ in their mul / add / fma mix): K words of `src` copied to
// `dst`, for the goals at PDDP_REF_X_GOAL (na words) and PDDP_REF_U_GOAL (m
// words) of a reference row.
#define PDDP_COPY(K, dst, src) \
  _Pragma("unroll") for (int i = 0; i < (K); ++i)(dst)[i] = (src)[i];

template <typename T>
PDDP_DEV const T* ref_row(const RefArgs<T>& g, int b, int i) {
  const int hold = g.ref_len - 1 - g.ref_t0;
  const int row = g.ref_t0 + (i < hold ? i : hold);
  return g.ref + ((size_t)b * g.ref_len + row) * PDDP_REF_ROW;
}

// ref_t0 clamped to the last row here (see RefArgs); false: PDDP_E_BADARG
template <typename T>
static bool ref_args(const T* table, const T* ref, int ref_len, int ref_t0,
                     RefArgs<T>* out) {
  if (ref == nullptr || ref_len < 1 || ref_t0 < 0) return false;
  *out = RefArgs<T>{table, ref, ref_len,
                    ref_t0 < ref_len - 1 ? ref_t0 : ref_len - 1};
  return true;
}

}  // namespace pddp
