// bnn_mlp_check.hpp - what every pddp_bnn_mlp_* entry point, f32
// (bnn_mlp.hip) and f64 (bnn_mlp_f64.hip), refuses before it launches.
#pragma once
#include "pddp_common.hpp"

namespace pddp {

// `a`: BnnMlpArgs or BnnMlpArgs64 (the same names).  group 0: the plain
// network, else forward mode in groups of `group` rows with `live` in use.
// The answers in this order: sizes and NULLs, the groups (BADARG); the
// network's limits (UNSUPPORTED); f64: the masks, which are read 32 bytes at
// a time (BADARG).  H is the launcher's switch: UNSUPPORTED after all these.
template <typename A>
int bnn_mlp_check(const A& a, int group, int live, int w1_max, int max_out) {
  constexpr bool f64 = sizeof(*a.X) == 8;
  if (a.R <= 0 || a.P <= 0 || a.in_dim <= 0 || a.H <= 0 || a.out_dim <= 0 ||
      !a.X || !a.W1 || !a.b1 || !a.MT1 || !a.W2 || !a.b2 || !a.MT2 || !a.W3 ||
      !a.b3 || !a.Y)
    return PDDP_E_BADARG;
  if (group != 0 &&
      ((group != 8 && group != 16 && group != 32) || a.R % group != 0 ||
       live < 1 || live > group))
    return PDDP_E_BADARG;
  if (a.in_dim >= w1_max || a.out_dim > max_out || (f64 && group == 32))
    return PDDP_E_UNSUPPORTED;
  if (f64 && (((uintptr_t)a.MT1 | (uintptr_t)a.MT2) & 31) != 0)
    return PDDP_E_BADARG;
  return 0;
}

}  // namespace pddp
