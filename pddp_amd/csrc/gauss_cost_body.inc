// gauss_cost_body.inc - the quadratic cost on the angle-augmented Gaussian
// moments (pddp/costs/quadratic.py:60-99, utils/angular.py:47-84,161-248):
//   X cost = (Ma - g)^T Q (Ma - g) + the action term + the trace term
// the text of qr_cost_default (default_kernels.hip) and of
// qr_cost_derivs_kernel's loop over the pairs (qr_cost_derivs.hip), over a
// number type X (T for values, HDual<T> for derivatives: gauss_numbers.hpp)
// and a static shape: constexpr NN non-angular dimensions followed by NANG
// angles, NA = NN + 2 NANG augmented ones.
// An included text, not a device function: inlined from a function its sums
// contract into other FMAs and the results are no longer the bytes they were
// (csrc/Makefile at FLAGS_problem_kernels; measured for this text, DESIGN.md
// 3.9a).  Included, both units compile to the instructions they had.
// The includer defines, and the text undefines at its end:
//   PDDP_COST_MU(a), PDDP_COST_COV(a, c)  mean and covariance of the state (X)
//       at positions of that order; the covariance is read as given, the
//       cross terms as (angle, non-angle): under FULL_COVARIANCE_MATRIX its
//       two triangles are separate inputs
//   PDDP_COST_Q(r, c), PDDP_COST_GOAL(r)  the cost matrix of this step and
//       the goal (T)
//   PDDP_COST_JITTER  a statement after which `jit` (T) is the jitter at
//       which the Cholesky of Cav [NA][NA], the augmented covariance's values,
//       succeeded; 0: none asked; < 0: the trace is the diagonal's -
//       encode()'s fall-back, and the encodings that keep variances only
//   PDDP_COST_ACTION  statements that add the action term to `cost`
// and two that only keep each unit's instructions what they were (how a zero
// is spelled decides what the vectoriser pairs, DESIGN.md 3.9a):
//   PDDP_COST_ZERO  the zero of X: lift<X>(T(0)) in default_kernels.hip,
//       hd(0.f) in qr_cost_derivs.hip
//   PDDP_COST_JITTER_TERM(s)  jitter tr(Q) as it is added: as a number of type
//       X in default_kernels.hip (three additions of zero for a hyper-dual),
//       to the value alone in qr_cost_derivs.hip
// (bnn_rollout.hip keeps its value-only copy: the polynomial sine, run-time
// dimensions, another summation order.)
  T Cav[NA][NA];
  X Ma[NA];
  X tr = PDDP_COST_ZERO, trd = PDDP_COST_ZERO;  // sum Ca_ij Q_ji; sum Ca_ii Q_ii
  auto put = [&](int r, int c, X v) {  // every entry is written once
    Cav[r][c] = val(v);
    tr = tr + PDDP_COST_Q(c, r) * v;
    if (r == c) trd = trd + PDDP_COST_Q(r, r) * v;
  };
#pragma unroll
  for (int r = 0; r < NN; ++r) {
    Ma[r] = PDDP_COST_MU(r);
#pragma unroll
    for (int c = 0; c < NN; ++c) put(r, c, PDDP_COST_COV(r, c));
  }
#pragma unroll
  for (int a1 = 0; a1 < NANG; ++a1) {
    const int i1 = NN + a1;
    const X m1 = PDDP_COST_MU(i1), v1 = PDDP_COST_COV(i1, i1);
    const X damp = exp_(T(-0.5) * v1);
    X s1, c1;
    sincos_x(m1, s1, c1);
    const X Es = damp * s1, Ec = damp * c1;
    const int r = NN + 2 * a1;
    Ma[r] = Es;
    Ma[r + 1] = Ec;
#pragma unroll
    for (int a2 = 0; a2 < NANG; ++a2) {
      const int i2 = NN + a2;
      const X m2 = PDDP_COST_MU(i2), v2 = PDDP_COST_COV(i2, i2),
              cij = PDDP_COST_COV(i1, i2);
      const X lq = T(-0.5) * (v1 + v2), qq = exp_(lq);
      const X ep = exp_(lq + cij) - qq, em = exp_(lq - cij) - qq;
      X sd, cd, ss, cs;
      sincos_x(m1 - m2, sd, cd);
      sincos_x(m1 + m2, ss, cs);
      const int cc = NN + 2 * a2;
      put(r, cc, T(0.5) * (ep * cd - em * cs));          // sin, sin
      put(r + 1, cc + 1, T(0.5) * (ep * cd + em * cs));  // cos, cos
      const X sc = T(0.5) * (ep * sd + em * ss);         // sin_1, cos_2
      put(r, cc + 1, sc);
      put(cc + 1, r, sc);
    }
#pragma unroll
    for (int c = 0; c < NN; ++c) {
      // row = the angle (utils/angular.py:243-245 sums over the row index)
      const X col = PDDP_COST_COV(i1, c);
      put(c, r, col * Ec);         // Cov(x, sin)
      put(c, r + 1, -(col * Es));  // Cov(x, cos)
      put(r, c, col * Ec);
      put(r + 1, c, -(col * Es));
    }
  }
  PDDP_COST_JITTER
  X cost = PDDP_COST_ZERO;
#pragma unroll
  for (int c = 0; c < NA; ++c) {
    X row = PDDP_COST_ZERO;
#pragma unroll
    for (int r = 0; r < NA; ++r)
      row = row + PDDP_COST_Q(r, c) * (Ma[r] - PDDP_COST_GOAL(r));
    cost = cost + row * (Ma[c] - PDDP_COST_GOAL(c));
  }
  PDDP_COST_ACTION
  if (jit >= T(0)) {
    T trq = T(0);
#pragma unroll
    for (int r = 0; r < NA; ++r) trq += PDDP_COST_Q(r, r);
    cost = cost + tr + PDDP_COST_JITTER_TERM(jit * trq);  // tr(Q (Ca + jitter I))
  } else {
    cost = cost + trd;  // encode()'s diagonal fall-back
  }
#undef PDDP_COST_ZERO
#undef PDDP_COST_MU
#undef PDDP_COST_COV
#undef PDDP_COST_Q
#undef PDDP_COST_GOAL
#undef PDDP_COST_JITTER
#undef PDDP_COST_JITTER_TERM
#undef PDDP_COST_ACTION
