// gauss_numbers.hpp - the number types and the jittered Cholesky that the
// kernels of the Gaussian state encodings share (default_kernels.hip,
// qr_cost_derivs.hip): hyper-dual numbers for a value with its gradient and
// Hessian entry, forward duals for one tangent, and the attempt ladder of
// utils/encoding.py:536-564.  The scalar exp_ / log_ / sincos_lib are
// pddp_common.hpp's.  (gp_step_body.hpp keeps gp::Dual - its division
// multiplies by a reciprocal - and its own ladder; bnn_rollout.hip keeps its
// run-time-sized Cholesky out of LDS: DESIGN.md 3.9a.)
#pragma once

#include "pddp_common.hpp"

namespace pddp {

template <typename T>
struct HDual {  // hyper-dual number: value, d/dx_i, d/dx_j, d2/dx_i dx_j
  typedef T S;  // (scalar operands are not deduced: 0.5f * HDual<double>)
  T v, a, b, ab;
};
template <typename T> PDDP_DEV HDual<T> operator+(HDual<T> x, HDual<T> y) { return {x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab}; }
template <typename T> PDDP_DEV HDual<T> operator-(HDual<T> x, HDual<T> y) { return {x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab}; }
template <typename T> PDDP_DEV HDual<T> operator-(HDual<T> x) { return {-x.v, -x.a, -x.b, -x.ab}; }
template <typename T> PDDP_DEV HDual<T> operator*(HDual<T> x, HDual<T> y) {
  return {x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b,
          x.ab * y.v + x.a * y.b + x.b * y.a + x.v * y.ab};
}
template <typename T> PDDP_DEV HDual<T> operator*(typename HDual<T>::S s, HDual<T> x) { return {s * x.v, s * x.a, s * x.b, s * x.ab}; }
template <typename T> PDDP_DEV HDual<T> operator+(HDual<T> x, typename HDual<T>::S s) { return {x.v + s, x.a, x.b, x.ab}; }
template <typename T> PDDP_DEV HDual<T> operator-(HDual<T> x, typename HDual<T>::S s) { return {x.v - s, x.a, x.b, x.ab}; }
template <typename T> PDDP_DEV HDual<T> exp_(HDual<T> x) {
  const T e = exp_(x.v);
  return {e, e * x.a, e * x.b, e * (x.ab + x.a * x.b)};
}
template <typename T> PDDP_DEV void sincos_x(T x, T& s, T& c) { sincos_lib(x, s, c); }
template <typename T> PDDP_DEV void sincos_x(HDual<T> x, HDual<T>& s, HDual<T>& c) {
  T sv, cv;
  sincos_lib(x.v, sv, cv);
  s = {sv, cv * x.a, cv * x.b, cv * x.ab - sv * x.a * x.b};
  c = {cv, -sv * x.a, -sv * x.b, -sv * x.ab - cv * x.a * x.b};
}
template <typename T> PDDP_DEV T val(T x) { return x; }
template <typename T> PDDP_DEV T val(HDual<T> x) { return x.v; }
template <typename X, typename T> PDDP_DEV X lift(T v) {
  if constexpr (sizeof(X) == sizeof(T)) return v;
  else return X{v, T(0), T(0), T(0)};
}

template <typename T>
struct FDual {  // forward dual number: value, one tangent
  T v, d;
};
template <typename T> PDDP_DEV FDual<T> operator+(FDual<T> x, FDual<T> y) { return {x.v + y.v, x.d + y.d}; }
template <typename T> PDDP_DEV FDual<T> operator-(FDual<T> x, FDual<T> y) { return {x.v - y.v, x.d - y.d}; }
template <typename T> PDDP_DEV FDual<T> operator*(FDual<T> x, FDual<T> y) { return {x.v * y.v, x.d * y.v + x.v * y.d}; }
template <typename T> PDDP_DEV FDual<T> operator/(FDual<T> x, FDual<T> y) {
  const T q = x.v / y.v;
  return {q, (x.d - q * y.d) / y.v};
}
template <typename T> PDDP_DEV FDual<T> sqrt_x(FDual<T> x) {
  const T r = sqrt_(x.v);
  return {r, x.d / (r + r)};
}
template <typename T> PDDP_DEV T sqrt_x(T x) { return sqrt_(x); }
template <typename T> PDDP_DEV T val(FDual<T> x) { return x.v; }

// the jittered upper Cholesky only decides which trace the cost sees
// (encoding.py:536-564: jitter 1e-12, 1e-11, ... <= 10, else the diagonal):
// the jitter of the first attempt that succeeds, -1 when none does
template <typename T, int NA>
PDDP_DEV T chol_jitter_of(const T (&C)[NA][NA]) {
  double jit = 1e-12;
  while (jit <= 10.0) {
    T U[NA][NA];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
#pragma unroll
      for (int j = i; j < NA; ++j) {
        T s = C[i][j] + (i == j ? (T)jit : T(0));
#pragma unroll
        for (int q = 0; q < i; ++q) s -= U[q][i] * U[q][j];
        if (i == j) {
          if (!(s > T(0))) ok = false;
          U[i][i] = sqrt_(s);
        } else {
          U[i][j] = s / U[i][i];
        }
      }
    }
    if (ok) return (T)jit;
    jit *= 10.0;
  }
  return T(-1);
}

}  // namespace pddp
