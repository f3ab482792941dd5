// closed_loop_draws.hpp - the draws of the closed-loop rollouts under noise:
// what the noisy and the tracked rollout kernel of closed_loop.hip and the
// hand-over of mpc_advance_noise.hip share.  include/pddp_hip.h states the
// draws; DESIGN.md 3.4g.
#pragma once

#include "pddp_common.hpp"

namespace pddp {

// Philox4x32-10.  The two 32 x 32 -> 64 products are 64-bit multiplies: one
// v_mad_u64_u32 gives both halves.  The key is wave-uniform (scalar registers).
PDDP_DEV void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t a = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t b = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = a;
    c[1] = (uint32_t)p1;
    c[2] = b;
    c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

template <typename T>
struct DrawBlock;  // kPer: the normals of one Philox call
template <>
struct DrawBlock<float> { static constexpr int kPer = 4; };
template <>
struct DrawBlock<double> { static constexpr int kPer = 2; };

// Box-Muller on uniforms that are exact in the type and inside (0, 1): the
// integer-to-uniform step is one explicit fma of exactly representable
// operands, so no contraction can change it.  Library log / sqrt / sincospi.
PDDP_DEV float uniform_of(uint32_t x) {
  return __builtin_fmaf((float)(x >> 9), 0x1p-23f, 0x1p-24f);
}
PDDP_DEV double uniform_of(uint32_t hi, uint32_t lo) {
  const uint64_t k = ((uint64_t)hi << 20) | (uint64_t)(lo >> 12);
  return __builtin_fma((double)k, 0x1p-52, 0x1p-53);
}
PDDP_DEV void box_muller(float u1, float u2, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}
PDDP_DEV void box_muller(double u1, double u2, double& z0, double& z1) {
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// Block k of the unit normals of rollout r at step t in stream w (0 process,
// 1 measurement): components kPer k .. kPer k + kPer - 1.  THE draw: the
// rollouts and pddp_closed_loop_draws_* both come through here.
PDDP_DEV void draw_block(uint64_t seed, uint64_t r, int t, int w, int k,
                         float (&z)[4]) {
  uint32_t c[4] = {(uint32_t)r, (uint32_t)(r >> 32), (uint32_t)t,
                   ((uint32_t)w << 16) | (uint32_t)k};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  box_muller(uniform_of(c[0]), uniform_of(c[1]), z[0], z[1]);
  box_muller(uniform_of(c[2]), uniform_of(c[3]), z[2], z[3]);
}
PDDP_DEV void draw_block(uint64_t seed, uint64_t r, int t, int w, int k,
                         double (&z)[2]) {
  uint32_t c[4] = {(uint32_t)r, (uint32_t)(r >> 32), (uint32_t)t,
                   ((uint32_t)w << 16) | (uint32_t)k};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  box_muller(uniform_of(c[0], c[1]), uniform_of(c[2], c[3]), z[0], z[1]);
}

// std (.) the n unit normals of (r, t, w); components beyond n are discarded.
template <typename T, int n>
PDDP_DEV void draw_scaled(uint64_t seed, uint64_t r, int t, int w,
                          const T (&std)[n], T (&out)[n]) {
  constexpr int kPer = DrawBlock<T>::kPer;
#pragma unroll
  for (int k = 0; k < (n + kPer - 1) / kPer; ++k) {
    T z[kPer];
    draw_block(seed, r, t, w, k, z);
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      if (k * kPer + i < n) out[k * kPer + i] = std[k * kPer + i] * z[i];
  }
}

// x += std (.) the n unit normals of (r, t, w), each component ONE explicit
// fma: no contraction can change it, so two kernels that form the sum from the
// same x agree bit for bit (the hand-over of an MPC trial and its first
// observation, mpc_advance_noise.hip).
PDDP_DEV float fma_of(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}
PDDP_DEV double fma_of(double a, double b, double c) {
  return __builtin_fma(a, b, c);
}
// (the two halves: the draws depend on no state and may be made ahead of the
// chain that ends in the sum)
template <typename T, int n>
PDDP_DEV void draw_units(uint64_t seed, uint64_t r, int t, int w, T (&out)[n]) {
  constexpr int kPer = DrawBlock<T>::kPer;
#pragma unroll
  for (int k = 0; k < (n + kPer - 1) / kPer; ++k) {
    T z[kPer];
    draw_block(seed, r, t, w, k, z);
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      if (k * kPer + i < n) out[k * kPer + i] = z[i];
  }
}
template <typename T, int n>
PDDP_DEV void add_scaled(const T* std, const T (&z)[n], T (&x)[n]) {
#pragma unroll
  for (int j = 0; j < n; ++j) x[j] = fma_of(std[j], z[j], x[j]);
}
template <typename T, int n>
PDDP_DEV void draw_added(uint64_t seed, uint64_t r, int t, int w, const T* std,
                         T (&x)[n]) {
  T z[n];
  draw_units<T, n>(seed, r, t, w, z);
  add_scaled<T, n>(std, z, x);
}

// the noise of a launch of rollouts
template <typename T>
struct NoiseArgs {
  const T* w_std;  // [n]; NULL exactly when the kernel's PROC is false
  const T* v_std;  // [n]; NULL exactly when the kernel's OBS is false
  uint64_t seed, offset;
};

}  // namespace pddp
