// riccati.hip - C-ABI entry points of the backward Riccati sweep
// (pddp/controllers/ilqr.py:529-674) and their dispatch.
#include "riccati_generic.hpp"
#include "riccati_n4.hpp"
#include "riccati_mfma16.hpp"
#include "riccati_mfma32.hpp"
#include "riccati_mfma32s.hpp"

namespace pddp {

// riccati_quad.hip (its own translation unit: compiled without SLP pairing)
int launch_n4_quad_f32(const RiccatiArgs<float>& a, hipStream_t st, bool fast,
                       bool loop_always);
int launch_n4_quad_f64(const RiccatiArgs<double>& a, hipStream_t st, bool fast,
                       bool loop_always);
static int launch_n4_quad(const RiccatiArgs<float>& a, hipStream_t st, bool f,
                          bool loop_always = false) {
  return launch_n4_quad_f32(a, st, f, loop_always);
}
static int launch_n4_quad(const RiccatiArgs<double>& a, hipStream_t st, bool f,
                          bool loop_always = false) {
  return launch_n4_quad_f64(a, st, f, loop_always);
}

template <typename T, int NMAX, int M>
static int launch_generic(const RiccatiArgs<T>& a, hipStream_t st) {
  PDDP_LAUNCH((riccati_generic_kernel<T, NMAX, M>), dim3(a.B), dim3(kWave), 0,
              st, a);
  return launch_status();
}

template <typename T, int M>
static int dispatch_nmax(const RiccatiArgs<T>& a, hipStream_t st) {
  if (a.n <= 8) return launch_generic<T, 8, M>(a, st);
  if (a.n <= 16) return launch_generic<T, 16, M>(a, st);
  if (a.n <= 32) return launch_generic<T, 32, M>(a, st);
  // n > 32: four wavefronts per trajectory, LDS sized for this n.  The CU has
  // 160 KB; f32 reaches n = 114, f64 n = 80.
  const size_t bytes = riccati_lds_elems(a.n, M) * sizeof(T);
  if (bytes > 160 * 1024) return PDDP_E_UNSUPPORTED;
  return launch_dyn_lds(riccati_large_kernel<T, M>, dim3(a.B),
                        dim3(kLargeThreads), bytes, st, a);
}

template <typename T>
static int riccati_backward_impl(int B, int N, int n, int m, const T* rec,
                                 const T* u_min, const T* u_max,
                                 const double* reg, int branch,
                                 const uint8_t* active, T* gains,
                                 int32_t* status, void* stream, int variant) {
  if (B <= 0 || N <= 0 || n <= 0 || m <= 0 || !rec || !reg || !gains ||
      !status)
    return PDDP_E_BADARG;
  if ((u_min == nullptr) != (u_max == nullptr)) return PDDP_E_BADARG;
  if (branch != PDDP_BRANCH_EIG && branch != PDDP_BRANCH_CHOLESKY)
    return PDDP_E_BADARG;
  RiccatiArgs<T> a{B, N, n, rec, u_min, u_max, reg, branch, active, gains,
                   status};
  hipStream_t st = (hipStream_t)stream;
  // variant: 0 auto; 1 generic kernel (any n, m <= 4, IEEE throughout);
  //          n = 4, m = 1: 6 / 7 sixteen lanes per trajectory
  //          (riccati_n4.hpp; IEEE division / v_rcp + v_sqrt, f32), BoxQP in
  //          closed form with the reference's loop as fall-back; 16 / 17 four
  //          lanes per trajectory (riccati_n4_quad.hpp), 18 = 16 with every
  //          BoxQP through the reference's loop;
  //          14 / 15 the matrix-core kernels for n <= 30, m = 1
  //          (riccati_mfma16.hpp / riccati_mfma32.hpp; fp64: the 16x16 form
  //          for n <= 14, variant 14); 26 / 27: 15 <= n <= 30, m = 1, f32,
  //          eig-clamp branches with one trajectory's step split over two
  //          wavefronts (riccati_mfma32s.hpp).
  //          auto: n = 4, m = 1: f32 from 12288 trajectories on -> 17,
  //          otherwise 7 (f32) / 6 (f64); other shapes with m = 1, n <= 30
  //          (f64: n <= 14) -> 15 / 14 (f32, 15 <= n <= 30, eig-clamp
  //          branches: 27); everything else -> 1
  if (variant == 26 || variant == 27) {
    if constexpr (sizeof(T) == 4) {
      if (m != 1) return PDDP_E_UNSUPPORTED;
      return launch_mfma32s(a, st, variant == 27);
    } else {
      return PDDP_E_UNSUPPORTED;
    }
  }
  if (variant == 14 || variant == 15 ||
      (variant == 0 && m == 1 && n != 4 && n <= (sizeof(T) == 4 ? 30 : 14))) {
    if (m != 1) return PDDP_E_UNSUPPORTED;
    if constexpr (sizeof(T) == 4) {
      if (n <= 14) return launch_mfma16<T>(a, st, variant != 14);
      // auto, eig-clamp branches: one trajectory's step on two wavefronts
      // (riccati_mfma32s.hpp: 421 -> 280-295 us at configs[3]'s 1024
      // trajectories per GPU, 1385 -> 1217 at 4096); its two-barrier form
      // while a CU holds at most four trajectories
      if (variant == 0 && branch != PDDP_BRANCH_CHOLESKY)
        return launch_mfma32s(a, st, true);
      return launch_mfma32(a, st, variant != 14);
    } else {
      if (variant == 15 || n > 14) return PDDP_E_UNSUPPORTED;
      return launch_mfma16<T>(a, st, false);
    }
  }
  if (variant >= 2 && !(n == 4 && m == 1)) return PDDP_E_UNSUPPORTED;
  //          16 / 17: four lanes per trajectory, sixteen trajectories per
  //          wavefront (riccati_n4_quad.hpp; IEEE / approximate division),
  //          all four branches
  //          18: variant 16 with every BoxQP through the reference's loop
  //          (bounded branches; the closed form's A/B twin)
  if (variant == 16 || variant == 17)
    return launch_n4_quad(a, st, variant == 17);
  if (variant == 18) return launch_n4_quad(a, st, false, true);
  if (variant != 0 && variant != 1 && variant != 6 && variant != 7)
    return PDDP_E_BADARG;

  if (variant == 0 && n == 4 && m == 1 && sizeof(T) == 4 && B >= 12288) {
    // large batches: four lanes per trajectory (riccati_n4_quad.hpp) - a
    // third of the issue slots per trajectory-step of the kernel below.
    // Measured inside the fit loop (bench.py --batch B): 66 / 90 / 98 us at
    // B = 8192 / 12288 / 16384 against 67 / 92 / 128 for the kernel below
    // (alone on records that sit in the Infinity Cache: 64 / 66 / 86 against
    // 69 / 90 / 131)
    return launch_n4_quad(a, st, true);
  }
  // (Rounds 2-4 carried three more formulations of this 4 x 4 recursion ON
  // RECORDS - the step split over two wavefronts, 8 / 9; the quad mapping on
  // three wavefronts, 20 / 21; the deferred rank-one form on four, 24 / 25:
  // 40 against 56 us at B = 4096 - each the default of some branch / batch.
  // Since the cartpole's rounds take their sweep from the nominal
  // (riccati_n4_elem.hpp, f32 and f64, 26 us inside round_n4.hip) the sweep
  // on records serves the reference-signature `backward()`, the Cholesky /
  // unbounded branches and plugin models of this shape; the three were
  // retired in round 5, docs/history.)
  if (variant != 1 && n == 4 && m == 1) {
    const bool fast = (variant == 0 || variant == 7) && sizeof(T) == 4;
    return launch_n4<T>(a, st, fast);
  }
  switch (m) {
    case 1: return dispatch_nmax<T, 1>(a, st);
    case 2: return dispatch_nmax<T, 2>(a, st);
    case 3: return dispatch_nmax<T, 3>(a, st);
    case 4: return dispatch_nmax<T, 4>(a, st);
  }
  return PDDP_E_UNSUPPORTED;
}

// Stand-alone batched BoxQP for m <= 4 (utils/constraint.py:150-266): one lane
// per problem, the routine of the generic sweep kernel (gains.hpp `boxqp`).
template <typename T, int M>
__global__ __launch_bounds__(kWave) void boxqp_kernel(
    int count, const T* x0, const T* Q, const T* c, const T* lower,
    const T* upper, T* x, int32_t* result, T* Ufree, uint8_t* free_mask) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  T x0r[M], Qr[M * M], cr[M], lo[M], hi[M], xr[M], U[M * M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    x0r[i] = x0[(size_t)p * M + i];
    cr[i] = c[(size_t)p * M + i];
    lo[i] = lower[(size_t)p * M + i];
    hi[i] = upper[(size_t)p * M + i];
  }
#pragma unroll
  for (int i = 0; i < M * M; ++i) Qr[i] = Q[(size_t)p * M * M + i];
  unsigned free_bits = 0u;
  const int res = boxqp<T, M>(x0r, Qr, cr, lo, hi, xr, U, free_bits);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    x[(size_t)p * M + i] = xr[i];
    free_mask[(size_t)p * M + i] = (free_bits >> i) & 1u;
  }
#pragma unroll
  for (int i = 0; i < M * M; ++i) Ufree[(size_t)p * M * M + i] = U[i];
  result[p] = res;
}

template <typename T>
static int boxqp_impl(int count, int m, const T* x0, const T* Q, const T* c,
                      const T* lower, const T* upper, T* x, int32_t* result,
                      T* Ufree, uint8_t* free_mask, void* stream) {
  if (count <= 0 || m <= 0 || !x0 || !Q || !c || !lower || !upper || !x ||
      !result || !Ufree || !free_mask)
    return PDDP_E_BADARG;
  const dim3 grid((count + kWave - 1) / kWave), block(kWave);
  hipStream_t st = (hipStream_t)stream;
#define PDDP_BOXQP_CASE(M)                                                   \
  case M:                                                                    \
    PDDP_LAUNCH((boxqp_kernel<T, M>), grid, block, 0, st, count, x0, Q, c,   \
                lower, upper, x, result, Ufree, free_mask);                  \
    return launch_status();
  switch (m) {
    PDDP_BOXQP_CASE(1)
    PDDP_BOXQP_CASE(2)
    PDDP_BOXQP_CASE(3)
    PDDP_BOXQP_CASE(4)
  }
#undef PDDP_BOXQP_CASE
  return PDDP_E_UNSUPPORTED;
}

}  // namespace pddp

extern "C" {

int pddp_boxqp_f32(int count, int m, const float* x0, const float* Q,
                   const float* c, const float* lower, const float* upper,
                   float* x, int32_t* result, float* Ufree,
                   uint8_t* free_mask, void* stream) {
  return pddp::boxqp_impl<float>(count, m, x0, Q, c, lower, upper, x, result,
                                 Ufree, free_mask, stream);
}
int pddp_boxqp_f64(int count, int m, const double* x0, const double* Q,
                   const double* c, const double* lower, const double* upper,
                   double* x, int32_t* result, double* Ufree,
                   uint8_t* free_mask, void* stream) {
  return pddp::boxqp_impl<double>(count, m, x0, Q, c, lower, upper, x, result,
                                  Ufree, free_mask, stream);
}

#ifdef PDDP_QP_STATS
int pddp_debug_qp_stats(unsigned long long* out, int reset) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::n4::g_qp_stats), 32);
  if (reset) {
    unsigned long long z[4] = {0, 0, 0, 0};
    hipMemcpyToSymbol(HIP_SYMBOL(pddp::n4::g_qp_stats), z, 32);
  }
  return 0;
}
#endif

int pddp_riccati_backward_f32(int B, int N, int n, int m, const float* rec,
                              const float* u_min, const float* u_max,
                              const double* reg, int branch,
                              const uint8_t* active, float* gains,
                              int32_t* status, void* stream) {
  return pddp::riccati_backward_impl<float>(B, N, n, m, rec, u_min, u_max, reg,
                                            branch, active, gains, status,
                                            stream, 0);
}
int pddp_riccati_backward_f64(int B, int N, int n, int m, const double* rec,
                              const double* u_min, const double* u_max,
                              const double* reg, int branch,
                              const uint8_t* active, double* gains,
                              int32_t* status, void* stream) {
  return pddp::riccati_backward_impl<double>(B, N, n, m, rec, u_min, u_max,
                                             reg, branch, active, gains,
                                             status, stream, 0);
}
/* Same sweep through a chosen kernel variant (A/B tests): 0 auto,
 * 1 the generic kernel, 6 / 7 and 16 / 17 / 18 the n = 4 sweeps, 14 / 15 the
 * matrix-core kernels, 26 / 27 their two-wavefront split - the list at
 * riccati_backward_impl. */
int pddp_riccati_backward_variant_f32(int B, int N, int n, int m,
                                      const float* rec, const float* u_min,
                                      const float* u_max, const double* reg,
                                      int branch, const uint8_t* active,
                                      float* gains, int32_t* status,
                                      void* stream, int variant) {
  return pddp::riccati_backward_impl<float>(B, N, n, m, rec, u_min, u_max, reg,
                                            branch, active, gains, status,
                                            stream, variant);
}
int pddp_riccati_backward_variant_f64(int B, int N, int n, int m,
                                      const double* rec, const double* u_min,
                                      const double* u_max, const double* reg,
                                      int branch, const uint8_t* active,
                                      double* gains, int32_t* status,
                                      void* stream, int variant) {
  return pddp::riccati_backward_impl<double>(B, N, n, m, rec, u_min, u_max,
                                             reg, branch, active, gains,
                                             status, stream, variant);
}

/* The sweep with two HIP events attached to its dispatch (bench.py's roofline
 * leg): elapsed(start, stop) is the kernel's own duration. */
int pddp_riccati_backward_timed_f32(int B, int N, int n, int m,
                                    const float* rec, const float* u_min,
                                    const float* u_max, const double* reg,
                                    int branch, const uint8_t* active,
                                    float* gains, int32_t* status,
                                    void* stream, int variant, void* start,
                                    void* stop) {
  pddp::launch_events() = {(hipEvent_t)start, (hipEvent_t)stop};
  const int rc = pddp::riccati_backward_impl<float>(
      B, N, n, m, rec, u_min, u_max, reg, branch, active, gains, status,
      stream, variant);
  pddp::launch_events() = pddp::LaunchEvents();
  return rc;
}
int pddp_riccati_backward_timed_f64(int B, int N, int n, int m,
                                    const double* rec, const double* u_min,
                                    const double* u_max, const double* reg,
                                    int branch, const uint8_t* active,
                                    double* gains, int32_t* status,
                                    void* stream, int variant, void* start,
                                    void* stop) {
  pddp::launch_events() = {(hipEvent_t)start, (hipEvent_t)stop};
  const int rc = pddp::riccati_backward_impl<double>(
      B, N, n, m, rec, u_min, u_max, reg, branch, active, gains, status,
      stream, variant);
  pddp::launch_events() = pddp::LaunchEvents();
  return rc;
}

int pddp_boxqp_m1_f32(int count, const float* x0, const float* Q,
                      const float* c, const float* lower, const float* upper,
                      float* x, int32_t* result, uint8_t* free_mask,
                      void* stream) {
  if (count <= 0 || !x0 || !Q || !c || !lower || !upper || !x || !result ||
      !free_mask)
    return PDDP_E_BADARG;
  PDDP_LAUNCH((pddp::n4::boxqp1_kernel<float, false>),
                     dim3((count + 3) / 4), dim3(pddp::kWave), 0,
                     (hipStream_t)stream, count, x0, Q, c, lower, upper, x,
                     result, free_mask);
  return pddp::launch_status();
}
int pddp_boxqp_m1_f64(int count, const double* x0, const double* Q,
                      const double* c, const double* lower,
                      const double* upper, double* x, int32_t* result,
                      uint8_t* free_mask, void* stream) {
  if (count <= 0 || !x0 || !Q || !c || !lower || !upper || !x || !result ||
      !free_mask)
    return PDDP_E_BADARG;
  PDDP_LAUNCH((pddp::n4::boxqp1_kernel<double, false>),
                     dim3((count + 3) / 4), dim3(pddp::kWave), 0,
                     (hipStream_t)stream, count, x0, Q, c, lower, upper, x,
                     result, free_mask);
  return pddp::launch_status();
}

}  // extern "C"

#ifdef PDDP_WG_TIMELINE
extern "C" int pddp_debug_mfma32s_clock(long long* out) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::m32s::g_mfma32s_clock),
                            sizeof(long long) * 2);
  return 0;
}
#endif
