// riccati_mfma16.hpp - backward Riccati sweep for n + 1 <= 15, m = 1 on the
// matrix cores: fp32 (v_mfma_f32_16x16x4_f32: exact f32, bitwise an fmaf
// chain) and fp64 (v_mfma_f64_16x16x4_f64), both gain branches (eig clamp ilqr.py:629-672, V_zz-regularised
// Cholesky :587-625), bounded or not.  The DEFAULT
// (Cholesky) encoding of cartpole is n = 14: BASELINE.json configs[2]'s sweep,
// 744 MB per launch at B = 4096, N = 100.
//
// One wavefront per trajectory; the whole step is TWO 16x16x16 products on
// augmented matrices and stays in registers:
//   F~ = [F_z | F_u | 0]            (rows k < n, column n = F_u)
//   X  = V F~                       A operand = V, B operand = F~
//   X[:, 15] := V_z                 (column 15 is free: n + 1 <= 15)
//   Q~ = L~ + F~^T X                A operand = F~^T, B operand = X
// with L~ = [[L_zz, L_uz^T, L_z], [L_uz, L_uu, L_u]]:  Q~ holds Q_zz (raw), Q_uz
// (row n), Q_uu ([n][n]) and in column 15 Q_z, Q_u (ilqr.py:489-526) - every
// second- AND first-order term of the step from eight MFMA instructions.
// Why nothing moves between lanes:
//   * the C/D layout (column on the lane, rows 4g + r in register r of lane
//     group g) of V' is, V' being symmetric, exactly the A operand of the next
//     X = V F~ when k-slab r of lane group g is taken to be k = 4g + r;
//   * with the same k assignment the D registers of X are the B operand of
//     the second product, and the four F~ words a lane reads from the record
//     (F~[4g + r][j], j = lane & 15) serve as B operand of the first product
//     AND as A operand (F~^T[i][k], i = lane & 15) of the second.
// One LDS round trip per step remains: the transpose for 0.5 (Q + Q^T) and the
// broadcast of Q_uz for the rank-one value update
//   V' = sym(Q_zz) + c Q_uz^T Q_uz,  V_z' = Q_z + Q_uz^T w
// (c, w from the scalar BoxQP; riccati_n4_pipe.hpp).  Records stream HBM -> LDS
// by full-wave LDS-DMA, R slots ahead.
// fp64: the f64 instruction's C/D layout puts row g + 4 r (not 4 g + r) in
// register r of lane group g; with the k-slab of MFMA r taken as k = g + 4 r
// everything above holds unchanged (`Tile<T>::row`).
// Shared texts, each written once and included (riccati_mfma16_nominal.hpp
// includes the same four): mfma_operand.inc (which record word an entry of
// F~ / L~ reads), mfma16_products.inc (both products, row n, the regularised
// row), mfma_gain_step.inc (the scalar gains; also riccati_mfma32.hpp and
// riccati_mfma32s.hpp), mfma16_value_update.inc (V', V_z' from the tile).  The
// step below keeps what is this kernel's own: the gathers at an immediate slot
// offset, the tile's vector store, the wait for and the refill of the slot.
#pragma once

#include "riccati_n4.hpp"

namespace pddp {
namespace m16 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kWaves = 4;  // independent trajectories (wavefronts) per workgroup
constexpr int kRing = 3;   // record slots in flight per wavefront
constexpr int kMaxDma = 4; // LDS-DMA instructions per record (64 x 16 B each)

// the 16x16x4 instruction of each type: accumulator vector, the matrix row
// (= k-slab) held by register r of lane group g, and where row n sits
template <typename T> struct Tile;
template <> struct Tile<float> {
  using Acc = f32x4;
  PDDP_DEV static int row(int g, int r) { return 4 * g + r; }
  PDDP_DEV static int group_of(int k) { return k >> 2; }
  PDDP_DEV static int reg_of(int k) { return k & 3; }
  PDDP_DEV static Acc mma(float x, float y, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0);
  }
  PDDP_DEV static float read_lane(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
  }
};
template <> struct Tile<double> {
  using Acc = f64x4;
  PDDP_DEV static int row(int g, int r) { return g + 4 * r; }
  PDDP_DEV static int group_of(int k) { return k & 3; }
  PDDP_DEV static int reg_of(int k) { return k >> 2; }
  PDDP_DEV static Acc mma(double x, double y, Acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c, 0, 0, 0);
  }
  PDDP_DEV static double read_lane(double v, int l) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  }
};

// NDMA: LDS-DMA instructions per record, chosen so that a slot (NDMA * 64
// chunks of 16 bytes) has strictly more chunks than the record: the slot's
// padding is zeroed once, the last DMA instruction's lanes past the record
// stay out, and operand entries outside the matrices read the first padding
// word - no per-entry zero selects; the slot stride is a compile-time
// constant, so that a step instantiated per ring slot gathers its operands
// with immediate offsets on addresses computed once (round 3: 141 -> 109
// vector instructions per step; at B = 4096 this kernel's four wavefronts per
// SIMD are bound by instruction issue, not by HBM).
template <typename T, bool BOUNDED, bool FAST, bool CHOL, int NDMA>
__global__ __launch_bounds__(kWave * kWaves) void riccati_mfma16_kernel(
    RiccatiArgs<T> a) {
  constexpr int slot_words = NDMA * kWave * (16 / (int)sizeof(T));
  using TL = Tile<T>;
  using Acc = typename TL::Acc;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  // per wave: kRing record slots, the 16x16 transpose tile; shared: step sizes
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int per_wave = kRing * slot_words + 256;
  T* ring = smem + wave * per_wave;
  T* tile = ring + kRing * slot_words;
  T* ls_tail = smem + kWaves * per_wave;
  if constexpr (BOUNDED) {
    for (int q = threadIdx.x; q < n4::kLsSteps; q += kWave * kWaves)
      ls_tail[q] = (T)n4::kLs.v[q];
  }
  const T lstep0 = (T)n4::kLs.v[lane & 15];
  __syncthreads();

  const int b = blockIdx.x * kWaves + wave;
  if (b >= a.B) return;
  if (a.active != nullptr && a.active[b] == 0) return;
  const int n = a.n, N = a.N;
  const RecLayout lay(n, 1);
  const int S = lay.stride;
  const int g = lane >> 4, j = lane & 15;
  // this wavefront's slots: zero the padding behind the record, once
  for (int sl = 0; sl < kRing; ++sl)
    for (int wd = S + lane; wd < slot_words; wd += kWave)
      ring[sl * slot_words + wd] = T(0);
  const T reg = (T)a.reg[b];
  T umin = T(0), umax = T(0);
  if constexpr (BOUNDED) { umin = a.u_min[0]; umax = a.u_max[0]; }

  // ---- word offsets of this lane's operands inside a record (S: the first
  // word of the zeroed padding)
  int oF[4], oL[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = TL::row(g, r);  // F~ row / L~ row
#define PDDP_OPERAND_F oF[r]
#define PDDP_OPERAND_L oL[r]
#define PDDP_OPERAND_JZ 15
#include "mfma_operand.inc"
  }
  // Cholesky branch (ilqr.py:587-625): Q_uu, Q_uz once more with V + reg I,
  // i.e. + reg f^T F~ (row n of F~^T F~): this lane's share needs f[4g + r]
  int oFf[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    oFf[r] = (TL::row(g, r) < n) ? lay.oFu + TL::row(g, r) : S;

  // ---- record DMA: chunk q of 16 bytes -> lane q % 64 of instruction q / 64
  const char* rec_b = reinterpret_cast<const char*>(
      a.rec + (size_t)b * (size_t)(N + 1) * S);
  const int chunks = S * (int)sizeof(T) / 16;  // S is a multiple of 4 words
  // (padding lanes past the record re-load an early chunk into the slot's pad)
  // (the launcher picked NDMA with (NDMA - 1) * 64 < chunks < NDMA * 64: the
  // last instruction's lanes past the record stay out of it)
  uint32_t qoff[NDMA];
#pragma unroll
  for (int i = 0; i < NDMA; ++i) qoff[i] = (uint32_t)(lane + i * kWave) * 16u;
  const bool in_tail = lane + (NDMA - 1) * kWave < chunks;
  auto dma = [&](int slot, int t) {
    const int tt = t < 0 ? 0 : t;
    const uint32_t base = (uint32_t)tt * (uint32_t)(S * sizeof(T));
    const uint32_t lbase =
        __builtin_amdgcn_readfirstlane(n4::lds_addr(ring + slot * slot_words));
#pragma unroll
    for (int i = 0; i < NDMA - 1; ++i)
      n4::lds_dma16(rec_b, base + qoff[i], lbase + i * kWave * 16);
    if (in_tail)
      n4::lds_dma16(rec_b, base + qoff[NDMA - 1],
                    lbase + (NDMA - 1) * kWave * 16);
  };

  // ---- terminal value function in the accumulator layout (ilqr.py:581-583)
  T V[4], Vz[4];
  {
    const T* term = a.rec + ((size_t)b * (size_t)(N + 1) + N) * S;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = TL::row(g, r);
      V[r] = (k < n && j < n) ? term[lay.oLzz + k * n + j] : T(0);
      Vz[r] = (k < n) ? term[lay.oLz + k] : T(0);
    }
  }
  for (int s = 0; s < kRing; ++s) dma(s, N - 1 - s);
  n4::wait_vmcnt<0>();  // (also the terminal loads above)

  T* gains_b = a.gains + (size_t)b * (size_t)N * lay.gstride;
  T kprev = T(0);
  int status = PDDP_BWD_OK;
  // gather addresses of slot 0, computed once: the step is instantiated per
  // ring slot and reaches the others through the read's immediate offset
  const T* pF[4];
  const T* pL[4];
  const T* pFf[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pF[r] = ring + oF[r];
    pL[r] = ring + oL[r];
    pFf[r] = ring + oFf[r];
  }
  const T* pU = ring + lay.oU;
  // (V_z travels as column 15 of X's initial value: zero in the other lanes)
#pragma unroll
  for (int r = 0; r < 4; ++r) Vz[r] = (j == 15) ? Vz[r] : T(0);
  auto step = [&](const int t, auto slot_c) {
    constexpr int slot = decltype(slot_c)::value;
    constexpr int so = slot * slot_words;
    // record t has landed once at most (kRing - 1) younger {DMA x NDMA, store}
    // groups are outstanding
    n4::wait_vmcnt<(kRing - 1) * (NDMA + 1)>();
    T Fa[4], La[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Fa[r] = pF[r][so];
      La[r] = pL[r][so];
    }
    const T Un = BOUNDED ? pU[so] : T(0);
#define PDDP_M16_F(r) pFf[r][so]
#define PDDP_M16_ROW_N_HERE
#include "mfma16_products.inc"
    // transpose tile: T[col][row] = Q~[row][col]; row 15 (free: n + 1 <= 15)
    // carries Q_uz_reg
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<f32x4*>(tile + j * 16 + 4 * g) = Q;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) tile[j * 16 + TL::row(g, r)] = Q[r];
    }
    if constexpr (CHOL) {
      if (g == gn) tile[j * 16 + 15] = rowg;
    }

#define PDDP_GAIN_ROW g == gn
#define PDDP_GAIN_COL j
#define PDDP_GAIN_KROW rowg
#include "mfma_gain_step.inc"
    const T c = sE * (sE * Quu - T(2));
    const T w = kt - sE * (Qu + Quu * kt);
    const T c2 = sE * sE * Quu;        // Cholesky branch: K = -sE Q_uz_reg
    const T wz = sE * (Qu + Quu * kt);
    // ---- k, K of step t: lanes of row n hold Q_uz[j] (j < n), lane j = n: k
    {
      const T val = (j < n) ? -(sE * rowg) : kt;
      T* dst = gains_b + (size_t)t * lay.gstride + (j < n ? 1 + j : 0);
      if (g == gn && j <= n) *dst = val;
    }
    // this slot is consumed: refill it, kRing steps further down the sweep
    dma(slot, t - kRing);

#include "mfma16_value_update.inc"
  };
  // record tau lives in slot (N - 1 - tau) % kRing
  int t = N - 1;
  static_assert(kRing == 3 || kRing == 4, "");
  for (; t >= kRing - 1; t -= kRing) {
    step(t, std::integral_constant<int, 0>{});
    step(t - 1, std::integral_constant<int, 1>{});
    step(t - 2, std::integral_constant<int, 2>{});
    if constexpr (kRing == 4) step(t - 3, std::integral_constant<int, 3>{});
  }
  if (t >= 0) step(t, std::integral_constant<int, 0>{});
  if (t >= 1) step(t - 1, std::integral_constant<int, 1>{});
  if constexpr (kRing == 4) {
    if (t >= 2) step(t - 2, std::integral_constant<int, 2>{});
  }
  n4::wait_vmcnt<0>();
  if (j == 0 && g == 0) a.status[b] = status;
}

}  // namespace m16

// n + 1 <= 15, m = 1; PDDP_E_UNSUPPORTED otherwise (fp64: IEEE division only)
template <typename T>
static int launch_mfma16(const RiccatiArgs<T>& a, hipStream_t st,
                         bool fast_math) {
  if (a.n + 1 > 15) return PDDP_E_UNSUPPORTED;
  const bool chol = a.branch == PDDP_BRANCH_CHOLESKY;
  const RecLayout lay(a.n, 1);
  const int chunks = lay.stride * (int)sizeof(T) / 16;
  // strictly more DMA lanes than chunks: the slot keeps a zeroed padding
  const int ndma = chunks / kWave + 1;
  if (ndma > m16::kMaxDma) return PDDP_E_UNSUPPORTED;
  const int slot_words = ndma * kWave * (16 / (int)sizeof(T));
  const size_t lds = sizeof(T) * ((size_t)m16::kWaves *
                                      (m16::kRing * slot_words + 256) +
                                  n4::kLsSteps);
  const dim3 grid((a.B + m16::kWaves - 1) / m16::kWaves),
      block(kWave * m16::kWaves);
  const bool bounded = a.u_min != nullptr;
#define PDDP_M16N(Bd, F, C, ND)                                                \
  PDDP_LAUNCH((m16::riccati_mfma16_kernel<T, Bd, F, C, ND>), grid, block, lds, \
              st, a)
#define PDDP_M16C(Bd, F, C)                                                    \
  do {                                                                         \
    switch (ndma) {                                                            \
      case 1: PDDP_M16N(Bd, F, C, 1); break;                                   \
      case 2: PDDP_M16N(Bd, F, C, 2); break;                                   \
      case 3: PDDP_M16N(Bd, F, C, 3); break;                                   \
      default: PDDP_M16N(Bd, F, C, 4); break;                                  \
    }                                                                          \
  } while (0)
#define PDDP_M16(Bd, F)                                                        \
  do {                                                                         \
    if (chol) PDDP_M16C(Bd, F, true);                                          \
    else PDDP_M16C(Bd, F, false);                                              \
  } while (0)
  if constexpr (sizeof(T) == 4) {
    if (bounded) { if (fast_math) PDDP_M16(true, true); else PDDP_M16(true, false); }
    else { if (fast_math) PDDP_M16(false, true); else PDDP_M16(false, false); }
  } else {
    if (bounded) PDDP_M16(true, false); else PDDP_M16(false, false);
  }
#undef PDDP_M16C
#undef PDDP_M16N
#undef PDDP_M16
  return launch_status();
}

}  // namespace pddp
