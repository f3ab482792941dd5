// mppi.hip - sampled shooting with a softmin-weighted (MPPI) update of the base
// sequence: shoot.hip's S perturbed candidates per trajectory, costed by the
// same law, and instead of the single cheapest one the weighted mean of ALL the
// perturbations added to the base, that sequence rolled out and costed inside
// the launch (pddp_mppi_*, pddp_mppi_batch_*, ILQRSolver.mppi).  The reference
// has no counterpart: include/pddp_hip.h states the law, DESIGN.md 3.4n the
// kernel.
//
//   Jc[b][s], best[b], J_best[b]:  pddp_shoot_*'s, word for word
//   w_s   = exp(-(Jc[b][s] - J_best[b]) / lam[b])   finite Jc, else 0
//   eta   = sum_s w_s;   W[b][s] = w_s / eta
//   ebar_t = (sum_{s>=1} w_s e_{s,t}) / eta         e: the raw AR(1) value
//   Uw[b][t] = clamp(fma(a_std, ebar_t, U[b][t]));  Zw, J_w: its rollout
//
// shoot.hip, closed_loop.hip and their texts are as they were: this unit
// carries its own copy of the candidate rollout (the Makefile's note on
// contraction: a loop moved into a device function changes the instructions of
// the kernels that use it) and uses draw_units, closed_loop_geometry, the
// (J, s) order of shoot's take_lower and models.hpp as they are.
//
// Three passes over the same ceil(S / G) turns of the lane group:
//   1. the candidates' rollouts and the argmin - shoot's;
//   2. eta: every lane re-reads its own Jc and sums its weights in s order,
//      then the group (below);
//   3. the draws again - Philox and the AR(1), no dynamics: at every step t
//      the m products w_s e_{s,t} are summed over the group, the turns in
//      their order by ONE lane per trajectory, which in the last turn has the
//      whole sum, forms Uw[b][t] and steps the weighted rollout with it.
// A sum over the group: a butterfly over the group's lanes of a wavefront
// (both partners form the same sum, idle lanes add 0), then the workgroup's
// wavefronts in their order through LDS.  Every shuffle and barrier sits under
// launch-uniform control flow: the turn count, N and m are uniform, lanes
// outside the batch, masked or without a weight take part with zeros.  The
// order depends on S alone, never on b or B.  No atomics.
#include <cmath>
#include <limits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"

namespace pddp {

constexpr int kMppiStream = 2;  // (shoot's: the candidates are shoot's)

template <typename T>
struct MppiArgs {
  int B, N, S, G;
  const T* z0;     // [B][n]
  const T* U;      // [B][N][m]
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the shared problem
  const T* u_min;
  const T* u_max;
  const T* a_std;  // [m]
  const T* lam;    // [B]
  T beta, gamma;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;          // [B][S]
  int32_t* best;  // [B]
  T* J_best;      // [B] or NULL
  T* W;           // [B][S] or NULL
  T* J_w;         // [B]
  T* Z_out;       // [B][N+1][n], with U_out [B][N][m]: both or neither
  T* U_out;
};

// shoot.hip's take_lower: (J, s) ordered lexicographically; (+inf, -1) is "no
// finite cost" and loses against every candidate, whose J is finite.
template <typename T>
PDDP_DEV void mppi_take_lower(T& J, int& s, T oJ, int os) {
  const bool take = oJ < J || (oJ == J && os < s);
  J = take ? oJ : J;
  s = take ? os : s;
}

PDDP_DEV float exp_of(float x) { return expf(x); }
PDDP_DEV double exp_of(double x) { return exp(x); }

// w_s: 1 for the best candidate (the exponent is -0), 0 for a cost that is
// not finite.  The difference and the quotient are rounded one by one.
template <typename T>
PDDP_DEV T softmin_weight(T J, T J_best, T lam) {
  const T arg = -((J - J_best) / lam);
  return is_finite(J) ? exp_of(arg) : T(0);
}

// The sums of v[0..K) over a trajectory's lane group, on every lane of the
// group: the butterfly, then (one trajectory over several wavefronts) the
// wavefronts in their order through `part` [K][waves], read by every lane
// after ONE barrier.  The caller alternates between two `part` blocks from one
// sum to the next, so a wavefront that runs ahead writes the block nobody
// still reads.
template <typename T, int K>
PDDP_DEV void group_sum(T (&v)[K], int span, bool multi,
                        T (&part)[K][kClosedLoopThreads / kWave]) {
  for (int off = 1; off < span; off <<= 1) {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] += __shfl_xor(v[j], off);
  }
  if (multi) {
    const int tid = threadIdx.x;
    if (tid % kWave == 0) {
#pragma unroll
      for (int j = 0; j < K; ++j) part[j][tid / kWave] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; ++j) {
      v[j] = part[j][0];
      for (int w = 1; w < (int)blockDim.x / kWave; ++w) v[j] += part[j][w];
    }
  }
}

template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_kernel(
    ProblemT<T> shared, MppiArgs<T> a) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int kWaves = kClosedLoopThreads / kWave;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const bool multi = blockDim.x > kWave;  // one trajectory, several wavefronts
  const int span = G < kWave ? G : kWave;

  // the problem of trajectory b, as shoot_kernel holds it
  ProblemT<T> P = shared;
  T umin[m], umax[m], astd[m], z0[n];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
#pragma unroll
  for (int j = 0; j < n; ++j) z0[j] = T(0);
  T lam = T(1);
  if (live) {
    if (a.table != nullptr) {
      const T* row = a.table + (size_t)b * PDDP_BATCH_ROW;
      P.dt = row[PDDP_BATCH_PARAMS];
#pragma unroll
      for (int i = 0; i < kModelParamCount<MODEL> - 1; ++i)
        P.p[i] = row[PDDP_BATCH_PARAMS + 1 + i];
#pragma unroll
      for (int i = 0; i < D::na; ++i) P.goal[i] = row[PDDP_BATCH_X_GOAL + i];
#pragma unroll
      for (int i = 0; i < D::m; ++i) P.ugoal[i] = row[PDDP_BATCH_U_GOAL + i];
    }
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
      astd[r] = a.a_std[r];
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z0[j] = a.z0[(size_t)b * n + j];
    lam = a.lam[b];
  }
  const T* Ub = a.U + (size_t)b * N * m;
  const T inf = std::numeric_limits<T>::infinity();
  const int turns = (S + G - 1) / G;

  // ---- pass 1: the candidates (shoot_kernel's rollout, its own copy) --------
  // the lane's own candidates meet in s order: ties go to the lower s
  T Jmin = inf;
  int smin = -1;
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    if (live && s < S) {
      const size_t bs = (size_t)b * S + s;
      const uint64_t roll = a.offset + (uint64_t)bs;
      const bool base = s == 0;  // the base sequence is a candidate
      T z[n], zn[n], un[m], ur[m], e[m];
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = z0[j];
#pragma unroll
      for (int j = 0; j < m; ++j) ur[j] = Ub[j];
      draw_units<T, m>(a.seed, roll, 0, kMppiStream, e);  // e_0 = xi_0
      T J = T(0);
      for (int t = 0; t < N; ++t) {
        // the next step's base action and normals, ahead of the dependent chain
        T ur2[m], xi[m];
        const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
        for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
        draw_units<T, m>(a.seed, roll, t + 1, kMppiStream, xi);
#pragma unroll
        for (int r = 0; r < m; ++r) {
          const T v = base ? ur[r] : fma_of(astd[r], e[r], ur[r]);
          un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
        }
        const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
        J += cost_value<T, MODEL>(P, z, un, tr, false);
        dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
        for (int j = 0; j < n; ++j) z[j] = zn[j];
#pragma unroll
        for (int j = 0; j < m; ++j) {
          ur[j] = ur2[j];
          e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
        }
      }
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      a.Jc[bs] = J;
      if (is_finite(J) && J < Jmin) {
        Jmin = J;
        smin = s;
      }
    }
  }

  // The argmin, in shoot's order: the lane's own in s order (above), a
  // butterfly over the group's lanes of a wavefront, then the workgroup's
  // wavefronts in their order through LDS.  Idle lanes hold (+inf, -1).
  for (int off = 1; off < span; off <<= 1)
    mppi_take_lower(Jmin, smin, __shfl_xor(Jmin, off), __shfl_xor(smin, off));
  if (multi) {
    __shared__ T part_J[kWaves];
    __shared__ int part_s[kWaves];
    if (tid % kWave == 0) {
      part_J[tid / kWave] = Jmin;
      part_s[tid / kWave] = smin;
    }
    __syncthreads();
    Jmin = part_J[0];
    smin = part_s[0];
    for (int w = 1; w < (int)blockDim.x / kWave; ++w)
      mppi_take_lower(Jmin, smin, part_J[w], part_s[w]);
  }
  // a temperature that is not positive (or NaN): as without a finite candidate
  if (!(lam > T(0))) {
    Jmin = inf;
    smin = -1;
  }
  const bool ok = live && smin >= 0;
  const bool owner = ok && lane == 0;  // ONE lane per trajectory
  if (live && lane == 0) {
    a.best[b] = smin;
    if (a.J_best != nullptr) a.J_best[b] = Jmin;
    if (!ok) a.J_w[b] = inf;
  }

  // ---- pass 2: eta.  A lane's own weights in s order, then the group. -------
  __shared__ T part_eta[1][kWaves];
  __shared__ T part_sum[2][m][kWaves];
  T eta_[1] = {T(0)};
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    if (ok && s < S)
      eta_[0] += softmin_weight(a.Jc[(size_t)b * S + s], Jmin, lam);
  }
  group_sum(eta_, span, multi, part_eta);
  const T eta = eta_[0];

  // ---- pass 3: the weighted perturbation, then the weighted rollout ---------
  T* Zo = a.Z_out + (size_t)b * (N + 1) * n;
  T* Uo = a.U_out + (size_t)b * N * m;
  const bool rows = a.U_out != nullptr;
  int phase = 0;
  for (int turn = 0; turn < turns; ++turn) {
    const bool last = turn == turns - 1;  // (uniform over the launch)
    const int s = lane + turn * G;
    const size_t bs = (size_t)b * S + s;
    const uint64_t roll = a.offset + (uint64_t)bs;
    T w = T(0);
    if (live && s < S) {
      if (ok) w = softmin_weight(a.Jc[bs], Jmin, lam);
      if (a.W != nullptr) a.W[bs] = ok ? w / eta : T(0);
    }
    // candidate 0 adds its weight to eta and nothing to the sum; a weight of
    // 0 adds 0 whatever its draws are, so they are not made
    const bool draw = s >= 1 && w > T(0);
    // the sum of the turns before this one: the owner's own stores in U_out
    const bool carry = owner && turn > 0 && rows;
    T e[m], ur[m], prev[m], z[n];
#pragma unroll
    for (int j = 0; j < m; ++j) {
      e[j] = T(0);
      ur[j] = owner ? Ub[j] : T(0);
      prev[j] = carry ? Uo[j] : T(0);
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z[j] = z0[j];
    if (draw) draw_units<T, m>(a.seed, roll, 0, kMppiStream, e);  // e_0 = xi_0
    T J = T(0);
    for (int t = 0; t < N; ++t) {
      // the next step's base action and carried sum, ahead of the chain
      T ur2[m], prev2[m], p[m];
      const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
      for (int j = 0; j < m; ++j) {
        ur2[j] = owner ? Ub[tn * m + j] : T(0);
        prev2[j] = carry ? Uo[tn * m + j] : T(0);
        // (an explicit fma: the product is rounded before it meets a sum)
        p[j] = draw ? fma_of(w, e[j], T(0)) : T(0);
      }
      if (draw) {
        T xi[m];
        draw_units<T, m>(a.seed, roll, t + 1, kMppiStream, xi);
#pragma unroll
        for (int j = 0; j < m; ++j)
          e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
      }
      group_sum(p, span, multi, part_sum[phase]);
      phase ^= 1;
      if (owner) {
        T acc[m];
#pragma unroll
        for (int j = 0; j < m; ++j) acc[j] = turn > 0 ? prev[j] + p[j] : p[j];
        if (!last) {
          if (rows) {
#pragma unroll
            for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = acc[j];
          }
        } else {
          T un[m], zn[n];
#pragma unroll
          for (int r = 0; r < m; ++r) {
            const T v = fma_of(astd[r], acc[r] / eta, ur[r]);
            un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
          }
          if (rows) {
#pragma unroll
            for (int j = 0; j < n; ++j) Zo[(size_t)t * n + j] = z[j];
#pragma unroll
            for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = un[j];
          }
          const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
          J += cost_value<T, MODEL>(P, z, un, tr, false);
          dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
          for (int j = 0; j < n; ++j) z[j] = zn[j];
        }
      }
#pragma unroll
      for (int j = 0; j < m; ++j) {
        ur[j] = ur2[j];
        prev[j] = prev2[j];
      }
    }
    if (owner && last) {
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      if (rows) {
#pragma unroll
        for (int j = 0; j < n; ++j) Zo[(size_t)N * n + j] = z[j];
      }
      a.J_w[b] = J;
    }
  }
}

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_mppi(const pddp_problem& p, MppiArgs<T> a, hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  ClosedLoopArgs<T> g{};  // (the mapping is closed_loop's: its geometry)
  g.B = a.B;
  g.S = a.S;
  dim3 blocks;
  const int threads = closed_loop_geometry(g, blocks);
  a.G = g.G;
  PDDP_LAUNCH((mppi_kernel<T, MODEL>), blocks, dim3(threads), 0, st, P, a);
  return launch_status();
}

template <typename T>
static int mppi_impl(const pddp_problem* p, bool batch, const T* table, int B,
                     int N, int S, const T* z0, const T* U, const T* u_min,
                     const T* u_max, const T* a_std, const T* lam,
                     double smooth, uint64_t seed, uint64_t sample_offset,
                     const uint8_t* active, T* Jc, int32_t* best, T* J_best,
                     T* W, T* J_w, T* Z_out, T* U_out, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || (long long)B * S > 0x7fffffffLL ||
      (batch && !table) || !z0 || !U || !a_std || !lam || !Jc || !best ||
      !J_w || (Z_out == nullptr) != (U_out == nullptr) ||
      (U_out != nullptr && (U_out == U || Z_out == z0)) ||
      // (a lane with more than one turn keeps the running sum in U_out)
      (U_out == nullptr && S > kClosedLoopThreads) ||
      !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  const double gamma = std::sqrt(1.0 - smooth * smooth);
  MppiArgs<T> a{B,      N,     S,        0,         z0,       U,
                table,  u_min, u_max,    a_std,     lam,      (T)smooth,
                (T)gamma, seed, sample_offset, active, Jc,    best,
                J_best, W,     J_w,      Z_out,     U_out};
  PDDP_DISPATCH_MODEL(launch_mppi, T, p, a, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_MPPI_PARAMS(T)                                                    \
  int B, int N, int S, const T* z0, const T* U, const T* u_min,                \
      const T* u_max, const T* a_std, const T* lam, double smooth,             \
      uint64_t seed, uint64_t sample_offset, const uint8_t* active, T* Jc,     \
      int32_t* best, T* J_best, T* W, T* J_w, T* Z_out, T* U_out, void* stream
#define PDDP_MPPI_ARGS                                                         \
  B, N, S, z0, U, u_min, u_max, a_std, lam, smooth, seed, sample_offset,       \
      active, Jc, best, J_best, W, J_w, Z_out, U_out, stream

#define PDDP_MPPI_ENTRY_POINTS(SUF, T)                                         \
  int pddp_mppi_##SUF(const pddp_problem* p, PDDP_MPPI_PARAMS(T)) {            \
    return pddp::mppi_impl<T>(p, false, nullptr, PDDP_MPPI_ARGS);              \
  }                                                                            \
  /* the same with a problem per trajectory: row b of `table` */               \
  int pddp_mppi_batch_##SUF(const pddp_problem* p, const T* table,             \
                            PDDP_MPPI_PARAMS(T)) {                             \
    return pddp::mppi_impl<T>(p, true, table, PDDP_MPPI_ARGS);                 \
  }

PDDP_MPPI_ENTRY_POINTS(f32, float)
PDDP_MPPI_ENTRY_POINTS(f64, double)
#undef PDDP_MPPI_ENTRY_POINTS
#undef PDDP_MPPI_ARGS
#undef PDDP_MPPI_PARAMS

}  // extern "C"
