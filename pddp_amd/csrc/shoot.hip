// shoot.hip - sampled shooting: S perturbed copies of every trajectory's action
// sequence rolled out open loop under the solver's model and cost, the
// cheapest found INSIDE the launch, and only that one's states and actions
// written (pddp_shoot_*, pddp_shoot_batch_*, ILQRSolver.shoot); the unit
// normals of the perturbation written out (pddp_shoot_draws_*).  The reference
// has no counterpart: include/pddp_hip.h states the law, DESIGN.md 3.4m the
// kernel.
//
//   candidate (b, s), r = sample_offset + b S + s:
//     xi_t = the m unit normals of (seed, r, t, stream 2)
//     e_0 = xi_0;  e_t = fma(beta, e_{t-1}, gamma xi_t)       AR(1), unit variance
//     u_t = clamp(fma(a_std, e_t, U[b][t]))   s >= 1;   clamp(U[b][t])   s == 0
//     J += l(x_t, u_t);  x_{t+1} = f_b(x_t, u_t);  J += l_f(x_N)
//
// Mapping, lane groups and the order in which a trajectory's costs meet are
// closed_loop.hip's (closed_loop_args.hpp); the draws are closed_loop_draws.hpp's
// as they are, stream 2.  One translation unit, one rollout kernel per model and
// type: the table of the _batch entry points is a nullable kernel argument, as
// closed_loop_kernel's plant rows are.
//
// The winner is rolled out a SECOND time in the same launch: the lanes walk one
// loop of ceil(S / G) + 1 turns whose body is the rollout; the last turn starts
// with the argmin, after which the one lane that owned the winner runs the body
// again with `keep` set - the same instructions, their stores enabled by a
// run-time predicate - so Z_out / U_out are the rollout Jc[b][best] was summed
// over, whatever the compiler made of the body.  No [B][N][S][.] tensor exists
// and no rollout's states are held in registers or LDS beyond its own step.
#include <cmath>
#include <limits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"

namespace pddp {

constexpr int kShootStream = 2;  // (0 process, 1 measurement: closed_loop.hip)

template <typename T>
struct ShootArgs {
  int B, N, S, G;
  const T* z0;     // [B][n]
  const T* U;      // [B][N][m]
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the shared problem
  const T* u_min;
  const T* u_max;
  const T* a_std;  // [m]
  T beta, gamma;
  uint64_t seed, offset;
  const uint8_t* active;
  T* Jc;          // [B][S]
  int32_t* best;  // [B]
  T* J_best;      // [B] or NULL
  T* Z_out;       // [B][N+1][n], with U_out [B][N][m]: both or neither
  T* U_out;
};

// (J, s) ordered lexicographically; (+inf, -1) is "no finite cost" and loses
// against every candidate, whose J is finite.
template <typename T>
PDDP_DEV void take_lower(T& J, int& s, T oJ, int os) {
  const bool take = oJ < J || (oJ == J && os < s);
  J = take ? oJ : J;
  s = take ? os : s;
}

template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void shoot_kernel(
    ProblemT<T> shared, ShootArgs<T> a) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;

  // the problem of trajectory b: the shared one with row b written over it, in
  // registers for the whole launch; Q, Qt and R stay scalar operands
  ProblemT<T> P = shared;
  T umin[m], umax[m], astd[m], z0[n];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
#pragma unroll
  for (int j = 0; j < n; ++j) z0[j] = T(0);
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
  }
  const T* Ub = a.U + (size_t)b * N * m;
  const T inf = std::numeric_limits<T>::infinity();

  // the lane's own candidates meet in s order: ties go to the lower s
  T Jmin = inf;
  int smin = -1;
  const int turns = (S + G - 1) / G;
  for (int turn = 0; turn <= turns; ++turn) {
    const bool keep = turn == turns;  // (uniform over the launch)
    int s = lane + turn * G;
    bool run = live && s < S;
    if (keep) {
      // The argmin of a trajectory meets in a fixed order: the lane's own in
      // s order (above), a butterfly over the group's lanes of a wavefront
      // (both partners of a pair choose the same of the two), then the
      // workgroup's wavefronts in their order through LDS, read by every
      // lane.  Idle lanes hold (+inf, -1).  No atomics.
      const int span = G < kWave ? G : kWave;
      for (int off = 1; off < span; off <<= 1)
        take_lower(Jmin, smin, __shfl_xor(Jmin, off), __shfl_xor(smin, off));
      if (blockDim.x > kWave) {  // one trajectory over several wavefronts
        constexpr int W = kClosedLoopThreads / kWave;
        __shared__ T part_J[W];
        __shared__ int part_s[W];
        if (tid % kWave == 0) {
          part_J[tid / kWave] = Jmin;
          part_s[tid / kWave] = smin;
        }
        __syncthreads();
        Jmin = part_J[0];
        smin = part_s[0];
        for (int w = 1; w < (int)blockDim.x / kWave; ++w)
          take_lower(Jmin, smin, part_J[w], part_s[w]);
      }
      if (live && lane == 0) {
        a.best[b] = smin;
        if (a.J_best != nullptr) a.J_best[b] = Jmin;
      }
      // the winner again, by the lane that ran it, its rows kept
      s = smin;
      run = live && a.Z_out != nullptr && smin >= 0 && lane == smin % G;
    }
    if (run) {
      const size_t bs = (size_t)b * S + s;
      const uint64_t roll = a.offset + (uint64_t)bs;
      const bool base = s == 0;  // the base sequence is a candidate
      T z[n], zn[n], un[m], ur[m], e[m];
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = z0[j];
#pragma unroll
      for (int j = 0; j < m; ++j) ur[j] = Ub[j];
      draw_units<T, m>(a.seed, roll, 0, kShootStream, e);  // e_0 = xi_0
      T* Zo = a.Z_out + (size_t)b * (N + 1) * n;
      T* Uo = a.U_out + (size_t)b * N * m;
      T J = T(0);
      for (int t = 0; t < N; ++t) {
        // the next step's base action and normals, ahead of the dependent chain
        T ur2[m], xi[m];
        const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
        for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
        draw_units<T, m>(a.seed, roll, t + 1, kShootStream, xi);
#pragma unroll
        for (int r = 0; r < m; ++r) {
          const T v = base ? ur[r] : fma_of(astd[r], e[r], ur[r]);
          un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
        }
        if (keep) {
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
#pragma unroll
        for (int j = 0; j < m; ++j) {
          ur[j] = ur2[j];
          e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
        }
      }
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      if (keep) {
#pragma unroll
        for (int j = 0; j < n; ++j) Zo[(size_t)N * n + j] = z[j];
      } else {
        a.Jc[bs] = J;
        if (is_finite(J) && J < Jmin) {
          Jmin = J;
          smin = s;
        }
      }
    }
  }
}

// ---- the unit normals written out ------------------------------------------

template <typename T>
struct ShootDrawArgs {
  int B, N, S, m;
  uint64_t seed, offset;
  T* E;  // [B][N][S][m]
};

// One lane per (b, t, s), s fastest, as closed_loop_draws_kernel.
template <typename T>
__global__ __launch_bounds__(kClosedLoopThreads) void shoot_draws_kernel(
    ShootDrawArgs<T> a) {
  constexpr int kPer = DrawBlock<T>::kPer;
  const size_t total = (size_t)a.B * a.N * a.S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t bt = i / a.S;
    const int s = (int)(i - bt * a.S);
    const size_t b = bt / a.N;
    const int t = (int)(bt - b * a.N);
    const uint64_t r = a.offset + (uint64_t)b * a.S + s;
    T* out = a.E + i * a.m;
    for (int k = 0; k * kPer < a.m; ++k) {
      T z[kPer];
      draw_block(a.seed, r, t, kShootStream, k, z);
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        if (k * kPer + j < a.m) out[k * kPer + j] = z[j];
    }
  }
}

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_shoot(const pddp_problem& p, ShootArgs<T> a, hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  ClosedLoopArgs<T> g{};  // (the mapping is closed_loop's: its geometry)
  g.B = a.B;
  g.S = a.S;
  dim3 blocks;
  const int threads = closed_loop_geometry(g, blocks);
  a.G = g.G;
  PDDP_LAUNCH((shoot_kernel<T, MODEL>), blocks, dim3(threads), 0, st, P, a);
  return launch_status();
}

template <typename T>
static int shoot_impl(const pddp_problem* p, bool batch, const T* table, int B,
                      int N, int S, const T* z0, const T* U, const T* u_min,
                      const T* u_max, const T* a_std, double smooth,
                      uint64_t seed, uint64_t sample_offset,
                      const uint8_t* active, T* Jc, int32_t* best, T* J_best,
                      T* Z_out, T* U_out, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || (long long)B * S > 0x7fffffffLL ||
      (batch && !table) || !z0 || !U || !a_std || !Jc || !best ||
      (Z_out == nullptr) != (U_out == nullptr) ||
      (U_out != nullptr && (U_out == U || Z_out == z0)) ||
      !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  const double gamma = std::sqrt(1.0 - smooth * smooth);
  ShootArgs<T> a{B,     N,     S,          0,        z0,
                 U,     table, u_min,      u_max,    a_std,
                 (T)smooth,    (T)gamma,   seed,     sample_offset,
                 active, Jc,   best,       J_best,   Z_out,
                 U_out};
  PDDP_DISPATCH_MODEL(launch_shoot, T, p, a, (hipStream_t)stream)
}

template <typename T>
static int shoot_draws_impl(int B, int N, int S, int m, uint64_t seed,
                            uint64_t sample_offset, T* E, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || m <= 0 || m > PDDP_MAX_ACTION || !E)
    return PDDP_E_BADARG;
  const size_t total = (size_t)B * N * S;
  const size_t want = (total + kClosedLoopThreads - 1) / kClosedLoopThreads;
  const size_t cap = (size_t)1 << 20;  // (the kernel strides over the rest)
  const dim3 blocks((unsigned)(want < cap ? want : cap));
  PDDP_LAUNCH((shoot_draws_kernel<T>), blocks, dim3(kClosedLoopThreads), 0,
              (hipStream_t)stream,
              (ShootDrawArgs<T>{B, N, S, m, seed, sample_offset, E}));
  return launch_status();
}

}  // namespace pddp

extern "C" {

#define PDDP_SHOOT_PARAMS(T)                                                   \
  int B, int N, int S, const T* z0, const T* U, const T* u_min,                \
      const T* u_max, const T* a_std, double smooth, uint64_t seed,            \
      uint64_t sample_offset, const uint8_t* active, T* Jc, int32_t* best,     \
      T* J_best, T* Z_out, T* U_out, void* stream
#define PDDP_SHOOT_ARGS                                                        \
  B, N, S, z0, U, u_min, u_max, a_std, smooth, seed, sample_offset, active,    \
      Jc, best, J_best, Z_out, U_out, stream

#define PDDP_SHOOT_ENTRY_POINTS(SUF, T)                                        \
  int pddp_shoot_##SUF(const pddp_problem* p, PDDP_SHOOT_PARAMS(T)) {          \
    return pddp::shoot_impl<T>(p, false, nullptr, PDDP_SHOOT_ARGS);            \
  }                                                                            \
  /* the same with a problem per trajectory: row b of `table` */               \
  int pddp_shoot_batch_##SUF(const pddp_problem* p, const T* table,            \
                             PDDP_SHOOT_PARAMS(T)) {                           \
    return pddp::shoot_impl<T>(p, true, table, PDDP_SHOOT_ARGS);               \
  }                                                                            \
  int pddp_shoot_draws_##SUF(int B, int N, int S, int m, uint64_t seed,        \
                             uint64_t sample_offset, T* E, void* stream) {     \
    return pddp::shoot_draws_impl<T>(B, N, S, m, seed, sample_offset, E,       \
                                     stream);                                  \
  }

PDDP_SHOOT_ENTRY_POINTS(f32, float)
PDDP_SHOOT_ENTRY_POINTS(f64, double)
#undef PDDP_SHOOT_ENTRY_POINTS
#undef PDDP_SHOOT_ARGS
#undef PDDP_SHOOT_PARAMS

}  // extern "C"
