// closed_loop.hip - closed-loop policy evaluation: S rollouts of every
// trajectory's time-varying feedback policy (Z, U, K), each from its own
// initial state on its own plant, and the statistics of a controller's costs.
//
//   the trial step of the outer loop   pddp/controllers/pddp.py:209-245
//                                      (_apply_controller, batched: the sample
//                                      models as the plant)
//   the feedback law                   ilqr.py:318-355 (forward, mpc=False)
//   the cost of a rollout              ilqr.py:764-791 (_trajectory_cost)
//
// A translation unit of its own (csrc/Makefile: FLAGS_closed_loop).  Its loop
// resembles the line search's but is its own text - the feedback law and the
// output layout differ; the parameter count is model_params.hpp's, the row
// writer stays written out at its one call site.
#include <limits>
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"

namespace pddp {

// Mapping: one lane per rollout, s fastest.  A trajectory owns G consecutive
// lanes, the launch's lane group:
//   S <= 64   G = S rounded up to a power of two, workgroups of one wavefront
//             holding 64 / G trajectories; lanes s >= S of a group idle;
//   S > 64    G = the workgroup = S rounded up to whole wavefronts, at most
//             four: one trajectory per workgroup, lane l runs the rollouts
//             s = l, l + G, ... one after the other.
// A group starts at a multiple of G in its wavefront (which multiple depends
// on b where G < 64), and the reduction's butterfly is relative to that
// aligned start; which rollouts a lane runs and in which order the costs meet
// depend on S alone, never on b: a controller's outputs are the same bits
// wherever it is in the batch.
constexpr int kClosedLoopThreads = 4 * kWave;

template <typename T>
struct ClosedLoopArgs {
  int B, N, S, G;
  const T* z0s;    // [B][S][n] or NULL: Z[b][0]
  const T* plant;  // [B][S][PDDP_BATCH_ROW] or NULL: the shared problem
  const T* u_min;
  const T* u_max;
  const uint8_t* active;
  T* Xc;  // [B][N+1][S][n], with Uc [B][N][S][m]: both or neither
  T* Uc;
  T* Jc;     // [B][S]
  T* stats;  // [B][4] or NULL
};

// The statistics of the finite costs a lane (then a lane group) has seen.
template <typename T>
struct CostStats {
  T sum, lo, hi;
  int count;
};
template <typename T>
PDDP_DEV void merge(CostStats<T>& a, T sum, T lo, T hi, int count) {
  a.sum += sum;
  a.lo = lo < a.lo ? lo : a.lo;
  a.hi = hi > a.hi ? hi : a.hi;
  a.count += count;
}

// The step's nominal row Z[b][t] | U[b][t] | K[b][t] is read by every lane,
// the lanes of a trajectory at the same addresses: one broadcast.  (Where a
// wavefront holds one trajectory, G >= 64, the row is wave-uniform; fetching it
// through scalar loads was built and measured slower)
template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void closed_loop_kernel(
    ProblemT<T> shared, ClosedLoopArgs<T> a, const T* __restrict__ Znom,
    const T* __restrict__ Unom, const T* __restrict__ gains) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int GS = m + m * n;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);

  CostStats<T> st{T(0), std::numeric_limits<T>::infinity(),
                  -std::numeric_limits<T>::infinity(), 0};
  if (live) {
    const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
    const bool feedback = gains != nullptr;
    const bool keep = a.Xc != nullptr;
    T umin[m], umax[m];
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
    }
    const T* Zb = Znom + (size_t)b * (N + 1) * n;
    const T* Ub = Unom + (size_t)b * N * m;
    // (only the K part of a gains row is read)
    const T* Kb = feedback ? gains + (size_t)b * N * GS + m : nullptr;
    const size_t xstep = (size_t)S * n, ustep = (size_t)S * m;

    for (int s = lane; s < S; s += G) {
      const size_t bs = (size_t)b * S + s;
      // the plant of this rollout: the shared problem with row (b, s) written
      // over it, in registers for the whole rollout; Q, Qt and R are never
      // written and stay scalar operands of the kernel argument
      ProblemT<T> P = shared;
      // (write_params_and_goals' statements in place: called, seven of the
      // eight kernels come out as other instructions)
      if (a.plant != nullptr) {
        const T* row = a.plant + bs * PDDP_BATCH_ROW;
        P.dt = row[PDDP_BATCH_PARAMS];
#pragma unroll
        for (int i = 0; i < kModelParamCount<MODEL> - 1; ++i)
          P.p[i] = row[PDDP_BATCH_PARAMS + 1 + i];
#pragma unroll
        for (int i = 0; i < D::na; ++i) P.goal[i] = row[PDDP_BATCH_X_GOAL + i];
#pragma unroll
        for (int i = 0; i < D::m; ++i) P.ugoal[i] = row[PDDP_BATCH_U_GOAL + i];
      }

      T z[n], zn[n], un[m];
      T zr[n], ur[m], kr[m * n];  // this step's nominal z, u and K
#pragma unroll
      for (int j = 0; j < n; ++j) zr[j] = Zb[j];
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = zr[j];
      if (a.z0s != nullptr) {
#pragma unroll
        for (int j = 0; j < n; ++j) z[j] = a.z0s[bs * n + j];
      }
#pragma unroll
      for (int j = 0; j < m; ++j) ur[j] = Ub[j];
#pragma unroll
      for (int j = 0; j < m * n; ++j) kr[j] = T(0);
      if (feedback) {
#pragma unroll
        for (int j = 0; j < m * n; ++j) kr[j] = Kb[j];
      }

      // time-major output [b][t][s][.]: at every step the lanes of a
      // trajectory write one contiguous segment (the note at LineSearchArgs)
      T* Xci = keep ? a.Xc + ((size_t)b * (N + 1) * S + s) * n : nullptr;
      T* Uci = keep ? a.Uc + ((size_t)b * N * S + s) * m : nullptr;
      T J = T(0);
      for (int t = 0; t < N; ++t) {
        // the next step's nominal row, requested ahead of the dependent chain
        T zr2[n], ur2[m], kr2[m * n];
        const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
        for (int j = 0; j < n; ++j) zr2[j] = Zb[tn * n + j];
#pragma unroll
        for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
#pragma unroll
        for (int j = 0; j < m * n; ++j) kr2[j] = T(0);
        if (feedback) {
#pragma unroll
          for (int j = 0; j < m * n; ++j) kr2[j] = Kb[(size_t)tn * GS + j];
        }

#pragma unroll
        for (int r = 0; r < m; ++r) {
          T v = ur[r];
          if (feedback) {  // u + K (x - z)                 (ilqr.py:345-355)
            T du = T(0);
#pragma unroll
            for (int c = 0; c < n; ++c) du += (z[c] - zr[c]) * kr[r * n + c];
            v = v + du;
          }
          un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
        }
        if (keep) {
#pragma unroll
          for (int j = 0; j < n; ++j) Xci[(size_t)t * xstep + j] = z[j];
#pragma unroll
          for (int j = 0; j < m; ++j) Uci[(size_t)t * ustep + j] = un[j];
        }
        const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
        J += cost_value<T, MODEL>(P, z, un, tr, false);
        dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
        for (int j = 0; j < n; ++j) {
          z[j] = zn[j];
          zr[j] = zr2[j];
        }
#pragma unroll
        for (int j = 0; j < m; ++j) ur[j] = ur2[j];
#pragma unroll
        for (int j = 0; j < m * n; ++j) kr[j] = kr2[j];
      }
      if (keep) {
#pragma unroll
        for (int j = 0; j < n; ++j) Xci[(size_t)N * xstep + j] = z[j];
      }
      J += cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
      a.Jc[bs] = J;
      if (is_finite(J)) merge(st, J, J, J, 1);
    }
  }
  if (a.stats == nullptr) return;  // (the whole launch)

  // The costs of a trajectory meet in a fixed order: the lane's own in s
  // order (above), a butterfly over the group's lanes of a wavefront (both
  // partners of a pair form the same sum: a + b == b + a), then the
  // workgroup's wavefronts in their order through LDS.  Idle lanes hold the
  // neutral element.  No atomics.
  const int span = G < kWave ? G : kWave;
  for (int off = 1; off < span; off <<= 1)
    merge(st, __shfl_xor(st.sum, off), __shfl_xor(st.lo, off),
          __shfl_xor(st.hi, off), __shfl_xor(st.count, off));
  if (blockDim.x > kWave) {  // one trajectory over several wavefronts
    constexpr int W = kClosedLoopThreads / kWave;
    __shared__ T part[W][3];
    __shared__ int part_count[W];
    const int wave = tid / kWave;
    if (tid % kWave == 0) {
      part[wave][0] = st.sum;
      part[wave][1] = st.lo;
      part[wave][2] = st.hi;
      part_count[wave] = st.count;
    }
    __syncthreads();
    if (tid == 0)
      for (int w = 1; w < (int)blockDim.x / kWave; ++w)
        merge(st, part[w][0], part[w][1], part[w][2], part_count[w]);
  }
  if (live && lane == 0) {
    const T inf = std::numeric_limits<T>::infinity();
    const bool any = st.count > 0;
    T* out = a.stats + (size_t)b * 4;
    out[0] = any ? st.sum / T(st.count) : inf;
    out[1] = any ? st.lo : inf;
    out[2] = any ? st.hi : inf;
    out[3] = T(st.count);
  }
}

template <typename T>
struct ClosedLoopLaunch {
  ClosedLoopArgs<T> a;
  const T* Z;
  const T* U;
  const T* gains;
};

template <typename T, int MODEL>
static int launch_closed_loop(const pddp_problem& p, ClosedLoopLaunch<T> w,
                              hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  ClosedLoopArgs<T>& a = w.a;
  int threads = kWave;
  if (a.S <= kWave) {
    a.G = 1;
    while (a.G < a.S) a.G <<= 1;
  } else {
    const int waves = (a.S + kWave - 1) / kWave;
    threads = kWave * (waves < 4 ? waves : 4);
    a.G = threads;
  }
  const int per_block = threads / a.G;
  const dim3 blocks((unsigned)(((long long)a.B + per_block - 1) / per_block));
  PDDP_LAUNCH((closed_loop_kernel<T, MODEL>), blocks, dim3(threads), 0, st, P,
              a, w.Z, w.U, w.gains);
  return launch_status();
}

template <typename T>
static int closed_loop_impl(const pddp_problem* p, int B, int N, int S,
                            const T* Z, const T* U, const T* gains,
                            const T* z0s, const T* plant, const T* u_min,
                            const T* u_max, const uint8_t* active, T* Xc,
                            T* Uc, T* Jc, T* stats, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || !Z || !U || !Jc ||
      (Xc == nullptr) != (Uc == nullptr))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  ClosedLoopLaunch<T> w{{B, N, S, 0, z0s, plant, u_min, u_max, active, Xc, Uc,
                         Jc, stats},
                        Z, U, gains};
  PDDP_DISPATCH_MODEL(launch_closed_loop, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

int pddp_closed_loop_f32(const pddp_problem* p, int B, int N, int S,
                         const float* Z, const float* U, const float* gains,
                         const float* z0s, const float* plant,
                         const float* u_min, const float* u_max,
                         const uint8_t* active, float* Xc, float* Uc,
                         float* Jc, float* stats, void* stream) {
  return pddp::closed_loop_impl<float>(p, B, N, S, Z, U, gains, z0s, plant,
                                       u_min, u_max, active, Xc, Uc, Jc, stats,
                                       stream);
}
int pddp_closed_loop_f64(const pddp_problem* p, int B, int N, int S,
                         const double* Z, const double* U, const double* gains,
                         const double* z0s, const double* plant,
                         const double* u_min, const double* u_max,
                         const uint8_t* active, double* Xc, double* Uc,
                         double* Jc, double* stats, void* stream) {
  return pddp::closed_loop_impl<double>(p, B, N, S, Z, U, gains, z0s, plant,
                                        u_min, u_max, active, Xc, Uc, Jc,
                                        stats, stream);
}

}  // extern "C"
