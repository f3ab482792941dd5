// mppi_trial.hip - a receding-horizon MPPI trial, every control step inside ONE
// launch: plan (K iterations of mppi.hip's law around the plan U), apply the
// first action to the plant, observe, shift the plan - for control steps
// t0 .. t0 + count - 1 of TT (pddp_mppi_trial_*, ILQRSolver.mppi_closed_loop).
// The reference has no counterpart: include/pddp_hip.h states the law,
// DESIGN.md 3.4o the kernel.
//
// mppi.hip, shoot.hip, closed_loop.hip and the hand-over's texts are as they
// were: this unit carries its own copy of the candidate rollout and of the
// weighted update (the Makefile's note on contraction) and uses draw_units,
// add_scaled, fma_of, closed_loop_geometry and models.hpp as they are.
//
// Mapping: mppi_kernel's - a trajectory owns a lane group of G lanes, lane 0
// of the group (the head) does what is done once per trajectory.  A
// trajectory never leaves its workgroup, so a control step needs no launch
// boundary.  What is new against mppi_kernel: lanes read what the head stored
// earlier in the launch - z0[b], and U[b] after a `took` copy or a shift.
// Every such hand-over is the head's stores, hand_over() (the wait on the
// stores, then the workgroup's barrier with its fence), then the group's
// loads; the candidate-0 cost and J_w the head needs for `took` it holds in
// its own registers.  The loops over c, k, the turns and t are launch-uniform
// and every shuffle and barrier sits under them alone: lanes outside the
// batch, masked or without a candidate take part with zeros.  No atomics.
#include <climits>
#include <cmath>
#include <limits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"
#include "closed_loop_args.hpp"
#include "closed_loop_draws.hpp"

namespace pddp {

constexpr int kTrialStream = 2;  // (mppi's: the candidates are mppi's)

template <typename T>
struct MppiTrialArgs {
  int B, N, S, G, K, TT, t0, count;
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  const T* plant;  // [B][PDDP_BATCH_ROW] or NULL: the controller's model
  T* z0;           // [B][n]
  T* U;            // [B][N][m]
  T* Z;            // [B][N+1][n]
  T* U_work;       // [B][N][m]
  const T* u_min;
  const T* u_max;
  const T* a_std;  // [m]
  const T* lam;    // [B]
  T beta, gamma;
  uint64_t seed, cand_offset, iter_stride;
  const T* disturbance;  // [B][TT][n] or NULL
  const T* w_std;        // [n] or NULL
  const T* v_std;        // [n] or NULL
  uint64_t rollout_offset;
  int step_offset;
  T* x_true;  // [B][n], with v_std
  const uint8_t* active;
  T* Jc;  // [B][S], or [B][TT][K][S] with log_costs
  int log_costs;
  T* Xlog;      // [B][TT+1][n]
  T* Ulog;      // [B][TT][m]
  T* Jcl;       // [B]
  T* Ylog;      // [B][TT+1][n] or NULL
  T* J0_log;    // [B][TT][K] or NULL
  T* Jw_log;    // [B][TT][K] or NULL
  T* ess_log;   // [B][TT] or NULL
  T* plan_log;  // [B][TT][N][m] or NULL
};

// mppi.hip's take_lower: (J, s) ordered lexicographically.
template <typename T>
PDDP_DEV void trial_take_lower(T& J, int& s, T oJ, int os) {
  const bool take = oJ < J || (oJ == J && os < s);
  J = take ? oJ : J;
  s = take ? os : s;
}

PDDP_DEV float trial_exp(float x) { return expf(x); }
PDDP_DEV double trial_exp(double x) { return exp(x); }

// mppi.hip's softmin_weight.
template <typename T>
PDDP_DEV T trial_weight(T J, T J_best, T lam) {
  const T arg = -((J - J_best) / lam);
  return is_finite(J) ? trial_exp(arg) : T(0);
}

// mppi.hip's group_sum: the sums of v[0..K) over a trajectory's lane group,
// on every lane of the group.
template <typename T, int K>
PDDP_DEV void trial_group_sum(T (&v)[K], int span, bool multi,
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

// Between the head's stores to z0[b] / U[b] and the group's loads of them: the
// storing wavefront waits for its stores, then the workgroup meets at the
// barrier, whose fence keeps the compiler from moving the loads ahead of it.
// A workgroup's wavefronts share their CU's L1: workgroup scope is enough.
PDDP_DEV void hand_over() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

template <typename T, int MODEL>
__global__ __launch_bounds__(kClosedLoopThreads) void mppi_trial_kernel(
    ProblemT<T> shared, MppiTrialArgs<T> a) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr int kWaves = kClosedLoopThreads / kWave;
  const int tid = threadIdx.x, G = a.G, N = a.N, S = a.S, K = a.K, TT = a.TT;
  const int group = tid / G, lane = tid - group * G;
  const long long bl = (long long)blockIdx.x * (blockDim.x / G) + group;
  const bool in_batch = bl < a.B;
  const int b = in_batch ? (int)bl : 0;
  // (nothing of a skipped trajectory is read or written)
  const bool live = in_batch && (a.active == nullptr || a.active[b] != 0);
  const bool head = live && lane == 0;  // ONE lane per trajectory
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const bool multi = blockDim.x > kWave;  // one trajectory, several wavefronts
  const int span = G < kWave ? G : kWave;

  // the controller's model of trajectory b, as mppi_kernel holds it
  ProblemT<T> P = shared;
  T umin[m], umax[m], astd[m];
#pragma unroll
  for (int r = 0; r < m; ++r) umin[r] = umax[r] = astd[r] = T(0);
  T lam = T(1);
  if (live) {
    if (a.table != nullptr)
      write_params_and_goals<T, MODEL>(P,
                                       a.table + (size_t)b * PDDP_BATCH_ROW);
#pragma unroll
    for (int r = 0; r < m; ++r) {
      umin[r] = bounded ? a.u_min[r] : T(0);
      umax[r] = bounded ? a.u_max[r] : T(0);
      astd[r] = a.a_std[r];
    }
    lam = a.lam[b];
  }
  T* Ub = a.U + (size_t)b * N * m;
  T* Uo = a.U_work + (size_t)b * N * m;
  const T inf = std::numeric_limits<T>::infinity();
  const int turns = (S + G - 1) / G;

  __shared__ T part_J[kWaves];
  __shared__ int part_s[kWaves];
  __shared__ T part_eta[2][kWaves];
  __shared__ T part_sum[2][m][kWaves];
  int phase = 0;

  // the trial's cost so far: the head's own word from step to step
  T Jcl = T(0);
  if (head && a.t0 > 0) Jcl = a.Jcl[b];

  for (int c = a.t0; c < a.t0 + a.count; ++c) {
    // what the controller sees at step c (the head's store of step c - 1)
    T z0[n];
#pragma unroll
    for (int j = 0; j < n; ++j) z0[j] = live ? a.z0[(size_t)b * n + j] : T(0);

    for (int k = 0; k < K; ++k) {
      const uint64_t offset =
          a.cand_offset + ((uint64_t)c * (uint64_t)K + (uint64_t)k) * a.iter_stride;
      T* Jcb = a.Jc + (a.log_costs != 0
                           ? (((size_t)b * TT + c) * K + k) * (size_t)S
                           : (size_t)b * S);

      // ---- pass 1: the candidates (mppi_kernel's rollout, its own copy) -----
      T Jmin = inf, J0 = inf;
      int smin = -1;
      for (int turn = 0; turn < turns; ++turn) {
        const int s = lane + turn * G;
        if (live && s < S) {
          const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
          const bool base = s == 0;  // the base sequence is a candidate
          T z[n], zn[n], un[m], ur[m], e[m];
#pragma unroll
          for (int j = 0; j < n; ++j) z[j] = z0[j];
#pragma unroll
          for (int j = 0; j < m; ++j) ur[j] = Ub[j];
          draw_units<T, m>(a.seed, roll, 0, kTrialStream, e);  // e_0 = xi_0
          T J = T(0);
          for (int t = 0; t < N; ++t) {
            // the next step's base action and normals, ahead of the chain
            T ur2[m], xi[m];
            const int tn = (t + 1 < N) ? t + 1 : t;
#pragma unroll
            for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
            draw_units<T, m>(a.seed, roll, t + 1, kTrialStream, xi);
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
          Jcb[s] = J;
          if (base) J0 = J;  // (the head's: lane 0 holds candidate 0)
          if (is_finite(J) && J < Jmin) {
            Jmin = J;
            smin = s;
          }
        }
      }

      // the argmin, in mppi's order
      for (int off = 1; off < span; off <<= 1)
        trial_take_lower(Jmin, smin, __shfl_xor(Jmin, off),
                         __shfl_xor(smin, off));
      if (multi) {
        if (tid % kWave == 0) {
          part_J[tid / kWave] = Jmin;
          part_s[tid / kWave] = smin;
        }
        __syncthreads();
        Jmin = part_J[0];
        smin = part_s[0];
        for (int w = 1; w < (int)blockDim.x / kWave; ++w)
          trial_take_lower(Jmin, smin, part_J[w], part_s[w]);
      }
      // a temperature that is not positive (or NaN): no finite candidate
      if (!(lam > T(0))) {
        Jmin = inf;
        smin = -1;
      }
      const bool ok = live && smin >= 0;
      const bool owner = ok && lane == 0;

      // ---- pass 2: eta, and the sum of the squared weights with it ----------
      T es[2] = {T(0), T(0)};
      for (int turn = 0; turn < turns; ++turn) {
        const int s = lane + turn * G;
        if (ok && s < S) {
          const T w = trial_weight(Jcb[s], Jmin, lam);
          es[0] += w;
          es[1] += w * w;
        }
      }
      trial_group_sum(es, span, multi, part_eta);
      const T eta = es[0];

      // ---- pass 3: the weighted perturbation, then the weighted rollout -----
      T Jw = inf;
      for (int turn = 0; turn < turns; ++turn) {
        const bool last = turn == turns - 1;  // (uniform over the launch)
        const int s = lane + turn * G;
        const uint64_t roll = offset + (uint64_t)((size_t)b * S + s);
        T w = T(0);
        if (ok && s < S) w = trial_weight(Jcb[s], Jmin, lam);
        // candidate 0 adds its weight to eta and nothing to the sum; a weight
        // of 0 adds 0 whatever its draws are, so they are not made
        const bool draw = s >= 1 && w > T(0);
        // the sum of the turns before this one: the owner's stores in U_work
        const bool carry = owner && turn > 0;
        T e[m], ur[m], prev[m], z[n];
#pragma unroll
        for (int j = 0; j < m; ++j) {
          e[j] = T(0);
          ur[j] = owner ? Ub[j] : T(0);
          prev[j] = carry ? Uo[j] : T(0);
        }
#pragma unroll
        for (int j = 0; j < n; ++j) z[j] = z0[j];
        if (draw) draw_units<T, m>(a.seed, roll, 0, kTrialStream, e);
        T J = T(0);
        for (int t = 0; t < N; ++t) {
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
            draw_units<T, m>(a.seed, roll, t + 1, kTrialStream, xi);
#pragma unroll
            for (int j = 0; j < m; ++j)
              e[j] = fma_of(a.beta, e[j], a.gamma * xi[j]);
          }
          trial_group_sum(p, span, multi, part_sum[phase]);
          phase ^= 1;
          if (owner) {
            T acc[m];
#pragma unroll
            for (int j = 0; j < m; ++j)
              acc[j] = turn > 0 ? prev[j] + p[j] : p[j];
            if (!last) {
#pragma unroll
              for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = acc[j];
            } else {
              T un[m], zn[n];
#pragma unroll
              for (int r = 0; r < m; ++r) {
                const T v = fma_of(astd[r], acc[r] / eta, ur[r]);
                un[r] = bounded ? clamp_nan(v, umin[r], umax[r]) : v;
              }
#pragma unroll
              for (int j = 0; j < m; ++j) Uo[(size_t)t * m + j] = un[j];
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
          Jw = J;
        }
      }

      // ---- the head: take the weighted sequence or keep the plan ------------
      if (head) {
        const size_t ck = ((size_t)b * TT + c) * K + k;
        if (a.J0_log != nullptr) a.J0_log[ck] = J0;
        if (a.Jw_log != nullptr) a.Jw_log[ck] = Jw;
        const bool took = is_finite(Jw) && Jw <= J0;
        if (k < K - 1) {
          if (took) {
            for (int i = 0; i < N * m; ++i) Ub[i] = Uo[i];
          }
        } else {
          const size_t bc = (size_t)b * TT + c;
          if (a.ess_log != nullptr)
            a.ess_log[bc] = ok ? (eta * eta) / es[1] : T(0);
          // the step's plan is `src`: logged, its first row applied, and U[b]
          // its shift (plain copies of unclamped words, the last row
          // repeated).  In place, row i + 1 is read before row i is written.
          const T* src = took ? Uo : Ub;
          T* Pb = a.plan_log != nullptr ? a.plan_log + bc * N * m : nullptr;
          T cur[m], nxt[m], u[m];
#pragma unroll
          for (int j = 0; j < m; ++j) {
            cur[j] = src[j];
            u[j] = bounded ? clamp1(cur[j], umin[j], umax[j]) : cur[j];
          }
          for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = 0; j < m; ++j)
              nxt[j] = i + 1 < N ? src[(i + 1) * m + j] : cur[j];
#pragma unroll
            for (int j = 0; j < m; ++j) {
              if (Pb != nullptr) Pb[i * m + j] = cur[j];
              Ub[i * m + j] = nxt[j];
              cur[j] = nxt[j];
            }
          }

          // apply u to the plant of row b, log the trial (the hand-over's
          // steps 2 - 4 with its noise hooks)
          T x[n], xn[n];
#pragma unroll
          for (int j = 0; j < n; ++j)
            x[j] = a.v_std != nullptr ? a.x_true[(size_t)b * n + j] : z0[j];
          const uint64_t roll = a.rollout_offset + (uint64_t)b;
          const int step = a.step_offset + c;
          {
            ProblemT<T> Pl = P;
            if (a.plant != nullptr)
              write_params_and_goals<T, MODEL>(
                  Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);
#pragma unroll
            for (int j = 0; j < n; ++j)
              a.Xlog[((size_t)b * (TT + 1) + c) * n + j] = x[j];
#pragma unroll
            for (int j = 0; j < m; ++j) a.Ulog[bc * m + j] = u[j];
            const Trig<T, MODEL> tr = trig_of<T, MODEL>(x);
            Jcl += cost_value<T, MODEL>(Pl, x, u, tr, false);
            dynamics<T, MODEL, false>(Pl, x, u, tr, xn, nullptr, nullptr);
            if (a.disturbance != nullptr) {
#pragma unroll
              for (int j = 0; j < n; ++j)
                xn[j] = xn[j] + a.disturbance[bc * n + j];
            }
            if (a.w_std != nullptr) {
              T wn[n];
              draw_units<T, n>(a.seed, roll, step, 0, wn);
              add_scaled<T, n>(a.w_std, wn, xn);
            }
            if (c == TT - 1) {
#pragma unroll
              for (int j = 0; j < n; ++j)
                a.Xlog[((size_t)b * (TT + 1) + TT) * n + j] = xn[j];
              Jcl += cost_value<T, MODEL>(Pl, xn, nullptr,
                                          trig_of<T, MODEL>(xn), true);
            }
            a.Jcl[b] = Jcl;
          }
          // observe: x' stays the plant's, the controller gets y'
          if (a.v_std != nullptr) {
            T vn[n];
#pragma unroll
            for (int j = 0; j < n; ++j) a.x_true[(size_t)b * n + j] = xn[j];
            draw_units<T, n>(a.seed, roll, step + 1, 1, vn);
            add_scaled<T, n>(a.v_std, vn, xn);
            if (a.Ylog != nullptr) {
#pragma unroll
              for (int j = 0; j < n; ++j)
                a.Ylog[((size_t)b * (TT + 1) + c + 1) * n + j] = xn[j];
            }
          }
#pragma unroll
          for (int j = 0; j < n; ++j) a.z0[(size_t)b * n + j] = xn[j];
        }
      }
      hand_over();
    }
  }

  // the rollout of the shifted plan, clamped, from what the controller sees
  // now, under the controller's model (the head re-reads its own stores)
  if (head) {
    T* Zb = a.Z + (size_t)b * (N + 1) * n;
    T z[n], zn[n], u[m];
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = a.z0[(size_t)b * n + j];
      Zb[j] = z[j];
    }
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < m; ++j) {
        u[j] = Ub[i * m + j];
        if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
      }
      const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
      dynamics<T, MODEL, false>(P, z, u, tr, zn, nullptr, nullptr);
#pragma unroll
      for (int j = 0; j < n; ++j) {
        z[j] = zn[j];
        Zb[(i + 1) * n + j] = z[j];
      }
    }
  }
}

// ---- host path ---------------------------------------------------------------

template <typename T, int MODEL>
static int launch_mppi_trial(const pddp_problem& p, MppiTrialArgs<T> a,
                             hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  ClosedLoopArgs<T> g{};  // (the mapping is closed_loop's: its geometry)
  g.B = a.B;
  g.S = a.S;
  dim3 blocks;
  const int threads = closed_loop_geometry(g, blocks);
  a.G = g.G;
  PDDP_LAUNCH((mppi_trial_kernel<T, MODEL>), blocks, dim3(threads), 0, st, P,
              a);
  return launch_status();
}

template <typename T>
static int mppi_trial_impl(const pddp_problem* p, MppiTrialArgs<T> a,
                           double smooth, void* stream) {
  if (a.B <= 0 || a.N <= 0 || a.S <= 0 ||
      (long long)a.B * a.S > 0x7fffffffLL || !a.z0 || !a.U || !a.a_std ||
      !a.lam || !a.Jc || !(smooth >= 0.0 && smooth < 1.0))  // (NaN fails both)
    return PDDP_E_BADARG;
  if (a.K < 1 || a.TT < 1 || a.t0 < 0 || a.count < 1 ||
      (long long)a.t0 + a.count > a.TT || !a.Z || !a.U_work || !a.Xlog ||
      !a.Ulog || !a.Jcl || a.U_work == a.U ||
      (a.v_std != nullptr && a.x_true == nullptr) ||
      // (step_offset + c + 1 is a counter word of the draws: an int)
      a.step_offset < 0 || a.step_offset > INT_MAX - a.TT)
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  a.beta = (T)smooth;
  a.gamma = (T)std::sqrt(1.0 - smooth * smooth);
  if (a.v_std == nullptr) a.x_true = a.Ylog = nullptr;
  PDDP_DISPATCH_MODEL(launch_mppi_trial, T, p, a, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_MPPI_TRIAL_ENTRY_POINT(SUF, T)                                    \
  int pddp_mppi_trial_##SUF(                                                   \
      const pddp_problem* p, const T* table, const T* plant, int B, int N,     \
      int S, int K, int TT, int t0, int count, T* z0, T* U, T* Z, T* U_work,   \
      const T* u_min, const T* u_max, const T* a_std, const T* lam,            \
      double smooth, uint64_t seed, uint64_t cand_offset,                      \
      uint64_t iter_stride, const T* disturbance, const T* w_std,              \
      const T* v_std, uint64_t rollout_offset, int step_offset, T* x_true,     \
      const uint8_t* active, T* Jc, int log_costs, T* Xlog, T* Ulog, T* Jcl,   \
      T* Ylog, T* J0_log, T* Jw_log, T* ess_log, T* plan_log, void* stream) {  \
    return pddp::mppi_trial_impl<T>(                                           \
        p,                                                                     \
        {B,         N,           S,        0,           K,                     \
         TT,        t0,          count,    table,       plant,                 \
         z0,        U,           Z,        U_work,      u_min,                 \
         u_max,     a_std,       lam,      T(0),        T(0),                  \
         seed,      cand_offset, iter_stride, disturbance, w_std,              \
         v_std,     rollout_offset, step_offset, x_true, active,               \
         Jc,        log_costs,   Xlog,     Ulog,        Jcl,                   \
         Ylog,      J0_log,      Jw_log,   ess_log,     plan_log},             \
        smooth, stream);                                                       \
  }

PDDP_MPPI_TRIAL_ENTRY_POINT(f32, float)
PDDP_MPPI_TRIAL_ENTRY_POINT(f64, double)
#undef PDDP_MPPI_TRIAL_ENTRY_POINT

}  // extern "C"
