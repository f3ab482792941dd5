// tracking.hip - reference tracking: the derivative records, the line search
// and the MPC hand-over with a goal PER TIME STEP (the pddp_*_track_* entry
// points, ILQRSolver.set_reference).
//
//   `ref` [B][ref_len][PDDP_REF_ROW]: x_goal (augmented coordinates) and u_goal
//   of trajectory b at every step of its reference (include/pddp_hip.h).
//   Horizon index i = 0 .. N reads row min(ref_t0 + i, ref_len - 1): the last
//   row is held.  Q, Q_term, R, the model, the encoding and the bounds stay
//   those of the pddp_problem; the model parameters are row b of `table` where
//   one is given (a run-time case, as in mpc_advance_kernel), else the
//   problem's.
//
// The backward sweep on records and the accept kernel never see the problem,
// so a round with a reference is derivs(track), backward, line_search(track),
// accept; only the integer `ref_t0` moves from one MPC control step to the
// next.
//
// A translation unit of its own: it includes models.hpp and problem_args.hpp
// as they are and shares no text with problem_kernels.hip or mpc_advance.hip
// (csrc/Makefile: moving shared text around changes the FMA contraction of the
// kernels there).  The loops below are those of derivs_body.inc,
// line_search_body.inc and mpc_advance_kernel, with the goals of `P` taken
// from a reference row where those read one problem.
#include <type_traits>
#include "models.hpp"
#include "problem_args.hpp"
#include "model_params.hpp"

namespace pddp {

// where the goals come from; ref_t0 arrives clamped to ref_len - 1, so that
// `ref_t0 + min(i, hold)` neither leaves the reference nor overflows
template <typename T>
struct RefArgs {
  const T* table;  // [B][PDDP_BATCH_ROW] or NULL: the model parameters
  const T* ref;    // [B][ref_len][PDDP_REF_ROW]
  int ref_len, ref_t0;
};

template <typename T>
PDDP_DEV const T* ref_row(const RefArgs<T>& r, int b, int i) {
  const int hold = r.ref_len - 1 - r.ref_t0;
  const int row = r.ref_t0 + (i < hold ? i : hold);
  return r.ref + ((size_t)b * r.ref_len + row) * PDDP_REF_ROW;
}

// the model parameters of `row` (the table's layout) written over P's
template <typename T, int MODEL>
PDDP_DEV void overwrite_params(ProblemT<T>& P, const T* row) {
  P.dt = row[PDDP_BATCH_PARAMS];
#pragma unroll
  for (int i = 0; i < kModelParamCount<MODEL> - 1; ++i)
    P.p[i] = row[PDDP_BATCH_PARAMS + 1 + i];
}

// --------------------------------------------------------------------------
// derivative records: one workgroup per trajectory, one lane per time step,
// records staged through LDS (derivs_body.inc); lane t takes its goals from
// its own reference row
// --------------------------------------------------------------------------

constexpr int kTrackDerivThreads = 64;

template <typename T, int MODEL>
__global__ __launch_bounds__(kTrackDerivThreads) void track_derivs_kernel(
    ProblemT<T> shared, DerivArgs<T> a, RefArgs<T> r) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  constexpr RecLayout lay(n, m);
  constexpr int S = lay.stride;
  constexpr int LD = kTrackDerivThreads + 1;  // conflict-free transposed reads
  __shared__ T stage[S * LD];
  __shared__ T Lsum[kTrackDerivThreads];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  ProblemT<T> P = shared;
  if (r.table != nullptr)
    overwrite_params<T, MODEL>(P, r.table + (size_t)b * PDDP_BATCH_ROW);
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  const int N = a.N;
  const T* Zb = a.Z + (size_t)b * (N + 1) * n;
  const T* Ub = a.U + (size_t)b * N * m;
  T* rec_b = a.rec + (size_t)b * (N + 1) * S;
  T Jacc = T(0);  // only meaningful in lane 0

  for (int t0 = 0; t0 <= N; t0 += kTrackDerivThreads) {
    const int t = t0 + tid;
    T l = T(0);
    if (t <= N) {
      T z[n], un[m], w[S];
      const T* row = ref_row(r, b, t);
#pragma unroll
      for (int j = 0; j < n; ++j) z[j] = Zb[t * n + j];
      const bool terminal = (t == N);
#pragma unroll
      for (int j = 0; j < m; ++j) un[j] = terminal ? T(0) : Ub[t * m + j];
#pragma unroll
      for (int i = 0; i < D::na; ++i) P.goal[i] = row[PDDP_REF_X_GOAL + i];
      // `terminal` a constant in each call: batch_derivs_kernel's note on a
      // run-time choice between two members of a copy (problem_kernels.hip)
      if (terminal) {
        l = record_of<T, MODEL>(P, z, un, true, bounded, a.u_min, a.u_max, w);
      } else {
#pragma unroll
        for (int i = 0; i < m; ++i) P.ugoal[i] = row[PDDP_REF_U_GOAL + i];
        l = record_of<T, MODEL>(P, z, un, false, bounded, a.u_min, a.u_max, w);
      }
      T* col = stage + tid;
#pragma unroll
      for (int j = 0; j < S; ++j) col[j * LD] = w[j];
      a.L[(size_t)b * (N + 1) + t] = l;
    }
    Lsum[tid] = l;
    __syncthreads();
    // coalesced write-out of this chunk's records
    const int nrec = min(kTrackDerivThreads, N + 1 - t0);
    T* dst = rec_b + (size_t)t0 * S;
    for (int o = tid; o < nrec * S; o += kTrackDerivThreads) {
      const int rr = o / S, w = o - rr * S;
      dst[o] = stage[w * LD + rr];
    }
    if (tid == 0)
      for (int rr = 0; rr < nrec; ++rr) Jacc += Lsum[rr];  // L.sum(), t order
    __syncthreads();
  }
  if (tid == 0) {
    a.J[b] = Jacc;
    if (a.state != nullptr) a.state[b] = PDDP_STATE_UNDEFINED;
  }
}

// --------------------------------------------------------------------------
// line search: one lane per (trajectory, alpha) candidate, any A
// (line_search_body.inc); the goal row of step t + 1 is requested together
// with that step's nominal row and gains, ahead of the dependent chain.  The
// A lanes of a trajectory read the same addresses: one broadcast.
// --------------------------------------------------------------------------

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void track_line_search_kernel(
    ProblemT<T> shared, LineSearchArgs<T> a, RefArgs<T> r) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m, na = D::na;
  constexpr int GS = m + m * n;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = a.B * a.A;
  if (idx >= total) return;
  const int b = idx / a.A, ai = idx - b * a.A;
  if (a.active != nullptr && a.active[b] == 0) return;
  if (a.bwd_status != nullptr && a.bwd_status[b] != 0) return;
  ProblemT<T> P = shared;
  if (r.table != nullptr)
    overwrite_params<T, MODEL>(P, r.table + (size_t)b * PDDP_BATCH_ROW);
  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  T umin[m], umax[m];
#pragma unroll
  for (int j = 0; j < m; ++j) {
    umin[j] = bounded ? a.u_min[j] : T(0);
    umax[j] = bounded ? a.u_max[j] : T(0);
  }
  const int N = a.N;
  const T alpha = a.alphas[ai];
  const T* Zb = a.Z + (size_t)b * (N + 1) * n;
  const T* Ub = a.U + (size_t)b * N * m;
  const T* Gb = a.gains + (size_t)b * N * GS;

  T z[n], zn[n], un[m];
  T zr[n], ur[m], gr[GS];  // this step's nominal z, u and gains
#pragma unroll
  for (int j = 0; j < n; ++j) {
    zr[j] = Zb[j];
    z[j] = zr[j];  // Z_new[0] = Z[0]                             (ilqr.py:690)
  }
#pragma unroll
  for (int j = 0; j < m; ++j) ur[j] = Ub[j];
#pragma unroll
  for (int j = 0; j < GS; ++j) gr[j] = Gb[j];
  {
    const T* row = ref_row(r, b, 0);
#pragma unroll
    for (int i = 0; i < na; ++i) P.goal[i] = row[PDDP_REF_X_GOAL + i];
#pragma unroll
    for (int i = 0; i < m; ++i) P.ugoal[i] = row[PDDP_REF_U_GOAL + i];
  }

  // time-major output [b][t][alpha][.] (the note at LineSearchArgs)
  T* Zci = a.Zc + ((size_t)b * (N + 1) * a.A + ai) * n;
  T* Uci = a.Uc + ((size_t)b * N * a.A + ai) * m;
  const size_t zstep = (size_t)a.A * n, ustep = (size_t)a.A * m;
  T J = T(0);
  for (int t = 0; t < N; ++t) {
    // prefetch the next step's nominal data and goals before the dependent
    // chain (the goals up to row N: the terminal cost's)
    T zr2[n], ur2[m], gr2[GS], xg2[na], ug2[m];
    const int tn = (t + 1 < N) ? t + 1 : t;
    const T* row = ref_row(r, b, t + 1);
#pragma unroll
    for (int j = 0; j < n; ++j) zr2[j] = Zb[tn * n + j];
#pragma unroll
    for (int j = 0; j < m; ++j) ur2[j] = Ub[tn * m + j];
#pragma unroll
    for (int j = 0; j < GS; ++j) gr2[j] = Gb[tn * GS + j];
#pragma unroll
    for (int i = 0; i < na; ++i) xg2[i] = row[PDDP_REF_X_GOAL + i];
#pragma unroll
    for (int i = 0; i < m; ++i) ug2[i] = row[PDDP_REF_U_GOAL + i];

#pragma unroll
    for (int j = 0; j < m; ++j) {
      T du = alpha * gr[j];  // alpha * k[i]                      (ilqr.py:708)
      T s = T(0);
#pragma unroll
      for (int c = 0; c < n; ++c) s += (z[c] - zr[c]) * gr[m + j * n + c];
      du = du + s;  // + dz K^T                                   (ilqr.py:710)
      T v = ur[j] + du;
      un[j] = bounded ? clamp_nan(v, umin[j], umax[j]) : v;
    }
#pragma unroll
    for (int j = 0; j < n; ++j) Zci[(size_t)t * zstep + j] = z[j];
#pragma unroll
    for (int j = 0; j < m; ++j) Uci[(size_t)t * ustep + j] = un[j];
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    J += cost_value<T, MODEL>(P, z, un, tr, false);
    dynamics<T, MODEL, false>(P, z, un, tr, zn, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = zn[j];
      zr[j] = zr2[j];
    }
#pragma unroll
    for (int j = 0; j < m; ++j) {
      ur[j] = ur2[j];
      P.ugoal[j] = ug2[j];
    }
#pragma unroll
    for (int j = 0; j < GS; ++j) gr[j] = gr2[j];
#pragma unroll
    for (int i = 0; i < na; ++i) P.goal[i] = xg2[i];
  }
#pragma unroll
  for (int j = 0; j < n; ++j) Zci[(size_t)N * zstep + j] = z[j];
  const T lf = cost_value<T, MODEL>(P, z, nullptr, trig_of<T, MODEL>(z), true);
  a.Jc[idx] = J + lf;  // L.sum(0) + l_f                           (ilqr.py:789)
}

// --------------------------------------------------------------------------
// the hand-over between two control steps of an MPC trial (mpc_advance_kernel,
// one lane per trajectory): the stage cost logged at control step t is taken
// under reference row ref_t0, the terminal cost at t == T - 1 under row
// ref_t0 + 1 (both clamped).  Dynamics, shift, rollout and re-arm read no goal.
// --------------------------------------------------------------------------

constexpr int kTrackLiveShards = PDDP_LIVE_SHARDS;

template <typename T>
struct TrackAdvanceArgs {
  int B, N, T_, t;   // control step t of T_
  const T* plant;    // [B][PDDP_BATCH_ROW] or NULL: the plant's parameters
  T* z0;             // [B][n]       in: x_t, out: x_{t+1}
  T* U;              // [B][N][m]    shifted in place (unclamped)
  T* Z;              // [B][N+1][n]  out: the rollout of the shifted nominal
  const T* u_min;
  const T* u_max;
  const T* disturbance;  // [B][T_][n] or NULL
  const uint8_t* mask;   // [B] or NULL
  T* Xlog;               // [B][T_+1][n]
  T* Ulog;               // [B][T_][m]
  T* Jcl;                // [B]
  int32_t* state_log;    // [B][T_]
  uint8_t* live_log;     // [B][T_]
  double* mu;
  double* delta;
  int32_t* state;
  int32_t* iter;
  uint8_t* active;
  uint8_t* fresh;
  int32_t* n_live;  // [PDDP_LIVE_SHARDS] or NULL
};

template <typename T, int MODEL>
__global__ __launch_bounds__(kWave) void track_mpc_advance_kernel(
    ProblemT<T> shared, TrackAdvanceArgs<T> a, RefArgs<T> r) {
  using D = ModelDims<MODEL>;
  constexpr int n = D::n, m = D::m;
  if (blockIdx.x == 0 && a.n_live != nullptr) {
    for (int i = threadIdx.x; i < kTrackLiveShards; i += blockDim.x)
      a.n_live[i] = 0;
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  if (a.mask != nullptr && a.mask[b] == 0) return;
  const int N = a.N, t = a.t, TT = a.T_;

  // 1. the controller as the step's rounds left it
  a.state_log[(size_t)b * TT + t] = a.state[b];
  a.live_log[(size_t)b * TT + t] = a.active[b] != 0 ? 1 : 0;

  const bool bounded = a.u_min != nullptr && a.u_max != nullptr;
  T umin[m], umax[m];
#pragma unroll
  for (int j = 0; j < m; ++j) {
    umin[j] = bounded ? a.u_min[j] : T(0);
    umax[j] = bounded ? a.u_max[j] : T(0);
  }
  T* Zb = a.Z + (size_t)b * (N + 1) * n;
  T* Ub = a.U + (size_t)b * N * m;
  T* Xb = a.Xlog + (size_t)b * (TT + 1) * n;

  // the controller's model (its goals are not read here)
  ProblemT<T> P = shared;
  if (r.table != nullptr)
    overwrite_params<T, MODEL>(P, r.table + (size_t)b * PDDP_BATCH_ROW);

  T z[n], zn[n], u[m], cur[m], nxt[m];
#pragma unroll
  for (int j = 0; j < n; ++j) z[j] = a.z0[(size_t)b * n + j];
#pragma unroll
  for (int j = 0; j < m; ++j) {
    u[j] = Ub[j];
    if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
  }
  // the warm start's first row, requested ahead of the plant step
  const int i1 = N > 1 ? 1 : 0;
#pragma unroll
  for (int j = 0; j < m; ++j) cur[j] = Ub[i1 * m + j];

  {
    // 2. - 4. apply u to the plant of row b, log the trial under the
    // reference: the plant row supplies the parameters only
    ProblemT<T> Pl = P;
    if (a.plant != nullptr)
      overwrite_params<T, MODEL>(Pl, a.plant + (size_t)b * PDDP_BATCH_ROW);
    const T* row = ref_row(r, b, 0);
#pragma unroll
    for (int i = 0; i < D::na; ++i) Pl.goal[i] = row[PDDP_REF_X_GOAL + i];
#pragma unroll
    for (int i = 0; i < m; ++i) Pl.ugoal[i] = row[PDDP_REF_U_GOAL + i];
    T w[n];
#pragma unroll
    for (int j = 0; j < n; ++j) w[j] = T(0);
    if (a.disturbance != nullptr) {
#pragma unroll
      for (int j = 0; j < n; ++j)
        w[j] = a.disturbance[((size_t)b * TT + t) * n + j];
    }
    T J = T(0);
    if (t > 0) J = a.Jcl[b];
#pragma unroll
    for (int j = 0; j < n; ++j) Xb[(size_t)t * n + j] = z[j];
#pragma unroll
    for (int j = 0; j < m; ++j) a.Ulog[((size_t)b * TT + t) * m + j] = u[j];
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    J += cost_value<T, MODEL>(Pl, z, u, tr, false);
    dynamics<T, MODEL, false>(Pl, z, u, tr, zn, nullptr, nullptr);
    if (a.disturbance != nullptr) {
#pragma unroll
      for (int j = 0; j < n; ++j) zn[j] = zn[j] + w[j];
    }
#pragma unroll
    for (int j = 0; j < n; ++j) z[j] = zn[j];
    if (t == TT - 1) {
      const T* row1 = ref_row(r, b, 1);
#pragma unroll
      for (int i = 0; i < D::na; ++i) Pl.goal[i] = row1[PDDP_REF_X_GOAL + i];
#pragma unroll
      for (int j = 0; j < n; ++j) Xb[(size_t)TT * n + j] = z[j];
      J += cost_value<T, MODEL>(Pl, z, nullptr, trig_of<T, MODEL>(z), true);
    }
    a.Jcl[b] = J;
  }

  // 5. + 6. the shift (new row i is old row i + 1, the last one repeated) and
  // the rollout of the shifted nominal from x' under the controller's model,
  // in one loop over time.  Row i + 2 is read before row i is written; the
  // last row is read for the last time in the iteration before it is written.
#pragma unroll
  for (int j = 0; j < n; ++j) {
    a.z0[(size_t)b * n + j] = z[j];
    Zb[j] = z[j];
  }
  for (int i = 0; i < N; ++i) {
    const int i2 = (i + 2 < N) ? i + 2 : N - 1;
#pragma unroll
    for (int j = 0; j < m; ++j) nxt[j] = Ub[i2 * m + j];
#pragma unroll
    for (int j = 0; j < m; ++j) {
      Ub[i * m + j] = cur[j];
      u[j] = cur[j];
      if (bounded) u[j] = clamp1(u[j], umin[j], umax[j]);
    }
    const Trig<T, MODEL> tr = trig_of<T, MODEL>(z);
    dynamics<T, MODEL, false>(P, z, u, tr, zn, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      z[j] = zn[j];
      Zb[(i + 1) * n + j] = z[j];
    }
#pragma unroll
    for (int j = 0; j < m; ++j) cur[j] = nxt[j];
  }

  // 7. re-arm: the words of reset_controller_state()       (ilqr.py:364-367)
  a.mu[b] = 0.0;
  a.delta[b] = 2.0;
  a.state[b] = PDDP_STATE_UNDEFINED;
  a.iter[b] = 1;
  a.active[b] = 1;
  a.fresh[b] = 1;
}

// --------------------------------------------------------------------------
// launchers and entry points
// --------------------------------------------------------------------------

template <typename Args, typename T>
struct WithRef {
  Args a;
  RefArgs<T> r;
};

template <typename T, int MODEL>
static int launch_track_derivs(const pddp_problem& p,
                               WithRef<DerivArgs<T>, T> w, hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  PDDP_LAUNCH((track_derivs_kernel<T, MODEL>), dim3(w.a.B),
              dim3(kTrackDerivThreads), 0, st, P, w.a, w.r);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_track_line_search(const pddp_problem& p,
                                    WithRef<LineSearchArgs<T>, T> w,
                                    hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const dim3 lanes((unsigned)(((long long)w.a.B * w.a.A + kWave - 1) / kWave));
  PDDP_LAUNCH((track_line_search_kernel<T, MODEL>), lanes, dim3(kWave), 0, st,
              P, w.a, w.r);
  return launch_status();
}
template <typename T, int MODEL>
static int launch_track_advance(const pddp_problem& p,
                                WithRef<TrackAdvanceArgs<T>, T> w,
                                hipStream_t st) {
  const ProblemT<T> P = convert_problem<T>(p);
  const dim3 blocks((w.a.B + kWave - 1) / kWave);
  PDDP_LAUNCH((track_mpc_advance_kernel<T, MODEL>), blocks, dim3(kWave), 0, st,
              P, w.a, w.r);
  return launch_status();
}

// ref_t0 clamped to the last row here (see RefArgs); false: PDDP_E_BADARG
template <typename T>
static bool ref_args(const T* table, const T* ref, int ref_len, int ref_t0,
                     RefArgs<T>* out) {
  if (ref == nullptr || ref_len < 1 || ref_t0 < 0) return false;
  *out = RefArgs<T>{table, ref, ref_len,
                    ref_t0 < ref_len - 1 ? ref_t0 : ref_len - 1};
  return true;
}

template <typename T>
static int track_derivs_impl(const pddp_problem* p, const T* table,
                             const T* ref, int ref_len, int ref_t0, int B,
                             int N, const T* Z, const T* U, const T* u_min,
                             const T* u_max, const uint8_t* mask, T* rec, T* L,
                             T* J, int32_t* state, void* stream) {
  WithRef<DerivArgs<T>, T> w{
      {B, N, Z, U, u_min, u_max, mask, rec, L, J, state}, {}};
  if (B <= 0 || N <= 0 || !Z || !U || !rec || !L || !J ||
      !ref_args(table, ref, ref_len, ref_t0, &w.r))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_derivs, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int track_line_search_impl(const pddp_problem* p, const T* table,
                                  const T* ref, int ref_len, int ref_t0, int B,
                                  int N, int A, const T* Z, const T* U,
                                  const T* gains, const T* alphas,
                                  const T* u_min, const T* u_max,
                                  const uint8_t* active,
                                  const int32_t* bwd_status, T* Zc, T* Uc,
                                  T* Jc, void* stream) {
  WithRef<LineSearchArgs<T>, T> w{{B, N, A, Z, U, gains, alphas, u_min, u_max,
                                   active, bwd_status, Zc, Uc, Jc},
                                  {}};
  if (B <= 0 || N <= 0 || A <= 0 || !Z || !U || !gains || !alphas || !Zc ||
      !Uc || !Jc || !ref_args(table, ref, ref_len, ref_t0, &w.r))
    return PDDP_E_BADARG;
  // (the kernel's int lane index)
  if ((long long)B * A > 0x7fffffffLL) return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_line_search, T, p, w, (hipStream_t)stream)
}

template <typename T>
static int track_advance_impl(const pddp_problem* p, const T* table,
                              const T* ref, int ref_len, int ref_t0, int B,
                              int N, int TT, int t, T* z0, T* U, T* Z,
                              const T* u_min, const T* u_max, const T* plant,
                              const T* disturbance, const uint8_t* mask,
                              T* Xlog, T* Ulog, T* Jcl, int32_t* state_log,
                              uint8_t* live_log, double* mu, double* delta,
                              int32_t* state, int32_t* iter, uint8_t* active,
                              uint8_t* fresh, int32_t* n_live, void* stream) {
  WithRef<TrackAdvanceArgs<T>, T> w{
      {B,     N,      TT,        t,        plant, z0,    U,
       Z,     u_min,  u_max,     disturbance,     mask,  Xlog,
       Ulog,  Jcl,    state_log, live_log, mu,    delta, state,
       iter,  active, fresh,     n_live},
      {}};
  if (B <= 0 || N <= 0 || TT <= 0 || t < 0 || t >= TT || !z0 || !U || !Z ||
      !Xlog || !Ulog || !Jcl || !state_log || !live_log || !mu || !delta ||
      !state || !iter || !active || !fresh ||
      !ref_args(table, ref, ref_len, ref_t0, &w.r))
    return PDDP_E_BADARG;
  if (int rc = check_problem(p)) return rc;
  PDDP_DISPATCH_MODEL(launch_track_advance, T, p, w, (hipStream_t)stream)
}

}  // namespace pddp

extern "C" {

#define PDDP_TRACK_ENTRY_POINTS(SUF, T)                                        \
  int pddp_derivs_track_##SUF(                                                 \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, int B, int N, const T* Z, const T* U, const T* u_min,        \
      const T* u_max, const uint8_t* mask, T* rec, T* L, T* J, int32_t* state, \
      void* stream) {                                                          \
    return pddp::track_derivs_impl<T>(p, table, ref, ref_len, ref_t0, B, N, Z, \
                                      U, u_min, u_max, mask, rec, L, J, state, \
                                      stream);                                 \
  }                                                                            \
  int pddp_line_search_track_##SUF(                                            \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, int B, int N, int A, const T* Z, const T* U, const T* gains, \
      const T* alphas, const T* u_min, const T* u_max, const uint8_t* active,  \
      const int32_t* bwd_status, T* Zc, T* Uc, T* Jc, void* stream) {          \
    return pddp::track_line_search_impl<T>(                                    \
        p, table, ref, ref_len, ref_t0, B, N, A, Z, U, gains, alphas, u_min,   \
        u_max, active, bwd_status, Zc, Uc, Jc, stream);                        \
  }                                                                            \
  int pddp_mpc_advance_track_##SUF(                                            \
      const pddp_problem* p, const T* table, const T* ref, int ref_len,        \
      int ref_t0, int B, int N, int TT, int t, T* z0, T* U, T* Z,              \
      const T* u_min, const T* u_max, const T* plant, const T* disturbance,    \
      const uint8_t* mask, T* Xlog, T* Ulog, T* Jcl, int32_t* state_log,       \
      uint8_t* live_log, double* mu, double* delta, int32_t* state,            \
      int32_t* iter, uint8_t* active, uint8_t* fresh, int32_t* n_live,         \
      void* stream) {                                                          \
    return pddp::track_advance_impl<T>(                                        \
        p, table, ref, ref_len, ref_t0, B, N, TT, t, z0, U, Z, u_min, u_max,   \
        plant, disturbance, mask, Xlog, Ulog, Jcl, state_log, live_log, mu,    \
        delta, state, iter, active, fresh, n_live, stream);                    \
  }

PDDP_TRACK_ENTRY_POINTS(f32, float)
PDDP_TRACK_ENTRY_POINTS(f64, double)
#undef PDDP_TRACK_ENTRY_POINTS

}  // extern "C"
