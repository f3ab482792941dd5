// gp_step.hip - the GP step's resident kernels (every per-training-point table
// of a row in LDS) and the host side of both forms: fill_model validates a
// pddp_gp_model and converts it, for_shape dispatches on the built pairs
// (PDDP_GP_SHAPES, gp_step_body.hpp), launch chooses between the resident and
// the chunked form (kernels: gp_step_chunked.hip) and issues every launch of a
// step or a rollout; then the C entry points.  The body: gp_step_body.hpp.
#include <atomic>
#include "gp_step_body.hpp"

namespace pddp {
namespace gp {

// pddp_gp_step_force_chunk / _force_rows_per_launch (tests): 0 = automatic
static std::atomic<int> g_force_chunk{0}, g_force_rows{0};

// 0 resident, 1 chunked, -1 neither; C: the chunk (M for the resident form)
template <int E, int D>
int form_of(int M, int K, bool jac, int element_size, int& C) {
  C = 0;
  if (M < 1 || K < 1 || K > 64 || (element_size != 4 && element_size != 8)) return -1;
  const int forced = g_force_chunk.load();
  const long long bytes = (long long)lds_of<E, D>(M, K, jac, element_size).total * element_size;
  if (bytes <= kGpLdsMax && forced <= 0) {
    C = M;
    return 0;
  }
  C = chunk_of<E, D>(M, K, jac, element_size, forced);
  if (C > 0) return 1;
  if (bytes <= kGpLdsMax) {  // (forced, but the chunked form has no room: resident)
    C = M;
    return 0;
  }
  return -1;
}


template <typename T, int E, int D, bool JAC>
__global__ __launch_bounds__(kThreads) void gp_step_kernel(const Args<T> A) {
  gp_step_body<T, E, D, JAC>(A);
}
#ifndef PDDP_GP_FWD_WAVES
#define PDDP_GP_FWD_WAVES 3
#endif
// The line search's kernel (float, no Jacobian) held to the registers of
// PDDP_GP_FWD_WAVES workgroups per CU: the serial front and back end of a row
// (A0, A1, A3: most of the workgroup waits) are filled by other rows' M^2 loops
template <int E, int D>
__global__ __launch_bounds__(kThreads)
__attribute__((amdgpu_waves_per_eu(PDDP_GP_FWD_WAVES, PDDP_GP_FWD_WAVES)))
void gp_step_fwd_f32_kernel(const Args<float> A) {
  gp_step_body<float, E, D, false>(A);
}
template <typename T, int E, int D>
__global__ __launch_bounds__(kThreads) void gp_roll_kernel(const Args<T> A, const Roll<T> RL) {
  gp_step_body<T, E, D, false, true>(A, RL);
}
template <int E, int D>
__global__ __launch_bounds__(kThreads)
__attribute__((amdgpu_waves_per_eu(PDDP_GP_FWD_WAVES, PDDP_GP_FWD_WAVES)))
void gp_roll_f32_kernel(const Args<float> A, const Roll<float> RL) {
  gp_step_body<float, E, D, false, true>(A, RL);
}
template <typename T, int E, int D>
struct RollKernels {
  static auto pick() { return gp_roll_kernel<T, E, D>; }
};
template <int E, int D>
struct RollKernels<float, E, D> {
  static auto pick() { return gp_roll_f32_kernel<E, D>; }
};

template <typename T, int E, int D>
struct Kernels {
  static auto pick(bool jac) { return jac ? gp_step_kernel<T, E, D, true> : gp_step_kernel<T, E, D, false>; }
};
template <int E, int D>
struct Kernels<float, E, D> {
  static auto pick(bool jac) {
    return jac ? gp_step_kernel<float, E, D, true> : gp_step_fwd_f32_kernel<E, D>;
  }
};

// Rows per launch (chunked form).  A row is one workgroup and almost all of it
// is B: NP pairs
// x M^2 terms at kCyclesPerTerm workgroup cycles each (measured: 3.35 M cycles
// for the float Jacobian row at M = 300, E = 6 - DESIGN.md 3.11 - is 1.8 per
// term; double: about three times that).  One launch gets the rows that 256
// CUs, a workgroup each, work off in kLaunchSeconds at kClockHz - the shared
// card is never held for seconds by one launch - and never fewer than one row
// per CU
constexpr double kCyclesPerTermF32 = 2.0, kCyclesPerTermF64 = 6.0;
constexpr double kLaunchSeconds = 0.15, kClockHz = 2.4e9;
constexpr int kCUs = 256;
template <typename T, int E>
int rows_per_launch_of(int M, int forced) {
  if (forced > 0) return forced;
  const double per_row = (sizeof(T) == 4 ? kCyclesPerTermF32 : kCyclesPerTermF64) *
                         (E * (E + 1) / 2) * (double)M * (double)M;
  const double rows = kLaunchSeconds * kClockHz * kCUs / per_row;
  return rows < kCUs ? kCUs : rows > 1e9 ? 1000000000 : (int)rows;
}

// more than 64 KB of dynamic LDS needs the opt-in
template <typename K>
int allow_lds(K kern, size_t bytes) {
  if (bytes <= 64 * 1024) return 0;
  return (int)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes);
}

// Every launch of one call on the one stream.  A step (roll null): the a.R
// rows; a rollout: its N steps and the terminal cost, N + 1 times the rows
// with nothing between them.  The rows of a time step go out in consecutive
// slices of `per` (rows are independent) - one slice in the resident form, and
// for the terminal launch, which has no M^2 loop.  launch_rows(r, row0, rows)
template <typename T, typename F>
int launch_sliced(int R, int per, const Roll<T>* roll, F&& launch_rows) {
  Roll<T> r = roll != nullptr ? *roll : Roll<T>();
  const int last = roll != nullptr ? r.N : 0;
  for (int t = 0; t <= last; ++t) {
    r.t = t;
    r.terminal = roll != nullptr && t == r.N ? 1 : 0;
    const int step = r.terminal ? R : per;
    for (int row0 = 0; row0 < R; row0 += step)
      launch_rows(r, row0, R - row0 < step ? R - row0 : step);
  }
  return (int)hipGetLastError();
}

// The form, its kernel and LDS, and the launches: of a step, or (roll: B, N, A
// and the pointers filled in) of the line search's rollout, which has no
// Jacobian
template <typename T, int E, int D>
int launch(const Args<T>& a, const Roll<T>* roll, bool jac, hipStream_t st) {
  const int K = a.n + a.m_act;
  if (K > 64) return PDDP_E_UNSUPPORTED;
  if (roll != nullptr &&
      (roll->na > 8 || roll->na != a.n_non + 2 * a.n_ang || a.m_act > kMaxAct))
    return PDDP_E_UNSUPPORTED;
  int C;
  const int form = form_of<E, D>(a.M, K, jac, (int)sizeof(T), C);
  if (form < 0) return PDDP_E_UNSUPPORTED;
  if (form == 1 && (C < 2 || (C & 1))) return PDDP_E_UNSUPPORTED;
  const size_t bytes = sizeof(T) * (size_t)(form == 1 ? chunked_words<E, D>(C, K, jac)
                                                      : lds_of<E, D>(a.M, K, jac, (int)sizeof(T)).total);
  if (bytes > (size_t)kGpLdsMax) return PDDP_E_UNSUPPORTED;
  const int per = form == 1 ? rows_per_launch_of<T, E>(a.M, g_force_rows.load()) : a.R;
  const dim3 block(kThreads);
  auto go = [&](auto kern, auto launch_kernel) {
    if (int rc = allow_lds(kern, bytes)) return rc;
    return launch_sliced<T>(a.R, per, roll, [&](const Roll<T>& r, int row0, int rows) {
      launch_kernel(kern, dim3(rows), r, Chunk{C, row0});
    });
  };
  if (form == 0 && roll == nullptr)
    return go(Kernels<T, E, D>::pick(jac), [&](auto kern, dim3 grid, const Roll<T>&, Chunk) {
      hipLaunchKernelGGL(kern, grid, block, bytes, st, a);
    });
  if (form == 0)
    return go(RollKernels<T, E, D>::pick(), [&](auto kern, dim3 grid, const Roll<T>& r, Chunk) {
      hipLaunchKernelGGL(kern, grid, block, bytes, st, a, r);
    });
  if (roll == nullptr)
    return go(chunked_step_kernel<T, E, D>(jac), [&](auto kern, dim3 grid, const Roll<T>&, Chunk ck) {
      hipLaunchKernelGGL(kern, grid, block, bytes, st, a, ck);
    });
  return go(chunked_roll_kernel<T, E, D>(), [&](auto kern, dim3 grid, const Roll<T>& r, Chunk ck) {
    hipLaunchKernelGGL(kern, grid, block, bytes, st, a, r, ck);
  });
}

// f(E, D) - as integral constants - for a built pair, else `unbuilt`
template <typename R, typename F>
R for_shape(int E, int D, R unbuilt, F&& f) {
#define PDDP_GP_CASE(E_, D_) \
  if (E == E_ && D == D_) return f(std::integral_constant<int, E_>(), std::integral_constant<int, D_>());
  PDDP_GP_SHAPES(PDDP_GP_CASE)
#undef PDDP_GP_CASE
  return unbuilt;
}
template <typename T>
int launch_model(const pddp_gp_model* g, const Args<T>& a, const Roll<T>* roll, bool jac,
                 void* stream) {
  return for_shape<int>(
      g->state_size, g->n_non + 2 * g->n_ang + g->action_size, PDDP_E_UNSUPPORTED,
      [&](auto E, auto D) { return launch<T, E(), D()>(a, roll, jac, (hipStream_t)stream); });
}

// The one place that validates a pddp_gp_model and converts it, in two steps,
// because a step with no rows answers 0 between them: the pointers ...
inline int model_pointers(const pddp_gp_model* g) {
  if (g == nullptr) return PDDP_E_BADARG;
  if (!g->Xt || !g->Xt_pairs || !g->beta || !g->beta_pairs || !g->Kinv || !g->inv_ell2 || !g->sf2 || !g->sn2)
    return PDDP_E_BADARG;
  return 0;
}
// ... then the shapes, the encoding (before the indices' ranges) and the
// conversion; the row arguments are left empty
template <typename T>
int fill_model(const pddp_gp_model* g, Args<T>& a) {
  if (g->n_ang < 0 || g->n_ang > kMaxAng || g->n_non < 0 || g->n_non > kMaxNon) return PDDP_E_BADARG;
  if (g->n_ang + g->n_non != g->state_size || g->M < 1 || g->action_size < 1) return PDDP_E_BADARG;
  const int E = g->state_size;
  a.M = g->M;
  a.m_act = g->action_size;
  a.n_ang = g->n_ang;
  a.n_non = g->n_non;
  a.encoding = g->encoding;
  switch (g->encoding) {
    case 1: a.n = E + E * (E + 1) / 2; break;
    case 2:
    case 3: a.n = 2 * E; break;
    case 4: a.n = E; break;
    default: return PDDP_E_UNSUPPORTED;  // FULL_COVARIANCE_MATRIX: the torch path
  }
  for (int i = 0; i < kMaxAng; ++i) a.ang[i] = i < g->n_ang ? g->ang[i] : 0;
  for (int i = 0; i < kMaxNon; ++i) a.non[i] = i < g->n_non ? g->non[i] : 0;
  for (int i = 0; i < g->n_ang; ++i)
    if (g->ang[i] < 0 || g->ang[i] >= E) return PDDP_E_BADARG;
  for (int i = 0; i < g->n_non; ++i)
    if (g->non[i] < 0 || g->non[i] >= E) return PDDP_E_BADARG;
  a.Xt = (const T*)g->Xt;
  a.XtP = (const T*)g->Xt_pairs;
  a.betaP = (const T*)g->beta_pairs;
  a.beta = (const T*)g->beta;
  a.Kinv = (const T*)g->Kinv;
  a.iL = (const T*)g->inv_ell2;
  a.sf2 = (const T*)g->sf2;
  a.sn2 = (const T*)g->sn2;
  a.R = 0;
  a.z = nullptr; a.u = nullptr; a.z_next = nullptr; a.Fz = nullptr; a.Fu = nullptr;
  a.row_mask = nullptr; a.rows_per_mask = 1;
  return 0;
}

template <typename T>
int rollout(const pddp_gp_model* g, const pddp_gp_rollout* q, void* stream) {
  if (q == nullptr || q->B <= 0 || q->N <= 0 || q->A <= 0 || !q->Z || !q->U || !q->gains ||
      !q->alphas || !q->Zc || !q->Uc || !q->Jc || !q->Q || !q->Q_term || !q->R || !q->x_goal ||
      !q->u_goal || ((q->u_min == nullptr) != (q->u_max == nullptr)))
    return PDDP_E_BADARG;
  Args<T> a;
  if (int rc = model_pointers(g)) return rc;
  if (int rc = fill_model<T>(g, a)) return rc;
  a.R = q->B * q->A;
  Roll<T> r;
  r.B = q->B; r.N = q->N; r.A = q->A; r.t = 0; r.terminal = 0;
  r.na = g->n_non + 2 * g->n_ang;
  r.Z = (const T*)q->Z; r.U = (const T*)q->U; r.gains = (const T*)q->gains;
  r.alphas = (const T*)q->alphas; r.u_min = (const T*)q->u_min; r.u_max = (const T*)q->u_max;
  r.active = q->active; r.status = q->bwd_status;
  r.Zc = (T*)q->Zc; r.Uc = (T*)q->Uc; r.Jc = (T*)q->Jc;
  r.Q = (const T*)q->Q; r.Qt = (const T*)q->Q_term; r.Rm = (const T*)q->R;
  r.xg = (const T*)q->x_goal; r.ug = (const T*)q->u_goal;
  return launch_model<T>(g, a, &r, false, stream);
}

template <typename T>
int step(const pddp_gp_model* g, int R, const T* z, const T* u, T* z_next, T* Fz, T* Fu, void* stream,
         const uint8_t* row_mask = nullptr, int rows_per_mask = 1) {
  if (R < 0 || z == nullptr || u == nullptr || z_next == nullptr) return PDDP_E_BADARG;
  if (int rc = model_pointers(g)) return rc;
  if ((Fz == nullptr) != (Fu == nullptr)) return PDDP_E_BADARG;
  if (row_mask != nullptr && rows_per_mask < 1) return PDDP_E_BADARG;
  if (R == 0) return 0;
  Args<T> a;
  if (int rc = fill_model<T>(g, a)) return rc;
  a.R = R;
  a.z = z;
  a.u = u;
  a.z_next = z_next;
  a.Fz = Fz;
  a.Fu = Fu;
  a.row_mask = row_mask;
  a.rows_per_mask = rows_per_mask;
  return launch_model<T>(g, a, nullptr, Fz != nullptr, stream);
}

// (the queries' arguments: for_shape, then M or C, n + m, jacobian, element size)
static int form_query(int state_size, int d, int M, int inputs, int jacobian, int element_size,
                      int& C) {
  C = 0;
  return for_shape(state_size, d, -1, [&](auto E, auto D) {
    return form_of<E(), D()>(M, inputs, jacobian != 0, element_size, C);
  });
}

}  // namespace gp
}  // namespace pddp

extern "C" {
#ifdef PDDP_GP_MARKS
int pddp_debug_gp_marks(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pddp::gp::g_gp_marks), sizeof(long long) * 64);
}
#endif
long long pddp_gp_step_lds_bytes(int state_size, int d, int M, int inputs, int jacobian,
                                 int element_size) {
  using namespace pddp::gp;
  const long long words = for_shape(state_size, d, -1LL, [&](auto E, auto D) -> long long {
    return lds_of<E(), D()>(M, inputs, jacobian != 0, element_size).total;
  });
  return words < 0 ? -1 : words * element_size;
}
int pddp_gp_step_form(int state_size, int d, int M, int inputs, int jacobian, int element_size) {
  int C;
  return pddp::gp::form_query(state_size, d, M, inputs, jacobian, element_size, C);
}
int pddp_gp_step_chunk(int state_size, int d, int M, int inputs, int jacobian, int element_size) {
  int C;
  return pddp::gp::form_query(state_size, d, M, inputs, jacobian, element_size, C) < 0 ? -1 : C;
}
long long pddp_gp_step_chunked_lds_bytes(int state_size, int d, int C, int inputs, int jacobian,
                                         int element_size) {
  using namespace pddp::gp;
  if (C < 1) return -1;
  const long long words = for_shape(state_size, d, -1LL, [&](auto E, auto D) -> long long {
    return chunked_words<E(), D()>(C, inputs, jacobian != 0);
  });
  return words < 0 ? -1 : words * element_size;
}
int pddp_gp_step_force_chunk(int C) {
  return pddp::gp::g_force_chunk.exchange(C < 0 ? 0 : C);
}
int pddp_gp_step_force_rows_per_launch(int rows) {
  return pddp::gp::g_force_rows.exchange(rows < 0 ? 0 : rows);
}
int pddp_gp_step_f32(const pddp_gp_model* g, int R, const float* z, const float* u, float* z_next,
                     float* Fz, float* Fu, void* stream) {
  return pddp::gp::step<float>(g, R, z, u, z_next, Fz, Fu, stream);
}
int pddp_gp_step_f64(const pddp_gp_model* g, int R, const double* z, const double* u, double* z_next,
                     double* Fz, double* Fu, void* stream) {
  return pddp::gp::step<double>(g, R, z, u, z_next, Fz, Fu, stream);
}
int pddp_gp_step_masked_f32(const pddp_gp_model* g, int R, const float* z, const float* u,
                            float* z_next, float* Fz, float* Fu, const uint8_t* row_mask,
                            int rows_per_mask, void* stream) {
  return pddp::gp::step<float>(g, R, z, u, z_next, Fz, Fu, stream, row_mask, rows_per_mask);
}
int pddp_gp_step_masked_f64(const pddp_gp_model* g, int R, const double* z, const double* u,
                            double* z_next, double* Fz, double* Fu, const uint8_t* row_mask,
                            int rows_per_mask, void* stream) {
  return pddp::gp::step<double>(g, R, z, u, z_next, Fz, Fu, stream, row_mask, rows_per_mask);
}
int pddp_gp_rollout_f32(const pddp_gp_model* g, const pddp_gp_rollout* r, void* stream) {
  return pddp::gp::rollout<float>(g, r, stream);
}
int pddp_gp_rollout_f64(const pddp_gp_model* g, const pddp_gp_rollout* r, void* stream) {
  return pddp::gp::rollout<double>(g, r, stream);
}
}
