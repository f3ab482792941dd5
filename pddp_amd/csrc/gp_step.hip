// gp_step.hip - the GP step's resident kernels (every per-training-point table
// of a row in LDS), the choice between them and the chunked form
// (gp_step_chunked.hip) and the C entry points.  The body: gp_step_body.hpp.
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

template <typename T, int E, int D>
int launch(const Args<T>& a, bool jac, hipStream_t st) {
  const int K = a.n + a.m_act;
  if (K > 64) return PDDP_E_UNSUPPORTED;
  int C;
  const int form = form_of<E, D>(a.M, K, jac, (int)sizeof(T), C);
  if (form < 0) return PDDP_E_UNSUPPORTED;
  if (form == 1) return launch_chunked<T, E, D>(a, jac, C, g_force_rows.load(), st);
  const Lds<E, D> o = lds_of<E, D>(a.M, K, jac, (int)sizeof(T));
  const size_t bytes = (size_t)o.total * sizeof(T);
  auto kern = Kernels<T, E, D>::pick(jac);
  if (bytes > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(a.R), dim3(kThreads), bytes, st, a);
  return (int)hipGetLastError();
}

template <typename T, int E, int D>
int launch_roll(Args<T> a, Roll<T> r, hipStream_t st) {
  if (a.n + a.m_act > 64 || r.na > 8 || r.na != a.n_non + 2 * a.n_ang || a.m_act > kMaxAct)
    return PDDP_E_UNSUPPORTED;
  int C;
  const int form = form_of<E, D>(a.M, a.n + a.m_act, false, (int)sizeof(T), C);
  if (form < 0) return PDDP_E_UNSUPPORTED;
  if (form == 1) return launch_roll_chunked<T, E, D>(a, r, C, g_force_rows.load(), st);
  const Lds<E, D> o(a.M, a.n + a.m_act, false);
  const size_t bytes = (size_t)o.total * sizeof(T);
  auto kern = RollKernels<T, E, D>::pick();
  if (bytes > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  a.R = r.B * r.A;
  // N steps and the terminal cost: N + 1 launches, nothing between them
  for (int t = 0; t <= r.N; ++t) {
    r.t = t;
    r.terminal = t == r.N ? 1 : 0;
    hipLaunchKernelGGL(kern, dim3(a.R), dim3(kThreads), bytes, st, a, r);
  }
  return (int)hipGetLastError();
}

template <typename T>
int fill_model(const pddp_gp_model* g, Args<T>& a) {
  if (g == nullptr) return PDDP_E_BADARG;
  if (!g->Xt || !g->Xt_pairs || !g->beta || !g->beta_pairs || !g->Kinv || !g->inv_ell2 || !g->sf2 || !g->sn2)
    return PDDP_E_BADARG;
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
  if (int rc = fill_model<T>(g, a)) return rc;
  Roll<T> r;
  r.B = q->B; r.N = q->N; r.A = q->A; r.t = 0; r.terminal = 0;
  r.na = g->n_non + 2 * g->n_ang;
  r.Z = (const T*)q->Z; r.U = (const T*)q->U; r.gains = (const T*)q->gains;
  r.alphas = (const T*)q->alphas; r.u_min = (const T*)q->u_min; r.u_max = (const T*)q->u_max;
  r.active = q->active; r.status = q->bwd_status;
  r.Zc = (T*)q->Zc; r.Uc = (T*)q->Uc; r.Jc = (T*)q->Jc;
  r.Q = (const T*)q->Q; r.Qt = (const T*)q->Q_term; r.Rm = (const T*)q->R;
  r.xg = (const T*)q->x_goal; r.ug = (const T*)q->u_goal;
  const int E = g->state_size, D = g->n_non + 2 * g->n_ang + g->action_size;
  hipStream_t st = (hipStream_t)stream;
  if (E == 2 && D == 4) return launch_roll<T, 2, 4>(a, r, st);
  if (E == 4 && D == 6) return launch_roll<T, 4, 6>(a, r, st);
  if (E == 6 && D == 9) return launch_roll<T, 6, 9>(a, r, st);
  return PDDP_E_UNSUPPORTED;
}

template <typename T>
int step(const pddp_gp_model* g, int R, const T* z, const T* u, T* z_next, T* Fz, T* Fu, void* stream,
         const uint8_t* row_mask = nullptr, int rows_per_mask = 1) {
  if (g == nullptr || R < 0 || z == nullptr || u == nullptr || z_next == nullptr) return PDDP_E_BADARG;
  if (!g->Xt || !g->Xt_pairs || !g->beta || !g->beta_pairs || !g->Kinv || !g->inv_ell2 || !g->sf2 || !g->sn2)
    return PDDP_E_BADARG;
  if ((Fz == nullptr) != (Fu == nullptr)) return PDDP_E_BADARG;
  if (row_mask != nullptr && rows_per_mask < 1) return PDDP_E_BADARG;
  if (R == 0) return 0;
  if (g->n_ang < 0 || g->n_ang > kMaxAng || g->n_non < 0 || g->n_non > kMaxNon) return PDDP_E_BADARG;
  if (g->n_ang + g->n_non != g->state_size || g->M < 1 || g->action_size < 1) return PDDP_E_BADARG;
  const int E = g->state_size, D = g->n_non + 2 * g->n_ang + g->action_size;
  Args<T> a;
  a.R = R;
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
  a.z = z;
  a.u = u;
  a.z_next = z_next;
  a.Fz = Fz;
  a.Fu = Fu;
  a.row_mask = row_mask;
  a.rows_per_mask = rows_per_mask;
  const bool jac = Fz != nullptr;
  hipStream_t st = (hipStream_t)stream;
  // the systems of the reference's examples: pendulum, cartpole, double cartpole
  if (E == 2 && D == 4) return launch<T, 2, 4>(a, jac, st);
  if (E == 4 && D == 6) return launch<T, 4, 6>(a, jac, st);
  if (E == 6 && D == 9) return launch<T, 6, 9>(a, jac, st);
  return PDDP_E_UNSUPPORTED;
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
  long long words = -1;
  if (state_size == 2 && d == 4) words = lds_of<2, 4>(M, inputs, jacobian != 0, element_size).total;
  if (state_size == 4 && d == 6) words = lds_of<4, 6>(M, inputs, jacobian != 0, element_size).total;
  if (state_size == 6 && d == 9) words = lds_of<6, 9>(M, inputs, jacobian != 0, element_size).total;
  return words < 0 ? -1 : words * element_size;
}
static int form_query(int state_size, int d, int M, int inputs, int jacobian, int element_size,
                      int& C) {
  using namespace pddp::gp;
  C = 0;
  if (state_size == 2 && d == 4) return form_of<2, 4>(M, inputs, jacobian != 0, element_size, C);
  if (state_size == 4 && d == 6) return form_of<4, 6>(M, inputs, jacobian != 0, element_size, C);
  if (state_size == 6 && d == 9) return form_of<6, 9>(M, inputs, jacobian != 0, element_size, C);
  return -1;
}
int pddp_gp_step_form(int state_size, int d, int M, int inputs, int jacobian, int element_size) {
  int C;
  return form_query(state_size, d, M, inputs, jacobian, element_size, C);
}
int pddp_gp_step_chunk(int state_size, int d, int M, int inputs, int jacobian, int element_size) {
  int C;
  return form_query(state_size, d, M, inputs, jacobian, element_size, C) < 0 ? -1 : C;
}
long long pddp_gp_step_chunked_lds_bytes(int state_size, int d, int C, int inputs, int jacobian,
                                         int element_size) {
  using namespace pddp::gp;
  long long words = -1;
  if (C < 1) return -1;
  if (state_size == 2 && d == 4) words = chunked_words<2, 4>(C, inputs, jacobian != 0);
  if (state_size == 4 && d == 6) words = chunked_words<4, 6>(C, inputs, jacobian != 0);
  if (state_size == 6 && d == 9) words = chunked_words<6, 9>(C, inputs, jacobian != 0);
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
