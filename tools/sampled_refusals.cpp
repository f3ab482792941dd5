// sampled_refusals.cpp - every entry point of the sampling planners
// (pddp_shoot_* and pddp_mppi_* in their five forms, pddp_shoot_draws_*,
// pddp_mppi_trial_*, pddp_mppi_trial_goals_*; f32 and f64) called with argument
// sets it must refuse before any launch, each alone and paired with a problem
// that check_problem refuses (NULL, another encoding, another model), so that
// the order in which the argument test and check_problem are reached shows in
// the code returned.  Prints one line per call; two builds of the library
// refuse alike when their outputs are the same text.  A
// stand-alone program for the CPU: nothing here reaches a launch, the pointers
// are addresses nobody reads.
//
//   hipcc -std=c++17 -I include tools/sampled_refusals.cpp \
//       -L pddp_amd/lib -lpddp_hip -Wl,-rpath,$PWD/pddp_amd/lib -o refusals
//
// Under the sanitizers the host code under test is compiled into the program
// (its definitions then take precedence over the library's; run on the CPU):
//   hipcc -std=c++17 --offload-arch=gfx950 -fPIC -fno-slp-vectorize \
//       -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//       -I include tools/sampled_refusals.cpp pddp_amd/csrc/shoot.hip \
//       pddp_amd/csrc/mppi.hip pddp_amd/csrc/mppi_trial.hip \
//       -L pddp_amd/lib -lpddp_hip -Wl,-rpath,$PWD/pddp_amd/lib -o refusals
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "pddp_hip.h"

namespace {

enum Family { SHOOT = 1, MPPI = 2, TRIAL = 4, TRIAL_GOALS = 8, DRAWS = 16 };
enum Form { PLAIN = 1, BATCH = 2, TRACK = 4, WEIGHTED = 8, TRACK_WEIGHTED = 16 };
constexpr int ALL_FORMS = 31, WITH_REF = TRACK | TRACK_WEIGHTED,
              WITH_WEIGHTS = WEIGHTED | TRACK_WEIGHTED;

template <typename T>
T* at(uintptr_t k) {  // a distinct address per argument, never read
  return reinterpret_cast<T*>(0x10000 + 0x1000 * k);
}

// every argument of every entry point, valid as set here
template <typename T>
struct Args {
  const T *table = at<T>(1), *plant = at<T>(2), *ref = at<T>(3),
          *weights = at<T>(4);
  int ref_len = 4, ref_t0 = 1;
  int B = 3, N = 6, S = 70, m = 1, K = 2, TT = 3, t0 = 0, count = 3;
  T *z0 = at<T>(5), *U = at<T>(6), *Z = at<T>(7), *U_work = at<T>(8);
  const T *u_min = at<T>(9), *u_max = at<T>(10), *a_std = at<T>(11),
          *lam = at<T>(12);
  double smooth = 0.5;
  const T *disturbance = nullptr, *w_std = nullptr, *v_std = nullptr;
  int step_offset = 2;
  T* x_true = at<T>(13);
  T* Jc = at<T>(14);
  int32_t* best = at<int32_t>(15);
  T *J_best = at<T>(16), *W = at<T>(17), *J_w = at<T>(18), *Z_out = at<T>(19),
    *U_out = at<T>(20), *E = at<T>(21);
  T *Xlog = at<T>(22), *Ulog = at<T>(23), *Jcl = at<T>(24), *Ylog = at<T>(25);
};

template <typename T>
struct Refusal {
  const char* name;
  int families, forms;
  bool passes;  // the argument test lets it through: only run with a bad problem
  std::function<void(Args<T>&)> set;
};

template <typename T>
std::vector<Refusal<T>> refusals() {
  using A = Args<T>;
  const int planners = SHOOT | MPPI, trials = TRIAL | TRIAL_GOALS,
            sampled = planners | trials, all = sampled | DRAWS;
  return {
      {"valid", all, ALL_FORMS, true, [](A&) {}},
      {"B=0", all, ALL_FORMS, false, [](A& a) { a.B = 0; }},
      {"N=0", all, ALL_FORMS, false, [](A& a) { a.N = 0; }},
      {"S=0", all, ALL_FORMS, false, [](A& a) { a.S = 0; }},
      {"B*S>=2^31", sampled, ALL_FORMS, false,
       [](A& a) { a.B = a.S = 65536; }},
      {"m=0", DRAWS, ALL_FORMS, false, [](A& a) { a.m = 0; }},
      {"m=5", DRAWS, ALL_FORMS, false, [](A& a) { a.m = 5; }},
      {"E=NULL", DRAWS, ALL_FORMS, false, [](A& a) { a.E = nullptr; }},
      {"z0=NULL", sampled, ALL_FORMS, false, [](A& a) { a.z0 = nullptr; }},
      {"U=NULL", sampled, ALL_FORMS, false, [](A& a) { a.U = nullptr; }},
      {"a_std=NULL", sampled, ALL_FORMS, false,
       [](A& a) { a.a_std = nullptr; }},
      {"Jc=NULL", sampled, ALL_FORMS, false, [](A& a) { a.Jc = nullptr; }},
      {"best=NULL", planners, ALL_FORMS, false,
       [](A& a) { a.best = nullptr; }},
      {"lam=NULL", MPPI | trials, ALL_FORMS, false,
       [](A& a) { a.lam = nullptr; }},
      {"J_w=NULL", MPPI, ALL_FORMS, false, [](A& a) { a.J_w = nullptr; }},
      {"Z_out without U_out", planners, ALL_FORMS, false,
       [](A& a) { a.U_out = nullptr; }},
      {"U_out without Z_out", planners, ALL_FORMS, false,
       [](A& a) { a.Z_out = nullptr; }},
      {"U_out==U", planners, ALL_FORMS, false, [](A& a) { a.U_out = a.U; }},
      {"Z_out==z0", planners, ALL_FORMS, false, [](A& a) { a.Z_out = a.z0; }},
      {"no rows, S=257", MPPI, ALL_FORMS, false,
       [](A& a) { a.Z_out = a.U_out = nullptr, a.S = 257; }},
      {"no rows, S=256", planners, ALL_FORMS, true,
       [](A& a) { a.Z_out = a.U_out = nullptr, a.S = 256; }},
      {"smooth=1", sampled, ALL_FORMS, false, [](A& a) { a.smooth = 1.0; }},
      {"smooth<0", sampled, ALL_FORMS, false, [](A& a) { a.smooth = -0.1; }},
      {"smooth=NaN", sampled, ALL_FORMS, false,
       [](A& a) { a.smooth = std::nan(""); }},
      {"table=NULL", planners, BATCH, false, [](A& a) { a.table = nullptr; }},
      {"table=NULL", sampled, ALL_FORMS & ~BATCH, true,
       [](A& a) { a.table = nullptr; }},
      {"ref=NULL", planners, WITH_REF, false, [](A& a) { a.ref = nullptr; }},
      {"ref_len=0", planners | TRIAL_GOALS, WITH_REF, false,
       [](A& a) { a.ref_len = 0; }},
      {"ref_t0<0", planners | TRIAL_GOALS, WITH_REF, false,
       [](A& a) { a.ref_t0 = -1; }},
      {"ref_t0 beyond ref_len", planners | TRIAL_GOALS, WITH_REF, true,
       [](A& a) { a.ref_t0 = 1000; }},
      {"ref_t0=INT_MAX", planners, WITH_REF, true,
       [](A& a) { a.ref_t0 = INT_MAX; }},
      {"weights=NULL", planners, WITH_WEIGHTS, false,
       [](A& a) { a.weights = nullptr; }},
      {"weights=NULL", TRIAL_GOALS, ALL_FORMS, true,
       [](A& a) { a.weights = nullptr; }},
      {"ref=NULL", TRIAL_GOALS, ALL_FORMS, true,
       [](A& a) { a.ref = nullptr; }},
      {"ref=NULL, ref_len=0", TRIAL_GOALS, ALL_FORMS, true,
       [](A& a) { a.ref = nullptr, a.ref_len = 0, a.ref_t0 = -1; }},
      {"ref=weights=NULL", TRIAL_GOALS, ALL_FORMS, false,
       [](A& a) { a.ref = a.weights = nullptr; }},
      {"ref_t0=INT_MAX-TT", TRIAL_GOALS, ALL_FORMS, true,
       [](A& a) { a.ref_t0 = INT_MAX - a.TT; }},
      {"ref_t0=INT_MAX-TT+1", TRIAL_GOALS, ALL_FORMS, false,
       [](A& a) { a.ref_t0 = INT_MAX - a.TT + 1; }},
      {"K=0", trials, ALL_FORMS, false, [](A& a) { a.K = 0; }},
      {"TT=0", trials, ALL_FORMS, false, [](A& a) { a.TT = 0; }},
      {"t0<0", trials, ALL_FORMS, false, [](A& a) { a.t0 = -1; }},
      {"count=0", trials, ALL_FORMS, false, [](A& a) { a.count = 0; }},
      {"t0+count>TT", trials, ALL_FORMS, false,
       [](A& a) { a.t0 = 1, a.count = 3; }},
      {"t0+count overflows", trials, ALL_FORMS, false,
       [](A& a) { a.t0 = INT_MAX, a.count = INT_MAX; }},
      {"Z=NULL", trials, ALL_FORMS, false, [](A& a) { a.Z = nullptr; }},
      {"U_work=NULL", trials, ALL_FORMS, false,
       [](A& a) { a.U_work = nullptr; }},
      {"U_work==U", trials, ALL_FORMS, false, [](A& a) { a.U_work = a.U; }},
      {"Xlog=NULL", trials, ALL_FORMS, false, [](A& a) { a.Xlog = nullptr; }},
      {"Ulog=NULL", trials, ALL_FORMS, false, [](A& a) { a.Ulog = nullptr; }},
      {"Jcl=NULL", trials, ALL_FORMS, false, [](A& a) { a.Jcl = nullptr; }},
      {"v_std without x_true", trials, ALL_FORMS, false,
       [](A& a) { a.v_std = at<T>(30), a.x_true = nullptr; }},
      {"x_true without v_std", trials, ALL_FORMS, true,
       [](A& a) { a.x_true = at<T>(31); }},
      {"step_offset<0", trials, ALL_FORMS, false,
       [](A& a) { a.step_offset = -1; }},
      {"step_offset=INT_MAX-TT", trials, ALL_FORMS, true,
       [](A& a) { a.step_offset = INT_MAX - a.TT; }},
      {"step_offset=INT_MAX-TT+1", trials, ALL_FORMS, false,
       [](A& a) { a.step_offset = INT_MAX - a.TT + 1; }},
  };
}

#define SHOOT_ARGS                                                             \
  a.B, a.N, a.S, a.z0, a.U, a.u_min, a.u_max, a.a_std, a.smooth, 7, 5,         \
      nullptr, a.Jc, a.best, a.J_best, a.Z_out, a.U_out, nullptr
#define MPPI_ARGS                                                              \
  a.B, a.N, a.S, a.z0, a.U, a.u_min, a.u_max, a.a_std, a.lam, a.smooth, 7, 5,  \
      nullptr, a.Jc, a.best, a.J_best, a.W, a.J_w, a.Z_out, a.U_out, nullptr
#define TRIAL_ARGS                                                             \
  a.B, a.N, a.S, a.K, a.TT, a.t0, a.count, a.z0, a.U, a.Z, a.U_work, a.u_min,  \
      a.u_max, a.a_std, a.lam, a.smooth, 7, 5, 210, a.disturbance, a.w_std,    \
      a.v_std, 9, a.step_offset, a.x_true, nullptr, a.Jc, 1, a.Xlog, a.Ulog,   \
      a.Jcl, a.Ylog, nullptr, nullptr, nullptr, nullptr, nullptr
#define REF a.ref, a.ref_len, a.ref_t0

template <typename T>
struct Entry {
  const char* name;
  int family, form;
  std::function<int(const pddp_problem*, const Args<T>&)> call;
};

#define PLANNER_ENTRIES(NAME, FAMILY, SUF, LIST)                               \
  {"pddp_" #NAME "_" #SUF, FAMILY, PLAIN,                                      \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_##SUF(p, LIST);                                      \
   }},                                                                         \
  {"pddp_" #NAME "_batch_" #SUF, FAMILY, BATCH,                                \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_batch_##SUF(p, a.table, LIST);                       \
   }},                                                                         \
  {"pddp_" #NAME "_track_" #SUF, FAMILY, TRACK,                                \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_track_##SUF(p, a.table, REF, LIST);                  \
   }},                                                                         \
  {"pddp_" #NAME "_weighted_" #SUF, FAMILY, WEIGHTED,                          \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_weighted_##SUF(p, a.table, a.weights, LIST);         \
   }},                                                                         \
  {"pddp_" #NAME "_track_weighted_" #SUF, FAMILY, TRACK_WEIGHTED,              \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_track_weighted_##SUF(p, a.table, REF, a.weights,     \
                                               LIST);                          \
   }}

#define ENTRIES(SUF)                                                           \
  {PLANNER_ENTRIES(shoot, SHOOT, SUF, SHOOT_ARGS),                             \
   PLANNER_ENTRIES(mppi, MPPI, SUF, MPPI_ARGS),                                \
   {"pddp_shoot_draws_" #SUF, DRAWS, PLAIN,                                    \
    [](const pddp_problem*, const Args<T>& a) {                                \
      return pddp_shoot_draws_##SUF(a.B, a.N, a.S, a.m, 7, 5, a.E, nullptr);   \
    }},                                                                        \
   {"pddp_mppi_trial_" #SUF, TRIAL, PLAIN,                                     \
    [](const pddp_problem* p, const Args<T>& a) {                              \
      return pddp_mppi_trial_##SUF(p, a.table, a.plant, TRIAL_ARGS);           \
    }},                                                                        \
   {"pddp_mppi_trial_goals_" #SUF, TRIAL_GOALS, TRACK_WEIGHTED,                \
    [](const pddp_problem* p, const Args<T>& a) {                              \
      return pddp_mppi_trial_goals_##SUF(p, a.table, a.plant, REF, a.weights,  \
                                         TRIAL_ARGS);                          \
    }}}

template <typename T>
std::vector<Entry<T>> entries();
template <>
std::vector<Entry<float>> entries<float>() {
  using T = float;
  return ENTRIES(f32);
}
template <>
std::vector<Entry<double>> entries<double>() {
  using T = double;
  return ENTRIES(f64);
}

template <typename T>
int run() {
  pddp_problem good{};
  good.model = PDDP_MODEL_CARTPOLE;
  good.encoding = PDDP_ENC_IGNORE_UNCERTAINTY;
  pddp_problem encoding = good, model = good;
  encoding.encoding = PDDP_ENC_VARIANCE_ONLY;
  model.model = 99;
  const struct {
    const char* name;
    const pddp_problem* p;
  } problems[] = {{"good problem", &good},
                  {"NULL problem", nullptr},
                  {"another encoding", &encoding},
                  {"another model", &model}};
  int calls = 0;
  for (const Entry<T>& e : entries<T>())
    for (const Refusal<T>& r : refusals<T>()) {
      if (!(r.families & e.family) || !(r.forms & e.form)) continue;
      for (const auto& pr : problems) {
        // (what would be launched is not called; the draws take no problem)
        if (r.passes && (pr.p == &good || e.family == DRAWS)) continue;
        if (e.family == DRAWS && pr.p != &good) continue;
        Args<T> a;
        r.set(a);
        std::printf("%-34s %-26s %-17s %d\n", e.name, r.name, pr.name,
                    e.call(pr.p, a));
        ++calls;
      }
    }
  return calls;
}

}  // namespace

int main() {
  const int calls = run<float>() + run<double>();
  std::printf("%d calls\n", calls);
  return 0;
}
