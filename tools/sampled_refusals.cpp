// sampled_refusals.cpp - every entry point of the sampling planners
// (pddp_shoot_*, pddp_mppi_* and pddp_cem_* in their five forms,
// pddp_shoot_draws_*, pddp_mppi_trial_*, pddp_mppi_trial_goals_*,
// pddp_cem_trial_*; f32 and f64) called with argument sets it must refuse
// before any launch, each alone and paired with a problem
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
//       pddp_amd/csrc/cem.hip pddp_amd/csrc/cem_trial.hip \
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

enum Family {
  SHOOT = 1, MPPI = 2, TRIAL = 4, TRIAL_GOALS = 8, DRAWS = 16, CEM = 32,
  CEM_TRIAL = 64
};
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
  // cem and its trial (K is the elites there, I the trial's iterations)
  int I = 2;
  T* sigma = at<T>(32);
  const T *sigma0 = at<T>(33), *std_min = at<T>(34);
  double mix = 0.25;
  int32_t *rank = at<int32_t>(35), *n_elite = at<int32_t>(36);
  T *J_m = at<T>(37), *S_out = at<T>(38);
  T *mean = at<T>(39), *width = at<T>(40), *Um = at<T>(41), *Sm = at<T>(42);
  const uint8_t* active = nullptr;
  T *Jtrace_log = at<T>(43), *Jm_log = at<T>(44);
  int32_t* nelite_log = at<int32_t>(45);
  T *plan_log = at<T>(46), *std_log = at<T>(47);
};

template <typename T>
struct Refusal {
  std::string name;
  int families, forms;
  bool passes;  // the argument test lets it through: only run with a bad problem
  std::function<void(Args<T>&)> set;
};

template <typename T>
std::vector<Refusal<T>> refusals() {
  using A = Args<T>;
  // (`planners`, `trials`, `sampled`: shoot's and mppi's, whose width is a_std;
  // the rows both families share name cem's next to them)
  const int planners = SHOOT | MPPI, trials = TRIAL | TRIAL_GOALS,
            sampled = planners | trials, cems = CEM | CEM_TRIAL,
            all = sampled | DRAWS | cems;
  std::vector<Refusal<T>> rows = {
      {"valid", all, ALL_FORMS, true, [](A&) {}},
      {"B=0", all, ALL_FORMS, false, [](A& a) { a.B = 0; }},
      {"N=0", all, ALL_FORMS, false, [](A& a) { a.N = 0; }},
      {"S=0", all, ALL_FORMS, false, [](A& a) { a.S = 0; }},
      {"B*S>=2^31", sampled | cems, ALL_FORMS, false,
       [](A& a) { a.B = a.S = 65536; }},
      {"m=0", DRAWS, ALL_FORMS, false, [](A& a) { a.m = 0; }},
      {"m=5", DRAWS, ALL_FORMS, false, [](A& a) { a.m = 5; }},
      {"E=NULL", DRAWS, ALL_FORMS, false, [](A& a) { a.E = nullptr; }},
      {"z0=NULL", sampled | cems, ALL_FORMS, false,
       [](A& a) { a.z0 = nullptr; }},
      {"U=NULL", sampled | cems, ALL_FORMS, false,
       [](A& a) { a.U = nullptr; }},
      {"sigma=NULL", cems, ALL_FORMS, false, [](A& a) { a.sigma = nullptr; }},
      {"sigma0=NULL", CEM_TRIAL, ALL_FORMS, true,
       [](A& a) { a.sigma0 = nullptr; }},
      {"std_min=NULL", cems, ALL_FORMS, true,
       [](A& a) { a.std_min = nullptr; }},
      {"a_std=NULL", sampled, ALL_FORMS, false,
       [](A& a) { a.a_std = nullptr; }},
      {"Jc=NULL", sampled | cems, ALL_FORMS, false,
       [](A& a) { a.Jc = nullptr; }},
      {"best=NULL", planners | CEM, ALL_FORMS, false,
       [](A& a) { a.best = nullptr; }},
      {"n_elite=NULL", CEM, ALL_FORMS, false,
       [](A& a) { a.n_elite = nullptr; }},
      {"J_m=NULL", CEM, ALL_FORMS, false, [](A& a) { a.J_m = nullptr; }},
      {"rank=J_best=NULL", CEM, ALL_FORMS, true,
       [](A& a) { a.rank = nullptr, a.J_best = nullptr; }},
      {"lam=NULL", MPPI | trials, ALL_FORMS, false,
       [](A& a) { a.lam = nullptr; }},
      {"J_w=NULL", MPPI, ALL_FORMS, false, [](A& a) { a.J_w = nullptr; }},
      // (the rows: shoot's and mppi's two, cem's three - all or none)
      {"Z_out without U_out", planners | CEM, ALL_FORMS, false,
       [](A& a) { a.U_out = nullptr; }},
      {"U_out without Z_out", planners | CEM, ALL_FORMS, false,
       [](A& a) { a.Z_out = nullptr; }},
      {"rows without S_out", CEM, ALL_FORMS, false,
       [](A& a) { a.S_out = nullptr; }},
      {"Z_out alone", CEM, ALL_FORMS, false,
       [](A& a) { a.U_out = a.S_out = nullptr; }},
      {"U_out alone", CEM, ALL_FORMS, false,
       [](A& a) { a.Z_out = a.S_out = nullptr; }},
      {"S_out alone", CEM, ALL_FORMS, false,
       [](A& a) { a.Z_out = a.U_out = nullptr; }},
      {"U_out==U", planners | CEM, ALL_FORMS, false,
       [](A& a) { a.U_out = a.U; }},
      {"Z_out==z0", planners | CEM, ALL_FORMS, false,
       [](A& a) { a.Z_out = a.z0; }},
      {"S_out==sigma", CEM, ALL_FORMS, false,
       [](A& a) { a.S_out = a.sigma; }},
      {"no rows, S=257", MPPI | CEM, ALL_FORMS, false,
       [](A& a) { a.Z_out = a.U_out = a.S_out = nullptr, a.S = 257; }},
      {"no rows, S=256", planners | CEM, ALL_FORMS, true,
       [](A& a) { a.Z_out = a.U_out = a.S_out = nullptr, a.S = 256; }},
      {"smooth=1", sampled | cems, ALL_FORMS, false,
       [](A& a) { a.smooth = 1.0; }},
      {"smooth<0", sampled | cems, ALL_FORMS, false,
       [](A& a) { a.smooth = -0.1; }},
      {"smooth=NaN", sampled | cems, ALL_FORMS, false,
       [](A& a) { a.smooth = std::nan(""); }},
      {"mix=1", cems, ALL_FORMS, false, [](A& a) { a.mix = 1.0; }},
      {"mix<0", cems, ALL_FORMS, false, [](A& a) { a.mix = -0.1; }},
      {"mix=NaN", cems, ALL_FORMS, false, [](A& a) { a.mix = std::nan(""); }},
      {"mix=0", cems, ALL_FORMS, true, [](A& a) { a.mix = 0.0; }},
      {"table=NULL", planners | CEM, BATCH, false,
       [](A& a) { a.table = nullptr; }},
      {"table=NULL", sampled | cems, ALL_FORMS & ~BATCH, true,
       [](A& a) { a.table = nullptr; }},
      {"ref=NULL", planners | CEM, WITH_REF, false,
       [](A& a) { a.ref = nullptr; }},
      {"ref_len=0", planners | CEM | TRIAL_GOALS, WITH_REF, false,
       [](A& a) { a.ref_len = 0; }},
      {"ref_t0<0", planners | CEM | TRIAL_GOALS, WITH_REF, false,
       [](A& a) { a.ref_t0 = -1; }},
      {"ref_t0 beyond ref_len", planners | CEM | TRIAL_GOALS, WITH_REF, true,
       [](A& a) { a.ref_t0 = 1000; }},
      {"ref_t0=INT_MAX", planners | CEM, WITH_REF, true,
       [](A& a) { a.ref_t0 = INT_MAX; }},
      {"weights=NULL", planners | CEM, WITH_WEIGHTS, false,
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
      {"K=0", trials | cems, ALL_FORMS, false, [](A& a) { a.K = 0; }},
      {"K=S+1", cems, ALL_FORMS, false, [](A& a) { a.K = a.S + 1; }},
      {"K=S", cems, ALL_FORMS, true, [](A& a) { a.K = a.S; }},
      {"K=1", cems, ALL_FORMS, true, [](A& a) { a.K = 1; }},
      {"I=0", CEM_TRIAL, ALL_FORMS, false, [](A& a) { a.I = 0; }},
      {"TT=0", trials | CEM_TRIAL, ALL_FORMS, false, [](A& a) { a.TT = 0; }},
      {"t0<0", trials | CEM_TRIAL, ALL_FORMS, false, [](A& a) { a.t0 = -1; }},
      {"count=0", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.count = 0; }},
      {"t0+count>TT", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.t0 = 1, a.count = 3; }},
      {"t0+count overflows", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.t0 = INT_MAX, a.count = INT_MAX; }},
      {"Z=NULL", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.Z = nullptr; }},
      {"U_work=NULL", trials, ALL_FORMS, false,
       [](A& a) { a.U_work = nullptr; }},
      {"U_work==U", trials, ALL_FORMS, false, [](A& a) { a.U_work = a.U; }},
      {"Xlog=NULL", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.Xlog = nullptr; }},
      {"Ulog=NULL", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.Ulog = nullptr; }},
      {"Jcl=NULL", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.Jcl = nullptr; }},
      {"v_std without x_true", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.v_std = at<T>(30), a.x_true = nullptr; }},
      {"x_true without v_std", trials | CEM_TRIAL, ALL_FORMS, true,
       [](A& a) { a.x_true = at<T>(31); }},
      {"step_offset<0", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.step_offset = -1; }},
      {"step_offset=INT_MAX-TT", trials | CEM_TRIAL, ALL_FORMS, true,
       [](A& a) { a.step_offset = INT_MAX - a.TT; }},
      {"step_offset=INT_MAX-TT+1", trials | CEM_TRIAL, ALL_FORMS, false,
       [](A& a) { a.step_offset = INT_MAX - a.TT + 1; }},
      {"no logs", CEM_TRIAL, ALL_FORMS, true,
       [](A& a) {
         a.Ylog = a.Jtrace_log = a.Jm_log = a.plan_log = a.std_log = nullptr;
         a.nelite_log = nullptr;
       }},
  };
  // the CEM trial's four work buffers: each there, no two the same, none any
  // other buffer of the call
  struct Work {
    const char* name;
    T* A::*field;
  };
  const Work work[] = {{"mean", &A::mean}, {"width", &A::width},
                       {"Um", &A::Um}, {"Sm", &A::Sm}};
  struct Other {
    const char* name;
    std::function<void(A&, T*)> set;
  };
#define OTHER(FIELD)                                                           \
  {#FIELD, [](A& a, T* w) { a.FIELD = reinterpret_cast<decltype(a.FIELD)>(w); }}
  const Other others[] = {
      OTHER(table), OTHER(plant), OTHER(z0), OTHER(U), OTHER(Z), OTHER(u_min),
      OTHER(u_max), OTHER(sigma), OTHER(sigma0), OTHER(std_min),
      OTHER(disturbance), OTHER(w_std), OTHER(v_std), OTHER(x_true),
      OTHER(active), OTHER(Jc), OTHER(Xlog), OTHER(Ulog), OTHER(Jcl),
      OTHER(Ylog), OTHER(Jtrace_log), OTHER(Jm_log), OTHER(nelite_log),
      OTHER(plan_log), OTHER(std_log)};
#undef OTHER
  for (int i = 0; i < 4; ++i) {
    const Work w = work[i];
    rows.push_back({std::string(w.name) + "=NULL", CEM_TRIAL, ALL_FORMS, false,
                    [w](A& a) { a.*(w.field) = nullptr; }});
    for (int j = 0; j < i; ++j) {
      const Work v = work[j];
      rows.push_back({std::string(w.name) + "==" + v.name, CEM_TRIAL,
                      ALL_FORMS, false,
                      [w, v](A& a) { a.*(w.field) = a.*(v.field); }});
    }
    for (const Other& o : others)
      rows.push_back({std::string(w.name) + "==" + o.name, CEM_TRIAL,
                      ALL_FORMS, false,
                      [w, o](A& a) { o.set(a, a.*(w.field)); }});
  }
  return rows;
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
#define CEM_ARGS                                                               \
  a.B, a.N, a.S, a.K, a.z0, a.U, a.u_min, a.u_max, a.sigma, a.std_min,         \
      a.smooth, a.mix, 7, 5, a.active, a.Jc, a.rank, a.best, a.J_best,         \
      a.n_elite, a.J_m, a.Z_out, a.U_out, a.S_out, nullptr
#define CEM_TRIAL_ARGS                                                         \
  a.B, a.N, a.S, a.K, a.I, a.TT, a.t0, a.count, a.z0, a.U, a.Z, a.mean,        \
      a.width, a.Um, a.Sm, a.u_min, a.u_max, a.sigma, a.sigma0, a.std_min,     \
      a.smooth, a.mix, 7, 5, 210, a.disturbance, a.w_std, a.v_std, 9,          \
      a.step_offset, a.x_true, a.active, a.Jc, 1, a.Xlog, a.Ulog, a.Jcl,       \
      a.Ylog, a.Jtrace_log, a.Jm_log, a.nelite_log, a.plan_log, a.std_log,     \
      nullptr
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
   PLANNER_ENTRIES(cem, CEM, SUF, CEM_ARGS),                                   \
   {"pddp_cem_trial_" #SUF, CEM_TRIAL, PLAIN,                                  \
    [](const pddp_problem* p, const Args<T>& a) {                              \
      return pddp_cem_trial_##SUF(p, a.table, a.plant, CEM_TRIAL_ARGS);        \
    }},                                                                        \
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
        std::printf("%-34s %-26s %-17s %d\n", e.name, r.name.c_str(), pr.name,
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
