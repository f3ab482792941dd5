// problem_refusals.cpp - the records and the line search in their five forms
// and the nominal rollout in its two (pddp_derivs_*, pddp_line_search_*: plain,
// _batch, _track, _weighted, _track_weighted; pddp_nominal_rollout_*: plain,
// _batch; f32 and f64: 24 entry points) called with argument sets they must
// refuse before any launch, each alone and paired with a problem that
// check_problem refuses (NULL, another encoding, another model), so that the
// order in which the argument test, the form test, the route to the Gaussian
// encodings' kernels and check_problem are reached shows in the code returned.
// Prints one line per call; two builds of the library refuse alike when their
// outputs are the same text.  A stand-alone program for the
// CPU, after tools/sampled_refusals.cpp: nothing here reaches a launch, the
// pointers are addresses nobody reads.  It never makes a call that would pass:
// an argument set the argument test lets through runs only with a problem that
// check_problem refuses, and not with "another encoding" on a plain form, which
// routes that problem to default_kernels.hip and would launch.
//
//   hipcc -std=c++17 -I include tools/problem_refusals.cpp \
//       -L pddp_amd/lib -lpddp_hip -Wl,-rpath,$PWD/pddp_amd/lib -o refusals
//
// Under the sanitizers the host code under test is compiled into the program
// (its definitions then take precedence over the library's; run on the CPU):
//   hipcc -std=c++17 --offload-arch=gfx950 -fPIC -fno-slp-vectorize \
//       -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//       -I include tools/problem_refusals.cpp \
//       pddp_amd/csrc/problem_kernels.hip \
//       -L pddp_amd/lib -lpddp_hip -Wl,-rpath,$PWD/pddp_amd/lib -o refusals
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "pddp_hip.h"

namespace {

enum Op { ROLLOUT = 1, DERIVS = 2, SEARCH = 4 };
enum Form { PLAIN = 1, BATCH = 2, TRACK = 4, WEIGHTED = 8, TRACK_WEIGHTED = 16 };
constexpr int ALL_OPS = 7, ALL_FORMS = 31, WITH_REF = TRACK | TRACK_WEIGHTED,
              WITH_WEIGHTS = WEIGHTED | TRACK_WEIGHTED;

template <typename T>
T* at(uintptr_t k) {  // a distinct address per argument, never read
  return reinterpret_cast<T*>(0x10000 + 0x1000 * k);
}

// every argument of every entry point, valid as set here
template <typename T>
struct Args {
  const T *table = at<T>(1), *ref = at<T>(2), *weights = at<T>(3);
  int ref_len = 4, ref_t0 = 1;
  int B = 3, N = 6, A = 11;
  const T *z0 = at<T>(4), *Z = at<T>(5), *U = at<T>(6), *gains = at<T>(7),
          *alphas = at<T>(8), *u_min = at<T>(9), *u_max = at<T>(10);
  const uint8_t* mask = at<uint8_t>(11);
  const int32_t* bwd_status = at<int32_t>(12);
  T *Z_out = at<T>(13), *rec = at<T>(14), *L = at<T>(15), *J = at<T>(16);
  int32_t* state = at<int32_t>(17);
  T *Zc = at<T>(18), *Uc = at<T>(19), *Jc = at<T>(20);
};

template <typename T>
struct Refusal {
  const char* name;
  int ops, forms;
  bool passes;  // the argument test lets it through: only run with a bad problem
  std::function<void(Args<T>&)> set;
};

template <typename T>
std::vector<Refusal<T>> refusals() {
  using R = Args<T>;
  const int records = DERIVS | SEARCH;
  return {
      {"valid", ALL_OPS, ALL_FORMS, true, [](R&) {}},
      {"B=0", ALL_OPS, ALL_FORMS, false, [](R& a) { a.B = 0; }},
      {"B<0", ALL_OPS, ALL_FORMS, false, [](R& a) { a.B = -1; }},
      {"N=0", ALL_OPS, ALL_FORMS, false, [](R& a) { a.N = 0; }},
      {"N<0", ALL_OPS, ALL_FORMS, false, [](R& a) { a.N = -1; }},
      {"A=0", SEARCH, ALL_FORMS, false, [](R& a) { a.A = 0; }},
      {"A<0", SEARCH, ALL_FORMS, false, [](R& a) { a.A = -1; }},
      {"B*A>=2^31", SEARCH, ALL_FORMS & ~PLAIN, false,
       [](R& a) { a.B = a.A = 65536; }},
      {"B*A>=2^31", SEARCH, PLAIN, true, [](R& a) { a.B = a.A = 65536; }},
      {"B*A=2^31-1", SEARCH, ALL_FORMS, true,
       [](R& a) { a.B = 0x7fffffff, a.A = 1; }},
      {"z0=NULL", ROLLOUT, ALL_FORMS, false, [](R& a) { a.z0 = nullptr; }},
      {"Z=NULL", ALL_OPS, ALL_FORMS, false,
       [](R& a) { a.Z = nullptr, a.Z_out = nullptr; }},
      {"U=NULL", ALL_OPS, ALL_FORMS, false, [](R& a) { a.U = nullptr; }},
      {"rec=NULL", DERIVS, ALL_FORMS, false, [](R& a) { a.rec = nullptr; }},
      {"L=NULL", DERIVS, ALL_FORMS, false, [](R& a) { a.L = nullptr; }},
      {"J=NULL", DERIVS, ALL_FORMS, false, [](R& a) { a.J = nullptr; }},
      {"gains=NULL", SEARCH, ALL_FORMS, false,
       [](R& a) { a.gains = nullptr; }},
      {"alphas=NULL", SEARCH, ALL_FORMS, false,
       [](R& a) { a.alphas = nullptr; }},
      {"Zc=NULL", SEARCH, ALL_FORMS, false, [](R& a) { a.Zc = nullptr; }},
      {"Uc=NULL", SEARCH, ALL_FORMS, false, [](R& a) { a.Uc = nullptr; }},
      {"Jc=NULL", SEARCH, ALL_FORMS, false, [](R& a) { a.Jc = nullptr; }},
      // (nullable everywhere: the bounds, the masks, state, bwd_status)
      {"u_min=u_max=NULL", ALL_OPS, ALL_FORMS, true,
       [](R& a) { a.u_min = a.u_max = nullptr; }},
      {"mask=NULL", ALL_OPS, ALL_FORMS, true, [](R& a) { a.mask = nullptr; }},
      {"state=NULL", DERIVS, ALL_FORMS, true,
       [](R& a) { a.state = nullptr; }},
      {"bwd_status=NULL", SEARCH, ALL_FORMS, true,
       [](R& a) { a.bwd_status = nullptr; }},
      // what a suffix promises
      {"table=NULL", ALL_OPS, BATCH, false, [](R& a) { a.table = nullptr; }},
      {"table=NULL", records, ALL_FORMS & ~BATCH, true,
       [](R& a) { a.table = nullptr; }},
      {"ref=NULL", records, WITH_REF, false, [](R& a) { a.ref = nullptr; }},
      {"ref_len=0", records, WITH_REF, false, [](R& a) { a.ref_len = 0; }},
      {"ref_len<0", records, WITH_REF, false, [](R& a) { a.ref_len = -3; }},
      {"ref_t0=-1", records, WITH_REF, false, [](R& a) { a.ref_t0 = -1; }},
      {"ref_t0 beyond ref_len", records, WITH_REF, true,
       [](R& a) { a.ref_t0 = 1000; }},
      {"ref_t0=INT_MAX", records, WITH_REF, true,
       [](R& a) { a.ref_t0 = 0x7fffffff; }},
      {"weights=NULL", records, WITH_WEIGHTS, false,
       [](R& a) { a.weights = nullptr; }},
      {"ref=weights=NULL", records, TRACK_WEIGHTED, false,
       [](R& a) { a.ref = a.weights = nullptr; }},
      {"B=0, table=NULL", ALL_OPS, BATCH, false,
       [](R& a) { a.B = 0, a.table = nullptr; }},
      {"N=0, ref=NULL", records, WITH_REF, false,
       [](R& a) { a.N = 0, a.ref = nullptr; }},
      {"U=NULL, weights=NULL", records, WITH_WEIGHTS, false,
       [](R& a) { a.U = nullptr, a.weights = nullptr; }},
  };
}

#define ROLLOUT_ARGS \
  a.B, a.N, a.z0, a.U, a.u_min, a.u_max, a.mask, a.Z_out, nullptr
#define DERIVS_ARGS                                                            \
  a.B, a.N, a.Z, a.U, a.u_min, a.u_max, a.mask, a.rec, a.L, a.J, a.state,      \
      nullptr
#define SEARCH_ARGS                                                            \
  a.B, a.N, a.A, a.Z, a.U, a.gains, a.alphas, a.u_min, a.u_max, a.mask,        \
      a.bwd_status, a.Zc, a.Uc, a.Jc, nullptr
#define REF a.ref, a.ref_len, a.ref_t0

template <typename T>
struct Entry {
  const char* name;
  int op, form;
  std::function<int(const pddp_problem*, const Args<T>&)> call;
};

#define PLAIN_AND_BATCH(NAME, OP, SUF, LIST)                                   \
  {"pddp_" #NAME "_" #SUF, OP, PLAIN,                                          \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_##SUF(p, LIST);                                      \
   }},                                                                         \
  {"pddp_" #NAME "_batch_" #SUF, OP, BATCH,                                    \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_batch_##SUF(p, a.table, LIST);                       \
   }}
#define GOAL_FORMS(NAME, OP, SUF, LIST)                                        \
  {"pddp_" #NAME "_track_" #SUF, OP, TRACK,                                    \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_track_##SUF(p, a.table, REF, LIST);                  \
   }},                                                                         \
  {"pddp_" #NAME "_weighted_" #SUF, OP, WEIGHTED,                              \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_weighted_##SUF(p, a.table, a.weights, LIST);         \
   }},                                                                         \
  {"pddp_" #NAME "_track_weighted_" #SUF, OP, TRACK_WEIGHTED,                  \
   [](const pddp_problem* p, const Args<T>& a) {                               \
     return pddp_##NAME##_track_weighted_##SUF(p, a.table, REF, a.weights,     \
                                               LIST);                          \
   }}

#define ENTRIES(SUF)                                                           \
  {PLAIN_AND_BATCH(derivs, DERIVS, SUF, DERIVS_ARGS),                          \
   GOAL_FORMS(derivs, DERIVS, SUF, DERIVS_ARGS),                               \
   PLAIN_AND_BATCH(line_search, SEARCH, SUF, SEARCH_ARGS),                     \
   GOAL_FORMS(line_search, SEARCH, SUF, SEARCH_ARGS),                          \
   PLAIN_AND_BATCH(nominal_rollout, ROLLOUT, SUF, ROLLOUT_ARGS)}

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
      if (!(r.ops & e.op) || !(r.forms & e.form)) continue;
      for (const auto& pr : problems) {
        // (what would be launched is not called: good arguments with the good
        // problem, or on a plain form with a Gaussian encoding)
        if (r.passes &&
            (pr.p == &good || (pr.p == &encoding && e.form == PLAIN)))
          continue;
        Args<T> a;
        r.set(a);
        std::printf("%-36s %-22s %-17s %d\n", e.name, r.name, pr.name,
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
