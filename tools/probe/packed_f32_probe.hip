// What does a packed f32 instruction cost ONE wavefront that has its SIMD to
// itself, with no matrix instruction beside it?  (The round kernel's rollouts:
// one wavefront per SIMD at 256 workgroups of four, a VALU-only dependent
// chain - DESIGN.md 3.5b.)  Each operation as a DEPENDENT chain (every
// instruction reads the one before) and as an INDEPENDENT stream (eight
// accumulators round-robin), against v_fma_f32 in both forms, plus the
// double-precision operations of the rollouts' sine / cosine range reduction.
// hipcc --offload-arch=gfx950 -O2 tools/probe/packed_f32_probe.hip -o /tmp/pkp && /tmp/pkp
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#define REP4(x) x x x x
#define REP8(x) REP4(x) REP4(x)

// 64 instructions per asm block on fixed registers: the accumulators are the
// pairs v[40:41] .. v[54:55], the constant is v[56:57] (loaded before the
// timed loop).  DEP: every instruction reads the one before (pair 0 only);
// otherwise eight independent accumulators round-robin.
#define CLOB                                                                 \
  "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49",       \
      "v50", "v51", "v52", "v53", "v54", "v55"

enum { kPkFma, kPkMul, kPkAdd, kFma32, kFma64, kRnd64, kCvt64, kOps };
static const char* kName[kOps] = {"v_pk_fma_f32", "v_pk_mul_f32",
                                  "v_pk_add_f32", "v_fma_f32",
                                  "v_fma_f64",    "v_rndne_f64",
                                  "v_cvt_f64_f32"};

// one instruction on accumulator R (R, the register number as a string):
// the destination, then the rest of the operand list
#define PKFMA_(R) "v_pk_fma_f32 v[" R ":" R "+1], v[" R ":" R "+1], v[56:57], v[56:57]\n\t"
#define PKMUL_(R) "v_pk_mul_f32 v[" R ":" R "+1], v[" R ":" R "+1], v[56:57]\n\t"
#define PKADD_(R) "v_pk_add_f32 v[" R ":" R "+1], v[" R ":" R "+1], v[56:57]\n\t"
#define FMA32_(R) "v_fma_f32 v" R ", v" R ", v56, v56\n\t"
#define FMA64_(R) "v_fma_f64 v[" R ":" R "+1], v[" R ":" R "+1], v[56:57], v[56:57]\n\t"
#define RND64_(R) "v_rndne_f64 v[" R ":" R "+1], v[" R ":" R "+1]\n\t"
// (dependent: the low word of the previous result; independent: the constant)
#define CVTD_(R) "v_cvt_f64_f32 v[" R ":" R "+1], v" R "\n\t"
#define CVTI_(R) "v_cvt_f64_f32 v[" R ":" R "+1], v56\n\t"
#define ALL8(M) M("40") M("42") M("44") M("46") M("48") M("50") M("52") M("54")

template <int OP, bool DEP>
__device__ __forceinline__ void body() {
#define GO(M, MI)                                                            \
  do {                                                                       \
    if constexpr (DEP) asm volatile(REP8(REP8(M("40"))) ::: CLOB);           \
    else asm volatile(REP8(ALL8(MI)) ::: CLOB);                              \
  } while (0)
  if constexpr (OP == kPkFma) GO(PKFMA_, PKFMA_);
  if constexpr (OP == kPkMul) GO(PKMUL_, PKMUL_);
  if constexpr (OP == kPkAdd) GO(PKADD_, PKADD_);
  if constexpr (OP == kFma32) GO(FMA32_, FMA32_);
  if constexpr (OP == kFma64) GO(FMA64_, FMA64_);
  if constexpr (OP == kRnd64) GO(RND64_, RND64_);
  if constexpr (OP == kCvt64) GO(CVTD_, CVTI_);
#undef GO
}

template <int OP, bool DEP>
__global__ __launch_bounds__(256) void probe(double* out, long long* cyc,
                                             int iters, double c) {
  const double x = 1.0 + threadIdx.x * 1e-3;
  asm volatile(
      "v_mov_b64 v[56:57], %0\n\tv_mov_b64 v[40:41], %1\n\t"
      "v_mov_b64 v[42:43], %1\n\tv_mov_b64 v[44:45], %1\n\t"
      "v_mov_b64 v[46:47], %1\n\tv_mov_b64 v[48:49], %1\n\t"
      "v_mov_b64 v[50:51], %1\n\tv_mov_b64 v[52:53], %1\n\t"
      "v_mov_b64 v[54:55], %1" ::"v"(c), "v"(x) : CLOB, "v56", "v57");
  body<OP, DEP>();
  __syncthreads();
  const long long t0 = clock64();
  for (int i = 0; i < iters; ++i) body<OP, DEP>();
  const long long t1 = clock64();
  double s;
  asm volatile("v_mov_b64 %0, v[40:41]" : "=v"(s));
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if ((threadIdx.x & 63) == 0)
    cyc[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = t1 - t0;
}

template <int OP, bool DEP>
static double run() {
  // 256 workgroups of four wavefronts: one wavefront per SIMD, every CU busy
  const int threads = 256, blocks = 256, iters = 400;
  double* out;
  long long* cyc;
  hipMalloc(&out, sizeof(double) * threads * blocks);
  hipMalloc(&cyc, sizeof(long long) * blocks * threads / 64);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  probe<OP, DEP><<<blocks, threads>>>(out, cyc, iters, 0.999);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  probe<OP, DEP><<<blocks, threads>>>(out, cyc, iters, 0.999);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  std::vector<long long> h(blocks * threads / 64);
  hipMemcpy(h.data(), cyc, sizeof(long long) * h.size(),
            hipMemcpyDeviceToHost);
  double mean = 0;
  for (auto v : h) mean += v;
  mean /= h.size();
  const double n_instr = 64.0 * iters;
  // clock64 = s_memtime: the shader clock; events give the wall time
  printf("%-14s %-11s : %6.2f clk/instr  (%.3f ns/instr by events)\n",
         kName[OP], DEP ? "dependent" : "independent", mean / n_instr,
         ms * 1e6 / n_instr);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  hipFree(out);
  hipFree(cyc);
  return mean / n_instr;
}

template <int OP>
static void both() {
  run<OP, true>();
  run<OP, false>();
}

int main() {
  both<kFma32>();
  both<kPkFma>();
  both<kPkMul>();
  both<kPkAdd>();
  both<kFma64>();
  both<kRnd64>();
  both<kCvt64>();
  both<kFma32>();  // (again at the end: the clock's drift over the run)
  return 0;
}
