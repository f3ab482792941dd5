// round_n4_body.hpp - the body of the one-launch round (round_n4.hip) as a
// device function, so that the kernels of the other gain branches
// (cartpole_branches.hip, BR of riccati_n4_elem.hpp) run the same text.
#pragma once

#include "riccati_n4_elem.hpp"
#include "line_search_lds.hpp"

namespace pddp {

template <unsigned QM, bool MULTI, int BR>
PDDP_DEV void round_n4_body(const RiccatiArgs<float>& a,
                            const n4d::GenArgs<float>& gen,
                            const ProblemT<float>& prob,
                            const LineSearchArgs<float>& ls,
                            const AcceptArgs<float>& ac, float* scratch,
                            int rounds, long long* phase_ticks, int use_carry) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // (bench.py's roofline leg: what share of the launch is sweep - rocprofv3
  // sees one kernel.  Wavefront 0 of the workgroup reads the chip's 100 MHz
  // clock around its phases and adds the differences up; NULL: nothing)
  const bool timed = phase_ticks != nullptr && threadIdx.x == 0;
  long long t_sweep = 0, t_search = 0;
  // `rounds` attempts of every trajectory, back to back: trajectories are
  // independent (ilqr.py:298-314 is a loop over ONE trajectory's attempts), a
  // workgroup owns its sixteen for the whole launch, and everything a round
  // hands to the next - nominal, regularisation state, masks, costs - was
  // written by this workgroup: a workgroup-scope fence and a barrier, no
  // launch boundary.  (A trajectory that has left the fit is skipped, as by
  // the next launch.)
  for (int r = 0;; ++r) {
    // (a zero the compiler cannot see through, added to the horizon: address
    // arithmetic and everything else that depends on it stays INSIDE the
    // round - hoisted out of this loop, both phases' invariants live across
    // both phases: 255 VGPRs and 53 spilled against 102)
    int z = 0;
    unsigned tid = threadIdx.x;
    if constexpr (MULTI) {
      asm volatile("s_mov_b32 %0, 0" : "=s"(z));
      asm volatile("" : "+v"(tid));  // (likewise: what the lane id feeds)
    }
    RiccatiArgs<float> a_r = a;
    a_r.N += z;
    LineSearchArgs<float> ls_r = ls;
    ls_r.N += z;
    AcceptArgs<float> ac_r = ac;
    ac_r.N += z;
    n4e::RoundOut ro;
    const long long t0 = timed ? wall_clock64() : 0;
    // (a pair without a live trajectory leaves here, both wavefronts alike -
    // it has none in any later round either; s_barrier does not wait for
    // wavefronts that have ended)
    // (several rounds per launch: the nominal's last rows ride in LDS)
    const int carry = MULTI && use_carry ? (r == 0 ? 1 : 0) : -1;
    if (!n4e::elem_sweep_body<float, QM, true, true, BR>(a_r, gen, prob,
                                                         smem_raw, ro, tid, carry))
      break;
    const long long t1 = timed ? wall_clock64() : 0;
    const PreStaged<float> pre{ro.Zs, ro.Us,      ro.Gs,
                               ro.status, ro.J_opt, ro.carry_rows};
    line_search_lds_body<float, PDDP_MODEL_CARTPOLE, true, n4e::kWaves, 2, QM,
                         false, true>(prob, ls_r, ac_r, scratch, nullptr,
                                      smem_raw, pre, tid);
    if (timed) {
      t_sweep += t1 - t0;
      t_search += wall_clock64() - t1;
    }
    if (!MULTI || r + 1 >= rounds) break;
    // the round's writes (global: nominal, mu, delta, J_opt, masks; LDS: read
    // to the end by the tail) before the next round's reads and LDS writes
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();
  }
  if (timed) {
    phase_ticks[2 * blockIdx.x] += t_sweep;
    phase_ticks[2 * blockIdx.x + 1] += t_search;
  }
}

// cartpole_branches.hip: every gain branch but n4e::kBrEigBox
int launch_round_n4_branches(const pddp_problem& p, const N4NominalPlan& pl,
                             const RiccatiArgs<float>& a,
                             const n4d::GenArgs<float>& gen,
                             const LineSearchArgs<float>& ls,
                             const AcceptArgs<float>& ac, float* scratch,
                             int rounds, long long* phase_ticks,
                             hipStream_t st);

}  // namespace pddp
