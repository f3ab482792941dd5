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
  // Several rounds per launch: what a trajectory carries from round to round
  // (accept.hpp RoundState) is kept in LDS as well, one record per trajectory.
  // Filled here from global memory, by BOTH wavefronts of a pair - the same
  // words to the same place, each reads back its own: no barrier - and from
  // then on every reader of a round (the sweep's entry, finish_costs, the
  // search's mask and state machine) asks LDS.  A global load at the start
  // of a round is queued behind the stores of the last round's tail: on
  // gfx950 loads and stores return through one in-order counter, and waiting
  // for `active` was waiting for the whole nominal to be acknowledged by L2.
  // (The action's bounds and the step sizes, launch constants that the
  // generator and the search load every round, go the same way for the same
  // reason - every wavefront writes all of them and reads its own.)
  [[maybe_unused]] RoundState* rs_wg = nullptr;
  [[maybe_unused]] const float* ub = nullptr;
  [[maybe_unused]] const float* alphas_l = nullptr;
  constexpr bool kBounds = MULTI && n4e::br_bounded(BR);
  if constexpr (kBounds) {
    __shared__ float sh_ub[2];
    const float lo = a.u_min[0], hi = a.u_max[0];
    sh_ub[0] = lo;
    sh_ub[1] = hi;
    ub = sh_ub;
  }
  if constexpr (MULTI) {
    __shared__ RoundState sh_rs[n4e::kWaves * n4e::kTrajW];
    __shared__ float sh_alpha[kMaxAlphas];
    rs_wg = sh_rs;
    alphas_l = sh_alpha;
    {
      const int ai = threadIdx.x & (kMaxAlphas - 1);
      sh_alpha[ai] = ls.alphas[ai < ls.A ? ai : ls.A - 1];
    }
    const int pair = (threadIdx.x >> 6) & (n4e::kWaves - 1);
    const int row = (threadIdx.x & (kWave - 1)) >> 4;
    const int b = (blockIdx.x * n4e::kWaves + pair) * n4e::kTrajW + row;
    const int bc = b < ac.B ? b : ac.B - 1;
    RoundState st;
    st.mu = ac.mu[bc];
    st.delta = ac.delta[bc];
    st.J_opt = ac.J_opt[bc];
    st.iter = ac.iter[bc];
    st.active = ac.active[bc];
    st.fresh = ac.fresh[bc];
    RoundState* rs = sh_rs + pair * n4e::kTrajW + row;
    rs->mu = st.mu;
    rs->delta = st.delta;
    rs->J_opt = st.J_opt;
    rs->iter = st.iter;
    rs->active = st.active;
    rs->fresh = st.fresh;
  }
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
    if constexpr (MULTI) ls_r.alphas = alphas_l;
    if constexpr (kBounds) {
      a_r.u_min = ls_r.u_min = ub;
      a_r.u_max = ls_r.u_max = ub + 1;
    }
    n4e::RoundOut ro;
    const long long t0 = timed ? wall_clock64() : 0;
    // (a pair without a live trajectory leaves here, both wavefronts alike -
    // it has none in any later round either; s_barrier does not wait for
    // wavefronts that have ended)
    // (several rounds per launch: the nominal's last rows ride in LDS)
    const int carry = MULTI && use_carry ? (r == 0 ? 1 : 0) : -1;
    if (!n4e::elem_sweep_body<float, QM, true, true, BR, MULTI>(
            a_r, gen, prob, smem_raw, ro, tid, carry, rs_wg))
      break;
    const long long t1 = timed ? wall_clock64() : 0;
    const PreStaged<float> pre{ro.Zs, ro.Us,      ro.Gs,
                               ro.status, ro.J_opt, ro.carry_rows};
    line_search_lds_body<float, PDDP_MODEL_CARTPOLE, true, n4e::kWaves, 2, QM,
                         false, true, MULTI>(prob, ls_r, ac_r, scratch,
                                             nullptr, smem_raw, pre, tid,
                                             rs_wg);
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
