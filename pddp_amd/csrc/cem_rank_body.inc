// cem_rank_body.inc - CEM's pass 2, the text of cem_kernel, cem_goals_kernel
// (cem_kernel_body.inc) and cem_trial_kernel (cem_trial_kernel_body.inc): the
// ranks.  A lane's candidates against all S of its trajectory, a chunk of G at
// a time through LDS: every lane stages the cost it wrote itself in pass 1
// (+inf where it is not finite, or there is no candidate), so no lane reads
// another lane's global store.  The loops and their barriers are
// launch-uniform: lanes outside the batch or masked stage +inf and count
// nothing.  `take_lower`'s order: (J, s) lexicographically.  Exact integer
// work.
//
// The including kernel has `live`, `lane`, `group`, `tid`, `G`, `S`, `turns`,
// `span`, `multi`, `inf`, the __shared__ words `stage`, `cut_J`, `cut_s`,
// `part_fin`, and defines
//   PDDP_CEM_COST(s)       the cost of candidate s of trajectory b, where pass 1
//                          stored it (cem_refit_body.inc reads it too)
//   PDDP_CEM_KEEP(point)   what pddp_cem_* keeps of the ranking and the trial
//                          does not (empty there): RANKED, per candidate with
//                          its `s`, `mine`, `fin`, `Js`, `below` - rank, best,
//                          J_best; CUT, per trajectory behind the pass -
//                          n_elite, and without a finite cost best, J_best,
//                          J_m; INDEX, first in a candidate's turn - a hook
//                          for statement order alone (cem_kernel_body.inc)
// It leaves `n_fin`, `Ke` (the elites: min(K, finite costs)), `ok`, `owner`
// (ONE lane per trajectory) and the cut `Jcut`, `scut`: the elite of the
// highest rank, (J, s).  cut_J / cut_s are written behind the barriers of this
// pass and read behind the one that closes it, under `ok` alone: a pass
// without a finite cost writes no cut and reads none, whatever an earlier one
// left there.
  // the finite costs of the trajectory: a lane's own, then the group
  int fin_[1] = {0};
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    if (live && s < S) fin_[0] += is_finite(PDDP_CEM_COST(s)) ? 1 : 0;
  }
  group_sum(fin_, span, multi, part_fin);
  const int n_fin = fin_[0];
  const int Ke = a.K < n_fin ? a.K : n_fin;
  for (int turn = 0; turn < turns; ++turn) {
    const int s = lane + turn * G;
    PDDP_CEM_KEEP(INDEX)
    const bool mine = live && s < S;
    const T Js = mine ? PDDP_CEM_COST(s) : inf;
    const bool fin = mine && is_finite(Js);
    int below = 0;
    for (int ch = 0; ch < turns; ++ch) {
      const int sc = lane + ch * G;
      T v = inf;
      if (live && sc < S) {
        v = PDDP_CEM_COST(sc);
        v = is_finite(v) ? v : inf;
      }
      __syncthreads();  // (the chunk before has been read)
      stage[tid] = v;
      __syncthreads();
      // s' = ch G + q against s = turn G + lane: every s' of an earlier chunk
      // is below s and every s' of a later one above, so only the lane's own
      // chunk needs the index (ch and turn are launch-uniform)
      // (unrolled: the LDS reads of eight costs are in flight together)
      const T* chunk = stage + group * G;
      if (ch < turn) {
#pragma unroll 8
        for (int q = 0; q < G; ++q) below += chunk[q] <= Js ? 1 : 0;
      } else if (ch > turn) {
#pragma unroll 8
        for (int q = 0; q < G; ++q) below += chunk[q] < Js ? 1 : 0;
      } else {
#pragma unroll 8
        for (int q = 0; q < G; ++q) {
          const T o = chunk[q];
          below += (o < Js || (o == Js && q < lane)) ? 1 : 0;
        }
      }
    }
    // the finite costs' ranks are 0 .. n_fin - 1, each once
    PDDP_CEM_KEEP(RANKED)
    if (fin && below == Ke - 1) {
      cut_J[group] = Js;
      cut_s[group] = s;
    }
  }
  __syncthreads();
  const bool ok = live && n_fin > 0;
  const bool owner = ok && lane == 0;  // ONE lane per trajectory
  const T Jcut = ok ? cut_J[group] : -inf;
  const int scut = ok ? cut_s[group] : -1;
  PDDP_CEM_KEEP(CUT)
