// sampled_argmin.inc - the argmin of a trajectory's candidates, in the one
// order all six kernels of the sampling planners use (DESIGN.md 3.4m): the
// lane's own in s order (the including kernel's loop), a butterfly over the
// group's lanes of a wavefront (both partners of a pair choose the same of the
// two), then the workgroup's wavefronts in their order through LDS, read by
// every lane.  Idle lanes hold (+inf, -1).  No atomics.  The including kernel
// has `Jmin`, `smin`, `span`, `tid` and the LDS words `part_J`,
// `part_s` [kClosedLoopThreads / kWave].  An included text, as
// sampled_rollout_body.inc.
      for (int off = 1; off < span; off <<= 1)
        take_lower(Jmin, smin, __shfl_xor(Jmin, off), __shfl_xor(smin, off));
      if (blockDim.x > kWave) {  // one trajectory over several wavefronts
        if (tid % kWave == 0) {
          part_J[tid / kWave] = Jmin;
          part_s[tid / kWave] = smin;
        }
        __syncthreads();
        Jmin = part_J[0];
        smin = part_s[0];
        for (int w = 1; w < (int)blockDim.x / kWave; ++w)
          take_lower(Jmin, smin, part_J[w], part_s[w]);
      }
