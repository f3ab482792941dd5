// closed_loop_args.hpp - what the three rollout kernels of closed_loop.hip
// share besides the kernel text (closed_loop_body.inc): the argument block with
// its test, the cost statistics and the launch geometry.
#pragma once

#include <limits>
#include "pddp_common.hpp"

namespace pddp {

// Mapping: one lane per rollout, s fastest.  A trajectory owns G consecutive
// lanes, the launch's lane group:
//   S <= 64   G = S rounded up to a power of two, workgroups of one wavefront
//             holding 64 / G trajectories; lanes s >= S of a group idle;
//   S > 64    G = the workgroup = S rounded up to whole wavefronts, at most
//             four: one trajectory per workgroup, lane l runs the rollouts
//             s = l, l + G, ... one after the other.
// A group starts at a multiple of G in its wavefront (which multiple depends
// on b where G < 64), and the reduction's butterfly is relative to that
// aligned start; which rollouts a lane runs and in which order the costs meet
// depend on S alone, never on b: a controller's outputs are the same bits
// wherever it is in the batch.
constexpr int kClosedLoopThreads = 4 * kWave;

template <typename T>
struct ClosedLoopArgs {
  int B, N, S, G;
  const T* z0s;    // [B][S][n] or NULL: Z[b][0]
  const T* plant;  // [B][S][PDDP_BATCH_ROW] or NULL: the shared problem
  const T* u_min;
  const T* u_max;
  const uint8_t* active;
  T* Xc;  // [B][N+1][S][n], with Uc [B][N][S][m]: both or neither
  T* Uc;
  T* Jc;     // [B][S]
  T* stats;  // [B][4] or NULL
};

// Host side of every entry point that takes the block: the argument test, with
// the nominal (Z, U) the launch carries beside it.
template <typename T>
inline bool args_ok(const ClosedLoopArgs<T>& a, const T* Z, const T* U) {
  return !(a.B <= 0 || a.N <= 0 || a.S <= 0 || !Z || !U || !a.Jc ||
           (a.Xc == nullptr) != (a.Uc == nullptr));
}

// The statistics of the finite costs a lane (then a lane group) has seen.
template <typename T>
struct CostStats {
  T sum, lo, hi;
  int count;
};
template <typename T>
PDDP_DEV void merge(CostStats<T>& a, T sum, T lo, T hi, int count) {
  a.sum += sum;
  a.lo = lo < a.lo ? lo : a.lo;
  a.hi = hi > a.hi ? hi : a.hi;
  a.count += count;
}

// The lane group and the grid of a launch with S rollouts per trajectory (the
// mapping above): sets a.G, returns the workgroup's threads.
template <typename T>
inline int closed_loop_geometry(ClosedLoopArgs<T>& a, dim3& blocks) {
  int threads = kWave;
  if (a.S <= kWave) {
    a.G = 1;
    while (a.G < a.S) a.G <<= 1;
  } else {
    const int waves = (a.S + kWave - 1) / kWave;
    threads = kWave * (waves < 4 ? waves : 4);
    a.G = threads;
  }
  const int per_block = threads / a.G;
  blocks = dim3((unsigned)(((long long)a.B + per_block - 1) / per_block));
  return threads;
}

}  // namespace pddp
