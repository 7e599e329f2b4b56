// Prioritized-replay EXTENSION, the two ends of a learner step as one launch each (include/idqn_hip.h: per_draw, per_write_back):
//   k_per_draw        = k_per_sample + k_per_weights      (the draw phase of per_phases.h)
//   k_per_write_back  = k_per_priorities + k_sumtree_set  (its write-back phase)
// Their outputs are the separate launches' outputs byte for byte.  n <= PER_STEP_MAX_N (per_step_args.h).
#pragma once
#include "per_phases.h"

// One wave per descent, four to a workgroup, cdiv(n, 4) workgroups -- the shape of k_per_sample, so the descents of a
// 256-sample batch run side by side (the stride of the whole grid: one descent per wave).  The last workgroup to arrive
// (device-scope counter `arrivals`, zero between launches; the fences order the leaf stores before the arrival and the arrival
// before the reads) computes the n weights from the leaves the other workgroups stored: agent-scope loads.
__global__ __launch_bounds__(PER_STEP_MAX_N) void k_per_draw(const PerSampler s, int n, unsigned* arrivals) {
    __shared__ int is_last;
    const double* __restrict__ const nodes = s.nodes;
    const int t = threadIdx.x;
    per_draw_stage_descents(nodes, s, n, blockIdx.x * 4 + (t >> 6), gridDim.x * 4, [&](int i, int32_t leaf) { s.leaves[i] = leaf; });
    __threadfence();
    __syncthreads();
    if (t == 0) is_last = atomicAdd(arrivals, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    if (t == 0) *arrivals = 0u;  // (nobody else reads it before the next launch)
    per_draw_stage_weights<PER_STEP_MAX_N>(nodes, s, n, [&](int i) { return __hip_atomic_load(&s.leaves[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
}

__global__ __launch_bounds__(ST_THREADS) void k_per_write_back(const PerSampler s, int n, int m) { per_write_back_phase(s, n, m); }
