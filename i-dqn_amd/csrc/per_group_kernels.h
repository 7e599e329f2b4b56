// Prioritized seed groups: the two sampler ends of a prioritized learner step for S trees in ONE launch each
// (idqn_group_per_learn_on_replay_fc; include/idqn_hip.h).  Between them runs k_fc_group_step (fc_group_kernels.h) unchanged, on a
// table whose records carry the members' weights and |TD| pointers and whose slots are the members' leaves.
//   k_per_group_draw        grid (S): the draw phase on record g       (uniforms -> leaves == replay slots, clamped -> weights)
//   k_per_group_write_back  grid (S): the write-back phase on record g (|TD| -> priorities -> running maximum -> the tree)
// The phases are the solo kernels' (per_phases.h), so a member's leaves, weights, priorities, maximum and tree are the solo
// launches' bytes.  Every output byte has one writer (the entry refuses a buffer named by two members); no communication between
// workgroups; plain loads and vector stores.  A record is what the solo launches of member g receive as their kernel argument.
#pragma once
#include "per_group_args.h"
#include "per_phases.h"

#define PER_GROUP_DRAW_T 1024

// ONE WORKGROUP PER MEMBER, no arrival counter: n <= 32 descents on 16 waves (wave w runs descents w and w + 16), the leaves meet
// in LDS behind one barrier, and the maximum is the fold over 32 slots.  No device-scope fence or atomic: nothing leaves the
// workgroup before the kernel ends.
__global__ __launch_bounds__(PER_GROUP_DRAW_T) void k_per_group_draw(const PerSampler* __restrict__ tab, int n) {
    __shared__ int32_t lf[PER_GROUP_MAX_N];
    const PerSampler s = tab[blockIdx.x];
    const double* __restrict__ const nodes = s.nodes;
    per_draw_stage_descents(nodes, s, n, threadIdx.x >> 6, PER_GROUP_DRAW_T / 64, [&](int i, int32_t leaf) { lf[i] = s.leaves[i] = leaf; });
    __syncthreads();
    per_draw_stage_weights<PER_GROUP_MAX_N>(nodes, s, n, [&](int i) { return lf[i]; });
}

__global__ __launch_bounds__(ST_THREADS) void k_per_group_write_back(const PerSampler* __restrict__ tab, int n, int m) {
    per_write_back_phase(tab[blockIdx.x], n, m);
}
