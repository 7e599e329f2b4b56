// Prioritized seed groups: the two sampler ends of a prioritized learner step for S trees in ONE launch each
// (idqn_group_per_learn_on_replay_fc; include/idqn_hip.h), and the turn between two consecutive steps of S trees in ONE launch
// (idqn_group_per_learn_steps_on_replay_fc).  Between them runs k_fc_group_step (fc_group_kernels.h) unchanged, on a
// table whose records carry the members' weights and |TD| pointers and whose slots are the members' leaves.
//   k_per_group_draw        grid (S): the draw phase on record g       (uniforms -> leaves == replay slots, clamped -> weights)
//   k_per_group_write_back  grid (S): the write-back phase on record g (|TD| -> priorities -> running maximum -> the tree)
//   k_per_group_turn        grid (S): the write-back phase on step i's record g, then the draw phase on step i + 1's record g
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

// The turn between steps i and i + 1 of every member: k_per_group_write_back on step i's records followed by k_per_group_draw on
// step i + 1's, which are adjacent launches of S workgroups each where workgroup g of the second reads the tree workgroup g of
// the first leaves and nothing else -- so ONE workgroup of ST_THREADS threads (16 waves) per member does both, as k_per_turn
// (per_turn_kernels.h) does for a member alone: the phases of per_phases.h, hence the two launches' bytes.  Descent j on wave
// j % 16 (n <= 32: two rounds), the leaves meet in LDS as in k_per_group_draw.  No arrival counter, no spin and nothing between
// workgroups: member g's buffers belong to workgroup g (the entry refuses a buffer named by two members).
// THE HAZARD BETWEEN THE PHASES, as in k_per_turn: the descents load nodes that OTHER waves of this workgroup stored in the
// write-back.  One workgroup runs on one CU (the build does not split workgroups over CUs), so every store and every load goes
// through that CU's one vector L1, which is write-through: a store leaves it for L2 and a later load of the same CU never finds
// an older copy of the line there.  What remains is ORDER, and that is per_turn_fence (per_phases.h); no agent-scope fence: no
// other CU takes part.  For the fence to be enough nothing may stay in a register or on the scalar path across it, so after the
// write-back the tree is read through `nodes`, the PLAIN pointer out of the record: no const, no __restrict__, no alias that
// carries either (k_per_group_draw's alias would tell the compiler that nobody stores to the tree during the kernel).  The root
// is read through the same pointer after stores to it in this kernel, so it stays on the vector path too.  The tables are
// const __restrict__: nothing writes them during the launch.
__global__ __launch_bounds__(ST_THREADS) void k_per_group_turn(const PerSampler* __restrict__ tab, const PerSampler* __restrict__ next_tab, int n,
                                                               int m) {
    __shared__ int32_t lf[PER_GROUP_MAX_N];
    const PerSampler s = tab[blockIdx.x];
    const PerSampler next = next_tab[blockIdx.x];  // (the same tree and settings; step i + 1's uniforms, leaves and weights)
    per_write_back_phase(s, n, m);
    per_turn_fence();
    double* nodes = s.nodes;
    per_draw_stage_descents(nodes, next, n, threadIdx.x >> 6, ST_THREADS / 64, [&](int i, int32_t leaf) { lf[i] = next.leaves[i] = leaf; });
    per_turn_fence();  // the leaves were put into LDS by lane 0 of other waves of this workgroup: the same order argument
    per_draw_stage_weights<PER_GROUP_MAX_N>(nodes, next, n, [&](int i) { return lf[i]; });
}
