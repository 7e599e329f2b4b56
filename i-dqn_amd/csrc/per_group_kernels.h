// Prioritized seed groups: the two sampler ends of a prioritized learner step for S trees in ONE launch each
// (idqn_group_per_learn_on_replay_fc; include/idqn_hip.h).  Between them runs k_fc_group_step (fc_group_kernels.h) unchanged, on a
// table whose records carry the members' weights and |TD| pointers and whose slots are the members' leaves.
//   k_per_group_draw        grid (S): k_per_draw's work on record g      (uniforms -> leaves == replay slots, clamped -> weights)
//   k_per_group_write_back  grid (S): k_per_write_back's body on record g (|TD| -> priorities -> running maximum -> the tree)
// Both call the device functions of sumtree_device.h the solo kernels call, in the same order per element, so a member's
// leaves, weights, priorities, maximum and tree are the solo launches' bytes.  Every output byte has one writer (the entry
// refuses a buffer named by two members); no communication between workgroups; plain loads and vector stores.
#pragma once
#include "per_group_args.h"
#include "sumtree_device.h"

struct PerGroupMember {  // what the solo launches of member g receive as kernel arguments (n and m are the call's)
    double* nodes;
    const double* uniforms;  // [n], in the uploaded block
    int32_t* leaves;
    float* weights;
    const float* td_abs;
    double *priorities, *max_dev, *scratch;
    double n_items, beta, eps, alpha;
    int depth, stratified, reduce_max, K;
};

#define PER_GROUP_DRAW_T 1024

// ONE WORKGROUP PER MEMBER, no arrival counter: n <= 32 descents on 16 waves (wave w runs descents w and w + 16, a
// wave-uniform loop: wave_descend shuffles over all 64 lanes), the leaves meet in LDS behind one barrier, then thread t < n
// owns sample t as in k_per_draw's last workgroup.  The maximum: every thread folds the 32 raw weights with fmax in index
// order.  fmax of finite non-negative values (per_raw_weight never yields a NaN: its power has a positive base) is exact
// and does not depend on grouping or order, and the pad entries are k_per_draw's 0.0, so it is the maximum k_per_draw's tree
// reduction and k_per_weights find.  No device-scope fence or atomic: nothing leaves the workgroup before the kernel ends.
__global__ __launch_bounds__(PER_GROUP_DRAW_T) void k_per_group_draw(const PerGroupMember* __restrict__ tab, int n) {
    __shared__ int32_t lf[PER_GROUP_MAX_N];
    __shared__ double raw[PER_GROUP_MAX_N];
    const PerGroupMember& mb = tab[blockIdx.x];
    const double* __restrict__ const nodes = mb.nodes;
    const double* __restrict__ const uniforms = mb.uniforms;
    const int depth = mb.depth, stratified = mb.stratified;
    const double n_items = mb.n_items, beta = mb.beta;
    const int t = threadIdx.x;
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    for (int i = t >> 6; i < n; i += PER_GROUP_DRAW_T / 64) {  // wave-uniform
        const unsigned int node = per_sample_node(nodes, depth, uniforms, i, n, stratified);
        if ((t & 63) == 0) {
            const int32_t leaf = per_clamp_leaf((int32_t)(node - first_leaf), n_items);
            lf[i] = leaf;
            mb.leaves[i] = leaf;
        }
    }
    __syncthreads();
    const double root = nodes[0];
    double w = 0.0;
    if (t < n) w = per_raw_weight(nodes[first_leaf + (unsigned int)lf[t]], root, n_items, beta);
    if (t < PER_GROUP_MAX_N) raw[t] = w;
    __syncthreads();
    if (t >= n) return;  // (no barrier below)
    double wmax = 0.0;
#pragma unroll
    for (int j = 0; j < PER_GROUP_MAX_N; ++j) wmax = fmax(wmax, raw[j]);
    mb.weights[t] = per_norm_weight(w, wmax);
}

// k_per_write_back's text (per_write_back_body.h) with its kernel arguments read from record blockIdx.x
__global__ __launch_bounds__(ST_THREADS) void k_per_group_write_back(const PerGroupMember* __restrict__ tab, int n, int m) {
    const PerGroupMember& mb = tab[blockIdx.x];
    double* __restrict__ const nodes = mb.nodes;
    const int32_t* __restrict__ const leaves = mb.leaves;
    const float* __restrict__ const td_abs = mb.td_abs;
    double* __restrict__ const priorities_out = mb.priorities;
    double* __restrict__ const max_dev = mb.max_dev;
    double* __restrict__ const delta_scratch = mb.scratch;
    const int depth = mb.depth, K = mb.K, reduce_max = mb.reduce_max;
    const double eps = mb.eps, alpha = mb.alpha;
#include "per_write_back_body.h"
}
