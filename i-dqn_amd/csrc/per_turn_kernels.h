// Prioritized-replay EXTENSION, the turn between two consecutive learner steps as ONE launch (include/idqn_hip.h: per_turn):
//   k_per_turn = k_per_write_back of step i  +  k_per_draw of step i + 1
// The write-back runs in one workgroup and the draw that follows must read the tree it leaves, so nothing can run between the two
// and one workgroup does both.  The write-back phase is the text of per_write_back_body.h; the draw phase is built from the device
// functions of sumtree_device.h that k_per_draw calls, in the same order per element, so the node array, the running maximum,
// the priorities, the next leaves and the next weights are the two launches' outputs byte for byte.  n <= PER_STEP_MAX_N.
#pragma once
#include "per_step_args.h"
#include "sumtree_device.h"

// One workgroup of ST_THREADS threads (16 waves).  Descents: one wave each, as in k_per_draw (wave_descend is a wave's function),
// descent i on wave i % 16 in cdiv(n, 16) rounds.  Weights: thread t < n owns sample t and the maximum is k_per_draw's fmax tree
// over 256 LDS slots -- fmax is exact under any grouping, and this is the same grouping anyway.  No arrival counter: there is
// nobody to wait for.  nodes carries no const / __restrict__ here: the draw phase reads what the write-back phase stored.
__global__ __launch_bounds__(ST_THREADS) void k_per_turn(double* nodes, int depth, const int32_t* __restrict__ leaves,
                                                         const float* __restrict__ td_abs, int K, int n, int m, int reduce_max, double eps,
                                                         double alpha, double* __restrict__ priorities_out, double* __restrict__ max_dev,
                                                         double* __restrict__ delta_scratch, const double* __restrict__ next_uniforms,
                                                         int stratified, double n_items, double beta, int32_t* next_leaves,
                                                         float* __restrict__ next_weights) {
#include "per_write_back_body.h"
    // The hazard between the phases: the descents below load nodes that OTHER waves of this workgroup stored in phase 4 of the set.
    // The kernel is one workgroup, so every store and every load goes through the one vector L1 of the CU the workgroup runs on
    // (the build does not split workgroups over CUs) and that L1 is write-through: a store leaves it for L2 and a later load of
    // the same CU never finds an older copy of the line there.  What remains is ORDER -- every wave's stores must have completed
    // before any wave's loads are issued -- and that the compiler neither keeps a node in a register across the phases nor moves
    // a load up.  Mechanism: workgroup-scope release fence (the wave waits for its outstanding stores), the workgroup barrier,
    // workgroup-scope acquire fence; plain vector loads after it.  No agent-scope fence: no other CU takes part.  The root is
    // read by per_sample_node through the same pointer after stores to it in this kernel, so it stays on the vector path.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    __shared__ double red[PER_STEP_MAX_N];
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    for (int i = tid >> 6; i < n; i += ST_THREADS / 64) {  // wave-uniform
        const unsigned int node = per_sample_node(nodes, depth, next_uniforms, i, n, stratified);
        if ((tid & 63) == 0) next_leaves[i] = per_clamp_leaf((int32_t)(node - first_leaf), n_items);
    }
    // the leaves were stored by lane 0 of other waves of this workgroup: the same order argument, the same mechanism
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const double root = nodes[0];
    double w = 0.0;
    if (tid < n) w = per_raw_weight(nodes[first_leaf + (unsigned int)next_leaves[tid]], root, n_items, beta);
    if (tid < PER_STEP_MAX_N) red[tid] = w;
    __syncthreads();
    for (int o = PER_STEP_MAX_N / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
    }
    if (tid < n) next_weights[tid] = per_norm_weight(w, red[0]);
}
