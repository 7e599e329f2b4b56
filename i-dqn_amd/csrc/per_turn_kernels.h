// Prioritized-replay EXTENSION, the turn between two consecutive learner steps as ONE launch (include/idqn_hip.h: per_turn):
//   k_per_turn = k_per_write_back of step i  +  k_per_draw of step i + 1
// The write-back runs in one workgroup and the draw that follows must read the tree it leaves, so nothing can run between the two
// and one workgroup does both: the two phases of per_phases.h, so the node array, the running maximum, the priorities, the next
// leaves and the next weights are the two launches' outputs byte for byte.  n <= PER_STEP_MAX_N.
#pragma once
#include "per_phases.h"

// (per_turn_fence, the order between two phases of one workgroup: per_phases.h)
// One workgroup of ST_THREADS threads (16 waves).  The kernel keeps its flat scalar arguments and builds the record of step i in
// registers: with the record passed by value, as k_per_draw and k_per_write_back take it, the same instruction sequence measured
// 0.3 us (n = 32) to 0.6 us (n = 256) slower (profiles/per_phases_refactor.json).  The draw of step i + 1 is on the same tree with
// its own uniforms, leaves and weights.  Descents: descent i on wave i % 16 in cdiv(n, 16) rounds.  No arrival counter: there is
// nobody to wait for.  nodes carries no const / __restrict__, here or as an alias: the draw reads what the write-back stored.
__global__ __launch_bounds__(ST_THREADS) void k_per_turn(double* nodes, int depth, const int32_t* __restrict__ leaves,
                                                         const float* __restrict__ td_abs, int K, int n, int m, int reduce_max, double eps,
                                                         double alpha, double* __restrict__ priorities_out, double* __restrict__ max_dev,
                                                         double* __restrict__ delta_scratch, const double* __restrict__ next_uniforms,
                                                         int stratified, double n_items, double beta, int32_t* next_leaves,
                                                         float* __restrict__ next_weights) {
    PerSampler s;
    s.nodes = nodes; s.uniforms = nullptr; s.leaves = const_cast<int32_t*>(leaves); s.weights = nullptr; s.td_abs = td_abs;
    s.priorities = priorities_out; s.max_dev = max_dev; s.scratch = delta_scratch; s.n_items = n_items; s.beta = beta; s.eps = eps; s.alpha = alpha;
    s.depth = depth; s.stratified = stratified; s.reduce_max = reduce_max; s.K = K;
    per_write_back_phase(s, n, m);
    // The hazard between the phases: the descents below load nodes that OTHER waves of this workgroup stored in phase 4 of the set.
    // The kernel is one workgroup, so every store and every load goes through the one vector L1 of the CU the workgroup runs on
    // (the build does not split workgroups over CUs) and that L1 is write-through: a store leaves it for L2 and a later load of
    // the same CU never finds an older copy of the line there.  What remains is ORDER, and that is per_turn_fence.  No agent-scope
    // fence: no other CU takes part.  The root is read by per_sample_node through the same pointer after stores to it in this
    // kernel, so it stays on the vector path.
    per_turn_fence();
    PerSampler next = s;
    next.uniforms = next_uniforms; next.leaves = next_leaves; next.weights = next_weights;
    per_draw_stage_descents(s.nodes, next, n, threadIdx.x >> 6, ST_THREADS / 64, [&](int i, int32_t leaf) { next_leaves[i] = leaf; });
    per_turn_fence();  // the leaves were stored by lane 0 of other waves of this workgroup: the same order argument
    per_draw_stage_weights<PER_STEP_MAX_N>(s.nodes, next, n, [&](int i) { return next_leaves[i]; });
}
