// The two phases of a prioritized sampler end (PerSampler, per_step_args.h), each stated once for the kernels that run them:
//   write-back  |TD| -> priorities -> running maximum -> the tree      k_per_write_back, k_per_group_write_back, k_per_turn, k_per_group_turn
//   draw        uniforms -> leaves == replay slots, clamped -> weights  k_per_draw, k_per_group_draw, k_per_turn, k_per_group_turn
// Both are built from the device functions of sumtree_device.h that the separate launches (k_per_priorities + k_sumtree_set,
// k_per_sample + k_per_weights) are built from, in the same order per element, so a kernel that calls them leaves those
// launches' bytes.  A kernel binds its record, does the synchronisation that is its own -- an election between workgroups, the
// fences between two phases of one workgroup -- and calls the phases; n <= PER_STEP_MAX_N, m: n rounded up to a power of two.
#pragma once
#include "per_step_args.h"
#include "sumtree_device.h"

// THE ORDER BETWEEN TWO PHASES OF ONE WORKGROUP (k_per_turn, k_per_group_turn): every wave's stores have completed before any
// wave's loads are issued, and the compiler neither keeps a value in a register across nor moves a load up: workgroup-scope
// release fence (the wave waits for its outstanding stores), the workgroup barrier, workgroup-scope acquire fence; plain vector
// loads after it
__device__ __forceinline__ void per_turn_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// WRITE-BACK, one workgroup of ST_THREADS threads.  Thread i < n computes priority i (k_per_priorities' arithmetic) into LDS --
// and into s.priorities when the caller wants them; the running maximum is the workgroup's maximum (an LDS integer maximum of
// the bit patterns) followed by ONE atomicMax on s.max_dev: the maximum of a set of bit patterns does not depend on how it is
// grouped, so it is the result of k_per_priorities' n atomics.  The body of k_sumtree_set follows with the values read from LDS.
__device__ __forceinline__ void per_write_back_phase(const PerSampler& s, int n, int m) {
    __shared__ unsigned long long key[PER_STEP_MAX_N];
    __shared__ unsigned int cur[PER_STEP_MAX_N];
    __shared__ double pri[PER_STEP_MAX_N];
    __shared__ unsigned long long pmax;
    // (the __restrict__ the flat kernel arguments carried; sumtree_set_body's parameters carry it for nodes, leaves and scratch)
    const float* __restrict__ const td_abs = s.td_abs;
    double* __restrict__ const priorities_out = s.priorities;
    double* __restrict__ const max_dev = s.max_dev;
    const int tid = threadIdx.x;
    if (tid == 0) pmax = 0ull;
    __syncthreads();
    if (tid < n) {
        const double pr = per_priority(td_abs + tid, s.K, n, s.reduce_max, s.eps, s.alpha);
        pri[tid] = pr;
        if (priorities_out) priorities_out[tid] = pr;
        atomicMax(&pmax, (unsigned long long)__double_as_longlong(pr));
    }
    __syncthreads();
    if (tid == 0 && max_dev) atomicMax(reinterpret_cast<unsigned long long*>(max_dev), pmax);
    sumtree_set_body(s.nodes, s.depth, s.leaves, StValuesLds{pri}, n, m, s.scratch, key, cur);
}

// DRAW, in two stages with the kernel's own synchronisation between them (the leaves of the first are read by other waves, or
// other workgroups, in the second).  `nodes` is s.nodes as the kernel may read it: a const __restrict__ alias where the kernel
// only reads the tree, the plain pointer where it has stored to it (k_per_turn: nothing may stay in a register or on the scalar
// path across its write-back).
//
// Descents: one wave per descent (wave_descend shuffles over all 64 lanes, so the loop is wave-uniform), descents first,
// first + stride, ... < n on the calling wave; lane 0 hands the clamped leaf to put(i, leaf).
// (Names: hipcc places equal-sized LDS arrays in symbol-name order.  "per_draw_stage_*" sorts behind "per_write_back_phase", which
// keeps the write-back's arrays in front in k_per_turn, as before the phases were functions; measured, the placement costs nothing.)
template <class Put>
__device__ __forceinline__ void per_draw_stage_descents(const double* nodes, const PerSampler& s, int n, int first, int stride, Put put) {
    const double* __restrict__ const uniforms = s.uniforms;
    const unsigned int first_leaf = (1u << (s.depth - 1)) - 1u;
    for (int i = first; i < n; i += stride) {
        const unsigned int node = per_sample_node(nodes, s.depth, uniforms, i, n, s.stratified);
        if ((threadIdx.x & 63) == 0) put(i, per_clamp_leaf((int32_t)(node - first_leaf), s.n_items));
    }
}

// Weights: thread t < n owns sample t, whose leaf is get(t); every thread of the workgroup calls (W <= the workgroup's size).
// The maximum is taken over W >= n LDS slots whose pad entries hold 0.0.  fmax of finite non-negative values (per_raw_weight
// never yields a NaN: its power has a positive base) is exact and does not depend on grouping or order, so the tree reduction of
// a wide W and the fold in index order that every thread of a narrow W runs for itself (no barrier, W broadcast reads) both find
// the maximum k_per_weights finds.
template <int W, class Get>
__device__ __forceinline__ void per_draw_stage_weights(const double* nodes, const PerSampler& s, int n, Get get) {
    __shared__ double red[W];
    const int t = threadIdx.x;
    const unsigned int first_leaf = (1u << (s.depth - 1)) - 1u;
    const double root = nodes[0];
    double w = 0.0;
    if (t < n) w = per_raw_weight(nodes[first_leaf + (unsigned int)get(t)], root, s.n_items, s.beta);
    if (t < W) red[t] = w;
    __syncthreads();
    double wmax = 0.0;
    if constexpr (W <= 32) {
        if (t >= n) return;  // (no barrier below)
#pragma unroll
        for (int j = 0; j < W; ++j) wmax = fmax(wmax, red[j]);
    } else {
        for (int o = W / 2; o >= 1; o >>= 1) {
            if (t < o) red[t] = fmax(red[t], red[t + o]);
            __syncthreads();
        }
        wmax = red[0];
    }
    if (t < n) s.weights[t] = per_norm_weight(w, wmax);
}
