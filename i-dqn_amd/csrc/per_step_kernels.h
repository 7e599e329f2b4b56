// Prioritized-replay EXTENSION, the two ends of a learner step as one launch each (include/idqn_hip.h: per_draw, per_write_back):
//   k_per_draw        = k_per_sample + k_per_weights      (targets -> leaves == replay slots, clamped -> importance weights)
//   k_per_write_back  = k_per_priorities + k_sumtree_set  (|TD| -> priorities -> running maximum -> the tree)
// Both are built from the device functions of sumtree_device.h the separate kernels are built from, in the same order per
// element, so their outputs are the separate launches' outputs byte for byte.  n <= PER_STEP_MAX_N (per_step_args.h).
#pragma once
#include "per_step_args.h"
#include "sumtree_device.h"

// One wave per descent, four to a workgroup, cdiv(n, 4) workgroups -- the shape of k_per_sample, so the descents of a
// 256-sample batch run side by side.  The last workgroup to arrive (device-scope counter `arrivals`, zero between launches;
// the fences order the leaf stores before the arrival and the arrival before the reads) computes the n weights: thread t owns
// sample t.  fmax is exact under any reduction order, so the tree reduction over 256 threads gives k_per_weights' maximum.
__global__ __launch_bounds__(256) void k_per_draw(const double* __restrict__ nodes, int depth, const double* __restrict__ uniforms, int n,
                                                  int stratified, double n_items, double beta, int32_t* leaves, float* __restrict__ out,
                                                  unsigned* arrivals) {
    __shared__ double red[256];
    __shared__ int is_last;
    const int t = threadIdx.x, i = blockIdx.x * 4 + (t >> 6);
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    if (i < n) {  // wave-uniform
        const unsigned int node = per_sample_node(nodes, depth, uniforms, i, n, stratified);
        if ((t & 63) == 0) leaves[i] = per_clamp_leaf((int32_t)(node - first_leaf), n_items);
    }
    __threadfence();
    __syncthreads();
    if (t == 0) is_last = atomicAdd(arrivals, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    if (t == 0) *arrivals = 0u;  // (nobody else reads it before the next launch)
    const double root = nodes[0];
    double w = 0.0;
    if (t < n) {
        const int32_t leaf = __hip_atomic_load(&leaves[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w = per_raw_weight(nodes[first_leaf + (unsigned int)leaf], root, n_items, beta);
    }
    red[t] = w;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) red[t] = fmax(red[t], red[t + o]);
        __syncthreads();
    }
    if (t < n) out[t] = per_norm_weight(w, red[0]);
}

// One workgroup.  Thread i < n computes priority i (k_per_priorities' arithmetic) into LDS -- and into priorities_out when the
// caller wants them; the running maximum is the workgroup's maximum (an LDS integer maximum of the bit patterns) followed by ONE
// atomicMax on max_dev: the maximum of a set of bit patterns does not depend on how it is grouped, so it is the result of
// k_per_priorities' n atomics.  The body of k_sumtree_set follows with the values read from LDS; m: n rounded up to a power of two.
// The text is per_write_back_body.h, shared with k_per_group_write_back (per_group_kernels.h: the same body on record g of a table).
__global__ __launch_bounds__(ST_THREADS) void k_per_write_back(double* __restrict__ nodes, int depth, const int32_t* __restrict__ leaves,
                                                               const float* __restrict__ td_abs, int K, int n, int m, int reduce_max,
                                                               double eps, double alpha, double* __restrict__ priorities_out,
                                                               double* __restrict__ max_dev, double* __restrict__ delta_scratch) {
#include "per_write_back_body.h"
}
