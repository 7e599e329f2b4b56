// Device functions the sum-tree kernels (sumtree.hip) and the phases of the fused prioritized-replay kernels (per_phases.h) share:
// the wave descent, the body of the batched set, and the target / weight / priority formulas.  One definition each, so the
// fused kernels are bit-identical to the launches they replace by construction.
#pragma once
#include "common.h"

#define ST_THREADS 1024
#define ST_MAX_N 4096

static inline int st_pow2_at_least(int n) {  // (host) m of the batched set: n rounded up to a power of two
    int m = 1;
    while (m < n) m <<= 1;
    return m;
}

// Latency-oriented descent for minibatch-sized queries: ONE WAVE PER QUERY.  The 2^(s+1)-1 nodes of the s <= 5
// levels below the current node are fetched by the 64 lanes in one round trip, then the wave descends those levels
// out of registers (shuffles): depth 21 costs 4 dependent memory round trips instead of 20.  Same comparisons and
// the same `t -= left_sum` sequence as the scalar walk, so the result is bit-identical.
__device__ __forceinline__ unsigned int wave_descend(const double* __restrict__ nodes, int depth, double t, int& bad) {
    const int lane = threadIdx.x & 63;
    unsigned int node = 0;
    int level = 0;
    const int h = lane + 1;                 // 1-based heap number inside the sub-tree; lane 63 idles
    const int j = 31 - __clz(h);            // its level inside the sub-tree
    const unsigned int p = h - (1u << j);  // its position in that level
    while (level < depth - 1) {
        const int s = min(5, depth - 1 - level);
        double v = 0.0;
        if (j <= s && lane < 63) v = nodes[(size_t)(node + 1u) * (1u << j) + p - 1u];
        int cur = 1;
        for (int step = 0; step < s; ++step) {
            const double here = __shfl(v, cur - 1);
            const double ls = __shfl(v, 2 * cur - 1);
            if (!(t < here)) bad |= 2;
            if (t < ls) {
                cur = 2 * cur;
            } else {
                t = t - ls;
                cur = 2 * cur + 1;
            }
        }
        const int jj = 31 - __clz(cur);
        node = (node + 1u) * (1u << jj) + (cur - (1u << jj)) - 1u;
        level += s;
    }
    return node;
}

// Prioritized-replay EXTENSION: the heap node target i of n descends to.  Targets are made on the device from uniforms in
// [0, 1): u * root, or the stratified (i + u) / n * root, clamped below the root; an empty tree answers its first leaf.
__device__ __forceinline__ unsigned int per_sample_node(const double* __restrict__ nodes, int depth, const double* __restrict__ uniforms,
                                                       int i, int n, int stratified) {
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    const double root = nodes[0];
    double t = stratified ? ((double)i + uniforms[i]) / (double)n * root : uniforms[i] * root;
    t = fmin(t, nextafter(root, 0.0));
    int bad = 0;
    return (root > 0.0) ? wave_descend(nodes, depth, t, bad) : first_leaf;
}

// a descent can land on an empty leaf at or past the item count when rounding in the tree sums leaves a sliver of
// mass there: pull it back onto the last live leaf, so that the gather that follows stays inside the store
__device__ __forceinline__ int32_t per_clamp_leaf(int32_t leaf, double n_items) { return min(max(leaf, 0), (int32_t)n_items - 1); }

// w_i = (n_items * p_i / root)^(-beta), before the normalisation by the largest weight of the batch (Schaul et al. 2016, eq. 2)
__device__ __forceinline__ double per_raw_weight(double p, double root, double n_items, double beta) {
    return (p > 0.0 && root > 0.0) ? pow(n_items * p / root, -beta) : 0.0;
}
__device__ __forceinline__ float per_norm_weight(double w, double wmax) { return wmax > 0.0 ? (float)(w / wmax) : 1.0f; }

// priority = (reduce_k |td[k * stride]| + eps)^alpha ; reduce = mean (0) or max (1) over the K heads, ascending k
__device__ __forceinline__ double per_priority(const float* __restrict__ td, int K, long stride, int reduce_max, double eps, double alpha) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = (double)td[(long)k * stride];
        acc = reduce_max ? fmax(acc, v) : acc + v;
    }
    if (!reduce_max) acc /= (double)K;
    return pow(acc + eps, alpha);
}

// The batched set (SumTree.set, sum_tree.py:20-47) by ONE workgroup of ST_THREADS threads: leaf idx[i] <- val(i), i < n <= m
// (m: n rounded up to a power of two).  key / cur are the workgroup's LDS arrays of at least m elements; val(i) is read once
// per i, by thread i % ST_THREADS, before the first barrier.  keys: (node index << 32) | original position; padded with ~0.
template <class Val>
__device__ __forceinline__ void sumtree_set_body(double* __restrict__ nodes, int depth, const int32_t* __restrict__ idx, Val val, int n,
                                                 int m, double* __restrict__ delta_scratch, unsigned long long* key, unsigned int* cur) {
    const int tid = threadIdx.x;
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
#ifdef ST_PROF
#define ST_STAMP(i) if (tid == 0) reinterpret_cast<long long*>(delta_scratch)[6000 + (i)] = wall_clock64();
#else
#define ST_STAMP(i)
#endif
    ST_STAMP(0)
    // 1. deltas against the CURRENT leaf values, before any de-duplication (sum_tree.py:33-34)
    for (int i = tid; i < m; i += ST_THREADS) {
        if (i < n) {
            unsigned int leaf = first_leaf + (unsigned int)idx[i];
            delta_scratch[i] = val(i) - nodes[leaf];
            key[i] = ((unsigned long long)leaf << 32) | (unsigned int)i;
        } else {
            key[i] = ~0ull;
        }
    }
    __syncthreads();
    ST_STAMP(1)
    // 2. sort by (leaf, position): ascending leaves, first occurrence first (np.unique).  Minibatch-sized sets sort by rank
    //    counting (keys are unique; LDS broadcast reads, four barriers in all) instead of the bitonic network's 36-45.
    if (m <= ST_THREADS / 2) {  // (n^2 comparisons: past 512 keys the bitonic network's 55 barriers are cheaper)
        // P threads per key (P = 1024 / m, a power of two): thread (key i = tid % m, part = tid / m) counts the keys below
        // key i among every P-th element; the partial counts meet in an LDS integer (order-free).  With one thread per
        // key the 256-leaf write-back spent 13.8 us here: 12 of the 16 waves had nothing to count but still walked the loop.
        const int P = ST_THREADS / m, i = tid & (m - 1), part = tid / m;
        const unsigned long long mine = i < n ? key[i] : ~0ull;
        if (tid < m) cur[tid] = 0u;  // (cur is free until phase 3)
        __syncthreads();
        if (i < n) {
            int rank = 0;
            for (int j0 = part; j0 < n; j0 += 8 * P) {
                unsigned long long kk[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) kk[u] = key[min(j0 + u * P, n - 1)];
#pragma unroll
                for (int u = 0; u < 8; ++u) rank += (j0 + u * P < n && kk[u] < mine) ? 1 : 0;
            }
            atomicAdd(&cur[i], (unsigned int)rank);
        }
        __syncthreads();
        const unsigned int rk = tid < n ? cur[tid] : 0u;
        const unsigned long long mine0 = tid < n ? key[tid] : ~0ull;
        __syncthreads();
        if (tid < n) key[rk] = mine0;
        __syncthreads();
    } else
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += ST_THREADS) {
                int p = i ^ j;
                if (p > i) {
                    unsigned long long a = key[i], b = key[p];
                    bool asc = (i & k) == 0;
                    if ((a > b) == asc) {
                        key[i] = b;
                        key[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    ST_STAMP(2)
    // 3. sorted deltas; duplicates of a leaf (every occurrence but the first) contribute exactly +0.0
    double dl[ST_MAX_N / ST_THREADS];
#pragma unroll
    for (int q = 0; q < ST_MAX_N / ST_THREADS; ++q) {
        int s = tid + q * ST_THREADS;
        dl[q] = 0.0;
        if (s < n) {
            unsigned int leaf = (unsigned int)(key[s] >> 32);
            bool dup = s > 0 && (unsigned int)(key[s - 1] >> 32) == leaf;
            dl[q] = dup ? 0.0 : delta_scratch[(unsigned int)key[s]];
            cur[s] = leaf;
        }
    }
    __syncthreads();
    // re-use the key array (as doubles) for the sorted deltas
    double* sdelta = reinterpret_cast<double*>(key);
#pragma unroll
    for (int q = 0; q < ST_MAX_N / ST_THREADS; ++q) {
        int s = tid + q * ST_THREADS;
        if (s < n) sdelta[s] = dl[q];
    }
    __syncthreads();
    // 4. every (level, run of equal ancestors) pair at once: a node belongs to exactly one level, so the levels are
    //    independent and all their read-modify-writes are in flight together (one memory round trip instead of
    //    `depth` dependent ones); the head of each run accumulates its run in ascending leaf order, which is the
    //    order np.add.at applies the sorted deltas in (sum_tree.py:39-47).  cur[] holds the sorted leaf nodes; the
    //    ancestor `level` levels up of 0-based heap node x is ((x + 1) >> level) - 1.
    ST_STAMP(3)
    const int pairs = n * depth;
    // Eight (leaf, level) pairs per thread and round: the node reads of all eight are in flight together (one memory round
    // trip per round instead of one per pair -- a 256-leaf write-back has 5376 pairs, i.e. 5-6 per thread).
    for (int pr0 = tid; pr0 < pairs; pr0 += 8 * ST_THREADS) {
        double xs[8];
        unsigned int nd[8];
        int st[8], lv[8];
        bool head[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int pr = pr0 + u * ST_THREADS;
            head[u] = false;
            if (pr < pairs) {
                const int s0 = pr / depth, level = pr - s0 * depth;  // the long runs near the root land on different lanes
                const unsigned int node = ((cur[s0] + 1u) >> level) - 1u;
                st[u] = s0; lv[u] = level; nd[u] = node;
                head[u] = s0 == 0 || ((cur[s0 - 1] + 1u) >> level) - 1u != node;
                if (head[u]) xs[u] = nodes[node];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (!head[u]) continue;
            // The run's deltas are added strictly one after the other (that order IS the result).  The end of the run does
            // not depend on the running sum: it is found first (ancestors of sorted leaves never decrease: a binary search,
            // skipped for the common run of one), so the dependent chain is ONE fp64 add per element -- with the end test
            // inside the chain the root's run cost ~100 cycles per element (13.8 us of a 256-leaf write-back).
            const unsigned int node = nd[u];
            const int level = lv[u];
            double x = xs[u];
            int e = st[u], end = e + 1;
            if (end < n && ((cur[end] + 1u) >> level) - 1u == node) {
                int lo = end, hi = n;  // invariant: elements [st, lo] belong to the run, element hi does not (or hi == n)
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (((cur[mid] + 1u) >> level) - 1u == node) lo = mid; else hi = mid;
                }
                end = hi;
            }
            for (; e + 8 <= end; e += 8) {
                double d[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) d[w] = sdelta[e + w];
#pragma unroll
                for (int w = 0; w < 8; ++w) x = x + d[w];
            }
            for (; e < end; ++e) x = x + sdelta[e];
            nodes[node] = x;
        }
    }
    ST_STAMP(4)
}

// val(i) of the plain set: the caller's array in device memory
struct StValuesGlobal {
    const double* __restrict__ v;
    __device__ __forceinline__ double operator()(int i) const { return v[i]; }
};

// val(i) of the write-back's set (per_write_back_phase, per_phases.h): the priorities the same workgroup has just left in LDS
struct StValuesLds {
    const double* v;
    __device__ __forceinline__ double operator()(int i) const { return v[i]; }
};
