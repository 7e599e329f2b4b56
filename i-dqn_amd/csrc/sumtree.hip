// HBM-resident fp64 sum tree: set / get / query, bit-exact with the reference's numpy code.
//
// Replaces slimdqn/sample_collection/sum_tree.py:20-102 of the reference.  The one thing that makes
// `set` non-trivial on a GPU is the accumulation ORDER: the reference sorts the updated leaves
// (np.unique) and then does one np.add.at per tree level, i.e. every node that several updated
// leaves share receives ((node + d0) + d1) + ... strictly in ascending-leaf order.  fp64 addition is
// not associative, so unordered atomics would drift from the reference by ulps.  Here a single
// workgroup sorts (leaf, position) keys in LDS; at each level the first lane of every run of equal
// node indices adds its run's deltas sequentially in a register and stores once.  Runs at one level
// touch distinct nodes and different levels touch distinct nodes, so no memory ordering is needed
// between lanes -- only the LDS arrays are shared.  Latency-bound pointer chasing over a 16.8 MB
// array (capacity 2^20); HBM bytes are negligible (n * depth * 16 B).
#include <stdarg.h>

#include <map>
#include <mutex>

#include "common.h"
#include "sumtree_device.h"
#include "per_step_kernels.h"
#include "per_turn_kernels.h"

static thread_local char g_err[512] = "";
void idqn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* idqn_last_error(void) { return g_err; }
// 2: idqn_config_t.n_quantiles, the i-IQN entry points; 3: sumtree_query_host(n_live), the idqn_dp_* family; 4: idqn_learn_on_replay.
// Still 4 after idqn_learn_on_replay_dev, idqn_dp_learn_on_replay and per_priorities_from_td_gathered, and idqn_learn_on_replay
// accepting the IDQN_F_STOP_* flags, and after per_draw, per_write_back and idqn_per_learn_on_replay, and after per_turn and
// idqn_per_learn_steps_on_replay: additions only -- no existing signature, struct or behaviour changed (backward compatible).
extern "C" int idqn_abi_version(void) { return 4; }

__global__ __launch_bounds__(ST_THREADS) void k_sumtree_set(double* __restrict__ nodes, int depth,
                                                            const int32_t* __restrict__ idx,
                                                            const double* __restrict__ val, int n, int m,
                                                            double* __restrict__ delta_scratch) {
    __shared__ unsigned long long key[ST_MAX_N];
    __shared__ unsigned int cur[ST_MAX_N];
    sumtree_set_body(nodes, depth, idx, StValuesGlobal{val}, n, m, delta_scratch, key, cur);  // (sumtree_device.h)
}

__global__ void k_sumtree_get(const double* __restrict__ nodes, int depth, const int32_t* __restrict__ idx, int n,
                              double* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = nodes[((1u << (depth - 1)) - 1u) + (unsigned int)idx[i]];
}

// Level-synchronous descent, one lane per target (sum_tree.py:76-102).
__global__ void k_sumtree_query(const double* __restrict__ nodes, int depth, const double* __restrict__ targets,
                                int n, int32_t* __restrict__ out, int32_t* __restrict__ status) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    double t = targets[i];
    int bad = 0;
    if (!(t >= 0.0 && t < nodes[0])) bad |= 1;  // ValueError in the reference (:73-74)
    unsigned int node = 0;
    while (node < first_leaf) {
        if (!(t < nodes[node])) bad |= 2;  // the reference's per-level assert (:81)
        unsigned int left = 2u * node + 1u;
        double ls = nodes[left];
        if (t < ls) {
            node = left;
        } else {
            t = t - ls;
            node = left + 1u;
        }
    }
    out[i] = (int32_t)(node - first_leaf);
    if (bad) atomicOr(status, bad);
}

// Latency-oriented variant for minibatch-sized queries: one wave per query (wave_descend, sumtree_device.h).
__global__ __launch_bounds__(256) void k_sumtree_query_wave(const double* __restrict__ nodes, int depth,
                                                            const double* __restrict__ targets, int n,
                                                            int32_t* __restrict__ out, int32_t* __restrict__ status) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;  // wave-uniform
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    const double t = targets[i];
    int bad = 0;
    if (!(t >= 0.0 && t < nodes[0])) bad |= 1;
    const unsigned int node = wave_descend(nodes, depth, t, bad);
    if ((threadIdx.x & 63) == 0) {
        out[i] = (int32_t)(node - first_leaf);
        if (bad) atomicOr(status, bad);
    }
}

// Extension (prioritized-replay loop without a host round trip for the root): targets are made on the device from
// uniforms in [0, 1): u * root, or the stratified (i + u) / n * root, clamped below the root.
__global__ __launch_bounds__(256) void k_per_sample(const double* __restrict__ nodes, int depth,
                                                    const double* __restrict__ uniforms, int n, int stratified,
                                                    int32_t* __restrict__ out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    const unsigned int node = per_sample_node(nodes, depth, uniforms, i, n, stratified);
    if ((threadIdx.x & 63) == 0) out[i] = (int32_t)(node - first_leaf);
}

extern "C" int sumtree_set(double* nodes_dev, int32_t depth, const int32_t* indices_dev, const double* values_dev,
                           int32_t n, void* scratch_dev, void* stream) {
    IDQN_REQUIRE(nodes_dev && indices_dev && values_dev && scratch_dev, "sumtree_set: null pointer");
    IDQN_REQUIRE(depth >= 1 && depth <= 31, "sumtree_set: depth %d out of range", depth);
    IDQN_REQUIRE(n >= 1 && n <= ST_MAX_N, "sumtree_set: n = %d, must be in [1, %d]", n, ST_MAX_N);
    hipLaunchKernelGGL(k_sumtree_set, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, nodes_dev, depth, indices_dev,
                       values_dev, n, st_pow2_at_least(n), (double*)scratch_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int sumtree_get(const double* nodes_dev, int32_t depth, const int32_t* indices_dev, int32_t n,
                           double* out_dev, void* stream) {
    IDQN_REQUIRE(nodes_dev && indices_dev && out_dev && n >= 1, "sumtree_get: bad arguments");
    hipLaunchKernelGGL(k_sumtree_get, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, nodes_dev, depth,
                       indices_dev, n, out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int sumtree_query(const double* nodes_dev, int32_t depth, const double* targets_dev, int32_t n,
                             int32_t* out_dev, int32_t* status_dev, void* stream) {
    IDQN_REQUIRE(nodes_dev && targets_dev && out_dev && status_dev && n >= 1, "sumtree_query: bad arguments");
    IDQN_REQUIRE(depth >= 1 && depth <= 31, "sumtree_query: depth %d out of range", depth);
    if (n <= 2048)  // minibatch-sized: latency matters, one wave per query
        hipLaunchKernelGGL(k_sumtree_query_wave, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, nodes_dev, depth,
                           targets_dev, n, out_dev, status_dev);
    else
        hipLaunchKernelGGL(k_sumtree_query, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, nodes_dev, depth,
                           targets_dev, n, out_dev, status_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// ---------------------------------------------------------------------------------------------------
// Prioritized-replay EXTENSION (the reference has no write-back path: its sample() drops the keys,
// replay_buffer.py:222-230, so there is no behaviour to match here -- parity unpinned).
// ---------------------------------------------------------------------------------------------------
// w_i = (n_items * p_i / root)^(-beta), normalised by the largest weight of the batch (Schaul et al. 2016, eq. 2).
__global__ __launch_bounds__(1024) void k_per_weights(const double* __restrict__ nodes, int depth,
                                                      int32_t* __restrict__ leaves, int n, double n_items,
                                                      double beta, float* __restrict__ out) {
    __shared__ double red[1024];
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    const double root = nodes[0];
    double wmax = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) leaves[i] = per_clamp_leaf(leaves[i], n_items);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double p = nodes[first_leaf + (unsigned int)leaves[i]];
        wmax = fmax(wmax, per_raw_weight(p, root, n_items, beta));
    }
    red[threadIdx.x] = wmax;
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    wmax = red[0];
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double p = nodes[first_leaf + (unsigned int)leaves[i]];
        out[i] = per_norm_weight(per_raw_weight(p, root, n_items, beta), wmax);
    }
}

// priority_i = (reduce_k |td[k][i]| + eps)^alpha ; reduce = mean (0) or max (1) over the K heads; also keeps the
// running maximum priority (the reference's `max_recorded_priority`, sum_tree.py:18,32) in max_dev[0].
// td_abs is [W][K][b] (the data-parallel step's gather of every rank's [K][b]; W = 1, b = n: the single-device [K][n]);
// priority i = r b + j of the global batch comes from rank r's sample j -- the same arithmetic in the same order either way
__global__ void k_per_priorities(const float* __restrict__ td_abs, int K, int n, int b, int reduce_max, double eps,
                                 double alpha, double* __restrict__ out, double* __restrict__ max_dev) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = i / b, j = i - r * b;
    const float* td = td_abs + (long)r * K * b + j;
    const double pr = per_priority(td, K, b, reduce_max, eps, alpha);
    out[i] = pr;
    if (max_dev) atomicMax(reinterpret_cast<unsigned long long*>(max_dev), (unsigned long long)__double_as_longlong(pr));
}

// One leaf, index passed by value (no index upload): leaf <- value, every ancestor += (value - old leaf) -- exactly
// what SumTree.set does for a single element (sum_tree.py:33-47).  value_dev, when given, overrides `value`.
// One wave: lane l owns the ancestor l levels up (depth <= 31 nodes, all distinct), so the read-modify-writes of the
// whole path are in flight together -- two dependent memory round trips instead of `depth` (the single-thread walk took
// 23 us on a 2^20-leaf tree).  Same arithmetic per node: node + delta.
__global__ __launch_bounds__(64) void k_sumtree_set_one(double* __restrict__ nodes, int depth, int index, double value,
                                                       const double* __restrict__ value_dev, int32_t* __restrict__ index_to_key,
                                                       int key) {
    const unsigned int leaf = ((1u << (depth - 1)) - 1u) + (unsigned int)index;
    const int lane = threadIdx.x;
    const double v = value_dev ? value_dev[0] : value;
    const double delta = v - nodes[leaf];  // (every lane reads the same word: one request)
    if (lane < depth) {
        const unsigned int node = ((leaf + 1u) >> lane) - 1u;
        nodes[node] = nodes[node] + delta;
    }
    if (index_to_key && lane == 0) index_to_key[index] = key;  // samplers.py:64-65 (PrioritizedSamplingDistribution.add)
}

// PrioritizedSamplingDistribution.remove (samplers.py:89-103) without the host read of the moved priority: the last
// entry's priority v = leaf[last] goes into the hole by the two-leaf set {hole: v, last: 0.0} (np.unique order: hole <
// last; deltas against the current leaves; where the two paths meet the node accumulates (x + d_hole) + d_last, as
// np.add.at does), and its key moves in index_to_key.  hole == last: the one-leaf set {hole: 0.0}.
// One wave, lane = level (all nodes of the two paths are distinct per level).
__global__ __launch_bounds__(64) void k_sampler_remove(double* __restrict__ nodes, int depth, int32_t* __restrict__ index_to_key,
                                                      int hole, int last) {
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    const unsigned int lh = first_leaf + (unsigned int)hole, ll = first_leaf + (unsigned int)last;
    const int lane = threadIdx.x;
    const double v = nodes[ll];
    const double d_hole = (hole == last ? 0.0 : v) - nodes[lh];
    const double d_last = 0.0 - v;
    const int moved = index_to_key ? index_to_key[last] : 0;
    if (lane < depth) {
        const unsigned int nh = ((lh + 1u) >> lane) - 1u, nl = ((ll + 1u) >> lane) - 1u;
        if (hole == last) {
            nodes[nh] = nodes[nh] + d_hole;
        } else if (nh == nl) {
            nodes[nh] = (nodes[nh] + d_hole) + d_last;
        } else {
            const double a = nodes[nh], b = nodes[nl];
            nodes[nh] = a + d_hole;
            nodes[nl] = b + d_last;
        }
    }
    if (index_to_key && lane == 0 && hole != last) index_to_key[hole] = moved;  // samplers.py:31-35 swap-with-last
}

extern "C" int sumtree_set_one(double* nodes_dev, int32_t depth, int32_t index, double value, const double* value_dev,
                               void* stream) {
    IDQN_REQUIRE(nodes_dev && depth >= 1 && depth <= 31, "sumtree_set_one: bad arguments");
    IDQN_REQUIRE(index >= 0 && (int64_t)index < ((int64_t)1 << (depth - 1)), "sumtree_set_one: index %d out of range", index);
    IDQN_REQUIRE(value_dev || value >= 0.0, "sumtree_set_one: negative value");
    hipLaunchKernelGGL(k_sumtree_set_one, dim3(1), dim3(64), 0, (hipStream_t)stream, nodes_dev, depth, index, value, value_dev,
                       (int32_t*)nullptr, 0);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int sampler_prioritized_add(double* nodes_dev, int32_t depth, int32_t* index_to_key_dev, int32_t index, int32_t key,
                                       double value, void* stream) {
    IDQN_REQUIRE(nodes_dev && index_to_key_dev && depth >= 1 && depth <= 31, "sampler_prioritized_add: bad arguments");
    IDQN_REQUIRE(index >= 0 && (int64_t)index < ((int64_t)1 << (depth - 1)), "sampler_prioritized_add: index %d out of range", index);
    IDQN_REQUIRE(value >= 0.0, "sampler_prioritized_add: negative value");
    hipLaunchKernelGGL(k_sumtree_set_one, dim3(1), dim3(64), 0, (hipStream_t)stream, nodes_dev, depth, index, value,
                       (const double*)nullptr, index_to_key_dev, key);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int sampler_prioritized_remove(double* nodes_dev, int32_t depth, int32_t* index_to_key_dev, int32_t hole, int32_t last,
                                          void* stream) {
    IDQN_REQUIRE(nodes_dev && depth >= 1 && depth <= 31, "sampler_prioritized_remove: bad arguments");
    IDQN_REQUIRE(hole >= 0 && hole <= last && (int64_t)last < ((int64_t)1 << (depth - 1)),
                 "sampler_prioritized_remove: hole %d / last %d out of range", hole, last);
    hipLaunchKernelGGL(k_sampler_remove, dim3(1), dim3(64), 0, (hipStream_t)stream, nodes_dev, depth, index_to_key_dev, hole, last);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// UniformSamplingDistribution's map on the device (samplers.py:26-49): add writes index_to_key[len] = key, remove writes the
// moved last key into the hole -- both are ONE int32 store, passed by value (the host map knows index and key); sample maps
// the host generator's indices to keys with a gather.  Only a sampler that opts in pays for it (the reference protocol hands
// host keys to host code; the device copy serves callers that keep the sampled keys on the device).
__global__ void k_sampler_map_set(int32_t* __restrict__ index_to_key, int index, int key) { index_to_key[index] = key; }
__global__ void k_sampler_map_indices(const int32_t* __restrict__ index_to_key, const int32_t* __restrict__ indices, int n,
                                      int32_t* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = index_to_key[indices[i]];
}
extern "C" int sampler_map_set(int32_t* index_to_key_dev, int32_t index, int32_t key, void* stream) {
    IDQN_REQUIRE(index_to_key_dev && index >= 0, "sampler_map_set: bad arguments");
    hipLaunchKernelGGL(k_sampler_map_set, dim3(1), dim3(1), 0, (hipStream_t)stream, index_to_key_dev, index, key);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}
extern "C" int sampler_map_indices(const int32_t* index_to_key_dev, const int32_t* indices_dev, int32_t n, int32_t* keys_out_dev,
                                   void* stream) {
    IDQN_REQUIRE(index_to_key_dev && indices_dev && keys_out_dev && n >= 1, "sampler_map_indices: bad arguments");
    hipLaunchKernelGGL(k_sampler_map_indices, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, index_to_key_dev, indices_dev, n,
                       keys_out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// ---------------------------------------------------------------------------------------------------
// One host read per query / sample (reference protocol: SumTree.query returns numpy, sum_tree.py:58-102;
// PrioritizedSamplingDistribution.sample returns host keys, samplers.py:105-116).  The n targets (or the n uniforms the
// host's PCG64 produced) sit in a mapped, coherent host mailbox; ONE launch reads them from there, descends, maps the
// leaves through index_to_key and writes leaves, keys, the root and the status bits back into the mailbox; the last wave
// to finish (an arrival counter in device memory) writes the sequence number the host polls.  No device -> host copy,
// no stream synchronisation, no separate read of the root.
// ---------------------------------------------------------------------------------------------------
struct SamplerMailbox {
    unsigned char* host;  // mapped + coherent: [0] f64 root, [8] i32 status, [12] u32 seq, [64] f64 in[max_n], i32 leaves[max_n], i32 keys[max_n]
    unsigned char* dev;   // its device address
    unsigned* ctl;        // device: [0] arrivals, [1] status bits of the launch in flight
    unsigned seq;
    int max_n;
};

__global__ __launch_bounds__(256) void k_sumtree_query_mail(const double* __restrict__ nodes, int depth, int n, int scale_by_root,
                                                            const int32_t* __restrict__ index_to_key, int n_live, unsigned char* mail,
                                                            int max_n, unsigned* ctl, unsigned seq) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;  // wave-uniform
    const unsigned int first_leaf = (1u << (depth - 1)) - 1u;
    const double* in = reinterpret_cast<const double*>(mail + 64);
    int32_t* leaves = reinterpret_cast<int32_t*>(mail + 64 + (size_t)max_n * 8);
    int32_t* keys = leaves + max_n;
    const double root = nodes[0];
    // numpy's Generator.uniform(0.0, root): low + (high - low) * next_double  (sum_tree targets of samplers.py:110)
    const double t = scale_by_root ? 0.0 + (root - 0.0) * in[i] : in[i];
    int bad = 0;
    if (!(t >= 0.0 && t < root)) bad |= 1;  // ValueError in the reference (sum_tree.py:73-74)
    unsigned int node = first_leaf;
    if (root > 0.0) node = wave_descend(nodes, depth, t, bad);
    if ((threadIdx.x & 63) == 0) {
        const int leaf = (int)(node - first_leaf);
        leaves[i] = leaf;
        // the map holds n_live entries: a descent that ends on an empty leaf behind them (drift in the node sums, a target at
        // the root) is the reference's IndexError from `_index_to_key[index]` (samplers.py:114), not a stale or foreign key
        const bool past = index_to_key && n_live >= 0 && leaf >= n_live;
        if (past) bad |= 4;
        keys[i] = index_to_key ? (past ? -1 : index_to_key[leaf]) : leaf;
        if (bad) atomicOr(&ctl[1], (unsigned)bad);
        __threadfence_system();  // this wave's results are visible to the host before its arrival counts
        if (atomicAdd(&ctl[0], 1u) == (unsigned)n - 1u) {  // the last wave of the launch announces it
            const unsigned st = atomicExch(&ctl[1], 0u);
            ctl[0] = 0u;
            *reinterpret_cast<double*>(mail) = root;
            *reinterpret_cast<volatile int32_t*>(mail + 8) = (int32_t)st;
            __threadfence_system();
            *reinterpret_cast<volatile unsigned*>(mail + 12) = seq;
        }
    }
}

extern "C" int sampler_mailbox_create(int32_t max_n, void** mailbox_out) {
    IDQN_REQUIRE(mailbox_out && max_n >= 1 && max_n <= (1 << 20), "sampler_mailbox_create: bad arguments");
    SamplerMailbox* mb = new SamplerMailbox();
    mb->max_n = max_n; mb->seq = 0;
    const size_t bytes = 64 + (size_t)max_n * 16;
    hipError_t e = hipHostMalloc((void**)&mb->host, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) { memset(mb->host, 0, bytes); e = hipHostGetDevicePointer((void**)&mb->dev, mb->host, 0); }
    if (e == hipSuccess) e = hipMalloc((void**)&mb->ctl, 64);
    if (e == hipSuccess) e = hipMemset(mb->ctl, 0, 64);
    // hipMemset of device memory returns before it has run, and the null stream does not order against the (non-blocking)
    // stream of the first query: on an idle stream of its own that launch started before the counters were zero
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        if (mb->ctl) (void)hipFree(mb->ctl);
        if (mb->host) (void)hipHostFree(mb->host);
        delete mb;
        IDQN_HIP_CHECK(e);
    }
    *mailbox_out = mb;
    return IDQN_OK;
}

extern "C" int sampler_mailbox_destroy(void* mailbox) {
    SamplerMailbox* mb = (SamplerMailbox*)mailbox;
    if (!mb) return IDQN_OK;
    (void)hipFree(mb->ctl);
    (void)hipHostFree(mb->host);
    delete mb;
    return IDQN_OK;
}

extern "C" int sumtree_query_host(const double* nodes_dev, int32_t depth, const double* values_host, int32_t n,
                                  int32_t scale_by_root, const int32_t* index_to_key_dev, int32_t n_live, void* mailbox,
                                  int32_t* leaves_out_host, int32_t* keys_out_host, double* root_out_host,
                                  int32_t* status_out_host, void* stream) {
    SamplerMailbox* mb = (SamplerMailbox*)mailbox;
    IDQN_REQUIRE(nodes_dev && values_host && mb && leaves_out_host && root_out_host && status_out_host, "sumtree_query_host: null pointer");
    IDQN_REQUIRE(depth >= 1 && depth <= 31, "sumtree_query_host: depth %d out of range", depth);
    IDQN_REQUIRE(n >= 1 && n <= mb->max_n, "sumtree_query_host: n = %d, the mailbox holds %d", n, mb->max_n);
    hipStream_t q = (hipStream_t)stream;
    memcpy(mb->host + 64, values_host, (size_t)n * 8);
    const unsigned want = ++mb->seq;
    hipLaunchKernelGGL(k_sumtree_query_mail, dim3(cdiv(n, 4)), dim3(256), 0, q, nodes_dev, depth, n, scale_by_root, index_to_key_dev,
                       (int)n_live, mb->dev, mb->max_n, mb->ctl, want);
    IDQN_HIP_CHECK(hipGetLastError());
    volatile unsigned* seqp = reinterpret_cast<volatile unsigned*>(mb->host + 12);
    bool seen = false;
    hipError_t qe = hipSuccess;
    for (long spin = 0; spin < (1L << 34); ++spin) {  // (far longer than anything queued in front of the launch)
        if (*seqp == want) { seen = true; break; }
        __builtin_ia32_pause();
        if ((spin & 0xfffff) == 0xfffff && (qe = hipStreamQuery(q)) != hipErrorNotReady) {
            // the stream has drained (or reports an error): the results were written before the kernel ended
            (void)hipStreamSynchronize(q);
            seen = *seqp == want;
            break;
        }
    }
    if (!seen) {
        (void)hipStreamSynchronize(q);
        unsigned ctl_now[2] = {0, 0};
        (void)hipMemcpy(ctl_now, mb->ctl, 8, hipMemcpyDeviceToHost);
        (void)hipMemset(mb->ctl, 0, 64);
        (void)hipStreamSynchronize(nullptr);
        IDQN_REQUIRE(false, "sumtree_query_host: the launch finished without delivering its results (stream query: %s, mailbox seq %u, wanted %u, "
                            "arrivals %u of %d)", hipGetErrorName(qe), *seqp, want, ctl_now[0], n);
    }
    *root_out_host = *reinterpret_cast<const double*>(mb->host);
    *status_out_host = *reinterpret_cast<const int32_t*>(mb->host + 8);
    const int32_t* lv = reinterpret_cast<const int32_t*>(mb->host + 64 + (size_t)mb->max_n * 8);
    memcpy(leaves_out_host, lv, (size_t)n * 4);
    if (keys_out_host) memcpy(keys_out_host, lv + mb->max_n, (size_t)n * 4);
    return IDQN_OK;
}

extern "C" int per_sample_leaves(const double* nodes_dev, int32_t depth, const double* uniforms_dev, int32_t n,
                                 int32_t stratified, int32_t* leaves_out_dev, void* stream) {
    IDQN_REQUIRE(nodes_dev && uniforms_dev && leaves_out_dev && n >= 1, "per_sample_leaves: bad arguments");
    IDQN_REQUIRE(depth >= 1 && depth <= 31, "per_sample_leaves: depth %d out of range", depth);
    hipLaunchKernelGGL(k_per_sample, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, nodes_dev, depth, uniforms_dev, n,
                       stratified, leaves_out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int per_importance_weights(const double* nodes_dev, int32_t depth, int32_t* leaves_dev, int32_t n,
                                      int64_t n_items, double beta, float* weights_out_dev, void* stream) {
    IDQN_REQUIRE(nodes_dev && leaves_dev && weights_out_dev && n >= 1 && n_items >= 1, "per_importance_weights: bad arguments");
    IDQN_REQUIRE(depth >= 1 && depth <= 31, "per_importance_weights: depth %d out of range", depth);
    hipLaunchKernelGGL(k_per_weights, dim3(1), dim3(1024), 0, (hipStream_t)stream, nodes_dev, depth, leaves_dev, n,
                       (double)n_items, beta, weights_out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int per_priorities_from_td(const float* td_abs_dev, int32_t n_heads, int32_t n, int32_t reduce_max, double eps,
                                      double alpha, double* priorities_out_dev, double* max_priority_dev, void* stream) {
    IDQN_REQUIRE(td_abs_dev && priorities_out_dev && n_heads >= 1 && n >= 1, "per_priorities_from_td: bad arguments");
    hipLaunchKernelGGL(k_per_priorities, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, td_abs_dev, n_heads, n, n,
                       reduce_max, eps, alpha, priorities_out_dev, max_priority_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int per_priorities_from_td_gathered(const float* td_all_dev, int32_t world, int32_t n_heads, int32_t shard,
                                               int32_t reduce_max, double eps, double alpha, double* priorities_out_dev,
                                               double* max_priority_dev, void* stream) {
    IDQN_REQUIRE(td_all_dev && priorities_out_dev && world >= 1 && n_heads >= 1 && shard >= 1 && (long)world * shard <= INT32_MAX,
                 "per_priorities_from_td_gathered: bad arguments");
    const int n = world * shard;
    hipLaunchKernelGGL(k_per_priorities, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, td_all_dev, n_heads, n, shard,
                       reduce_max, eps, alpha, priorities_out_dev, max_priority_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// ---------------------------------------------------------------------------------------------------
// The two ends of a prioritized learner step as one launch each, and the turn between two steps (per_step_kernels.h,
// per_turn_kernels.h: the phases of per_phases.h; include/idqn_hip.h).
// ---------------------------------------------------------------------------------------------------
// k_per_draw's arrival counter: one per stream (launches on a stream run one after the other and each leaves its counter at
// zero), made on the stream's first call and kept for the life of the process.
static int per_draw_counter(hipStream_t q, unsigned** out) {
    static std::mutex mu;
    static std::map<hipStream_t, unsigned*> counters;
    std::lock_guard<std::mutex> lock(mu);
    unsigned*& c = counters[q];
    if (!c) {
        unsigned* p = nullptr;
        hipError_t e = hipMalloc((void**)&p, 64);
        if (e == hipSuccess) e = hipMemset(p, 0, 64);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the zero-fill runs on the null stream)
        if (e != hipSuccess) {
            if (p) (void)hipFree(p);
            counters.erase(q);
            IDQN_HIP_CHECK(e);
        }
        c = p;
    }
    *out = c;
    return IDQN_OK;
}

// Each entry: check the record (per_step_args.h), launch on it.
extern "C" int per_draw(const double* nodes_dev, int32_t depth, const double* uniforms_dev, int32_t n, int32_t stratified,
                        int64_t n_items, double beta, int32_t* leaves_out_dev, float* weights_out_dev, void* stream) {
    const PerSampler s = per_sampler(nodes_dev, depth, n_items, uniforms_dev, stratified, beta, leaves_out_dev, weights_out_dev, nullptr, 0, 0,
                                     0.0, 0.0, nullptr, nullptr, nullptr);
    const char* bad = per_draw_args_error(s, n);
    IDQN_REQUIRE(!bad, "per_draw: %s (depth %d, n %d, n_items %ld)", bad, depth, n, (long)n_items);
    unsigned* arrivals = nullptr;
    if (const int rc = per_draw_counter((hipStream_t)stream, &arrivals)) return rc;
    hipLaunchKernelGGL(k_per_draw, dim3(cdiv(n, 4)), dim3(PER_STEP_MAX_N), 0, (hipStream_t)stream, s, n, arrivals);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int per_write_back(double* nodes_dev, int32_t depth, const int32_t* leaves_dev, const float* td_abs_dev, int32_t n_heads,
                              int32_t n, int32_t reduce_max, double eps, double alpha, double* priorities_out_dev,
                              double* max_priority_dev, void* scratch_dev, void* stream) {
    const PerSampler s = per_sampler(nodes_dev, depth, 0, nullptr, 0, 0.0, leaves_dev, nullptr, td_abs_dev, n_heads, reduce_max, eps, alpha,
                                     priorities_out_dev, max_priority_dev, scratch_dev);
    const char* bad = per_write_back_args_error(s, n);
    IDQN_REQUIRE(!bad, "per_write_back: %s (depth %d, n %d, n_heads %d)", bad, depth, n, n_heads);
    hipLaunchKernelGGL(k_per_write_back, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, s, n, st_pow2_at_least(n));
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// per_write_back on (leaves, |TD|) followed by per_draw on the next uniforms as ONE launch of one workgroup (per_turn_kernels.h).
extern "C" int per_turn(double* nodes_dev, int32_t depth, const int32_t* leaves_dev, const float* td_abs_dev, int32_t n_heads, int32_t n,
                        int32_t reduce_max, double eps, double alpha, double* priorities_out_dev, double* max_priority_dev,
                        void* scratch_dev, const double* next_uniforms_dev, int32_t stratified, int64_t n_items, double beta,
                        int32_t* next_leaves_out_dev, float* next_weights_out_dev, void* stream) {
    const PerSampler s = per_sampler(nodes_dev, depth, n_items, nullptr, stratified, beta, leaves_dev, nullptr, td_abs_dev, n_heads, reduce_max, eps,
                                     alpha, priorities_out_dev, max_priority_dev, scratch_dev);
    PerSampler next = s;  // (the records k_per_turn builds from its flat arguments)
    next.uniforms = next_uniforms_dev; next.leaves = next_leaves_out_dev; next.weights = next_weights_out_dev;
    const char* bad = per_write_back_args_error(s, n);
    if (!bad) bad = per_draw_args_error(next, n);
    IDQN_REQUIRE(!bad, "per_turn: %s (depth %d, n %d, n_heads %d, n_items %ld)", bad, depth, n, n_heads, (long)n_items);
    hipLaunchKernelGGL(k_per_turn, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, nodes_dev, depth, leaves_dev, td_abs_dev, n_heads, n,
                       st_pow2_at_least(n), reduce_max, eps, alpha, priorities_out_dev, max_priority_dev, (double*)scratch_dev, next_uniforms_dev, stratified,
                       (double)n_items, beta, next_leaves_out_dev, next_weights_out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}
