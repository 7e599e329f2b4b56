// The record of a prioritized sampler end and its argument checks: what per_draw / per_write_back / per_turn (sumtree.hip), the
// calls that chain them around learner steps (idqn_per_learn_on_replay, idqn_per_learn_steps_on_replay, qnet.hip) and the group
// call (per_group_args.h) share.  Plain host C++ without a HIP dependency: a check returns NULL when the record is fine, else
// the refusal text, so that a caller can refuse before it enqueues, allocates or stages anything.
#pragma once
#include <stdint.h>

#define PER_STEP_MAX_N 256  // targets per k_per_draw / leaves per k_per_write_back launch

// One prioritized sampler end: a tree and the buffers of one draw (uniforms -> leaves, weights) and one write-back (leaves, |TD| ->
// priorities, running maximum, the tree) on it.  The kernels of per_phases.h take it by value, read it from a table or (k_per_turn) build it from flat arguments; an entry
// that runs one end only leaves the other end's fields zero.  n (and m) are the launch's.
struct PerSampler {
    double* nodes;
    const double* uniforms;  // [n], device (a record made only to be checked may carry the host pointer: the checks test it for NULL)
    int32_t* leaves;
    float* weights;
    const float* td_abs;  // [K][n]
    double *priorities, *max_dev, *scratch;  // priorities, max_dev: may be NULL
    double n_items, beta, eps, alpha;
    int depth, stratified, reduce_max, K;
};

// (The const-ness of nodes and leaves is the entry's: the draw writes leaves and reads nodes, the write-back the other way round.)
static inline PerSampler per_sampler(const double* nodes, int32_t depth, int64_t n_items, const double* uniforms, int32_t stratified, double beta,
                                     const int32_t* leaves, float* weights, const float* td_abs, int32_t n_heads, int32_t reduce_max, double eps,
                                     double alpha, double* priorities, double* max_dev, void* scratch) {
    PerSampler s;
    s.nodes = const_cast<double*>(nodes); s.uniforms = uniforms; s.leaves = const_cast<int32_t*>(leaves); s.weights = weights;
    s.td_abs = td_abs; s.priorities = priorities; s.max_dev = max_dev; s.scratch = (double*)scratch;
    s.n_items = (double)n_items; s.beta = beta; s.eps = eps; s.alpha = alpha;
    s.depth = depth; s.stratified = stratified; s.reduce_max = reduce_max; s.K = n_heads;
    return s;
}

// The record of an idqn_per_step_t / idqn_per_steps_t (include/idqn_hip.h: the same field names) whose draw reads `uniforms`
template <class P>
static inline PerSampler per_sampler_of(const P& p, const double* uniforms, int32_t n_heads) {
    return per_sampler(p.nodes_dev, p.depth, p.n_items, uniforms, p.stratified, p.beta, p.leaves_dev, p.weights_dev, p.td_abs_dev, n_heads,
                       p.reduce_max, p.eps, p.alpha, p.priorities_dev, p.max_priority_dev, p.tree_scratch_dev);
}

static inline const char* per_draw_args_error(const PerSampler& s, int32_t n) {
    if (!s.nodes || !s.uniforms || !s.leaves || !s.weights) return "null pointer";
    if (s.depth < 1 || s.depth > 31) return "depth not in [1, 31]";
    if (n < 1 || n > PER_STEP_MAX_N) return "n not in [1, 256]";
    if (s.n_items < 1.0) return "n_items < 1";
    return nullptr;
}

static inline const char* per_write_back_args_error(const PerSampler& s, int32_t n) {
    if (!s.nodes || !s.leaves || !s.td_abs || !s.scratch) return "null pointer";
    if (s.depth < 1 || s.depth > 31) return "depth not in [1, 31]";
    if (n < 1 || n > PER_STEP_MAX_N) return "n not in [1, 256]";
    if (s.K < 1) return "n_heads < 1";
    return nullptr;
}

// a record that serves a whole step: the draw's check, then the write-back's
static inline const char* per_step_args_error(const PerSampler& s, int32_t n) {
    const char* bad = per_draw_args_error(s, n);
    return bad ? bad : per_write_back_args_error(s, n);
}
