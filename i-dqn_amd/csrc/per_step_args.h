// Argument checks of per_draw / per_write_back (sumtree.hip) and of the call that chains them around a learner step
// (idqn_per_learn_on_replay, qnet.hip).  Plain host C++ without a HIP dependency: each returns NULL when the arguments are
// fine, else the refusal text, so that a caller can refuse before it enqueues, allocates or stages anything.
#pragma once
#include <stdint.h>

#define PER_STEP_MAX_N 256  // targets per k_per_draw / leaves per k_per_write_back launch

static inline const char* per_draw_args_error(const void* nodes, int32_t depth, const void* uniforms, int32_t n, int64_t n_items,
                                              const void* leaves_out, const void* weights_out) {
    if (!nodes || !uniforms || !leaves_out || !weights_out) return "null pointer";
    if (depth < 1 || depth > 31) return "depth not in [1, 31]";
    if (n < 1 || n > PER_STEP_MAX_N) return "n not in [1, 256]";
    if (n_items < 1) return "n_items < 1";
    return nullptr;
}

static inline const char* per_write_back_args_error(const void* nodes, int32_t depth, const void* leaves, const void* td_abs,
                                                    int32_t n_heads, int32_t n, const void* scratch) {
    if (!nodes || !leaves || !td_abs || !scratch) return "null pointer";
    if (depth < 1 || depth > 31) return "depth not in [1, 31]";
    if (n < 1 || n > PER_STEP_MAX_N) return "n not in [1, 256]";
    if (n_heads < 1) return "n_heads < 1";
    return nullptr;
}
