// Host side of idqn_act_host_many_impala (qnet.hip) before anything is enqueued: the range checks of a call, the check of
// the grouped head table its Dense_0 launch walks, and the plan of that launch.  Plain host C++ without a HIP dependency, as
// act_group_args.h: tools/probes/imp_act_many_args_probe.cpp runs it under the sanitizers, and imp_act_many_kernels.h takes
// its constants from here.
#pragma once
#include <stdint.h>

#define IMP_ACT_MAX 32   // states per call (= ACT_MANY_MAX; qnet.hip asserts it)
#define IMP_ACT_SC 8     // states a Dense_0 lane holds in registers at once: a group of more states walks its weights again
#define IMP_ACT_PASS 64  // features of one Dense_0 pass (= IMP_D0_IC: the blocked sum of k_imp_d0_fwd; qnet.hip asserts it)
#define IMP_ACT_OC 64    // hidden units of a Dense_0 workgroup, one per lane of a wave
#define IMP_ACT_PPW 4    // passes of a Dense_0 workgroup, one per wave

// NULL when the call is fine, else the refusal text, with the state it is about in *e_out (-1: not about a state)
static inline const char* imp_act_many_args_error(int32_t n, int32_t n_heads, int32_t which, const int32_t* heads, const void* states,
                                                  const void* q_out, const void* actions, int* e_out) {
    *e_out = -1;
    if (!heads || !states || !q_out || !actions) return "null pointer";
    if (n < 1 || n > IMP_ACT_MAX) return "n is outside [1, 32]";
    if (which != 0 && which != 1) return "which is neither 0 (online) nor 1 (target)";
    if (n_heads < 1) return "the handle has no heads";
    for (int e = 0; e < n; ++e)
        if (heads[e] < 0 || heads[e] >= n_heads) {
            *e_out = e;
            return "a state's head is outside [0, n_heads)";
        }
    return nullptr;
}

// The grouped table of a call that passed imp_act_many_args_error: head[e] is heads[e]; order[] is a permutation of the n
// states; group g is the states order[g_start[g] .. g_start[g] + g_count[g]), all on head g_head[g], in call order; the
// groups tile [0, n) without a gap, with strictly ascending heads (so one group per head in use, <= min(n, n_heads)).
// NULL when the table is fine, else what is wrong with it, with the group (or state) it is about in *at_out.
static inline const char* imp_act_many_table_error(int32_t n, int32_t n_heads, const int32_t* heads, const int32_t* head, int32_t n_groups,
                                                   const int32_t* order, const int32_t* g_head, const int32_t* g_start,
                                                   const int32_t* g_count, int* at_out) {
    *at_out = -1;
    if (!heads || !head || !order || !g_head || !g_start || !g_count) return "null pointer";
    if (n < 1 || n > IMP_ACT_MAX) return "n is outside [1, 32]";
    if (n_groups < 1 || n_groups > n || n_groups > n_heads) return "the number of groups is outside [1, min(n, n_heads)]";
    uint32_t seen = 0;
    for (int e = 0; e < n; ++e) {
        *at_out = e;
        if (head[e] != heads[e]) return "a state's head differs from the call's";
        if (order[e] < 0 || order[e] >= n) return "an order entry is outside [0, n)";
        if (seen & (1u << order[e])) return "a state appears twice in the order";
        seen |= 1u << order[e];
    }
    int at = 0;
    for (int g = 0; g < n_groups; ++g) {
        *at_out = g;
        if (g_head[g] < 0 || g_head[g] >= n_heads) return "a group's head is outside [0, n_heads)";
        if (g > 0 && g_head[g] <= g_head[g - 1]) return "the groups' heads do not ascend";
        if (g_start[g] != at) return "a group does not start where the one before it ends";
        if (g_count[g] < 1 || g_count[g] > n - at) return "a group's count is outside [1, states left]";
        for (int i = 0; i < g_count[g]; ++i) {
            const int e = order[at + i];
            if (heads[e] != g_head[g]) return "a state is in the group of another head";
            if (i > 0 && e <= order[at + i - 1]) return "the states of a group are not in call order";
        }
        at += g_count[g];
    }
    *at_out = -1;
    if (at != n) return "the groups do not cover the n states";
    return nullptr;
}

// Dense_0 of a head with a hidden layer, F features into D hidden units, for the states of one group:
//   n_pass = ceil(F / 64) passes (the last one ragged when F is no multiple of 64), each summed on its own;
//   a workgroup owns 64 hidden units x 4 passes (wave w: pass 4 r + w of range r; waves past n_pass idle);
//   the grid is (col_blocks, ranges, groups); every (state, pass, unit) partial is stored, [n][n_pass][D] floats.
struct imp_act_many_d0_plan_t {
    int32_t n_pass, ranges, col_blocks, last_pass_features, last_range_passes, last_block_units;
    int64_t part_floats;  // for IMP_ACT_MAX states
};
static inline imp_act_many_d0_plan_t imp_act_many_d0_plan(int32_t F, int32_t D) {
    imp_act_many_d0_plan_t p;
    p.n_pass = (F + IMP_ACT_PASS - 1) / IMP_ACT_PASS;
    p.ranges = (p.n_pass + IMP_ACT_PPW - 1) / IMP_ACT_PPW;
    p.col_blocks = (D + IMP_ACT_OC - 1) / IMP_ACT_OC;
    p.last_pass_features = F - (p.n_pass - 1) * IMP_ACT_PASS;
    p.last_range_passes = p.n_pass - (p.ranges - 1) * IMP_ACT_PPW;
    p.last_block_units = D - (p.col_blocks - 1) * IMP_ACT_OC;
    p.part_floats = (int64_t)IMP_ACT_MAX * p.n_pass * D;
    return p;
}
// register chunks a group of `count` states takes, and the states of its last chunk
static inline int imp_act_many_chunks(int32_t count) { return (count + IMP_ACT_SC - 1) / IMP_ACT_SC; }
static inline int imp_act_many_last_chunk(int32_t count) { return count - (imp_act_many_chunks(count) - 1) * IMP_ACT_SC; }
