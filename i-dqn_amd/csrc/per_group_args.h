// Argument and aliasing checks of idqn_group_per_learn_on_replay_fc (qnet.hip) on the S prioritized-replay records of a call
// (those of its n-step form: per_group_steps_args.h).
// Plain host C++ without a HIP dependency, as per_step_args.h: NULL when the records are fine, else the refusal text with
// the member(s) it is about in *g_out (and *j_out: the earlier member that names the same buffer, else -1), so that the
// entry can refuse before it enqueues, allocates or stages anything.
#pragma once
#include "../../include/idqn_hip.h"
#include "per_step_args.h"

#define PER_GROUP_MAX_N 32  // samples per member: the one-launch step's batch limit (RPS_PAR_SLOTS)

// The pair loop: two members that name the same output buffer (P: idqn_per_step_t or idqn_per_steps_t, the same field names)
template <class P>
static inline const char* per_group_alias_error(const P* per, int32_t n_members, int* g_out, int* j_out) {
    for (int g = 1; g < n_members; ++g)
        for (int j = 0; j < g; ++j) {
            const P &a = per[g], &b = per[j];
            const char* bad = nullptr;
            if (a.nodes_dev == b.nodes_dev) bad = "two members name the same nodes_dev: one buffer would have two writers";
            else if (a.leaves_dev == b.leaves_dev) bad = "two members name the same leaves_dev: one buffer would have two writers";
            else if (a.weights_dev == b.weights_dev) bad = "two members name the same weights_dev: one buffer would have two writers";
            else if (a.td_abs_dev == b.td_abs_dev) bad = "two members name the same td_abs_dev: one buffer would have two writers";
            else if (a.tree_scratch_dev == b.tree_scratch_dev) bad = "two members name the same tree_scratch_dev: one buffer would have two writers";
            else if (a.priorities_dev && a.priorities_dev == b.priorities_dev) bad = "two members name the same priorities_dev: one buffer would have two writers";
            else if (a.max_priority_dev && a.max_priority_dev == b.max_priority_dev) bad = "two members name the same max_priority_dev: one buffer would have two writers";
            if (bad) {
                *g_out = g;
                *j_out = j;
                return bad;
            }
        }
    return nullptr;
}

static inline const char* per_group_args_error(const idqn_per_step_t* per, int32_t n_members, int32_t batch, int32_t n_heads, int* g_out,
                                               int* j_out) {
    *g_out = -1;
    *j_out = -1;
    if (!per) return "null pointer";
    if (batch < 1 || batch > PER_GROUP_MAX_N) return "batch not in [1, 32]";
    for (int g = 0; g < n_members; ++g) {
        const idqn_per_step_t& p = per[g];
        *g_out = g;
        if (p.tau_dev) return "tau_dev is set: a group serves MLP members, which take no fractions";
        if (const char* bad = per_step_args_error(per_sampler_of(p, p.uniforms_host, n_heads), batch)) return bad;  // (uniforms: NULL or not)
    }
    if (const char* bad = per_group_alias_error(per, n_members, g_out, j_out)) return bad;
    *g_out = -1;
    return nullptr;
}
