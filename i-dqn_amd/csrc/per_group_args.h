// Argument and aliasing checks of idqn_group_per_learn_on_replay_fc and idqn_group_per_learn_steps_on_replay_fc (qnet.hip) on the
// S prioritized-replay records of a call, and the layout of the block the call stages.
// Plain host C++ without a HIP dependency, as per_step_args.h: NULL when the records are fine, else the refusal text with
// the member(s) it is about in *g_out (and *j_out: the earlier member that names the same buffer, else -1), so that the
// entry can refuse before it enqueues, allocates or stages anything.
#pragma once
#include <stddef.h>

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

// (tau_dev is a field of the single step's record alone)
static inline const float* per_tau_of(const idqn_per_step_t& p) { return p.tau_dev; }
static inline const float* per_tau_of(const idqn_per_steps_t&) { return nullptr; }

// P: idqn_per_step_t (n_steps == 1) or idqn_per_steps_t; a row of a step is a record of the single call, so its checks are that call's
template <class P>
static inline const char* per_group_args_error(const P* per, int32_t n_members, int32_t n_steps, int32_t batch, int32_t n_heads, int* g_out,
                                               int* j_out) {
    *g_out = -1;
    *j_out = -1;
    if (!per) return "null pointer";
    // (through the library the n-step entry reports this range under its own text before it gets here, and the single entry
    // passes 1: the test below keeps the check whole for a caller that has not, as tools/probes/per_args_probe.cpp)
    if (n_steps < 1 || n_steps > IDQN_MAX_STEPS_PER_CALL) return "n_steps not in [1, 32]";
    if (batch < 1 || batch > PER_GROUP_MAX_N) return "batch not in [1, 32]";
    for (int g = 0; g < n_members; ++g) {
        const P& p = per[g];
        *g_out = g;
        if (per_tau_of(p)) return "tau_dev is set: a group serves MLP members, which take no fractions";
        if (const char* bad = per_step_args_error(per_sampler_of(p, p.uniforms_host, n_heads), batch)) return bad;  // (uniforms: NULL or not)
    }
    if (const char* bad = per_group_alias_error(per, n_members, g_out, j_out)) return bad;
    *g_out = -1;
    return nullptr;
}
static_assert(IDQN_MAX_STEPS_PER_CALL == 32, "the refusal text above names the limit");

// The staged block of a call: {member records [n_steps][S], PerSampler [n_steps][S], uniforms float64 [S][n_steps][batch]}, each
// part 16-byte aligned; `bytes` is what the call uploads.  member_bytes: sizeof(FcGroupMember) (a device-side type).
struct PerGroupStepsBlock {
    size_t samplers_off, uniforms_off, bytes;
};
static inline PerGroupStepsBlock per_group_steps_block(size_t member_bytes, int32_t n_members, int32_t n_steps, int32_t batch) {
    const size_t recs = (size_t)n_members * (size_t)n_steps, a16 = 15;
    PerGroupStepsBlock b;
    b.samplers_off = (recs * member_bytes + a16) & ~a16;
    b.uniforms_off = b.samplers_off + ((recs * sizeof(PerSampler) + a16) & ~a16);
    b.bytes = b.uniforms_off + recs * (size_t)batch * sizeof(double);
    return b;
}
