// Argument and aliasing checks of idqn_group_per_learn_steps_on_replay_fc (qnet.hip) on the S prioritized-replay records of a
// call, and the layout of the block the call stages.  Plain host C++ without a HIP dependency, as per_group_args.h, whose
// record check (per_step_args_error) and pair loop (per_group_alias_error) it runs: NULL when the records are fine, else the
// refusal text with the member(s) it is about in *g_out (and *j_out: the earlier member that names the same buffer, else -1),
// so that the entry can refuse before it enqueues, allocates or stages anything.
#pragma once
#include <stddef.h>

#include "per_group_args.h"

static inline const char* per_group_steps_args_error(const idqn_per_steps_t* per, int32_t n_members, int32_t n_steps, int32_t batch,
                                                     int32_t n_heads, int* g_out, int* j_out) {
    *g_out = -1;
    *j_out = -1;
    if (!per) return "null pointer";
    if (n_steps < 1 || n_steps > IDQN_MAX_STEPS_PER_CALL) return "n_steps not in [1, 32]";
    if (batch < 1 || batch > PER_GROUP_MAX_N) return "batch not in [1, 32]";
    for (int g = 0; g < n_members; ++g) {
        *g_out = g;
        // (uniforms: NULL or not; a row of a step is a record of the single group call, so its checks are that call's)
        if (const char* bad = per_step_args_error(per_sampler_of(per[g], per[g].uniforms_host, n_heads), batch)) return bad;
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
