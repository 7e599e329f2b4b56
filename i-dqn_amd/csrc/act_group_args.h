// Host side of idqn_act_group_host (qnet.hip) before anything is enqueued: the range checks of a call's assignment
// (state e on head heads[e] of member member[e]) and the group arrays its Dense_0 launch walks -- the states sorted
// (stable) by (member, head), and one group per run of states with the same pair.  Plain host C++ without a HIP
// dependency, as per_group_args.h: tools/probes/act_group_args_probe.cpp runs it under the sanitizers.
//
// A group never spans two members: the same head on two members names two parameter bases, and a workgroup of
// k_act_group_dense0 streams ONE base's W0 rows for all states of its group.
#pragma once
#include <stdint.h>

#define ACT_GROUP_MAX 32  // states per call, members per group (= ACT_MANY_MAX; qnet.hip asserts it)

// NULL when the assignment is fine, else the refusal text, with the state it is about in *e_out (-1: not about a state)
static inline const char* act_group_args_error(int32_t n, int32_t n_members, int32_t n_heads, int32_t which, const int32_t* member,
                                               const int32_t* heads, int* e_out) {
    *e_out = -1;
    if (!member || !heads) return "null pointer";
    if (n < 1 || n > ACT_GROUP_MAX) return "n is outside [1, 32]";
    if (which != 0 && which != 1) return "which is neither 0 (online) nor 1 (target)";
    if (n_members < 1 || n_members > ACT_GROUP_MAX || n_heads < 1) return "the group has no members or no heads";
    for (int e = 0; e < n; ++e) {
        *e_out = e;
        if (member[e] < 0 || member[e] >= n_members) return "a state's member is outside the group";
        if (heads[e] < 0 || heads[e] >= n_heads) return "a state's head is outside [0, n_heads)";
    }
    *e_out = -1;
    return nullptr;
}

// order[n]: the state indices sorted by (member, head), states of one pair in call order; group g is the states
// order[g_start[g] .. g_start[g] + g_count[g]) of member g_member[g] on head g_head[g].  Every array holds ACT_GROUP_MAX
// entries; entries past n (past the groups) are left as they are.  Returns the number of groups, <= min(n, S K, 32).
// The assignment has passed act_group_args_error.
static inline int act_group_build(int32_t n, const int32_t* member, const int32_t* heads, int32_t* order, int32_t* g_member,
                                  int32_t* g_head, int32_t* g_start, int32_t* g_count) {
    for (int e = 0; e < n; ++e) {  // insertion sort: n <= 32, and equal pairs keep their order
        int at = e;
        while (at > 0) {
            const int p = order[at - 1];
            if (member[p] < member[e] || (member[p] == member[e] && heads[p] <= heads[e])) break;
            order[at] = p;
            --at;
        }
        order[at] = e;
    }
    int ng = 0;
    for (int i = 0; i < n; ++i) {
        const int e = order[i];
        if (ng > 0 && g_member[ng - 1] == member[e] && g_head[ng - 1] == heads[e]) {
            ++g_count[ng - 1];
        } else {
            g_member[ng] = member[e];
            g_head[ng] = heads[e];
            g_start[ng] = i;
            g_count[ng] = 1;
            ++ng;
        }
    }
    return ng;
}
