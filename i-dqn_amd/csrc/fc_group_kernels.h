// Seed groups: S independent MLP ("fc") agents learn and act in ONE launch (idqn_group_*; include/idqn_hip.h).
//
// The one-launch step k_fc_step_par (fc_par_kernels.h), its persistent sibling k_fc_steps_par (fc_steps_kernels.h) and the
// acting kernel k_fc_act_many1 (fc_act_many_kernels.h) use one workgroup per head or state: K = 3 workgroups of a 256-CU chip
// for the LunarLander net.  Within a step the K heads never talk to each other, so S agents are S * K such workgroups:
//   * k_fc_group_step / k_fc_group_steps, grid (K, S): workgroup (k, g) calls fc_step_par / fc_steps_par -- the
//     functions k_fc_step_par / k_fc_steps_par call (phases: fc_par_phases.h) -- for head k of member g.  What a solo
//     launch receives as kernel arguments (FcArgs, the LDS plan, AdamConsts, the arenas, the ring source) is record g of a
//     device table FcGroupMember[S]: loads at uniform addresses from memory nothing writes during the launch.  Every
//     member's bytes after the launch are therefore the bytes of a solo launch on that member.
//   * k_fc_group_act_many1, grid (n): the body of k_fc_act_many1 with the state's parameter base read from a table in the
//     uploaded block (FcGroupActTable: member, parameter set and head resolved by the host) instead of one handle's arena.
// No communication between workgroups beyond act_many_deliver's existing mailbox count; every output byte has one writer (the
// entry refuses a handle named twice); plain loads and vector stores.
#pragma once
#include "fc_act_many_kernels.h"
#include "fc_steps_kernels.h"

struct FcGroupMember {  // what a solo launch of member g receives as kernel arguments
    FcArgs a;
    FcParPlan plan;
    AdamConsts ad;
    float *theta, *mu, *nu;
    FcRingSrc<RpsSlotsDev> src;
};

__global__ __launch_bounds__(FCM_T) void k_fc_group_step(const FcGroupMember* __restrict__ tab, int do_adam) {
    const FcGroupMember& m = tab[blockIdx.y];
    fc_step_par<false>(m.a, m.plan, m.ad, m.theta, m.mu, m.nu, do_adam, m.src);
}

__global__ __launch_bounds__(FCM_T) void k_fc_group_steps(const FcGroupMember* __restrict__ tab, int n_steps) {
    const FcGroupMember& m = tab[blockIdx.y];
    fc_steps_par(m.a, m.plan, m.ad, m.theta, m.mu, m.nu, n_steps, m.src);
}

// The head of the group's acting block: ActManyTable as in every many-state chain (n is used), then the parameter base of
// each state's (member, parameter set, head); the n float32 states follow.
struct FcGroupActTable {
    ActManyTable tab;
    const float* params[ACT_MANY_MAX];
};

__global__ __launch_bounds__(512) void k_fc_group_act_many1(FcActManyArgs a, const FcGroupActTable* __restrict__ gt) {
#define FC_ACT_MANY1_PARAMS(e) gt->params[e]
#include "fc_act_many1_body.h"
#undef FC_ACT_MANY1_PARAMS
}
