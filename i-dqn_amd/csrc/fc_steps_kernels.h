// n consecutive replay-sourced MLP ("fc") gradient steps in ONE launch (idqn_learn_steps_on_replay_fc / _dev): the persistent
// sibling of k_fc_step_par (fc_par_kernels.h).
//
// A chain of k_fc_step_par launches repeats, per launch and head, the request of theta, theta_target, m and v from HBM (four
// arenas), their staging into LDS, ~1 us of matrix work and the write-back of theta, m and v -- and the next launch reads the
// same bytes again.  One workgroup owns one head, head k reads only target[k], and neither the target arena nor the replay ring
// changes between the steps of one call: so the n steps are a loop inside the workgroup.
//   * kernel entry requests theta, theta_target, m and v ONCE, in 16-byte pieces, as k_fc_step_par does; all four stay in
//     registers for the whole call; theta, m and v go back to HBM once, behind the last step;
//   * every step puts the freshly updated theta and the target net from registers into their LDS copies (the target's copy
//     becomes the gradient arena behind the forwards, exactly as in the single step: the LDS plan is fc_par_plan's);
//   * the minibatch of step i + 1 is requested while step i runs, its chain of dependent loads cut at the phase boundaries:
//     the samples' slots at the top of step i, their element rows in front of the forwards (32 lanes, handed to the other
//     threads through LDS), the frames behind the TD phase (in flight during the backward) -- no step after the first waits
//     for the ring;
//   * count, cum (a running double, added once per step in step order), losses, the bias-correction scratch, the gradient and
//     the Q debug rows are written for the last step.
// The phases are k_fc_step_par's statement for statement (same tiles on the same waves, same k order, same expressions), so
// that the state after the call equals n single launches byte for byte; prioritized-replay buffers are refused by the entry
// (weights and |TD| belong to one step), so the loss weight is the constant 1.  No communication between workgroups; plain
// loads and vector stores.
#pragma once
#include "fc_par_kernels.h"

// The LDS plan of k_fc_steps_par.  The target net is re-staged from registers every step, so the gradient needs no arena of its
// own: the layout is fc_par_plan's plus, behind its last block (misc_off + 128), the 32 element rows of the next step's
// minibatch (floats = 0: the net does not fit and the entry loops over the single step).
#define FCS_ROW_WORDS (32 * 8)
static inline FcParPlan fc_steps_plan(const FcNet& n, long P) {
    FcParPlan p = fc_par_plan(n, P);
    if (p.floats) p.floats = p.misc_off + 128 + FCS_ROW_WORDS;
    if (p.floats * 4 > FCP_LDS_BUDGET) p.floats = 0;
    return p;
}

template <class Src>
__global__ __launch_bounds__(FCM_T) void k_fc_steps_par(FcArgs a, FcParPlan p, AdamConsts ad, float* theta, float* mu, float* nu, int n_steps, Src src) {
#include "fc_steps_par_body.h"
}
