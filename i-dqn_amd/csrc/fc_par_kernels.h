// MLP ("fc") i-DQN gradient step, ONE launch per step: every global read requested at kernel entry, both forwards side by side,
// the gradient assembled in LDS, Adam in one coalesced pass.
//
// Reference: slimdqn/networks/architectures/dqn.py:61-70 (squeeze, [Dense + ReLU] x len(features), Dense), idqn.py:96-124
// (TD target, loss, value_and_grad, optax.adam).  An 11 k-parameter head is < 1 us of matrix work: the step is the length of
// its chain of dependent phases and of the memory round trips inside them.  k_fc_step_mfma (fc_kernels.h) runs one workgroup
// per head through
//   zero LDS | inputs | 3 x (stage W_target to LDS | layer) | 3 x (stage W_online | layer) | TD | 3 x (restage | gradients)
// and a second launch applies Adam: 58 us at K = 3, [100, 100] (profiles/r5_final_loop.txt).  A first one-launch version
// (forwards side by side, weight operands from global in 16-step chunks, Adam operands fetched per gradient tile) took 40 us:
// phase stamps (profiles/r6_fc_phases.txt) showed every phase waiting for global loads it had only just issued.  Here:
//     A second version that kept the forward's weight operands in registers (one dword load per lane and MFMA step) was no
//     faster: 1,000 dword load instructions per workgroup are a longer queue than their latency.
//   * kernel entry requests what the step reads with 16-byte loads in arena order: both nets' parameters (6 + 6 loads per
//     thread), the minibatch, the rewards / actions / terminals; the online theta stays in registers until the last phase
//     (m and v follow behind the forward);
//   * both nets' matrices go to LDS out of those registers, row-major with an odd pitch: the forward tiles read them
//     column-wise, the data gradients row-wise, both conflict-free; the target net's copy is dead after its forward and its
//     LDS becomes the gradient arena;
//   * the target net (waves 4-7) and the online net (waves 0-3) run their forwards at the same time, one column tile per wave,
//     one barrier per layer;
//   * a layer's data-gradient and weight-gradient tiles are dealt to the eight waves together; every gradient tile lands in an
//     LDS copy of the head's arena, and ONE pass writes it out coalesced and applies optax.adam to the registers from entry.
// Batches of <= 32 samples, layer widths <= 128, heads of <= 12 k parameters; anything else runs k_fc_step_mfma / k_fc_step_lds.
// Exact f32 products (v_mfma_f32_32x32x2_f32), k-ordered sums.
#pragma once
#include "dense0_update.h"
#include "fc_kernels.h"
#include "replay_src_kernels.h"

#define FCP_NPT 24   // parameters per thread of the flat (Adam) view: heads of up to 512 x 24 = 12,288 arena floats
#define FCP_LDS_BUDGET (160 * 1024 - 256)

struct FcParPlan {
    long floats;                  // LDS floats (0: the net does not fit this kernel)
    int drows;                    // rows of a target / delta buffer
    long act_row[FC_MAX_LAYERS + 1];  // first row of the online activations of layer input l
    long buf_off, wo_off, wt_off, misc_off;  // wo / wt: the two nets' parameters in ARENA order; wt later holds the gradient
};
static inline FcParPlan fc_par_plan(const FcNet& n, long P) {
    FcParPlan p;
    memset(&p, 0, sizeof(p));
    long rows = 0;
    bool ok = P <= 512L * FCP_NPT && P % 4 == 0;
    for (int l = 0; l <= n.L; ++l) { p.act_row[l] = rows; rows += n.d[l]; }
    for (int l = 0; l < n.L; ++l) ok = ok && n.d[l] <= 128 && n.d[l + 1] <= 128;  // one column tile per wave of a group of four
    ok = ok && 32L * n.d[0] <= 8L * FCM_T;
    p.drows = (n.dmax + 31) / 32 * 32;
    p.buf_off = rows * FCM_BSP;
    long off = p.buf_off + 2L * p.drows * FCM_BSP + 32L * FCM_BSP;  // (32 rows of slack: edge tiles read rows past a buffer's end)
    off = (off + 3) & ~3L;
    p.wo_off = off;
    off += P + 32;        // (+ 32: the last matrix's edge tile reads up to 31 floats past the arena's end)
    p.wt_off = off;
    off += P + 32;
    p.misc_off = off;
    p.floats = off + 128;
    if (!ok || p.floats * 4 > FCP_LDS_BUDGET) p.floats = 0;
    return p;
}

// `src` is the minibatch source (replay_src_kernels.h): FcBatchSrc, the caller's contiguous batch (the step as it always was), or
// FcRingSrc, the replay frame ring (idqn_learn_on_replay_fc / _dev) -- the same single launch either way.
template <class Src>
__global__ __launch_bounds__(FCM_T) void k_fc_step_par(FcArgs a, FcParPlan p, AdamConsts ad, float* theta, float* mu, float* nu, int do_adam, int prof, Src src) {
#include "fc_step_par_body.h"
}
