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
#include "fc_par_phases.h"
#include "replay_src_kernels.h"

#define FCP_NPT 24   // parameters per thread of the flat (Adam) view: heads of up to 512 x 24 = 12,288 arena floats
#define FCP_LDS_BUDGET (160 * 1024 - 256)

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

// One step of head blockIdx.x: the phases of fc_par_phases.h, with every global read requested at entry.  `src` is the minibatch
// source (replay_src_kernels.h): FcBatchSrc, the caller's contiguous batch, or FcRingSrc, the replay frame ring.
template <bool PROF, class Src>
__device__ __forceinline__ void fc_step_par(const FcArgs& a, const FcParPlan& p, const AdamConsts& ad, float* theta, float* mu, float* nu, int do_adam,
                                            const Src& src) {
    extern __shared__ __attribute__((aligned(16))) float fl[];
    const int k = blockIdx.x, t = threadIdx.x;
    const FcNet& n = a.net;
    const int B = a.B, A = n.d[n.L];
    const long P = a.P;
    float* dA = fl + p.buf_off;                       // target ping, then delta buffers
    float* dB = dA + (long)p.drows * FCM_BSP;
    float* Gs = fl + p.wt_off;                        // (behind the forwards)
    float* misc = fl + p.misc_off;
    float *sq = misc + 32, *bc = misc + 64;
    float* G = a.grad + (long)k * P;
    float* TH = theta + (long)k * P;
    float* MU = mu + (long)k * P;
    float* NU = nu + (long)k * P;
    fcp_stamp<PROF>(a, k, 0);
    // ---- everything the step reads from global memory is requested HERE, before anything waits, in 16-byte pieces
    constexpr int NV = FCP_NPT / 4;
    float4 th4[NV], tt4[NV], mm4[NV], vv4[NV];
    fcp_load2(TH, a.target + (long)k * P, P, th4, tt4);
    float xin[8], xin2[8];  // the minibatch: element e = t + 512 j of [32][d0] (d0 <= 128)
    float r_b = 0.f;
    int a_b = 0, t_b = 1;
    if constexpr (!Src::replay) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = t + FCM_T * j;
            const bool in = e < B * n.d[0];
            xin[j] = in ? a.s[e] : 0.f;
            xin2[j] = in ? a.s2[e] : 0.f;
        }
        if (t < 32 && t < B) { r_b = a.reward[t]; a_b = a.action[t]; t_b = (int)a.terminal[t]; }
    } else {
        fcp_ring_minibatch(src, B, n.d[0], xin, xin2, r_b, a_b, t_b);  // (behind the parameter loads issued above)
    }
    const float w_b = (t < 32 && t < B && a.is_weight) ? a.is_weight[t] : 1.0f;
    fcp_stage<PROF>(a, p, fl, k, t, n.d[0], xin, xin2, th4, tt4);
    const float* tq = fcp_forwards<PROF>(a, p, fl, k, a.count[k] + 1, bc, true);  // the target net's Q [A][BSP]
    const float* q = fl + p.act_row[n.L] * FCM_BSP;    // the online net's
    fcp_store_q(a, k, A, tq, q);
    const float g_b = fcp_td<true>(a, k, A, tq, q, r_b, a_b, t_b, w_b, sq);
    if (do_adam) fcp_load2(MU, NU, P, mm4, vv4);  // Adam's other operands: back long before the last phase
    float* delta = tq == dA ? dB : dA;
    float* dprev = tq == dA ? dA : dB;
    fcp_delta_zero(delta, A);
    __syncthreads();
    fcp_delta_set(Gs, P, t, delta, B, a_b, g_b);
    __syncthreads();
    fcp_stamp<PROF>(a, k, 8);
    const float loss_sum = fcp_loss_sum(sq);
    fcp_backward<PROF>(a, p, fl, k, Gs, delta, dprev);
    // ---- the gradient leaves LDS in arena order, 16 bytes per lane; optax.adam on the operands requested at kernel entry
    const float rbc1 = bc[0], rbc2 = bc[1];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long e = 4L * (t + FCM_T * j);
        if (e < P) {
            const float4 g = *reinterpret_cast<const float4*>(Gs + e);
            *reinterpret_cast<float4*>(G + e) = g;
            if (do_adam) {
                fcp_adam4(ad, rbc1, rbc2, g, th4[j], mm4[j], vv4[j]);
                *reinterpret_cast<float4*>(TH + e) = th4[j];
                *reinterpret_cast<float4*>(MU + e) = mm4[j];
                *reinterpret_cast<float4*>(NU + e) = vv4[j];
            }
        }
    }
    fcp_stamp<PROF>(a, k, 15);
    if (t == 0) {
        a.losses[k] = loss_sum / (float)a.Bdiv;
        if (a.finish_step) {
            a.count[k] += 1;
            a.cum[k] = a.cum[k] + (double)(loss_sum / (float)a.Bdiv);
        }
    }
}

// PROF (the phase stamps, IDQN_FC_PROF) is the host's choice of instantiation: a kernel holds ONE copy of the step
template <bool PROF, class Src>
__global__ __launch_bounds__(FCM_T) void k_fc_step_par(FcArgs a, FcParPlan p, AdamConsts ad, float* theta, float* mu, float* nu, int do_adam, Src src) {
    fc_step_par<PROF>(a, p, ad, theta, mu, nu, do_adam, src);
}
