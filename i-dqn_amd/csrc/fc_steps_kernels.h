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
// The phases are k_fc_step_par's own functions (fc_par_phases.h: same tiles on the same waves, same k order, same expressions), so
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

// n_steps steps of head blockIdx.x; Src is an FcRingSrc whose slots are [n_steps][B] in device memory
template <class Src>
__device__ __forceinline__ void fc_steps_par(const FcArgs& a, const FcParPlan& p, const AdamConsts& ad, float* theta, float* mu, float* nu, int n_steps,
                                             const Src& src) {
    extern __shared__ __attribute__((aligned(16))) float fl[];
    const int k = blockIdx.x, t = threadIdx.x;
    const FcNet& n = a.net;
    const int B = a.B, A = n.d[n.L];
    const long P = a.P;
    float* dA = fl + p.buf_off;
    float* dB = dA + (long)p.drows * FCM_BSP;
    float* Gs = fl + p.wt_off;
    float* misc = fl + p.misc_off;
    float *sq = misc + 32, *bc = misc + 64;
    int32_t* rowsL = reinterpret_cast<int32_t*>(misc + 128);  // [32][8]: the element rows of the next step's samples (16-byte aligned)
    float* G = a.grad + (long)k * P;
    float* TH = theta + (long)k * P;
    float* MU = mu + (long)k * P;
    float* NU = nu + (long)k * P;
    const int32_t* slots = src.sl.slot;  // [n_steps][B]
    // ---- the four arenas, once, and the first step's minibatch
    constexpr int NV = FCP_NPT / 4;
    float4 th4[NV], tt4[NV], mm4[NV], vv4[NV];
    fcp_load2(TH, a.target + (long)k * P, P, th4, tt4);
    float xin[8], xin2[8];
    float r_b = 0.f;
    int a_b = 0, t_b = 1;
    fcp_ring_minibatch(src, B, n.d[0], xin, xin2, r_b, a_b, t_b);
    fcp_load2(MU, NU, P, mm4, vv4);
    const int32_t count0 = a.count[k];
    double cum = a.cum[k];  // (thread 0's copy is the one written back)
    float loss_last = 0.f;
    for (int step = 0; step < n_steps; ++step) {
        const bool last = step == n_steps - 1;
        // the per-thread index arithmetic of the phases is redone every step: hoisted out of the step loop its results (a few
        // dozen addresses per lane) would sit in registers beside the four arenas and spill
        int tv = t, d0 = n.d[0];
        asm volatile("" : "+v"(tv));
        asm volatile("" : "+s"(d0));
        // (next minibatch, 1 of 3) the slot of sample t of step + 1
        int sl_b = 0;
        if (!last && t < 32 && t < B) sl_b = slots[(long)(step + 1) * B + t];
        fcp_stage<false>(a, p, fl, k, tv, d0, xin, xin2, th4, tt4);  // (theta as the last step left it)
        // (next minibatch, 2 of 3) its element row (32 bytes, 32-byte aligned): back by the end of the forwards
        int4 rw0 = make_int4(0, 0, 0, 0), rw1 = make_int4(0, 0, 0, 1);
        if (!last && t < 32 && t < B) {
            const int4* m = reinterpret_cast<const int4*>(src.rows + (long)sl_b * 8);
            rw0 = m[0]; rw1 = m[1];
        }
        const float* tq = fcp_forwards<false>(a, p, fl, k, count0 + step + 1, bc, last);  // the target net's Q [A][BSP]
        const float* q = fl + p.act_row[n.L] * FCM_BSP;    // the online net's
        if (last) fcp_store_q(a, k, A, tq, q);
        const float g_b = fcp_td<false>(a, k, A, tq, q, r_b, a_b, t_b, 1.0f, sq);
        float* delta = tq == dA ? dB : dA;
        float* dprev = tq == dA ? dA : dB;
        fcp_delta_zero(delta, A);
        if (!last && t < 32 && t < B) {  // the next step's rows to LDS: every thread needs the rows of its elements' samples
            reinterpret_cast<int4*>(rowsL)[2 * t] = rw0;
            reinterpret_cast<int4*>(rowsL)[2 * t + 1] = rw1;
        }
        __syncthreads();
        fcp_delta_set(Gs, P, tv, delta, B, a_b, g_b);
        // (next minibatch, 3 of 3) the frames of step + 1, in flight while the backward runs; this step's inputs are in LDS
        if (!last) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = tv + FCM_T * j;
                xin[j] = xin2[j] = 0.f;
                if (e < B * d0) {
                    const int b = e / d0, i = e - b * d0;
                    const int4 rw = reinterpret_cast<const int4*>(rowsL)[2 * b];  // {newest, valid} of state and next_state
                    const int pix = i / src.stack, back = src.stack - 1 - (i - pix * src.stack);
                    if (back < rw.y) xin[j] = src.frames[rps_ring_slot(rw.x, back, src.n_frames) * src.frame_elems + pix];
                    if (back < rw.w) xin2[j] = src.frames[rps_ring_slot(rw.z, back, src.n_frames) * src.frame_elems + pix];
                }
            }
            if (t < 32 && t < B) { a_b = rw1.x; r_b = __int_as_float(rw1.y); t_b = (int)(uint8_t)rw1.z; }
        }
        __syncthreads();
        const float loss_sum = fcp_loss_sum(sq);
        fcp_backward<false>(a, p, fl, k, Gs, delta, dprev);
        // ---- optax.adam on the registers; the gradient leaves LDS for HBM behind the last step only
        const float rbc1 = bc[0], rbc2 = bc[1];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const long e = 4L * (tv + FCM_T * j);
            if (e < P) {
                const float4 g = *reinterpret_cast<const float4*>(Gs + e);
                if (last) *reinterpret_cast<float4*>(G + e) = g;
                fcp_adam4(ad, rbc1, rbc2, g, th4[j], mm4[j], vv4[j]);
            }
        }
        loss_last = loss_sum / (float)a.Bdiv;
        cum = cum + (double)(loss_sum / (float)a.Bdiv);
        __syncthreads();  // (bc and the gradient arena are read; the next step rewrites them)
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long e = 4L * (t + FCM_T * j);
        if (e < P) {
            *reinterpret_cast<float4*>(TH + e) = th4[j];
            *reinterpret_cast<float4*>(MU + e) = mm4[j];
            *reinterpret_cast<float4*>(NU + e) = vv4[j];
        }
    }
    if (t == 0) {
        a.losses[k] = loss_last;
        a.count[k] = count0 + n_steps;
        a.cum[k] = cum;
    }
}

template <class Src>
__global__ __launch_bounds__(FCM_T) void k_fc_steps_par(FcArgs a, FcParPlan p, AdamConsts ad, float* theta, float* mu, float* nu, int n_steps, Src src) {
    fc_steps_par(a, p, ad, theta, mu, nu, n_steps, src);
}
