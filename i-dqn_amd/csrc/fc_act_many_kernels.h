// Acting path for UP TO 32 host states, one head each, on the handles idqn_act_host_many refuses: MLP ("fc") handles and
// general-shape cnn handles (idqn_act_host_many_fc).  The single-state chains of those handles with a state dimension
// added; plain f32, no matrix cores -- a latency path of at most 32 workgroups per launch.
//
// PER-STATE ARITHMETIC IS THE SINGLE-STATE PATH'S, OPERATION FOR OPERATION:
//   k_fc_act_many1    is k_fc_q1 (fc_kernels.h): the same 8 wave slices of the k index, the same 16-wide load / fma chunks
//                     with the same zero fill, bias first and then part[0..7] in order, ReLU on all layers but the last;
//   k_fc_act_many     is k_fc_q at n = 1: fc_layer itself, one sequential fmaf chain per output, over a ping-pong
//                     workspace of the state's own;
//   k_gconv_fwd_many  is k_gconv_fwd (gcnn_kernels.h) at B = 1: bias first, then one sequential fmaf chain over
//                     (kh, kw, ci) with out-of-range taps skipped.
// The argmax is k_argmax_rows' (qnet.hip): first maximum, strict >.  Q-values and actions of state e are therefore the
// BYTES idqn_act_host gives for (head[e], state e) -- tests/test_gpu_fc_act_many.py compares without a tolerance.  A
// change to the summation order of k_fc_q1, fc_layer or k_gconv_fwd has to be made here too.
//
// Nothing is shared between the states of one head: a head's whole parameter set is KBs and L2 serves the repeats.
//
// Heads and the parameter set are DATA: ActManyTable (act_many_kernels.h; n, which and head[] are used) sits at the head of
// the pinned block whose tail holds the states -- f32 rows for fc, uint8 pixels for the general-shape cnn -- and is
// uploaded by the chain's one copy node, so a captured chain serves every head assignment and both sets.
// The actions reach the host through act_many_deliver (act_many_kernels.h).
#pragma once
#include "act_many_kernels.h"
#include "fc_kernels.h"

struct FcActManyArgs {
    FcNet net;
    ActManyNets nets;
    const float* s;      // input row of state e at s + e * s_ld: the block's f32 states (fc) or the conv features (general cnn)
    long s_ld;
    float* ws;           // k_fc_act_many only: [n][2][dmax]
    float* q_out;        // [n][A]
    int32_t* action;     // [n]
    volatile int32_t* mail;  // host mailbox or nullptr, and its device counters: act_many_deliver
    unsigned* ctr;
    int n;
};

// Thread 0 of workgroup e, after the A outputs of its state are in q (LDS or global, written before a barrier): the first
// maximum by the rule of k_argmax_rows, then act_many_deliver (act_many_kernels.h).
__device__ __forceinline__ void fc_act_many_tail(const FcActManyArgs& a, int e, const float* q, int A) {
    int best = 0;
    float bv = q[0];
    for (int ac = 1; ac < A; ++ac) {
        const float v = q[ac];
        if (v > bv) { bv = v; best = ac; }
    }
    a.action[e] = best;
    if (a.mail) act_many_deliver(a.action, a.mail, a.ctr, a.n);
}

// k_fc_q1 per state: grid (n), every layer width <= FC_MAX_WIDTH
__global__ __launch_bounds__(512) void k_fc_act_many1(FcActManyArgs a) {
#define FC_ACT_MANY1_PARAMS(e) act_many_params(a.nets, a.nets.tab->head[e])
#include "fc_act_many1_body.h"
#undef FC_ACT_MANY1_PARAMS
}

// k_fc_q at n = 1 per state: grid (n), any widths
__global__ __launch_bounds__(256) void k_fc_act_many(FcActManyArgs a) {
    const FcNet& n = a.net;
    const int dm = n.dmax, t = threadIdx.x, e = blockIdx.x;
    const float* params = act_many_params(a.nets, a.nets.tab->head[e]);
    const float* s_in = a.s + (long)e * a.s_ld;
    float *cur = a.ws + (long)e * 2 * dm, *nxt = cur + dm;
    for (int i = t; i < n.d[0]; i += 256) cur[i] = s_in[i];
    __syncthreads();
    for (int l = 0; l < n.L; ++l) {
        fc_layer(cur, dm, params + n.w_off[l], params + n.b_off[l], nxt, dm, 1, n.d[l], n.d[l + 1], l != n.L - 1);
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    const int A = n.d[n.L];
    for (int i = t; i < A; i += 256) a.q_out[(long)e * A + i] = cur[i];
    if (t == 0) fc_act_many_tail(a, e, cur, A);  // (fc_layer ends in a barrier: the row is complete)
}

struct GConvManyArgs {
    ActManyNets nets;
    const uint8_t* in_u8;  // layer 0: [n][IH][IW][CI] uint8, the states of the block
    const float* in;       // layers 1, 2: [n][IH][IW][CI] f32
    float* out;            // [n][OH][OW][CO]  relu(conv + bias)
    long w_off, b_off;
    int IH, IW, CI, OH, OW, CO, KS, S, PLh, PLw;
};

// k_gconv_fwd with the state in blockIdx.y and that state's net from the table: grid (<= ceil(OH OW CO / 256), n)
__global__ __launch_bounds__(256) void k_gconv_fwd_many(GConvManyArgs a) {
    const int e = blockIdx.y;
    const long n_out = (long)a.OH * a.OW * a.CO, n_in = (long)a.IH * a.IW * a.CI;
    const float* P = act_many_params(a.nets, a.nets.tab->head[e]);
    const float* W = P + a.w_off;
    const uint8_t* in_u8 = a.in ? nullptr : a.in_u8 + (long)e * n_in;  // layer 0
    const float* in = a.in ? a.in + (long)e * n_in : nullptr;          // layers 1, 2
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (long)gridDim.x * 256) {
        long r = i;
        const int co = (int)(r % a.CO); r /= a.CO;
        const int ow = (int)(r % a.OW);
        const int oh = (int)(r / a.OW);
        float s = P[a.b_off + co];
        for (int kh = 0; kh < a.KS; ++kh) {
            const int ih = oh * a.S + kh - a.PLh;
            if (ih < 0 || ih >= a.IH) continue;
            for (int kw = 0; kw < a.KS; ++kw) {
                const int iw = ow * a.S + kw - a.PLw;
                if (iw < 0 || iw >= a.IW) continue;
                const long xi = ((long)ih * a.IW + iw) * a.CI;
                for (int ci = 0; ci < a.CI; ++ci) {
                    const float x = a.in ? in[xi + ci] : (float)in_u8[xi + ci] / 255.0f;  // architectures/dqn.py:44
                    s = fmaf(x, W[((long)(kh * a.KS + kw) * a.CI + ci) * a.CO + co], s);
                }
            }
        }
        a.out[(long)e * n_out + i] = fmaxf(s, 0.f);
    }
}
