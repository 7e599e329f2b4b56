// Acting path of the impala architecture for UP TO 32 host states, one head each (idqn_act_host_many_impala): the single-state
// chain of idqn_act_host on an impala handle -- impala_trunk on one image, k_imp_d0_fwd, k_fc_q, k_argmax_rows -- with a state
// dimension added.
//
// PER-STATE ARITHMETIC IS THE SINGLE-STATE PATH'S, OPERATION FOR OPERATION:
//   trunk                 the n states run as n nets of one image each through k_imp_conv / k_imp_pool_fwd themselves
//                         (impala_kernels.h: every image is computed on its own, in an order that does not depend on its place in
//                         the launch).  Net e's parameter base is entry e of a device array that k_imp_act_many_bases fills from
//                         the uploaded table, so the captured launches hold no base; the uint8 conv takes state `net`
//                         (k_imp_conv's PER_NET_U8 instantiation: the only difference is which image a workgroup reads).
//   k_imp_act_many_d0     is k_imp_d0_fwd at B = 1 without its epilogue: a pass of 64 features is one chain
//                         pa = fmaf(x[i], W[i][o], pa) from 0 over the pass's features in order.  k_imp_d0_fwd then adds the pass
//                         sums to the bias in pass order; here every (state, pass, unit) sum is STORED, and
//   k_imp_act_many_tail   adds them to the bias in pass order, applies the ReLU, and runs the layers behind Dense_0 as k_fc_q
//                         does at n = 1 (fc_layer itself, as k_fc_act_many).  A head without a hidden layer (d0_split false) has no
//                         Dense_0 launch: the tail runs the whole head on the flattened features.
// The argmax is k_argmax_rows' (first maximum, strict >).  Q rows and actions of state e are therefore the BYTES idqn_act_host
// gives for (head[e], state e): tests/test_gpu_impala_act_many.py compares without a tolerance.  A change to the summation
// order of k_imp_d0_fwd or fc_layer has to be made here too.
//
// What is shared is the Dense_0 stream: the host sorts the states into groups by head (ActManyTable, grouped), and a wave of
// k_imp_act_many_d0 loads its 64 x 64 block of Dense_0/kernel once per chunk of IMP_ACT_SC states of its group.  The grid
// covers the chip: (D / 64 column blocks) x (passes / 4 ranges) x groups workgroups -- 8 x 31 per group at the workload's widths
// (F = 7744: 121 passes, the last range holds one), where k_imp_d0_fwd runs 8.
//
// Stores are plain vector stores and nothing is accumulated across workgroups: two calls on equal state give equal bytes.
// (The one atomic of the chain is the finished-workgroup COUNT of act_many_deliver, the mailbox tail every many-state entry
// shares; no value that reaches the caller passes through it.)
#pragma once
#include "fc_act_many_kernels.h"
#include "imp_act_many_args.h"
#include "impala_kernels.h"

static_assert(IMP_ACT_MAX == ACT_MANY_MAX && IMP_ACT_PASS == IMP_D0_IC, "imp_act_many_args.h restates these two");

struct ImpActManyBasesArgs {
    ActManyNets nets;
    const float** wbase;  // [ACT_MANY_MAX]
};
// one workgroup: wbase[e] = the parameter base of state e's head (entries past n: state 0's, never read)
__global__ __launch_bounds__(64) void k_imp_act_many_bases(ImpActManyBasesArgs a) {
    const int e = threadIdx.x;
    if (e < ACT_MANY_MAX) a.wbase[e] = act_many_params(a.nets, a.nets.tab->head[e < a.nets.tab->n ? e : 0]);
}

struct ImpActManyD0Args {
    ActManyNets nets;
    const float* x;  // [n][F]  the head's input (ReLU outputs of the third Stack)
    float* part;     // [n][NP][D]  pass sums
    long w_off;
    int F, D, NP;    // NP = ceil(F / 64)
};

// grid (ceil(D / 64), ceil(NP / 4), min(n, K)); blockIdx.z past the call's groups exits at once.
// Lane: hidden unit = lane of the wave; wave w: pass 4 blockIdx.y + w; IMP_ACT_SC states of the group per register chunk.
__global__ __launch_bounds__(256) void k_imp_act_many_d0(ImpActManyD0Args a) {
    __shared__ __attribute__((aligned(16))) float xs[IMP_ACT_SC][IMP_ACT_PPW * IMP_ACT_PASS];
    const ActManyTable* tb = a.nets.tab;
    const int g = blockIdx.z;
    if (g >= tb->n_groups) return;
    const int cnt = tb->g_count[g], first = tb->g_start[g];
    const float* W = act_many_params(a.nets, tb->g_head[g]) + a.w_off;
    const int tid = threadIdx.x, wv = tid >> 6, o = blockIdx.x * IMP_ACT_OC + (tid & 63);
    const int f0 = blockIdx.y * (IMP_ACT_PPW * IMP_ACT_PASS), pass = blockIdx.y * IMP_ACT_PPW + wv, i0 = pass * IMP_ACT_PASS;
    const bool live = o < a.D && pass < a.NP;
    const int nf = live ? min(IMP_ACT_PASS, a.F - i0) : 0;  // features of this wave's pass (idle lanes: none)
    for (int c0 = 0; c0 < cnt; c0 += IMP_ACT_SC) {
        const int nc = min(IMP_ACT_SC, cnt - c0);
        __syncthreads();  // the previous chunk has been read
        for (int e = tid; e < IMP_ACT_SC * IMP_ACT_PPW * IMP_ACT_PASS; e += 256) {
            const int s = e / (IMP_ACT_PPW * IMP_ACT_PASS), f = e % (IMP_ACT_PPW * IMP_ACT_PASS);
            xs[s][f] = (s < nc && f0 + f < a.F) ? a.x[(long)tb->order[first + c0 + s] * a.F + f0 + f] : 0.f;
        }
        __syncthreads();
        float pa[IMP_ACT_SC];
#pragma unroll
        for (int s = 0; s < IMP_ACT_SC; ++s) pa[s] = 0.f;
        for (int il = 0; il < nf; il += 16) {
            float w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = W[(long)(i0 + min(il + u, nf - 1)) * a.D + o];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (il + u < nf) {
#pragma unroll
                    for (int s = 0; s < IMP_ACT_SC; ++s) pa[s] = fmaf(xs[s][wv * IMP_ACT_PASS + il + u], w[u], pa[s]);
                }
        }
        if (live) {
#pragma unroll
            for (int s = 0; s < IMP_ACT_SC; ++s)
                if (s < nc) a.part[((long)tb->order[first + c0 + s] * a.NP + pass) * a.D + o] = pa[s];
        }
    }
}

struct ImpActManyTailArgs {
    FcActManyArgs f;    // net: the layers behind Dense_0 (d0_split) or the whole head; s / s_ld: the features (no split only)
    const float* part;  // [n][NP][D] pass sums of Dense_0, or nullptr (no hidden layer)
    long b0_off;        // Dense_0/bias
    int NP, D;
};

// one workgroup per state, on that state's own head: grid (n)
__global__ __launch_bounds__(256) void k_imp_act_many_tail(ImpActManyTailArgs a) {
    const FcNet& n = a.f.net;
    const int dm = n.dmax, t = threadIdx.x, e = blockIdx.x;
    const float* params = act_many_params(a.f.nets, a.f.nets.tab->head[e]);
    float *cur = a.f.ws + (long)e * 2 * dm, *nxt = cur + dm;
    if (a.part) {  // relu(bias + the pass sums in pass order): k_imp_d0_fwd's `acc = bias; acc += pa` per pass
        const float* part = a.part + (long)e * a.NP * a.D;
        for (int o = t; o < a.D; o += 256) {
            float s = params[a.b0_off + o];
            for (int p = 0; p < a.NP; p += 16) {
                float v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = part[(long)min(p + u, a.NP - 1) * a.D + o];
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    if (p + u < a.NP) s += v[u];
            }
            cur[o] = fmaxf(s, 0.f);
        }
    } else {
        const float* s_in = a.f.s + (long)e * a.f.s_ld;
        for (int i = t; i < n.d[0]; i += 256) cur[i] = s_in[i];
    }
    __syncthreads();
    for (int l = 0; l < n.L; ++l) {
        fc_layer(cur, dm, params + n.w_off[l], params + n.b_off[l], nxt, dm, 1, n.d[l], n.d[l + 1], l != n.L - 1);
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    const int A = n.d[n.L];
    for (int i = t; i < A; i += 256) a.f.q_out[(long)e * A + i] = cur[i];
    if (t == 0) fc_act_many_tail(a.f, e, cur, A);  // (fc_layer ends in a barrier: the row is complete)
}
