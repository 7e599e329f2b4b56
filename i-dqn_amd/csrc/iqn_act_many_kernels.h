// Acting path of the i-IQN heads for UP TO 32 host states, one head and N <= 64 fractions each (idqn_iqn_act_host_many):
// the single-state chain of iqn_act_kernels.h with a state dimension added, as act_many_kernels.h is to act_kernels.h.
//
// PER-STATE ARITHMETIC IS THE SINGLE-STATE PATH'S, OPERATION FOR OPERATION AND IN THE SAME ORDER: the trunk is
// k_act_many_conv (byte-identical per state to the k_act_conv launches of act_trunk); k_iqn_act_many_cos rounds the same
// fp64 product once; k_iqn_act_many_embed runs the same 64-fma chains in i order; k_iqn_act_many_dense0 keeps the NRG row
// groups, the p0 / p1 row-pair slices of the 8 waves, one v_mfma_f32_32x32x2_f32 per row pair and fraction tile in row-pair
// order into an accumulator of the state's own, and the in-wave-order LDS combination of k_iqn_act_dense0;
// k_iqn_act_many_head sums the groups in order with the same GU, runs the same two rounds of LDS wave reduction, the same
// mean over l = 0 .. N - 1 and the same first-maximum scan as k_iqn_act_head.  Q row e and action e are therefore the
// BYTES idqn_iqn_act_host gives for (which, heads[e], state e, tau[e]) -- tests/test_gpu_iqn_act_many.py compares without
// a tolerance.  A change to either header's summation order has to be made in both.
//
// What is shared is the Dense_0 stream: the host sorts the states into groups by head, and a workgroup of
// k_iqn_act_many_dense0 loads its W0 operands once per chunk of IQN_ACT_MANY_SC states of its group and applies them to
// SC x MT independent accumulators (a group of <= SC states streams its head's W0 once from HBM; a larger group re-reads a
// workgroup's rows from L2).
//
// Heads, groups, the parameter set and the fractions are DATA: the pinned block {ActManyTable, tau [32][64], states} is
// uploaded by the chain's one copy node, so a captured chain serves every head assignment, both sets and every tau.
// The actions reach the host through act_many_deliver (act_many_kernels.h).
#pragma once
#include "act_many_kernels.h"
#include "iqn_act_kernels.h"

#define IQN_ACT_MANY_SC 4  // states per register chunk of Dense_0: 4 x 2 x 16 accumulator registers at MT = 2

struct IqnActManyBlock {  // head of the pinned block and of its device copy; the n states follow it
    ActManyTable tab;
    float tau[ACT_MANY_MAX][64];  // row e: the N fractions of state e
};
static_assert(sizeof(IqnActManyBlock) == 1024 + ACT_MANY_MAX * 64 * 4, "IqnActManyBlock: table, then the fractions");

struct IqnActManyCosArgs {
    const float* tau;  // [n][64]
    float* cosv;       // [n][64][64]
};
// k_iqn_act_cos with the state in blockIdx.y: grid (N, n)
__global__ __launch_bounds__(64) void k_iqn_act_many_cos(IqnActManyCosArgs a) {
    const int l = blockIdx.x, i = threadIdx.x, e = blockIdx.y;
    a.cosv[((long)e * 64 + l) * IQN_ACT_EMBED + i] = (float)cospi((double)(i + 1) * (double)a.tau[e * 64 + l]);
}

struct IqnActManyEmbedArgs {
    ActManyNets nets;
    const float* cosv;  // [n][64][64]
    const float* psi;   // [n][F]
    float* x;           // [n][F][NP]
    long we_off, be_off;
    int F, N, NP;
};
// k_iqn_act_embed with the state in blockIdx.z: grid (ceil(F / 64), MT, n)
__global__ __launch_bounds__(256) void k_iqn_act_many_embed(IqnActManyEmbedArgs a) {
    __shared__ float cs[32][IQN_ACT_EMBED];
    __shared__ float tile[64][33];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, f0 = blockIdx.x * 64, l0 = blockIdx.y * 32, e = blockIdx.z;
    const float* params = act_many_params(a.nets, a.nets.tab->head[e]);
    const float* cosv = a.cosv + (long)e * 64 * IQN_ACT_EMBED;
    float* x = a.x + (long)e * a.F * a.NP;
    for (int i = t; i < 32 * IQN_ACT_EMBED; i += 256) {
        const int l = l0 + i / IQN_ACT_EMBED;
        cs[i / IQN_ACT_EMBED][i % IQN_ACT_EMBED] = l < a.N ? cosv[(long)l * IQN_ACT_EMBED + i % IQN_ACT_EMBED] : 0.f;
    }
    const int f = min(f0 + lane, a.F - 1);
    float we[IQN_ACT_EMBED];
#pragma unroll
    for (int i = 0; i < IQN_ACT_EMBED; ++i) we[i] = params[a.we_off + (long)i * a.F + f];
    const float be = params[a.be_off + f], psi = a.psi[(long)e * a.F + f];
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[n] = 0.f;
#pragma unroll
    for (int i4 = 0; i4 < IQN_ACT_EMBED; i4 += 4) {
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const float4 c = *reinterpret_cast<const float4*>(&cs[w + 4 * n][i4]);
            acc[n] = fmaf(c.x, we[i4], acc[n]);
            acc[n] = fmaf(c.y, we[i4 + 1], acc[n]);
            acc[n] = fmaf(c.z, we[i4 + 2], acc[n]);
            acc[n] = fmaf(c.w, we[i4 + 3], acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) tile[lane][w + 4 * n] = l0 + w + 4 * n < a.N ? psi * fmaxf(acc[n] + be, 0.f) : 0.f;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = t + 256 * it, ff = idx >> 5, ll = idx & 31;
        if (f0 + ff < a.F) x[(long)(f0 + ff) * a.NP + l0 + ll] = tile[ff][ll];
    }
}

struct IqnActManyDenseArgs {
    ActManyNets nets;
    const float* x;  // [n][F][NP]
    float* part;     // [n][NRG][J / 32][2][NP][16]: one single-state layout per state
    long w_off;
    int F, J, NP, NRG;
};
// k_iqn_act_dense0 per GROUP of states with one head: grid (NRG * J / 32, min(n, K)); blockIdx.y past the call's groups
// exits at once.  The 8 W0 operands of a round are loaded once and applied to every state of the chunk: state i's
// accumulators see exactly the MFMA sequence of the single-state kernel (row pairs p0 .. p1 - 1 in order).
template <int MT>
__global__ __launch_bounds__(512) void k_iqn_act_many_dense0(IqnActManyDenseArgs a) {
    __shared__ float sl[8][16][64];
    const ActManyTable* tb = a.nets.tab;
    const int g = blockIdx.y;
    if (g >= tb->n_groups) return;
    const int cnt = tb->g_count[g], first = tb->g_start[g];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, nct = a.J / 32;
    const int rg = blockIdx.x / nct, ct = blockIdx.x - rg * nct;
    const int FP = a.F / 2, slice = rg * 8 + wv, ns = a.NRG * 8;
    const int p0 = (int)((long)FP * slice / ns), p1 = (int)((long)FP * (slice + 1) / ns);
    const float* W = act_many_params(a.nets, tb->g_head[g]) + a.w_off + (long)(lane >> 5) * a.J + ct * 32 + (lane & 31);
    const long xs = (long)a.F * a.NP, ps = (long)a.NRG * nct * 2 * a.NP * 16;  // floats of x / of partials per state
    const float* X0 = a.x + (long)(lane >> 5) * a.NP + (lane & 31);
    for (int c0 = 0; c0 < cnt; c0 += IQN_ACT_MANY_SC) {
        const int nc = min(IQN_ACT_MANY_SC, cnt - c0);
        int st[IQN_ACT_MANY_SC];
        f32x16 acc[IQN_ACT_MANY_SC][MT];
#pragma unroll
        for (int i = 0; i < IQN_ACT_MANY_SC; ++i) {
            st[i] = tb->order[first + c0 + min(i, nc - 1)];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][m][r] = 0.f;
        }
        for (int p = p0; p < p1; p += 8) {
            float wr[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wr[u] = W[(long)min(p + u, p1 - 1) * 2 * a.J];
#pragma unroll
            for (int i = 0; i < IQN_ACT_MANY_SC; ++i)
                if (i < nc) {
                    const float* X = X0 + (long)st[i] * xs;
                    float xr[8][MT];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int m = 0; m < MT; ++m) xr[u][m] = X[(long)min(p + u, p1 - 1) * 2 * a.NP + 32 * m];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (p + u < p1) {
#pragma unroll
                            for (int m = 0; m < MT; ++m) acc[i][m] = mfma32(wr[u], xr[u][m], acc[i][m]);
                        }
                }
        }
#pragma unroll
        for (int i = 0; i < IQN_ACT_MANY_SC; ++i)
            if (i < nc) {
                float* part = a.part + (long)st[i] * ps;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    __syncthreads();  // the previous tile's readers are done with sl
#pragma unroll
                    for (int r = 0; r < 16; ++r) sl[wv][r][lane] = acc[i][m][r];
                    __syncthreads();
#pragma unroll
                    for (int it = 0; it < 2; ++it) {  // as k_iqn_act_dense0: 2 (k) x 32 (l) x 16 (s) values, waves in order
                        const int idx = t + 512 * it, s = idx & 15, lq = (idx >> 4) & 31, k = idx >> 9, jj = 2 * s + k;
                        const int r = 4 * (jj >> 3) + (jj & 3), ln = 32 * ((jj >> 2) & 1) + lq;
                        float v = sl[0][r][ln];
#pragma unroll
                        for (int w2 = 1; w2 < 8; ++w2) v += sl[w2][r][ln];
                        part[((((long)rg * nct + ct) * 2 + k) * a.NP + 32 * m + lq) * 16 + s] = v;
                    }
                }
            }
    }
}

struct IqnActManyHeadArgs {
    ActManyNets nets;
    const float* part;  // [n][NRG][J / 32][2][NP][16]
    long b0_off, w1_off, b1_off;
    int NRG, J, A, N, NP, n;
    float* q_out;       // [n][A]
    int32_t* action;    // [n]
    volatile int32_t* mail;  // host mailbox or nullptr, and its device counters: act_many_deliver
    unsigned* ctr;
};
// k_iqn_act_head, one workgroup of 16 waves per state; the actions leave through act_many_deliver (act_many_kernels.h).
template <int MT>
__global__ __launch_bounds__(1024) void k_iqn_act_many_head(IqnActManyHeadArgs a) {
    __shared__ float sl[8][16][64];
    __shared__ float zf[32][64];
    __shared__ float qs[32];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, k = lane >> 5, lq = lane & 31, nct = a.J / 32, e = blockIdx.x;
    const float* params = act_many_params(a.nets, a.nets.tab->head[e]);
    const long gstride = (long)nct * 2 * a.NP * 16;
    const float* part = a.part + (long)e * a.NRG * gstride;
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    if (wv < nct) {
        float hs[MT][16];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int s = 0; s < 16; ++s) hs[m][s] = 0.f;
        const float* P = part + (((long)wv * 2 + k) * a.NP + lq) * 16;
        constexpr int GU = 4 / MT;  // as k_iqn_act_head
        for (int g = 0; g < a.NRG; g += GU) {
            float4 v[GU][MT][4];
#pragma unroll
            for (int u = 0; u < GU; ++u) {
                const float* Pg = P + (long)min(g + u, a.NRG - 1) * gstride;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[u][m][c] = *reinterpret_cast<const float4*>(Pg + (long)m * 32 * 16 + 4 * c);
            }
#pragma unroll
            for (int u = 0; u < GU; ++u)
                if (g + u < a.NRG) {
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            hs[m][4 * c] += v[u][m][c].x; hs[m][4 * c + 1] += v[u][m][c].y;
                            hs[m][4 * c + 2] += v[u][m][c].z; hs[m][4 * c + 3] += v[u][m][c].w;
                        }
                }
        }
        float w1[16], b0[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int j = 32 * wv + 2 * s + k;
            w1[s] = lq < a.A ? params[a.w1_off + (long)j * a.A + lq] : 0.f;
            b0[s] = params[a.b0_off + j];
        }
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma32(w1[s], fmaxf(hs[m][s] + b0[s], 0.f), acc[m]);
    }
    const int r_ = t >> 6, a_ = mfma_row(r_, lane >> 5);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        float z = 0.f;
        for (int half = 0; half * 8 < nct; ++half) {
            __syncthreads();
            if ((wv >> 3) == half) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sl[wv & 7][r][lane] = acc[m][r];
            }
            __syncthreads();
            const int nw = min(8, nct - half * 8);
            for (int w2 = 0; w2 < nw; ++w2) z += sl[w2][r_][lane];
        }
        zf[a_][32 * m + lq] = a_ < a.A ? z + params[a.b1_off + a_] : 0.f;
    }
    __syncthreads();
    if (t < a.A) {
        float q = 0.f;
        for (int l = 0; l < a.N; ++l) q += zf[t][l];
        q /= (float)a.N;
        qs[t] = q;
        a.q_out[(long)e * a.A + t] = q;
    }
    __syncthreads();
    if (t == 0) {
        int best = 0;
        float bv = qs[0];
        for (int ac = 1; ac < a.A; ++ac)
            if (qs[ac] > bv) { bv = qs[ac]; best = ac; }
        a.action[e] = best;
        if (a.mail) act_many_deliver(a.action, a.mail, a.ctr, a.n);
    }
}
