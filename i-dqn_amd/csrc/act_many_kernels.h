// Acting path for UP TO 32 host states, one head each (idqn_act_host_many): the single-state chain of act_kernels.h with
// a state dimension added.  Same data conventions: uint8 pixels and HWIO / [in][out] leaves as they are, no staging, no
// packing, f32 fma chains.
//
// PER-STATE ARITHMETIC IS THE SINGLE-STATE PATH'S, OPERATION FOR OPERATION: k_act_many_conv cuts (kh, kw, ci) into the
// same units over the same KS lane slices and adds the slices in the same order as k_act_conv; k_act_many_dense0 uses the
// same NRG row groups, the same 8 row sub-groups x 16 rows per round and the same in-order LDS combination as
// k_act_dense0; k_act_many_head sums the NRG partial rows by the same 4 groups, combines them in the same order and runs
// the same Dense_1 wave reduction and first-maximum scan as k_act_head.  Q-values and actions of state e are therefore
// the BYTES idqn_act_host gives for (head[e], state e) -- tests/test_gpu_act_many.py compares without a tolerance.  A
// change to either header's summation order has to be made in both.
//
// What is shared is the Dense_0 stream: the host sorts the states into groups by head, and a workgroup of
// k_act_many_dense0 loads its W0 rows once per chunk of ACT_MANY_SC states of its group (a group of <= ACT_MANY_SC states
// streams its head's 15.9 MB once from HBM; a larger group re-reads a workgroup's ~15 KB of rows from L2).
//
// Heads, groups and the parameter set are DATA: ActManyTable sits at the head of the pinned block whose tail holds the
// states and is uploaded by the chain's one copy node, so a captured chain serves every head assignment and both sets.
// The actions reach the host through act_many_deliver below, shared with iqn_act_many_kernels.h and fc_act_many_kernels.h.
//
// ACTING GROUPS (idqn_act_group_host): the same three bodies with the state's parameter base read from ActGroupTable in the
// uploaded block -- states of different agents in one call.  Each body is stated ONCE, as a __device__ function template over
// the parameter source (ActManyNets / ActGroupNets); k_act_many_* and k_act_group_* are its two instantiations.
#pragma once
#include "common.h"

#define ACT_MANY_MAX 32  // states per call
#define ACT_MANY_SC 8    // states per register chunk of Dense_0

struct ActManyTable {  // 1024 bytes; the n states follow it, in the pinned block and in its device copy
    int32_t n, n_groups, which, pad;
    int32_t head[ACT_MANY_MAX];     // head of state e
    int32_t order[ACT_MANY_MAX];    // state indices sorted by head (stable)
    int32_t g_head[ACT_MANY_MAX];   // group g: head, and its states order[g_start[g] .. g_start[g] + g_count[g])
    int32_t g_start[ACT_MANY_MAX];
    int32_t g_count[ACT_MANY_MAX];
    int32_t fill[256 - 4 - 5 * ACT_MANY_MAX];
};
static_assert(sizeof(ActManyTable) == 1024, "ActManyTable is the 1 KB head of the acting block");

struct ActManyNets {
    const ActManyTable* tab;
    const float *online, *target;  // arenas [K][pstride]
    long pstride;
};
__device__ __forceinline__ const float* act_many_params(const ActManyNets& m, int head) {
    return (m.tab->which ? m.target : m.online) + (long)head * m.pstride;
}

// The head of an acting group's block (idqn_act_group_host): ActManyTable as in every many-state chain, then the parameter
// base of each state's (member, parameter set, head), resolved by the host as FcGroupActTable's are; the n uint8 states follow.
// A Dense_0 group is a run of states with one (member, head): every state of it names the same base.
struct ActGroupTable {
    ActManyTable tab;
    const float* params[ACT_MANY_MAX];
};
static_assert(sizeof(ActGroupTable) == 1024 + 8 * ACT_MANY_MAX, "ActGroupTable is the head of the group's acting block");
struct ActGroupNets {
    const ActGroupTable* gt;
};

// WHERE A PARAMETER BASE COMES FROM is all the three kernel bodies below leave open: one handle's arena by the table's head
// (ActManyNets), or the group's table of bases (ActGroupNets).  Memory nothing writes during the launch, at uniform addresses.
__device__ __forceinline__ const ActManyTable* act_many_table(const ActManyNets& m) { return m.tab; }
__device__ __forceinline__ const float* act_many_state_params(const ActManyNets& m, int e) { return act_many_params(m, m.tab->head[e]); }
__device__ __forceinline__ const float* act_many_group_params(const ActManyNets& m, int g) { return act_many_params(m, m.tab->g_head[g]); }
__device__ __forceinline__ const ActManyTable* act_many_table(const ActGroupNets& m) { return &m.gt->tab; }
__device__ __forceinline__ const float* act_many_state_params(const ActGroupNets& m, int e) { return m.gt->params[e]; }
__device__ __forceinline__ const float* act_many_group_params(const ActGroupNets& m, int g) {
    return m.gt->params[m.gt->tab.order[m.gt->tab.g_start[g]]];
}

// The end of every many-state chain, called by ONE thread of each of the n final workgroups after it has stored its state's
// action.  mail: {action[ACT_MANY_MAX], sequence number} in mapped, coherent host memory; ctr: the device counters behind it,
// ctr[0] the sequence number, ctr[1] the workgroups that have finished.  The workgroup that finishes last (an atomic count of
// the finished ones) copies the n actions into the mailbox, then the sequence number that announces them, and clears the count.
__device__ __forceinline__ void act_many_deliver(int32_t* action, volatile int32_t* mail, unsigned* ctr, int n) {
    __threadfence();  // this workgroup's action is visible device-wide before it is counted
    const unsigned done = atomicAdd(&ctr[1], 1u);
    if (done == (unsigned)n - 1u) {
        __threadfence();
        for (int i = 0; i < n; ++i) mail[i] = __hip_atomic_load(&action[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ctr[1] = 0u;
        const unsigned sq = ctr[0] + 1u;
        ctr[0] = sq;
        __threadfence_system();  // the actions are visible to the host before the number that announces them
        mail[ACT_MANY_MAX] = (int32_t)sq;
    }
}

template <class Nets>
struct ActManyConvArgsT {
    Nets nets;
    const uint8_t* in_u8;  // layer 0: [n][IH][IW][CI] uint8
    const float* in;       // later layers: [n][IH][IW][CI] f32
    float* out;            // [n][OH][OW][CO] f32, after bias + ReLU
    long w_off, b_off;
    int IH, IW, CI, OH, OW, CO, K, S, PLh, PLw;
    int KS;
};
typedef ActManyConvArgsT<ActManyNets> ActManyConvArgs;
typedef ActManyConvArgsT<ActGroupNets> ActGroupConvArgs;

// k_act_conv with the state in blockIdx.y: grid (ceil(n_out / (256 / KS)), n)
template <int CIU, int UPT, class Nets>
__device__ __forceinline__ void act_many_conv(const ActManyConvArgsT<Nets>& a) {
    __shared__ float red[256];
    __shared__ float lut[256];
    const int t = threadIdx.x, per = 256 / a.KS, oi = t % per, ks = t / per, e = blockIdx.y;
    if (a.in_u8) {
        lut[t] = (float)t / 255.0f;
        __syncthreads();
    }
    const long o = (long)blockIdx.x * per + oi;
    const int n_out = a.OH * a.OW * a.CO, n_in = a.IH * a.IW * a.CI, ccs = a.CI / CIU, n_units = a.K * a.K * ccs;
    const float* params = act_many_state_params(a.nets, e);
    const uint8_t* in_u8 = a.in_u8 ? a.in_u8 + (long)e * n_in : nullptr;
    const float* in = a.in ? a.in + (long)e * n_in : nullptr;
    float acc = 0.f;
    if (o < n_out) {
        const int co = (int)(o % a.CO), pos = (int)(o / a.CO), oh = pos / a.OW, ow = pos - oh * a.OW;
        const float* W = params + a.w_off + co;
        float wv[UPT][CIU], xv[UPT][CIU];
#pragma unroll
        for (int n = 0; n < UPT; ++n) {
            const int u = ks + n * a.KS, uc = min(u, n_units - 1);
            const int tap = uc / ccs, c0 = (uc - tap * ccs) * CIU, kh = tap / a.K, kw = tap - kh * a.K;
            const int ih = oh * a.S + kh - a.PLh, iw = ow * a.S + kw - a.PLw;
            const bool live = u < n_units && ih >= 0 && ih < a.IH && iw >= 0 && iw < a.IW;
            const long xi = live ? ((long)ih * a.IW + iw) * a.CI + c0 : 0;
            const float* w = W + ((long)tap * a.CI + c0) * a.CO;
#pragma unroll
            for (int ci = 0; ci < CIU; ++ci) wv[n][ci] = live ? w[(long)ci * a.CO] : 0.f;
            if (in_u8) {
                if (CIU == 4) {  // (n_in is a multiple of 4 and the states start 1 KB into the block: aligned)
                    const unsigned px = *reinterpret_cast<const unsigned*>(in_u8 + xi);
#pragma unroll
                    for (int ci = 0; ci < CIU; ++ci) xv[n][ci] = lut[(px >> (8 * ci)) & 0xffu];
                } else {
#pragma unroll
                    for (int ci = 0; ci < CIU; ++ci) xv[n][ci] = lut[in_u8[xi + ci]];
                }
            } else {
#pragma unroll
                for (int ci = 0; ci < CIU; ++ci) xv[n][ci] = in[xi + ci];
            }
        }
#pragma unroll
        for (int n = 0; n < UPT; ++n)
#pragma unroll
            for (int ci = 0; ci < CIU; ++ci) acc = fmaf(xv[n][ci], wv[n][ci], acc);
    }
    red[t] = acc;
    __syncthreads();
    if (ks == 0 && o < n_out) {
        float s = red[oi];
        for (int j = 1; j < a.KS; ++j) s += red[j * per + oi];  // slices in order
        const int co = (int)(o % a.CO);
        a.out[(long)e * n_out + o] = fmaxf(s + params[a.b_off + co], 0.f);
    }
}
template <int CIU, int UPT>
__global__ __launch_bounds__(256) void k_act_many_conv(ActManyConvArgs a) { act_many_conv<CIU, UPT>(a); }
template <int CIU, int UPT>
__global__ __launch_bounds__(256) void k_act_group_conv(ActGroupConvArgs a) { act_many_conv<CIU, UPT>(a); }

template <class Nets>
struct ActManyDenseArgsT {
    Nets nets;
    const float* a3;  // [n][F]
    float* part;      // [n][NRG][J]
    long w_off;
    int F, J, NRG;
};
typedef ActManyDenseArgsT<ActManyNets> ActManyDenseArgs;
typedef ActManyDenseArgsT<ActGroupNets> ActGroupDenseArgs;
// k_act_dense0 per GROUP of states with one head (of one member): grid (NRG * J / 128, min(n, K)) -- an acting group:
// min(n, S K, 32) --; blockIdx.y past the call's groups exits at once.  The 16 W0 float4 of a round are loaded once and
// applied to every state of the chunk.
template <class Nets>
__device__ __forceinline__ void act_many_dense0(const ActManyDenseArgsT<Nets>& a) {
    __shared__ float4 red[ACT_MANY_SC][8][32];
    const ActManyTable* tb = act_many_table(a.nets);
    const int g = blockIdx.y;
    if (g >= tb->n_groups) return;
    const int cnt = tb->g_count[g], first = tb->g_start[g];
    const float* W0 = act_many_group_params(a.nets, g) + a.w_off;
    const int t = threadIdx.x, cq = t & 31, rs = t >> 5, nq = a.J / 128;
    const int rg = blockIdx.x / nq, jq = (blockIdx.x - rg * nq) * 128 + cq * 4;
    const int r0 = (int)((long)a.F * rg / a.NRG), r1 = (int)((long)a.F * (rg + 1) / a.NRG);
    for (int c0 = 0; c0 < cnt; c0 += ACT_MANY_SC) {
        const int nc = min(ACT_MANY_SC, cnt - c0);
        int st[ACT_MANY_SC];
        float4 s[ACT_MANY_SC];
#pragma unroll
        for (int i = 0; i < ACT_MANY_SC; ++i) {
            st[i] = tb->order[first + c0 + min(i, nc - 1)];
            s[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int rb = r0 + rs; rb < r1; rb += 8 * 16) {
            float4 w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int r = min(rb + 8 * u, r1 - 1);
                w[u] = *reinterpret_cast<const float4*>(W0 + (long)r * a.J + jq);
            }
#pragma unroll
            for (int i = 0; i < ACT_MANY_SC; ++i)
                if (i < nc) {
                    const float* a3 = a.a3 + (long)st[i] * a.F;
                    float x[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) x[u] = a3[min(rb + 8 * u, r1 - 1)];
#pragma unroll
                    for (int u = 0; u < 16; ++u)
                        if (rb + 8 * u < r1) {
                            s[i].x = fmaf(x[u], w[u].x, s[i].x); s[i].y = fmaf(x[u], w[u].y, s[i].y);
                            s[i].z = fmaf(x[u], w[u].z, s[i].z); s[i].w = fmaf(x[u], w[u].w, s[i].w);
                        }
                }
        }
#pragma unroll
        for (int i = 0; i < ACT_MANY_SC; ++i) red[i][rs][cq] = s[i];
        __syncthreads();
        if (rs == 0) {
#pragma unroll
            for (int i = 0; i < ACT_MANY_SC; ++i)
                if (i < nc) {
                    float4 v = red[i][0][cq];
#pragma unroll
                    for (int j = 1; j < 8; ++j) { const float4 y = red[i][j][cq]; v.x += y.x; v.y += y.y; v.z += y.z; v.w += y.w; }
                    *reinterpret_cast<float4*>(a.part + ((long)st[i] * a.NRG + rg) * a.J + jq) = v;
                }
        }
        __syncthreads();  // the next chunk overwrites red
    }
}
__global__ __launch_bounds__(256) void k_act_many_dense0(ActManyDenseArgs a) { act_many_dense0(a); }
__global__ __launch_bounds__(256) void k_act_group_dense0(ActGroupDenseArgs a) { act_many_dense0(a); }

template <class Nets>
struct ActManyHeadArgsT {
    Nets nets;
    const float* part;  // [n][NP][J]
    long b0_off, w1_off, b1_off;
    int NP, J, A, n;
    float* q_out;       // [n][A]
    int32_t* action;    // [n]
    volatile int32_t* mail;  // host mailbox or nullptr, and its device counters: act_many_deliver
    unsigned* ctr;
};
typedef ActManyHeadArgsT<ActManyNets> ActManyHeadArgs;
typedef ActManyHeadArgsT<ActGroupNets> ActGroupHeadArgs;
// k_act_head, one workgroup of 1024 per state; the actions leave through act_many_deliver.
template <class Nets>
__device__ __forceinline__ void act_many_head(const ActManyHeadArgsT<Nets>& a) {
    __shared__ float hp[4][512];
    __shared__ float hs[512];
    __shared__ float qs[32];
    const int t = threadIdx.x, g = t >> 8, jp = (t & 255) * 2, e = blockIdx.x;
    const float* params = act_many_state_params(a.nets, e);
    const float* part = a.part + (long)e * a.NP * a.J;
    if (jp < a.J) {
        const int p0 = a.NP * g / 4, p1 = a.NP * (g + 1) / 4;
        float sx = 0.f, sy = 0.f;
        for (int p = p0; p < p1; p += 32) {
            float2 v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = *reinterpret_cast<const float2*>(part + (long)min(p + u, p1 - 1) * a.J + jp);
#pragma unroll
            for (int u = 0; u < 32; ++u)
                if (p + u < p1) { sx += v[u].x; sy += v[u].y; }
        }
        hp[g][jp] = sx;
        hp[g][jp + 1] = sy;
    }
    __syncthreads();
    if (t < a.J) hs[t] = fmaxf(((hp[0][t] + hp[1][t]) + (hp[2][t] + hp[3][t])) + params[a.b0_off + t], 0.f);
    __syncthreads();
    const int wave = t >> 6, lane = t & 63;
    for (int ac = wave; ac < a.A; ac += 16) {
        float s = 0.f, wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = lane + 64 * u < a.J ? params[a.w1_off + (long)(lane + 64 * u) * a.A + ac] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(lane + 64 * u < a.J ? hs[lane + 64 * u] : 0.f, wv[u], s);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) {
            const float q = s + params[a.b1_off + ac];
            qs[ac] = q;
            a.q_out[(long)e * a.A + ac] = q;
        }
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
__global__ __launch_bounds__(1024) void k_act_many_head(ActManyHeadArgs a) { act_many_head(a); }
__global__ __launch_bounds__(1024) void k_act_group_head(ActGroupHeadArgs a) { act_many_head(a); }
