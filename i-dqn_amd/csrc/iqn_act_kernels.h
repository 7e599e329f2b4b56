// Acting path of the i-IQN heads for ONE state and its N <= 64 quantile fractions (oracle/iqn_ref.py:157-160, the acting
// rule behind idqn.py:126-131): psi(s) from the three k_act_conv launches of act_kernels.h, then
//   k_iqn_act_cos      c[l][i] = cos(pi (i + 1) tau_l), fp64 rounded once -- as k_iqn_cos forms them
//   k_iqn_act_embed    x[f][l] = psi[f] * relu(be[f] + sum_i c[l][i] We[i][f])          (rows l >= N are written as zeros)
//   k_iqn_act_dense0   partial Dense_0 products of NRG row groups on the f32 matrix cores, W0 streamed exactly once
//   k_iqn_act_head     h = relu(b0 + partials in group order), Z = h W1 + b1, q = mean_l Z, first maximum, mailbox
// Everything is transposed with respect to the training kernels: the 32-wide "column" side of v_mfma_f32_32x32x2_f32
// carries the FRACTIONS (NP = 32 or 64 of them, zero rows behind N), its row side 32 hidden units (Dense_0) or the
// actions (Dense_1), so that the partials of one launch are the B operand of the next as they lie in memory.
// All sums run in a fixed order: no atomics, the same bits on every call.
// iqn_act_many_kernels.h repeats this arithmetic per state: a change of summation order has to be made in both headers.
#pragma once
#include "common.h"

constexpr int IQN_ACT_EMBED = 64;  // cos features per fraction (IQN_EMBED of iqn_kernels.h)

struct IqnActCosArgs {
    const float* tau;  // [N] in (0, 1)
    float* cosv;       // [N][64]
};
__global__ __launch_bounds__(64) void k_iqn_act_cos(IqnActCosArgs a) {
    const int l = blockIdx.x, i = threadIdx.x;
    a.cosv[l * IQN_ACT_EMBED + i] = (float)cospi((double)(i + 1) * (double)a.tau[l]);
}

struct IqnActEmbedArgs {
    const float* cosv;    // [N][64]
    const float* psi;     // [F]
    const float* params;
    float* x;             // [F][NP]
    long we_off, be_off;
    int F, N, NP;
};
// workgroup = 64 features x the 32 fractions of tile blockIdx.y: wave w takes fractions w, w + 4, ... (8 chains of 64 fmas
// in i order per thread, the embedding kernel's column in registers, the cosines broadcast from LDS); the tile is turned
// in LDS so that x leaves in 128-byte rows.
__global__ __launch_bounds__(256) void k_iqn_act_embed(IqnActEmbedArgs a) {
    __shared__ float cs[32][IQN_ACT_EMBED];
    __shared__ float tile[64][33];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, f0 = blockIdx.x * 64, l0 = blockIdx.y * 32;
    for (int i = t; i < 32 * IQN_ACT_EMBED; i += 256) {
        const int l = l0 + i / IQN_ACT_EMBED;
        cs[i / IQN_ACT_EMBED][i % IQN_ACT_EMBED] = l < a.N ? a.cosv[(long)l * IQN_ACT_EMBED + i % IQN_ACT_EMBED] : 0.f;
    }
    const int f = min(f0 + lane, a.F - 1);
    float we[IQN_ACT_EMBED];
#pragma unroll
    for (int i = 0; i < IQN_ACT_EMBED; ++i) we[i] = a.params[a.we_off + (long)i * a.F + f];
    const float be = a.params[a.be_off + f], psi = a.psi[f];
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
        if (f0 + ff < a.F) a.x[(long)(f0 + ff) * a.NP + l0 + ll] = tile[ff][ll];
    }
}

// Partials of Dense_0, laid out as the head reads them: part[rg][ct][k][l][s] = sum over the rows of group rg of
// x[l][f] W0[f][32 ct + 2 s + k]  (ct: tile of 32 hidden units, s < 16, k < 2, l < NP) -- lane (k, l) of the head's wave
// ct finds its 16 B-operand values of one group in 64 consecutive bytes.
struct IqnActDenseArgs {
    const float* x;       // [F][NP]
    const float* params;
    float* part;          // [NRG][J / 32][2][NP][16]
    long w_off;
    int F, J, NP, NRG;
};
// workgroup = (row group rg, tile ct of 32 hidden units) x 8 waves, each with 1 / 8 of the group's row pairs: one MFMA per
// row pair and fraction tile (A = two 128-byte pieces of W0 rows, B = two rows of x), 8 row pairs requested before their
// MFMAs run.  The 8 waves' tiles are added in wave order through LDS.  NRG x J / 32 workgroups of 8 waves keep
// 16 KB of W0 in flight each; NRG x NP x J floats of partials are left (see DESIGN 3.4 for the choice of NRG).
template <int MT>  // fraction tiles: NP = 32 MT
__global__ __launch_bounds__(512) void k_iqn_act_dense0(IqnActDenseArgs a) {
    __shared__ float sl[8][16][64];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, nct = a.J / 32;
    const int rg = blockIdx.x / nct, ct = blockIdx.x - rg * nct;
    const int FP = a.F / 2, slice = rg * 8 + wv, ns = a.NRG * 8;
    const int p0 = (int)((long)FP * slice / ns), p1 = (int)((long)FP * (slice + 1) / ns);
    const float* W = a.params + a.w_off + (long)(lane >> 5) * a.J + ct * 32 + (lane & 31);
    const float* X = a.x + (long)(lane >> 5) * a.NP + (lane & 31);
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    for (int p = p0; p < p1; p += 8) {
        float wr[8], xr[8][MT];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int pp = min(p + u, p1 - 1);
            wr[u] = W[(long)pp * 2 * a.J];
#pragma unroll
            for (int m = 0; m < MT; ++m) xr[u][m] = X[(long)pp * 2 * a.NP + 32 * m];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (p + u < p1) {
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = mfma32(wr[u], xr[u][m], acc[m]);
            }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (m) __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) sl[wv][r][lane] = acc[m][r];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2; ++it) {  // 2 (k) x 32 (l) x 16 (s) values of this fraction tile, in the order they are stored
            const int idx = t + 512 * it, s = idx & 15, lq = (idx >> 4) & 31, k = idx >> 9, jj = 2 * s + k;
            const int r = 4 * (jj >> 3) + (jj & 3), ln = 32 * ((jj >> 2) & 1) + lq;  // mfma_row(r, ln >> 5) == jj
            float v = sl[0][r][ln];
#pragma unroll
            for (int w2 = 1; w2 < 8; ++w2) v += sl[w2][r][ln];
            a.part[((((long)rg * nct + ct) * 2 + k) * a.NP + 32 * m + lq) * 16 + s] = v;
        }
    }
}

struct IqnActHeadArgs {
    const float* part;  // [NRG][J / 32][2][NP][16]
    const float* params;
    long b0_off, w1_off, b1_off;
    int NRG, J, A, N, NP;
    float* q_out;       // [A]
    int32_t* action;    // [1]
    volatile int32_t* mail;  // host mailbox {action, sequence} or nullptr -- as ActHeadArgs
    unsigned* seq;
};
// one workgroup of 16 waves; wave ct < J / 32 owns 32 hidden units: lane (k, l) sums the partials of h[l][32 ct + 2 s + k]
// over the groups in order, adds the bias, clamps, and feeds them as the B operand of Z^T[a][l] += W1^T[a][j] h^T[j][l]
// (A operand: Dense_1's rows as they lie, actions behind A are zero rows).  The waves' Z tiles are added in wave order
// through LDS (two rounds of 8), b1 joins, thread a sums its row over l = 0 .. N - 1 and divides by N.
template <int MT>
__global__ __launch_bounds__(1024) void k_iqn_act_head(IqnActHeadArgs a) {
    __shared__ float sl[8][16][64];
    __shared__ float zf[32][64];
    __shared__ float qs[32];
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, k = lane >> 5, lq = lane & 31, nct = a.J / 32;
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
        const long gstride = (long)nct * 2 * a.NP * 16;
        const float* P = a.part + (((long)wv * 2 + k) * a.NP + lq) * 16;
        constexpr int GU = 4 / MT;  // groups requested at once (16 float4 per lane), added in group order
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
            w1[s] = lq < a.A ? a.params[a.w1_off + (long)j * a.A + lq] : 0.f;
            b0[s] = a.params[a.b0_off + j];
        }
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma32(w1[s], fmaxf(hs[m][s] + b0[s], 0.f), acc[m]);
    }
    // thread (r, ln) = t of this round's fraction tile: Z^T[a = mfma_row(r, ln >> 5)][l = 32 m + (ln & 31)]
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
        zf[a_][32 * m + lq] = a_ < a.A ? z + a.params[a.b1_off + a_] : 0.f;
    }
    __syncthreads();
    if (t < a.A) {
        float q = 0.f;
        for (int l = 0; l < a.N; ++l) q += zf[t][l];
        q /= (float)a.N;
        qs[t] = q;
        a.q_out[t] = q;
    }
    __syncthreads();
    if (t == 0) {
        int best = 0;
        float bv = qs[0];
        for (int ac = 1; ac < a.A; ++ac)
            if (qs[ac] > bv) { bv = qs[ac]; best = ac; }
        a.action[0] = best;
        if (a.mail) {
            const unsigned n = a.seq[0] + 1u;
            a.seq[0] = n;
            a.mail[0] = best;
            __threadfence_system();  // the action is visible to the host before the number that announces it
            a.mail[1] = (int32_t)n;
        }
    }
}
