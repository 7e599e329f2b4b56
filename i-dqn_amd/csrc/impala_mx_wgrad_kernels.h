// impala architecture: weight + bias gradient of the 3x3 / stride 1 / SAME convolutions on the bf16 matrix cores with
// f32-accurate products (IDQN_IMP_WGRAD=bf16x3; the plan and the tile constants are in imp_mx_wgrad_args.h, the eligibility
// rule is imx_eligible of imp_mx_args.h).  Same tensors and the same partial layout as k_imp_wgrad (impala_kernels.h,
// ImpWgradArgs): dW[kh][kw][ci][co] = sum_{b, oh, ow} x[b][oh + kh - 1][ow + kw - 1][ci] dy[b][oh][ow][co], db[co] = sum dy;
// one partial per (head, chunk) in part[K][n_chunks][9 CI CO + CO], which the unchanged k_imp_wreduce adds in chunk order.
//
// A GEMM per tap: M = input channels, N = output channels, K = positions.  A workgroup (256 lanes) owns one chunk of
// IMXW_TILES tiles (IMXW_TH x IMXW_TW output positions of one image each), IMXW_MB input and IMXW_NB output channels; a
// k-step of v_mfma_f32_32x32x16_bf16 is one tile row (16 consecutive columns).  The 32x32x16 shape is the one whose maps
// the forward kernel already uses and needs half the LDS bytes per product of 16x16x32; a 16-channel leaf fills half an M tile.
//
// Operand maps (lane l: r = l & 31, h = l >> 5): A[r][k = 8 h + j] = x(channel c0 + r, row oh + kh - 1, column w0 + 8 h + j
// + kw - 1), B[k = 8 h + j][r] = dy(row oh, column w0 + 8 h + j, output channel cob + r); the result has the output channel on
// the lane and input channels (i & 3) + 8 (i >> 2) + 4 h in registers i = 0 .. 15, so one store writes 32 consecutive leaf
// elements.
//
// The tap shift on the K axis: both operands are transposed to [channel][row][column] bf16 as they are staged, split into
// their three terms (split3_pk, RELU_IN before the split; nothing is split ahead of the launch).  dy is staged once per
// tile; of x's halo tile (IMXW_TH + 2 rows, 18 columns) THREE copies are staged, [kw][term][channel][row][16], copy kw
// holding halo columns kw .. kw + 15, so the fragment of tap (kh, kw) is row + kh of copy kw: every fragment of either
// operand is one aligned 16-byte LDS read and the inner loop is reads and MFMAs only.  (Reading one copy and funnel-shifting
// in registers would save two thirds of x's LDS but puts eight VALU shifts and a second read per fragment between the
// MFMAs.)  A staging lane packs two neighbouring columns into a dword; copy 1, whose pairs start on odd columns, takes a second
// split of (column + 1, column + 2).  The channel pitches (84 and 68 dwords) put 16 lanes' 16-byte reads on all 64 banks.
//
// The nine taps are dealt to the four waves (tap g = wave + 4 u: three, two, two, two), so every wave owns whole outputs and
// no sum crosses waves.
//
// Summation order, fixed by the plan alone (no atomics, no scratch; two launches on equal inputs give equal bytes):
//   an output element's chunk partial runs over the chunk's tiles ascending (image major, tile row, tile column), inside a
//   tile over its rows ascending; a row is six MFMAs (each sums its 16 columns in the matrix core), the partial products
//   smallest first -- x2 dy0, x0 dy2, x1 dy1, x1 dy0, x0 dy1, x0 dy0 (convp.h).  The first five, at most 2^-8 of the product,
//   chain into the chunk's SMALL accumulator, x0 dy0 into its MAIN accumulator; both start at zero and the partial is
//   small + main.  The chunk is the block of the blocked sum: a main chain is at most IMXW_TILES x IMXW_TH = 64 roundings
//   long whatever the batch, and k_imp_wreduce adds the chunks in order.
//   Bias: staging lane j = tid >> 5 (output channel tid & 31) adds, in f32, the two columns 2 j, 2 j + 1 of every row it
//   stages, column 2 j first, rows ascending, tiles ascending; the eight lanes of a channel are then added j ascending.
#pragma once
#include "convp.h"
#include "imp_mx_wgrad_args.h"
#include "impala_kernels.h"

#define IMXW_XP ((IMXW_TH + 2) * 8 + 4)  // dwords of one (copy, term, channel) of x: 10 rows x 16 bf16, + 16 bytes
#define IMXW_DP (IMXW_TH * 8 + 4)        // dwords of one (term, channel) of dy

// grid (chunk, M block x N block, head); needs a.CI % 16 == 0 and a.CO % 32 == 0 (imx_eligible)
template <bool RELU_IN>
__global__ __launch_bounds__(256) void k_imp_wgrad_mx(ImpWgradArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned s_x[9 * IMXW_MB * IMXW_XP];   // [kw][term][channel][row][8]
    __shared__ __attribute__((aligned(16))) unsigned s_dy[3 * IMXW_NB * IMXW_DP];  // [term][channel][row][8]; later the bias sums
    const int n_nb = (a.CO + IMXW_NB - 1) / IMXW_NB;
    const int c0 = (int)(blockIdx.y / n_nb) * IMXW_MB, cob = (int)(blockIdx.y % n_nb) * IMXW_NB, k = blockIdx.z;
    const int tiles_w = (a.W + IMXW_TW - 1) / IMXW_TW, tiles_h = (a.H + IMXW_TH - 1) / IMXW_TH, per_img = tiles_w * tiles_h;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    f32x16 ps[3], pm[3];  // tap wv + 4 u: the small products and x0 dy0
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) ps[u][i] = pm[u][i] = 0.f;
    float bsum = 0.f;
    const int t_end = min((int)(blockIdx.x + 1) * IMXW_TILES, a.n_tiles);
    for (int t = blockIdx.x * IMXW_TILES; t < t_end; ++t) {
        const int b = t / per_img, ti = t % per_img, h0 = (ti / tiles_w) * IMXW_TH, w0 = (ti % tiles_w) * IMXW_TW;
        const float* img = a.in + ((long)k * a.B + b) * a.H * a.W * a.CI;
        const float* dyi = a.dy + ((long)k * a.B + b) * a.H * a.W * a.CO;
        __syncthreads();  // the previous tile has been read
        for (int e = tid; e < IMXW_MB * (IMXW_TH + 2) * 9; e += 256) {  // channel, halo row, halo columns 2 cp, 2 cp + 1 (, 2 cp + 2)
            const int ci = e & (IMXW_MB - 1), pr = e / IMXW_MB, cp = pr % 9, row = pr / 9;
            const int ih = h0 - 1 + row, iw = w0 - 1 + 2 * cp;
            float v[3] = {0.f, 0.f, 0.f};
            if (ih >= 0 && ih < a.H && c0 + ci < a.CI) {
                const float* src = img + (long)ih * a.W * a.CI + c0 + ci;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (iw + j >= 0 && iw + j < a.W) v[j] = RELU_IN ? fmaxf(src[(long)(iw + j) * a.CI], 0.f) : src[(long)(iw + j) * a.CI];
            }
            unsigned p[3], q[3];
            split3_pk(v[0], v[1], p[0], p[1], p[2]);
            split3_pk(v[1], v[2], q[0], q[1], q[2]);
            const int at = ci * IMXW_XP + row * 8 + cp;
#pragma unroll
            for (int tm = 0; tm < 3; ++tm) {
                if (cp < 8) {
                    s_x[(0 * 3 + tm) * IMXW_MB * IMXW_XP + at] = p[tm];
                    s_x[(1 * 3 + tm) * IMXW_MB * IMXW_XP + at] = q[tm];
                }
                if (cp > 0) s_x[(2 * 3 + tm) * IMXW_MB * IMXW_XP + at - 1] = p[tm];
            }
        }
        for (int e = tid; e < IMXW_NB * IMXW_TH * 8; e += 256) {  // channel, row, columns 2 cp, 2 cp + 1
            const int co = e & (IMXW_NB - 1), pr = e / IMXW_NB, cp = pr & 7, row = pr >> 3;
            const int oh = h0 + row, ow = w0 + 2 * cp;
            float d0 = 0.f, d1 = 0.f;
            if (oh < a.H && cob + co < a.CO) {
                const float* src = dyi + (long)oh * a.W * a.CO + cob + co;
                if (ow < a.W) d0 = src[(long)ow * a.CO];
                if (ow + 1 < a.W) d1 = src[(long)(ow + 1) * a.CO];
            }
            bsum += d0;
            bsum += d1;
            unsigned p[3];
            split3_pk(d0, d1, p[0], p[1], p[2]);
#pragma unroll
            for (int tm = 0; tm < 3; ++tm) s_dy[(tm * IMXW_NB + co) * IMXW_DP + row * 8 + cp] = p[tm];
        }
        __syncthreads();
        const int rows = min(IMXW_TH, a.H - h0);
        for (int row = 0; row < rows; ++row) {
            bf16x8 D[3];
#pragma unroll
            for (int tm = 0; tm < 3; ++tm) D[tm] = __builtin_bit_cast(bf16x8, *(const u32x4*)(s_dy + (tm * IMXW_NB + r) * IMXW_DP + row * 8 + 4 * hh));
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int g = wv + 4 * u;
                if (g >= 9) continue;  // wave-uniform
                const int kh = g / 3, kw = g % 3;
                bf16x8 X[3];
#pragma unroll
                for (int tm = 0; tm < 3; ++tm)
                    X[tm] = __builtin_bit_cast(bf16x8, *(const u32x4*)(s_x + ((kw * 3 + tm) * IMXW_MB + r) * IMXW_XP + (row + kh) * 8 + 4 * hh));
                ps[u] = mfma_bf16(X[2], D[0], ps[u]);
                ps[u] = mfma_bf16(X[0], D[2], ps[u]);
                ps[u] = mfma_bf16(X[1], D[1], ps[u]);
                ps[u] = mfma_bf16(X[1], D[0], ps[u]);
                ps[u] = mfma_bf16(X[0], D[1], ps[u]);
                pm[u] = mfma_bf16(X[0], D[0], pm[u]);
            }
        }
    }
    const long nw = 9L * a.CI * a.CO;
    float* part = a.part + ((long)k * a.n_chunks + blockIdx.x) * (nw + a.CO);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int g = wv + 4 * u;
        if (g >= 9 || cob + r >= a.CO) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ci = c0 + mfma_row(i, hh);
            if (ci < a.CI) part[((long)g * a.CI + ci) * a.CO + cob + r] = ps[u][i] + pm[u][i];
        }
    }
    float* s_b = (float*)s_dy;
    __syncthreads();  // the last tile has been read
    s_b[tid] = bsum;
    __syncthreads();
    if (c0 == 0 && tid < IMXW_NB && cob + tid < a.CO) {
        float s = s_b[tid];
        for (int j = 1; j < 8; ++j) s += s_b[tid + IMXW_NB * j];
        part[nw + cob + tid] = s;
    }
}
