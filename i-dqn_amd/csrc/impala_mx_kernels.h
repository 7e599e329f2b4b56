// impala architecture: the 3x3 / stride 1 / SAME convolutions, forward and data gradient, on the bf16 matrix cores with
// f32-accurate products (IDQN_IMP_CONV=bf16x3; the eligibility rule and the tile constants are in imp_mx_args.h).
// Same tensors as k_imp_conv (impala_kernels.h): NHWC f32 activations [net][sample][h][w][c], HWIO leaves, ImpConvArgs.
//
// An implicit GEMM per image.  A workgroup (256 lanes) owns an IMX_TH x IMX_TW tile of output positions of ONE image and
// IMX_NB output channels; M = positions, N = output channels, K = 9 taps x CI.  Wave w owns tile rows 4 w .. 4 w + 3 as
// two M tiles of v_mfma_f32_32x32x16_bf16 (M tile m: rows 4 w + 2 m, 4 w + 2 m + 1; A row r = tile row r >> 4, column
// r & 15); both reuse one weight fragment.  An M tile never leaves its image: a state's result does not depend on the
// batch around it.
//
// Operand maps (lane l: r = l & 31, h = l >> 5): A[r][k = 8 h + j] = x(position r shifted by the tap, channel c0 + 8 h + j),
// B[k = 8 h + j][r] = w(tap, channel c0 + 8 h + j, output channel cob + r); the result has the output channel on the lane
// and positions (i & 3) + 8 (i >> 2) + 4 h in registers i = 0 .. 15, so one store writes 32 consecutive channels.
//
// LDS pass = IMX_KC input channels: the halo tile (18 x 18 positions) and the 9 x 16 x 32 weights are split into their three
// bf16 terms as they are staged (split3_pk, RELU_IN before the split) and laid out in fragment order, [term][h][position][8]
// and [term][tap][lane][8], so every fragment is one 16-byte LDS read.  The data gradient reads the mirrored, transposed
// leaf, as k_imp_conv does.
//
// Summation order, fixed (no atomics, no scratch; two launches on equal inputs give equal bytes):
//   pass p = channels 16 p .. 16 p + 15, ascending; inside a pass the taps (kh, kw) ascending; inside a tap the six partial
//   products smallest first -- x2 w0, x0 w2, x1 w1, x1 w0, x0 w1, x0 w0 (convp.h) -- each one MFMA (its 16 channels summed by
//   the matrix core).  The first five, at most 2^-8 of the product, chain into the pass's SMALL accumulator, x0 w0 into its
//   MAIN accumulator; both start at zero.  After the pass, total += (small + main).  The total starts at the bias (forward)
//   or zero (data gradient).  A blocked sum, as k_imp_conv's: an output takes 9 roundings at full magnitude per pass and two
//   per pass boundary (the 45 of the small chain are 2^-8 of that) -- not 9 CI, and not the 54 per pass of one chain for all
//   six products, whose error was 1.7 x this one's in the numpy restatement (the pool after Conv_0 is discontinuous --
//   DESIGN.md 3.6.1).
// Epilogue in registers: [* (mask > 0)] [+ aux] [relu], as k_imp_conv.
#pragma once
#include "convp.h"
#include "imp_mx_args.h"
#include "impala_kernels.h"

#define IMX_HW (IMX_TW + 2)                    // halo tile width
#define IMX_HALO ((IMX_TH + 2) * (IMX_TW + 2)) // halo tile positions (324)
#define IMX_XT (2 * IMX_HALO)                  // 16-byte fragments of one term of the halo tile
#define IMX_WT (9 * 64)                        // 16-byte fragments of one term of the weights

__device__ __forceinline__ void imx_split8(const float* v, u32x4& q0, u32x4& q1, u32x4& q2) {
    unsigned p0[4], p1[4], p2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) split3_pk(v[2 * m], v[2 * m + 1], p0[m], p1[m], p2[m]);
    q0 = (u32x4){p0[0], p0[1], p0[2], p0[3]};
    q1 = (u32x4){p1[0], p1[1], p1[2], p1[3]};
    q2 = (u32x4){p2[0], p2[1], p2[2], p2[3]};
}

// forward: out = [relu]( conv(in [relu'd on load]) + bias [+ aux] );  DGRAD: out = dgrad(in) [* (mask > 0)] [+ aux]
// needs a.CI % IMX_KC == 0 (imx_eligible); a.CO may end inside an N tile.  grid (tiles, N tiles, nets x samples)
template <bool RELU_IN, bool RELU_OUT, bool ADD, bool DGRAD, bool MASK>
__global__ __launch_bounds__(256, 2) void k_imp_conv_mx(ImpConvArgs a) {  // two workgroups per CU: LDS allows them, the registers must
    __shared__ u32x4 s_x[3 * IMX_XT];
    __shared__ u32x4 s_w[3 * IMX_WT];
    const int tiles_w = (a.W + IMX_TW - 1) / IMX_TW;
    const int h0 = (int)(blockIdx.x / tiles_w) * IMX_TH, w0 = (int)(blockIdx.x % tiles_w) * IMX_TW, cob = blockIdx.y * IMX_NB;
    const int net = blockIdx.z / a.B, b = blockIdx.z % a.B;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const float* P = a.wbase[net];
    const float* Wg = P + a.w_off;
    const float* img = a.in + ((long)net * a.B + b) * a.H * a.W * a.CI;
    const int co = cob + r;
    const float bias = (!DGRAD && co < a.CO) ? P[a.b_off + co] : 0.f;
    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] = bias;
    bool live[2];  // wave-uniform: an M tile below the frame is not computed
#pragma unroll
    for (int m = 0; m < 2; ++m) live[m] = h0 + 4 * wv + 2 * m < a.H;
    const int xpos = (4 * wv + (r >> 4)) * IMX_HW + (r & 15) + hh * IMX_HALO;  // this lane's fragment of M tile 0, tap (0, 0)
    for (int c0 = 0; c0 < a.CI; c0 += IMX_KC) {
        __syncthreads();  // the previous pass has been read
        for (int e = tid; e < IMX_XT; e += 256) {
            const int eh = e & 1, pos = e >> 1, col = pos % IMX_HW, row = pos / IMX_HW;
            const int ih = h0 - 1 + row, iw = w0 - 1 + col;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
                const float4* src = (const float4*)(img + ((long)ih * a.W + iw) * a.CI + c0 + 8 * eh);
                const float4 va = src[0], vb = src[1];
                v[0] = va.x; v[1] = va.y; v[2] = va.z; v[3] = va.w; v[4] = vb.x; v[5] = vb.y; v[6] = vb.z; v[7] = vb.w;
                if (RELU_IN)
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
            }
            const int at = eh * IMX_HALO + pos;
            imx_split8(v, s_x[at], s_x[IMX_XT + at], s_x[2 * IMX_XT + at]);
        }
        for (int e = tid; e < IMX_WT; e += 256) {  // fragment (tap, lane (co, h)): channels c0 + 8 h .. + 7
            const int el = e & 63, tap = e >> 6, cog = cob + (el & 31), ci = c0 + 8 * (el >> 5);
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (cog < a.CO) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v[j] = DGRAD ? Wg[((long)(8 - tap) * a.CO + cog) * a.CI + ci + j]  // leaf [3][3][CO][CI], taps mirrored
                                 : Wg[((long)tap * a.CI + ci + j) * a.CO + cog];
            }
            imx_split8(v, s_w[e], s_w[IMX_WT + e], s_w[2 * IMX_WT + e]);
        }
        __syncthreads();
        f32x16 ps[2], pm[2];  // the pass's small products (everything but x0 w0) and its main products (x0 w0)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) ps[m][i] = pm[m][i] = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tap = kh * 3 + kw;
                bf16x8 W[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) W[t] = __builtin_bit_cast(bf16x8, s_w[t * IMX_WT + tap * 64 + lane]);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    if (!live[m]) continue;
                    const int at = xpos + (2 * m + kh) * IMX_HW + kw;
                    bf16x8 A[3];
#pragma unroll
                    for (int t = 0; t < 3; ++t) A[t] = __builtin_bit_cast(bf16x8, s_x[t * IMX_XT + at]);
                    ps[m] = mfma_bf16(A[2], W[0], ps[m]);
                    ps[m] = mfma_bf16(A[0], W[2], ps[m]);
                    ps[m] = mfma_bf16(A[1], W[1], ps[m]);
                    ps[m] = mfma_bf16(A[1], W[0], ps[m]);
                    ps[m] = mfma_bf16(A[0], W[1], ps[m]);
                    pm[m] = mfma_bf16(A[0], W[0], pm[m]);
                }
            }
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m] += ps[m] + pm[m];
    }
    if (co >= a.CO) return;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (!live[m]) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
            const int oh = h0 + 4 * wv + 2 * m + (row >> 4), ow = w0 + (row & 15);
            if (oh >= a.H || ow >= a.W) continue;
            const long at = ((((long)net * a.B + b) * a.H + oh) * a.W + ow) * a.CO + co;
            float v = acc[m][i];
            if (MASK) v = a.mask[at] > 0.f ? v : 0.f;
            if (ADD) v += a.aux[at];
            if (RELU_OUT) v = fmaxf(v, 0.f);
            a.out[at] = v;
        }
    }
}
