// impala architecture (slimdqn/networks/architectures/dqn.py:7-29,54-60): f32 HIP kernels of the three residual Stacks.
// Fixed to this geometry -- 3x3 convs, stride 1, SAME (pad 1 / 1); max-pool 3x3, stride 2, SAME with -inf padding -- and
// written for any channel count >= 1.  NHWC f32 activations [net][sample][h][w][c], HWIO kernels as the leaves hold them;
// the dense head runs on k_fc_step (fc_kernels.h); its first layer, when a hidden layer exists, on the k_imp_d0_* kernels below.
//
// A conv workgroup (256 lanes) owns an IMP_TH x IMP_TW tile of output positions of ONE image and IMP_COB output channels:
// it stages the input tile with its one-pixel halo, IMP_CIC (or 4) input channels at a time, and the matching 9 x CIC x 32
// weights in LDS; a lane keeps two vertically adjacent positions x IMP_CB channels in registers (wave w = channels 8 w ..),
// sums each pass in accumulators of its own and adds them to the total (a blocked sum: the pool after Conv_0 is discontinuous).
// The data gradient is the same kernel on the flipped, transposed weights (DGRAD), with the ReLU mask of the forward
// tensor and the `+ skip` of the residual in its epilogue.  The weight gradient keeps 9 taps x 4 output channels per lane,
// walks IMP_WG_TILES tiles per workgroup (one chunk), sums its four waves through LDS in wave order and leaves one partial
// per chunk; k_imp_wreduce adds the partials in chunk order.  No sum here depends on scheduling: there are no atomics.
#pragma once
#include "common.h"

#define IMP_TH 8                      // tile height (output rows)
#define IMP_TW 16                     // tile width
#define IMP_ROWP 24                   // LDS row pitch of the halo tile (18 columns used; 2 rows apart = 48 banks)
#define IMP_CHP ((IMP_TH + 2) * IMP_ROWP + 4)  // LDS channel pitch (244: eight channels on eight different banks)
#define IMP_CB 8                      // output channels a lane holds
#define IMP_COB 32                    // output channels of a workgroup (4 waves x IMP_CB)
#define IMP_CIC 8                     // input channels per LDS pass
#define IMP_WG_TILES 16               // tiles per weight-gradient chunk

enum { IMP_SRC_F32 = 0, IMP_SRC_U8 = 1 };

// the halo tile rows h0 - 1 .. h0 + IMP_TH, columns w0 - 1 .. w0 + IMP_TW, channels c0 .. c0 + CIC of one image -> LDS
// [c][row][col]; zero outside the image and past channel C
template <int SRC, bool RELU, int CIC>
__device__ __forceinline__ void imp_stage_tile(float* lds, const void* img, int H, int W, int C, int h0, int w0, int c0) {
    constexpr int TWH = IMP_TW + 2, THH = IMP_TH + 2;
    for (int e = threadIdx.x; e < THH * TWH * CIC; e += 256) {
        const int c = e % CIC, p = e / CIC, col = p % TWH, row = p / TWH;
        const int ih = h0 - 1 + row, iw = w0 - 1 + col, ci = c0 + c;
        float v = 0.f;
        if (ih >= 0 && ih < H && iw >= 0 && iw < W && ci < C) {
            const long idx = ((long)ih * W + iw) * C + ci;
            if (SRC == IMP_SRC_U8) v = (float)((const uint8_t*)img)[idx] / 255.0f;  // architectures/dqn.py:56
            else v = ((const float*)img)[idx];
            if (RELU) v = fmaxf(v, 0.f);
        }
        lds[c * IMP_CHP + row * IMP_ROWP + col] = v;
    }
}

struct ImpConvArgs {
    const uint8_t* in_u8[2];    // SRC_U8: the two uint8 minibatches [B][H][W][CI]; nets < n_split read [0]
    const float* in;            // [n_nets][B][H][W][CI]
    float* out;                 // [n_nets][B][H][W][CO]
    const float* aux;           // forward: the residual; DGRAD: the skip gradient (may alias out).  [n_nets][B][H][W][CO]
    const float* mask;          // DGRAD + MASK: the forward tensor whose sign masks the result, [n_nets][B][H][W][CO]
    const float* const* wbase;  // [n_nets]
    long w_off, b_off;
    int n_nets, n_split, B, H, W, CI, CO;  // channels of THIS pass (DGRAD: CI = the leaf's output channels, CO = its input channels)
};

// forward: out = [relu]( conv(in [relu'd on load]) + bias [+ aux] );  DGRAD: out = dgrad(in) [* (mask > 0)] [+ aux]
// PER_NET_U8 (SRC_U8 with B = 1, imp_act_many_kernels.h): net e reads image e of in_u8[0], not the minibatch all nets share
template <int SRC, bool RELU_IN, bool RELU_OUT, bool ADD, bool DGRAD, bool MASK, int CIC, bool PER_NET_U8 = false>
__global__ __launch_bounds__(256) void k_imp_conv(ImpConvArgs a) {
    __shared__ float s_in[CIC * IMP_CHP];
    __shared__ __attribute__((aligned(16))) float s_w[CIC * 9 * IMP_COB];
    const int tiles_w = (a.W + IMP_TW - 1) / IMP_TW;
    const int h0 = (int)(blockIdx.x / tiles_w) * IMP_TH, w0 = (int)(blockIdx.x % tiles_w) * IMP_TW, cob = blockIdx.y * IMP_COB;
    const int net = blockIdx.z / a.B, b = blockIdx.z % a.B;
    const int tid = threadIdx.x, cg = tid >> 6, p = tid & 63, tx = p & 15, ty = (p >> 4) * 2;
    const float* P = a.wbase[net];
    const float* Wg = P + a.w_off;
    const long img_elems = (long)a.H * a.W * a.CI;
    const void* img = SRC == IMP_SRC_U8 ? (PER_NET_U8 ? (const void*)(a.in_u8[0] + (long)net * img_elems)
                                                      : (const void*)(a.in_u8[net < a.n_split ? 0 : 1] + (long)b * img_elems))
                                        : (const void*)(a.in + ((long)net * a.B + b) * img_elems);
    float acc[2][IMP_CB];
#pragma unroll
    for (int j = 0; j < IMP_CB; ++j) {
        const int co = cob + cg * IMP_CB + j;
        acc[0][j] = acc[1][j] = (!DGRAD && co < a.CO) ? P[a.b_off + co] : 0.f;
    }
    for (int c0 = 0; c0 < a.CI; c0 += CIC) {
        __syncthreads();  // the previous pass has been read
        imp_stage_tile<SRC, RELU_IN, CIC>(s_in, img, a.H, a.W, a.CI, h0, w0, c0);
        for (int e = tid; e < CIC * 9 * IMP_COB; e += 256) {  // s_w[c][tap][co]
            const int co = e % IMP_COB, r = e / IMP_COB, tap = r % 9, ci = c0 + r / 9, cog = cob + co;
            float v = 0.f;
            if (ci < a.CI && cog < a.CO)
                v = DGRAD ? Wg[((long)(8 - tap) * a.CO + cog) * a.CI + ci]  // leaf [3][3][CO][CI], taps mirrored
                          : Wg[((long)tap * a.CI + ci) * a.CO + cog];
            s_w[e] = v;
        }
        __syncthreads();
        // a pass sums its CIC x 9 products on their own and is then added to the total: the rounding error of a long
        // channel sum grows with CI / CIC + 9 CIC terms, not with 9 CI as one running fma chain's does
        float pa[2][IMP_CB];
#pragma unroll
        for (int j = 0; j < IMP_CB; ++j) pa[0][j] = pa[1][j] = 0.f;
#pragma unroll
        for (int c = 0; c < CIC; ++c) {
            float x[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) x[r][k] = s_in[c * IMP_CHP + (ty + r) * IMP_ROWP + tx + k];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float4* wp = (const float4*)(s_w + (c * 9 + kh * 3 + kw) * IMP_COB + cg * IMP_CB);
                    const float4 wa = wp[0], wb = wp[1];
                    const float w[IMP_CB] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                    for (int j = 0; j < IMP_CB; ++j) {
                        pa[0][j] = fmaf(x[kh][kw], w[j], pa[0][j]);
                        pa[1][j] = fmaf(x[kh + 1][kw], w[j], pa[1][j]);
                    }
                }
        }
#pragma unroll
        for (int j = 0; j < IMP_CB; ++j) {
            acc[0][j] += pa[0][j];
            acc[1][j] += pa[1][j];
        }
    }
    const int ow = w0 + tx;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oh = h0 + ty + r;
        if (oh >= a.H || ow >= a.W) continue;
        const long base = ((((long)net * a.B + b) * a.H + oh) * a.W + ow) * a.CO;
#pragma unroll
        for (int j = 0; j < IMP_CB; ++j) {
            const int co = cob + cg * IMP_CB + j;
            if (co >= a.CO) continue;
            float v = acc[r][j];
            if (MASK) v = a.mask[base + co] > 0.f ? v : 0.f;
            if (ADD) v += a.aux[base + co];
            if (RELU_OUT) v = fmaxf(v, 0.f);
            a.out[base + co] = v;
        }
    }
}

// ---- max-pool 3x3 / 2, SAME ------------------------------------------------------------------------------------------
struct ImpPoolArgs {
    const float* c0;  // [N][H][W][C]   the pool's input (Conv_0's output)
    float* out;       // forward: [N][PH][PW][C]
    const float* dy;  // backward: [N][PH][PW][C]
    float* dx;        // backward: [N][H][W][C]
    long N;           // images (nets x samples)
    int H, W, C, PH, PW, lo_h, lo_w;
};

__global__ __launch_bounds__(256) void k_imp_pool_fwd(ImpPoolArgs a) {
    const long n = a.N * a.PH * a.PW * a.C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        long r = e;
        const int c = (int)(r % a.C); r /= a.C;
        const int pw = (int)(r % a.PW); r /= a.PW;
        const int ph = (int)(r % a.PH);
        const long img = r / a.PH;
        const float* src = a.c0 + img * a.H * a.W * a.C + c;
        float m = -INFINITY;
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = ph * 2 - a.lo_h + kh;
            if (ih < 0 || ih >= a.H) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int iw = pw * 2 - a.lo_w + kw;
                if (iw < 0 || iw >= a.W) continue;
                m = fmaxf(m, src[((long)ih * a.W + iw) * a.C]);
            }
        }
        a.out[e] = m;
    }
}

// A gather: every input element adds the gradients of the (at most four) windows whose maximum it is, windows in
// (row, column) order.  The maximum of a window is its FIRST largest element in (row, column) order (torch's CPU
// max_pool2d backward); padding is never selected.  The argmax is recomputed from c0.
__global__ __launch_bounds__(256) void k_imp_pool_bwd(ImpPoolArgs a) {
    const long n = a.N * a.H * a.W * a.C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        long r = e;
        const int c = (int)(r % a.C); r /= a.C;
        const int iw = (int)(r % a.W); r /= a.W;
        const int ih = (int)(r % a.H);
        const long img = r / a.H;
        const float* src = a.c0 + img * a.H * a.W * a.C + c;
        const float* dy = a.dy + img * a.PH * a.PW * a.C + c;
        // windows that contain (ih, iw): 2 p - lo <= i <= 2 p - lo + 2
        const int th = ih + a.lo_h, tw = iw + a.lo_w;
        const int ph0 = th >= 2 ? (th - 1) / 2 : 0, ph1 = min(th / 2, a.PH - 1);
        const int pw0 = tw >= 2 ? (tw - 1) / 2 : 0, pw1 = min(tw / 2, a.PW - 1);
        float s = 0.f;
        for (int ph = ph0; ph <= ph1; ++ph)
            for (int pw = pw0; pw <= pw1; ++pw) {
                float best = 0.f;
                int bh = -1, bw = -1;
                for (int kh = 0; kh < 3; ++kh) {
                    const int jh = ph * 2 - a.lo_h + kh;
                    if (jh < 0 || jh >= a.H) continue;
                    for (int kw = 0; kw < 3; ++kw) {
                        const int jw = pw * 2 - a.lo_w + kw;
                        if (jw < 0 || jw >= a.W) continue;
                        const float v = src[((long)jh * a.W + jw) * a.C];
                        if (bh < 0 || v > best) { best = v; bh = jh; bw = jw; }
                    }
                }
                if (bh == ih && bw == iw) s += dy[((long)ph * a.PW + pw) * a.C];
            }
        a.dx[e] = s;
    }
}

// ---- weight + bias gradient ------------------------------------------------------------------------------------------
struct ImpWgradArgs {
    const uint8_t* in_u8;  // SRC_U8: the state minibatch [B][H][W][CI] (every head reads it)
    const float* in;       // [K][B][H][W][CI]  the conv's forward input
    const float* dy;       // [K][B][H][W][CO]  gradient of the conv's output
    float* part;           // [K][n_chunks][9 CI CO + CO]
    int B, H, W, CI, CO, n_chunks, n_tiles;  // n_tiles = B * tiles per image
};

// grid (chunk, ci block x co block, head).  Lane: wave = two rows of the tile, ci = lane / 8, four output channels.
template <int SRC, bool RELU_IN>
__global__ __launch_bounds__(256) void k_imp_wgrad(ImpWgradArgs a) {
    __shared__ float s_in[IMP_CIC * IMP_CHP];
    __shared__ __attribute__((aligned(16))) float s_dy[IMP_TH * IMP_TW * IMP_COB];  // later: the wave sums [9][8][32] + bias [32]
    const int n_cob = (a.CO + IMP_COB - 1) / IMP_COB;
    const int cib = blockIdx.y / n_cob, c0 = cib * IMP_CIC, cob = (int)(blockIdx.y % n_cob) * IMP_COB, k = blockIdx.z;
    const int tiles_w = (a.W + IMP_TW - 1) / IMP_TW, tiles_h = (a.H + IMP_TH - 1) / IMP_TH, per_img = tiles_w * tiles_h;
    const int tid = threadIdx.x, pg = tid >> 6, lane = tid & 63, cq = lane & 7, ci = lane >> 3;
    float acc[9][4], bacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = 0.f;
    const int t_end = min((int)(blockIdx.x + 1) * IMP_WG_TILES, a.n_tiles);
    for (int t = blockIdx.x * IMP_WG_TILES; t < t_end; ++t) {
        const int b = t / per_img, ti = t % per_img, h0 = (ti / tiles_w) * IMP_TH, w0 = (ti % tiles_w) * IMP_TW;
        const void* img = SRC == IMP_SRC_U8 ? (const void*)(a.in_u8 + (long)b * a.H * a.W * a.CI)
                                            : (const void*)(a.in + ((long)k * a.B + b) * a.H * a.W * a.CI);
        const float* dyi = a.dy + ((long)k * a.B + b) * a.H * a.W * a.CO;
        __syncthreads();  // the previous tile has been read
        imp_stage_tile<SRC, RELU_IN, IMP_CIC>(s_in, img, a.H, a.W, a.CI, h0, w0, c0);
        for (int e = tid; e < IMP_TH * IMP_TW * IMP_COB; e += 256) {
            const int co = e % IMP_COB, pos = e / IMP_COB, oh = h0 + pos / IMP_TW, ow = w0 + pos % IMP_TW;
            s_dy[e] = (oh < a.H && ow < a.W && cob + co < a.CO) ? dyi[((long)oh * a.W + ow) * a.CO + cob + co] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int i = 0; i < 2 * IMP_TW; ++i) {
            const int r = pg * 2 + i / IMP_TW, cc = i % IMP_TW;
            const float4 d4 = *(const float4*)(s_dy + (r * IMP_TW + cc) * IMP_COB + cq * 4);
            const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float x = s_in[ci * IMP_CHP + (r + kh) * IMP_ROWP + cc + kw];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[kh * 3 + kw][j] = fmaf(x, d[j], acc[kh * 3 + kw][j]);
                }
#pragma unroll
            for (int j = 0; j < 4; ++j) bacc[j] += d[j];
        }
    }
    // the four waves' sums, in wave order
    float* s_red = s_dy;
    float* s_b = s_dy + 9 * IMP_CIC * IMP_COB;
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (pg == w) {
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float* q = s_red + (t * IMP_CIC + ci) * IMP_COB + cq * 4 + j;
                    *q = w == 0 ? acc[t][j] : *q + acc[t][j];
                }
            if (ci == 0)
#pragma unroll
                for (int j = 0; j < 4; ++j) s_b[cq * 4 + j] = w == 0 ? bacc[j] : s_b[cq * 4 + j] + bacc[j];
        }
    }
    __syncthreads();
    const long nw = 9L * a.CI * a.CO;
    float* part = a.part + ((long)k * a.n_chunks + blockIdx.x) * (nw + a.CO);
    for (int e = tid; e < 9 * IMP_CIC * IMP_COB; e += 256) {
        const int co = e % IMP_COB, c = (e / IMP_COB) % IMP_CIC, t = e / (IMP_COB * IMP_CIC);
        if (c0 + c < a.CI && cob + co < a.CO) part[((long)t * a.CI + c0 + c) * a.CO + cob + co] = s_red[e];
    }
    if (cib == 0 && tid < IMP_COB && cob + tid < a.CO) part[nw + cob + tid] = s_b[tid];
}

struct ImpWreduceArgs {
    const float* part;  // [K][n_chunks][nw + CO]
    float* grad;
    GradMap gm;
    long w_off, b_off, nw;
    int CO, n_chunks;
};

// the chunks' partials, added in chunk order, into the gradient arena.  grid (elements / 256, head)
__global__ __launch_bounds__(256) void k_imp_wreduce(ImpWreduceArgs a) {
    const int k = blockIdx.y;
    const long n = a.nw + a.CO;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const float* p = a.part + (long)k * a.n_chunks * n + e;
        float s = p[0];
        for (int c = 1; c < a.n_chunks; ++c) s += p[(long)c * n];
        a.grad[a.gm.at(k, e < a.nw ? a.w_off + e : a.b_off + (e - a.nw))] = s;
    }
}

// ---- Dense_0 of the head, spread over the chip ---------------------------------------------------------------------------
// The head's first layer reads the flattened Stack-2 output (F = PH PW C features, 7744 at the workload's widths) into D
// hidden units: one workgroup per head (k_fc_step) cannot stream it.  Three kernels take that layer; k_fc_step keeps the
// layers behind it and hands back dL/d(pre-activation) of the hidden units.  Every sum runs in a fixed order: the forward
// and the data gradient add blocks of IMP_D0_IC products, the weight gradient adds the samples in order.
#define IMP_D0_IC 64    // input features (forward) / hidden units (data gradient) per LDS pass
#define IMP_D0_OC 64    // hidden units a forward / weight-gradient workgroup owns
#define IMP_D0_SB 32    // samples per block
#define IMP_D0_XP 36    // LDS pitch of a [feature][sample] tile (float4 reads stay aligned)
#define IMP_D0_R 32     // input features a weight-gradient / data-gradient workgroup owns

struct ImpD0Args {
    const float* x;             // [n_nets][B][F]  the head's input (ReLU outputs)
    float* hid;                 // forward out: [n_nets][B][D] = relu(x W + b)
    const float* dh;            // [K][B][D]  dL/d(pre-activation)
    float* din;                 // data gradient out: [K][B][F], masked by x > 0
    const float* const* wbase;  // [n_nets]
    float* grad;
    GradMap gm;
    long w_off, b_off;
    int B, F, D;
};

// grid (D / 64, sample blocks, nets).  Lane: hidden unit = lane of the wave, eight samples = the wave's index.
__global__ __launch_bounds__(256) void k_imp_d0_fwd(ImpD0Args a) {
    __shared__ __attribute__((aligned(16))) float xs[IMP_D0_IC * IMP_D0_XP];
    const int tid = threadIdx.x, o = blockIdx.x * IMP_D0_OC + (tid & 63), sg = tid >> 6, b0 = blockIdx.y * IMP_D0_SB, net = blockIdx.z;
    const float* P = a.wbase[net];
    const float* W = P + a.w_off;
    const float* x = a.x + (long)net * a.B * a.F;
    const bool live = o < a.D;
    float acc[8];
    const float bias = live ? P[a.b_off + o] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bias;
    for (int i0 = 0; i0 < a.F; i0 += IMP_D0_IC) {
        __syncthreads();
        for (int e = tid; e < IMP_D0_SB * IMP_D0_IC; e += 256) {
            const int il = e % IMP_D0_IC, bl = e / IMP_D0_IC;
            xs[il * IMP_D0_XP + bl] = (b0 + bl < a.B && i0 + il < a.F) ? x[(long)(b0 + bl) * a.F + i0 + il] : 0.f;
        }
        __syncthreads();
        float pa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int n = min(IMP_D0_IC, a.F - i0);
        if (live)
            for (int il = 0; il < n; ++il) {
                const float w = W[(long)(i0 + il) * a.D + o];
                const float4 xa = *(const float4*)(xs + il * IMP_D0_XP + sg * 8), xb = *(const float4*)(xs + il * IMP_D0_XP + sg * 8 + 4);
                pa[0] = fmaf(xa.x, w, pa[0]); pa[1] = fmaf(xa.y, w, pa[1]); pa[2] = fmaf(xa.z, w, pa[2]); pa[3] = fmaf(xa.w, w, pa[3]);
                pa[4] = fmaf(xb.x, w, pa[4]); pa[5] = fmaf(xb.y, w, pa[5]); pa[6] = fmaf(xb.z, w, pa[6]); pa[7] = fmaf(xb.w, w, pa[7]);
            }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += pa[j];
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = b0 + sg * 8 + j;
        if (b < a.B) a.hid[((long)net * a.B + b) * a.D + o] = fmaxf(acc[j], 0.f);
    }
}

// gW[i][o] = sum_b x[b][i] dh[b][o], gb[o] = sum_b dh[b][o], samples in order.  grid (F / 32, D / 64, head).
// Lane: hidden unit = lane of the wave, eight input features = the wave's index.
__global__ __launch_bounds__(256) void k_imp_d0_wgrad(ImpD0Args a) {
    __shared__ __attribute__((aligned(16))) float xs[IMP_D0_SB * IMP_D0_XP];  // [sample][feature]
    __shared__ float ds[IMP_D0_SB * IMP_D0_OC];                               // [sample][unit]
    const int tid = threadIdx.x, ol = tid & 63, rg = tid >> 6, i0 = blockIdx.x * IMP_D0_R, o0 = blockIdx.y * IMP_D0_OC, k = blockIdx.z;
    const float* x = a.x + (long)k * a.B * a.F;
    const float* dh = a.dh + (long)k * a.B * a.D;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bacc = 0.f;
    for (int b0 = 0; b0 < a.B; b0 += IMP_D0_SB) {
        __syncthreads();
        for (int e = tid; e < IMP_D0_SB * IMP_D0_R; e += 256) {
            const int il = e % IMP_D0_R, bl = e / IMP_D0_R;
            xs[bl * IMP_D0_XP + il] = (b0 + bl < a.B && i0 + il < a.F) ? x[(long)(b0 + bl) * a.F + i0 + il] : 0.f;
        }
        for (int e = tid; e < IMP_D0_SB * IMP_D0_OC; e += 256) {
            const int oo = e % IMP_D0_OC, bl = e / IMP_D0_OC;
            ds[e] = (b0 + bl < a.B && o0 + oo < a.D) ? dh[(long)(b0 + bl) * a.D + o0 + oo] : 0.f;
        }
        __syncthreads();
        const int nb = min(IMP_D0_SB, a.B - b0);
        for (int bl = 0; bl < nb; ++bl) {
            const float d = ds[bl * IMP_D0_OC + ol];
            const float4 xa = *(const float4*)(xs + bl * IMP_D0_XP + rg * 8), xb = *(const float4*)(xs + bl * IMP_D0_XP + rg * 8 + 4);
            acc[0] = fmaf(xa.x, d, acc[0]); acc[1] = fmaf(xa.y, d, acc[1]); acc[2] = fmaf(xa.z, d, acc[2]); acc[3] = fmaf(xa.w, d, acc[3]);
            acc[4] = fmaf(xb.x, d, acc[4]); acc[5] = fmaf(xb.y, d, acc[5]); acc[6] = fmaf(xb.z, d, acc[6]); acc[7] = fmaf(xb.w, d, acc[7]);
            bacc += d;
        }
    }
    const int o = o0 + ol;
    if (o >= a.D) return;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = i0 + rg * 8 + j;
        if (i < a.F) a.grad[a.gm.at(k, a.w_off + (long)i * a.D + o)] = acc[j];
    }
    if (blockIdx.x == 0 && rg == 0) a.grad[a.gm.at(k, a.b_off + o)] = bacc;
}

// din[b][i] = [x[b][i] > 0] sum_o dh[b][o] W[i][o].  grid (F / 32, sample blocks, head).
// Lane: input feature = lane % 32, four samples = lane / 32.
__global__ __launch_bounds__(256) void k_imp_d0_dgrad(ImpD0Args a) {
    __shared__ float ws[IMP_D0_R * (IMP_D0_IC + 1)];                          // [feature][unit], odd pitch
    __shared__ __attribute__((aligned(16))) float ds[IMP_D0_IC * IMP_D0_XP];  // [unit][sample]
    const int tid = threadIdx.x, il = tid & 31, sg = tid >> 5, i0 = blockIdx.x * IMP_D0_R, b0 = blockIdx.y * IMP_D0_SB, k = blockIdx.z;
    const float* W = a.wbase[k] + a.w_off;
    const float* dh = a.dh + (long)k * a.B * a.D;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int o0 = 0; o0 < a.D; o0 += IMP_D0_IC) {
        __syncthreads();
        for (int e = tid; e < IMP_D0_R * IMP_D0_IC; e += 256) {
            const int oo = e % IMP_D0_IC, r = e / IMP_D0_IC;
            ws[r * (IMP_D0_IC + 1) + oo] = (i0 + r < a.F && o0 + oo < a.D) ? W[(long)(i0 + r) * a.D + o0 + oo] : 0.f;
        }
        for (int e = tid; e < IMP_D0_SB * IMP_D0_IC; e += 256) {
            const int oo = e % IMP_D0_IC, bl = e / IMP_D0_IC;
            ds[oo * IMP_D0_XP + bl] = (b0 + bl < a.B && o0 + oo < a.D) ? dh[(long)(b0 + bl) * a.D + o0 + oo] : 0.f;
        }
        __syncthreads();
        float pa[4] = {0.f, 0.f, 0.f, 0.f};
        for (int oo = 0; oo < IMP_D0_IC; ++oo) {
            const float w = ws[il * (IMP_D0_IC + 1) + oo];
            const float4 d = *(const float4*)(ds + oo * IMP_D0_XP + sg * 4);
            pa[0] = fmaf(d.x, w, pa[0]); pa[1] = fmaf(d.y, w, pa[1]); pa[2] = fmaf(d.z, w, pa[2]); pa[3] = fmaf(d.w, w, pa[3]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += pa[j];
    }
    const int i = i0 + il;
    if (i >= a.F) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = b0 + sg * 4 + j;
        if (b < a.B) {
            const long at = ((long)k * a.B + b) * a.F + i;
            a.din[at] = a.x[at] > 0.f ? acc[j] : 0.f;
        }
    }
}
