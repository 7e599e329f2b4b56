// Plane-layout convolution, forward and data gradient: the phases of a workgroup, each stated once.
//   cfwd_body     (convp_fwd_body.h)  one item per workgroup (k_cfwd, the data-gradient role of k_cpair): a schedule over
//                                     these functions -- who loads, the ring hand-over, the epilogue's hand-off and the
//                                     phase stamps are its own
//   cfwd_pp_body  (convp_pp.hip)      persistent, three wave groups rotating through compute / load / epilogue (k_cfwd_pp):
//                                     uses the fragment helpers, the sizes and the store counts; the superstep, the tile
//                                     epilogue and the operand addresses are typed out there -- THE SAME TEXT as
//                                     cf_superstep, cf_tile_*, cf_mask_src, cf_bias_row below (a change here is made there
//                                     too) -- because calling them cost that kernel 0.9 % per step
//                                     (profiles/conv_phases_refactor.txt)
// The two kernels promise the same bytes (tests/test_gpu_switches.py, tests/test_gpu_conv_pp_shapes.py).
// Everything is forced inline.  convp.h has the layouts and the bf16x3 arithmetic.
#pragma once
#include "convp.h"

// ---- sizes (host and device) ------------------------------------------------------------------------------------
// Turn-around tile of one wave: [3 planes x 2 KB][f32 copy 4 KB], each part only when the launch writes it
#define CF_TURN_PLANES_BYTES 6144u
#define CF_TURN_F32_BYTES 4096u
__host__ __device__ inline unsigned cf_turn_bytes(bool planes_out, bool f32_out) {
    return (planes_out ? CF_TURN_PLANES_BYTES : 0u) + (f32_out ? CF_TURN_F32_BYTES : 0u);
}
// Data gradient: the ReLU mask of a tile = plane 0 of the forward activation at its output pixel, 32 channels x 64 B
#define CF_MASK_TILE_BYTES 2048u
// Vector-memory operations the pieces below issue per tile (the persistent kernel counts its own in issue order)
#define CF_PLANE_STORES 6                           // cf_tile_store: 3 planes x 2 runs of 1 KiB
#define CF_F32_STORES 4                             // cf_tile_store: 4 runs of 1 KiB
#define CF_PB_STORES 1                              // cf_bias_grad_sum
#define CF_MASK_COPIES (CF_MASK_TILE_BYTES / 1024)  // cf_mask_copy

namespace {

// ---- fragments --------------------------------------------------------------------------------------------------
__device__ __forceinline__ s16x4 tr_half(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}
__device__ __forceinline__ bf16x8 join8(s16x4 v0, s16x4 v1) {
    return __builtin_shufflevector(__builtin_bit_cast(bf16x4, v0), __builtin_bit_cast(bf16x4, v1), 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 frag_lin(const unsigned char* p) {
    return *(const __attribute__((address_space(3))) bf16x8*)p;
}
// byte offset of a lane's transposed-read rows inside a 1 KiB activation block
__device__ __forceinline__ unsigned cf_lo_tr(int lane) {
    const int h = lane >> 5;
    return (8 * h + ((lane & 15) >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
}

// ---- the matrix work of one superstep: NQ x NT tile-steps of 6 (Conv_0: 3) MFMAs out of the stage `cur` -----------
// abase[i]: where tile i's activation blocks sit in a stage.  Fragment reads of tile-step u + 1 are issued one per gap
// BETWEEN the MFMAs of tile-step u (the wave issues an MFMA, is free for the ~32 cycles it runs, and blocks at the next,
// dependent one): sched_barrier pins that order.  The activation halves of tile-step u + 2 are requested in the gaps of
// tile-step u (a ring of three register sets), the weight planes of tap q + 1 during the last-but-one tile-step of tap q:
// every ds_read has at least one whole tile-step (~190 cycles) to return before an MFMA waits for it.
// (Moving the barrier in front of the last two tile-steps and requesting the next stage's first fragments under them -- no
// drain / refill of the matrix pipe at the barrier -- was built and measured in the persistent kernel: same duration, 10-40
// more registers, profiles/r6_pp_phases.txt.)
#define CF_GAP(m)                                                                                              \
    {                                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        if (next_a && (m) < 2 * NPA) ah[(u + 2) % 3][((m) / 2) % NPA][(m) % 2] = tr_half(an + ((m) / 2) * 1024 + ((m) % 2) * 256); \
        if (next_w && (m) < 3) wf[(q + 1) & 1][(m) < 3 ? (m) : 0] = frag_lin(wn + (m) * 1024);                 \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
    }
template <int NPA, int CT, int NQ, int NT>
__device__ __forceinline__ void cf_superstep(const unsigned char* cur, const unsigned (&abase)[NT], const int ct, const unsigned lane16,
                                             const unsigned lo_tr, f32x16 (&acc)[NT]) {
    constexpr int BLKA = NPA * 1024, U = NQ * NT, WSTEP = NT >= 2 ? NT - 2 : 0;
    bf16x8 wf[2][3];
    s16x4 ah[3][NPA][2];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) wf[0][pl] = frag_lin(cur + (ct * 3 + pl) * 1024 + lane16);
#pragma unroll
    for (int u0 = 0; u0 < 2 && u0 < U; ++u0)
#pragma unroll
        for (int pl = 0; pl < NPA; ++pl) {
            const unsigned char* ap = cur + abase[u0 % NT] + (u0 / NT) * BLKA + pl * 1024 + lo_tr;
            ah[u0][pl][0] = tr_half(ap);
            ah[u0][pl][1] = tr_half(ap + 256);
        }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int u = q * NT + i;
            const bool next_w = (i == WSTEP && q + 1 < NQ), next_a = (u + 2 < U);
            const int qn = (u + 2) / NT, in_ = (u + 2) % NT;
            const unsigned char* an = cur + abase[next_a ? in_ : 0] + qn * BLKA + lo_tr;
            const unsigned char* wn = cur + (((q + 1) * CT + ct) * 3) * 1024 + lane16;
            bf16x8 A[NPA];
#pragma unroll
            for (int pl = 0; pl < NPA; ++pl) A[pl] = join8(ah[u % 3][pl][0], ah[u % 3][pl][1]);
            const bf16x8* W = wf[q & 1];
            __builtin_amdgcn_sched_barrier(0);
            if (NPA == 3) {  // smallest terms first
                acc[i] = mfma_bf16(A[2], W[0], acc[i]);
                CF_GAP(0)
                acc[i] = mfma_bf16(A[0], W[2], acc[i]);
                CF_GAP(1)
                acc[i] = mfma_bf16(A[1], W[1], acc[i]);
                CF_GAP(2)
                acc[i] = mfma_bf16(A[1], W[0], acc[i]);
                CF_GAP(3)
                acc[i] = mfma_bf16(A[0], W[1], acc[i]);
                CF_GAP(4)
                acc[i] = mfma_bf16(A[0], W[0], acc[i]);
                CF_GAP(5)
            } else {
                acc[i] = mfma_bf16(A[0], W[2], acc[i]);
                CF_GAP(0)
                acc[i] = mfma_bf16(A[0], W[1], acc[i]);
                CF_GAP(1)
                acc[i] = mfma_bf16(A[0], W[0], acc[i]);
                CF_GAP(2)
            }
        }
    }
}
#undef CF_GAP

// ---- epilogue operands ------------------------------------------------------------------------------------------
// output position (oh, ow) of a variant's grid -> (yh, yw) of the layer's (forward: the same; data gradient: its parity)
__device__ __forceinline__ void cf_out_pos(const CVar& v, const int oh, const int ow, int& yh, int& yw) {
    yh = oh * v.out_mul + v.out_add_h;
    yw = ow * v.out_mul + v.out_add_w;
}
// the bias row of a net's layer in the f32 parameter arenas
__device__ __forceinline__ const float* cf_bias_row(const CFwdArgs& a, const int net) {
    return (net < a.n_first ? a.pbase[0] + (long)net * a.pstride : a.pbase[1] + (long)(net - a.n_first) * a.pstride) + a.b_off;
}
// the mask of tile (out_slot, yh, yw, ct): CF_MASK_TILE_BYTES of plane 0 of the forward activation
__device__ __forceinline__ unsigned long cf_mask_src(const CFwdArgs& a, const int out_slot, const int yh, const int yw, const int ct) {
    return (unsigned long)a.mask3 + (unsigned long)out_slot * a.mask_slot +
           ((unsigned long)((yh + a.mask_lo_h) * a.mask_Wp + (yw + a.mask_lo_w)) * (3UL * a.mask_C) + ct * 32) * 64;
}
__device__ __forceinline__ void cf_mask_copy(const unsigned lane16, const unsigned long msrc, const unsigned lds_dst) {  // CF_MASK_COPIES LDS-DMA copies
#pragma unroll
    for (unsigned j = 0; j < CF_MASK_COPIES; ++j) dma16(lane16, msrc + j * 1024, lds_dst + j * 1024);
}

// ---- tile epilogue: lane = channel co = ct * 32 + cl, registers = samples (r & 3) + 8 (r >> 2) + 4 h ----------------
// the accumulators of one tile -> its values: bias + ReLU (epilogue 0), or the ReLU mask of the layer below, read from
// the tile's mask M in LDS (epilogue 1)
__device__ __forceinline__ void cf_tile_values(const CFwdArgs& a, const f32x16& av, const float bias, const unsigned char* M, const int cl,
                                               const int h, float (&val)[16]) {
    if (a.epilogue == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) val[r] = fmaxf(av[r] + bias, 0.f);
    } else {
        const unsigned char* Ml = M + cl * 64 + 8 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x2 mk = *LDS_PTR(const u32x2, Ml + 16 * g);
            const float m0 = __uint_as_float(mk.x << 16), m1 = __uint_as_float(mk.x & 0xffff0000u);
            const float m2 = __uint_as_float(mk.y << 16), m3 = __uint_as_float(mk.y & 0xffff0000u);
            val[4 * g + 0] = m0 > 0.f ? av[4 * g + 0] : 0.f;
            val[4 * g + 1] = m1 > 0.f ? av[4 * g + 1] : 0.f;
            val[4 * g + 2] = m2 > 0.f ? av[4 * g + 2] : 0.f;
            val[4 * g + 3] = m3 > 0.f ? av[4 * g + 3] : 0.f;
        }
    }
}
// bias gradient: the sum of a tile's values over its 32 samples, fixed order: registers, then the two half-waves
// (CF_PB_STORES stores)
__device__ __forceinline__ void cf_bias_grad_sum(const CFwdArgs& a, const float (&val)[16], const int out_slot, const int yh, const int yw,
                                                 const int co, const int h) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += val[r];
    s += __shfl_xor(s, 32);
    if (h == 0) a.pb[((long)out_slot * (a.out_H * a.out_W) + (long)yh * a.out_W + yw) * a.CO + co] = s;
}

// A lane's values of a tile are 8-byte pieces of 64-byte rows; written straight to HBM every store instruction would
// touch 32 rows (measured: ~330 cycles each).  Each wave therefore turns a tile around in LDS, in its own turn-around
// tile R, and stores whole 1 KiB runs: 16 rows of a plane, or 8 rows of the f32 copy, per instruction.  Swizzles (the
// writer's and the reader's must agree, which is why both are here):
//   plane rows  64 B = 4 slots of 16 B: slot ^ (row >> 1) & 3     written by row cl, read as row lane >> 2, slot lane & 3
//   f32 rows   128 B = 8 slots of 16 B: slot ^ (row & 7)          written by row cl, read as row lane >> 3, slot lane & 7
struct CfSwizzle {
    unsigned wsw, rsw, fsw;  // plane rows as written; plane rows / f32 rows as read (byte offset of the lane's 16 B)
};
__device__ __forceinline__ CfSwizzle cf_swizzle(const int lane) {
    const int cl = lane & 31;
    return {(unsigned)(cl >> 1) & 3, (lane * 16) ^ ((((unsigned)lane >> 3) & 3) << 4), (lane * 16) ^ ((((unsigned)lane >> 3) & 7) << 4)};
}
// values -> R: the exact 3-way bf16 split into the planes, and / or the f32 rows
__device__ __forceinline__ void cf_tile_to_lds(const CFwdArgs& a, const float (&val)[16], unsigned char* R, const CfSwizzle& sw, const int cl,
                                               const int h) {
    const unsigned wsw = sw.wsw;
    if (a.out3) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned q0a, q1a, q2a, q0b, q1b, q2b;
            split3_pk(val[4 * g + 0], val[4 * g + 1], q0a, q1a, q2a);
            split3_pk(val[4 * g + 2], val[4 * g + 3], q0b, q1b, q2b);
            unsigned char* wp = R + cl * 64 + ((g ^ wsw) * 16) + 8 * h;
            *LDS_PTR(u32x2, wp) = (u32x2){q0a, q0b};
            *LDS_PTR(u32x2, wp + 2048) = (u32x2){q1a, q1b};
            *LDS_PTR(u32x2, wp + 4096) = (u32x2){q2a, q2b};
        }
    }
    if (a.out_f32) {
        const unsigned r_f32 = a.out3 ? CF_TURN_PLANES_BYTES : 0;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *LDS_PTR(f32x4, R + r_f32 + cl * 128 + (((2 * g + h) ^ (cl & 7)) * 16)) =
                (f32x4){val[4 * g], val[4 * g + 1], val[4 * g + 2], val[4 * g + 3]};
    }
}
// R -> HBM: CF_PLANE_STORES stores into the output planes and / or CF_F32_STORES into the f32 rows, behind the wave's
// own writes of R and in front of its next ones
__device__ __forceinline__ void cf_tile_store(const CFwdArgs& a, const unsigned char* R, const CfSwizzle& sw, const int out_slot, const int yh,
                                              const int yw, const int ct, const int lane) {
    const unsigned rsw = sw.rsw, fsw = sw.fsw;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave, LDS is in order: its writes are visible to its reads
    if (a.out3) {
        unsigned char* O = (unsigned char*)a.out3 + (unsigned long)out_slot * a.out_slot +
                           ((unsigned long)((yh + a.out_lo_h) * a.out_Wp + (yw + a.out_lo_w)) * (3UL * a.CO) + ct * 32) * 64 + (unsigned)(lane * 16);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int j = 0; j < CF_PLANE_STORES / 3; ++j) {
                const u32x4 x = *LDS_PTR(const u32x4, R + pl * 2048 + j * 1024 + rsw);
                *reinterpret_cast<u32x4*>(O + (unsigned long)pl * a.CO * 64 + j * 1024) = x;
            }
    }
    if (a.out_f32) {
        const unsigned r_f32 = a.out3 ? CF_TURN_PLANES_BYTES : 0;
        float* F = a.out_f32 + (long)out_slot * a.f32_slot + (((long)yh * a.f32_W + yw) * a.CO + ct * 32) * 32 + lane * 4;
#pragma unroll
        for (int j = 0; j < CF_F32_STORES; ++j) {
            const f32x4 x = *LDS_PTR(const f32x4, R + r_f32 + j * 1024 + fsw);
            *reinterpret_cast<f32x4*>(F + j * 256) = x;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the tile has left LDS before the next one overwrites it
}

}  // namespace
