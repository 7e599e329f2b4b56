// Plane-layout convolution, forward and data gradient: the one-item workgroup body (convp.h has the layouts and the
// arithmetic; convp_fwd_phases.h the superstep's matrix work and the tile epilogue, which the persistent kernel of
// convp_pp.hip restates -- this file is the one-item SCHEDULE over them: who loads, the ring hand-over, the epilogue's hand-off).
// Kernels: convp_fwd.hip (one role per launch), convp_pair.hip (a data gradient beside a weight gradient).
//   forward        architectures/dqn.py:42-52  flax nn.Conv (NHWC x HWIO, cross-correlation) + bias + ReLU
//   data gradient  jax.value_and_grad, idqn.py:105: a stride-1 convolution over the zero-bordered dout planes with the
//                  re-indexed kernel (packed by k_stage), one variant per output parity; ReLU mask of the layer below
//
// Work decomposition: a workgroup (512 threads, ONE per CU: waves 0-3 compute, one per SIMD; waves 4-7 only issue the
// LDS-DMA copies) owns `np` consecutive output positions of one (net, batch block) for all CO channels: np * CT tiles of
// 32 samples x 32 channels, dealt round-robin to the compute waves (<= NT each).  The host sizes the items so that one
// launch is at most one workgroup per CU with equal work.
// K loop: a superstep = one kernel row kh and one 16-channel chunk.  Per superstep the loader waves stage
//   * the NQ taps x CT tiles x 3 planes of packed weights (one contiguous run), and
//   * for every input row its positions touch, the STRIP of pixel chunks they read -- neighbouring output positions
//     share pixels (3x3 stride 1: each staged chunk serves 3 taps), which keeps the L2 -> LDS traffic per MFMA low;
// into a ring of 2-3 stage buffers, two supersteps ahead (counted s_waitcnt vmcnt + one s_barrier per superstep), while
// the compute waves run NQ x NT tile-steps of 6 (Conv_0: 3) MFMAs from LDS fragments.
// Orientation: A = activations (rows = samples), B = weights (columns = channels), so a lane ends up with 4 x 4
// consecutive samples of ONE channel: plane rows are written as 8-byte pieces, the bias / mask is one value per lane.
#pragma once
#include "convp_fwd_phases.h"

namespace {

// b = this workgroup's item index (already remapped XCD-contiguously): its entry of the item table a.items.
template <int NPA, int CT, int NQ, int NT>
__device__ __forceinline__ void cfwd_body(const CFwdArgs& a, unsigned stage_bytes, int ring, unsigned mask_off, long long* prof_arg,
                                          const int b) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    constexpr int WB = NQ * CT * 3 * 1024, BLKA = NPA * 1024, NWP = NQ * CT * 3;
    const int t = threadIdx.x, lane = t & 63, h = lane >> 5, cl = lane & 31;
    // waves 0-3 compute (one per SIMD), waves 4-7 only issue the LDS-DMA copies: a wave that did both kept its matrix pipe
    // idle for the ~1000 cycles per superstep its ~11 copies take to issue
    const int wave8 = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool loader = wave8 >= 4;
    const int wave = wave8 & 3;
    // The phase stamps exist in the debug build only: in the shipped one `prof` is a constant and the stamps, their counter
    // reads in front of the first copy and the ten scalar registers they kept live across the superstep loop fold away.
    // (In the debug build they are unconditional up to the loop: a branch here splits the block and the kernel-argument
    // loads, which the scheduler otherwise batches at the top, become a chain of dependent round trips.)
#ifdef IDQN_DEBUG_KNOBS
    long long* const prof = prof_arg;
    const long long pt0 = clock64(), pw0 = wall_clock64();
#else
    constexpr long long* prof = nullptr;
    constexpr long long pt0 = 0, pw0 = 0;
    (void)prof_arg;
#endif
    // the item: one 64-byte scalar load of the plan's table (convp_items.h), no division in front of the first copy
    const auto dp = (const __attribute__((address_space(4))) u32x4*)(uintptr_t)(a.items + b);
    const u32x4 d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
    const int net = (int)d1.x, out_slot = (int)d1.y, vi = (int)d1.z, p0 = (int)d1.w, np = (int)d2.x, oh0 = (int)d2.y;
    const CVar& v = a.var[vi];
    const unsigned long in_base = (unsigned long)a.in + ((unsigned long)d0.x | (unsigned long)d0.y << 32);
    // strips: input row r of this workgroup serves output columns [c0, c0 + ncol) of output row oh0 + r
    int nx[CP_MAX_STRIPS], c0[CP_MAX_STRIPS], nc[CP_MAX_STRIPS];
    unsigned soff[CP_MAX_STRIPS];
    unsigned long sb[CP_MAX_STRIPS];
    {
        const unsigned cw[2] = {d2.z, d2.w}, nw[2] = {d3.x, d3.y};
        const long row_step = (long)a.S * a.row_bytes, col_step = (long)a.S * a.pix_bytes;
        unsigned accb = 0;
#pragma unroll
        for (int r = 0; r < CP_MAX_STRIPS; ++r) {
            c0[r] = (int)((r & 1) ? cw[r >> 1] >> 16 : cw[r >> 1] & 0xffffu);
            nc[r] = (int)((r & 1) ? nw[r >> 1] >> 16 : nw[r >> 1] & 0xffffu);
            nx[r] = nc[r] > 0 ? (nc[r] - 1) * a.SX + NQ : 0;
            soff[r] = accb;
            accb += (unsigned)nx[r] * BLKA;
            sb[r] = in_base + (unsigned long)(r * row_step + (long)(c0[r] - c0[0]) * col_step);
        }
    }
    // tiles of this wave: tile index wave + 4 i -> position j = idx / CT, channel tile ct = idx % CT (= wave % CT);
    // tpos = (output row << 16 | column) of the variant's grid, -1: no tile
    const int ct = wave % CT;
    unsigned abase[NT];
    int tpos[NT];
    const int e0 = nc[0], e1 = e0 + nc[1], e2 = e1 + nc[2];  // positions of the item before strip 1, 2, 3
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int j = (wave + 4 * i) / CT, jj = min(j, np - 1);
        const int r = (jj >= e0 ? 1 : 0) + (jj >= e1 ? 1 : 0) + (jj >= e2 ? 1 : 0);
        const int x = jj - (r == 0 ? 0 : r == 1 ? e0 : r == 2 ? e1 : e2);  // column inside strip r
        int c0r = c0[0];
        unsigned so = soff[0];
#pragma unroll
        for (int s = 1; s < CP_MAX_STRIPS; ++s) {
            c0r = (r == s) ? c0[s] : c0r;
            so = (r == s) ? soff[s] : so;
        }
        tpos[i] = j < np ? ((oh0 + r) << 16 | (c0r + x)) : -1;
        abase[i] = WB + so + (unsigned)(x * a.SX) * BLKA;
    }
    const unsigned lo_tr = cf_lo_tr(lane);
    const unsigned lane16 = lane * 16;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&lds[0];
    const unsigned long wb0 = (unsigned long)a.wq + ((unsigned long)d0.z | (unsigned long)d0.w << 32);
    const int NSS = a.KH * a.NCC;

    auto stage_w = [&](int ss, unsigned buf, int first, int step) {  // the packed kernels of superstep ss
        const unsigned long wsrc = wb0 + (unsigned long)ss * WB;
        for (int i = first; i < NWP; i += step) dma16(lane16, wsrc + (unsigned long)i * 1024, buf + i * 1024);
    };
    auto stage_x = [&](int ss, unsigned buf, int first, int step) {  // its pixel strips
        const int kh = ss / a.NCC, cc = ss - kh * a.NCC;
        const unsigned long so_ = (unsigned long)kh * (unsigned long)a.row_bytes + (unsigned long)cc * 1024;
#pragma unroll
        for (int r = 0; r < CP_MAX_STRIPS; ++r) {
            const unsigned long src = sb[r] + so_;
            const unsigned dst = buf + WB + soff[r];
            for (int x = first; x < nx[r]; x += step) {
#pragma unroll
                for (int pl = 0; pl < NPA; ++pl)
                    dma16(lane16, src + (unsigned long)x * (unsigned long)a.xstep + (unsigned long)pl * (unsigned long)a.plane_bytes,
                          dst + (x * NPA + pl) * 1024);
            }
        }
    };
    auto stage = [&](int ss, unsigned buf, int first, int step) {
        stage_w(ss, buf, first, step);
        stage_x(ss, buf, first, step);
    };

    // epilogue operands that only depend on the item: requested now, used after the loop
    const int co = ct * 32 + cl;
    float bias = 0.f;
    if (a.epilogue == 0) bias = cf_bias_row(a, net)[co];
    // data gradient: the ReLU masks of this wave's tiles are copied into LDS behind the stage buffers while the last
    // superstep computes
    const unsigned mask_lds = mask_off + wave * (NT * CF_MASK_TILE_BYTES);
    auto tile_out = [&](int p, int& yh, int& yw) { cf_out_pos(v, p >> 16, p & 0xffff, yh, yw); };

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

#ifdef IDQN_DEBUG_KNOBS
    const long long pt1 = clock64();
#else
    constexpr long long pt1 = 0;
#endif
    long long pwait = 0, pt2 = 0;
    if (loader) {
        // ---- loader waves: copy `ring - 1` supersteps ahead while the compute waves work ----------------------------
        // Superstep ss + ring - 1 goes into the buffer superstep ss - 1 was read from, right after barrier ss.  Before
        // barrier ss a loader only needs ITS copies of superstep ss to have landed: vmcnt counts in issue order, so it
        // waits until at most the copies of the younger supersteps (cnt per superstep, the same every time) are left.
        int cnt = (NWP - wave + 3) / 4, cnt_x = 0;
#pragma unroll
        for (int r = 0; r < CP_MAX_STRIPS; ++r) cnt_x += ((nx[r] - wave + 3) / 4) * NPA;
        cnt += cnt_x;
        const int ahead = ring - 1;
        for (int s0 = 0; s0 < ahead && s0 < NSS; ++s0) stage(s0, lds0 + s0 * stage_bytes, wave, 4);
        int nbuf = ahead == 2 ? 2 : 1;  // buffer of superstep ss + ahead
        long long l_wait = 0, l_bar = 0, l_issue = 0;
        for (int ss = 0; ss < NSS; ++ss) {
            const long long c0 = prof ? clock64() : 0;
            wait_vmcnt((ahead == 2 && ss + 1 < NSS) ? cnt : 0);
            const long long c1 = prof ? clock64() : 0;
            __builtin_amdgcn_s_barrier();  // everybody's copies of ss have landed; nobody still reads the buffer re-filled next
            const long long c2 = prof ? clock64() : 0;
            if (ss + ahead < NSS) stage(ss + ahead, lds0 + nbuf * stage_bytes, wave, 4);
            if (prof) { l_wait += c1 - c0; l_bar += c2 - c1; l_issue += clock64() - c2; }
            nbuf = nbuf + 1 == ring ? 0 : nbuf + 1;
            if (ss + 1 == NSS && a.epilogue == 1) {
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    if (tpos[i] < 0) continue;
                    int yh, yw;
                    tile_out(tpos[i], yh, yw);
                    cf_mask_copy(lane16, cf_mask_src(a, out_slot, yh, yw, ct), lds0 + mask_lds + i * CF_MASK_TILE_BYTES);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the mask copies
        if (prof && t == 256) {
            long long* pr = prof + 8L * 4096 + (long)b * 8;
            pr[0] = l_wait; pr[1] = l_bar; pr[2] = l_issue; pr[3] = cnt;
        }
    }
    // ---- compute waves -------------------------------------------------------------------------------------------
    int cbuf = 0;
    for (int ss = 0; ss < NSS && !loader; ++ss) {
        const unsigned cur_off = cbuf * stage_bytes;
        cbuf = cbuf + 1 == ring ? 0 : cbuf + 1;
        const long long pw = prof ? clock64() : 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (prof) { const long long now = clock64(); pwait += now - pw; if (ss == 0) pt2 = now; }
        cf_superstep<NPA, CT, NQ, NT>(lds + cur_off, abase, ct, lane16, lo_tr, acc);
    }

    const long long pt3 = prof ? clock64() : 0;
    // ---- epilogue: every tile is turned around in LDS (the stage buffers are free now; convp_fwd_phases.h has the why) ----
    // The work (bias / mask, the 3-way bf16 split: ~120 VALU instructions per tile) is shared with the loader waves, idle
    // by now: compute wave w keeps its first KEEP tiles and hands the others, as raw accumulators through LDS, to loader
    // wave w + 4, which has the same tile table.
    constexpr int KEEP = (NT + 1) / 2, NH = NT - KEEP;
    const unsigned rsz = cf_turn_bytes(a.out3 != nullptr, a.out_f32 != nullptr);
    unsigned char* R = lds + wave8 * rsz;                       // this wave's turn-around tile: [3 planes x 2 KB][f32 4 KB]
    unsigned char* H = lds + 8 * rsz + wave * (NH * 4096);      // hand-off tiles of compute wave `wave`
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the loaders' mask copies have landed; every wave is done with the stage buffers
    if (NH > 0) {
        if (!loader) {
#pragma unroll
            for (int i = KEEP; i < NT; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *LDS_PTR(f32x4, H + (i - KEEP) * 4096 + g * 1024 + lane16) =
                        (f32x4){acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    const CfSwizzle sw = cf_swizzle(lane);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (tpos[i] < 0 || loader != (i >= KEEP)) continue;  // wave-uniform
        f32x16 av;
        if (i >= KEEP) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 x = *LDS_PTR(const f32x4, H + (i >= KEEP ? i - KEEP : 0) * 4096 + g * 1024 + lane16);
                av[4 * g] = x[0]; av[4 * g + 1] = x[1]; av[4 * g + 2] = x[2]; av[4 * g + 3] = x[3];
            }
        } else {
            av = acc[i];
        }
        int yh, yw;
        tile_out(tpos[i], yh, yw);
        float val[16];
        cf_tile_values(a, av, bias, lds + mask_lds + i * CF_MASK_TILE_BYTES, cl, h, val);
        if (a.epilogue == 1 && a.pb) cf_bias_grad_sum(a, val, out_slot, yh, yw, co, h);
        cf_tile_to_lds(a, val, R, sw, cl, h);
        cf_tile_store(a, R, sw, out_slot, yh, yw, ct, lane);
    }
    if (prof && t == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        long long* pr = prof + (long)b * 8;
        pr[0] = pw0; pr[1] = pt1 - pt0; pr[2] = pt2 - pt1; pr[3] = pt3 - pt2; pr[4] = clock64() - pt3; pr[5] = pwait; pr[6] = wall_clock64();
        pr[7] = np;
    }
}


}  // namespace
