// Host side of the impala matrix-core weight gradient (IDQN_IMP_WGRAD=bf16x3, impala_mx_wgrad_kernels.h): the launch plan.
// The switch takes the values of IDQN_IMP_CONV (imx_mode_of) and the layers the rule of the forward and the data gradient
// (imx_eligible), both from imp_mx_args.h.  Plain host C++ without a HIP dependency, as imp_mx_args.h:
// tools/probes/imp_mx_wgrad_args_probe.cpp prints the plan for the tests, and the kernel takes its constants from here.
#pragma once
#include "imp_mx_args.h"

#define IMXW_TH 8      // tile height: a tile row (IMXW_TW positions of one image row) is one k-step of the 32x32x16 MFMA
#define IMXW_TW 16     // tile width = the MFMA's K
#define IMXW_MB 32     // input channels of a workgroup: one M tile (a leaf of 16 channels fills half of it)
#define IMXW_NB 32     // output channels of a workgroup: one N tile
#define IMXW_TILES 8   // tiles of a chunk: a workgroup's accumulators run over 8 x 8 k-steps, then leave one partial

// One launch on B frames of H x W, leaf ci -> co: grid (n_chunks, m_blocks * n_blocks, heads); chunk c owns the tiles
// c * IMXW_TILES .. of the n_tiles = B * tiles_h * tiles_w tiles (image major, then tile row, then tile column), the last
// chunk what is left.  part_len floats per (head, chunk): 9 ci co kernel partials, then co bias partials.
struct imxw_plan_t { uint32_t tiles_h, tiles_w, n_tiles, n_chunks, m_blocks, n_blocks; int64_t part_len; };
static inline imxw_plan_t imxw_plan(int32_t B, int32_t H, int32_t W, int32_t ci, int32_t co) {
    imxw_plan_t p;
    p.tiles_h = (uint32_t)((H + IMXW_TH - 1) / IMXW_TH);
    p.tiles_w = (uint32_t)((W + IMXW_TW - 1) / IMXW_TW);
    p.n_tiles = (uint32_t)B * p.tiles_h * p.tiles_w;
    p.n_chunks = (p.n_tiles + IMXW_TILES - 1) / IMXW_TILES;
    p.m_blocks = (uint32_t)((ci + IMXW_MB - 1) / IMXW_MB);
    p.n_blocks = (uint32_t)((co + IMXW_NB - 1) / IMXW_NB);
    p.part_len = 9LL * ci * co + co;
    return p;
}
