// Host side of the impala matrix-core conv mode (IDQN_IMP_CONV=bf16x3, impala_mx_kernels.h): the values of the switch, the
// per-layer eligibility rule and the launch plan.  Plain host C++ without a HIP dependency, as imp_act_many_args.h:
// tools/probes/imp_mx_args_probe.cpp prints the rule for the tests, and impala_mx_kernels.h takes its constants from here.
#pragma once
#include <stdint.h>
#include <string.h>

#define IMX_TH 16    // tile height (output rows) of a workgroup: wave w owns rows 4 w .. 4 w + 3
#define IMX_TW 16    // tile width: one M tile of the 32x32x16 MFMA is two tile rows
#define IMX_KC 16    // input channels of a k-step (one MFMA), and of an LDS pass: a pass sums 9 taps x 16 channels
#define IMX_NB 32    // output channels of a workgroup: one N tile

enum { IMX_MODE_VALU = 0, IMX_MODE_BF16X3 = 1, IMX_MODE_BAD = -1 };

// IDQN_IMP_CONV: unset or "valu" = the vector-ALU kernels, "bf16x3" = the matrix-core kernel where a layer is eligible
static inline int imx_mode_of(const char* v) {
    if (!v || !strcmp(v, "valu")) return IMX_MODE_VALU;
    if (!strcmp(v, "bf16x3")) return IMX_MODE_BF16X3;
    return IMX_MODE_BAD;
}

// A 3x3 conv layer whose LEAF has ci input and co output channels runs on the matrix cores, forward and data gradient,
// when ci is a whole number of k-steps and co a whole number of N tiles.  The data gradient sums over co (a multiple of 16
// then) and writes ci channels: its last N tile may be half empty, which the kernel pads with zero weights.
static inline int imx_eligible(int32_t leaf_ci, int32_t leaf_co) {
    return leaf_ci > 0 && leaf_co > 0 && leaf_ci % IMX_KC == 0 && leaf_co % IMX_NB == 0;
}

// grid of a launch on H x W frames writing `co` channels for n_img images: (tiles, N tiles, images)
struct imx_plan_t { uint32_t tiles, n_tiles, images; };
static inline imx_plan_t imx_plan(int32_t H, int32_t W, int32_t co, int64_t n_img) {
    imx_plan_t p;
    p.tiles = (uint32_t)(((H + IMX_TH - 1) / IMX_TH) * ((W + IMX_TW - 1) / IMX_TW));
    p.n_tiles = (uint32_t)((co + IMX_NB - 1) / IMX_NB);
    p.images = (uint32_t)n_img;
    return p;
}
