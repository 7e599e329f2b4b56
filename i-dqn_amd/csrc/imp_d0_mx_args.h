// Host side of the impala f32 matrix-core Dense_0 forward (IDQN_IMP_D0=mfma, impala_d0_mx_kernels.h): the values of the
// switch, which handles have such a launch, and the launch plan.  Plain host C++ without a HIP dependency, as imp_mx_args.h:
// tools/probes/imp_d0_mx_args_probe.cpp prints the plan for the tests, and the kernel takes its constants from here.
#pragma once
#include <stdint.h>
#include <string.h>

#define IMPD0X_PASS 64   // features of one pass: the block of k_imp_d0_fwd's blocked sum (= IMP_D0_IC; qnet.hip asserts it)
#define IMPD0X_TILE 32   // samples and hidden units of a workgroup: one accumulator of the 32x32x2 MFMA
#define IMPD0X_WAVES 4   // passes of a round: pass p runs on wave p % 4
#define IMPD0X_XP 33     // LDS pitch of a staged [feature][sample] row: odd, so the staging stores and the fragment reads
                         // of 32 consecutive lanes fall on 32 banks

enum { IMPD0_MODE_VALU = 0, IMPD0_MODE_MFMA = 1, IMPD0_MODE_BAD = -1 };

// IDQN_IMP_D0: unset or "valu" = k_imp_d0_fwd, "mfma" = k_imp_d0_fwd_mx; anything else is refused by idqn_create
static inline int impd0_mode_of(const char* v) {
    if (!v || !strcmp(v, "valu")) return IMPD0_MODE_VALU;
    if (!strcmp(v, "mfma")) return IMPD0_MODE_MFMA;
    return IMPD0_MODE_BAD;
}

// Only an impala handle whose head has a hidden dense layer (n_dense >= 2 dense layers: Dense_0 then at least the output
// layer) launches a Dense_0 forward of its own; for every other handle the mode is a no-op.
static inline int impd0x_applies(int is_impala, int32_t n_dense) { return is_impala && n_dense >= 2; }

// One launch for `nets` nets of B samples, F features and D hidden units each: grid (unit tiles, sample blocks, nets) of
// 256 lanes; `passes` passes of IMPD0X_PASS features (the last one ragged when F is no multiple), dealt to the waves in
// `rounds` rounds of IMPD0X_WAVES, the last round holding `last_round` of them (1 .. IMPD0X_WAVES).  lds_bytes: the round's
// x tiles, then the four waves' pass sums.
struct impd0x_plan_t { uint32_t passes, rounds, last_round, grid_x, grid_y, grid_z, lds_bytes; };
static inline impd0x_plan_t impd0x_plan(int32_t B, int32_t F, int32_t D, int32_t nets) {
    impd0x_plan_t p;
    p.passes = (uint32_t)((F + IMPD0X_PASS - 1) / IMPD0X_PASS);
    p.rounds = (p.passes + IMPD0X_WAVES - 1) / IMPD0X_WAVES;
    p.last_round = p.passes - (p.rounds - 1) * IMPD0X_WAVES;
    p.grid_x = (uint32_t)((D + IMPD0X_TILE - 1) / IMPD0X_TILE);
    p.grid_y = (uint32_t)((B + IMPD0X_TILE - 1) / IMPD0X_TILE);
    p.grid_z = (uint32_t)nets;
    p.lds_bytes = 4u * (IMPD0X_WAVES * IMPD0X_PASS * IMPD0X_XP + IMPD0X_WAVES * IMPD0X_TILE * IMPD0X_TILE);
    return p;
}

// what the launch code requires of a shape before it launches (a handle's shapes always pass): the grid's y and z are bounded
// by 65535, and the kernel addresses a leaf and a net's [B][F] block with 32-bit byte offsets
static inline int impd0x_shape_ok(int32_t B, int32_t F, int32_t D, int32_t nets) {
    return B >= 1 && F >= 1 && D >= 1 && nets >= 1 && nets <= 65535 && (B + IMPD0X_TILE - 1) / IMPD0X_TILE <= 65535 &&
           (int64_t)F * D <= (1LL << 29) && (int64_t)B * F <= (1LL << 29);
}
