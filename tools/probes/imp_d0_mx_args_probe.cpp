// Stand-alone host check of csrc/imp_d0_mx_args.h: the switch, the rule and the launch plan of the f32 matrix-core Dense_0
// forward (IDQN_IMP_D0=mfma) at their boundaries.
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I i-dqn_amd/csrc
//         tools/probes/imp_d0_mx_args_probe.cpp && ./a.out
// With arguments "B F D nets [B F D nets ...]": prints the plan per tuple, one per line, as
// "passes rounds last_round grid_x grid_y grid_z lds_bytes shape_ok" (tests/test_impala_d0_mx_host.py compares it with its
// restatement).  With "mode VALUE ...": prints the switch's reading of the unset variable, then of each value.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "imp_d0_mx_args.h"

static int failures = 0, checks = 0;
static void expect_int(const char* what, long got, long want) {
    ++checks;
    if (got != want) {
        printf("FAIL %s: got %ld, want %ld\n", what, got, want);
        ++failures;
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "mode")) {
        printf("%d\n", impd0_mode_of(nullptr));
        for (int i = 2; i < argc; ++i) printf("%d\n", impd0_mode_of(argv[i]));
        return 0;
    }
    if (argc > 1) {
        if ((argc - 1) % 4) return 2;
        for (int i = 1; i + 3 < argc; i += 4) {
            const int B = atoi(argv[i]), F = atoi(argv[i + 1]), D = atoi(argv[i + 2]), nets = atoi(argv[i + 3]);
            const impd0x_plan_t p = impd0x_plan(B, F, D, nets);
            printf("%u %u %u %u %u %u %u %d\n", p.passes, p.rounds, p.last_round, p.grid_x, p.grid_y, p.grid_z, p.lds_bytes, impd0x_shape_ok(B, F, D, nets));
        }
        return 0;
    }
    printf("constants %d %d %d %d\n", IMPD0X_PASS, IMPD0X_TILE, IMPD0X_WAVES, IMPD0X_XP);
    expect_int("unset is valu", impd0_mode_of(nullptr), IMPD0_MODE_VALU);
    expect_int("valu", impd0_mode_of("valu"), IMPD0_MODE_VALU);
    expect_int("mfma", impd0_mode_of("mfma"), IMPD0_MODE_MFMA);
    for (const char* v : {"", "bf16x3", "MFMA", "mfma ", "1", "valu,mfma"}) expect_int("refused", impd0_mode_of(v), IMPD0_MODE_BAD);
    expect_int("a head with a hidden layer", impd0x_applies(1, 2), 1);
    expect_int("two hidden layers", impd0x_applies(1, 3), 1);
    expect_int("no hidden layer", impd0x_applies(1, 1), 0);
    expect_int("not impala", impd0x_applies(0, 2), 0);
    expect_int("an odd pitch", IMPD0X_XP % 2, 1);
    expect_int("a tile is one MFMA accumulator", IMPD0X_TILE, 32);
    for (int B : {1, 31, 32, 33, 64, 65, 256})
        for (int F = 1; F <= 1100; ++F)
            for (int D : {1, 31, 32, 33, 64, 65, 512})
                for (int nets : {1, 2, 10}) {
                    const impd0x_plan_t p = impd0x_plan(B, F, D, nets);
                    expect_int("passes cover F", (long)p.passes * IMPD0X_PASS >= F && (long)(p.passes - 1) * IMPD0X_PASS < F, 1);
                    expect_int("rounds cover the passes", (long)p.rounds * IMPD0X_WAVES >= p.passes && (long)(p.rounds - 1) * IMPD0X_WAVES < p.passes, 1);
                    expect_int("the last round", p.last_round >= 1 && p.last_round <= IMPD0X_WAVES && (p.rounds - 1) * IMPD0X_WAVES + p.last_round == p.passes, 1);
                    expect_int("unit tiles cover D", (long)p.grid_x * IMPD0X_TILE >= D && (long)(p.grid_x - 1) * IMPD0X_TILE < D, 1);
                    expect_int("sample blocks cover B", (long)p.grid_y * IMPD0X_TILE >= B && (long)(p.grid_y - 1) * IMPD0X_TILE < B, 1);
                    expect_int("nets", p.grid_z, nets);
                    expect_int("LDS", p.lds_bytes, 50176);
                    expect_int("shape", impd0x_shape_ok(B, F, D, nets), 1);
                }
    const impd0x_plan_t w = impd0x_plan(32, 7744, 512, 10);
    expect_int("the workload: passes", w.passes, 121);
    expect_int("the workload: rounds", w.rounds, 31);
    expect_int("the workload: the last round holds one pass", w.last_round, 1);
    expect_int("the workload: workgroups", (long)w.grid_x * w.grid_y * w.grid_z, 160);
    expect_int("one acting net: workgroups", (long)impd0x_plan(1, 7744, 512, 1).grid_x, 16);
    expect_int("LDS under the 64 KB of a static allocation", w.lds_bytes <= 65536, 1);
    expect_int("no samples", impd0x_shape_ok(0, 64, 64, 1), 0);
    expect_int("no nets", impd0x_shape_ok(1, 64, 64, 0), 0);
    expect_int("too many nets for the grid", impd0x_shape_ok(1, 64, 64, 65536), 0);
    expect_int("a leaf behind 32-bit byte offsets", impd0x_shape_ok(1, 1 << 20, 1 << 10, 1), 0);
    expect_int("activations behind 32-bit byte offsets", impd0x_shape_ok(1 << 15, 1 << 15, 32, 1), 0);
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures != 0;
}
