// Stand-alone host check of csrc/imp_mx_wgrad_args.h: the launch plan of the matrix-core weight gradient
// (IDQN_IMP_WGRAD=bf16x3) at its boundaries.
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I i-dqn_amd/csrc
//         tools/probes/imp_mx_wgrad_args_probe.cpp && ./a.out
// With arguments "B H W ci co [B H W ci co ...]": prints the plan per tuple, one per line, as
// "tiles_h tiles_w n_tiles n_chunks m_blocks n_blocks part_len eligible" (tests/test_impala_mx_wgrad_host.py compares it
// with its restatement).
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "imp_mx_wgrad_args.h"

static int failures = 0, checks = 0;
static void expect_int(const char* what, long got, long want) {
    ++checks;
    if (got != want) {
        printf("FAIL %s: got %ld, want %ld\n", what, got, want);
        ++failures;
    }
}

int main(int argc, char** argv) {
    if (argc > 1) {
        if ((argc - 1) % 5) return 2;
        for (int i = 1; i + 4 < argc; i += 5) {
            const int ci = atoi(argv[i + 3]), co = atoi(argv[i + 4]);
            const imxw_plan_t p = imxw_plan(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), ci, co);
            printf("%u %u %u %u %u %u %lld %d\n", p.tiles_h, p.tiles_w, p.n_tiles, p.n_chunks, p.m_blocks, p.n_blocks, (long long)p.part_len,
                   imx_eligible(ci, co));
        }
        return 0;
    }
    printf("constants %d %d %d %d %d\n", IMXW_TH, IMXW_TW, IMXW_MB, IMXW_NB, IMXW_TILES);
    expect_int("a k-step is the MFMA's K", IMXW_TW, 16);
    expect_int("an M tile holds whole eligible steps", IMXW_MB % IMX_KC, 0);
    expect_int("an N tile is the rule's", IMXW_NB, IMX_NB);
    for (int B = 1; B <= 33; ++B)
        for (int H : {1, 7, 8, 9, 15, 16, 17, 42, 84})
            for (int W : {1, 15, 16, 17, 31, 32, 33, 42})
                for (int ci : {16, 32, 48, 64})
                    for (int co : {32, 64, 96}) {
                        const imxw_plan_t p = imxw_plan(B, H, W, ci, co);
                        expect_int("tiles cover H", (long)p.tiles_h * IMXW_TH >= H && (long)(p.tiles_h - 1) * IMXW_TH < H, 1);
                        expect_int("tiles cover W", (long)p.tiles_w * IMXW_TW >= W && (long)(p.tiles_w - 1) * IMXW_TW < W, 1);
                        expect_int("tiles", p.n_tiles, (long)B * p.tiles_h * p.tiles_w);
                        expect_int("chunks cover the tiles", (long)p.n_chunks * IMXW_TILES >= p.n_tiles && (long)(p.n_chunks - 1) * IMXW_TILES < p.n_tiles, 1);
                        expect_int("M blocks cover ci", (long)p.m_blocks * IMXW_MB >= ci && (long)(p.m_blocks - 1) * IMXW_MB < ci, 1);
                        expect_int("N blocks cover co", (long)p.n_blocks * IMXW_NB == co, 1);
                        expect_int("partial", p.part_len, 9L * ci * co + co);
                    }
    expect_int("the workload's Stack 0, B = 32: chunks", imxw_plan(32, 42, 42, 32, 32).n_chunks, 72);
    expect_int("one tile", imxw_plan(1, 8, 16, 16, 32).n_chunks, 1);
    expect_int("exactly one chunk", imxw_plan(2, 16, 32, 32, 32).n_tiles, 8);
    expect_int("exactly one chunk", imxw_plan(2, 16, 32, 32, 32).n_chunks, 1);
    expect_int("one chunk plus one tile", imxw_plan(1, 17, 33, 32, 32).n_chunks, 2);
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures != 0;
}
