// Stand-alone host check of csrc/imp_mx_args.h: the values of IDQN_IMP_CONV, the eligibility rule of the matrix-core conv
// kernel at its boundaries, and the launch plan.
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I i-dqn_amd/csrc
//         tools/probes/imp_mx_args_probe.cpp && ./a.out
// With arguments "ci co [ci co ...]": prints imx_eligible per pair, one per line; with "plan H W co n": the grid
// (tests/test_impala_mx_shapes_host.py compares both with its restatement).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "imp_mx_args.h"

static int failures = 0, checks = 0;
static void expect_int(const char* what, long got, long want) {
    ++checks;
    if (got != want) {
        printf("FAIL %s: got %ld, want %ld\n", what, got, want);
        ++failures;
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "plan")) {
        if (argc != 6) return 2;
        const imx_plan_t p = imx_plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atol(argv[5]));
        printf("%u %u %u\n", p.tiles, p.n_tiles, p.images);
        return 0;
    }
    if (argc > 1) {
        if ((argc - 1) % 2) return 2;
        for (int i = 1; i + 1 < argc; i += 2) printf("%d\n", imx_eligible(atoi(argv[i]), atoi(argv[i + 1])));
        return 0;
    }
    printf("constants %d %d %d %d\n", IMX_TH, IMX_TW, IMX_KC, IMX_NB);
    expect_int("unset", imx_mode_of(nullptr), IMX_MODE_VALU);
    expect_int("valu", imx_mode_of("valu"), IMX_MODE_VALU);
    expect_int("bf16x3", imx_mode_of("bf16x3"), IMX_MODE_BF16X3);
    for (const char* bad : {"", "VALU", "bf16", "bf16x3 ", "1", "f32", "mfma"}) expect_int(bad, imx_mode_of(bad), IMX_MODE_BAD);
    for (int ci = -16; ci <= 160; ++ci)
        for (int co = -32; co <= 160; ++co)
            expect_int("eligible", imx_eligible(ci, co), ci > 0 && co > 0 && ci % 16 == 0 && co % 32 == 0);
    expect_int("workload 32 -> 64", imx_eligible(32, 64), 1);
    expect_int("frame channels", imx_eligible(4, 32), 0);
    expect_int("16 -> 16", imx_eligible(16, 16), 0);
    expect_int("16 -> 32", imx_eligible(16, 32), 1);
    expect_int("33 -> 32", imx_eligible(33, 32), 0);
    for (int H = 1; H <= 90; ++H)
        for (int W : {1, 15, 16, 17, 42, 84})
            for (int co : {1, 16, 32, 33, 64}) {
                const imx_plan_t p = imx_plan(H, W, co, 7);
                const long th = p.tiles / ((W + 15) / 16);
                expect_int("tiles cover H", th * 16 >= H && (th - 1) * 16 < H, 1);
                expect_int("N tiles cover co", p.n_tiles * 32 >= (unsigned)co && (p.n_tiles - 1) * 32 < (unsigned)co, 1);
                expect_int("images", p.images, 7);
            }
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures != 0;
}
