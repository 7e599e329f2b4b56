// Stand-alone host check of the conv item tables (csrc/convp_items.h) for a sanitizer build; no device call.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/probes/conv_items_check.hip -o conv_items_check && ./conv_items_check
// Fills exactly-sized heap tables (a write past an end is an AddressSanitizer report) for the headline forward roles, a
// four-variant data-gradient launch and a ragged frame at one and two sample blocks, and checks that the items cover every
// (slot, variant, position) once.  The persistent kernel's table (convp_fill_pp_items) at the 17x17, 9x69 and 43x49 frames
// of tests/conv_pp_shapes.py: the items tile every output row of every (slot, variant) exactly once, none crosses a row,
// p0 = row * OW + col0, and item b has the slot and variant the one-item table gives index b for the same ranges.
#include <cstdio>
#include <vector>

#include "../../i-dqn_amd/csrc/convp_items.h"

static int check(const char* what, CFwdArgs a, int n_nets) {
    const int n_items = a.items_per_slot * n_nets * a.nb;
    std::vector<CFwdDesc> tab((size_t)n_items);
    if (!convp_fill_fwd_items(a, n_items, tab.data())) { printf("%s: refused\n", what); return 1; }
    long total = 0, want = 0;
    for (int v = 0; v < a.n_var; ++v) want += (long)a.var[v].OH * a.var[v].OW * n_nets * a.nb;
    std::vector<std::vector<char>> seen;
    for (int v = 0; v < a.n_var; ++v) seen.emplace_back((size_t)a.var[v].OH * a.var[v].OW * n_nets * a.nb, 0);
    for (const CFwdDesc& d : tab) {
        int cols = 0;
        for (int s = 0; s < CP_MAX_STRIPS; ++s) cols += d.ncol[s];
        if (cols != d.np || d.out_slot != d.net * a.nb + d.bb) { printf("%s: inconsistent item\n", what); return 1; }
        for (int p = d.p0; p < d.p0 + d.np; ++p) {
            char& c = seen[d.var][(size_t)d.out_slot * a.var[d.var].OH * a.var[d.var].OW + p];
            if (c) { printf("%s: position %d of slot %d twice\n", what, p, d.out_slot); return 1; }
            c = 1;
            ++total;
        }
    }
    if (total != want) { printf("%s: %ld of %ld positions\n", what, total, want); return 1; }
    printf("%s: %d items, %ld positions, ok\n", what, n_items, total);
    return 0;
}

static int check_pp(const char* what, CFwdArgs a, int n_nets, int parts) {
    a.row_parts = parts; a.items_per_slot = 0;
    for (int v = 0; v < a.n_var; ++v) { a.r_begin[v] = a.items_per_slot; a.r_cnt[v] = a.var[v].OH * parts; a.items_per_slot += a.r_cnt[v]; }
    const int n_items = a.items_per_slot * n_nets * a.nb;
    std::vector<CItem> tab((size_t)n_items);
    std::vector<CFwdDesc> one((size_t)n_items);
    if (!convp_fill_pp_items(a, n_items, tab.data()) || !convp_fill_fwd_items(a, n_items, one.data())) { printf("%s: refused\n", what); return 1; }
    std::vector<std::vector<char>> seen;
    for (int v = 0; v < a.n_var; ++v) seen.emplace_back((size_t)a.var[v].OH * a.var[v].OW * n_nets * a.nb, 0);
    long total = 0, want = 0;
    for (int v = 0; v < a.n_var; ++v) want += (long)a.var[v].OH * a.var[v].OW * n_nets * a.nb;
    for (int b = 0; b < n_items; ++b) {
        const CItem& it = tab[b];
        const int slot = it.net * a.nb + it.bb;
        if (it.var < 0 || it.var >= a.n_var || it.net < 0 || it.net >= n_nets || it.bb < 0 || it.bb >= a.nb) { printf("%s: item %d out of range\n", what, b); return 1; }
        const int OW = a.var[it.var].OW, OH = a.var[it.var].OH;
        if (slot != one[b].out_slot || it.var != one[b].var) { printf("%s: item %d is (slot %d, variant %d), the one-item table has (%d, %d)\n", what, b, slot, it.var, one[b].out_slot, one[b].var); return 1; }
        if (it.row < 0 || it.row >= OH || it.np <= 0 || it.col0 < 0 || it.col0 + it.np > OW) { printf("%s: item %d crosses its row\n", what, b); return 1; }
        if (it.p0 != it.row * OW + it.col0) { printf("%s: item %d p0 %d is not row %d x %d + column %d\n", what, b, it.p0, it.row, OW, it.col0); return 1; }
        for (int p = it.p0; p < it.p0 + it.np; ++p) {
            char& c = seen[it.var][(size_t)slot * OH * OW + p];
            if (c) { printf("%s: position %d of slot %d twice\n", what, p, slot); return 1; }
            c = 1;
            ++total;
        }
    }
    if (total != want) { printf("%s: %ld of %ld positions\n", what, total, want); return 1; }
    printf("%s: %d items in %d parts per row, %ld positions, ok\n", what, n_items, parts, total);
    return 0;
}

static CFwdArgs fwd(int OH, int OW, int R, int nb, int S, int range_major, int in_split) {
    CFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.items_per_slot = R; a.range_major = range_major; a.nb = nb; a.n_var = 1; a.in_split = in_split; a.S = S;
    a.pix_bytes = 3 * 32 * 64; a.row_bytes = (OW * S + 4) * a.pix_bytes; a.in_slot = (long)(OH * S + 4) * a.row_bytes; a.wq_stride = 1 << 20;
    a.r_cnt[0] = R; a.var[0].OH = OH; a.var[0].OW = OW;
    return a;
}

int main() {
    int bad = 0;
    bad += check("Conv_0 forward, K = 5", fwd(21, 21, 25, 1, 4, 1, 5), 10);
    bad += check("Conv_1 forward, K = 5", fwd(11, 11, 21, 1, 2, 0, 0), 10);
    bad += check("Conv_2 forward, K = 5, B = 64", fwd(11, 11, 12, 2, 1, 0, 0), 10);
    bad += check("36x28 Conv_1 forward, K = 2", fwd(5, 4, 20, 1, 2, 0, 0), 4);
    CFwdArgs d = fwd(11, 11, 31, 1, 1, 0, 0);  // Conv_1 data gradient at K = 5: parities 11x11, 11x10, 10x11, 10x10
    d.n_var = 4;
    const int oh[4] = {11, 11, 10, 10}, ow[4] = {11, 10, 11, 10}, rc[4] = {9, 8, 7, 7};
    for (int v = 0, begin = 0; v < 4; begin += rc[v++]) {
        d.r_begin[v] = begin; d.r_cnt[v] = rc[v]; d.var[v].OH = oh[v]; d.var[v].OW = ow[v];
        d.var[v].in_off_h = 1 - v / 2; d.var[v].in_off_w = 1 - v % 2; d.var[v].w_off = (long)v * 4 * 64 * 32 * 6;
    }
    bad += check("Conv_1 data gradient, K = 5", d, 5);
    // persistent tables: Conv_0 (range-major) and Conv_1 / Conv_2 (net-major) of the 17x17, 9x69 and 43x49 frames, and the
    // four-parity Conv_1 data gradient of 17x17 (5x5 input: 3x3, 3x2, 2x3, 2x2) and 9x69 (3x18: 2x9, 2x9, 1x9, 1x9)
    bad += check_pp("17x17 Conv_0 persistent, K = 17, B = 250", fwd(5, 5, 1, 8, 4, 1, 17), 34, 1);
    bad += check_pp("17x17 Conv_2 persistent, K = 17, B = 250", fwd(3, 3, 1, 8, 1, 0, 0), 34, 1);
    bad += check_pp("9x69 Conv_0 persistent, K = 9, B = 130", fwd(3, 18, 1, 5, 4, 1, 9), 18, 1);
    bad += check_pp("9x69 Conv_1 persistent, 9 columns in 2", fwd(2, 9, 1, 5, 2, 0, 0), 18, 2);
    bad += check_pp("9x69 Conv_2 persistent, 9 columns in 4", fwd(2, 9, 1, 5, 1, 0, 0), 18, 4);
    bad += check_pp("43x49 Conv_0 persistent, K = 5, B = 256", fwd(11, 13, 1, 8, 4, 1, 5), 10, 1);
    bad += check_pp("43x49 Conv_1 persistent, 7 columns in 2", fwd(6, 7, 1, 8, 2, 0, 0), 10, 2);
    const int oh17[4] = {3, 3, 2, 2}, ow17[4] = {3, 2, 3, 2}, oh69[4] = {2, 2, 1, 1}, ow69[4] = {9, 9, 9, 9};
    CFwdArgs e = fwd(3, 3, 1, 8, 1, 0, 0), f = fwd(2, 9, 1, 5, 1, 0, 0);
    e.n_var = f.n_var = 4;
    for (int v = 0; v < 4; ++v) {
        e.var[v].OH = oh17[v]; e.var[v].OW = ow17[v]; f.var[v].OH = oh69[v]; f.var[v].OW = ow69[v];
        e.var[v].in_off_h = f.var[v].in_off_h = 1 - v / 2; e.var[v].in_off_w = f.var[v].in_off_w = 1 - v % 2;
    }
    bad += check_pp("17x17 Conv_1 data gradient persistent, K = 17", e, 17, 1);
    bad += check_pp("9x69 Conv_1 data gradient persistent, 9 columns in 2", f, 9, 2);
    return bad ? 1 : 0;
}
