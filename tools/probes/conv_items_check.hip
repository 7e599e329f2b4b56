// Stand-alone host check of the conv item tables (csrc/convp_items.h) for a sanitizer build; no device call.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/probes/conv_items_check.hip -o conv_items_check && ./conv_items_check
// Fills exactly-sized heap tables (a write past an end is an AddressSanitizer report) for the headline forward roles, a
// four-variant data-gradient launch and a ragged frame at one and two sample blocks, and checks that the items cover every
// (slot, variant, position) once.
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
    return bad ? 1 : 0;
}
