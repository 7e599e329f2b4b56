// Stand-alone host check of csrc/act_group_args.h: every refusal of idqn_act_group_host's assignment at its boundary, and the
// sorted order and group arrays against a restatement (a stable std::sort and a scan) for all-one-pair, alternating, unsorted
// and random assignments at every n in [1, 32].
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I i-dqn_amd/csrc
//         tools/probes/act_group_args_probe.cpp && ./a.out
// The arrays are allocated at their exact sizes (n inputs, 32 outputs), so a builder or a check that read or wrote past them
// would trip the sanitizer.
//
// With a file name as its argument the program prints the tables of the assignments in that file instead (one per line:
// n, then n members, then n heads): "n_groups | order | g_member | g_head | g_start | g_count" -- tests/test_act_group_host.py
// compares them with its numpy restatement.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <numeric>
#include <random>
#include <vector>

#include "act_group_args.h"

static int failures = 0, checks = 0;
static void expect(const char* what, const char* got, const char* want) {
    const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
    ++checks;
    if (!ok) {
        printf("FAIL %s: got %s, want %s\n", what, got ? got : "(fine)", want ? want : "(fine)");
        ++failures;
    }
}

struct Table {
    int ng;
    int32_t *order, *g_member, *g_head, *g_start, *g_count;  // [32] each, heap: exact sizes
    Table() {
        int32_t** all[5] = {&order, &g_member, &g_head, &g_start, &g_count};
        for (auto p : all) {
            *p = (int32_t*)malloc(ACT_GROUP_MAX * sizeof(int32_t));
            for (int i = 0; i < ACT_GROUP_MAX; ++i) (*p)[i] = -7;
        }
        ng = 0;
    }
    ~Table() {
        for (int32_t* p : {order, g_member, g_head, g_start, g_count}) free(p);
    }
};

static void build(int n, const int32_t* member, const int32_t* heads, Table& t) {
    // (inputs of exactly n entries)
    int32_t* m = (int32_t*)malloc(n * sizeof(int32_t));
    int32_t* h = (int32_t*)malloc(n * sizeof(int32_t));
    memcpy(m, member, n * sizeof(int32_t));
    memcpy(h, heads, n * sizeof(int32_t));
    t.ng = act_group_build(n, m, h, t.order, t.g_member, t.g_head, t.g_start, t.g_count);
    free(m);
    free(h);
}

static void check_table(const char* what, int n, int S, int K, const std::vector<int32_t>& member, const std::vector<int32_t>& heads) {
    Table t;
    build(n, member.data(), heads.data(), t);
    std::vector<int> want(n);
    std::iota(want.begin(), want.end(), 0);
    std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return member[a] * K + heads[a] < member[b] * K + heads[b]; });
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && t.order[i] == want[i];
    int ng = 0, covered = 0;
    for (int i = 0; i < n;) {
        int j = i;
        while (j < n && member[want[j]] == member[want[i]] && heads[want[j]] == heads[want[i]]) ++j;
        ok = ok && ng < t.ng && t.g_member[ng] == member[want[i]] && t.g_head[ng] == heads[want[i]] && t.g_start[ng] == i && t.g_count[ng] == j - i;
        covered += j - i;
        ++ng;
        i = j;
    }
    ok = ok && ng == t.ng && covered == n && ng <= std::min(n, std::min(S * K, ACT_GROUP_MAX));
    for (int i = n; i < ACT_GROUP_MAX; ++i) ok = ok && t.order[i] == -7;  // nothing past n, nothing past the groups
    for (int g = t.ng; g < ACT_GROUP_MAX; ++g) ok = ok && t.g_member[g] == -7 && t.g_head[g] == -7 && t.g_start[g] == -7 && t.g_count[g] == -7;
    ++checks;
    if (!ok) {
        printf("FAIL table %s (n = %d, S = %d, K = %d)\n", what, n, S, K);
        ++failures;
    }
}

static int print_table(FILE* f, int n) {  // 0, or 2 on a malformed line
    if (n < 1 || n > ACT_GROUP_MAX) return 2;
    std::vector<int32_t> m(n), h(n);
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%d", &m[i]) != 1) return 2;
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%d", &h[i]) != 1) return 2;
    Table t;
    build(n, m.data(), h.data(), t);
    printf("%d |", t.ng);
    for (int i = 0; i < n; ++i) printf(" %d", t.order[i]);
    const int32_t* arrays[4] = {t.g_member, t.g_head, t.g_start, t.g_count};
    for (const int32_t* a : arrays) {
        printf(" |");
        for (int g = 0; g < t.ng; ++g) printf(" %d", a[g]);
    }
    printf("\n");
    return 0;
}

static int print_tables(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    int n, rc = 0;
    while (rc == 0 && fscanf(f, "%d", &n) == 1) rc = print_table(f, n);
    fclose(f);
    return rc;
}

int main(int argc, char** argv) {
    if (argc > 1) return print_tables(argv[1]);
    int e;
    // ---- range checks -----------------------------------------------------------------------------------------------
    {
        const int S = 3, K = 5;
        for (int n : {-1, 0, 1, 5, 32, 33}) {
            const int len = n < 1 ? 1 : n;
            int32_t* m = (int32_t*)calloc(len, sizeof(int32_t));
            int32_t* h = (int32_t*)calloc(len, sizeof(int32_t));
            expect("n", act_group_args_error(n, S, K, 0, m, h, &e), n < 1 || n > 32 ? "n is outside [1, 32]" : nullptr);
            if (n >= 1 && n <= 32) {
                expect("null members", act_group_args_error(n, S, K, 0, nullptr, h, &e), "null pointer");
                expect("null heads", act_group_args_error(n, S, K, 0, m, nullptr, &e), "null pointer");
                for (int w : {-1, 0, 1, 2}) expect("which", act_group_args_error(n, S, K, w, m, h, &e), w == 0 || w == 1 ? nullptr : "which");
                for (int at : {0, n / 2, n - 1}) {
                    for (int v : {-1, 0, S - 1, S, 1 << 30}) {
                        m[at] = v;
                        expect("member", act_group_args_error(n, S, K, 1, m, h, &e), v < 0 || v >= S ? "member is outside" : nullptr);
                        if ((v < 0 || v >= S) && e != at) expect("member: state", "e_out", "the state refused");
                        m[at] = 0;
                    }
                    for (int v : {-1, 0, K - 1, K, 1 << 30}) {
                        h[at] = v;
                        expect("head", act_group_args_error(n, S, K, 1, m, h, &e), v < 0 || v >= K ? "head is outside" : nullptr);
                        if ((v < 0 || v >= K) && e != at) expect("head: state", "e_out", "the state refused");
                        h[at] = 0;
                    }
                }
                expect("no members", act_group_args_error(n, 0, K, 0, m, h, &e), "no members or no heads");
                expect("33 members", act_group_args_error(n, 33, K, 0, m, h, &e), "no members or no heads");
                expect("no heads", act_group_args_error(n, S, 0, 0, m, h, &e), "no members or no heads");
            }
            free(m);
            free(h);
        }
    }
    // ---- tables -----------------------------------------------------------------------------------------------------
    std::mt19937 rng(5);
    for (int n = 1; n <= ACT_GROUP_MAX; ++n) {
        for (int S : {1, 2, 3, 8, 32}) {
            for (int K : {1, 2, 5}) {
                std::vector<int32_t> m(n), h(n);
                for (int i = 0; i < n; ++i) m[i] = S - 1, h[i] = K - 1;
                check_table("all on one pair", n, S, K, m, h);
                for (int i = 0; i < n; ++i) m[i] = i % S, h[i] = 0;
                check_table("the same head on every member", n, S, K, m, h);
                for (int i = 0; i < n; ++i) m[i] = (n - 1 - i) % S, h[i] = (n - 1 - i) % K;
                check_table("descending", n, S, K, m, h);
                for (int i = 0; i < n; ++i) m[i] = 0, h[i] = 0;
                m[n / 2] = S - 1;
                check_table("a lone state in the middle", n, S, K, m, h);
                for (int i = 0; i < n; ++i) m[i] = i & 1 ? S - 1 : 0, h[i] = i & 1 ? 0 : K - 1;
                check_table("alternating", n, S, K, m, h);
                for (int r = 0; r < 4; ++r) {
                    for (int i = 0; i < n; ++i) m[i] = (int)(rng() % S), h[i] = (int)(rng() % K);
                    check_table("random", n, S, K, m, h);
                }
            }
        }
    }
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures != 0;
}
