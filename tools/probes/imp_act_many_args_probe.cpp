// Stand-alone host check of csrc/imp_act_many_args.h: the argument checks of idqn_act_host_many_impala at their boundaries, the
// check of the grouped head table against hand-made good and bad tables and against every table a reference builder makes for
// a sweep of assignments, and the Dense_0 plan at its edges.
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I i-dqn_amd/csrc
//         tools/probes/imp_act_many_args_probe.cpp && ./a.out
// With a file argument: one table per line, "n K | heads | n_groups | order | g_head | g_start | g_count" (the arrays at their
// exact lengths); prints "ok" or the refusal text per line (tests/test_impala_act_many_host.py feeds it numpy's tables).
// Every array is allocated at its exact length, so a check that read past it would trip the sanitizer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "imp_act_many_args.h"

static int failures = 0, checks = 0;
static void expect(const char* what, const char* got, const char* want) {
    const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
    ++checks;
    if (!ok) {
        printf("FAIL %s: got %s, want %s\n", what, got ? got : "(fine)", want ? want : "(fine)");
        ++failures;
    }
}
static void expect_int(const char* what, long got, long want) {
    ++checks;
    if (got != want) {
        printf("FAIL %s: got %ld, want %ld\n", what, got, want);
        ++failures;
    }
}

struct Table {
    std::vector<int32_t> head, order, g_head, g_start, g_count;
    int32_t n_groups = 0;
};
// the grouping, stated independently of the library's builder: heads ascending, call order within a head
static Table build(const std::vector<int32_t>& heads, int K) {
    Table t;
    t.head = heads;
    for (int k = 0; k < K; ++k) {
        const int start = (int)t.order.size();
        for (int e = 0; e < (int)heads.size(); ++e)
            if (heads[e] == k) t.order.push_back(e);
        if ((int)t.order.size() > start) {
            t.g_head.push_back(k);
            t.g_start.push_back(start);
            t.g_count.push_back((int)t.order.size() - start);
        }
    }
    t.n_groups = (int)t.g_head.size();
    return t;
}
static const char* check(const std::vector<int32_t>& heads, int K, const Table& t, int* at) {
    return imp_act_many_table_error((int32_t)heads.size(), K, heads.data(), t.head.data(), t.n_groups, t.order.data(), t.g_head.data(),
                                    t.g_start.data(), t.g_count.data(), at);
}

static std::vector<int32_t> ints(const std::string& s) {
    std::vector<int32_t> v;
    std::istringstream in(s);
    long x;
    while (in >> x) v.push_back((int32_t)x);
    return v;
}

static int from_file(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        std::vector<std::string> parts;
        std::string cur;
        for (const char* p = line; *p; ++p) {
            if (*p == '|') { parts.push_back(cur); cur.clear(); }
            else cur.push_back(*p);
        }
        parts.push_back(cur);
        if (parts.size() != 7) { fclose(f); return 3; }
        const std::vector<int32_t> nk = ints(parts[0]), heads = ints(parts[1]), ng = ints(parts[2]);
        if (nk.size() != 2 || ng.size() != 1) { fclose(f); return 3; }
        Table t;
        t.head = heads; t.n_groups = ng[0]; t.order = ints(parts[3]); t.g_head = ints(parts[4]); t.g_start = ints(parts[5]); t.g_count = ints(parts[6]);
        if ((int)heads.size() != nk[0] || (int)t.order.size() != nk[0] || (int)t.g_head.size() < t.n_groups ||
            (int)t.g_start.size() < t.n_groups || (int)t.g_count.size() < t.n_groups) { fclose(f); return 3; }
        int at;
        const char* bad = check(heads, nk[1], t, &at);
        printf("%s\n", bad ? bad : "ok");
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return from_file(argv[1]);
    int at;
    // ---- arguments ----
    {
        int32_t* heads = (int32_t*)malloc(32 * sizeof(int32_t));  // exactly 32
        for (int e = 0; e < 32; ++e) heads[e] = e % 5;
        char s, q, a;
        for (int n : {-1, 0, 1, 2, 31, 32, 33, 1 << 30})
            expect("n", imp_act_many_args_error(n, 5, 0, heads, &s, &q, &a, &at), n < 1 || n > 32 ? "n is outside [1, 32]" : nullptr);
        for (int w : {-1, 0, 1, 2}) expect("which", imp_act_many_args_error(4, 5, w, heads, &s, &q, &a, &at), w == 0 || w == 1 ? nullptr : "which");
        expect("null heads", imp_act_many_args_error(4, 5, 0, nullptr, &s, &q, &a, &at), "null pointer");
        expect("null states", imp_act_many_args_error(4, 5, 0, heads, nullptr, &q, &a, &at), "null pointer");
        expect("null q", imp_act_many_args_error(4, 5, 0, heads, &s, nullptr, &a, &at), "null pointer");
        expect("null actions", imp_act_many_args_error(4, 5, 0, heads, &s, &q, nullptr, &at), "null pointer");
        expect("no heads", imp_act_many_args_error(1, 0, 0, heads, &s, &q, &a, &at), "no heads");
        for (int e : {0, 7, 31})
            for (int v : {-1, 4, 5, 1 << 30}) {
                const int32_t keep = heads[e];
                heads[e] = v;
                const char* got = imp_act_many_args_error(32, 5, 1, heads, &s, &q, &a, &at);
                expect("head", got, v >= 0 && v < 5 ? nullptr : "head is outside");
                if (got) expect_int("head: the state", at, e);
                heads[e] = keep;
            }
        heads[20] = 9;  // past n: not looked at
        expect("head past n", imp_act_many_args_error(20, 5, 0, heads, &s, &q, &a, &at), nullptr);
        free(heads);
    }
    // ---- tables: the builder's, for a sweep of assignments ----
    unsigned rng = 12345u;
    auto draw = [&](int m) { rng = rng * 1664525u + 1013904223u; return (int)((rng >> 8) % (unsigned)m); };
    for (int n = 1; n <= 32; ++n)
        for (int K : {1, 2, 3, 5, 32, 40})
            for (int mode = 0; mode < 4; ++mode) {
                std::vector<int32_t> heads(n);
                for (int e = 0; e < n; ++e) heads[e] = mode == 0 ? K - 1 : mode == 1 ? e % K : mode == 2 ? K - 1 - e % K : draw(K);
                const Table t = build(heads, K);
                expect("built table", check(heads, K, t, &at), nullptr);
                expect_int("built table: groups", t.n_groups <= n && t.n_groups <= K, 1);
            }
    // ---- tables: hand-made ----
    {
        const std::vector<int32_t> heads = {2, 0, 2, 1, 0, 2, 0};  // K = 4: head 3 unused
        Table good;
        good.head = heads; good.n_groups = 3;
        good.order = {1, 4, 6, 3, 0, 2, 5}; good.g_head = {0, 1, 2}; good.g_start = {0, 3, 4}; good.g_count = {3, 1, 3};
        expect("hand-made", check(heads, 4, good, &at), nullptr);
        const Table same = build(heads, 4);
        expect_int("hand-made equals the builder", same.order == good.order && same.g_head == good.g_head && same.g_start == good.g_start &&
                                                       same.g_count == good.g_count && same.n_groups == 3, 1);
        Table t = good;
        t.head[3] = 2;
        expect("head differs", check(heads, 4, t, &at), "differs from the call's");
        t = good; t.order[2] = 7;
        expect("order outside", check(heads, 4, t, &at), "outside [0, n)");
        t = good; t.order[2] = -1;
        expect("order negative", check(heads, 4, t, &at), "outside [0, n)");
        t = good; t.order[2] = 4;
        expect("order twice", check(heads, 4, t, &at), "appears twice");
        t = good; std::swap(t.order[0], t.order[1]);
        expect("group out of call order", check(heads, 4, t, &at), "not in call order");
        t = good; std::swap(t.order[2], t.order[3]);
        expect("state in another head's group", check(heads, 4, t, &at), "group of another head");
        t = good; t.n_groups = 0;
        expect("no groups", check(heads, 4, t, &at), "number of groups");
        t = good; t.n_groups = 2;
        expect("groups short", check(heads, 4, t, &at), "do not cover");
        t = good; t.order = {0, 2, 5, 3, 1, 4, 6}; t.g_head = {2, 1, 0};  // consistent groups, heads descending
        expect("heads descend", check(heads, 4, t, &at), "do not ascend");
        t = good; t.g_head = {0, 1, 1};
        expect("head twice", check(heads, 4, t, &at), "do not ascend");
        t = good; t.g_head = {0, 1, 4};
        expect("group head outside", check(heads, 4, t, &at), "group's head is outside");
        t = good; t.g_head = {-1, 1, 2};
        expect("group head negative", check(heads, 4, t, &at), "group's head is outside");
        t = good; t.g_start = {0, 2, 4};
        expect("gap", check(heads, 4, t, &at), "does not start where");
        t = good; t.g_count = {3, 0, 3};
        expect("empty group", check(heads, 4, t, &at), "count is outside");
        t = good; t.g_count = {3, 1, 4};
        expect("count past n", check(heads, 4, t, &at), "count is outside");
        t = good; t.g_count = {3, 1, 2};
        expect("last group short", check(heads, 4, t, &at), "do not cover");
        expect_int("last group short: not about a group", at, -1);
        // more groups than heads / than states
        const std::vector<int32_t> one = {0};
        Table o = build(one, 1);
        expect("one state", check(one, 1, o, &at), nullptr);
        o.n_groups = 2; o.g_head = {0, 1}; o.g_start = {0, 1}; o.g_count = {1, 1};
        expect("more groups than states", check(one, 3, o, &at), "number of groups");
        expect("null array", imp_act_many_table_error(1, 1, one.data(), nullptr, 1, o.order.data(), o.g_head.data(), o.g_start.data(),
                                                      o.g_count.data(), &at), "null pointer");
        expect("n = 0", imp_act_many_table_error(0, 1, one.data(), one.data(), 1, o.order.data(), o.g_head.data(), o.g_start.data(),
                                                 o.g_count.data(), &at), "n is outside");
        // 32 states on 32 heads, descending: the order is the reversal
        std::vector<int32_t> desc(32);
        for (int e = 0; e < 32; ++e) desc[e] = 31 - e;
        const Table d = build(desc, 32);
        expect("32 groups", check(desc, 32, d, &at), nullptr);
        for (int e = 0; e < 32; ++e) expect_int("32 groups: order", d.order[e], 31 - e);
    }
    // ---- the Dense_0 plan ----
    {
        struct { int F, D, n_pass, ranges, cb, lpf, lrp, lbu; } rows[] = {
            {7744, 512, 121, 31, 8, 64, 1, 64}, {605, 9, 10, 3, 1, 29, 2, 9}, {60, 65, 1, 1, 2, 60, 1, 1}, {128, 64, 2, 1, 1, 64, 2, 64},
            {198, 6, 4, 1, 1, 6, 4, 6},         {8, 12, 1, 1, 1, 8, 1, 12},   {1, 1, 1, 1, 1, 1, 1, 1},    {64, 64, 1, 1, 1, 64, 1, 64},
            {65, 128, 2, 1, 2, 1, 2, 64},       {256, 1, 4, 1, 1, 64, 4, 1},  {257, 63, 5, 2, 1, 1, 1, 63},
        };
        for (const auto& r : rows) {
            const imp_act_many_d0_plan_t p = imp_act_many_d0_plan(r.F, r.D);
            expect_int("n_pass", p.n_pass, r.n_pass);
            expect_int("ranges", p.ranges, r.ranges);
            expect_int("col_blocks", p.col_blocks, r.cb);
            expect_int("last_pass_features", p.last_pass_features, r.lpf);
            expect_int("last_range_passes", p.last_range_passes, r.lrp);
            expect_int("last_block_units", p.last_block_units, r.lbu);
            expect_int("part_floats", (long)p.part_floats, 32L * r.n_pass * r.D);
        }
        for (int F = 1; F <= 600; ++F)
            for (int D : {1, 63, 64, 65, 512}) {
                const imp_act_many_d0_plan_t p = imp_act_many_d0_plan(F, D);
                // every feature in exactly one pass, every pass in exactly one range, every unit in exactly one block
                expect_int("passes cover F", (p.n_pass - 1) * IMP_ACT_PASS + p.last_pass_features, F);
                expect_int("last pass", p.last_pass_features >= 1 && p.last_pass_features <= IMP_ACT_PASS, 1);
                expect_int("ranges cover the passes", (p.ranges - 1) * IMP_ACT_PPW + p.last_range_passes, p.n_pass);
                expect_int("last range", p.last_range_passes >= 1 && p.last_range_passes <= IMP_ACT_PPW, 1);
                expect_int("blocks cover D", (p.col_blocks - 1) * IMP_ACT_OC + p.last_block_units, D);
            }
        for (int c = 1; c <= 32; ++c) {
            expect_int("chunks cover the group", (imp_act_many_chunks(c) - 1) * IMP_ACT_SC + imp_act_many_last_chunk(c), c);
            expect_int("last chunk", imp_act_many_last_chunk(c) >= 1 && imp_act_many_last_chunk(c) <= IMP_ACT_SC, 1);
        }
        expect_int("chunks(8)", imp_act_many_chunks(8), 1);
        expect_int("chunks(9)", imp_act_many_chunks(9), 2);
        expect_int("chunks(32)", imp_act_many_chunks(32), 4);
    }
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures != 0;
}
