// Stand-alone host check of csrc/per_step_args.h and csrc/per_group_args.h: the record builders and the refusals at their
// boundaries; for the group check, on both record types, the accepting case and every refusal -- NULL, n_steps and batch out of
// range, depth, n_items, n_heads, tau_dev, every pointer of a record, every aliasing pair -- and the layout of the staged block.
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I i-dqn_amd/csrc tools/probes/per_args_probe.cpp && ./a.out
// The group records are allocated at their exact count, so a check that read past member S - 1 would trip the sanitizer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "per_group_args.h"

static int failures = 0, checks = 0;
static void expect(const char* what, const char* got, const char* want) {
    const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
    ++checks;
    if (!ok) {
        printf("FAIL %s: got %s, want %s\n", what, got ? got : "(fine)", want ? want : "(fine)");
        ++failures;
    }
}
static void expect_members(const char* what, int g, int j, int want_g, int want_j) {
    ++checks;
    if (g != want_g || j != want_j) {
        printf("FAIL %s: members (%d, %d), want (%d, %d)\n", what, g, j, want_g, want_j);
        ++failures;
    }
}

static const int S = 3;
// (only the addresses are looked at)
static double nodes[S][2], pri[S][1], mx[S][1], scratch[S][1], u[S][1];
static int32_t leaves[S][1];
static float w[S][1], td[S][1], tau[1];

static void set_tau(idqn_per_step_t& p) { p.tau_dev = tau; }
static void set_tau(idqn_per_steps_t&) {}

// The group check on records of type P; n_steps: the single step's record goes with 1
template <class P>
static void group_checks(const char* type, int n_steps) {
    P* per = (P*)malloc(S * sizeof(P));  // exactly S records
    if (!per) exit(2);
    int g = 0, j = 0;
    auto member = [&](int i) {
        P p;
        memset(&p, 0, sizeof(p));
        p.nodes_dev = nodes[i]; p.depth = 4 + i; p.n_items = 8; p.uniforms_host = u[i]; p.stratified = 1; p.beta = 0.4; p.eps = 1e-3; p.alpha = 0.6;
        p.max_priority_dev = mx[i]; p.leaves_dev = leaves[i]; p.weights_dev = w[i]; p.td_abs_dev = td[i]; p.priorities_dev = pri[i];
        p.tree_scratch_dev = scratch[i];
        return p;
    };
    auto fill = [&] { for (int i = 0; i < S; ++i) per[i] = member(i); };
    auto run = [&](int n_members = S, int n = -99, int batch = 32, int K = 3) {
        return per_group_args_error(per, n_members, n == -99 ? n_steps : n, batch, K, &g, &j);
    };
    fill();
    expect(type, run(), nullptr);
    expect_members("valid", g, j, -1, -1);
    expect("valid, one member", run(1), nullptr);
    expect("valid, two members", run(2), nullptr);
    expect("null records", per_group_args_error((const P*)nullptr, S, n_steps, 32, 3, &g, &j), "null pointer");
    for (int n : {-1, 0, 1, 32, 33}) expect("n_steps", run(S, n), n < 1 || n > 32 ? "n_steps not in" : nullptr);
    for (int b : {-1, 0, 1, 7, 32, 33}) expect("batch", run(S, n_steps, b), b < 1 || b > 32 ? "batch not in" : nullptr);
    for (int depth : {0, 1, 31, 32}) {
        fill();
        per[1].depth = depth;
        expect("depth", run(), depth < 1 || depth > 31 ? "depth" : nullptr);
        if (depth < 1 || depth > 31) expect_members("depth", g, j, 1, -1);
    }
    for (int64_t items : {(int64_t)-1, (int64_t)0, (int64_t)1}) {
        fill();
        per[2].n_items = items;
        expect("n_items", run(), items < 1 ? "n_items < 1" : nullptr);
        if (items < 1) expect_members("n_items", g, j, 2, -1);
    }
    fill();
    expect("n_heads 0", run(S, n_steps, 32, 0), "n_heads < 1");
    set_tau(per[0]);  // the single step's record alone has the field
    expect("tau", run(), per_tau_of(per[0]) ? "tau_dev is set" : nullptr);
    if (per_tau_of(per[0])) expect_members("tau", g, j, 0, -1);
    // every pointer of a record; priorities_dev and max_priority_dev may be NULL
    for (int f = 0; f < 8; ++f) {
        fill();
        P& p = per[S - 1];
        switch (f) {
            case 0: p.nodes_dev = nullptr; break;
            case 1: p.uniforms_host = nullptr; break;
            case 2: p.leaves_dev = nullptr; break;
            case 3: p.weights_dev = nullptr; break;
            case 4: p.td_abs_dev = nullptr; break;
            case 5: p.tree_scratch_dev = nullptr; break;
            case 6: p.priorities_dev = nullptr; break;
            default: p.max_priority_dev = nullptr; break;
        }
        expect("null field", run(), f < 6 ? "null pointer" : nullptr);
        if (f < 6) expect_members("null field", g, j, S - 1, -1);
    }
    // every aliasing pair: member 1, then member 2, names a buffer of member 0
    const char* names[] = {"nodes_dev", "leaves_dev", "weights_dev", "td_abs_dev", "tree_scratch_dev", "priorities_dev", "max_priority_dev"};
    for (int later : {1, 2})
        for (int f = 0; f < 7; ++f) {
            fill();
            P &a = per[later], &b = per[0];
            switch (f) {
                case 0: a.nodes_dev = b.nodes_dev; break;
                case 1: a.leaves_dev = b.leaves_dev; break;
                case 2: a.weights_dev = b.weights_dev; break;
                case 3: a.td_abs_dev = b.td_abs_dev; break;
                case 4: a.tree_scratch_dev = b.tree_scratch_dev; break;
                case 5: a.priorities_dev = b.priorities_dev; break;
                default: a.max_priority_dev = b.max_priority_dev; break;
            }
            expect("alias", run(), names[f]);
            expect_members(names[f], g, j, later, 0);
            if (later == 2) expect("alias: not among the first two", run(2), nullptr);
        }
    fill();
    for (int i = 0; i < S; ++i) per[i].priorities_dev = per[i].max_priority_dev = nullptr;  // NULLs are not one buffer
    expect("optional outputs all NULL", run(), nullptr);
    free(per);
}

int main() {
    auto rec = [&](int depth, int64_t n_items, int K) {
        return per_sampler(nodes[0], depth, n_items, u[0], 1, 0.4, leaves[0], w[0], td[0], K, 0, 1e-3, 0.6, pri[0], mx[0], scratch[0]);
    };
    const PerSampler ok = rec(4, 8, 2);
    if (ok.nodes != nodes[0] || ok.uniforms != u[0] || ok.leaves != leaves[0] || ok.weights != w[0] || ok.td_abs != td[0] || ok.priorities != pri[0] ||
        ok.max_dev != mx[0] || ok.scratch != scratch[0] || ok.n_items != 8.0 || ok.beta != 0.4 || ok.eps != 1e-3 || ok.alpha != 0.6 ||
        ok.depth != 4 || ok.stratified != 1 || ok.reduce_max != 0 || ok.K != 2) {
        printf("FAIL per_sampler: a field went astray\n");
        ++failures;
    }
    // depth 0, 1, 31, 32; n 0, 1, 256, 257; n_items 0; n_heads 0
    for (int depth : {0, 1, 31, 32}) {
        const char* want = depth < 1 || depth > 31 ? "depth" : nullptr;
        expect("draw depth", per_draw_args_error(rec(depth, 8, 2), 4), want);
        expect("write-back depth", per_write_back_args_error(rec(depth, 8, 2), 4), want);
        expect("step depth", per_step_args_error(rec(depth, 8, 2), 4), want);
    }
    for (int n : {0, 1, 256, 257}) {
        const char* want = n < 1 || n > 256 ? "n not in" : nullptr;
        expect("draw n", per_draw_args_error(ok, n), want);
        expect("write-back n", per_write_back_args_error(ok, n), want);
    }
    expect("n_items 0", per_draw_args_error(rec(4, 0, 2), 4), "n_items < 1");
    expect("n_items 0: not the write-back's business", per_write_back_args_error(rec(4, 0, 2), 4), nullptr);
    expect("n_heads 0", per_write_back_args_error(rec(4, 8, 0), 4), "n_heads < 1");
    expect("n_heads 0: not the draw's business", per_draw_args_error(rec(4, 8, 0), 4), nullptr);
    expect("step: the draw's refusal first", per_step_args_error(rec(4, 0, 0), 4), "n_items < 1");
    // every pointer of each end; priorities and max_dev may be NULL
    for (int f = 0; f < 8; ++f) {
        PerSampler s = ok;
        void** field[] = {(void**)&s.nodes, (void**)&s.uniforms, (void**)&s.leaves, (void**)&s.weights, (void**)&s.td_abs, (void**)&s.scratch,
                          (void**)&s.priorities, (void**)&s.max_dev};
        *field[f] = nullptr;
        expect("draw null", per_draw_args_error(s, 4), f < 4 ? "null pointer" : nullptr);
        expect("write-back null", per_write_back_args_error(s, 4), f == 0 || f == 2 || f == 4 || f == 5 ? "null pointer" : nullptr);
        expect("step null", per_step_args_error(s, 4), f < 6 ? "null pointer" : nullptr);
    }

    group_checks<idqn_per_step_t>("group valid, single-step records", 1);
    group_checks<idqn_per_steps_t>("group valid, n-step records", 3);
    // the block: parts in order, 16-byte aligned, the uniforms last; one step of it is the single group call's block
    for (int n_members : {1, 3, 32})
        for (int n_steps : {1, 2, 32})
            for (int batch : {1, 7, 32}) {
                const size_t mb = 328;  // (any record size that is a multiple of 8)
                const PerGroupStepsBlock b = per_group_steps_block(mb, n_members, n_steps, batch);
                const size_t recs = (size_t)n_members * n_steps;
                ++checks;
                if (b.samplers_off % 16 || b.uniforms_off % 16 || b.samplers_off < recs * mb || b.samplers_off >= recs * mb + 16 ||
                    b.uniforms_off < b.samplers_off + recs * sizeof(PerSampler) || b.uniforms_off >= b.samplers_off + recs * sizeof(PerSampler) + 16 ||
                    b.bytes != b.uniforms_off + recs * batch * 8 ||
                    b.bytes > per_group_steps_block(mb, n_members, IDQN_MAX_STEPS_PER_CALL, PER_GROUP_MAX_N).bytes) {
                    printf("FAIL block layout at S = %d, n = %d, B = %d\n", n_members, n_steps, batch);
                    ++failures;
                }
            }
    printf(failures ? "per_args_probe: %d checks, %d FAILED\n" : "per_args_probe: %d checks, ok\n", checks, failures);
    return failures != 0;
}
