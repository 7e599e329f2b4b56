// Stand-alone host check of csrc/per_step_args.h and csrc/per_group_args.h: the record builders and the refusals at their
// boundaries.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I i-dqn_amd/csrc tools/probes/per_args_probe.cpp && ./a.out
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "per_group_args.h"

static int failures = 0;
static void expect(const char* what, const char* got, const char* want) {
    const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
    if (!ok) {
        printf("FAIL %s: got %s, want %s\n", what, got ? got : "(fine)", want ? want : "(fine)");
        ++failures;
    }
}

int main() {
    double nodes[2], pri[1], mx[1], scratch[1], u[1];
    int32_t leaves[1];
    float w[1], td[1];
    auto rec = [&](int depth, int64_t n_items, int K) {
        return per_sampler(nodes, depth, n_items, u, 1, 0.4, leaves, w, td, K, 0, 1e-3, 0.6, pri, mx, scratch);
    };
    const PerSampler ok = rec(4, 8, 2);
    if (ok.nodes != nodes || ok.uniforms != u || ok.leaves != leaves || ok.weights != w || ok.td_abs != td || ok.priorities != pri ||
        ok.max_dev != mx || ok.scratch != scratch || ok.n_items != 8.0 || ok.beta != 0.4 || ok.eps != 1e-3 || ok.alpha != 0.6 ||
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

    // the group check: members, batch 0 / 1 / 32 / 33, and every aliasing pair
    double n2[2], p2[1], m2[1], s2[1];
    int32_t l2[1];
    float w2[1], t2[1];
    auto member = [&](bool second) {
        idqn_per_step_t p;
        memset(&p, 0, sizeof(p));
        p.nodes_dev = second ? n2 : nodes; p.depth = 4; p.n_items = 8; p.uniforms_host = u; p.stratified = 1; p.beta = 0.4; p.eps = 1e-3;
        p.alpha = 0.6; p.max_priority_dev = second ? m2 : mx; p.leaves_dev = second ? l2 : leaves; p.weights_dev = second ? w2 : w;
        p.td_abs_dev = second ? t2 : td; p.priorities_dev = second ? p2 : pri; p.tree_scratch_dev = second ? s2 : scratch;
        return p;
    };
    int g = 0, j = 0;
    idqn_per_step_t per[2] = {member(false), member(true)};
    expect("group fine", per_group_args_error(per, 2, 32, 3, &g, &j), nullptr);
    expect("group null", per_group_args_error(nullptr, 2, 32, 3, &g, &j), "null pointer");
    for (int batch : {0, 1, 32, 33}) expect("group batch", per_group_args_error(per, 2, batch, 3, &g, &j), batch < 1 || batch > 32 ? "batch not in" : nullptr);
    for (int depth : {0, 1, 31, 32}) {
        per[1].depth = depth;
        expect("group depth", per_group_args_error(per, 2, 32, 3, &g, &j), depth < 1 || depth > 31 ? "depth" : nullptr);
        if ((depth < 1 || depth > 31) && (g != 1 || j != -1)) { printf("FAIL group depth: member %d / %d\n", g, j); ++failures; }
    }
    per[1] = member(true);
    per[1].n_items = 0;
    expect("group n_items 0", per_group_args_error(per, 2, 32, 3, &g, &j), "n_items < 1");
    per[1] = member(true);
    expect("group n_heads 0", per_group_args_error(per, 2, 32, 0, &g, &j), "n_heads < 1");
    float tau[1];
    per[0].tau_dev = tau;
    expect("group tau", per_group_args_error(per, 2, 32, 3, &g, &j), "tau_dev is set");
    per[0] = member(false);
    const char* names[] = {"nodes_dev", "leaves_dev", "weights_dev", "td_abs_dev", "tree_scratch_dev", "priorities_dev", "max_priority_dev"};
    for (int f = 0; f < 7; ++f) {
        per[1] = member(true);
        idqn_per_step_t &a = per[1], &b = per[0];
        switch (f) {
            case 0: a.nodes_dev = b.nodes_dev; break;
            case 1: a.leaves_dev = b.leaves_dev; break;
            case 2: a.weights_dev = b.weights_dev; break;
            case 3: a.td_abs_dev = b.td_abs_dev; break;
            case 4: a.tree_scratch_dev = b.tree_scratch_dev; break;
            case 5: a.priorities_dev = b.priorities_dev; break;
            default: a.max_priority_dev = b.max_priority_dev; break;
        }
        const char* got = per_group_args_error(per, 2, 32, 3, &g, &j);
        expect("group alias", got, names[f]);
        if (g != 1 || j != 0) { printf("FAIL group alias %s: members %d / %d\n", names[f], g, j); ++failures; }
    }
    per[1] = member(true);
    per[0].priorities_dev = per[1].priorities_dev = nullptr;  // two NULLs are not one buffer
    per[0].max_priority_dev = per[1].max_priority_dev = nullptr;
    expect("group: optional outputs both NULL", per_group_args_error(per, 2, 32, 3, &g, &j), nullptr);
    printf(failures ? "per_args_probe: %d FAILED\n" : "per_args_probe: ok\n", failures);
    return failures != 0;
}
