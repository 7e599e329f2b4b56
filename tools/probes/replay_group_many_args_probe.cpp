// Stand-alone host check of csrc/replay_group_many_args.h: valid tables, and every refusal of replay_group_add_many at its
// boundary -- NULL, counts out of range, misaligned blocks and offsets, offsets and slots outside their range, aliased destinations.
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I i-dqn_amd/csrc
//         tools/probes/replay_group_many_args_probe.cpp && ./a.out
// The block is allocated at its exact size, so a check that read past the bytes it was told about would trip the sanitizer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "replay_group_many_args.h"

static int failures = 0, checks = 0;
static void expect(const char* what, const char* got, const char* want) {
    const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
    ++checks;
    if (!ok) {
        printf("FAIL %s: got %s, want %s\n", what, got ? got : "(fine)", want ? want : "(fine)");
        ++failures;
    }
}

typedef replay_group_many_member_t rec_t;
static const int S = 3;
static const int64_t HEAD = S * (int64_t)sizeof(rec_t);
static uint8_t rings[S][64];
static int32_t rows[S][8 * 16];
static uint8_t* block;  // [BLOCK], 16-byte aligned, exactly BLOCK bytes
static uint8_t* dev;
static int64_t BLOCK;

// member g: frames of fb[g] bytes, n_in = 2, three writes (one mirror), two rows; tables then frames behind the records
static void fill(rec_t* m) {
    const int64_t fb[S] = {32, 36, 7};
    int64_t at = HEAD;
    memset(block, 0, (size_t)BLOCK);
    for (int g = 0; g < S; ++g) {
        m[g] = rec_t{rings[g], rows[g], 9, fb[g], 16, 2, 3, 2, 0, at, at + 24, 0};
        int32_t* t = (int32_t*)(block + at);
        const int32_t pairs[6] = {0, 3, 1, 8, 1, 0}, table[2] = {15, 0};
        memcpy(t, pairs, sizeof pairs);
        memcpy(t + 6, table, sizeof table);
        at += 24 + 2 * 36;
    }
    for (int g = 0; g < S; ++g) {
        at = (at + 15) & ~(int64_t)15;
        m[g].frames_offset = at;
        at += 2 * fb[g];
    }
    if (at != BLOCK) {
        printf("FAIL layout: %ld bytes used of %ld\n", (long)at, (long)BLOCK);
        ++failures;
    }
}

int main() {
    BLOCK = HEAD + S * 96;
    for (int64_t fb : {32, 36}) BLOCK = ((BLOCK + 15) & ~(int64_t)15) + 2 * fb;
    BLOCK = ((BLOCK + 15) & ~(int64_t)15) + 2 * 7;
    void* p = nullptr;
    if (posix_memalign(&p, 16, (size_t)BLOCK)) return 2;  // (exactly BLOCK bytes: the sanitizer's redzone starts where the block ends)
    block = (uint8_t*)p;
    if (posix_memalign(&p, 16, 16)) return 2;
    dev = (uint8_t*)p;  // (only its address is looked at)
    uint8_t* const base = block;
    rec_t m[S + 1];
    int g, j;
    auto run = [&](int n = S, const rec_t* recs = nullptr, const void* host = nullptr, const void* d = nullptr, int64_t bytes = -1) {
        return replay_group_many_args_error(n, recs ? recs : m, host ? host : block, d ? d : dev, bytes < 0 ? BLOCK : bytes, &g, &j);
    };
    fill(m);
    expect("valid", run(), nullptr);
    expect("valid, one member", run(1), nullptr);
    // NULL
    expect("null members", replay_group_many_args_error(S, nullptr, block, dev, BLOCK, &g, &j), "null pointer");
    expect("null host block", replay_group_many_args_error(S, m, nullptr, dev, BLOCK, &g, &j), "null pointer");
    expect("null device block", replay_group_many_args_error(S, m, block, nullptr, BLOCK, &g, &j), "null pointer");
    m[1].ring_dev = nullptr;
    expect("null ring", run(), "null ring or rows");
    fill(m);
    m[2].rows_dev = nullptr;
    expect("null rows", run(), "null ring or rows");
    // counts
    fill(m);
    for (int n : {0, 1, 3, 33, -1}) expect("n_members", run(n), n < 1 || n > 32 ? "outside [1, 32]" : nullptr);
    fill(m);
    for (int v : {-1, 0, 2, 32, 33}) {
        fill(m);
        m[0].n_in = v;
        expect("n_in", run(), v < 0 || v > 32 ? "n_in is outside" : v == 0 ? "writes without a frame" : v == 2 ? nullptr : "the frames");
    }
    for (int v : {-1, 65}) {
        fill(m);
        m[1].n_writes = v;
        expect("n_writes", run(), "n_writes is outside");
    }
    for (int v : {-1, 129}) {
        fill(m);
        m[1].n_rows = v;
        expect("n_rows", run(), "n_rows is outside");
    }
    fill(m);
    m[2].n_writes = m[2].n_rows = 0;
    expect("empty member", run(), "neither a write nor a row");
    fill(m);
    m[0].n_writes = 0;  // rows only, then frames only
    expect("rows only", run(), nullptr);
    fill(m);
    m[0].n_rows = 0;
    expect("writes only", run(), nullptr);
    for (int64_t v : {(int64_t)0, (int64_t)-1}) {
        fill(m);
        m[0].n_frames = v;
        expect("n_frames", run(), "must be positive");
        fill(m);
        m[0].frame_bytes = v;
        expect("frame_bytes", run(), "must be positive");
        fill(m);
        m[0].capacity = v;
        expect("capacity", run(), "must be positive");
    }
    // alignment
    fill(m);
    expect("misaligned host block", run(S, nullptr, block + 4), "16-byte aligned");
    expect("misaligned device block", run(S, nullptr, nullptr, dev + 8), "16-byte aligned");
    m[0].rows_dev = (int32_t*)((uint8_t*)rows[0] + 2);
    expect("misaligned rows_dev", run(), "4-byte aligned");
    fill(m);
    m[1].pairs_offset += 2;
    expect("misaligned pair table", run(), "pair table");
    fill(m);
    m[1].rows_offset += 1;
    expect("misaligned row table", run(), "row table");
    fill(m);
    m[1].frames_offset += 4;
    expect("misaligned frames", run(), "the frames");
    // offsets outside the block
    fill(m);
    expect("block below the records", run(S, nullptr, nullptr, nullptr, HEAD - 1), "block_bytes");
    expect("block above 2^31", run(S, nullptr, nullptr, nullptr, ((int64_t)1 << 31) + 16), "block_bytes");
    for (int64_t v : {(int64_t)-8, HEAD - 8, BLOCK - 16, BLOCK, (int64_t)1 << 40, INT64_MAX - 3}) {
        fill(m);
        m[0].pairs_offset = v;
        expect("pair table outside", run(), "pair table");
        fill(m);
        m[0].rows_offset = v;
        expect("row table outside", run(), "row table");
    }
    for (int64_t v : {(int64_t)-16, (int64_t)0, BLOCK - 48, BLOCK, (int64_t)1 << 40, INT64_MAX - 15}) {
        fill(m);
        m[0].frames_offset = v;
        expect("frames outside", run(), "the frames");
    }
    fill(m);
    m[2].frame_bytes = BLOCK + 1;
    expect("frame larger than the block", run(), "the frames");
    fill(m);
    m[2].frame_bytes = INT64_MAX / 2;
    expect("frame_bytes * n_in overflows", run(), "the frames");
    fill(m);
    expect("block one byte short", run(S, nullptr, nullptr, nullptr, BLOCK - 1), "the frames");
    // slots and sources
    for (int32_t v : {-1, 2}) {
        fill(m);
        ((int32_t*)(block + m[1].pairs_offset))[2] = v;
        expect("source index", run(), "source index");
    }
    for (int32_t v : {-1, 9}) {
        fill(m);
        ((int32_t*)(block + m[1].pairs_offset))[5] = v;
        expect("ring slot", run(), "ring slot is outside");
    }
    for (int32_t v : {-1, 16}) {
        fill(m);
        ((int32_t*)(block + m[2].rows_offset))[1] = v;
        expect("element slot", run(), "element slot is outside");
    }
    // aliased destinations
    fill(m);
    ((int32_t*)(block + m[1].pairs_offset))[5] = 3;
    expect("ring slot twice", run(), "ring slot is written twice");
    if (g != 1) expect("ring slot twice: member", "member", "1");
    fill(m);
    ((int32_t*)(block + m[2].rows_offset))[1] = 15;
    expect("element slot twice", run(), "element slot is written twice");
    fill(m);
    m[2].ring_dev = m[0].ring_dev;
    expect("shared ring", run(), "same ring");
    if (g != 2 || j != 0) expect("shared ring: members", "(g, j)", "(2, 0)");
    fill(m);
    m[2].rows_dev = m[1].rows_dev;
    expect("shared rows", run(), "same rows");
    if (g != 2 || j != 1) expect("shared rows: members", "(g, j)", "(2, 1)");
    fill(m);
    m[1].ring_dev = m[0].rows_dev;
    expect("ring is another's rows", run(), "another member's rows");
    // the records at the head of the block itself, as the collector passes them
    fill(m);
    memcpy(block, m, (size_t)HEAD);
    expect("records in the block", run(S, (const rec_t*)block), nullptr);
    // 32 members with the largest tables
    {
        const int N = 32;
        const int64_t head = N * (int64_t)sizeof(rec_t), per = 64 * 8 + 128 * 36, bytes = head + N * per + 16 * N;
        if (posix_memalign(&p, 16, (size_t)bytes)) return 2;
        uint8_t* big = (uint8_t*)p;
        static uint8_t r[N][16];
        static int32_t t[N][4];
        rec_t recs[N];
        for (int i = 0; i < N; ++i) {
            const int64_t at = head + i * per;
            recs[i] = rec_t{r[i], t[i], 64, 16, 128, 1, 64, 128, 0, at, at + 512, head + N * per + 16 * i};
            int32_t* p = (int32_t*)(big + at);
            for (int w = 0; w < 64; ++w) p[2 * w] = 0, p[2 * w + 1] = w;
            for (int k = 0; k < 128; ++k) p[128 + k] = 127 - k;
            memset(p + 256, 0, 128 * 32);
        }
        expect("32 full members", replay_group_many_args_error(N, recs, big, dev, bytes, &g, &j), nullptr);
        ((int32_t*)(big + recs[31].rows_offset))[127] = 127;
        expect("32 full members, last slot twice", replay_group_many_args_error(N, recs, big, dev, bytes, &g, &j), "element slot is written twice");
        free(big);
    }
    free(base);
    free(dev);
    printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures != 0;
}
