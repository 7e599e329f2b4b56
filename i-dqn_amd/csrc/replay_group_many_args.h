// Argument, range and aliasing checks of replay_group_add_many (replay.hip) on the S member records of a call and on the tables
// the caller staged in the pinned block.  Plain host C++ without a HIP dependency, as per_group_args.h: NULL when the call is
// fine, else the refusal text with the member it is about in *g_out (and *j_out: the earlier member that names the same buffer,
// else -1), so that the entry can refuse before it enqueues anything and before it writes the block.  Nothing is written here.
#pragma once
#include "../../include/idqn_hip.h"

#define REPLAY_MANY_MAX_MEMBERS 32
#define REPLAY_MANY_MAX_IN 32       // per member: the limits of replay_add_step (replay.hip asserts that they are the same numbers)
#define REPLAY_MANY_MAX_WRITES 64
#define REPLAY_MANY_MAX_ROWS 128
#define REPLAY_MANY_MAX_BLOCK ((int64_t)1 << 31)

// [offset, offset + bytes) lies behind the records and inside the block, at a multiple of `align`
static inline bool replay_many_inside(int64_t offset, int64_t bytes, int64_t align, int64_t head, int64_t block_bytes) {
    return offset >= head && (offset & (align - 1)) == 0 && bytes <= block_bytes && offset <= block_bytes - bytes;
}

static inline const char* replay_group_many_args_error(int32_t n_members, const replay_group_many_member_t* members, const void* block_host,
                                                       const void* block_dev, int64_t block_bytes, int* g_out, int* j_out) {
    *g_out = -1;
    *j_out = -1;
    if (!members || !block_host || !block_dev) return "null pointer";
    if (n_members < 1 || n_members > REPLAY_MANY_MAX_MEMBERS) return "the number of members is outside [1, 32]";
    if ((((uintptr_t)block_host | (uintptr_t)block_dev) & 15) != 0) return "the blocks must be 16-byte aligned";
    const int64_t head = (int64_t)n_members * (int64_t)sizeof(replay_group_many_member_t);
    if (block_bytes < head || block_bytes > REPLAY_MANY_MAX_BLOCK) return "block_bytes is below the bytes of the records, or above 2^31";
    const uint8_t* block = (const uint8_t*)block_host;
    for (int g = 0; g < n_members; ++g) {
        const replay_group_many_member_t& m = members[g];
        *g_out = g;
        if (!m.ring_dev || !m.rows_dev) return "null ring or rows";
        if (((uintptr_t)m.rows_dev & 3) != 0) return "rows_dev must be 4-byte aligned";
        if (m.n_frames < 1 || m.frame_bytes < 1 || m.capacity < 1) return "n_frames, frame_bytes and capacity must be positive";
        if (m.n_in < 0 || m.n_in > REPLAY_MANY_MAX_IN) return "n_in is outside [0, 32]";
        if (m.n_writes < 0 || m.n_writes > REPLAY_MANY_MAX_WRITES) return "n_writes is outside [0, 64]";
        if (m.n_rows < 0 || m.n_rows > REPLAY_MANY_MAX_ROWS) return "n_rows is outside [0, 128]";
        if (m.n_writes + m.n_rows < 1) return "neither a write nor a row";
        if (m.n_writes > 0 && m.n_in < 1) return "writes without a frame";
        if (m.n_in > 0) {
            if (m.frame_bytes > block_bytes || !replay_many_inside(m.frames_offset, (int64_t)m.n_in * m.frame_bytes, 16, head, block_bytes))
                return "the frames (16-byte aligned, behind the records) leave the block";
        }
        if (m.n_writes > 0) {
            if (!replay_many_inside(m.pairs_offset, (int64_t)m.n_writes * 8, 4, head, block_bytes))
                return "the pair table (4-byte aligned, behind the records) leaves the block";
            const int32_t* pairs = (const int32_t*)(block + m.pairs_offset);
            for (int w = 0; w < m.n_writes; ++w) {
                const int32_t src = pairs[2 * w], dst = pairs[2 * w + 1];
                if (src < 0 || src >= m.n_in) return "a write's source index is outside [0, n_in)";
                if (dst < 0 || dst >= m.n_frames) return "a write's ring slot is outside [0, n_frames)";
                for (int v = 0; v < w; ++v)
                    if (pairs[2 * v + 1] == dst) return "a ring slot is written twice";
            }
        }
        if (m.n_rows > 0) {
            if (!replay_many_inside(m.rows_offset, (int64_t)m.n_rows * 36, 4, head, block_bytes))
                return "the row table (4-byte aligned, behind the records) leaves the block";
            const int32_t* slots = (const int32_t*)(block + m.rows_offset);
            for (int r = 0; r < m.n_rows; ++r) {
                if (slots[r] < 0 || slots[r] >= m.capacity) return "a row's element slot is outside [0, capacity)";
                for (int v = 0; v < r; ++v)
                    if (slots[v] == slots[r]) return "an element slot is written twice";
            }
        }
        for (int j = 0; j < g; ++j) {
            const replay_group_many_member_t& o = members[j];
            const char* bad = nullptr;
            if (o.ring_dev == m.ring_dev) bad = "two members name the same ring: one buffer would have two writers";
            else if ((void*)o.rows_dev == (void*)m.rows_dev) bad = "two members name the same rows: one buffer would have two writers";
            else if (o.ring_dev == (void*)m.rows_dev || (void*)o.rows_dev == m.ring_dev)
                bad = "one member's ring is another member's rows: one buffer would have two writers";
            if (bad) {
                *j_out = j;
                return bad;
            }
        }
    }
    *g_out = -1;
    return nullptr;
}
