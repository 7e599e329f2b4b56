// One lock-step collection of a SEED GROUP: S independent ReplayBuffers (own rings, capacities, samplers and keys), each taking
// one new frame and its pending element rows -- replay_add_step's treatment (ONE pinned block -> ONE asynchronous copy -> ONE
// launch) for S separate buffers instead of the E time lines of one.  Included by replay.hip only.
//
// Block layout (host and device staging alike; `block_bytes` travel):
//   replay_group_member_t [S]           the member records, from byte 0 (the entry copies the caller's table there)
//   per member, anywhere behind them:   int32 [n_rows] destination element slots, then int32 [n_rows][8] the rows
//                                       (byte offset rows_offset, a multiple of 4)
//                                       uint8 [frame_bytes] the new frame (byte offset frame_offset, a multiple of 16)
// Grid (work items, S): workgroup (x, g) reads record g; x < chunks(g) copies a share of member g's frame, the next
// cdiv(8 * n_rows, 256) workgroups write its rows, the rest (the grid is as wide as the widest member needs) return.  Frame
// workgroups follow the tiers of k_replay_add_step -- 16 B per lane, else 4 B, else bytes -- chosen PER MEMBER from its
// frame_bytes and the alignment of its source and destination.  Plain vector stores, no atomics, nothing between workgroups:
// every output byte has one writer (a member's frame slot is one, its row slots are distinct, and no two members share a ring
// or a row table: checked by the host entry).  Like k_replay_add_step the kernel skips a write whose slot is out of range -- or
// whose source leaves the block -- rather than trusting the staged table.
#pragma once
#include "common.h"

#define REPLAY_GROUP_MAX_MEMBERS 32
#ifndef REPLAY_GROUP_MAX_ROWS
#error "replay.hip defines REPLAY_GROUP_MAX_ROWS (beside REPLAY_STEP_MAX_ROWS) before it includes this header"
#endif

// replay_group_member_t: include/idqn_hip.h
static_assert(sizeof(replay_group_member_t) == 64, "replay_group_member_t is 64 bytes on both sides of the ABI");

// a lane moves 16 B per iteration on the wide tier: two chunks cover an 84 x 84 frame in one iteration per lane
__host__ __device__ inline int replay_group_chunks(long frame_bytes) {
    const long c = (frame_bytes + 16 * 256 - 1) / (16 * 256);
    return (int)(c < 1 ? 1 : c > 8 ? 8 : c);
}

__global__ __launch_bounds__(256) void k_replay_group_add_step(const uint8_t* __restrict__ block, long block_bytes) {
    const replay_group_member_t m = reinterpret_cast<const replay_group_member_t*>(block)[blockIdx.y];
    const int chunks = m.frame_slot >= 0 ? replay_group_chunks(m.frame_bytes) : 0;
    const int x = blockIdx.x;
    if (x >= chunks) {  // the element rows: one int32 per lane
        const int i = (x - chunks) * 256 + threadIdx.x;
        if (i >= m.n_rows * 8 || m.n_rows > REPLAY_GROUP_MAX_ROWS) return;
        if (m.rows_offset < 0 || (m.rows_offset & 3) || m.rows_offset + (long)m.n_rows * 36 > block_bytes) return;
        const int32_t* table = reinterpret_cast<const int32_t*>(block + m.rows_offset);
        const long slot = table[i >> 3];
        if (slot < 0 || slot >= m.capacity) return;
        m.rows_dev[slot * 8 + (i & 7)] = table[m.n_rows + i];
        return;
    }
    if (m.frame_slot >= m.n_frames || m.frame_bytes < 1 || m.frame_offset < 0 || m.frame_offset + m.frame_bytes > block_bytes) return;
    const uint8_t* src = block + m.frame_offset;
    uint8_t* dst = reinterpret_cast<uint8_t*>(m.ring_dev) + (long)m.frame_slot * m.frame_bytes;
    const long tid = (long)x * 256 + threadIdx.x, nthr = (long)chunks * 256;
    if ((m.frame_bytes & 15) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (long i = tid; i < (m.frame_bytes >> 4); i += nthr) d4[i] = s4[i];
    } else if ((m.frame_bytes & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0) {
        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d1 = reinterpret_cast<uint32_t*>(dst);
        for (long i = tid; i < (m.frame_bytes >> 2); i += nthr) d1[i] = s1[i];
    } else {
        for (long i = tid; i < m.frame_bytes; i += nthr) dst[i] = src[i];
    }
}

// One VECTOR step of a seed group: S independent VectorReplayBuffers (segmented rings, replay_add_step's layout), each taking the
// n_in new frames, n_writes (source index, destination slot) pairs and n_rows element rows of one replay_add_step call -- that
// call's treatment for S separate buffers (include/idqn_hip.h, replay_group_add_many).
//
// Block layout (host and device staging alike; `block_bytes` travel):
//   replay_group_many_member_t [S]      the member records, from byte 0 (the entry copies the caller's table there)
//   per member, anywhere behind them:   int32 [n_writes][2] the pairs (pairs_offset, a multiple of 4)
//                                       int32 [n_rows] destination element slots, then int32 [n_rows][8] the rows (rows_offset, 4)
//                                       uint8 [n_in][frame_bytes] the new frames (frames_offset, a multiple of 16)
// Grid (work items, S): workgroup (x, g) reads record g (blockIdx.y is uniform: scalar loads of the 80 bytes); x < n_writes *
// chunks(g) copies share x % chunks of write x / chunks, the next cdiv(8 * n_rows, 256) workgroups write the rows, one int32 per
// lane, the rest (the grid is as wide as the widest member needs) return.  The three tiers -- 16 B per lane, else 4 B, else bytes
// -- are chosen PER WRITE from the member's frame_bytes and the alignment of that write's source and destination.  Plain vector
// stores, no LDS, no atomics, nothing between workgroups: every output byte has one writer (a member's destination ring slots are
// pairwise distinct, so are its element slots, and no two members share a ring or a row table: replay_group_many_args.h, checked
// by the entry).  The kernel skips a write whose slot is out of range or whose source or table leaves the block rather than
// trusting the staged block.
// (a pointer read from the record is a generic one to the compiler; the destinations are global memory: global stores, not flat)
#define REPLAY_GLOBAL __attribute__((address_space(1)))
typedef uint32_t replay_u32x4 __attribute__((ext_vector_type(4)));  // (uint4 is a class whose operator= takes generic pointers only)
static_assert(sizeof(replay_group_many_member_t) == 80, "replay_group_many_member_t is 80 bytes on both sides of the ABI");

__global__ __launch_bounds__(256) void k_replay_group_add_many(const uint8_t* __restrict__ block, long block_bytes) {
    const replay_group_many_member_t m = reinterpret_cast<const replay_group_many_member_t*>(block)[blockIdx.y];
    if (m.n_in < 0 || m.n_in > REPLAY_STEP_MAX_IN || m.n_writes < 0 || m.n_writes > REPLAY_STEP_MAX_WRITES || m.n_rows < 0 ||
        m.n_rows > REPLAY_STEP_MAX_ROWS || m.frame_bytes < 1 || m.frame_bytes > block_bytes)
        return;
    const int chunks = replay_group_chunks(m.frame_bytes);
    const int frame_blocks = m.n_writes * chunks;
    const int x = blockIdx.x;
    if (x >= frame_blocks) {  // the element rows: one int32 per lane
        const int i = (x - frame_blocks) * 256 + threadIdx.x;
        if (i >= m.n_rows * 8) return;
        if (m.rows_offset < 0 || (m.rows_offset & 3) || m.rows_offset + (long)m.n_rows * 36 > block_bytes) return;
        const int32_t* table = reinterpret_cast<const int32_t*>(block + m.rows_offset);
        const long slot = table[i >> 3];
        if (slot < 0 || slot >= m.capacity) return;
        ((REPLAY_GLOBAL int32_t*)m.rows_dev)[slot * 8 + (i & 7)] = table[m.n_rows + i];
        return;
    }
    const int w = x / chunks, c = x - w * chunks;
    if (m.pairs_offset < 0 || (m.pairs_offset & 3) || m.pairs_offset + (long)m.n_writes * 8 > block_bytes) return;
    const int32_t* pairs = reinterpret_cast<const int32_t*>(block + m.pairs_offset);
    const long src_i = pairs[2 * w], dst_i = pairs[2 * w + 1];
    if (src_i < 0 || src_i >= m.n_in || dst_i < 0 || dst_i >= m.n_frames) return;
    if (m.frames_offset < 0 || m.frames_offset > block_bytes || m.frames_offset + (src_i + 1) * m.frame_bytes > block_bytes) return;
    const uint8_t* src = block + m.frames_offset + src_i * m.frame_bytes;
    REPLAY_GLOBAL uint8_t* dst = (REPLAY_GLOBAL uint8_t*)m.ring_dev + dst_i * m.frame_bytes;
    const long tid = (long)c * 256 + threadIdx.x, nthr = (long)chunks * 256;
    if ((m.frame_bytes & 15) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const replay_u32x4* s4 = reinterpret_cast<const replay_u32x4*>(src);
        REPLAY_GLOBAL replay_u32x4* d4 = reinterpret_cast<REPLAY_GLOBAL replay_u32x4*>(dst);
        for (long i = tid; i < (m.frame_bytes >> 4); i += nthr) d4[i] = s4[i];
    } else if ((m.frame_bytes & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0) {
        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
        REPLAY_GLOBAL uint32_t* d1 = reinterpret_cast<REPLAY_GLOBAL uint32_t*>(dst);
        for (long i = tid; i < (m.frame_bytes >> 2); i += nthr) d1[i] = s1[i];
    } else {
        for (long i = tid; i < m.frame_bytes; i += nthr) dst[i] = src[i];
    }
}
