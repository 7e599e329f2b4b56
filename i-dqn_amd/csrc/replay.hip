// HBM replay store: gather of sampled slots into a contiguous minibatch.
//
// Replaces the fetch + unpack + np.stack of ReplayBuffer.sample (reference
// slimdqn/sample_collection/replay_buffer.py:223-229): the reference keeps snappy-compressed
// elements in a host OrderedDict; here every element's (state, next_state) pair sits uncompressed in
// HBM at slot = key % capacity, so the "decompress + stack" is a pure row gather.  HBM-bound byte
// copy: 2 * n * obs_bytes read + written, 16 B per lane, one workgroup per (sample, half).
#include "common.h"
#include <algorithm>

__global__ __launch_bounds__(256) void k_replay_gather(const uint8_t* __restrict__ store, long obs_bytes,
                                                       const int32_t* __restrict__ slots, uint8_t* __restrict__ s_out,
                                                       uint8_t* __restrict__ n_out) {
    const int b = blockIdx.x, half = blockIdx.y;
    const uint8_t* src = store + ((long)slots[b] * 2 + half) * obs_bytes;
    uint8_t* dst = (half ? n_out : s_out) + (long)b * obs_bytes;
    const long nvec = obs_bytes >> 4;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (long i = threadIdx.x; i < nvec; i += 256) d4[i] = s4[i];
        for (long i = (nvec << 4) + threadIdx.x; i < obs_bytes; i += 256) dst[i] = src[i];
    } else {
        for (long i = threadIdx.x; i < obs_bytes; i += 256) dst[i] = src[i];
    }
}

__global__ void k_replay_gather_scalars(const int32_t* __restrict__ a_store, const float* __restrict__ r_store,
                                        const uint8_t* __restrict__ t_store, const int32_t* __restrict__ slots, int n,
                                        int32_t* __restrict__ a_out, float* __restrict__ r_out,
                                        uint8_t* __restrict__ t_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = slots[i];
    a_out[i] = a_store[s];
    r_out[i] = r_store[s];
    t_out[i] = t_store[s];
}

// ---------------------------------------------------------------------------------------------------
// Frame-ring store: every environment frame is written to HBM ONCE (ring slot = transition index % n_frames);
// a replay element is 8 int32 of metadata and its frame stacks are assembled at sample time -- the device-side
// counterpart of the reference's stack building (replay_buffer.py:119-137: `state[..., ch] = observation`, zero
// frames before the episode start) fused with the gather + np.stack of sample() (:223-229).
// meta row: {newest state frame slot, valid state frames, newest next_state frame slot, valid next frames,
//            action, reward (f32 bits), terminal, 0}.
// Output element (pixel, ch) of a stack = frame[newest - (stack-1-ch)][pixel], or 0 where ch < stack - valid.
// grid (sample, state|next, chunk); the uint8 x 4-stack case packs one u32 per pixel (16 B per lane).
__global__ __launch_bounds__(256) void k_replay_gather_stacked(const uint8_t* __restrict__ frames, long n_frames,
                                                               long frame_elems, int itemsize, int stack,
                                                               const int32_t* __restrict__ meta,
                                                               const int32_t* __restrict__ slots,
                                                               uint8_t* __restrict__ s_out, uint8_t* __restrict__ n_out,
                                                               int32_t* __restrict__ a_out, float* __restrict__ r_out,
                                                               uint8_t* __restrict__ t_out) {
    const int b = blockIdx.x, half = blockIdx.y;
    const int32_t* m = meta + (long)slots[b] * 8;
    const long newest = m[2 * half], valid = m[2 * half + 1];
    const long frame_bytes = frame_elems * itemsize;
    uint8_t* dst = (half ? n_out : s_out) + (long)b * frame_bytes * stack;
    if (half == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
        a_out[b] = m[4];
        r_out[b] = __int_as_float(m[5]);
        t_out[b] = (uint8_t)m[6];
    }
    const long tid = (long)blockIdx.z * 256 + threadIdx.x, nthr = (long)gridDim.z * 256;
    if (itemsize == 1 && stack == 4 && (frame_bytes & 15) == 0 && ((uintptr_t)frames & 15) == 0 && ((uintptr_t)dst & 15) == 0) {
        const uint4* f[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const long back = 3 - ch;
            f[ch] = back < valid ? reinterpret_cast<const uint4*>(frames + ((newest - back + n_frames) % n_frames) * frame_bytes)
                                 : nullptr;
        }
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        for (long i = tid; i < (frame_bytes >> 4); i += nthr) {  // 16 pixels per lane: 4 x 16 B in, 64 B out
            uint4 v[4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) v[ch] = f[ch] ? f[ch][i] : zero;
            const uint32_t w[4][4] = {{v[0].x, v[1].x, v[2].x, v[3].x}, {v[0].y, v[1].y, v[2].y, v[3].y},
                                      {v[0].z, v[1].z, v[2].z, v[3].z}, {v[0].w, v[1].w, v[2].w, v[3].w}};
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // 4 pixels x 4 channels: byte transpose of a 4 x 4 block
                const uint32_t a = w[g][0], b = w[g][1], c = w[g][2], d = w[g][3];
                uint4 o;
                o.x = (a & 0xff) | ((b & 0xff) << 8) | ((c & 0xff) << 16) | (d << 24);
                o.y = ((a >> 8) & 0xff) | (b & 0xff00) | ((c & 0xff00) << 8) | ((d & 0xff00) << 16);
                o.z = ((a >> 16) & 0xff) | ((b >> 8) & 0xff00) | (c & 0xff0000) | ((d & 0xff0000) << 8);
                o.w = (a >> 24) | ((b >> 16) & 0xff00) | ((c >> 8) & 0xff0000) | (d & 0xff000000);
                d4[4 * i + g] = o;
            }
        }
        return;
    }
    if (itemsize == 1 && stack == 4 && (frame_bytes & 3) == 0 && ((uintptr_t)frames & 3) == 0 && ((uintptr_t)dst & 15) == 0) {
        const uint32_t* f[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const long back = 3 - ch;
            f[ch] = back < valid ? reinterpret_cast<const uint32_t*>(frames + ((newest - back + n_frames) % n_frames) * frame_bytes)
                                 : nullptr;
        }
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (long i = tid; i < (frame_bytes >> 2); i += nthr) {  // 4 pixels per lane
            const uint32_t a = f[0] ? f[0][i] : 0u, b = f[1] ? f[1][i] : 0u, c = f[2] ? f[2][i] : 0u, d = f[3] ? f[3][i] : 0u;
            uint4 o;
            o.x = (a & 0xff) | ((b & 0xff) << 8) | ((c & 0xff) << 16) | (d << 24);
            o.y = ((a >> 8) & 0xff) | (b & 0xff00) | ((c & 0xff00) << 8) | ((d & 0xff00) << 16);
            o.z = ((a >> 16) & 0xff) | ((b >> 8) & 0xff00) | (c & 0xff0000) | ((d & 0xff0000) << 8);
            o.w = (a >> 24) | ((b >> 16) & 0xff00) | ((c >> 8) & 0xff0000) | (d & 0xff000000);
            d4[i] = o;
        }
        return;
    }
    const long total = frame_bytes * stack;  // generic: any element size / stack depth, one byte per iteration
    for (long o = tid; o < total; o += nthr) {
        const long e = o / itemsize, byte = o - e * itemsize;
        const long pix = e / stack, ch = e - pix * stack, back = stack - 1 - ch;
        uint8_t v = 0;
        if (back < valid) v = frames[((newest - back + n_frames) % n_frames) * frame_bytes + pix * itemsize + byte];
        dst[o] = v;
    }
}

extern "C" int replay_gather_stacked(const uint8_t* frames_dev, int64_t n_frames, int64_t frame_elems, int32_t itemsize,
                                     int32_t stack, const int32_t* meta_dev, const int32_t* slots_dev, int32_t n,
                                     uint8_t* state_out_dev, uint8_t* next_state_out_dev, int32_t* action_out_dev,
                                     float* reward_out_dev, uint8_t* terminal_out_dev, void* stream) {
    IDQN_REQUIRE(frames_dev && meta_dev && slots_dev && state_out_dev && next_state_out_dev && action_out_dev &&
                     reward_out_dev && terminal_out_dev, "replay_gather_stacked: null pointer");
    IDQN_REQUIRE(n >= 1 && n_frames >= 1 && frame_elems >= 1 && itemsize >= 1 && itemsize <= 16 && stack >= 1 && stack <= 64,
                 "replay_gather_stacked: n = %d, n_frames = %ld, frame_elems = %ld, itemsize = %d, stack = %d", n,
                 (long)n_frames, (long)frame_elems, itemsize, stack);
    const long bytes = (long)frame_elems * itemsize * stack;
    // one iteration per lane where possible: a lane emits 64 B (16 pixels x 4 channels) on the packed path
    const int chunks = (int)std::min<long>(16, std::max<long>(1, (bytes + 64 * 256 - 1) / (64 * 256)));
    hipLaunchKernelGGL(k_replay_gather_stacked, dim3(n, 2, chunks), dim3(256), 0, (hipStream_t)stream, frames_dev,
                       (long)n_frames, (long)frame_elems, itemsize, stack, meta_dev, slots_dev, state_out_dev,
                       next_state_out_dev, action_out_dev, reward_out_dev, terminal_out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int replay_gather(const uint8_t* store_dev, int64_t obs_bytes, const int32_t* slots_dev, int32_t n,
                             uint8_t* state_out_dev, uint8_t* next_state_out_dev, void* stream) {
    IDQN_REQUIRE(store_dev && slots_dev && state_out_dev && next_state_out_dev, "replay_gather: null pointer");
    IDQN_REQUIRE(n >= 1 && obs_bytes >= 1, "replay_gather: n = %d, obs_bytes = %ld", n, (long)obs_bytes);
    hipLaunchKernelGGL(k_replay_gather, dim3(n, 2), dim3(256), 0, (hipStream_t)stream, store_dev, (long)obs_bytes,
                       slots_dev, state_out_dev, next_state_out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int replay_gather_scalars(const int32_t* action_store_dev, const float* reward_store_dev,
                                     const uint8_t* terminal_store_dev, const int32_t* slots_dev, int32_t n,
                                     int32_t* action_out_dev, float* reward_out_dev, uint8_t* terminal_out_dev,
                                     void* stream) {
    IDQN_REQUIRE(action_store_dev && reward_store_dev && terminal_store_dev && slots_dev && n >= 1,
                 "replay_gather_scalars: bad arguments");
    hipLaunchKernelGGL(k_replay_gather_scalars, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       action_store_dev, reward_store_dev, terminal_store_dev, slots_dev, n, action_out_dev,
                       reward_out_dev, terminal_out_dev);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// ReplayBuffer.add's device half (slimdqn/sample_collection/replay_buffer.py:206-213: the reference stores the
// transition on the host): the newest frame goes from a PINNED host staging slot to its slot of the frame ring in HBM,
// asynchronously on the caller's stream.  The caller owns the reuse discipline of the staging slots.
extern "C" int replay_add_frame(void* frame_ring_dev, int64_t slot, int64_t frame_bytes, const void* frame_host_pinned,
                                void* stream) {
    IDQN_REQUIRE(frame_ring_dev && frame_host_pinned && slot >= 0 && frame_bytes > 0, "replay_add_frame: bad arguments");
    IDQN_HIP_CHECK(hipMemcpyAsync((char*)frame_ring_dev + slot * frame_bytes, frame_host_pinned, (size_t)frame_bytes,
                                  hipMemcpyHostToDevice, (hipStream_t)stream));
    return IDQN_OK;
}

// Growing the frame ring (rare: element-less transitions used up the slack): the live frames, transition indices
// [first_t, first_t + count), move from slot t % old_n of the old ring to slot t % new_n of the new one.
__global__ __launch_bounds__(256) void k_ring_regrow(const uint8_t* __restrict__ old_ring, long old_n,
                                                     uint8_t* __restrict__ new_ring, long new_n, long first_t,
                                                     long frame_bytes) {
    const long t = first_t + blockIdx.x;
    const uint8_t* src = old_ring + (t % old_n) * frame_bytes;
    uint8_t* dst = new_ring + (t % new_n) * frame_bytes;
    if ((frame_bytes & 15) == 0 && (((uintptr_t)old_ring | (uintptr_t)new_ring) & 15) == 0) {
        for (long i = threadIdx.x; i < frame_bytes / 16; i += 256)
            reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    } else {
        for (long i = threadIdx.x; i < frame_bytes; i += 256) dst[i] = src[i];
    }
}

extern "C" int replay_ring_regrow(const void* old_ring_dev, int64_t old_n, void* new_ring_dev, int64_t new_n,
                                  int64_t first_t, int64_t count, int64_t frame_bytes, void* stream) {
    IDQN_REQUIRE(old_ring_dev && new_ring_dev && old_ring_dev != new_ring_dev, "replay_ring_regrow: two distinct rings required");
    IDQN_REQUIRE(old_n >= 1 && new_n >= old_n && first_t >= 0 && count >= 0 && count <= old_n && frame_bytes >= 1,
                 "replay_ring_regrow: old_n = %ld, new_n = %ld, first_t = %ld, count = %ld, frame_bytes = %ld", (long)old_n,
                 (long)new_n, (long)first_t, (long)count, (long)frame_bytes);
    for (int64_t done = 0; done < count; done += 1 << 30) {  // grid.x limit; one launch in practice
        const int64_t n = std::min<int64_t>(count - done, 1 << 30);
        hipLaunchKernelGGL(k_ring_regrow, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)old_ring_dev,
                           (long)old_n, (uint8_t*)new_ring_dev, (long)new_n, (long)(first_t + done), (long)frame_bytes);
        IDQN_HIP_CHECK(hipGetLastError());
    }
    return IDQN_OK;
}

// One vector-environment step of the segmented frame ring (VectorReplayBuffer: E time lines, each in a segment of its own
// with its last stack-1 frames mirrored below the segment's first main slot, so that every stack is `stack` CONSECUTIVE slots
// and the gathers above read it as they are): ONE pinned block -> ONE asynchronous copy -> ONE launch that scatters every new
// frame to its one or two ring slots and every new element row to rows_dev.  Block layout (host and device staging alike):
//   int32 [2 * REPLAY_STEP_MAX_WRITES]   (source frame index, destination ring slot) pairs, n_writes used
//   int32 [REPLAY_STEP_MAX_ROWS]         destination element slots, n_rows used
//   int32 [REPLAY_STEP_MAX_ROWS][8]      the new rows
//   uint8 [n_in][frame_bytes]            the new frames (byte offset REPLAY_STEP_HEADER_BYTES, a multiple of 16)
// Frame workgroups follow the tiers of k_replay_gather_stacked: 16 B per lane, else 4 B, else bytes.  Row workgroups are their
// own (blockIdx.x >= n_writes * chunks).  Plain vector stores, no atomics; destinations are distinct (checked by the host
// entry), and the kernel skips a pair or a row whose index is out of range rather than trusting the staged table.
#define REPLAY_STEP_MAX_IN 32
#define REPLAY_STEP_MAX_WRITES 64
#define REPLAY_STEP_MAX_ROWS 128
#define REPLAY_GROUP_MAX_ROWS 32  // replay_group_add_step (replay_group_kernels.h): rows per MEMBER and call -- a lock-step add makes
                                  // one row, an episode end update_horizon of them; a member with more sends them itself first
#define REPLAY_STEP_HEADER_BYTES ((2 * REPLAY_STEP_MAX_WRITES + REPLAY_STEP_MAX_ROWS + 8 * REPLAY_STEP_MAX_ROWS) * 4)

__global__ __launch_bounds__(256) void k_replay_add_step(const uint8_t* __restrict__ block, uint8_t* __restrict__ ring,
                                                         long n_frames, long frame_bytes, int32_t* __restrict__ rows_out,
                                                         long capacity, int n_in, int n_writes, int n_rows, int chunks) {
    const int32_t* table = reinterpret_cast<const int32_t*>(block);
    const int frame_blocks = n_writes * chunks;
    if ((int)blockIdx.x >= frame_blocks) {  // the element rows: one int32 per lane
        const int i = ((int)blockIdx.x - frame_blocks) * 256 + threadIdx.x;
        if (i >= n_rows * 8) return;
        const long slot = table[2 * REPLAY_STEP_MAX_WRITES + (i >> 3)];
        if (slot < 0 || slot >= capacity) return;
        rows_out[slot * 8 + (i & 7)] = table[2 * REPLAY_STEP_MAX_WRITES + REPLAY_STEP_MAX_ROWS + i];
        return;
    }
    const int w = blockIdx.x / chunks, c = blockIdx.x - w * chunks;
    const long src_i = table[2 * w], dst_i = table[2 * w + 1];
    if (src_i < 0 || src_i >= n_in || dst_i < 0 || dst_i >= n_frames) return;
    const uint8_t* src = block + REPLAY_STEP_HEADER_BYTES + src_i * frame_bytes;
    uint8_t* dst = ring + dst_i * frame_bytes;
    const long tid = (long)c * 256 + threadIdx.x, nthr = (long)chunks * 256;
    if ((frame_bytes & 15) == 0 && (((uintptr_t)block | (uintptr_t)ring) & 15) == 0) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (long i = tid; i < (frame_bytes >> 4); i += nthr) d4[i] = s4[i];
    } else if ((frame_bytes & 3) == 0 && (((uintptr_t)block | (uintptr_t)ring) & 3) == 0) {
        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d1 = reinterpret_cast<uint32_t*>(dst);
        for (long i = tid; i < (frame_bytes >> 2); i += nthr) d1[i] = s1[i];
    } else {
        for (long i = tid; i < frame_bytes; i += nthr) dst[i] = src[i];
    }
}

extern "C" int replay_add_step(void* frame_ring_dev, int64_t n_frames, int64_t frame_bytes, int32_t* rows_dev, int64_t capacity,
                               const void* block_host_pinned, void* block_staging_dev, int32_t n_in, int32_t n_writes,
                               int32_t n_rows, void* stream) {
    IDQN_REQUIRE(frame_ring_dev && rows_dev && block_host_pinned && block_staging_dev, "replay_add_step: null pointer");
    IDQN_REQUIRE(n_frames >= 1 && frame_bytes >= 1 && capacity >= 1 && n_in >= 0 && n_in <= REPLAY_STEP_MAX_IN && n_writes >= 0 &&
                     n_writes <= REPLAY_STEP_MAX_WRITES && n_rows >= 0 && n_rows <= REPLAY_STEP_MAX_ROWS && n_writes + n_rows >= 1 &&
                     (n_writes == 0 || n_in >= 1),
                 "replay_add_step: n_frames = %ld, frame_bytes = %ld, capacity = %ld, n_in = %d (<= %d), n_writes = %d (<= %d), "
                 "n_rows = %d (<= %d)", (long)n_frames, (long)frame_bytes, (long)capacity, n_in, REPLAY_STEP_MAX_IN, n_writes,
                 REPLAY_STEP_MAX_WRITES, n_rows, REPLAY_STEP_MAX_ROWS);
    IDQN_REQUIRE(((uintptr_t)block_host_pinned & 3) == 0 && ((uintptr_t)block_staging_dev & 3) == 0 && ((uintptr_t)rows_dev & 3) == 0,
                 "replay_add_step: the blocks and rows_dev must be 4-byte aligned");
    const int32_t* table = (const int32_t*)block_host_pinned;
    for (int w = 0; w < n_writes; ++w) {
        const int32_t src = table[2 * w], dst = table[2 * w + 1];
        IDQN_REQUIRE(src >= 0 && src < n_in && dst >= 0 && dst < n_frames,
                     "replay_add_step: write %d = (source %d, slot %d) outside n_in = %d / n_frames = %ld", w, src, dst, n_in,
                     (long)n_frames);
        for (int v = 0; v < w; ++v)
            IDQN_REQUIRE(table[2 * v + 1] != dst, "replay_add_step: ring slot %d is written twice", dst);
    }
    const int32_t* row_slots = table + 2 * REPLAY_STEP_MAX_WRITES;
    for (int r = 0; r < n_rows; ++r) {
        IDQN_REQUIRE(row_slots[r] >= 0 && row_slots[r] < capacity, "replay_add_step: row %d goes to slot %d outside capacity = %ld", r,
                     row_slots[r], (long)capacity);
        for (int v = 0; v < r; ++v) IDQN_REQUIRE(row_slots[v] != row_slots[r], "replay_add_step: element slot %d is written twice", row_slots[r]);
    }
    IDQN_HIP_CHECK(hipMemcpyAsync(block_staging_dev, block_host_pinned, (size_t)REPLAY_STEP_HEADER_BYTES + (size_t)n_in * frame_bytes,
                                  hipMemcpyHostToDevice, (hipStream_t)stream));
    // a lane moves 16 B per iteration on the wide tier: two chunks cover an 84 x 84 frame in one iteration per lane
    const int chunks = (int)std::min<long>(8, std::max<long>(1, (frame_bytes + 16 * 256 - 1) / (16 * 256)));
    const int blocks = n_writes * chunks + cdiv((long)n_rows * 8, 256);
    hipLaunchKernelGGL(k_replay_add_step, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)block_staging_dev,
                       (uint8_t*)frame_ring_dev, (long)n_frames, (long)frame_bytes, rows_dev, (long)capacity, n_in, n_writes, n_rows,
                       chunks);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// The S replay adds of a lock-step iteration of a seed group as one call (include/idqn_hip.h, replay_group_add_step).
#include "replay_group_kernels.h"

extern "C" int replay_group_add_step(int32_t n_members, const replay_group_member_t* members, void* block_host_pinned,
                                     void* block_staging_dev, int64_t block_bytes, void* stream) {
    IDQN_REQUIRE(members && block_host_pinned && block_staging_dev, "replay_group_add_step: null pointer");
    IDQN_REQUIRE(n_members >= 1 && n_members <= REPLAY_GROUP_MAX_MEMBERS, "replay_group_add_step: %d members outside [1, %d]", n_members,
                 REPLAY_GROUP_MAX_MEMBERS);
    IDQN_REQUIRE(((uintptr_t)block_host_pinned & 15) == 0 && ((uintptr_t)block_staging_dev & 15) == 0,
                 "replay_group_add_step: the blocks must be 16-byte aligned");
    const int64_t head = (int64_t)n_members * (int64_t)sizeof(replay_group_member_t);
    IDQN_REQUIRE(block_bytes >= head && block_bytes <= ((int64_t)1 << 31), "replay_group_add_step: block_bytes = %ld below the %ld bytes of the records",
                 (long)block_bytes, (long)head);
    const uint8_t* block = (const uint8_t*)block_host_pinned;
    int width = 0;
    for (int g = 0; g < n_members; ++g) {
        const replay_group_member_t& m = members[g];
        IDQN_REQUIRE(m.ring_dev && m.rows_dev && ((uintptr_t)m.rows_dev & 3) == 0, "replay_group_add_step: member %d: null ring or rows, or rows not 4-byte aligned", g);
        IDQN_REQUIRE(m.n_frames >= 1 && m.frame_bytes >= 1 && m.capacity >= 1 && m.n_rows >= 0 && m.n_rows <= REPLAY_GROUP_MAX_ROWS,
                     "replay_group_add_step: member %d: n_frames = %ld, frame_bytes = %ld, capacity = %ld, n_rows = %d (<= %d)", g,
                     (long)m.n_frames, (long)m.frame_bytes, (long)m.capacity, m.n_rows, REPLAY_GROUP_MAX_ROWS);
        IDQN_REQUIRE(m.frame_slot == -1 || (m.frame_slot >= 0 && m.frame_slot < m.n_frames),
                     "replay_group_add_step: member %d: frame slot %d outside [0, %ld) (-1: no frame)", g, m.frame_slot, (long)m.n_frames);
        if (m.frame_slot >= 0)
            IDQN_REQUIRE((m.frame_offset & 15) == 0 && m.frame_offset >= head && m.frame_bytes <= block_bytes &&
                             m.frame_offset <= block_bytes - m.frame_bytes,
                         "replay_group_add_step: member %d: frame at byte %ld (16-byte aligned, behind the records) leaves the block of %ld", g,
                         (long)m.frame_offset, (long)block_bytes);
        if (m.n_rows) {
            IDQN_REQUIRE((m.rows_offset & 3) == 0 && m.rows_offset >= head && m.rows_offset <= block_bytes - (int64_t)m.n_rows * 36,
                         "replay_group_add_step: member %d: row table at byte %ld (4-byte aligned, behind the records) leaves the block of %ld", g,
                         (long)m.rows_offset, (long)block_bytes);
            const int32_t* slots = (const int32_t*)(block + m.rows_offset);
            for (int r = 0; r < m.n_rows; ++r) {
                IDQN_REQUIRE(slots[r] >= 0 && slots[r] < m.capacity, "replay_group_add_step: member %d: row %d goes to slot %d outside capacity = %ld",
                             g, r, slots[r], (long)m.capacity);
                for (int v = 0; v < r; ++v)
                    IDQN_REQUIRE(slots[v] != slots[r], "replay_group_add_step: member %d: element slot %d is written twice", g, slots[r]);
            }
        }
        for (int v = 0; v < g; ++v)
            IDQN_REQUIRE(members[v].ring_dev != m.ring_dev && (void*)members[v].rows_dev != (void*)m.rows_dev &&
                             members[v].ring_dev != (void*)m.rows_dev && (void*)members[v].rows_dev != m.ring_dev,
                         "replay_group_add_step: members %d and %d name the same ring or the same rows", v, g);
        width = std::max(width, (m.frame_slot >= 0 ? replay_group_chunks((long)m.frame_bytes) : 0) + (int)cdiv((long)m.n_rows * 8, 256));
    }
    memmove(block_host_pinned, members, (size_t)head);  // the records travel at the head of the block
    IDQN_HIP_CHECK(hipMemcpyAsync(block_staging_dev, block_host_pinned, (size_t)block_bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    if (width == 0) return IDQN_OK;  // (no member had a frame or a row)
    hipLaunchKernelGGL(k_replay_group_add_step, dim3(width, n_members), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)block_staging_dev, (long)block_bytes);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// One vector step of a seed group of VectorReplayBuffers as one call (include/idqn_hip.h, replay_group_add_many); the checks are
// host C++ of their own (replay_group_many_args.h) and run before the block is written and before anything is enqueued.
#include "replay_group_many_args.h"
static_assert(REPLAY_MANY_MAX_MEMBERS == REPLAY_GROUP_MAX_MEMBERS && REPLAY_MANY_MAX_IN == REPLAY_STEP_MAX_IN &&
                  REPLAY_MANY_MAX_WRITES == REPLAY_STEP_MAX_WRITES && REPLAY_MANY_MAX_ROWS == REPLAY_STEP_MAX_ROWS,
              "replay_group_add_many takes replay_add_step's limits per member");

extern "C" int replay_group_add_many(int32_t n_members, const replay_group_many_member_t* members, void* block_host_pinned,
                                     void* block_staging_dev, int64_t block_bytes, void* stream) {
    int g = -1, j = -1;
    const char* bad = replay_group_many_args_error(n_members, members, block_host_pinned, block_staging_dev, block_bytes, &g, &j);
    IDQN_REQUIRE(!bad, "replay_group_add_many: member %d (with member %d): %s", g, j, bad ? bad : "");
    int width = 0;
    for (int i = 0; i < n_members; ++i)
        width = std::max(width, members[i].n_writes * replay_group_chunks((long)members[i].frame_bytes) + (int)cdiv((long)members[i].n_rows * 8, 256));
    memmove(block_host_pinned, members, (size_t)n_members * sizeof(replay_group_many_member_t));  // the records travel at the head of the block
    IDQN_HIP_CHECK(hipMemcpyAsync(block_staging_dev, block_host_pinned, (size_t)block_bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    hipLaunchKernelGGL(k_replay_group_add_many, dim3(width, n_members), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)block_staging_dev, (long)block_bytes);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}
