// Replay-sourced learner step of the MLP ("fc") and general-shape cnn handles (idqn_learn_on_replay_fc / _dev):
// update_online_params = ReplayBuffer.sample() + learn_on_batch (idqn.py:65-72, replay_buffer.py:215-230) as ONE C call.
//
// Two ways from the frame ring to the step, both with the row semantics of k_replay_gather_stacked (replay.hip): element row
// {newest state frame slot, valid state frames, newest next_state frame slot, valid next frames, action, reward bits, terminal, 0};
// output element (pixel, ch) of a stack = frame[newest - (stack - 1 - ch)][pixel] modulo n_frames, or 0 where ch < stack - valid.
//   * k_rps_stage: ONE staging launch writes the two stacked minibatches and the action / reward / terminal scalars into buffers
//     the handle owns; the general-shape cnn step and k_fc_step_mfma / k_fc_step_lds then run unchanged on those buffers.
//   * FcRingSrc: the minibatch source of k_fc_step_par<FcRingSrc> (fc_par_kernels.h) -- the one-launch step resolves slot -> row -> frame
//     in its entry phase and requests the minibatch from the ring, so the one-launch step stays one launch.
// The slots travel as kernel arguments (RpsSlots*: no upload, no gather launch) or are read from a device array (RpsSlotsDev).
// Plain loads and vector stores; every output element has one writer.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define RPS_ARG_SLOTS 256  // slots per staging launch when they travel as kernel arguments
#define RPS_PAR_SLOTS 32   // ... of the one-launch MLP step (batches of <= 32 samples)

struct RpsSlots { int32_t slot[RPS_ARG_SLOTS]; };
struct RpsSlotsPar { int32_t slot[RPS_PAR_SLOTS]; };
struct RpsSlotsDev { const int32_t* slot; };

// ring slot of the frame `back` transitions before `newest` (0 <= result < n_frames for any row contents)
__device__ __forceinline__ long rps_ring_slot(long newest, long back, long n_frames) {
    const long r = (newest - back) % n_frames;
    return r < 0 ? r + n_frames : r;
}

struct RpsStageArgs {
    const uint8_t* frames;  // [n_frames][frame_elems] of T
    const int32_t* rows;    // [capacity][8]
    long n_frames, frame_elems;
    int stack, B, first;    // samples [first, first + gridDim.x) of the batch; slot i of `sl` belongs to sample first + i
    void *s_out, *n_out;    // [B][frame_elems][stack] of T
    int32_t* a_out;
    float* r_out;
    uint8_t* t_out;
};

// grid (samples, state | next_state, chunks).  T = float: one element per lane and iteration.  T = uint8_t: four consecutive
// output bytes per lane and iteration as one 32-bit store where a sample's stack is a multiple of four bytes, else bytes.
template <class T, class Slots>
__global__ __launch_bounds__(256) void k_rps_stage(RpsStageArgs a, Slots sl) {
    const int i = blockIdx.x, b = a.first + i, half = blockIdx.y;
    if (b >= a.B) return;
    const int32_t* m = a.rows + (long)sl.slot[i] * 8;
    const long newest = m[2 * half], valid = m[2 * half + 1];
    if (half == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
        a.a_out[b] = m[4];
        a.r_out[b] = __int_as_float(m[5]);
        a.t_out[b] = (uint8_t)m[6];
    }
    const T* frames = reinterpret_cast<const T*>(a.frames);
    const long total = a.frame_elems * a.stack;
    T* dst = reinterpret_cast<T*>(half ? a.n_out : a.s_out) + (long)b * total;
    const long tid = (long)blockIdx.z * 256 + threadIdx.x, nthr = (long)gridDim.z * 256;
    auto elem = [&](long o) -> T {
        const long pix = o / a.stack, back = a.stack - 1 - (o - pix * a.stack);
        return back < valid ? frames[rps_ring_slot(newest, back, a.n_frames) * a.frame_elems + pix] : (T)0;
    };
    if (sizeof(T) == 1 && (total & 3) == 0) {  // (dst: a hipMalloc base + b * total, 4-byte aligned)
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
        for (long w = tid; w < (total >> 2); w += nthr) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (uint32_t)(uint8_t)elem(4 * w + j) << (8 * j);
            d4[w] = v;
        }
        return;
    }
    for (long o = tid; o < total; o += nthr) dst[o] = elem(o);
}

// The minibatch of k_fc_step_par: the caller's contiguous batch (FcBatchSrc: a.s / a.s2 / a.action / a.reward / a.terminal) ...
struct FcBatchSrc {
    static constexpr bool replay = false;
};
// ... or float32 frames of the ring: feature i of sample b = frame element i / stack of stack channel i % stack.
template <class Slots>
struct FcRingSrc {
    static constexpr bool replay = true;
    const float* frames;  // [n_frames][frame_elems]
    const int32_t* rows;
    long n_frames, frame_elems;
    int stack;
    Slots sl;
    __device__ __forceinline__ const int32_t* row(int b) const { return rows + (long)sl.slot[b] * 8; }
    __device__ __forceinline__ float feature(const int32_t* m, int half, int i) const {
        const long newest = m[2 * half], valid = m[2 * half + 1];
        const int pix = i / stack, back = stack - 1 - (i - pix * stack);
        return back < valid ? frames[rps_ring_slot(newest, back, n_frames) * frame_elems + pix] : 0.f;
    }
};
