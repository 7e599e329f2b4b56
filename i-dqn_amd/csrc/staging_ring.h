// Host-argument staging ring (host code only): IDQN_STEPS_STAGING_DEPTH x {pinned block, device twin, event}.  A call that has
// ordinary host memory to hand to a launch takes the next block (acquire), writes the block's pinned half (pin()), enqueues its
// upload into the device twin (upload) and, behind the LAST launch that reads the twin (dev()), records the block's event
// (guard).  A block is rewritten only after that event has passed -- acquire waits for it -- so back-to-back calls need no
// synchronisation of their own.  Serves the handle's ring (slots of idqn_learn_steps_on_replay_fc, uniforms of the prioritized
// entries) and the one ring of a seed group, on which its four learner entries interleave.
//
// Allocation rule, the same for every ring: the first acquire makes the WHOLE ring, every block `block_bytes` large, and nothing
// is allocated later; when any part of that fails, what it got is freed again and the ring stays empty (a later acquire starts
// over).  release() frees the ring (the destroy functions, after the device is idle).
#pragma once
#include "common.h"

struct StagingRing {
    // the current block (the one the last acquire handed out): its pinned half and its device twin
    uint8_t* pin() const { return pin_[cur_]; }
    uint8_t* dev() const { return dev_[cur_]; }

    int acquire(size_t block_bytes) {
        if (!made_) {
            hipError_t e = hipSuccess;
            for (int i = 0; i < IDQN_STEPS_STAGING_DEPTH && e == hipSuccess; ++i) {
                e = hipHostMalloc((void**)&pin_[i], block_bytes, hipHostMallocDefault);
                if (e == hipSuccess) e = hipMalloc((void**)&dev_[i], block_bytes);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming);
            }
            if (e != hipSuccess) release();
            IDQN_HIP_CHECK(e);
            made_ = true;
        }
        cur_ = next_;
        if (busy_[cur_]) IDQN_HIP_CHECK(hipEventSynchronize(ev_[cur_]));  // the launches that read this block are done
        busy_[cur_] = false;
        return IDQN_OK;
    }

    // the first `bytes` of the current block -> its device twin, on q; the next acquire takes the next block
    int upload(size_t bytes, hipStream_t q) {
        IDQN_HIP_CHECK(hipMemcpyAsync(dev_[cur_], pin_[cur_], bytes, hipMemcpyHostToDevice, q));
        next_ = (cur_ + 1) % IDQN_STEPS_STAGING_DEPTH;
        return IDQN_OK;
    }

    // behind the last launch on q that reads the current block
    int guard(hipStream_t q) {
        IDQN_HIP_CHECK(hipEventRecord(ev_[cur_], q));
        busy_[cur_] = true;
        return IDQN_OK;
    }

    void release() {
        for (int i = 0; i < IDQN_STEPS_STAGING_DEPTH; ++i) {
            if (pin_[i]) (void)hipHostFree(pin_[i]);
            if (dev_[i]) (void)hipFree(dev_[i]);
            if (ev_[i]) (void)hipEventDestroy(ev_[i]);
            pin_[i] = dev_[i] = nullptr; ev_[i] = nullptr; busy_[i] = false;
        }
        made_ = false;
    }

private:
    uint8_t* pin_[IDQN_STEPS_STAGING_DEPTH] = {};
    uint8_t* dev_[IDQN_STEPS_STAGING_DEPTH] = {};
    hipEvent_t ev_[IDQN_STEPS_STAGING_DEPTH] = {};
    bool busy_[IDQN_STEPS_STAGING_DEPTH] = {};
    bool made_ = false;
    int next_ = 0, cur_ = 0;
};
