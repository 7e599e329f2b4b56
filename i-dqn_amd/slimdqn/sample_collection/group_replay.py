"""The S replay adds of one lock-step iteration of a seed group as ONE call (no reference counterpart: the reference starts one
process per seed, each with a ``ReplayBuffer`` of its own).

``SeedTrainer`` advances S (agent, environment, replay buffer) triples in lock step.  Its buffers stay S separate
``ReplayBuffer`` objects -- own rings, capacities, samplers and keys, so that a seed sees what it would see trained alone --
and ``rb.add`` on each of them costs one ``replay_add_frame`` copy per frame plus one or two more for the element rows at the
next ``sample_slots()``: 2 S to 3 S C calls and asynchronous copies per iteration, 32 bytes each for a LunarLander frame.
``GroupCollector.add_many`` runs the HOST half of every member's ``add`` (``ReplayBuffer._add_host``: allocation, ring growth,
the n-step window, the pinned row mirror, the sampler, the counters -- in ``add``'s order) and sends the device half of all of
them as one pinned block, one asynchronous copy and one launch (``replay_group_add_step``, csrc/replay_group_kernels.h):

    replay_group_member_t [n]      the member records (ring, rows, sizes, where its frame and row table lie in the block)
    per member                     int32 [n_rows] element slots + int32 [n_rows][8] rows: its pending rows [_flushed, add_count)
    per member, 16-byte aligned    its new frame

Afterwards every buffer is in the state its own ``add`` followed by ``_flush_meta`` would have left: the rows are on the device,
``_flushed == add_count``, and the next ``sample_slots()`` / ``ring_view()`` finds nothing to send.
"""
import numpy as np

from slimdqn import _hip
from slimdqn.sample_collection.replay_buffer import ReplayBuffer

RECORD_BYTES = 64  # sizeof(replay_group_member_t)


class GroupCollector:
    # The sizes S (transitions per call) at which the one call is taken by default: those where its median lay below the
    # minimum of the S solo adds (tools/bench_group_collect.py -> profiles/group_collect.json: true at S = 2, 4, 8, 16 and 32,
    # with a margin that grows with S -- 48.6 against 56.3 us at S = 2, 464 against 852 us at S = 32 -- so the sizes between
    # the measured ones are taken with them; at S = 1 the call is the slower leg, 36.0 against 28.7 us).  Other sizes run the
    # members' own ``add``.  ``force=True`` / ``False`` at construction overrides the table either way.
    group_add_sizes = frozenset(range(2, _hip.REPLAY_GROUP_MAX_MEMBERS + 1))
    DEPTH = _hip.STEPS_STAGING_DEPTH  # pinned + device staging blocks in turn, one event each (as idqn_learn_steps_on_replay_fc)

    def __init__(self, replay_buffers, force=None):
        self.replay_buffers = list(replay_buffers)
        self.force = force
        self._plain = [self._is_plain(rb) for rb in self.replay_buffers]
        self._static = [None] * len(self.replay_buffers)  # per member: (frames tensor, the constant head of its record)
        self._blocks, self._block_bytes, self._turn = [], 0, 0
        self.group_calls = 0  # (what tools and tests read: the calls that took the one-call route)

    @staticmethod
    def _is_plain(rb) -> bool:
        """A ``ReplayBuffer`` whose ``add`` is ``ReplayBuffer.add`` itself: not a ``VectorReplayBuffer``, not a subclass with an
        ``add`` (or host half) of its own -- those are added through their own ``add``."""
        t = type(rb)
        return (isinstance(rb, ReplayBuffer) and t.add is ReplayBuffer.add and t._add_host is ReplayBuffer._add_host
                and t._add_elements is ReplayBuffer._add_elements and t._flush_meta is ReplayBuffer._flush_meta)

    # ---- staging: DEPTH (pinned block, device block, event) triples, used in turn ---------------------------------------
    def _alloc_block(self, nbytes):
        """``(numpy uint8 view of a pinned block, its address, address of a device block of the same size, owners)``."""
        import torch

        pin = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        return pin.numpy(), pin.data_ptr(), dev.data_ptr(), (pin, dev)

    def _new_event(self):
        import torch

        return torch.cuda.Event()

    def _ensure_blocks(self, nbytes):
        if nbytes <= self._block_bytes:
            return
        for b in self._blocks:  # (rare: the first call, or a member with larger frames joined)
            if b["used"]:
                b["event"].synchronize()
        size = max(4096, 2 * nbytes)
        self._blocks = []
        for _ in range(self.DEPTH):
            u8, host, dev, owners = self._alloc_block(size)
            assert host % 16 == 0 and dev % 16 == 0
            self._blocks.append({"u8": u8, "i32": u8.view(np.int32), "i64": u8.view(np.int64), "host": host, "dev": dev, "owners": owners,
                                 "event": self._new_event(), "used": False})
        self._block_bytes = size

    # ---- the call ---------------------------------------------------------------------------------------------------------
    def _route(self, n) -> bool:
        if self.__dict__.get("_group_add_ok") is False or not 1 <= n <= _hip.REPLAY_GROUP_MAX_MEMBERS:
            return False
        return bool(self.force) if self.force is not None else n in self.group_add_sizes

    def _record_head(self, m, rb):
        """(ring, rows, n_frames, frame_bytes, capacity) of member m's record; re-read when its ring was replaced (grown)."""
        st = self._static[m]
        if st is None or st[0] is not rb._frames:
            st = (rb._frames, (rb._frames.data_ptr(), rb._meta_dev.data_ptr(), rb._n_frames, rb._frame_bytes, rb._max_capacity))
            self._static[m] = st
        return st[1]

    def add_many(self, transitions, members=None, **kwargs) -> None:
        """Adds ``transitions[i]`` to buffer ``members[i]`` (default: one per buffer, in order; any subset of the buffers, each at
        most once); ``kwargs`` go to every sampler's ``add`` as they would through ``rb.add(transition, **kwargs)``."""
        rbs = self.replay_buffers
        members = range(len(transitions)) if members is None else list(members)
        assert len(members) == len(transitions) and len(set(members)) == len(members), "one transition per named buffer"
        if not self._route(len(members)):
            for m, tr in zip(members, transitions):
                rbs[m].add(tr, **kwargs)
            return
        # the host half of every member's add; whoever cannot join goes its own way before the block is filled
        cap_rows, joint, nbytes = _hip.REPLAY_GROUP_MAX_ROWS, [], 0
        for m, tr in zip(members, transitions):
            rb = rbs[m]
            if not self._plain[m]:
                rb.add(tr, **kwargs)
                continue
            frame, slot = rb._add_host(tr, **kwargs)  # (a deferred add is flushed first: the member's own add)
            lo, hi = rb._flushed, rb._add_count
            if hi - lo > min(cap_rows, rb._max_capacity):  # after _grow_ring reset _flushed, or after many solo adds
                rb._flush_meta()
                lo = hi
            joint.append((m, rb, frame, slot, lo, hi))
            nbytes += 36 * (hi - lo) + ((rb._frame_bytes + 15) & ~15)
        if not joint:
            return
        n = len(joint)
        head = RECORD_BYTES * n
        nbytes += head + 16
        self._ensure_blocks(nbytes)
        blk = self._blocks[self._turn % self.DEPTH]
        if blk["used"]:
            blk["event"].synchronize()  # the copy that last read this block (DEPTH calls ago) has passed
        u8, i32, i64 = blk["u8"], blk["i32"], blk["i64"]
        at = head  # row tables first (4-byte granules), then the frames (16-byte aligned)
        row_at = []
        for _, rb, _, _, lo, hi in joint:
            row_at.append(at)
            k = hi - lo
            if k == 1:
                s, o = lo % rb._max_capacity, at >> 2
                i32[o] = s
                i32[o + 1:o + 9] = rb._meta[s]
            elif k:
                slots, o = np.arange(lo, hi, dtype=np.int64) % rb._max_capacity, at >> 2
                i32[o:o + k] = slots
                i32[o + k:o + 9 * k] = rb._meta[slots].reshape(-1)
            at += 36 * k
        for j, (m, rb, frame, slot, lo, hi) in enumerate(joint):
            at = (at + 15) & ~15
            u8[at:at + frame.size] = frame
            # replay_group_member_t: five int64, frame_offset, (frame_slot, n_rows) as two int32, rows_offset
            i64[8 * j:8 * j + 8] = self._record_head(m, rb) + (at, slot | ((hi - lo) << 32), row_at[j])
            at += frame.size
        assert at <= nbytes <= self._block_bytes
        lib, q = _hip.lib(), _hip.current_stream()
        rc = lib.replay_group_add_step(n, blk["host"], blk["host"], blk["dev"], at, q)
        if rc == _hip.E_INVALID and self.__dict__.get("_group_add_ok") is None:
            # not this library / these buffers: the members' own add from now on, and the device half of THIS call by their
            # own copies -- the frames lie in the block; the rows stay pending for the members' own _flush_meta
            self._group_add_ok = False
            for j, (m, rb, frame, slot, lo, hi) in enumerate(joint):
                off = int(i64[8 * j + 5])
                _hip.check(lib.replay_add_frame(_hip.ptr(rb._frames), slot, rb._frame_bytes, blk["host"] + off, q), "replay_add_frame")
        else:
            _hip.check(rc, "replay_group_add_step")
            self._group_add_ok = True
            self.group_calls += 1
            for _, rb, _, _, _, hi in joint:
                rb._flushed = hi
        blk["event"].record()
        blk["used"] = True
        self._turn += 1
