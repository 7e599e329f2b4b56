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


VECTOR_RECORD_BYTES = 80  # sizeof(replay_group_many_member_t)


class GroupVectorCollector(GroupCollector):
    """``GroupCollector`` for members that are ``VectorReplayBuffer`` objects: one vector step of S seeds, E_g time lines each, as
    ONE call (``replay_group_add_many``, csrc/replay_group_kernels.h).  ``add_many`` runs the host half of every member's
    ``add_many`` (``VectorReplayBuffer._add_many_host``: allocation, the segment plan, ring growth, the sampler, the counters), in
    member order, and sends all device halves as one pinned block, one asynchronous copy and one launch:

        replay_group_many_member_t [n]   the member records (ring, rows, sizes, counts, where its tables and frames lie)
        per member, 4-byte aligned       int32 [n_writes][2] (frame index, ring slot) pairs; int32 [n_rows] element slots +
                                         int32 [n_rows][8] rows
        per member, 16-byte aligned      its new frames, [n_in][frame_bytes]

    Afterwards every buffer is in the state its own ``add_many`` would have left.  The staging ring (``DEPTH`` pinned / device block
    pairs, one event each) is ``GroupCollector``'s."""

    # The group sizes S (members that step in a call) at which the one call is the default: those where its median lay below the
    # minimum of the S solo ``add_many`` calls at E = 2 AND at E = 8 (tools/bench_group_vector_collect.py ->
    # profiles/group_vector_collect.json: true at S = 2, 4, 8 and 16 with a margin that grows with S -- 78.4 against 90.0 us at
    # S = 2, E = 2; 987.8 against 1196.4 us at S = 16, E = 8 -- so the sizes between the measured ones are taken with them; at
    # S = 1 the call is the slower leg, 49.6 against 46.1 us at E = 2 and 86.0 against 82.4 us at E = 8; S = 17 .. 32 were not
    # measured and stay off).  Other sizes run the members' own ``add_many``; ``force=True`` / ``False`` overrides the table.
    group_add_many_sizes = frozenset(range(2, 17))

    def __init__(self, replay_buffers, force=None):
        self.replay_buffers = list(replay_buffers)
        self.force = force
        self._vector = [self._is_vector(rb) for rb in self.replay_buffers]
        self._static = [None] * len(self.replay_buffers)
        self._blocks, self._block_bytes, self._turn = [], 0, 0
        self.group_calls = 0

    @staticmethod
    def _is_vector(rb) -> bool:
        """A ``VectorReplayBuffer`` whose ``add_many`` and its two halves are the class's own."""
        from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer as V

        t = type(rb)
        return (isinstance(rb, V) and t.add_many is V.add_many and t._add_many_host is V._add_many_host and t._plan_many is V._plan_many
                and t._finish_many is V._finish_many and t._issue_step is V._issue_step and t._issue is V._issue)

    def _route(self, n) -> bool:
        if self.__dict__.get("_group_add_many_ok") is False or not 1 <= n <= _hip.REPLAY_GROUP_MAX_MEMBERS:
            return False
        return bool(self.force) if self.force is not None else n in self.group_add_many_sizes

    @staticmethod
    def _solo(rb, entries, **kwargs) -> None:
        """A member's own route: ``add_many``, or -- a buffer without one -- ``add`` per entry."""
        if hasattr(rb, "add_many"):
            rb.add_many(entries, **kwargs)
        else:
            for tr in entries:
                if tr is not None:
                    rb.add(tr, **kwargs)

    def add_many(self, transitions, members=None, **kwargs) -> None:
        """``transitions[i]``: the list of E entries (a transition or ``None`` each) of buffer ``members[i]`` (default: one list per
        buffer, in order); ``kwargs`` go to every sampler's ``add`` as through ``rb.add_many(entries, **kwargs)``."""
        rbs = self.replay_buffers
        members = range(len(transitions)) if members is None else list(members)
        assert len(members) == len(transitions) and len(set(members)) == len(members), "one list of entries per named buffer"
        stepping = sum(1 for m, trs in zip(members, transitions) if self._vector[m] and any(tr is not None for tr in trs))
        if not self._route(stepping):
            for m, trs in zip(members, transitions):
                self._solo(rbs[m], trs, **kwargs)
            return
        # the host half of every member's add_many, in member order; whoever cannot join sends its device half itself, now
        joint, nbytes = [], 0
        for m, trs in zip(members, transitions):
            rb = rbs[m]
            if not self._vector[m]:
                self._solo(rb, trs, **kwargs)
                continue
            grown = rb._plan.n_growths
            host = rb._add_many_host(trs, **kwargs)
            if host is None:  # (no environment of this member stepped)
                continue
            frames, writes, slots = host
            if rb._plan.n_growths != grown or len(slots) > _hip.REPLAY_STEP_MAX_ROWS:
                rb._issue_step(frames, writes, slots)
                continue
            joint.append((m, rb, frames, writes, slots))
            nbytes += 8 * len(writes) + 36 * len(slots) + ((len(frames) * rb._frame_bytes + 15) & ~15)
        if not joint:
            return
        n = len(joint)
        head = VECTOR_RECORD_BYTES * n
        nbytes += head + 16
        self._ensure_blocks(nbytes)
        blk = self._blocks[self._turn % self.DEPTH]
        if blk["used"]:
            blk["event"].synchronize()  # the copy that last read this block (DEPTH calls ago) has passed
        u8, i32, i64 = blk["u8"], blk["i32"], blk["i64"]
        at, tables = head, []  # the tables first (4-byte granules), then the frames (16-byte aligned)
        for _, rb, _, writes, slots in joint:
            w, k, o = len(writes), len(slots), at >> 2
            if w:
                i32[o:o + 2 * w] = np.asarray(writes, np.int32).reshape(-1)
            o += 2 * w
            if k:
                i32[o:o + k] = slots
                i32[o + k:o + 9 * k] = rb._plan.rows[slots].reshape(-1)
            tables.append((at, at + 8 * w))
            at += 8 * w + 36 * k
        for j, (m, rb, frames, writes, slots) in enumerate(joint):
            at = (at + 15) & ~15
            fb = rb._frame_bytes
            for i, f in enumerate(frames):
                u8[at + i * fb:at + (i + 1) * fb] = f.view(np.uint8).reshape(-1)
            # replay_group_many_member_t: five int64, (n_in, n_writes) and (n_rows, 0) as int32 pairs, three offsets
            i64[10 * j:10 * j + 10] = self._record_head(m, rb) + (len(frames) | (len(writes) << 32), len(slots)) + tables[j] + (at,)
            at += len(frames) * fb
        assert at <= nbytes <= self._block_bytes
        lib, q = _hip.lib(), _hip.current_stream()
        rc = lib.replay_group_add_many(n, blk["host"], blk["host"], blk["dev"], at, q)
        if rc == _hip.E_INVALID and self.__dict__.get("_group_add_many_ok") is None:
            # not this library / these buffers: the members' own add_many from now on, and the device half of THIS call by
            # their own replay_add_step calls (the entry refuses before it writes or enqueues anything)
            self._group_add_many_ok = False
            for _, rb, frames, writes, slots in joint:
                rb._issue_step(frames, writes, slots)
            return
        _hip.check(rc, "replay_group_add_many")
        self._group_add_many_ok = True
        self.group_calls += 1
        blk["event"].record()
        blk["used"] = True
        self._turn += 1
