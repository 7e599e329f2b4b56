"""``GroupCollector`` (slimdqn/sample_collection/group_replay.py) on numpy stubs, no library and no GPU: the 'device' is host
memory, ``replay_group_add_step`` is a numpy model that checks what the C entry checks, copies the pinned block to the staging
block and applies it from there, and the two copies of the solo path (``replay_add_frame``) are a memmove -- so a twin set of
buffers driven by ``rb.add`` can be compared with the set driven by ``add_many`` (tests/group_collect.py)."""
import ctypes as C

import numpy as np
import pytest

from group_collect import Twins, make_script

E_INVALID = -1


class _Mem:
    """A numpy array with the two tensor methods the buffers and the collector use."""

    def __init__(self, arr):
        self.arr = arr

    def data_ptr(self):
        return self.arr.ctypes.data

    def numpy(self):
        return self.arr


class _Event:
    def record(self):
        pass

    def synchronize(self):
        pass


def _addr(x):
    return int(x.value if isinstance(x, C.c_void_p) else x)


def _view(addr, nbytes):
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(addr))


class _Lib:
    """The C entries the collection path calls, on host memory."""

    def __init__(self, refuse=False):
        self.refuse, self.calls, self.copies = refuse, [], 0

    def idqn_last_error(self):
        return b"stub"

    def replay_add_frame(self, dst, slot, nbytes, src, q):
        self.copies += 1
        C.memmove(_addr(dst) + slot * nbytes, _addr(src), nbytes)
        return 0

    def replay_group_add_step(self, n, members, host, dev, nbytes, q):
        from slimdqn import _hip

        if self.refuse or not 1 <= n <= 32 or _addr(host) % 16 or _addr(dev) % 16 or nbytes < 64 * n:
            return E_INVALID
        recs = (_hip.GroupAddMember * n).from_address(_addr(members))
        block = _view(_addr(host), nbytes)
        seen = set()
        for m in recs:
            if not (m.ring_dev and m.rows_dev) or m.ring_dev in seen or m.rows_dev in seen or m.n_rows > 32:
                return E_INVALID
            seen |= {m.ring_dev, m.rows_dev}
            if not (m.frame_slot == -1 or 0 <= m.frame_slot < m.n_frames):
                return E_INVALID
            if m.frame_slot >= 0 and (m.frame_offset % 16 or not 64 * n <= m.frame_offset <= nbytes - m.frame_bytes):
                return E_INVALID
            if m.n_rows:
                if m.rows_offset % 4 or not 64 * n <= m.rows_offset <= nbytes - 36 * m.n_rows:
                    return E_INVALID
                slots = block[m.rows_offset:m.rows_offset + 4 * m.n_rows].view(np.int32)
                if len(set(slots.tolist())) != m.n_rows or slots.min() < 0 or slots.max() >= m.capacity:
                    return E_INVALID
        C.memmove(_addr(host), _addr(members), 64 * n)
        C.memmove(_addr(dev), _addr(host), nbytes)  # the one copy; the 'launch' reads the staging block only
        staged = _view(_addr(dev), nbytes)
        call = []
        for m in (_hip.GroupAddMember * n).from_address(_addr(dev)):
            if m.frame_slot >= 0:
                C.memmove(m.ring_dev + m.frame_slot * m.frame_bytes, _addr(dev) + m.frame_offset, m.frame_bytes)
            table = staged[m.rows_offset:m.rows_offset + 36 * m.n_rows].view(np.int32)
            rows = _view(m.rows_dev, 32 * m.capacity).view(np.int32).reshape(-1, 8)
            for r in range(m.n_rows):
                rows[table[r]] = table[m.n_rows + 8 * r:m.n_rows + 8 * r + 8]
            call.append((m.frame_slot, m.n_rows, m.frame_bytes, m.capacity))
        self.calls.append(call)
        return 0


def _allocate(self, frame):
    """``ReplayBuffer._allocate`` with host memory in place of the device and pinned allocations."""
    self._frame_shape, self._obs_dtype = tuple(frame.shape), frame.dtype
    self._frame_elems, self._itemsize = int(frame.size), int(frame.dtype.itemsize)
    self._frame_bytes = self._frame_elems * self._itemsize
    self._obs_shape = self._frame_shape + (self._stack_size,)
    cap = self._max_capacity
    self._n_frames = cap + self._update_horizon + self._stack_size + max(64, cap // 16)
    self._frames = _Mem(np.full((self._n_frames, self._frame_bytes), 0xCD, np.uint8))
    self._meta_pin = _Mem(np.zeros((cap, 8), np.int32))
    self._meta = self._meta_pin.arr
    self._meta_dev = _Mem(np.zeros((cap, 8), np.int32))
    self._meta_ev, self._meta_ev_lo, self._meta_ev_obj = None, 0, None
    self._first_frame = np.zeros(cap, np.int64)
    self._action, self._reward64 = np.zeros(cap, np.int64), np.zeros(cap, np.float64)
    self._pin = _Mem(np.zeros((self.STAGING, self._frame_bytes), np.uint8))
    self._pin_np, self._pin_events, self._pin_ptr = self._pin.arr, [None, None], self._pin.data_ptr()


@pytest.fixture
def stub(monkeypatch):
    import torch

    from slimdqn import _hip
    from slimdqn.sample_collection.group_replay import GroupCollector
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer

    lib = _Lib()
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(ReplayBuffer, "_allocate", _allocate)

    def alloc(self, nbytes):
        raw = [np.zeros(nbytes + 16, np.uint8) for _ in range(2)]
        pin, dev = (r[(-r.ctypes.data) % 16:][:nbytes] for r in raw)
        return pin, pin.ctypes.data, dev.ctypes.data, raw

    monkeypatch.setattr(GroupCollector, "_alloc_block", alloc)
    monkeypatch.setattr(GroupCollector, "_new_event", lambda self: _Event())
    return lib


# (frame shape, dtype, capacity, stack, update_horizon): frames of 32, 12 and 15 bytes, capacities that wrap within the script
KINDS = [((8,), np.float32, 7, 1, 1), ((3,), np.float32, 5, 1, 3), ((5, 3), np.uint8, 5, 2, 1)]


def _buffers(kinds=KINDS):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    return [ReplayBuffer(UniformSamplingDistribution(g), batch_size=4, max_capacity=cap, stack_size=stack, update_horizon=n, gamma=0.99)
            for g, (_, _, cap, stack, n) in enumerate(kinds)]


def _twins(kinds=KINDS):
    return Twins(_buffers(kinds), _buffers(kinds), lambda rb: rb._frames.arr, lambda rb: rb._meta_dev.arr)


def _scripts(steps, kinds=KINDS, **kw):
    return [make_script(10 + g, shape, dtype, steps, terminal_every=7 + g, truncate_every=5, **kw) for g, (shape, dtype, *_) in enumerate(kinds)]


def test_block_round_trip_for_members_of_different_frames_and_capacities(stub):
    from slimdqn.sample_collection.group_replay import GroupCollector

    tw = _twins()
    col, scripts = GroupCollector(tw.group, force=True), _scripts(40)
    for t in range(40):
        before = stub.copies
        tw.step(col, [s[t] for s in scripts])
        assert stub.copies - before == len(KINDS), "the collector itself issues no copy: these are the solo twins' frames"
        tw.check(where=f"step {t}")
    assert col.group_calls == len(stub.calls) == 40 and col._group_add_ok is True
    assert all([c[2:] for c in call] == [(32, 7), (12, 5), (15, 5)] for call in stub.calls)
    assert max(c[1] for call in stub.calls for c in call) == 3, "an episode end of the update_horizon = 3 member emits 3 rows in one step"
    assert all(rb._add_count > rb._max_capacity for rb in tw.group), "FIFO eviction and slot wrap-around were reached"
    for a, b in zip(tw.solo, tw.group):  # equal draws from equal sampler streams
        assert np.array_equal(a.sample_slots(), b.sample_slots())


def test_default_sizes_decide_the_route(stub):
    from slimdqn.sample_collection.group_replay import GroupCollector

    tw = _twins()
    col, scripts = GroupCollector(tw.group), _scripts(6)
    assert isinstance(GroupCollector.group_add_sizes, frozenset)
    for t in range(3):
        tw.step(col, [s[t] for s in scripts])
    assert (col.group_calls == 3) == (len(KINDS) in GroupCollector.group_add_sizes)
    col.group_add_sizes = frozenset({len(KINDS)})
    for t in range(3, 6):
        tw.step(col, [s[t] for s in scripts])
    assert col.group_calls >= 3
    tw.check()


def test_member_over_the_row_cap_flushes_itself_and_joins_without_rows(stub):
    from slimdqn import _hip
    from slimdqn.sample_collection.group_replay import GroupCollector

    kinds = [((8,), np.float32, 64, 1, 1), ((3,), np.float32, 5, 1, 1)]
    tw = _twins(kinds)
    col, scripts = GroupCollector(tw.group, force=True), _scripts(60, kinds)
    for t in range(50):  # solo adds, never sampled: 35-odd rows pending on member 0, more than its capacity on member 1
        for g in range(2):
            for rb in (tw.solo[g], tw.group[g]):
                rb.add(scripts[g][t])
            tw.frames[g].append(scripts[g][t].observation)
    pending = [rb._add_count - rb._flushed for rb in tw.group]
    assert pending[0] > _hip.REPLAY_GROUP_MAX_ROWS and pending[1] > 5
    copies = stub.copies
    tw.step(col, [s[50] for s in scripts])
    assert [c[:2] for c in stub.calls[-1]] == [(tw.group[0]._t - 1, 0), ((tw.group[1]._t - 1) % tw.group[1]._n_frames, 0)]
    assert stub.copies - copies >= 2 + 2, "both members sent their rows themselves (and the solo twins their frames)"
    tw.check(where="after the fallback")
    tw.step(col, [s[51] for s in scripts])
    assert [c[1] for c in stub.calls[-1]] == [1, 1], "from then on the rows travel in the block again"
    tw.check()


def test_deferred_add_is_flushed_first(stub):
    from slimdqn.sample_collection.group_replay import GroupCollector

    tw = _twins()
    col, scripts = GroupCollector(tw.group, force=True), _scripts(8)
    for t in range(0, 8, 2):
        for g in range(len(KINDS)):
            tw.solo[g].add(scripts[g][t])
            tw.group[g].add_deferred(scripts[g][t])
            tw.frames[g].append(scripts[g][t].observation)
        assert all(rb._deferred is not None for rb in tw.group)
        tw.step(col, [s[t + 1] for s in scripts])
        assert all(rb._deferred is None for rb in tw.group)
        tw.check(where=f"step {t}")


def test_subset_of_members(stub):
    from slimdqn.sample_collection.group_replay import GroupCollector

    tw = _twins()
    col, scripts = GroupCollector(tw.group, force=True), _scripts(30)
    at = [0] * len(KINDS)
    for t in range(30):
        members = [g for g in range(len(KINDS)) if (t + g) % 3 or t < 4] if t < 20 else [2]  # (a seed that finished stops stepping)
        tw.step(col, [scripts[g][at[g]] for g in members], members)
        for g in members:
            at[g] += 1
        assert len(stub.calls[-1]) == len(members)
        tw.check(where=f"step {t}")
    assert len(set(at)) > 1


def test_refusal_on_the_first_call_sets_the_flag_and_loses_nothing(stub):
    from slimdqn.sample_collection.group_replay import GroupCollector

    stub.refuse = True
    tw = _twins()
    col, scripts = GroupCollector(tw.group, force=True), _scripts(12)
    for t in range(12):
        tw.step(col, [s[t] for s in scripts])
        for b in tw.group:
            b._flush_meta()  # (refused: the rows stayed pending, as after the members' own add)
        tw.check(where=f"step {t}")
    assert col._group_add_ok is False and col.group_calls == 0 and stub.calls == []


def test_not_a_plain_buffer_goes_through_its_own_add(stub):
    from slimdqn.sample_collection.group_replay import GroupCollector
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    class Counting(ReplayBuffer):
        seen = 0

        def add(self, transition, **kwargs):
            self.seen += 1
            super().add(transition, **kwargs)

    class Foreign:
        def __init__(self):
            self.added = []

        def add(self, tr):
            self.added.append(tr)

    own = Counting(UniformSamplingDistribution(0), batch_size=4, max_capacity=7, stack_size=1)
    plain = _buffers(KINDS[:1])[0]
    foreign = Foreign()
    col, script = GroupCollector([own, plain, foreign], force=True), make_script(3, (8,), np.float32, 5)
    assert col._plain == [False, True, False]
    for tr in script:
        col.add_many([tr, tr, tr])
    assert own.seen == 5 and len(foreign.added) == 5 and own._add_count == plain._add_count == 4
    assert all(len(call) == 1 for call in stub.calls) and len(stub.calls) == 5
    own._flush_meta()
    assert np.array_equal(own._meta_dev.arr, plain._meta_dev.arr) and np.array_equal(own._frames.arr[:5], plain._frames.arr[:5])
