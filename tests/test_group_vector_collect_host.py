"""``GroupVectorCollector`` and ``SeedVectorTrainer`` on numpy stubs, no library and no GPU: the 'device' is host memory,
``replay_group_add_many`` and ``replay_add_step`` are numpy models that check what the C entries check, copy the pinned block to the
staging block and apply it from there -- so a twin set of ``VectorReplayBuffer`` objects driven by ``rb.add_many`` can be compared
with the set driven by the collector (tests/group_vector_collect.py), and the tables the collector stages with what each member's
``SegmentPlan.plan_step`` yields."""
import ctypes as C

import numpy as np
import pytest

from group_vector_collect import VectorTwins, make_vector_script

E_INVALID = -1
RECORD = 80


class _Mem:
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
    return int((x.value or 0) if isinstance(x, C.c_void_p) else x)


def _view(addr, nbytes):
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(addr))


def _apply(ring, fb, rows, src_frames, pairs, slots, new_rows):
    for src, dst in pairs:
        C.memmove(ring + int(dst) * fb, src_frames + int(src) * fb, fb)
    for slot, row in zip(slots, new_rows):
        _view(rows + 32 * int(slot), 32).view(np.int32)[:] = row


class _Lib:
    """The C entries the vector collection path calls, on host memory."""

    def __init__(self):
        self.refuse, self.group_calls, self.step_calls = False, [], []

    def idqn_last_error(self):
        return b"stub"

    def replay_add_step(self, ring, n_frames, fb, rows, cap, pin, dev, n_in, n_writes, n_rows, q):
        W, R, head = 64, 128, 5120
        nbytes = head + n_in * fb
        C.memmove(_addr(dev), _addr(pin), nbytes)
        table = _view(_addr(dev), head).view(np.int32)
        pairs, slots = table[:2 * n_writes].reshape(-1, 2), table[2 * W:2 * W + n_rows]
        if not (0 <= n_in <= 32 and 0 <= n_writes <= W and 0 <= n_rows <= R and n_writes + n_rows >= 1) or len(set(slots.tolist())) != n_rows \
                or len(set(pairs[:, 1].tolist())) != n_writes:
            return E_INVALID
        _apply(_addr(ring), fb, _addr(rows), _addr(dev) + head, pairs, slots, table[2 * W + R:2 * W + R + 8 * n_rows].reshape(-1, 8))
        self.step_calls.append((_addr(ring), n_in, pairs.tolist(), slots.tolist()))
        return 0

    def replay_group_add_many(self, n, members, host, dev, nbytes, q):
        from slimdqn import _hip

        assert C.sizeof(_hip.GroupAddManyMember) == RECORD
        if self.refuse or not 1 <= n <= 32 or _addr(host) % 16 or _addr(dev) % 16 or nbytes < RECORD * n:
            return E_INVALID
        block, seen = _view(_addr(host), nbytes), set()
        inside = lambda off, size, align: off % align == 0 and RECORD * n <= off <= nbytes - size
        for m in (_hip.GroupAddManyMember * n).from_address(_addr(members)):
            if not (m.ring_dev and m.rows_dev) or m.ring_dev in seen or m.rows_dev in seen:
                return E_INVALID
            seen |= {m.ring_dev, m.rows_dev}
            if not (0 <= m.n_in <= 32 and 0 <= m.n_writes <= 64 and 0 <= m.n_rows <= 128 and m.n_writes + m.n_rows >= 1 and (m.n_in or not m.n_writes)):
                return E_INVALID
            if m.n_in and not inside(m.frames_offset, m.n_in * m.frame_bytes, 16):
                return E_INVALID
            if m.n_writes:
                if not inside(m.pairs_offset, 8 * m.n_writes, 4):
                    return E_INVALID
                pairs = block[m.pairs_offset:m.pairs_offset + 8 * m.n_writes].view(np.int32).reshape(-1, 2)
                if pairs[:, 0].min() < 0 or pairs[:, 0].max() >= m.n_in or pairs[:, 1].min() < 0 or pairs[:, 1].max() >= m.n_frames \
                        or len(set(pairs[:, 1].tolist())) != m.n_writes:
                    return E_INVALID
            if m.n_rows:
                if not inside(m.rows_offset, 36 * m.n_rows, 4):
                    return E_INVALID
                slots = block[m.rows_offset:m.rows_offset + 4 * m.n_rows].view(np.int32)
                if len(set(slots.tolist())) != m.n_rows or slots.min() < 0 or slots.max() >= m.capacity:
                    return E_INVALID
        C.memmove(_addr(host), _addr(members), RECORD * n)
        C.memmove(_addr(dev), _addr(host), nbytes)  # the one copy; the 'launch' reads the staging block only
        staged, call = _view(_addr(dev), nbytes), []
        for m in (_hip.GroupAddManyMember * n).from_address(_addr(dev)):
            pairs = staged[m.pairs_offset:m.pairs_offset + 8 * m.n_writes].view(np.int32).reshape(-1, 2)
            table = staged[m.rows_offset:m.rows_offset + 36 * m.n_rows].view(np.int32)
            slots, rows = table[:m.n_rows], table[m.n_rows:].reshape(-1, 8)
            _apply(m.ring_dev, m.frame_bytes, m.rows_dev, _addr(dev) + m.frames_offset, pairs, slots, rows)
            frames = staged[m.frames_offset:m.frames_offset + m.n_in * m.frame_bytes].reshape(m.n_in, -1).copy()
            call.append(dict(ring=m.ring_dev, n_in=m.n_in, pairs=pairs.tolist(), slots=slots.tolist(), rows=rows.copy(), frames=frames,
                             offsets=(m.pairs_offset, m.rows_offset, m.frames_offset), sizes=(m.n_frames, m.frame_bytes, m.capacity)))
        self.group_calls.append(call)
        return 0


def _allocate(self, frame):
    """``VectorReplayBuffer._allocate`` with host memory in place of the device and pinned allocations."""
    self._frame_shape, self._obs_dtype = tuple(frame.shape), frame.dtype
    self._frame_elems, self._itemsize = int(frame.size), int(frame.dtype.itemsize)
    self._frame_bytes = self._frame_elems * self._itemsize
    self._obs_shape = self._frame_shape + (self._stack_size,)
    self._n_frames = self._plan.n_frames
    self._frames = _Mem(np.full((self._n_frames, self._frame_bytes), 0xCD, np.uint8))
    self._meta_dev = _Mem(np.zeros((self._max_capacity, 8), np.int32))
    W, R, head = 64, 128, 5120
    self._block_pin = np.zeros((2, head + 32 * self._frame_bytes), np.uint8)
    self._block_dev = _Mem(np.zeros(head + 32 * self._frame_bytes, np.uint8))
    self._block = []
    for h in range(2):
        raw = self._block_pin[h]
        table = raw[:head].view(np.int32)
        self._block.append(dict(ptr=raw.ctypes.data, pairs=table[:2 * W].reshape(W, 2), row_slots=table[2 * W:2 * W + R],
                                rows=table[2 * W + R:].reshape(R, 8), frames=raw[head:].reshape(32, self._frame_bytes), event=_Event(), busy=False))
    self._half = 0


def _apply_growth(self, growth):
    new = np.full((growth.n_frames, self._frame_bytes), 0xCD, np.uint8)
    new[growth.dst] = self._frames.arr[growth.src]
    self._meta_dev.arr[:] = self._plan.rows
    self._frames, self._n_frames = _Mem(new), growth.n_frames


@pytest.fixture
def stub(monkeypatch):
    import torch

    from slimdqn import _hip
    from slimdqn.sample_collection.group_replay import GroupCollector
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    lib = _Lib()
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(VectorReplayBuffer, "_allocate", _allocate)
    monkeypatch.setattr(VectorReplayBuffer, "_apply_growth", _apply_growth)

    def alloc(self, nbytes):
        raw = [np.zeros(nbytes + 16, np.uint8) for _ in range(2)]
        pin, dev = (r[(-r.ctypes.data) % 16:][:nbytes] for r in raw)
        return pin, pin.ctypes.data, dev.ctypes.data, raw

    monkeypatch.setattr(GroupCollector, "_alloc_block", alloc)
    monkeypatch.setattr(GroupCollector, "_new_event", lambda self: _Event())
    return lib


# (frame shape, dtype, n_envs, capacity, stack, update_horizon, segment): frames of 32, 36 and 7 bytes; segments that wrap at once
KINDS = [((8,), np.float32, 2, 7, 1, 3, 6), ((9,), np.float32, 3, 12, 4, 1, 8), ((7,), np.uint8, 1, 5, 4, 3, 9)]


def _buffers(kinds=KINDS):
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    return [VectorReplayBuffer(UniformSamplingDistribution(g), batch_size=4, max_capacity=cap, stack_size=stack, update_horizon=n, gamma=0.99,
                               n_envs=E, segment=seg) for g, (_, _, E, cap, stack, n, seg) in enumerate(kinds)]


def _twins(kinds=KINDS):
    return VectorTwins(_buffers(kinds), _buffers(kinds), ring=lambda rb: rb._frames.arr, rows=lambda rb: rb._meta_dev.arr)


def _scripts(kinds, steps, **kw):
    return [make_vector_script(10 + g, E, shape, dtype, steps, **kw) for g, (shape, dtype, E, *_) in enumerate(kinds)]


def test_staged_tables_equal_each_members_plan_step(stub):
    """40 scripted steps of three members (E = 2, 3, 1; stacks 1 and 4; every segment wraps, mirror writes, several rows per
    episode end, idle time lines, a step without member 1): the records, offsets and tables of every call equal what a shadow
    ``SegmentPlan`` per member plans, and the buffers equal their solo twins after every step."""
    from slimdqn.sample_collection.group_replay import GroupVectorCollector
    from slimdqn.sample_collection.vector_replay_buffer import SegmentPlan

    twins = _twins()
    col = GroupVectorCollector(twins.group, force=True)
    shadows = [SegmentPlan(E, cap, stack, n, 0.99, seg) for (_, _, E, cap, stack, n, seg) in KINDS]
    scripts = _scripts(KINDS, 40)
    scripts[1][5] = [None] * 3  # member 1 has no frame at all at step 5
    mirrors = 0
    for t in range(40):
        entries = [s[t] for s in scripts]
        stub.group_calls.clear(), stub.step_calls.clear()
        twins.step(col, entries)
        twins.check(f"step {t}")
        want = []
        for g, (plan, row) in enumerate(zip(shadows, entries)):
            if all(tr is None for tr in row):
                continue
            step = plan.plan_step(row)
            if step.growth is None:
                slots = list(dict.fromkeys(k % plan.capacity for k in reversed(step.keys)))[::-1]
                want.append((g, step, slots, [np.ascontiguousarray(tr.observation).view(np.uint8).reshape(-1) for tr in row if tr is not None]))
        assert len(stub.group_calls) == (1 if want else 0)
        if not want:
            continue
        call, at = stub.group_calls[0], RECORD * len(want)
        assert len(call) == len(want)
        for rec, (g, step, slots, frames) in zip(call, want):
            rb = twins.group[g]
            assert rec["ring"] == rb._frames.data_ptr() and rec["sizes"] == (rb._n_frames, rb._frame_bytes, rb._max_capacity)
            assert rec["n_in"] == len(step.frame_envs) == len(frames) and rec["pairs"] == [list(w) for w in step.writes]
            assert rec["slots"] == slots and np.array_equal(rec["rows"], shadows[g].rows[slots])
            assert np.array_equal(rec["frames"], np.stack(frames))
            assert rec["offsets"][:2] == (at, at + 8 * len(step.writes))  # tables back to back, in member order
            at += 8 * len(step.writes) + 36 * len(slots)
            mirrors += len(step.writes) - len(frames)
        for rec, (g, step, slots, frames) in zip(call, want):  # then the frames, each member's at the next multiple of 16
            at = (at + 15) & ~15
            assert rec["offsets"][2] == at
            at += len(frames) * twins.group[g]._frame_bytes
    assert mirrors > 0 and col.group_calls >= 30 and all(rb._add_count > rb._max_capacity for rb in twins.group)


def test_slot_collision_keeps_the_last_keys_row(stub):
    """A capacity below a step's elements: a slot is named twice in one step and the last key's row must win, as in ``add_many``."""
    from slimdqn.sample_collection.group_replay import GroupVectorCollector

    kinds = [((8,), np.float32, 3, 2, 1, 3, 8), ((3,), np.float32, 2, 2, 2, 2, 8)]
    twins = VectorTwins(_buffers(kinds), _buffers(kinds), ring=lambda rb: rb._frames.arr, rows=lambda rb: rb._meta_dev.arr)
    col = GroupVectorCollector(twins.group, force=True)
    collided = 0
    for t, entries in enumerate(zip(*_scripts(kinds, 30, lengths=(4, 4, 4), p_none=0.0))):
        before = [rb._add_count for rb in twins.group]
        twins.step(col, list(entries))
        twins.check(f"step {t}")
        collided += sum(rb._add_count - b > rb._max_capacity for rb, b in zip(twins.group, before))
    assert collided > 0 and col.group_calls == 30


def test_fallbacks_growth_row_cap_foreign_member_and_refusal(stub):
    from slimdqn.sample_collection.group_replay import GroupVectorCollector
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    # growth: one-transition episodes make no element but use up the frames an old element still needs
    kinds = [((8,), np.float32, 2, 30, 2, 1, 6), ((8,), np.float32, 2, 30, 1, 1, 64)]
    twins = _twins(kinds)
    col = GroupVectorCollector(twins.group, force=True)
    rng = np.random.default_rng(0)
    tr = lambda end: TransitionElement(rng.standard_normal(8).astype(np.float32), 1, 0.5, False, end)
    for t in range(14):
        stub.step_calls.clear()
        grown = twins.group[0]._plan.n_growths
        twins.step(col, [[tr(t >= 4), tr(t >= 4)], [tr(False), tr(False)]])
        twins.check(f"growth step {t}")
        own = [c for c in stub.step_calls if c[0] == twins.group[0]._frames.data_ptr()]
        assert len(own) == (1 if twins.group[0]._plan.n_growths != grown else 0), t  # the member that grew sent its own step
    assert twins.growths[0] >= 1 and twins.group[0]._plan.n_growths == twins.growths[0] and col.group_calls == 14

    # more than 128 rows: 32 time lines whose episodes end together, update_horizon 5 -> 160 rows in that step
    kinds = [((8,), np.float32, 32, 400, 1, 5, 40), ((8,), np.float32, 2, 30, 1, 1, 64)]
    twins = _twins(kinds)
    col = GroupVectorCollector(twins.group, force=True)
    most = 0
    for t, entries in enumerate(zip(*_scripts(kinds, 16, lengths=(7,), p_none=0.0))):
        stub.group_calls.clear(), stub.step_calls.clear()
        before = twins.group[0]._add_count
        twins.step(col, list(entries))
        twins.check(f"row-cap step {t}")
        rows = twins.group[0]._add_count - before
        most = max(most, rows)
        big = [c for c in stub.step_calls if c[0] == twins.group[0]._frames.data_ptr()]
        assert len(big) == (2 if rows > 128 else 0) and len(stub.group_calls[0]) == (1 if rows > 128 else 2), (t, rows)
    assert most > 128

    # a member that is not a VectorReplayBuffer goes through its own add; the others share the call
    kinds = KINDS[:2]
    twins = _twins(kinds)
    foreign, adds = ReplayBuffer(UniformSamplingDistribution(9), batch_size=4, max_capacity=9, stack_size=1, update_horizon=1, gamma=0.99), []
    foreign.add = lambda t, **kw: adds.append(t)
    col = GroupVectorCollector(twins.group + [foreign], force=True)
    assert col._vector == [True, True, False]

    class _WithForeign:
        def add_many(self, entries, members=None, **kw):
            col.add_many(list(entries) + [[tr(False)]], **kw)

    for t, entries in enumerate(zip(*_scripts(kinds, 6))):
        twins.step(_WithForeign(), list(entries))
        twins.check(f"foreign step {t}")
    assert len(adds) == 6 and col.group_calls == 6

    # the entry refuses the first call: the flag is set, this call's device halves go through replay_add_step, and so does
    # everything after; a refusal after the entry has served is an error, as with GroupCollector
    from slimdqn import _hip

    twins = _twins()
    col = GroupVectorCollector(twins.group, force=True)
    scripts = _scripts(KINDS, 12)
    for t in range(8):
        stub.refuse = t == 0
        stub.group_calls.clear(), stub.step_calls.clear()
        twins.step(col, [s[t] for s in scripts])
        twins.check(f"refusal step {t}")
        assert col.__dict__.get("_group_add_many_ok") is False and not stub.group_calls
    assert col.group_calls == 0
    served = GroupVectorCollector(_buffers(), force=True)
    served.add_many([s[0] for s in scripts])
    stub.refuse = True
    with pytest.raises(_hip.HipExtensionError):
        served.add_many([s[1] for s in scripts])
    stub.refuse = False

    # force=False: the members' own add_many; no force: the sizes of the default table
    twins = _twins()
    sizes = GroupVectorCollector.group_add_many_sizes
    assert all(1 <= s <= 32 for s in sizes)
    for k, col in enumerate((GroupVectorCollector(twins.group, force=False), GroupVectorCollector(twins.group))):
        for t in range(4 * k, 4 * k + 4):
            stub.group_calls.clear()
            entries = [s[t] for s in scripts]
            stepping = sum(any(tr is not None for tr in row) for row in entries)
            twins.step(col, entries)
            twins.check(f"default step {t}")
            assert len(stub.group_calls) == (1 if k == 1 and stepping in sizes else 0)


def test_add_many_host_then_issue_is_add_many(stub):
    """``_add_many_host`` followed by the device half leaves planner, sampler, counters, ring and rows as ``add_many`` leaves them --
    and with the issue stubbed out, everything on the host side still."""

    class _ByHalves:
        def __init__(self, rbs, issue):
            self.rbs, self.issue = rbs, issue

        def add_many(self, entries, members=None, **kw):
            for rb, row in zip(self.rbs, entries):
                host = rb._add_many_host(row, **kw)
                assert (host is None) == all(tr is None for tr in row)
                if host is not None and self.issue:
                    rb._issue_step(*host)

    twins = _twins()
    scripts = _scripts(KINDS, 30)
    scripts[0][7] = [None] * 2
    for t in range(30):
        twins.step(_ByHalves(twins.group, True), [s[t] for s in scripts])
        twins.check(f"step {t}")
    # no device half at all: the host state is add_many's, the 'device' untouched
    roomy = [k[:6] + (64,) for k in KINDS]  # (segments that never grow: growth is part of the host half and sends every row again)
    solo, group = _buffers(roomy), _buffers(roomy)
    for t in range(30):
        for a, b, s in zip(solo, group, scripts):
            a.add_many(s[t])
            host = b._add_many_host(s[t])
            if host is not None:
                frames, writes, slots = host
                assert len(frames) == sum(tr is not None for tr in s[t]) and len(set(slots)) == len(slots)
                assert [w[0] for w in writes] == sorted(w[0] for w in writes) and {w[0] for w in writes} == set(range(len(frames)))
    for a, b in zip(solo, group):
        pa, pb = a._plan, b._plan
        assert a._add_count == b._add_count and (pa.frame_count, pa.add_count, pa.segment) == (pb.frame_count, pb.add_count, pb.segment)
        assert np.array_equal(pa.rows, pb.rows) and [list(d) for d in pa._live] == [list(d) for d in pb._live]
        assert list(a._sampling_distribution._index_to_key) == list(b._sampling_distribution._index_to_key)
        assert pb.n_growths == 0 and (b._frames.arr == 0xCD).all() and not b._meta_dev.arr.any() and a._meta_dev.arr.any()


# ---- SeedVectorTrainer on stub agents, environments and buffers ---------------------------------------------------------------
class _Agent:
    """Logs what the trainer asks of it; its greedy action is a function of (agent, state, head)."""
    params, n_networks, update_to_data, target_update_frequency = None, 3, 1, 10

    def __init__(self, g, log):
        self.g, self.log = g, log

    def action(self, state, head):
        self.log.append(("greedy", np.asarray(state).tobytes(), int(head)))
        return int(abs(float(np.asarray(state).reshape(-1)[0]) * 1000 + head + self.g)) % 4

    def best_actions(self, params, states, keys):
        from slimdqn import prng

        assert len(states) <= 32
        return np.asarray([self.action(s, prng.randint(k, 0, self.n_networks)) for s, k in zip(states, keys)], np.int64)

    def update_params_many(self, first, n, rb):
        self.log.append(("update_params_many", first, n))
        return [(s, {"loss": float(s + self.g)}) for s in range(first, first + n) if s % self.target_update_frequency == 0]

    def get_model(self):
        return {"g": self.g}


class _Group:
    """``AgentGroup``'s face for the trainer: shared acting and learner calls over the stub agents, sizes recorded."""

    def __init__(self, agents):
        self.agents, self.act_sizes, self.learn_calls = agents, [], 0

    def _stock(self):
        return True

    def select_heads(self, keys, members):
        from slimdqn import prng

        return [prng.randint(k, 0, self.agents[m].n_networks) for k, m in zip(keys, members)]

    def best_actions(self, which, heads, states, members):
        self.act_sizes.append(len(states))
        assert 1 <= len(states) <= 32 and which == 0 and list(members) == sorted(members)
        return np.asarray([self.agents[m].action(s, h) for m, h, s in zip(members, heads, states)], np.int64)

    def update_params_many(self, first, n, rbs):
        self.learn_calls += 1
        return [a.update_params_many(first, n, rb) for a, rb in zip(self.agents, rbs)]

    def close(self):
        pass


class _RB:
    _clipping = None

    def __init__(self, log):
        self.log = log

    def add_many(self, transitions):
        self.log.append(("add_many", [None if t is None else (t.observation.tobytes(), t.action, t.reward, t.is_terminal, t.episode_end) for t in transitions]))


class _Logger:
    def __init__(self, events):
        self.events, self.records = events, []

    def log(self, record):
        self.events.append(("log", sorted(record.items())))
        self.records.append(record)


def _seed(g, E, n_epochs, budget):
    from slimdqn.environments.synthetic import SyntheticVector

    log = []
    logger = _Logger(log)
    p = dict(seed=g, epsilon_end=0.05, epsilon_duration=40, n_epochs=n_epochs, n_training_steps_per_epoch=budget, n_initial_samples=21, horizon=9,
             wandb=logger)
    envs = [SyntheticVector(100 * g + e, episode_length=(7, 5, 11, 4)[(e + g) % 4]) for e in range(E)]
    return log, p, _Agent(g, log), envs, _RB(log)


@pytest.mark.parametrize("S,E,epochs", [(5, 8, (2, 2, 2, 2, 2)), (3, 2, (1, 3, 2)), (1, 3, (2,))])
def test_seed_vector_trainer_call_sequence_is_vector_trainers(S, E, epochs):
    """Per seed: the same greedy states and heads, transitions, learner runs, log records and saves, in the same order, as a
    ``VectorTrainer`` alone on the same key -- with seeds that finish at different times -- and no acting call above 32 states."""
    from experiments.base.dqn import VectorTrainer
    from experiments.base.seeds import SeedVectorTrainer
    from slimdqn import prng
    from slimdqn.sample_collection.group_replay import GroupVectorCollector

    mk = lambda: [_seed(g, E, epochs[g], 60 + 10 * g) for g in range(S)]
    solo, together = mk(), mk()
    save = lambda store: (lambda p, returns, lengths, model: store.append((p["seed"], returns, lengths, model)))
    want_saves, got_saves, want_out = [], [], []
    for g, (log, p, agent, envs, rb) in enumerate(solo):
        want_out.append(VectorTrainer(prng.PRNGKey(70 + g), p, agent, envs, rb, save_fn=save(want_saves)).run())
    group = _Group([s[2] for s in together])
    trainer = SeedVectorTrainer([prng.PRNGKey(70 + g) for g in range(S)], [s[1] for s in together], group.agents, [s[3] for s in together],
                                [s[4] for s in together], save_fn=save(got_saves), group=group,
                                collector=GroupVectorCollector([s[4] for s in together], force=True))
    got_out = trainer.run()
    for g in range(S):
        assert together[g][0] == solo[g][0], f"seed {g}: call sequence"
        assert [list(x) for x in got_out[g]] == [list(x) for x in want_out[g]]
        assert any(e[0] == "update_params_many" for e in solo[g][0]) and any(e[0] == "greedy" for e in solo[g][0])
    assert sorted(got_saves, key=lambda s: s[0]) == sorted(want_saves, key=lambda s: s[0]) and len(want_saves) == sum(epochs)
    assert group.act_sizes and max(group.act_sizes) <= 32 and group.learn_calls > 0
    if S * E > 32:
        assert max(group.act_sizes) == 32  # 40 greedy states went out as 32 + 8
