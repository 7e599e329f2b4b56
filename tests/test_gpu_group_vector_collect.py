"""GPU: one vector step of S seeds x E time lines as one call -- ``replay_group_add_many`` / ``GroupVectorCollector`` against every
member's own ``add_many`` on twin buffers (tests/group_vector_collect.py), the entry's refusals, the group learner step on the
collected rings, and ``SeedVectorTrainer`` against S ``VectorTrainer`` runs.  Every comparison is byte for byte, WITHOUT a tolerance:
the call moves bytes and the trainers make the same device calls on the same inputs.

Shapes: the smallest at which the kernel can go wrong -- frames of 32 B (16-byte tier), 36 B (4-byte tier), 7 B (byte tier) and
64 x 4 uint8; E = 1, 2 and 3 in one group; stacks 1 and 4 with capacities of 5 to 12 elements and segments of 6 to 9 frames, so that
every segment wraps, mirror slots are written and rings grow within 40 steps; ``update_horizon`` 3 (several rows per episode end);
idle time lines and a step in which a member has no frame; a capacity below a step's elements; 160 rows in one step."""
import ctypes as C

import numpy as np
import pytest

from group_vector_collect import VectorTwins, make_vector_script

pytestmark = pytest.mark.gpu

RECORD = 80  # sizeof(replay_group_many_member_t)

# name -> (steps, [(frame shape, dtype, n_envs, capacity, stack, update_horizon, segment)])
GROUPS = {
    "three_tiers_E123": (40, [((8,), np.float32, 1, 5, 1, 3, 6), ((9,), np.float32, 2, 12, 4, 3, 8), ((7,), np.uint8, 3, 9, 4, 3, 9)]),
    "wide_frame_and_collision": (30, [((64, 4), np.uint8, 2, 8, 4, 3, 7), ((8,), np.float32, 3, 2, 1, 3, 8)]),
    "row_cap": (9, [((8,), np.float32, 32, 400, 1, 5, 40), ((3,), np.float32, 2, 6, 2, 1, 6)]),
}


def _sampler(g, capacity, prioritized):
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution

    # (a key is added before the oldest one is removed: the tree holds one entry more than the buffer)
    return PrioritizedSamplingDistribution(g, capacity + 1) if prioritized else UniformSamplingDistribution(g)


def _buffers(kinds, prioritized=False):
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    return [VectorReplayBuffer(_sampler(g, cap, prioritized), batch_size=4, max_capacity=cap, stack_size=stack, update_horizon=n, gamma=0.99,
                               n_envs=E, segment=seg) for g, (_, _, E, cap, stack, n, seg) in enumerate(kinds)]


def _ring(rb):
    return rb._frames.cpu().numpy()


def _rows(rb):
    return rb._meta_dev.cpu().numpy()


def _trees(a, b, tag):
    import torch

    torch.cuda.synchronize()
    ta, tb = a._sampling_distribution._sum_tree, b._sampling_distribution._sum_tree
    assert ta._nodes_dev.cpu().numpy().tobytes() == tb._nodes_dev.cpu().numpy().tobytes(), f"{tag}: sum tree"
    assert ta.max_recorded_priority == tb.max_recorded_priority, tag
    assert a._sampling_distribution._i2k_dev.cpu().numpy().tobytes() == b._sampling_distribution._i2k_dev.cpu().numpy().tobytes(), f"{tag}: device key map"


def _scripts(kinds, steps, **kw):
    return [make_vector_script(20 + g, E, shape, dtype, steps, **kw) for g, (shape, dtype, E, *_) in enumerate(kinds)]


@pytest.mark.parametrize("name", list(GROUPS))
def test_collector_equals_every_members_add_many(name):
    from slimdqn.sample_collection.group_replay import GroupVectorCollector

    steps, kinds = GROUPS[name]
    twins = VectorTwins(_buffers(kinds), _buffers(kinds), _ring, _rows)
    col = GroupVectorCollector(twins.group, force=True)
    scripts = _scripts(kinds, steps, **(dict(lengths=(7,), p_none=0.0) if name == "row_cap" else {}))
    if name == "three_tiers_E123":
        scripts[1][5] = [None] * 2  # a step in which member 1 has no frame at all
    most_rows, collided, mirrors = 0, 0, 0
    for t in range(steps):
        before = [rb._add_count for rb in twins.group]
        twins.step(col, [s[t] for s in scripts])
        twins.check(f"{name} step {t}")
        made = [rb._add_count - b for rb, b in zip(twins.group, before)]
        most_rows, collided = max(most_rows, max(made)), collided + sum(m > rb._max_capacity for m, rb in zip(made, twins.group))
    assert col.__dict__.get("_group_add_many_ok") is True and col.group_calls >= steps // 2
    for rb in twins.group:
        p = rb._plan
        mirrors += sum(p.mirror_slot(e, t) is not None for e in range(p.n_envs) for t in range(p.frame_count[e]))
    if name == "three_tiers_E123":
        assert sum(twins.growths) >= 1 and mirrors > 0 and all(rb._add_count > rb._max_capacity for rb in twins.group)
        assert all(max(rb._plan.frame_count) > rb._plan.segment or g for rb, g in zip(twins.group, twins.growths))  # wrapped, or grew
    if name == "wide_frame_and_collision":
        assert collided > 0 and mirrors > 0
    if name == "row_cap":
        assert most_rows > 128  # that member took its own two replay_add_step calls, the other one the group call


def test_prioritized_members_keep_their_tree_updates():
    """S = 2 prioritized members: the keys, the device key map and the sum tree (the sampler's own launches, which the collector
    leaves alone) after every step, and the draws from them."""
    from slimdqn.sample_collection.group_replay import GroupVectorCollector

    kinds = GROUPS["three_tiers_E123"][1][:2]
    twins = VectorTwins(_buffers(kinds, True), _buffers(kinds, True), _ring, _rows, extra=_trees)
    col = GroupVectorCollector(twins.group, force=True)
    scripts = _scripts(kinds, 25)
    for t in range(25):
        twins.step(col, [s[t] for s in scripts], priority=0.5 + (t % 3))
        twins.check(f"prioritized step {t}")
    assert col.group_calls >= 23


class _Table:
    """A valid two-member call laid out by hand from the header's description: member 0 two 32-byte frames, three writes, two
    rows; member 1 one 36-byte frame, one write, one row."""

    def __init__(self):
        import torch

        from slimdqn import _hip

        self.rings = [torch.full((9, 32), 0xCD, dtype=torch.uint8, device="cuda"), torch.full((6, 36), 0xCD, dtype=torch.uint8, device="cuda")]
        self.rows = [torch.full((16, 8), -5, dtype=torch.int32, device="cuda"), torch.full((4, 8), -5, dtype=torch.int32, device="cuda")]
        self.pin = torch.zeros(1024, dtype=torch.uint8).pin_memory()
        self.dev = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        self.raw = self.pin.numpy()
        self.i32 = self.raw.view(np.int32)
        self.recs = (_hip.GroupAddManyMember * 2)()
        self.fill()

    def fill(self):
        self.raw[:] = 0
        head = 2 * RECORD
        self.i32[head // 4:head // 4 + 6] = [0, 3, 1, 8, 1, 0]
        self.i32[head // 4 + 6:head // 4 + 8] = [15, 0]
        self.i32[head // 4 + 8:head // 4 + 24] = 7
        at = head + 24 + 72
        self.i32[at // 4:at // 4 + 2] = [0, 5]
        self.i32[at // 4 + 2] = 3
        self.i32[at // 4 + 3:at // 4 + 11] = 9
        end = at + 8 + 36
        f0 = (end + 15) & ~15
        f1 = (f0 + 64 + 15) & ~15
        self.raw[f0:f0 + 32], self.raw[f0 + 32:f0 + 64], self.raw[f1:f1 + 36] = 1, 2, 3
        self.nbytes = f1 + 36
        vals = [(self.rings[0], self.rows[0], 9, 32, 16, 2, 3, 2, head, head + 24, f0), (self.rings[1], self.rows[1], 6, 36, 4, 1, 1, 1, at, at + 8, f1)]
        for r, (ring, rows, nf, fb, cap, n_in, nw, nr, po, ro, fo) in zip(self.recs, vals):
            r.ring_dev, r.rows_dev, r.n_frames, r.frame_bytes, r.capacity = ring.data_ptr(), rows.data_ptr(), nf, fb, cap
            r.n_in, r.n_writes, r.n_rows, r.reserved, r.pairs_offset, r.rows_offset, r.frames_offset = n_in, nw, nr, 0, po, ro, fo

    def call(self, n=2, recs="own", pin="own", dev="own", nbytes=None):
        import torch

        from slimdqn import _hip

        recs = C.addressof(self.recs) if recs == "own" else recs
        pin = self.pin.data_ptr() if pin == "own" else pin
        dev = self.dev.data_ptr() if dev == "own" else dev
        rc = _hip.lib().replay_group_add_many(n, recs, pin, dev, self.nbytes if nbytes is None else nbytes, _hip.current_stream())
        torch.cuda.synchronize()
        return rc, _hip.lib().idqn_last_error().decode()

    def untouched(self):
        return all((r.cpu().numpy() == 0xCD).all() for r in self.rings) and all((r.cpu().numpy() == -5).all() for r in self.rows)


def test_refusals_one_by_one_leave_the_buffers_unchanged():
    from slimdqn import _hip

    t = _Table()
    head = 2 * RECORD

    def refused(text, mutate=None, **kw):
        t.fill()
        if mutate is not None:
            mutate(t)
        rc, msg = t.call(**kw)
        assert rc == _hip.E_INVALID and text in msg and "replay_group_add_many" in msg, (text, rc, msg)
        assert t.untouched(), text

    def setf(g, **fields):
        def m(t):
            for k, v in fields.items():
                setattr(t.recs[g], k, v)
        return m

    def poke(offset_of, index, value):
        def m(t):
            t.i32[offset_of(t) // 4 + index] = value
        return m

    refused("null pointer", recs=None)
    refused("null pointer", pin=None)
    refused("null pointer", dev=None)
    refused("null ring or rows", setf(1, ring_dev=None))
    refused("null ring or rows", setf(0, rows_dev=None))
    refused("outside [1, 32]", n=0)
    refused("outside [1, 32]", n=33)
    refused("16-byte aligned", pin=t.pin.data_ptr() + 4)
    refused("16-byte aligned", dev=t.dev.data_ptr() + 8)
    refused("n_in is outside", setf(0, n_in=33))
    refused("n_writes is outside", setf(0, n_writes=65))
    refused("n_rows is outside", setf(1, n_rows=129))
    refused("neither a write nor a row", setf(1, n_writes=0, n_rows=0))
    refused("writes without a frame", setf(1, n_in=0))
    refused("pair table", setf(0, pairs_offset=head + 2))
    refused("pair table", setf(0, pairs_offset=head - 8))
    refused("pair table", setf(1, pairs_offset=1 << 40))
    refused("row table", setf(0, rows_offset=-4))
    refused("row table", lambda t: setattr(t.recs[1], "rows_offset", t.nbytes - 32))
    refused("the frames", lambda t: setattr(t.recs[0], "frames_offset", t.recs[0].frames_offset + 4))
    refused("the frames", lambda t: setattr(t.recs[1], "frames_offset", t.nbytes - 32))
    refused("the frames", nbytes=t.nbytes - 1)
    refused("block_bytes", nbytes=head - 1)
    refused("source index", poke(lambda t: t.recs[0].pairs_offset, 2, 2))
    refused("ring slot is outside", poke(lambda t: t.recs[0].pairs_offset, 3, 9))
    refused("ring slot is outside", poke(lambda t: t.recs[1].pairs_offset, 1, -1))
    refused("element slot is outside", poke(lambda t: t.recs[0].rows_offset, 0, 16))
    refused("element slot is outside", poke(lambda t: t.recs[1].rows_offset, 0, 4))  # inside the ring, outside the capacity
    refused("ring slot is written twice", poke(lambda t: t.recs[0].pairs_offset, 5, 3))
    refused("element slot is written twice", poke(lambda t: t.recs[0].rows_offset, 1, 15))
    refused("same ring", lambda t: setattr(t.recs[1], "ring_dev", t.rings[0].data_ptr()))
    refused("same rows", lambda t: setattr(t.recs[1], "rows_dev", t.rows[0].data_ptr()))
    # ... and the same table with nothing wrong goes through, writes exactly what it names, and the records travel in the block
    t.fill()
    rc, msg = t.call()
    assert rc == 0, msg
    r0, r1 = t.rings[0].cpu().numpy(), t.rings[1].cpu().numpy()
    assert (r0[3] == 1).all() and (r0[8] == 2).all() and (r0[0] == 2).all() and (np.delete(r0, [0, 3, 8], 0) == 0xCD).all()
    assert (r1[5] == 3).all() and (r1[:5] == 0xCD).all()
    m0, m1 = t.rows[0].cpu().numpy(), t.rows[1].cpu().numpy()
    assert (m0[[0, 15]] == 7).all() and (m0[1:15] == -5).all() and (m1[3] == 9).all() and (m1[:3] == -5).all()
    assert t.dev.cpu().numpy()[:head].tobytes() == bytes(t.recs)


def test_group_learner_steps_on_the_collected_rings():
    """Behind the adds: one ``idqn_group_learn_steps_on_replay_fc`` call (n = 2, B = 4) on the rings the collector filled, against
    the same call on the rings the members' own ``add_many`` filled -- every arena of every member."""
    import torch

    from slimdqn.sample_collection.group_replay import GroupVectorCollector
    from test_gpu_seed_group import _Group, _agent, _same

    kinds = [((8,), np.float32, 2, 40, 1, 2, 24), ((8,), np.float32, 3, 30, 1, 2, 16)]
    twins = VectorTwins(_buffers(kinds), _buffers(kinds), _ring, _rows)
    col = GroupVectorCollector(twins.group, force=True)
    for t, entries in enumerate(zip(*_scripts(kinds, 30))):
        twins.step(col, list(entries))
    twins.check("before the learner call")
    slots = np.stack([np.stack([np.asarray(rb.sample_slots(), np.int32) for _ in range(2)]) for rb in twins.group])  # [S][n = 2][B = 4]
    agents = [[_agent("lunar", g) for g in range(2)] for _ in range(2)]
    for side, rbs in zip(agents, (twins.solo, twins.group)):
        group = _Group(side)
        assert group.learn_steps(rbs, slots) == 0
        torch.cuda.synchronize()
        group.close()
    for g in range(2):
        _same(agents[0][g], agents[1][g], f"member {g}")
        assert int(agents[1][g]._count[0].item()) == 2


def _trainer_side(S, E, p_over=None):
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    out = []
    for g in range(S):
        p = dict(seed=g, epsilon_end=0.05, epsilon_duration=80, n_epochs=2, n_training_steps_per_epoch=100 + 20 * g, n_initial_samples=40, horizon=30,
                 wandb=NullLogger())
        agent = iDQN(prng.PRNGKey(200 + g), 8, 4, 2, [16], "fc", 1e-3, 0.99, 1, 1, 20, 5, adam_eps=1e-8)
        envs = [SyntheticVector(10 * g + e, episode_length=(13, 9)[e % 2]) for e in range(E)]
        rb = VectorReplayBuffer(UniformSamplingDistribution(g), 32, 150, stack_size=1, update_horizon=1, gamma=0.99, n_envs=E)
        rb.reuse_sample_buffers = True
        out.append((prng.PRNGKey(300 + g), p, agent, envs, rb))
    return out


@pytest.mark.parametrize("force", [True, False])
def test_seed_vector_trainer_equals_vector_trainers(force):
    """S = 2, E = 2, two epochs of 100 and 120 steps per seed (a few hundred lock-step iterations, the second seed outliving the
    first), LunarLander net at K = 2, features [16]: parameters, target, Adam moments, counters, loss sums, replay rows and rings,
    sampler generator and every log record against ``VectorTrainer`` alone on the same key.  Collector forced on -- and the
    n-step learner calls taken from runs of 2 on, so that the persistent group kernel runs -- and forced off with the defaults."""
    import torch

    from experiments.base.dqn import VectorTrainer
    from experiments.base.seeds import SeedVectorTrainer
    from slimdqn.sample_collection.group_replay import GroupVectorCollector
    from test_gpu_seed_group import _same

    S, E = 2, 2
    solo, together = _trainer_side(S, E), _trainer_side(S, E)
    if force:  # a vector step owes E = 2 gradient steps, below the default threshold of the n-step calls: lower it on both sides
        for side in solo + together:
            side[2].learn_steps_min = 2
    want = [VectorTrainer(*side).run() for side in solo]
    keys, ps, agents, envs, rbs = (list(x) for x in zip(*together))
    collector = GroupVectorCollector(rbs, force=force)
    trainer = SeedVectorTrainer(keys, ps, agents, envs, rbs, collector=collector)
    group = trainer.group
    got = trainer.run()
    torch.cuda.synchronize()
    assert (collector.group_calls > 100) == force
    assert group.__dict__.get("_group_act_ok") is True and group.__dict__.get("_group_learn_ok") is True
    assert group.__dict__.get("_group_steps_ok") is (True if force else None)  # the persistent group kernel served the runs of 2
    for g in range(S):
        _same(agents[g], solo[g][2], f"seed {g}")
        a, b = rbs[g], solo[g][4]
        assert a._add_count == b._add_count > 150 and np.array_equal(a._plan.rows, b._plan.rows)
        assert np.array_equal(_rows(a), _rows(b)) and np.array_equal(_rows(a), a._plan.rows)
        live = np.unique(a._plan.rows[:, [0, 2]])
        assert np.array_equal(_ring(a)[live], _ring(b)[live])
        assert a._sampling_distribution._rng_key.bit_generator.state == b._sampling_distribution._rng_key.bit_generator.state
        assert ps[g]["wandb"].records == solo[g][1]["wandb"].records and sum("epoch" in r for r in ps[g]["wandb"].records) == 2
        assert any("loss" in r for r in ps[g]["wandb"].records) and int(agents[g]._count[0].item()) > 100
        assert [list(x) for x in got[g]] == [list(x) for x in want[g]]
