"""GPU: ``replay_group_add_step`` / ``GroupCollector.add_many`` against the buffers' own ``add``.  Two twin sets of buffers take
the same scripted transitions, one through ``rb.add``, one through ``add_many``; after EVERY step the counters, the host
mirrors, the element rows on the device, the ring bytes of every slot written so far (also against the frames that went in) and
the samplers' keys are compared byte for byte (tests/group_collect.py), at intervals ``sample()`` batches under equal sampler
seeds.  No tolerance anywhere: the call moves bytes."""
import ctypes as C

import numpy as np
import pytest

from group_collect import Twins, make_script

pytestmark = pytest.mark.gpu

# (frame shape, dtype, capacity, stack, update_horizon): one member per copy tier -- 32 B (16 B per lane), 12 B (4 B), 15 B
# (bytes) -- capacities 7 and 5 (FIFO eviction and row-slot wrap within 40 steps), an update_horizon of 3 (an episode end emits
# several rows in one step), and an Atari-shaped member (84 x 84 uint8, stack 4: two frame workgroups)
TIERS = [((8,), np.float32, 7, 1, 1), ((3,), np.float32, 5, 1, 3), ((5, 3), np.uint8, 5, 2, 1)]
ATARI = ((84, 84), np.uint8, 7, 4, 1)


def _buffers(kinds, sampler=None):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    sampler = sampler or (lambda g, cap: UniformSamplingDistribution(g))
    return [ReplayBuffer(sampler(g, cap), batch_size=4, max_capacity=cap, stack_size=stack, update_horizon=n, gamma=0.99)
            for g, (_, _, cap, stack, n) in enumerate(kinds)]


def _twins(kinds, sampler=None):
    return Twins(_buffers(kinds, sampler), _buffers(kinds, sampler), lambda rb: rb._frames.cpu().numpy(), lambda rb: rb._meta_dev.cpu().numpy())


def _scripts(kinds, steps, **kw):
    return [make_script(10 + g, shape, dtype, steps, terminal_every=7 + g % 5, truncate_every=5, **kw)
            for g, (shape, dtype, *_) in enumerate(kinds)]


def _same_batches(tw):
    for g, (a, b) in enumerate(zip(tw.solo, tw.group)):
        x, y = a.sample(), b.sample()
        for name in ("state", "action", "reward", "next_state", "is_terminal"):
            assert np.asarray(getattr(x, name)).tobytes() == np.asarray(getattr(y, name)).tobytes(), f"member {g}: {name} of a sampled batch"


@pytest.mark.parametrize("S", [1, 3, 32])
def test_add_many_equals_add(S):
    """40 lock-step collections (ten times the staging depth: every block is reused behind its event), steps 24-31 on a subset
    of the members (as after a seed finishes); S = 1: the Atari-shaped member alone, 3: one per tier, 32: all four kinds in turn."""
    from slimdqn.sample_collection.group_replay import GroupCollector

    kinds = {1: [ATARI], 3: TIERS}.get(S) or [(TIERS + [ATARI])[g % 4] for g in range(S)]
    tw = _twins(kinds)
    col, scripts = GroupCollector(tw.group, force=True), _scripts(kinds, 40)
    assert 40 > 3 * col.DEPTH
    at = [0] * S
    for t in range(40):
        members = [g for g in range(S) if g % 3 != 1] if 24 <= t < 32 and S > 1 else list(range(S))
        tw.step(col, [scripts[g][at[g]] for g in members], members)
        for g in members:
            at[g] += 1
        tw.check(where=f"step {t}")
        if t % 10 == 9:
            _same_batches(tw)
    assert col.group_calls == 40 and col._group_add_ok is True
    assert all(rb._add_count > rb._max_capacity for rb in tw.group), "FIFO eviction and slot wrap-around were reached"


def test_ring_growth_and_a_member_over_the_row_cap():
    """Member 1 (capacity 5) meets truncated one-transition episodes until its ring's slack is used up: one ``_grow_ring`` inside
    ``add_many``.  Member 0 (capacity 64) arrives with more than 32 rows pending from solo adds: it sends them itself and joins
    with none."""
    from slimdqn import _hip
    from slimdqn.sample_collection.group_replay import GroupCollector

    kinds = [((8,), np.float32, 64, 1, 1), ((3,), np.float32, 5, 1, 3), ((5, 3), np.uint8, 5, 2, 1)]
    tw = _twins(kinds)
    col = GroupCollector(tw.group, force=True)
    scripts = [make_script(1, (8,), np.float32, 150, terminal_every=9), make_script(2, (3,), np.float32, 100, truncate_from=12),
               make_script(3, (5, 3), np.uint8, 100, terminal_every=6)]
    for t in range(50):
        for rb in (tw.solo[0], tw.group[0]):
            rb.add(scripts[0][t])
        tw.frames[0].append(scripts[0][t].observation)
    assert tw.group[0]._add_count - tw.group[0]._flushed > _hip.REPLAY_GROUP_MAX_ROWS
    for t in range(100):
        tw.step(col, [scripts[0][50 + t], scripts[1][t], scripts[2][t]])
        tw.check(where=f"step {t}")
    assert tw.grown == [0, 1, 0] and col.group_calls == 100
    _same_batches(tw)


def test_prioritized_member_keeps_its_tree():
    import torch

    from slimdqn.sample_collection.per import SlotPrioritizedSampler
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.group_replay import GroupCollector

    sampler = lambda g, cap: SlotPrioritizedSampler(g, cap) if g == 1 else UniformSamplingDistribution(g)
    solo, group = _buffers(TIERS, sampler), _buffers(TIERS, sampler)
    col, scripts = GroupCollector(group, force=True), _scripts(TIERS, 30)
    for t in range(30):
        for g in range(3):
            solo[g].add(scripts[g][t])
        col.add_many([s[t] for s in scripts])
        torch.cuda.synchronize()
        a, b = solo[1], group[1]
        a._flush_meta()
        assert (a._add_count, a._t) == (b._add_count, b._t) and b._flushed == b._add_count
        assert np.array_equal(a._meta_dev.cpu().numpy(), b._meta_dev.cpu().numpy())
        sa, sb = a._sampling_distribution, b._sampling_distribution
        assert np.array_equal(sa._key_of_slot, sb._key_of_slot) and len(sa) == len(sb)
        assert sa._sum_tree._nodes_dev.cpu().numpy().tobytes() == sb._sum_tree._nodes_dev.cpu().numpy().tobytes(), f"step {t}: tree nodes"
    assert solo[1]._add_count > 5


def test_group_learner_step_after_the_adds():
    """``idqn_group_learn_on_replay_fc`` (AgentGroup) on the collected buffers against the same call on the twins: S = 3, the
    LunarLander net, B = 32."""
    import torch

    from slimdqn.networks.group import AgentGroup
    from slimdqn.sample_collection.group_replay import GroupCollector
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from test_gpu_seed_group import _agent, _same

    S = 3
    mk = lambda: [ReplayBuffer(UniformSamplingDistribution(g), batch_size=32, max_capacity=40, stack_size=1, update_horizon=2, gamma=0.99)
                  for g in range(S)]
    solo, group = mk(), mk()
    for rb in solo + group:
        rb.reuse_sample_buffers = True
    col = GroupCollector(group, force=True)
    scripts = [make_script(20 + g, (8,), np.float32, 70, terminal_every=7) for g in range(S)]
    ga, sa = [_agent("lunar", g) for g in range(S)], [_agent("lunar", g) for g in range(S)]
    gg, sg = AgentGroup(ga), AgentGroup(sa)
    for t in range(70):
        for g in range(S):
            solo[g].add(scripts[g][t])
        col.add_many([s[t] for s in scripts])
        if t >= 50:
            gg.update_online_params(t, group)
            sg.update_online_params(t, solo)
    torch.cuda.synchronize()
    assert col.group_calls == 70 and gg.__dict__.get("_group_learn_ok") is True and sg.__dict__.get("_group_learn_ok") is True
    for g in range(S):
        _same(ga[g], sa[g], f"member {g}")
        assert ga[g]._losses.cpu().numpy().tobytes() == sa[g]._losses.cpu().numpy().tobytes()
        assert np.isfinite(ga[g]._losses.cpu().numpy()).all() and ga[g]._count.cpu().numpy().min() >= 20
    gg.close(), sg.close()


def test_seed_trainer_is_the_same_with_and_without_the_collector(capsys):
    import torch

    from experiments.base.seeds import SeedTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.group_replay import GroupCollector
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    def run(force):
        S, saved = 3, []
        ps = [dict(seed=s, epsilon_end=0.01, epsilon_duration=60, n_epochs=2, n_training_steps_per_epoch=40, n_initial_samples=10 + 3 * s,
                   horizon=15, wandb=NullLogger()) for s in range(S)]
        rbs = [ReplayBuffer(UniformSamplingDistribution(s), batch_size=32, max_capacity=50 + 7 * s, stack_size=1, update_horizon=1, gamma=0.99)
               for s in range(S)]
        agents = [iDQN(s, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 20, 10) for s in range(S)]
        envs = [SyntheticVector(s, episode_length=11 + 2 * s) for s in range(S)]
        col = GroupCollector(rbs, force=force)
        st = SeedTrainer([prng.PRNGKey(s) for s in range(S)], ps, agents, envs, rbs, collector=col,
                         save_fn=lambda p, r, l, m: saved.append((p["seed"], [list(x) for x in r], [list(x) for x in l])))
        out = st.run()
        torch.cuda.synchronize()
        for rb in rbs:
            rb._flush_meta()
        state = [(a._online.cpu().numpy().tobytes(), a._target.cpu().numpy().tobytes(), rb._add_count, rb._t, rb._meta_dev.cpu().numpy().tobytes(),
                  rb._frames.cpu().numpy()[np.arange(max(0, rb._t - rb._n_frames), rb._t) % rb._n_frames].tobytes(),
                  list(rb._sampling_distribution._index_to_key)) for a, rb in zip(agents, rbs)]
        return out, saved, state, col.group_calls, st.total_steps

    on, off = run(True), run(False)
    assert on[3] >= 80 and off[3] == 0 and on[4] == off[4] >= 80
    assert on[0] == off[0], "returns and lengths"
    assert on[1] == off[1], "saved models' histories"
    for g, (a, b) in enumerate(zip(on[2], off[2])):
        assert a == b, f"seed {g}: final parameters or buffer contents differ"


def test_refusals_write_nothing():
    import torch

    from slimdqn import _hip

    lib, q = _hip.lib(), _hip.current_stream()
    rings = [torch.full((10, 32), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    rows = [torch.full((6, 8), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    pin = torch.zeros(4096, dtype=torch.uint8).pin_memory()
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    raw = pin.numpy()

    def call(n, edit=None, block=None, staging=None, members="table"):
        recs = (_hip.GroupAddMember * 33)()
        for g in range(2):
            m = recs[g]
            m.ring_dev, m.rows_dev, m.n_frames, m.frame_bytes, m.capacity = rings[g].data_ptr(), rows[g].data_ptr(), 10, 32, 6
            m.frame_offset, m.frame_slot, m.n_rows, m.rows_offset = 512 + 32 * g, 3 + g, 2, 128 + 72 * g
            raw[128 + 72 * g:128 + 72 * g + 8].view(np.int32)[:] = (1, 4)
            raw[128 + 72 * g + 8:128 + 72 * g + 72].view(np.int32)[:] = np.arange(16) + 100 * g
            raw[512 + 32 * g:544 + 32 * g] = 17 + g
        if edit:
            edit(recs)
        return lib.replay_group_add_step(n, None if members is None else C.addressof(recs), pin.data_ptr() if block is None else block,
                                         dev.data_ptr() if staging is None else staging, 576, q)

    def dup_ring(r):
        r[1].ring_dev = r[0].ring_dev

    def dup_rows(r):
        r[1].rows_dev = r[0].rows_dev

    def bad_frame_slot(r):
        r[1].frame_slot = 10

    def negative_frame_slot(r):
        r[0].frame_slot = -2

    def dup_row_slot(r):
        raw[128:136].view(np.int32)[:] = (4, 4)

    def bad_row_slot(r):
        raw[200:208].view(np.int32)[:] = (1, 6)

    def too_many_rows(r):
        r[0].n_rows = _hip.REPLAY_GROUP_MAX_ROWS + 1

    def misaligned_frame(r):
        r[0].frame_offset = 520

    def frame_leaves_block(r):
        r[1].frame_offset = 560

    for edit in (dup_ring, dup_rows, bad_frame_slot, negative_frame_slot, dup_row_slot, bad_row_slot, too_many_rows, misaligned_frame, frame_leaves_block):
        assert call(2, edit) == _hip.E_INVALID, edit.__name__
        assert lib.idqn_last_error().decode().startswith("replay_group_add_step"), edit.__name__
    assert call(0) == _hip.E_INVALID and call(33) == _hip.E_INVALID
    assert call(2, members=None) == _hip.E_INVALID
    assert call(2, block=pin.data_ptr() + 4) == _hip.E_INVALID and call(2, staging=dev.data_ptr() + 8) == _hip.E_INVALID
    torch.cuda.synchronize()
    assert all((r.cpu().numpy() == 0xAB).all() for r in rings) and all((r.cpu().numpy() == -7).all() for r in rows), "a refused call wrote"
    assert (dev.cpu().numpy() == 0).all(), "a refused call copied its block"
    # ... and the same table, unedited, is taken: frames to slots 3 and 4, rows to slots 1 and 4 of each member
    assert call(2) == 0
    torch.cuda.synchronize()
    for g in range(2):
        ring, row = rings[g].cpu().numpy(), rows[g].cpu().numpy()
        assert (ring[3 + g] == 17 + g).all() and (np.delete(ring, 3 + g, 0) == 0xAB).all()
        assert np.array_equal(row[[1, 4]].reshape(-1), np.arange(16) + 100 * g) and (np.delete(row, [1, 4], 0) == -7).all()
