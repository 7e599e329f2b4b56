"""GPU: vector-environment collection on the device -- ``replay_add_step`` against the numpy model, ``VectorReplayBuffer``
against the host oracle, the replay-sourced learner steps on the segmented ring (bit-identical to gather + learn: the layout's
whole point is that the existing kernels read it unmodified), and a short ``VectorTrainer`` loop.

The stream generator, the oracle (one ``TrajectoryAccumulator.push`` per environment, keys interleaved in environment order,
FIFO of ``max_capacity``) and the numpy store model come from tests/test_vector_replay_host.py.
"""
import ctypes as C

import numpy as np
import pytest

from test_vector_replay_host import FRAME_KINDS, SENTINEL, HostStore, Oracle, assert_same_element, make_stream

pytestmark = pytest.mark.gpu

W, R, HEAD = 64, 128, 5120  # include/idqn_hip.h, replay_add_step: write pairs, row cap, byte offset of the frames


class _Block:
    """The step block of ``replay_add_step`` laid out by hand from the header's description: pinned host side + device staging."""

    def __init__(self, frame_bytes):
        import torch

        self.frame_bytes = frame_bytes
        self.pin = torch.zeros(HEAD + 32 * frame_bytes, dtype=torch.uint8).pin_memory()
        self.dev = torch.zeros(HEAD + 32 * frame_bytes, dtype=torch.uint8, device="cuda")
        self.raw = self.pin.numpy()
        self.table = self.raw[:HEAD].view(np.int32)

    def fill(self, frames, writes, row_slots, rows):
        for i, (src, dst) in enumerate(writes):
            self.table[2 * i], self.table[2 * i + 1] = src, dst
        self.table[2 * W : 2 * W + len(row_slots)] = row_slots
        self.table[2 * W + R : 2 * W + R + 8 * len(row_slots)] = np.asarray(rows, np.int32).reshape(-1)
        for i, f in enumerate(frames):
            self.raw[HEAD + i * self.frame_bytes : HEAD + (i + 1) * self.frame_bytes] = f


def _add_step(ring, rows_dev, block, n_in, n_writes, n_rows, n_frames=None, capacity=None, **null):
    import torch

    from slimdqn import _hip

    args = dict(p_ring=_hip.ptr(ring), p_rows=_hip.ptr(rows_dev), p_pin=C.c_void_p(block.pin.data_ptr()), p_dev=_hip.ptr(block.dev))
    args.update(null)
    rc = _hip.lib().replay_add_step(args["p_ring"], ring.shape[0] if n_frames is None else n_frames, ring.shape[1], args["p_rows"],
                                    rows_dev.shape[0] if capacity is None else capacity, args["p_pin"], args["p_dev"], n_in, n_writes,
                                    n_rows, _hip.current_stream())
    torch.cuda.synchronize()  # (the test refills the one pinned block right away)
    return rc


@pytest.mark.parametrize("stack", [1, 4])
@pytest.mark.parametrize("n_envs", [1, 5, 32])
@pytest.mark.parametrize("kind", list(FRAME_KINDS))
def test_replay_add_step_equals_the_numpy_model(kind, n_envs, stack):
    """A scripted sequence of vector steps (main-slot wrap, both mirror ends, FIFO wrap of the rows, growth applied by index):
    ring and rows, copied back, equal the numpy model byte for byte -- so every slot no step wrote still holds its sentinel."""
    import torch

    from slimdqn.sample_collection.vector_replay_buffer import SegmentPlan

    capacity, horizon = 40, 1
    plan = SegmentPlan(n_envs, capacity, stack, horizon, 0.9, segment=6)
    model = HostStore(plan, kind)
    fb = model.frame_bytes
    ring = torch.full((plan.n_frames, fb), SENTINEL, dtype=torch.uint8, device="cuda")
    rows_dev = torch.zeros((capacity, 8), dtype=torch.int32, device="cuda")
    block = _Block(fb)
    n_steps = max(20, 3 * capacity // n_envs)
    for transitions in make_stream(3 + n_envs, n_envs, n_steps, kind):
        step = plan.plan_step(transitions)
        model.apply(step, transitions)
        if step.growth is not None:  # (the buffer's rare path, here by torch indexing: not what this test is about)
            new = torch.full((step.growth.n_frames, fb), SENTINEL, dtype=torch.uint8, device="cuda")
            new[torch.from_numpy(step.growth.dst).cuda()] = ring[torch.from_numpy(step.growth.src).cuda()]
            ring = new
            rows_dev.copy_(torch.from_numpy(plan.rows))
        if not step.frame_envs:
            continue
        frames = [np.ascontiguousarray(transitions[e].observation).view(np.uint8).reshape(-1) for e in step.frame_envs]
        slots = list(dict.fromkeys(k % capacity for k in reversed(step.keys)))[::-1]
        assert len(step.writes) <= W and len(slots) <= R
        block.fill(frames, step.writes, slots, plan.rows[slots] if slots else [])
        assert _add_step(ring, rows_dev, block, len(frames), len(step.writes), len(slots)) == 0
    np.testing.assert_array_equal(ring.cpu().numpy(), model.ring)
    np.testing.assert_array_equal(rows_dev.cpu().numpy(), model.rows)
    assert plan.add_count > capacity and max(plan.frame_count) > 6 and (stack == 1 or model.mirror_writes > 0)


def test_replay_add_step_refuses_bad_arguments():
    """Every documented refusal answers IDQN_E_INVALID and enqueues nothing: ring and rows keep their sentinels."""
    import torch

    from slimdqn import _hip

    fb, n_frames, capacity = 16, 20, 10
    ring = torch.full((n_frames, fb), SENTINEL, dtype=torch.uint8, device="cuda")
    rows_dev = torch.full((capacity, 8), -5, dtype=torch.int32, device="cuda")
    block = _Block(fb)
    frames = [np.full(fb, i, np.uint8) for i in range(3)]

    def attempt(writes, row_slots, n_in=3, n_writes=None, n_rows=None, **kw):
        block.table[:] = 0
        block.fill(frames, writes, row_slots, np.ones((len(row_slots), 8), np.int32))
        return _add_step(ring, rows_dev, block, n_in, len(writes) if n_writes is None else n_writes,
                         len(row_slots) if n_rows is None else n_rows, **kw)

    ok_w, ok_r = [(0, 1), (1, 2), (2, 19)], [0, 9]
    bad = [
        attempt(ok_w, ok_r, p_ring=None), attempt(ok_w, ok_r, p_rows=None), attempt(ok_w, ok_r, p_pin=None), attempt(ok_w, ok_r, p_dev=None),
        attempt(ok_w, ok_r, n_in=33), attempt(ok_w, ok_r, n_in=-1), attempt(ok_w, ok_r, n_writes=65), attempt(ok_w, ok_r, n_writes=-1),
        attempt(ok_w, ok_r, n_rows=129), attempt(ok_w, ok_r, n_rows=-1), attempt([], [], n_in=0),
        attempt([(0, 20)], ok_r), attempt([(0, -1)], ok_r), attempt([(3, 1)], ok_r), attempt([(-1, 1)], ok_r),
        attempt(ok_w, [10]), attempt(ok_w, [-1]), attempt([(0, 4), (1, 4)], ok_r), attempt(ok_w, [3, 3]),
        attempt(ok_w, ok_r, n_frames=19), attempt(ok_w, ok_r, capacity=9), attempt(ok_w, [], n_in=0),
    ]
    assert bad == [_hip.E_INVALID] * len(bad), bad
    assert (ring.cpu().numpy() == SENTINEL).all() and (rows_dev.cpu().numpy() == -5).all()
    assert attempt(ok_w, ok_r) == 0  # ... and the same call with nothing wrong goes through
    got = ring.cpu().numpy()
    assert (got[1] == 0).all() and (got[2] == 1).all() and (got[19] == 2).all() and (np.delete(got, [1, 2, 19], 0) == SENTINEL).all()
    got = rows_dev.cpu().numpy()
    assert (got[[0, 9]] == 1).all() and (got[1:9] == -5).all()
    assert attempt([], [4], n_in=0) == 0 and (rows_dev.cpu().numpy()[4] == 1).all()  # rows alone (the tail of a split step)


def _fill(rb, oracle, stream):
    for transitions in stream:
        rb.add_many(transitions)
        oracle.step(transitions)


@pytest.mark.parametrize("kind", list(FRAME_KINDS))
def test_vector_replay_buffer_equals_the_oracle(kind):
    """E = 5, stack 4, S = 6, 20 steps: ``_memory[key]`` of every live key, a seeded uniform ``sample()`` against the same keys
    gathered from the oracle, and growth on the way (40 elements over 5 segments of 6 frames cannot stay live)."""
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    n_envs, stack, horizon, capacity, B = 5, 4, 1, 40, 16
    rb = VectorReplayBuffer(UniformSamplingDistribution(5), B, capacity, stack_size=stack, update_horizon=horizon, gamma=0.9,
                            n_envs=n_envs, segment=6)
    oracle, twin = Oracle(n_envs, capacity, stack, horizon, 0.9), UniformSamplingDistribution(5)
    _fill(rb, oracle, make_stream(21, n_envs, 20, kind))
    for key in range(oracle.count):  # the sampler calls of ReplayBuffer.add, in key order
        twin.add(key)
        if key + 1 > capacity:
            twin.remove(key - capacity)
    assert rb.add_count == oracle.count > capacity and rb._plan.n_growths > 0
    assert rb._n_frames == rb._plan.n_frames == rb._frames.shape[0]
    assert list(rb._memory.keys()) == list(oracle.memory)
    for key, want in oracle.memory.items():
        assert_same_element(rb._memory[key], want, f"key {key}")
    got, keys = rb.sample(), twin.sample(B)
    state, nxt = np.asarray(got.state), np.asarray(got.next_state)
    assert state.shape == (B,) + FRAME_KINDS[kind][0] + (stack,) and state.dtype == FRAME_KINDS[kind][1]
    for i, key in enumerate(keys):
        want = oracle.memory[int(key)]
        assert state[i].tobytes() == want.state.tobytes() and nxt[i].tobytes() == want.next_state.tobytes(), (i, key)
        assert int(got.action[i]) == want.action and bool(got.is_terminal[i]) == want.is_terminal
        assert np.float32(got.reward[i]) == np.float32(want.reward)
    with pytest.raises(ValueError):
        rb.add_many([None] * 4)
    with pytest.raises(TypeError):
        rb.add(next(tr for tr in make_stream(1, 1, 3, kind, p_none=0.0)[0]))


def test_a_step_with_more_rows_than_the_cap_is_split():
    """32 environments ending an episode of 6 steps together at horizon 5: 160 elements in one step, two calls."""
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    n_envs, stack, horizon, capacity = 32, 4, 5, 150  # (160 keys on 150 slots: ten slots are named twice in that step)
    rb = VectorReplayBuffer(UniformSamplingDistribution(1), 8, capacity, stack_size=stack, update_horizon=horizon, gamma=0.9, n_envs=n_envs)
    oracle = Oracle(n_envs, capacity, stack, horizon, 0.9)
    stream = make_stream(2, n_envs, 13, "u8x16", episode_lengths=(6,), p_none=0.0)
    before = 0
    for transitions in stream:
        rb.add_many(transitions)
        oracle.step(transitions)
        assert rb.add_count - before in (0, 32, 160)
        before = rb.add_count
    assert oracle.count == rb.add_count and rb.add_count > capacity
    for key, want in oracle.memory.items():
        assert_same_element(rb._memory[key], want, f"key {key}")


def _vector_buffer_20x20(seed, B):
    """E = 3 on 20 x 20 uint8 frames, segments of 32 main slots, filled past capacity and around the segments."""
    from slimdqn.sample_collection.replay_buffer import TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    rb = VectorReplayBuffer(UniformSamplingDistribution(seed), B, 60, stack_size=4, update_horizon=1, gamma=0.99, n_envs=3, segment=32)
    rng = np.random.default_rng(seed)
    lengths, n = (13, 9, 17), [0, 0, 0]
    for _ in range(138):  # 4 * 32 + 10: the live elements straddle the wrap of the main slots, some stacks start in the mirror
        row = []
        for e in range(3):
            n[e] += 1
            last = n[e] >= lengths[e]
            n[e] = 0 if last else n[e]
            row.append(TransitionElement(rng.integers(0, 256, (20, 20), dtype=np.uint8), int(rng.integers(5)), float(rng.normal()), last, last))
        rb.add_many(row)
    rb.reuse_sample_buffers = True
    assert rb._plan.n_growths == 0 and rb.add_count > 60 and min(rb._plan.frame_count) == 4 * 32 + 10
    return rb


def _reads_mirror(rb, slots):
    """How many of the sampled elements have a stack that reaches into its segment's mirror slots."""
    p, rows = rb._plan, rb._plan.rows[np.asarray(slots)]
    return sum(any((int(r[i]) - (int(r[i + 1]) - 1)) % p.segment_slots < p.stack - 1 for i in (0, 2)) for r in rows)


STATE = ("_online", "_mu", "_nu", "_count", "_losses", "_cum")


def test_idqn_learn_on_replay_reads_the_vector_ring():
    """``idqn_learn_on_replay`` on ``ring_view()`` of the vector buffer against ``rb._gather(slots)`` + ``idqn_learn_on_batch`` on
    a twin handle: parameters, Adam state and losses bit for bit (the existing contract; the entry and its kernels are unchanged)."""
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    obs, A, feats, K, B = (20, 20, 4), 5, [32, 32, 32, 128], 2, 32
    rb = _vector_buffer_20x20(7, B)
    fused, twin = (iDQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4) for _ in range(2))
    mirrored = 0
    for _ in range(3):
        slots = rb.sample_slots()
        mirrored += _reads_mirror(rb, slots)
        frames, n_frames, frame_bytes, rows, stack, _, _ = rb.ring_view()
        fused._ensure_handle(B)
        _hip.check(_hip.lib().idqn_learn_on_replay(fused._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                   np.ascontiguousarray(slots, np.int32).ctypes.data, B, int(stack), B, 0,
                                                   _hip.current_stream()), "idqn_learn_on_replay")
        twin._learn(rb._gather(slots))
    torch.cuda.synchronize()
    assert mirrored > 0, "no sampled stack uses mirror slots"
    for name in STATE:
        np.testing.assert_array_equal(getattr(fused, name).cpu().numpy(), getattr(twin, name).cpu().numpy(), err_msg=name)
    assert np.isfinite(fused._losses.cpu().numpy()).all() and (fused._count.cpu().numpy() == 3).all()
    # ... and through the agent's own door: update_online_params takes the fused route on this buffer, unchanged
    fused.update_online_params(0, rb)
    assert fused.__dict__.get("_replay_fused_ok") is True


def test_idqn_iqn_learn_on_replay_reads_the_vector_ring():
    import torch

    from slimdqn import _hip
    from slimdqn.networks.iiqn import iIQN

    obs, A, feats, K, B, N = (20, 20, 4), 5, [32, 32, 32, 256], 2, 32, 4
    rb = _vector_buffer_20x20(8, B)
    fused, twin = (iIQN(3, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N) for _ in range(2))
    rng, mirrored = np.random.default_rng(12), 0
    for _ in range(2):
        slots = rb.sample_slots()
        mirrored += _reads_mirror(rb, slots)
        taus = rng.random((K, 3, N, B)).astype(np.float32) * 0.98 + 0.01
        _hip.check(fused._learn_on_replay(rb.ring_view(), slots_host=slots, taus=taus), "idqn_iqn_learn_on_replay")
        twin._learn(rb._gather(slots), taus=taus)
    torch.cuda.synchronize()
    assert mirrored > 0, "no sampled stack uses mirror slots"
    for name in STATE:
        np.testing.assert_array_equal(getattr(fused, name).cpu().numpy(), getattr(twin, name).cpu().numpy(), err_msg=name)
    assert np.isfinite(fused._losses.cpu().numpy()).all() and (fused._count.cpu().numpy() == 2).all()


def test_vector_trainer_short_loop(monkeypatch):
    """``VectorTrainer`` on 4 ``SyntheticAtari`` with ``iDQN``: it runs (gradient steps included), every vector step's actions
    equal ``select_action`` per environment on a twin agent holding the same parameters, and the buffer equals the oracle fed
    with the transitions it was given."""
    import torch

    from experiments.base.dqn import VectorTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticAtari
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection import utils
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    obs, A, feats, K, E, capacity = (84, 84, 4), 6, [32, 64, 64, 512], 2, 4, 64
    agent, twin = (iDQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 2, 16, 8, adam_eps=1.5e-4) for _ in range(2))
    envs = [SyntheticAtari(e, episode_length=(9, 6, 11, 7)[e]) for e in range(E)]
    rb = VectorReplayBuffer(UniformSamplingDistribution(0), 32, capacity, stack_size=4, update_horizon=1, gamma=0.99,
                            clipping=lambda r: float(np.clip(r, -1, 1)), n_envs=E)
    rb.reuse_sample_buffers = True
    oracle, compared = Oracle(E, capacity, 4, 1, 0.99), [0, 0]
    real_select, real_add = utils.select_actions, rb.add_many

    def select_actions(best_actions_fn, params, states, keys, n_actions, epsilon_fn, n):
        actions = real_select(best_actions_fn, params, states, keys, n_actions, epsilon_fn, n)
        for name in ("_online", "_target"):
            getattr(twin, name).copy_(getattr(agent, name))
        want = [int(utils.select_action(twin.best_action, twin.params, s, k, n_actions, epsilon_fn, n).item()) for s, k in zip(states, keys)]
        assert [int(a) for a in actions] == want
        compared[0] += 1
        compared[1] += sum(prng.uniform(prng.split(k, 3)[0]) > epsilon_fn(n) for k in keys)
        return actions

    def add_many(transitions):
        oracle.step([None if tr is None else tr._replace(observation=np.copy(tr.observation)) for tr in transitions])
        real_add(transitions)

    monkeypatch.setattr(utils, "select_actions", select_actions)
    rb.add_many = add_many
    p = dict(epsilon_end=0.05, epsilon_duration=30, n_epochs=1, n_training_steps_per_epoch=120, n_initial_samples=40, horizon=1000,
             wandb=NullLogger())
    trainer = VectorTrainer(prng.PRNGKey(1), p, agent, envs, rb)
    returns, lengths = trainer.run()
    torch.cuda.synchronize()
    assert trainer.total_steps >= 120 and sum(lengths[0]) == trainer.total_steps and compared[0] >= 30 and compared[1] > 20
    assert (agent._count.cpu().numpy() == (trainer.total_steps - 40) // 2).all()  # update_to_data = 2, from step 41 on
    assert agent.__dict__.get("_replay_fused_ok") is True and np.isfinite(agent._losses.cpu().numpy()).all()
    assert any("loss" in r for r in p["wandb"].records)
    assert rb.add_count == oracle.count > capacity
    for key, want in oracle.memory.items():
        assert_same_element(rb._memory[key], want, f"key {key}")
