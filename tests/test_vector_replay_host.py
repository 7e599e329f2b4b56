"""CPU: the integer logic of vector-environment collection (slimdqn/sample_collection/vector_replay_buffer.py, SegmentPlan) and
the VectorTrainer's event order.

The planner is driven against a numpy array that stands in for the HBM ring and the element rows (``HostStore``); stacks are
read back with the gather kernels' own formula, ``(newest - back + n_frames) % n_frames``.  The oracle is one host
``TrajectoryAccumulator.push`` per environment (the reference's materialised elements), interleaved in key order -- environment
0's elements of a step first, then environment 1's, ... -- and kept in a FIFO of ``max_capacity``.
tests/test_gpu_vector_replay.py imports the stream generator, the oracle and the store model from here.
"""
import collections
import itertools

import numpy as np
import pytest

from slimdqn import prng
from slimdqn.sample_collection.replay_buffer import ReplayBuffer, ReplayElement, TrajectoryAccumulator, TransitionElement
from slimdqn.sample_collection.vector_replay_buffer import SegmentPlan, segment_frames

FRAME_KINDS = {"u8x16": ((4, 4), np.uint8), "u8x15": ((3, 5), np.uint8), "f32x32": ((8,), np.float32)}  # 16, 15, 32 bytes
SENTINEL = 0xAB
EPISODE_LENGTHS = (5, 7, 3, 4, 11, 2)  # (the first ones coprime to the segment sizes: stacks land on every slot phase)


def make_stream(seed, n_envs, n_steps, kind, episode_lengths=EPISODE_LENGTHS, p_none=0.15, n_actions=5):
    """``n_steps`` vector steps: per environment a fresh frame, episodes of that environment's own length ending in turn with a
    terminal and a truncation, and now and then ``None`` (the environment does not step)."""
    shape, dtype = FRAME_KINDS[kind]
    rng = np.random.default_rng(seed)
    in_episode, n_episodes, steps = [0] * n_envs, [0] * n_envs, []
    for _ in range(n_steps):
        row = []
        for e in range(n_envs):
            if rng.random() < p_none:
                row.append(None)
                continue
            frame = (rng.integers(0, 256, shape).astype(dtype) if dtype == np.uint8 else rng.standard_normal(shape).astype(dtype))
            in_episode[e] += 1
            last = in_episode[e] >= episode_lengths[e % len(episode_lengths)]
            terminal = last and n_episodes[e] % 2 == 0
            if last:
                in_episode[e], n_episodes[e] = 0, n_episodes[e] + 1
            row.append(TransitionElement(frame, int(rng.integers(n_actions)), float(rng.normal()), terminal, last))
        steps.append(row)
    return steps


class Oracle:
    """The reference's elements: one accumulator per environment, keys in the stated order, FIFO of ``capacity``."""

    def __init__(self, n_envs, capacity, stack, horizon, gamma):
        self.accs = [TrajectoryAccumulator(stack, horizon, gamma) for _ in range(n_envs)]
        self.capacity, self.count, self.memory = capacity, 0, collections.OrderedDict()

    def step(self, transitions):
        for e, tr in enumerate(transitions):
            if tr is None:
                continue
            for element in self.accs[e].push(tr):
                self.memory[self.count] = element
                self.count += 1
                if self.count > self.capacity:
                    self.memory.popitem(last=False)


class HostStore:
    """numpy stand-in for the device store: applies a ``StepPlan`` the way ``VectorReplayBuffer.add_many`` does."""

    def __init__(self, plan, kind):
        self.plan, (self.shape, self.dtype) = plan, FRAME_KINDS[kind]
        self.frame_bytes = int(np.prod(self.shape)) * np.dtype(self.dtype).itemsize
        self.ring = np.full((plan.n_frames, self.frame_bytes), SENTINEL, np.uint8)
        self.rows = np.zeros((plan.capacity, 8), np.int32)
        self.mirror_writes = 0

    def apply(self, step, transitions):
        if step.growth is not None:
            new = np.full((step.growth.n_frames, self.frame_bytes), SENTINEL, np.uint8)
            new[step.growth.dst] = self.ring[step.growth.src]
            self.ring, self.rows[:] = new, self.plan.rows
        frames = [np.ascontiguousarray(transitions[e].observation).view(np.uint8).reshape(-1) for e in step.frame_envs]
        assert len({dst for _, dst in step.writes}) == len(step.writes), "a ring slot is written twice in one step"
        for src, dst in step.writes:
            assert 0 <= dst < self.plan.n_frames
            self.ring[dst] = frames[src]
        self.mirror_writes += len(step.writes) - len(frames)
        for key in step.keys:
            self.rows[key % self.plan.capacity] = self.plan.rows[key % self.plan.capacity]

    def stack_of(self, newest, valid):
        n_frames, stack = self.ring.shape[0], self.plan.stack
        out = np.zeros(self.shape + (stack,), self.dtype)
        for ch in range(stack):
            back = stack - 1 - ch
            if back < valid:
                out[..., ch] = self.ring[(newest - back + n_frames) % n_frames].view(self.dtype).reshape(self.shape)
        return out

    def element(self, key):
        r = self.rows[key % self.plan.capacity]
        done = bool(r[6])
        return ReplayElement(self.stack_of(int(r[0]), int(r[1])), int(r[4]), float(self.plan.reward64[key % self.plan.capacity]),
                             self.stack_of(int(r[2]), int(r[3])), done, done)

    def uses_mirror(self, key):
        """Does a stack of ``key`` read a mirror slot (a slot below its segment's first main slot)?"""
        r, p = self.rows[key % self.plan.capacity], self.plan
        return any((int(r[i]) - (int(r[i + 1]) - 1)) % p.segment_slots < p.stack - 1 for i in (0, 2))


def assert_same_element(got, want, what=""):
    assert got.state.dtype == want.state.dtype and got.state.tobytes() == want.state.tobytes(), f"{what}: state"
    assert got.next_state.tobytes() == want.next_state.tobytes(), f"{what}: next_state"
    assert (int(got.action), bool(got.is_terminal), bool(got.episode_end)) == (int(want.action), bool(want.is_terminal), bool(want.episode_end)), what
    assert float(got.reward) == float(want.reward), f"{what}: reward"


def assert_store_equals_oracle(store, oracle):
    plan = store.plan
    assert plan.add_count == oracle.count
    assert list(oracle.memory) == list(range(max(0, plan.add_count - plan.capacity), plan.add_count))
    for key, want in oracle.memory.items():
        assert_same_element(store.element(key), want, f"key {key}")
        r = store.rows[key % plan.capacity]
        assert np.float32(want.reward).view(np.int32) == r[5]  # the f32 the device hands out
        lo = int(plan.env_of[key % plan.capacity]) * plan.segment_slots
        for newest, valid in ((int(r[0]), int(r[1])), (int(r[2]), int(r[3]))):
            assert lo + plan.stack - 1 <= newest < lo + plan.segment_slots and newest - (valid - 1) >= lo  # inside its segment


SIZES = list(itertools.product((1, 2, 5, 32), (1, 4), (1, 3), (7, 40), tuple(FRAME_KINDS)))


@pytest.mark.parametrize("n_envs,stack,horizon,capacity,kind", SIZES)
def test_every_live_element_equals_the_oracle(n_envs, stack, horizon, capacity, kind):
    segment = max(6, horizon + stack)
    plan = SegmentPlan(n_envs, capacity, stack, horizon, 0.9, segment=segment)
    store, oracle = HostStore(plan, kind), Oracle(n_envs, capacity, stack, horizon, 0.9)
    mirrored = False
    n_steps = max(45, 6 * capacity // n_envs)  # (enough for the FIFO to evict and the grown segments to wrap, whatever E is)
    for transitions in make_stream(11 * n_envs + stack + horizon, n_envs, n_steps, kind):
        step = plan.plan_step(transitions)
        store.apply(step, transitions)
        oracle.step(transitions)
        assert_store_equals_oracle(store, oracle)
        mirrored |= any(store.uses_mirror(k) for k in oracle.memory)
    assert oracle.count > capacity  # FIFO eviction happened
    assert max(plan.frame_count) > plan.segment  # the main slots wrapped (after any growth)
    if stack > 1:
        assert store.mirror_writes > 0 and mirrored  # frames went to both ends, and a live stack read its mirror slots
        used = {dst % plan.segment_slots for dst in range(plan.n_frames) if (store.ring[dst] != SENTINEL).any()}
        assert {0, stack - 2} <= used  # both ends of the mirror
    else:
        assert store.mirror_writes == 0 and plan.segment_slots == plan.segment
    if capacity == 7 and n_envs == 32 and horizon == 1:  # (32 environments evict 7 elements within a step; at horizon 3 the
        assert plan.n_growths == 0 and plan.segment == segment  # forced segment is exactly the window and may still grow once)
    if capacity == 40 and n_envs == 1:
        assert plan.n_growths > 0  # 40 live elements of one environment do not fit 6 frames


def test_segment_size_and_limits():
    assert segment_frames(1000, 8, 4, 3) == 125 + 3 + 4 + 64
    assert segment_frames(10**6, 4, 4, 1) == 250000 + 1 + 4 + 62500
    plan = SegmentPlan(5, 40, 4, 1, 0.99)
    assert plan.segment == 8 + 1 + 4 + 64 and plan.segment_slots == plan.segment + 3 and plan.n_frames == 5 * plan.segment_slots
    assert SegmentPlan(3, 40, 1, 1, 0.99).segment_slots == SegmentPlan(3, 40, 1, 1, 0.99).segment  # stack 1: no mirror
    for bad in (0, 33):
        with pytest.raises(ValueError):
            SegmentPlan(bad, 40, 4, 1, 0.99)
    with pytest.raises(ValueError):
        SegmentPlan(2, 40, 4, 3, 0.99, segment=6)  # a window of 7 frames does not fit
    with pytest.raises(ValueError):
        plan.plan_step([None] * 4)


def test_liveness_guard_grows_the_ring():
    """Short truncated episodes (fewer than ``update_horizon`` steps: no elements) in all but one environment: the one that does
    emit keeps far more live elements than its share, at the default segment size; its oldest frames must survive."""
    n_envs, stack, horizon, capacity, kind = 4, 4, 3, 400, "u8x15"
    plan = SegmentPlan(n_envs, capacity, stack, horizon, 0.99)
    s0 = plan.segment
    assert s0 == 100 + 3 + 4 + 64
    store, oracle = HostStore(plan, kind), Oracle(n_envs, capacity, stack, horizon, 0.99)
    stream = make_stream(5, n_envs, s0 + 60, kind, episode_lengths=(50, 2, 3, 2), p_none=0.0)
    for i, transitions in enumerate(stream):
        transitions = [tr if e == 0 or not tr.is_terminal else tr._replace(is_terminal=False) for e, tr in enumerate(transitions)]
        step = plan.plan_step(transitions)
        store.apply(step, transitions)
        oracle.step(transitions)
        if step.growth is not None or i % 25 == 0 or i == len(stream) - 1:
            assert_store_equals_oracle(store, oracle)
    assert plan.n_growths == 1 and plan.segment == 2 * s0 and store.ring.shape[0] == plan.n_frames
    assert (plan.env_of[: oracle.count] == 0).all() and oracle.count > s0  # only environment 0 made elements, more than S of them


class _LogSampler:
    def __init__(self):
        self.calls = []

    def add(self, key, **kwargs):
        self.calls.append(("add", int(key), kwargs))

    def remove(self, key):
        self.calls.append(("remove", int(key)))


class _HostReplayBuffer(ReplayBuffer):
    """``ReplayBuffer``'s host logic (window, keys, rows, sampler calls) without its device half."""

    def _upload_frame(self, observation):
        if self._frames is None:
            cap = self._max_capacity
            self._frames = True
            self._n_frames = cap + self._update_horizon + self._stack_size + max(64, cap // 16)
            self._meta, self._first_frame = np.zeros((cap, 8), np.int32), np.zeros(cap, np.int64)
            self._action, self._reward64 = np.zeros(cap, np.int64), np.zeros(cap, np.float64)
            self._meta_ev = None
        self._t += 1
        return self._t - 1


@pytest.mark.parametrize("stack,horizon", [(4, 1), (4, 3), (1, 3)])
def test_one_environment_is_replay_buffer(stack, horizon):
    capacity = 40
    rb = _HostReplayBuffer(_LogSampler(), 8, capacity, stack_size=stack, update_horizon=horizon, gamma=0.9)
    plan, sampler = SegmentPlan(1, capacity, stack, horizon, 0.9), _LogSampler()
    for (tr,) in make_stream(3, 1, 130, "u8x16", p_none=0.0):
        rb.add(tr, priority=1.5)
        step = plan.plan_step([tr])
        plan.apply_sampler(sampler, step.keys, priority=1.5)
        assert plan.add_count == rb.add_count
    assert plan.n_growths == 0 and rb._n_frames < 130 and rb.add_count > capacity
    assert sampler.calls == rb._sampling_distribution.calls
    np.testing.assert_array_equal(plan.rows[:, [1, 3, 4, 5, 6, 7]], rb._meta[:, [1, 3, 4, 5, 6, 7]])
    np.testing.assert_array_equal(plan.newest_s % rb._n_frames, rb._meta[:, 0])  # the same frames, numbered per layout
    np.testing.assert_array_equal(plan.newest_n % rb._n_frames, rb._meta[:, 2])
    np.testing.assert_array_equal(plan.rows[:, 0], plan.stack - 1 + plan.newest_s % plan.segment)
    np.testing.assert_array_equal(plan.first_frame, rb._first_frame)
    np.testing.assert_array_equal(plan.reward64, rb._reward64)


# ---- select_actions + the VectorTrainer's event order, with fake device objects (the style of test_trainer_host.py) ------------
class _FakeVectorRB:
    _clipping = staticmethod(lambda r: max(-1.0, min(1.0, r)))

    def __init__(self):
        self.steps = []

    def add_many(self, transitions):
        self.steps.append(list(transitions))

    def add(self, transition):
        self.steps.append([transition])


class _FakeAgent:
    params = None

    def __init__(self, vectorised=True):
        self.calls, self.vector_calls = [], 0
        if vectorised:
            self.best_actions = self._best_actions

    def best_action(self, params, state, key):
        from slimdqn.sample_collection.utils import HostAction

        return HostAction(prng.randint(key, 0, 4))

    def _best_actions(self, params, states, keys):
        self.vector_calls += 1
        return np.asarray([prng.randint(k, 0, 4) for k in keys], np.int64)

    def update_online_params(self, step, rb):
        self.calls.append(("online", step))

    def update_target_params(self, step):
        self.calls.append(("target", step))
        return (step % 10 == 0), ({"loss": 1.0} if step % 10 == 0 else {})

    def get_model(self):
        return {"params": {}}


def _params(**kw):
    from experiments.base.utils import NullLogger

    return dict(dict(epsilon_end=0.01, epsilon_duration=10, n_epochs=2, n_training_steps_per_epoch=60, n_initial_samples=7,
                     horizon=1000, wandb=NullLogger()), **kw)


def _envs(n, lengths=(7, 5, 11, 4)):
    from slimdqn.environments.synthetic import SyntheticVector

    return [SyntheticVector(e, episode_length=lengths[e % len(lengths)]) for e in range(n)]


def test_vector_trainer_event_order():
    from experiments.base.dqn import VectorTrainer

    p, agent, rb, envs = _params(), _FakeAgent(), _FakeVectorRB(), _envs(4)
    trainer = VectorTrainer(prng.PRNGKey(0), p, agent, envs, rb)
    boundaries = []
    epoch = trainer.run_epoch
    trainer.run_epoch = lambda index: (epoch(index), boundaries.append(([e.n_steps for e in envs], trainer.total_steps)))
    returns, lengths = trainer.run()
    total = trainer.total_steps
    n_transitions = sum(tr is not None for step in rb.steps for tr in step)
    assert total == n_transitions == sum(sum(l) for l in lengths)  # total_steps advances once per environment step
    assert all(len(step) == 4 for step in rb.steps) and agent.vector_calls <= len(rb.steps)
    # gradient and target updates at exactly the total_steps values a loop of single steps gives: every value past
    # n_initial_samples once, online then target
    assert agent.calls == [(kind, s) for s in range(8, total + 1) for kind in ("online", "target")]
    # an epoch ends with every environment on an episode boundary, at or past its budget; the ones that got there first waited
    assert len(boundaries) == 2 and all(steps == [0, 0, 0, 0] for steps, _ in boundaries)
    assert boundaries[0][1] >= 60 and boundaries[1][1] - boundaries[0][1] >= 60
    assert any(tr is None for tr in rb.steps[-1]) and all(tr is not None for tr in rb.steps[0])
    for step in rb.steps:
        for tr in step:
            assert tr is None or -1.0 <= tr.reward <= 1.0  # reward clipping applied to what is stored
    assert all(tr.episode_end for tr in rb.steps[-1] if tr is not None)
    assert sum("epoch" in r for r in p["wandb"].records) == 2 and any("loss" in r for r in p["wandb"].records)
    assert len(returns) == 2 and all(len(r) == len(l) for r, l in zip(returns, lengths))


def test_one_environment_vector_trainer_is_trainer():
    """E = 1: the same key splits, actions, transitions and agent calls as ``Trainer`` on the same environment."""
    from experiments.base.dqn import train, train_vector

    out = []
    for vector in (False, True):
        agent, rb, env = _FakeAgent(), _FakeVectorRB(), _envs(1)[0]
        p = _params(epsilon_duration=40)
        if vector:
            train_vector(prng.PRNGKey(4), p, agent, [env], rb)
        else:
            train(prng.PRNGKey(4), p, agent, env, rb)
        out.append((agent.calls, [step[0] for step in rb.steps], [r for r in p["wandb"].records]))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    assert len(out[0][1]) == len(out[1][1]) > 120
    for a, b in zip(out[0][1], out[1][1]):
        np.testing.assert_array_equal(a.observation, b.observation)
        assert a[1:] == b[1:]
    assert len({tr.action for tr in out[1][1]}) > 1


def test_collect_vector_samples_equals_single_collection_and_falls_back():
    """Environment i sees what ``collect_single_sample`` with its key shows it; an agent without ``best_actions`` (no vectorised
    acting path) acts through a loop of ``best_action``: the same actions."""
    from slimdqn.sample_collection.utils import collect_single_sample, collect_vector_samples, linear_schedule

    eps, p = linear_schedule(1.0, 0.01, 10), _params()
    keys = list(prng.split(prng.PRNGKey(9), 5))
    results = []
    for mode in ("vector", "fallback", "single"):
        agent, rb, envs = _FakeAgent(vectorised=(mode == "vector")), _FakeVectorRB(), _envs(5)
        for env in envs:
            env.reset()
        for step in range(12):  # (epsilon falls from 1 to 0.01: both branches of the draw)
            if mode == "single":
                for k, env in zip(keys, envs):
                    collect_single_sample(k, env, agent, rb, p, eps, step)
            else:
                rewards, ended = collect_vector_samples(keys, envs, agent, rb, p, eps, step)
                assert len(rewards) == len(ended) == 5
        flat = [tr for s in rb.steps for tr in s]
        results.append([(tr.observation.tobytes(),) + tuple(tr[1:]) for tr in flat])
        assert mode != "vector" or 0 < agent.vector_calls <= 12
        assert mode != "fallback" or not hasattr(agent, "best_actions")
    assert results[0] == results[1] == results[2]
    # an inactive environment neither acts nor steps and reaches the buffer as None
    agent, rb, envs = _FakeAgent(), _FakeVectorRB(), _envs(3)
    for env in envs:
        env.reset()
    rewards, ended = collect_vector_samples(keys[:2], envs, agent, rb, p, eps, 100, active=[True, False, True])
    assert rewards[1] is None and ended[1] is False and rb.steps[0][1] is None and envs[1].n_steps == 0
    assert rb.steps[0][0] is not None and rb.steps[0][2] is not None
