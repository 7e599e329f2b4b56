"""CPU: the replay restatements against traces captured from the reference's own replay buffer (tests/replay_pinned.py).

* ``oracle/replay_ref.py`` with the oracle samplers: ``add_count``, live keys, every live element, the sampler's draws and the
  stacked batches, rewards as float64 bit for bit;
* ``TrajectoryAccumulator.push`` (the product's window logic, materialised) in a FIFO of ``max_capacity``;
* ``SegmentPlan`` for one environment on the numpy store model of tests/test_vector_replay_host.py (rows, ring slots, mirror,
  growth: what ``VectorReplayBuffer`` sends to the device), with the oracle samplers behind ``apply_sampler``;
* ``SegmentPlan`` for three environments fed three captured time lines at once.
"""
import collections

import numpy as np
import pytest

import replay_pinned as rp
from oracle.replay_ref import ReplayRef, Transition
from oracle.samplers_ref import PrioritizedRef, UniformRef
from slimdqn.sample_collection.replay_buffer import TrajectoryAccumulator, TransitionElement
from slimdqn.sample_collection.vector_replay_buffer import SegmentPlan
from test_vector_replay_host import SENTINEL, HostStore


def test_the_capture_holds_what_its_table_says():
    """The file on disk (not the generator's memory of it): streams, checkpoints, draws, and that no frame is a zero frame."""
    streams = rp.load()
    assert tuple(streams) == rp.NAMES
    for s in streams.values():
        assert s.observation.shape == (s.n_transitions,) + s.shape and s.observation.dtype == s.dtype
        assert (s.observation.reshape(s.n_transitions, -1) != 0).all()
        assert s.last.keys and len(s.last.samples) == 2 and s.last.elements[s.last.keys[0]].state.shape == s.shape + (s.stack,)
        assert s.reward.dtype == np.float64 and all(c.elements[k].reward.dtype == np.float64 for c in s.checkpoints.values() for k in c.keys)
    assert {s.stack for s in streams.values()} == {1, 2, 3, 4} and {s.n for s in streams.values()} == {1, 2, 3, 5, 7}
    assert {int(np.prod(s.shape)) * s.dtype.itemsize for s in streams.values()} >= {4, 6, 36, 63, 64, 7056}


@pytest.mark.parametrize("name", rp.NAMES)
def test_replay_ref_equals_the_reference(name):
    s = rp.load()[name]
    rb = ReplayRef(rp.make_sampler(s, UniformRef, PrioritizedRef), batch_size=s.batch, max_capacity=s.cap, stack_size=s.stack,
                   update_horizon=s.n, gamma=s.gamma)
    rp.replay(s, rb, Transition, "f64", lambda rb, keys: [rb.memory[k] for k in keys])


class _AccumulatorFifo:
    """``TrajectoryAccumulator.push`` behind the reference's key / eviction rule (no sampler: nothing is drawn)."""

    def __init__(self, s):
        self.acc, self.cap = TrajectoryAccumulator(s.stack, s.n, s.gamma), s.cap
        self.add_count, self._memory = 0, collections.OrderedDict()

    def add(self, tr, **kwargs):
        for el in self.acc.push(tr):
            self._memory[self.add_count] = el
            self.add_count += 1
            if self.add_count > self.cap:
                self._memory.popitem(last=False)


@pytest.mark.parametrize("name", rp.NAMES)
def test_trajectory_accumulator_equals_the_reference(name):
    s = rp.load()[name]
    rp.replay(s, _AccumulatorFifo(s), TransitionElement, "f64", lambda rb, keys: [rb._memory[k] for k in keys], sample=False)


class _Store(HostStore):
    def __init__(self, plan, shape, dtype):
        self.plan, self.shape, self.dtype = plan, shape, dtype
        self.frame_bytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ring = np.full((plan.n_frames, self.frame_bytes), SENTINEL, np.uint8)
        self.rows = np.zeros((plan.capacity, 8), np.int32)
        self.mirror_writes = 0


class _PlannedBuffer:
    """``SegmentPlan`` + the numpy store, with ``VectorReplayBuffer``'s order of events (plan, store, sampler calls)."""

    def __init__(self, s, n_envs, capacity, sampler=None, segment=None):
        self.plan = SegmentPlan(n_envs, capacity, s.stack, s.n, s.gamma, segment=segment)
        self.store = _Store(self.plan, s.shape, s.dtype)
        self._sampling_distribution, self._batch = sampler, s.batch

    add_count = property(lambda self: self.plan.add_count)
    _memory = property(lambda self: {k: None for k in range(max(0, self.plan.add_count - self.plan.capacity), self.plan.add_count)})

    def add_many(self, transitions, **kwargs):
        step = self.plan.plan_step(transitions)
        self.store.apply(step, transitions)
        if self._sampling_distribution is not None:
            self.plan.apply_sampler(self._sampling_distribution, step.keys, **kwargs)

    def add(self, tr, **kwargs):
        self.add_many([tr], **kwargs)

    def elements(self, keys):
        out = []
        for k in keys:
            el = self.store.element(k)
            r = self.store.rows[k % self.plan.capacity]
            assert r[5] == np.float32(el.reward).view(np.int32)  # the row's reward is the f32 rounding of the double
            out.append(el)
        return out

    def sample(self, size=None):
        els = self.elements(self._sampling_distribution.sample(self._batch if size is None else size))
        return rp.Element(*[np.stack([getattr(e, f) for e in els]) for f in rp.FIELDS])

    def update(self, keys, **kwargs):
        self._sampling_distribution.update(keys, **kwargs)


@pytest.mark.parametrize("name", rp.NAMES)
def test_segment_plan_of_one_environment_equals_the_reference(name):
    s = rp.load()[name]
    rb = _PlannedBuffer(s, 1, s.cap, rp.make_sampler(s, UniformRef, PrioritizedRef))
    rp.replay(s, rb, TransitionElement, "f64", lambda rb, keys: rb.elements(keys))
    if name == "u8x36":
        assert rb.plan.n_growths > 0  # the element-less run outlasted the segment


def test_segment_plan_of_three_environments_equals_three_captures():
    s = rp.load()[rp.VECTOR_LINES[0]]
    rb = _PlannedBuffer(s, 3, rp.VECTOR_CAPACITY, segment=rp.VECTOR_SEGMENT)
    covered = rp.replay_three_lines(TransitionElement, rb.add_many, lambda: rb.plan, rb.elements, "f64")
    rp.assert_three_lines_covered(covered, rb.plan)
