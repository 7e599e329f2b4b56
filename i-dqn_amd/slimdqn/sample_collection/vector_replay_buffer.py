"""Replay buffer fed by E environments at once: E time lines in one HBM frame ring.

``ReplayBuffer`` puts frame ``t`` of its one environment at ring slot ``t % n_frames`` and every gather rebuilds a stack
from CONSECUTIVE slots, so two environments cannot interleave their frames in it.  Here every environment owns a
contiguous SEGMENT of one allocation ``[E * L][frame_bytes]``, ``L = S + (stack - 1)``:

* frame ``t`` of environment ``e`` (its own count) goes to the main slot ``e * L + (stack - 1) + t % S``;
* when ``t % S >= S - (stack - 1)`` it also goes to the mirror slot ``e * L + t % S - (S - (stack - 1))``: the first
  ``stack - 1`` slots of a segment always hold copies of its last ``stack - 1`` main slots;
* the newest frame of a stack is named by its main slot (``>= e * L + stack - 1``), so its ``stack - 1`` predecessors are
  the slots directly below it, inside the segment, and ``newest - back`` never goes below 0.

The element rows hold these absolute slots and the kernels are told ``n_frames = E * L``: ``replay_gather_stacked`` and
the replay-sourced learner steps (``idqn_learn_on_replay``, ``idqn_iqn_learn_on_replay``, their ``_dev`` forms) read the
vector ring as they are.  Keys stay the global ``add_count`` (FIFO over ``max_capacity``, slot ``key % max_capacity``);
within one vector step environment 0's elements get their keys first, then environment 1's, and so on.

``SegmentPlan`` is the integer logic (host only, numpy only); ``VectorReplayBuffer`` moves the bytes: one pinned block and
one ``replay_add_step`` call per vector step.
"""
import collections
import typing
from typing import Any, List, Optional, Sequence

import numpy as np

from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TrajectoryAccumulator, TransitionElement

MAX_ENVS = 32  # REPLAY_STEP_MAX_IN of csrc/replay.hip: frames per replay_add_step call


def segment_frames(capacity: int, n_envs: int, stack_size: int, update_horizon: int) -> int:
    """Main slots per segment: an environment's share of the elements, the window, and slack for element-less transitions."""
    return -(-capacity // n_envs) + update_horizon + stack_size + max(64, capacity // (4 * n_envs))


class Growth(typing.NamedTuple):
    """The ring doubled its segments: ``new[dst[i]] = old[src[i]]`` moves every frame the old ring held (mirrors included)."""

    segment: int  # the new S
    n_frames: int  # the new E * L
    src: np.ndarray
    dst: np.ndarray


class StepPlan(typing.NamedTuple):
    """What one vector step does to the store, in the order it has to happen: ``growth`` (if any) first, then frame ``i`` of
    ``frame_envs`` (the observation of that environment's transition) to ring slot ``dst`` for every ``(i, dst)`` of
    ``writes``, then the rows of ``keys`` (``SegmentPlan.rows[key % capacity]``; a slot named twice keeps its last key)."""

    growth: Optional[Growth]
    frame_envs: List[int]
    writes: List[typing.Tuple[int, int]]
    keys: List[int]


class SegmentPlan:
    """Per-environment frame counters, write slots (main and mirror), element rows, the liveness guard and growth."""

    def __init__(self, n_envs: int, max_capacity: int, stack_size: int, update_horizon: int, gamma: float,
                 segment: Optional[int] = None):
        if not 1 <= n_envs <= MAX_ENVS:
            raise ValueError(f"n_envs = {n_envs} outside [1, {MAX_ENVS}]")
        self.n_envs, self.capacity, self.stack, self.horizon = n_envs, max_capacity, stack_size, update_horizon
        self.segment = segment_frames(max_capacity, n_envs, stack_size, update_horizon) if segment is None else int(segment)
        # the frames of an element made at frame t lie in the accumulator's window, (t - horizon - stack, t]: they must not
        # have been overwritten by t itself
        if self.segment < update_horizon + stack_size:
            raise ValueError(f"segment = {self.segment} frames cannot hold a window of {update_horizon + stack_size}")
        self.accumulators = [TrajectoryAccumulator(stack_size, update_horizon, gamma) for _ in range(n_envs)]
        self.frame_count = [0] * n_envs
        self.add_count = 0
        self.n_growths = 0
        cap = max_capacity
        self.rows = np.zeros((cap, 8), np.int32)  # replay_gather_stacked documents the row
        self.env_of = np.zeros(cap, np.int32)
        self.newest_s = np.zeros(cap, np.int64)  # frame numbers (the environment's own count) of the two stack ends
        self.newest_n = np.zeros(cap, np.int64)
        self.first_frame = np.zeros(cap, np.int64)  # oldest frame number an element refers to
        self.action = np.zeros(cap, np.int64)
        self.reward64 = np.zeros(cap, np.float64)
        self._live = [collections.deque() for _ in range(n_envs)]  # (key, first frame) of an environment's elements, oldest first

    # ---- layout ------------------------------------------------------------------------------------
    @property
    def segment_slots(self) -> int:
        return self.segment + self.stack - 1

    @property
    def n_frames(self) -> int:
        return self.n_envs * self.segment_slots

    def main_slot(self, env: int, t: int) -> int:
        return env * self.segment_slots + (self.stack - 1) + t % self.segment

    def mirror_slot(self, env: int, t: int) -> Optional[int]:
        r = t % self.segment - (self.segment - (self.stack - 1))
        return env * self.segment_slots + r if r >= 0 else None

    # ---- liveness and growth -------------------------------------------------------------------------
    def oldest_needed(self, env: int) -> Optional[int]:
        """First frame of the oldest live element of ``env`` (its elements' first frames never decrease), or None."""
        live, lo = self._live[env], self.add_count - self.capacity
        while live and live[0][0] < lo:
            live.popleft()
        return live[0][1] if live else None

    def _must_grow(self, env: int) -> bool:
        need = self.oldest_needed(env)  # frame t overwrites both copies of frame t - S
        return need is not None and need <= self.frame_count[env] - self.segment

    def _double(self) -> None:
        """S doubles; the rows hold absolute slots, so they are re-derived for every live element."""
        self.segment, self.n_growths = 2 * self.segment, self.n_growths + 1
        keys = np.arange(max(0, self.add_count - self.capacity), self.add_count, dtype=np.int64)
        if keys.size:
            slots = keys % self.capacity
            base = self.env_of[slots].astype(np.int64) * self.segment_slots + (self.stack - 1)
            self.rows[slots, 0] = base + self.newest_s[slots] % self.segment
            self.rows[slots, 2] = base + self.newest_n[slots] % self.segment
            assert not self._must_grow_any()  # (the old ring held every frame a live element needs: S more slots are enough)

    def _must_grow_any(self) -> bool:
        return any(self._must_grow(e) for e in range(self.n_envs))

    def _growth(self, old_counts, old_segment) -> Growth:
        """Every frame the ring of ``old_segment`` held when its environments had made ``old_counts`` frames, to its main slot
        (and its mirror slot, if it has one) of the present layout."""
        old_slots, src, dst = old_segment + self.stack - 1, [], []
        for e, count in enumerate(old_counts):
            for t in range(max(0, count - old_segment), count):
                slot = e * old_slots + (self.stack - 1) + t % old_segment
                src.append(slot)
                dst.append(self.main_slot(e, t))
                m = self.mirror_slot(e, t)
                if m is not None:
                    src.append(slot)
                    dst.append(m)
        return Growth(self.segment, self.n_frames, np.asarray(src, np.int64), np.asarray(dst, np.int64))

    # ---- one vector step -----------------------------------------------------------------------------
    def plan_step(self, transitions: Sequence[Optional[TransitionElement]]) -> StepPlan:
        """Advances the E time lines by one transition each (``None``: that environment does not step)."""
        if len(transitions) != self.n_envs:
            raise ValueError(f"add_many takes {self.n_envs} entries (a transition or None per environment), got {len(transitions)}")
        old_counts, old_segment = list(self.frame_count), self.segment
        frame_envs, frame_numbers, keys = [], [], []
        for e, transition in enumerate(transitions):
            if transition is None:
                continue
            # the guard, right before the slot is overwritten and on the liveness of this very moment (the elements the
            # environments before this one made in this step have evicted their share).  Slots are laid out once the step is
            # planned, so a step never mixes two segment sizes.
            if self._must_grow(e):
                self._double()
            t = self.frame_count[e]
            self.frame_count[e] = t + 1
            frame_envs.append(e)
            frame_numbers.append(t)
            light = transition._replace(observation=None)  # the window decides positions; pixels never enter it
            for plan, window_size in self.accumulators[e].plan(light):
                key = self.add_count
                self._write(key, e, plan, window_size, t)
                keys.append(key)
                self.add_count = key + 1
        writes = []
        for i, (e, t) in enumerate(zip(frame_envs, frame_numbers)):
            writes.append((i, self.main_slot(e, t)))
            m = self.mirror_slot(e, t)
            if m is not None:
                writes.append((i, m))
        growth = self._growth(old_counts, old_segment) if self.segment != old_segment else None
        return StepPlan(growth, frame_envs, writes, keys)

    def _write(self, key, env, plan, window_size, t_now) -> None:
        slot = key % self.capacity
        to_t = lambda pos: t_now - (window_size - 1 - pos)  # window position -> frame number
        valid_s, valid_n = min(self.stack, plan.last_s + 1), min(self.stack, plan.last_n + 1)
        t_s, t_n = to_t(plan.last_s), to_t(plan.last_n)
        row = self.rows[slot]
        row[0], row[1] = self.main_slot(env, t_s), valid_s
        row[2], row[3] = self.main_slot(env, t_n), valid_n
        row[4] = int(plan.action)
        row[5] = np.float32(plan.reward).view(np.int32)  # f64 -> f32, as ReplayBuffer._write
        row[6] = int(bool(plan.done))
        row[7] = 0
        self.env_of[slot], self.newest_s[slot], self.newest_n[slot] = env, t_s, t_n
        self.first_frame[slot] = t_s - valid_s + 1
        self.action[slot], self.reward64[slot] = plan.action, plan.reward
        self._live[env].append((key, t_s - valid_s + 1))

    def apply_sampler(self, sampler, keys: Sequence[int], **kwargs: Any) -> None:
        """``ReplayBuffer.add``'s sampler calls for the keys of a step, in key order: add, then the FIFO removal."""
        for key in keys:
            sampler.add(key, **kwargs)
            if key + 1 > self.capacity:
                sampler.remove(key - self.capacity)


class VectorReplayBuffer(ReplayBuffer):
    """``ReplayBuffer`` for ``n_envs`` environments stepped together (``add_many``); everything that reads the store --
    ``sample``, ``sample_slots``, ``_gather``, ``_gather_device``, ``ring_view``, ``update``, ``_memory`` -- is inherited."""

    def __init__(self, sampling_distribution, batch_size: int, max_capacity: int, stack_size: int = 4, update_horizon: int = 1,
                 gamma: float = 0.99, checkpoint_duration: int = 4, compress: bool = True, clipping: callable = None,
                 n_envs: int = 1, segment: Optional[int] = None):
        super().__init__(sampling_distribution, batch_size, max_capacity, stack_size, update_horizon, gamma,
                         checkpoint_duration, compress, clipping)
        self._n_envs = n_envs
        self._plan = SegmentPlan(n_envs, max_capacity, stack_size, update_horizon, gamma, segment)
        self._accumulator = None  # (one per environment, in the planner)

    # host mirrors `_memory[key]` reads
    _meta = property(lambda self: self._plan.rows)
    _action = property(lambda self: self._plan.action)
    _reward64 = property(lambda self: self._plan.reward64)
    _first_frame = property(lambda self: self._plan.first_frame)

    def _allocate(self, frame: np.ndarray) -> None:
        import torch

        from slimdqn import _hip

        _hip.lib()  # no extension -> no replay buffer
        self._frame_shape, self._obs_dtype = tuple(frame.shape), frame.dtype
        self._frame_elems, self._itemsize = int(frame.size), int(frame.dtype.itemsize)
        self._frame_bytes = self._frame_elems * self._itemsize
        self._obs_shape = self._frame_shape + (self._stack_size,)
        self._n_frames = self._plan.n_frames
        self._frames = torch.empty((self._n_frames, self._frame_bytes), dtype=torch.uint8, device="cuda")
        self._meta_dev = torch.zeros((self._max_capacity, 8), dtype=torch.int32, device="cuda")
        # the step block (include/idqn_hip.h, replay_add_step), twice in pinned memory and once on the device; one event
        # per pinned half: a half is refilled once the stream has passed the call that read it
        head, size = _hip.REPLAY_STEP_HEADER_BYTES, _hip.REPLAY_STEP_HEADER_BYTES + _hip.REPLAY_STEP_MAX_IN * self._frame_bytes
        self._block_pin = torch.zeros((2, size), dtype=torch.uint8).pin_memory()
        self._block_dev = torch.zeros(size, dtype=torch.uint8, device="cuda")
        W, R = _hip.REPLAY_STEP_MAX_WRITES, _hip.REPLAY_STEP_MAX_ROWS
        self._block = []
        for h in range(2):
            raw = self._block_pin[h].numpy()
            table = raw[:head].view(np.int32)
            self._block.append(dict(ptr=self._block_pin[h].data_ptr(), pairs=table[: 2 * W].reshape(W, 2), row_slots=table[2 * W : 2 * W + R],
                                    rows=table[2 * W + R :].reshape(R, 8), frames=raw[head:].reshape(_hip.REPLAY_STEP_MAX_IN, self._frame_bytes),
                                    event=torch.cuda.Event(), busy=False))
        self._half = 0

    def _flush_meta(self) -> None:
        """The rows travel with their frames (``replay_add_step``): nothing is left to send at sample time."""

    def _apply_growth(self, growth) -> None:
        """Rare (element-less transitions used up a segment's slack): a new ring, the old frames moved by index, every row
        sent again; synchronises."""
        import torch

        new = torch.empty((growth.n_frames, self._frame_bytes), dtype=torch.uint8, device="cuda")
        if growth.src.size:
            new[torch.from_numpy(growth.dst).cuda()] = self._frames[torch.from_numpy(growth.src).cuda()]
        self._meta_dev.copy_(torch.from_numpy(self._plan.rows))
        torch.cuda.synchronize()
        self._frames, self._n_frames = new, growth.n_frames

    def _issue(self, n_in: int, writes, slots, first: bool) -> None:
        """One ``replay_add_step`` call from the current pinned half (frames already staged there when ``first``)."""
        from slimdqn import _hip

        blk = self._block[self._half]
        n_writes = len(writes) if first else 0
        if first:
            blk["pairs"][:n_writes] = writes
        blk["row_slots"][: len(slots)] = slots
        blk["rows"][: len(slots)] = self._plan.rows[slots]
        _hip.check(_hip.lib().replay_add_step(
            _hip.ptr(self._frames), self._n_frames, self._frame_bytes, _hip.ptr(self._meta_dev), self._max_capacity, blk["ptr"],
            _hip.ptr(self._block_dev), n_in if first else 0, n_writes, len(slots), _hip.current_stream()), "replay_add_step")
        blk["event"].record()
        blk["busy"] = True
        self._half ^= 1

    def _claim_half(self):
        blk = self._block[self._half]
        if blk["busy"]:
            blk["event"].synchronize()
            blk["busy"] = False
        return blk

    # ---- reference API -------------------------------------------------------------------------------
    def _plan_many(self, transitions: Sequence[Optional[TransitionElement]]):
        """The host work of a vector step up to the device call: allocation at the first frame, ``plan_step``, ring growth and
        the de-duplicated slot list.  ``(frames, step, slots)``, or None when no environment stepped."""
        if len(transitions) != self._n_envs:
            raise ValueError(f"add_many takes {self._n_envs} entries (a transition or None per environment), got {len(transitions)}")
        frames = [np.ascontiguousarray(tr.observation) for tr in transitions if tr is not None]
        if not frames:
            return None
        if self._frames is None:
            self._allocate(frames[0])
        for f in frames:
            assert f.shape == self._frame_shape and f.dtype == self._obs_dtype, "observation shape / dtype changed"
        step = self._plan.plan_step(transitions)
        if step.growth is not None:
            self._apply_growth(step.growth)
        # a slot named twice within one step (a buffer smaller than a step's elements) keeps its last key's row
        slots = list(dict.fromkeys(int(k % self._max_capacity) for k in reversed(step.keys)))[::-1]
        return frames, step, slots

    def _finish_many(self, step, **kwargs: Any) -> None:
        """The sampler's ``add`` / ``remove`` of the step's keys, then the counter: what ``add_many`` does after its device call."""
        self._plan.apply_sampler(self._sampling_distribution, step.keys, **kwargs)
        self._add_count = self._plan.add_count

    def _add_many_host(self, transitions: Sequence[Optional[TransitionElement]], **kwargs: Any):
        """``add_many`` without its device call (the seam ``ReplayBuffer._add_host`` is for ``add``): returns ``(frames, writes,
        slots)`` -- the new frames in environment order, the (frame index, ring slot) pairs and the de-duplicated element slots,
        whose rows are ``self._plan.rows[slots]`` -- for a caller that sends them itself (``_issue_step``, or
        ``slimdqn.sample_collection.group_replay.GroupVectorCollector``); None when no environment stepped."""
        planned = self._plan_many(transitions)
        if planned is None:
            return None
        frames, step, slots = planned
        self._finish_many(step, **kwargs)
        return frames, step.writes, slots

    def _issue_step(self, frames, writes, slots) -> None:
        """The device half of a vector step: one ``replay_add_step`` call (more only when the step makes more than 128 rows)."""
        from slimdqn import _hip

        blk = self._claim_half()
        for i, f in enumerate(frames):
            blk["frames"][i] = f.view(np.uint8).reshape(-1)
        R = _hip.REPLAY_STEP_MAX_ROWS
        self._issue(len(frames), writes, slots[:R], True)
        for lo in range(R, len(slots), R):
            self._claim_half()
            self._issue(0, (), slots[lo : lo + R], False)

    def add_many(self, transitions: Sequence[Optional[TransitionElement]], **kwargs: Any) -> None:
        """One transition per environment (``None``: that environment does not step): E frames and their elements go to
        the device in one ``replay_add_step`` call (more only when a step makes more than 128 rows); ``kwargs`` go to the
        sampler's ``add`` of every new key, as in ``ReplayBuffer.add``."""
        planned = self._plan_many(transitions)
        if planned is None:
            return
        frames, step, slots = planned
        self._issue_step(frames, step.writes, slots)
        self._finish_many(step, **kwargs)

    def add(self, transition: TransitionElement, **kwargs: Any) -> None:
        if self._n_envs != 1:
            raise TypeError(f"a VectorReplayBuffer of {self._n_envs} environments takes add_many(), one entry per environment")
        if getattr(self, "_deferred", None) is not None:
            self.flush_deferred()
        self.add_many([transition], **kwargs)
