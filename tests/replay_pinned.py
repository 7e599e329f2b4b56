"""Shared by tests/test_replay_pinned_host.py and tests/test_gpu_replay_pinned.py: the traces captured from the reference's OWN
replay buffer (``oracle/make_golden.py --replay`` -> tests/golden/int_path_replay.npz) and the code that replays them.

What the file holds, per stream (``meta_json`` lists the streams; every array's name starts with the stream's name):

* the stream: ``_observation`` [T, frame], ``_action``, ``_reward`` (f64), ``_is_terminal``, ``_episode_end``, ``_priority`` (what
  ``add(priority=...)`` was given when the stream's sampler is the prioritized one);
* at checkpoints (``meta["checkpoints"]``: after transition ``t``; ``add_count``; ``n_live``): the live keys in the order of the
  reference's ``_memory`` and every field of every live element, concatenated over the checkpoints in ``_live_*``;
* at every checkpoint with live keys two ``sample()`` calls (batch size, then 3): the sampler's keys and the stacked batch the
  reference returned, concatenated in ``_drawn_*``; behind them, for a prioritized stream, one ``update(keys, priorities)``
  (``_update_*``).

The streams' corners (asserted by the generator where it records them):

| property | values |
|---|---|
| stack / update horizon | 1, 2, 3, 4 / 1, 2, 3, 5, 7, with n > stack (u8x63, i64x3) and n >= the longest episode (u8x64) |
| frames | uint8, float32, int64; 4, 6, 36, 63, 64 bytes, 20 x 20 and 84 x 84 uint8 |
| endings | a terminal and a truncation at every trajectory length 1 .. n + 1, both flags at once, terminals back to back |
| capacity | 1, 2, and 5 < n + stack = 11: elements made and evicted inside one terminal flush |
| ring | u8x4 wraps the frame ring 3.5 times; u8x36 holds a run of element-less truncated episodes longer than the ring |
| gamma, rewards | 0.97 and 1.0; normal deviates, whose n-step sums are no f32 |
| draws | a state stack and a next_state stack that cross an episode start; a batch with a repeated key |
"""
import collections
import json
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("state", "action", "reward", "next_state", "is_terminal", "episode_end")
Element = collections.namedtuple("Element", FIELDS)
_cache = {}


def load():
    """``{name: stream}``; a stream is a namespace of its meta entries and arrays, its checkpoints split up."""
    if "streams" in _cache:
        return _cache["streams"]
    z = np.load(os.path.join(GOLDEN, "int_path_replay.npz"))
    streams = {}
    for m in json.loads(bytes(z["meta_json"]).decode()):
        name = m["name"]
        get = lambda what: z[f"{name}_{what}"]
        s = types.SimpleNamespace(**m)
        s.shape, s.dtype = tuple(m["shape"]), np.dtype(m["dtype"])
        for what in ("observation", "action", "reward", "is_terminal", "episode_end", "priority"):
            setattr(s, what, get(what))
        live = {f: get("live_" + f) for f in ("keys",) + FIELDS}
        drawn = {f: get("drawn_" + f) for f in ("keys",) + FIELDS}
        update = {f: get("update_" + f) for f in ("keys", "priorities")} if m["sampler"] == "prioritized" else None
        lo = dlo = ulo = 0
        s.checkpoints = {}
        for cp in m["checkpoints"]:
            c = types.SimpleNamespace(t=cp["t"], add_count=cp["add_count"], samples=[], update=None)
            hi = lo + cp["n_live"]
            c.keys = [int(k) for k in live["keys"][lo:hi]]
            c.elements = {k: Element(*[live[f][lo + i] for f in FIELDS]) for i, k in enumerate(c.keys)}
            lo = hi
            for size in cp["samples"]:
                c.samples.append((drawn["keys"][dlo : dlo + size], Element(*[drawn[f][dlo : dlo + size] for f in FIELDS])))
                dlo += size
            if cp.get("n_update"):
                c.update = (update["keys"][ulo : ulo + cp["n_update"]], update["priorities"][ulo : ulo + cp["n_update"]])
                ulo += cp["n_update"]
            s.checkpoints[c.t] = c
        assert lo == len(live["keys"]) and dlo == len(drawn["keys"])
        s.last = s.checkpoints[s.n_transitions - 1]
        streams[name] = s
    _cache["streams"] = streams
    return streams


NAMES = ("u8x4", "u8x6", "u8x36", "u8x63", "u8x64", "u8x84x84", "i64x3", "f32s1", "f32s2", "u8x20x20", "vec0", "vec1", "vec2")


def transition(stream, t, Transition):
    return Transition(stream.observation[t], int(stream.action[t]), float(stream.reward[t]), bool(stream.is_terminal[t]),
                      bool(stream.episode_end[t]))


def add_kwargs(stream, t):
    return {"priority": float(stream.priority[t])} if stream.sampler == "prioritized" else {}


def make_sampler(stream, Uniform, Prioritized):
    if stream.sampler == "uniform":
        return Uniform(stream.sampler_seed)
    return Prioritized(stream.sampler_seed, stream.tree_capacity, stream.alpha)


def same_reward(got, want, reward):
    """``reward``: "f64" -- the captured double, bit for bit; "f32" -- its rounding to float32 (what the device holds)."""
    if reward == "f64":
        return np.float64(got).tobytes() == np.float64(want).tobytes()
    return np.asarray(got).dtype == np.float32 and np.float32(got).tobytes() == np.float32(want).tobytes()


def assert_element(got, want, reward, what):
    """One element (or one row of a batch) against the captured one: stacks in bytes, dtype and shape; scalars by value."""
    for f in ("state", "next_state"):
        g, w = np.asarray(getattr(got, f)), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {f}"
    assert int(got.action) == int(want.action), f"{what}: action {got.action} != {want.action}"
    assert bool(got.is_terminal) == bool(want.is_terminal), f"{what}: is_terminal"
    assert bool(got.episode_end) == bool(want.episode_end), f"{what}: episode_end"
    assert same_reward(got.reward, want.reward, reward), f"{what}: reward {got.reward!r} != {want.reward!r}"


def assert_batch(got, want, reward, what):
    n = len(want.action)
    for f in FIELDS:
        assert len(np.asarray(getattr(got, f))) == n, f"{what}: {f} has {len(np.asarray(getattr(got, f)))} rows, not {n}"
    cols = [np.asarray(getattr(got, f)) for f in FIELDS]
    for i in range(n):
        assert_element(Element(*[c[i] for c in cols]), Element(*[getattr(want, f)[i] for f in FIELDS]), reward, f"{what}, row {i}")


def replay(stream, rb, Transition, reward, live_elements, sample=True, on_checkpoint=None):
    """Feeds the stream to ``rb`` (anything with the reference's ``add`` / ``sample`` / ``update`` / ``add_count`` / ``_memory``).
    At every checkpoint: ``add_count``, the live keys in order, every live element (``live_elements(rb, keys)`` -> elements in that
    order), then the captured draws -- the sampler must draw the captured keys, and ``sample()`` must return the captured batch."""
    sampler = getattr(rb, "_sampling_distribution", None)
    forced = []
    if sample:
        real = sampler.sample

        def forced_sample(size):
            drawn, keys = real(size), forced.pop(0)  # (the real draw keeps the generator where the reference's is)
            assert len(keys) == size and np.asarray(drawn).tolist() == keys.tolist(), "the sampler draws other keys than the reference's"
            return keys

        sampler.sample = forced_sample
    for t in range(stream.n_transitions):
        rb.add(transition(stream, t, Transition), **add_kwargs(stream, t))
        cp = stream.checkpoints.get(t)
        if cp is None:
            continue
        what = f"{stream.name} after transition {t}"
        assert rb.add_count == cp.add_count, f"{what}: add_count {rb.add_count} != {cp.add_count}"
        assert [int(k) for k in rb._memory.keys()] == cp.keys, f"{what}: live keys"
        if cp.keys:
            got = live_elements(rb, cp.keys)
            assert len(got) == len(cp.keys)
            for key, el in zip(cp.keys, got):
                assert_element(el, cp.elements[key], reward, f"{what}, key {key}")
        if on_checkpoint is not None:
            on_checkpoint(rb, cp)
        if not sample:
            continue
        for j, (keys, batch) in enumerate(cp.samples):
            forced.append(keys)
            got = rb.sample() if j == 0 else rb.sample(len(keys))
            assert not forced
            assert_batch(got, batch, reward, f"{what}, draw {j}")
        if cp.update is not None:
            rb.update(cp.update[0], priorities=cp.update[1])


# ---- three captured time lines in one vector ring -------------------------------------------------------------------------------
VECTOR_LINES, VECTOR_CAPACITY, VECTOR_SEGMENT = ("vec0", "vec1", "vec2"), 40, 24


def reads_mirror(plan, key):
    """Does a stack of ``key`` reach below its segment's first main slot (into the mirror slots)?"""
    r = plan.rows[key % plan.capacity]
    return any((int(r[i]) - (int(r[i + 1]) - 1)) % plan.segment_slots < plan.stack - 1 for i in (0, 2))


def replay_three_lines(Transition, add_many, plan_of, live_elements, reward):
    """E = 3: vector step ``t`` holds transition ``t`` of each of the three streams.  The j-th element a segment makes is key j of
    its stream's capture, whatever global key the interleaving gives it; the capture holds every key of those streams (their
    capacity is larger than what they make), so every element that is live in the vector ring is compared, for the whole run:
    past the first eviction, around the main slots and through the mirror slots.  Returns what was covered."""
    streams = [load()[name] for name in VECTOR_LINES]
    T = streams[0].n_transitions
    assert all(s.n_transitions == T and s.last.add_count <= s.cap for s in streams)  # nothing evicted in the captures
    assert len({(s.shape, s.dtype, s.stack, s.n, s.gamma) for s in streams}) == 1
    made, origin, before = [0, 0, 0], {}, 0
    covered = dict(compared=0, mirror=0, after_wrap=0, evicted=0, per_line=[set(), set(), set()])
    for t in range(T):
        add_many([transition(s, t, Transition) for s in streams])
        plan = plan_of()
        assert plan.add_count - before <= plan.capacity  # (every key of the step still has its row)
        for key in range(before, plan.add_count):
            e = int(plan.env_of[key % plan.capacity])
            origin[key] = (e, made[e])
            made[e] += 1
        before = plan.add_count
        if t % 8 != 7 and t != T - 1:
            continue
        keys = list(range(max(0, plan.add_count - plan.capacity), plan.add_count))
        for key, el in zip(keys, live_elements(keys)):
            e, j = origin[key]
            assert j in streams[e].last.elements, f"key {key} = element {j} of {streams[e].name} is not in the capture"
            assert_element(el, streams[e].last.elements[j], reward, f"step {t}, key {key} (element {j} of {streams[e].name})")
            covered["compared"] += 1
            covered["per_line"][e].add(j)
            covered["mirror"] += reads_mirror(plan, key)
            covered["after_wrap"] += plan.frame_count[e] > plan.segment + plan.stack
        covered["evicted"] = max(0, plan.add_count - plan.capacity)
    assert made == [s.last.add_count for s in streams]  # each segment made exactly its stream's elements, in its order
    return covered


def assert_three_lines_covered(covered, plan):
    """The comparable range is not empty, reaches past the first eviction and covers a wrap of the main slots whose live stacks
    read the mirror slots."""
    assert covered["compared"] > 3 * VECTOR_CAPACITY and all(len(c) > VECTOR_CAPACITY // 3 for c in covered["per_line"])
    assert covered["evicted"] > 0 and covered["after_wrap"] > 0 and covered["mirror"] > 0
    assert min(plan.frame_count) > 2 * plan.segment  # every segment went around at least twice
