"""What the group-collection tests share (tests/test_group_collect_host.py on numpy stubs, tests/test_gpu_group_collect.py on
the device): scripted transition streams and the twin comparison -- one set of buffers driven by ``rb.add``, an identical set
by ``GroupCollector.add_many``, compared field by field and byte by byte, without a tolerance."""
import numpy as np

from slimdqn.sample_collection.replay_buffer import TransitionElement


def make_script(seed, shape, dtype, steps, terminal_every=0, truncate_every=0, truncate_from=None):
    """``steps`` transitions of frames ``shape`` / ``dtype``: a terminal every ``terminal_every`` steps, a truncated
    (non-terminal) episode end every ``truncate_every`` steps, and from step ``truncate_from`` on a truncated end at EVERY step
    (one-transition episodes make no element: the ring's slack runs out and ``_grow_ring`` has to run)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(steps):
        if np.dtype(dtype) == np.uint8:
            obs = rng.integers(0, 256, shape, dtype=np.uint8)
        else:
            obs = rng.standard_normal(shape).astype(dtype)
        terminal = bool(terminal_every and t % terminal_every == terminal_every - 1)
        end = terminal or bool(truncate_every and t % truncate_every == truncate_every - 1) or (truncate_from is not None and t >= truncate_from)
        out.append(TransitionElement(obs, int(rng.integers(4)), float(rng.normal()), terminal, end))
    return out


class Twins:
    """Pairs (solo, group) of buffers built alike; ``check`` compares every pair.  ``ring`` / ``rows`` read a buffer's frame
    ring [n_frames][frame_bytes] and device rows [capacity][8] as numpy arrays (the stub and the device differ only there)."""

    def __init__(self, solo, group, ring, rows):
        self.solo, self.group, self.ring, self.rows = list(solo), list(group), ring, rows
        self.valid_from = [0] * len(self.solo)  # oldest frame (transition index) whose ring slot holds defined bytes
        self.n_frames = [None] * len(self.solo)
        self.grown = [0] * len(self.solo)
        self.frames = [[] for _ in self.solo]

    def step(self, collector, transitions, members=None, **kwargs):
        """One lock-step collection: ``rb.add`` on the solo twins, ``add_many`` on the others."""
        members = list(range(len(transitions))) if members is None else list(members)
        for m, tr in zip(members, transitions):
            self.solo[m].add(tr, **kwargs)
            self.frames[m].append(tr.observation)
        collector.add_many(transitions, None if members == list(range(len(self.solo))) else members, **kwargs)

    def check(self, flush_solo=True, where=""):
        for g, (a, b) in enumerate(zip(self.solo, self.group)):
            tag = f"{where} member {g}"
            assert (a._add_count, a._t) == (b._add_count, b._t), tag
            if a._frames is None:
                assert b._frames is None, tag
                continue
            if flush_solo:
                a._flush_meta()  # the solo twin's rows travel at its next sample; the collector's have travelled already
                assert b._flushed == b._add_count == a._flushed, (tag, a._flushed, b._flushed, b._add_count)
            assert a._n_frames == b._n_frames and a._frame_bytes == b._frame_bytes, tag
            if self.n_frames[g] not in (None, a._n_frames):  # the ring grew: only the frames alive elements need were moved
                self.valid_from[g] = int(a._first_frame[max(0, a._add_count - a._max_capacity) % a._max_capacity])
                self.grown[g] += 1
            self.n_frames[g] = a._n_frames
            assert np.array_equal(a._meta, b._meta) and np.array_equal(a._first_frame, b._first_frame), tag
            assert np.array_equal(a._action, b._action) and np.array_equal(a._reward64, b._reward64), tag
            assert np.array_equal(self.rows(a), self.rows(b)), f"{tag}: element rows on the device"
            assert np.array_equal(self.rows(b), b._meta), f"{tag}: device rows against the host mirror"
            ts = np.arange(max(self.valid_from[g], a._t - a._n_frames), a._t)
            ra, rb = self.ring(a), self.ring(b)
            assert ra.shape == rb.shape == (a._n_frames, a._frame_bytes), tag
            assert np.array_equal(ra[ts % a._n_frames], rb[ts % a._n_frames]), f"{tag}: ring bytes of the written slots"
            if len(ts):  # ... which are the frames that went in (self.frames[g][t]: frame of transition t)
                want = np.stack([np.ascontiguousarray(self.frames[g][t]).view(np.uint8).reshape(-1) for t in ts])
                assert np.array_equal(rb[ts % a._n_frames], want), f"{tag}: ring bytes against the frames added"
            sa, sb = a._sampling_distribution, b._sampling_distribution
            assert list(sa._index_to_key) == list(sb._index_to_key) and dict(sa._key_to_index) == dict(sb._key_to_index), f"{tag}: sampler keys"
