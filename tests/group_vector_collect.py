"""What the group vector-collection tests share (tests/test_group_vector_collect_host.py on numpy stubs,
tests/test_gpu_group_vector_collect.py on the device): scripted vector steps and the twin comparison -- one set of
``VectorReplayBuffer`` objects driven by ``rb.add_many``, an identical set by ``GroupVectorCollector.add_many``, compared field by
field and byte by byte, without a tolerance, after every step."""
import numpy as np

from slimdqn.sample_collection.replay_buffer import TransitionElement


def make_vector_script(seed, n_envs, shape, dtype, steps, lengths=(4, 7, 5), p_none=0.15, idle=(), n_actions=4):
    """``steps`` vector steps of ``n_envs`` entries: environment e runs episodes of ``lengths[e % len]`` transitions, every other one
    ended by a terminal, the rest truncated; an entry is ``None`` with probability ``p_none`` (that time line idles) and every
    entry is ``None`` at the steps named in ``idle`` (the member has no frame at all)."""
    rng = np.random.default_rng(seed)
    count, episode, out = [0] * n_envs, [0] * n_envs, []
    for t in range(steps):
        row = []
        for e in range(n_envs):
            if t in idle or rng.random() < p_none:
                row.append(None)
                continue
            if np.dtype(dtype) == np.uint8:
                obs = rng.integers(0, 256, shape, dtype=np.uint8)
            else:
                obs = rng.standard_normal(shape).astype(dtype)
            count[e] += 1
            end = count[e] == lengths[e % len(lengths)]
            terminal = end and episode[e] % 2 == 0
            if end:
                count[e], episode[e] = 0, episode[e] + 1
            row.append(TransitionElement(obs, int(rng.integers(n_actions)), float(rng.normal()), terminal, end))
        out.append(row)
    return out


class VectorTwins:
    """Pairs (solo, group) of vector buffers built alike.  ``ring`` / ``rows`` read a buffer's frame ring [n_frames][frame_bytes]
    and device rows [capacity][8] as numpy arrays (the stub and the device differ only there); ``extra(a, b, tag)`` compares
    whatever else the caller's samplers hold on the device."""

    def __init__(self, solo, group, ring, rows, extra=None):
        self.solo, self.group, self.ring, self.rows, self.extra = list(solo), list(group), ring, rows, extra
        n = len(self.solo)
        self.frames = [[[] for _ in range(rb._n_envs)] for rb in self.solo]  # [member][env][t]: the frames that went in
        self.first_valid = [[0] * rb._n_envs for rb in self.solo]  # oldest frame number whose ring slots hold defined bytes
        self.growths = [0] * n

    def step(self, collector, entries, members=None, **kwargs):
        """One vector step of every named member: ``rb.add_many`` on the solo twins, one ``add_many`` on the others."""
        members = list(range(len(entries))) if members is None else list(members)
        for m, row in zip(members, entries):
            rb = self.solo[m]
            counts, segment = list(rb._plan.frame_count), rb._plan.segment
            rb.add_many(row, **kwargs)
            if rb._plan.segment != segment:  # growth moved what the old ring held: frames [count - old segment, count)
                self.first_valid[m] = [max(f, c - segment) for f, c in zip(self.first_valid[m], counts)]
                self.growths[m] += 1
            for e, tr in enumerate(row):
                if tr is not None:
                    self.frames[m][e].append(tr.observation)
        collector.add_many(entries, None if members == list(range(len(self.solo))) else members, **kwargs)

    def check(self, where="", draw=True):
        for g, (a, b) in enumerate(zip(self.solo, self.group)):
            tag = f"{where} member {g}"
            pa, pb = a._plan, b._plan
            assert a._add_count == b._add_count == pb.add_count, tag
            assert (pa.frame_count, pa.add_count, pa.segment, pa.n_growths) == (pb.frame_count, pb.add_count, pb.segment, pb.n_growths), tag
            if a._frames is None:
                assert b._frames is None, tag
                continue
            assert a._n_frames == b._n_frames == pa.n_frames and a._frame_bytes == b._frame_bytes, tag
            for name in ("rows", "env_of", "newest_s", "newest_n", "first_frame", "action", "reward64"):
                assert np.array_equal(getattr(pa, name), getattr(pb, name)), f"{tag}: planner field {name}"
            assert [list(d) for d in pa._live] == [list(d) for d in pb._live], f"{tag}: live elements"
            assert np.array_equal(self.rows(a), self.rows(b)), f"{tag}: element rows on the device"
            assert np.array_equal(self.rows(b), pb.rows), f"{tag}: device rows against the host mirror"
            ra, rb_ = self.ring(a), self.ring(b)
            assert ra.shape == rb_.shape == (a._n_frames, a._frame_bytes), tag
            slots, want = [], []
            for e in range(a._n_envs):
                count = pa.frame_count[e]
                for t in range(max(self.first_valid[g][e], count - pa.segment), count):
                    frame = np.ascontiguousarray(self.frames[g][e][t]).view(np.uint8).reshape(-1)
                    slots.append(pa.main_slot(e, t))
                    want.append(frame)
                    if pa.mirror_slot(e, t) is not None:
                        slots.append(pa.mirror_slot(e, t))
                        want.append(frame)
            if slots:
                assert len(set(slots)) == len(slots), tag
                assert np.array_equal(ra[slots], rb_[slots]), f"{tag}: ring bytes of the written slots"
                assert np.array_equal(rb_[slots], np.stack(want)), f"{tag}: ring bytes against the frames added"
            sa, sb = a._sampling_distribution, b._sampling_distribution
            assert list(sa._index_to_key) == list(sb._index_to_key) and dict(sa._key_to_index) == dict(sb._key_to_index), f"{tag}: sampler keys"
            if self.extra is not None:
                self.extra(a, b, tag)
            if draw and len(sa._index_to_key):
                assert np.array_equal(np.asarray(a.sample_slots()), np.asarray(b.sample_slots())), f"{tag}: sample_slots under the same generator"
