"""CPU, gloo at world 2 and 4: the host protocol of ``DataParallelLearner`` (slimdqn/networks/parallel.py).

The device pieces (frame ring, sum tree, samplers) are replaced by the CPU oracle (oracle/replay_ref.py, samplers_ref.py,
sumtree_ref.py), as tests/test_dp_gloo.py does for the agent.  What is checked is what the learner itself decides:
  * every rank draws the same global batch itself (the reference-captured sampler traces), and the contiguous shards of the
    slots and of the importance weights partition it;
  * the all-gathered |TD| ``[W][K][b]`` reassembles into global-batch order;
  * ``replicas_digest`` agrees on replicated buffers (filled through ``DataParallelLearner.add``, i.e. broadcast from rank 0)
    and tells them apart after one extra ``add`` on one rank.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _paths():
    root = os.path.dirname(HERE)
    for p in (root, os.path.join(root, "i-dqn_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


def _oracle_classes():
    from oracle.replay_ref import ReplayRef, Transition
    from oracle.samplers_ref import PrioritizedRef, UniformRef

    class Uniform(UniformRef):  # the generator under the name the product's samplers use
        _rng_key = property(lambda self: self.rng)

    class Prioritized(PrioritizedRef):
        _rng_key = property(lambda self: self.rng)

    class Replay(ReplayRef):
        _batch_size = property(lambda self: self.batch_size)

        def sample_slots(self, size=None):
            keys = self.sampler.sample(self.batch_size if size is None else size)
            return (np.asarray(keys, np.int64) % self.max_capacity).astype(np.int32)

    return Uniform, Prioritized, Replay, Transition


class _TraceReplay:
    """Replay stand-in over a bare sampler: the sampler traces are key-level scripts (capacity > every key: slot == key)."""

    def __init__(self, sampler, batch_size):
        self._sampling_distribution, self._batch_size, self.add_count, self._max_capacity = sampler, batch_size, 0, 1 << 30

    def sample_slots(self, size=None):
        return (np.asarray(self._sampling_distribution.sample(size or self._batch_size), np.int64) % self._max_capacity).astype(np.int32)


def _weights(tree, leaves, n_items, beta):
    """per_importance_weights restated: (n p / root)^-beta / max over the GLOBAL batch."""
    p = np.asarray([tree.get(int(i)) for i in leaves])
    w = (n_items * p / tree.root) ** (-beta)
    return (w / w.max()).astype(np.float32)


def _all(obj):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def _check_sharding(rank, world):
    import kat_int_path as kat

    from slimdqn.networks.parallel import DataParallelLearner, shard_range

    Uniform, Prioritized, _, _ = _oracle_classes()
    z, meta = kat.load_sampler_traces()
    # uniform traces: every rank replays the script and draws through the learner's path (rb.sample_slots(B))
    for ci in range(3):
        rb = _TraceReplay(Uniform(meta[ci]["seed"]), 8 * world)
        learner = DataParallelLearner(None, rb, prioritized=False)
        drawn, n_sharded = [], 0
        for op, arg in z[f"u{ci}_script"]:
            if op == 0:
                rb._sampling_distribution.add(int(arg))
            elif op == 1:
                rb._sampling_distribution.remove(int(arg))
            else:
                keys = rb.sample_slots(int(arg))
                drawn.append(keys)
                if int(arg) % world == 0:  # a global batch: the contiguous shards partition it, in rank order
                    lo, hi = shard_range(rank, world, int(arg))
                    assert np.concatenate(_all(keys[lo:hi])).tolist() == keys.tolist()
                    n_sharded += 1
        np.testing.assert_array_equal(np.concatenate(drawn), z[f"u{ci}_samples"])
        assert n_sharded > 0
        every = _all(np.concatenate(drawn).tolist())
        assert all(e == every[0] for e in every), "ranks drew different keys"
        # the learner's own shard of a B-sample draw
        keys = rb.sample_slots()
        shards = _all(learner.shard(keys).tolist())
        assert sum(shards, []) == keys.tolist() and all(len(s) == 8 for s in shards)
    # prioritized traces: the same keys on every rank, and the weights' max-normalisation is the global batch's
    for pi, m in enumerate([x for x in meta if x["kind"] == "prioritized"]):
        s = Prioritized(m["seed"], m["cap"], m["alpha"])
        for rec in m["recs"]:
            if rec["op"] == 0:
                s.add(rec["key"], priority=rec["prio"])
            elif rec["op"] == 1:
                s.remove(rec["key"])
            elif rec["op"] == 3:
                s.update(np.asarray(rec["keys"], np.int32), np.asarray(rec["prios"], np.float64))
            else:
                np.testing.assert_array_equal(s.sample(rec["n"]), rec["out"])
        np.testing.assert_array_equal(np.asarray(s._sum_tree._nodes), z[f"p{pi}_final_nodes"])
        B = 4 * world
        learner = DataParallelLearner(None, _TraceReplay(s, B), prioritized=False)
        leaves = s.tree.query(s.rng.uniform(0.0, s.tree.root, size=B))
        w = _weights(s.tree, leaves, len(s.index_to_key), 0.4)
        got_l, got_w = _all(learner.shard(leaves).tolist()), _all(learner.shard(w).tolist())
        assert sum(got_l, []) == leaves.tolist()
        np.testing.assert_array_equal(np.asarray(sum(got_w, []), np.float32), w)
        assert max(sum(got_w, [])) == 1.0


def _check_gather(rank, world):
    from slimdqn.networks.parallel import DataParallelLearner, global_order

    K, b = 3, 5
    B = world * b
    learner = DataParallelLearner(None, _TraceReplay(None, B), prioritized=False)
    k, j = np.meshgrid(np.arange(K), np.arange(b), indexing="ij")
    td = torch.from_numpy((1000 * k + rank * b + j).astype(np.float32))  # exact in f32
    gathered = learner.gather_td(td)
    assert tuple(gathered.shape) == (world, K, b)
    want = (1000 * np.arange(K)[:, None] + np.arange(B)[None, :]).astype(np.float32)
    np.testing.assert_array_equal(global_order(gathered).numpy(), want)
    np.testing.assert_array_equal(global_order(gathered.numpy()), want)
    # and it inverts the gather: rank r's block of the global order is rank r's own [K][b]
    for r in range(world):
        np.testing.assert_array_equal(global_order(gathered).numpy()[:, r * b : (r + 1) * b], gathered[r].numpy())


def _check_digest(rank, world):
    from slimdqn.networks.parallel import DataParallelLearner

    Uniform, Prioritized, Replay, Transition = _oracle_classes()
    for make in (lambda: Uniform(3), lambda: Prioritized(3, 64, 0.6)):
        rb = Replay(make(), 2 * world, 64, stack_size=4, update_horizon=1, gamma=0.99)
        learner = DataParallelLearner(None, rb, prioritized=False)
        rng = np.random.default_rng(5)
        kw = {"priority": 1.0} if isinstance(rb.sampler, Prioritized) else {}
        for i in range(30):  # only rank 0 has the transitions: add() broadcasts them
            tr = Transition(rng.integers(0, 256, (6, 6), dtype=np.uint8), int(rng.integers(4)), float(rng.normal()),
                            bool(i % 11 == 10), False)
            learner.add(tr if rank == 0 else None, **(kw if rank == 0 else {}))
        assert rb.add_count > 0
        rb.sample_slots()  # the draw advances every replica's generator alike
        d = learner.replicas_digest()
        assert len(d) == world and len(set(d)) == 1, d
        if rank == 1:  # one extra add on one rank only
            rb.add(Transition(np.zeros((6, 6), np.uint8), 0, 0.0, False, False), **kw)
        d = learner.replicas_digest()
        assert d[1] != d[0] and len(set(d[:1] + d[2:])) == 1, d


def _worker(rank, world, port, what, out):
    _paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        {"sharding": _check_sharding, "gather": _check_gather, "digest": _check_digest}[what](rank, world)
        open(os.path.join(out, f"ok{rank}"), "w").close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("what", ["sharding", "gather", "digest"])
def test_dp_learner_protocol(tmp_path, what, world):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(world, port, what, str(tmp_path)), nprocs=world, join=True)
    assert sorted(os.listdir(tmp_path)) == [f"ok{r}" for r in range(world)]


def test_unequal_shards_are_refused():
    _paths()
    from slimdqn.networks.parallel import shard_range

    assert shard_range(1, 4, 256) == (64, 128)
    with pytest.raises(ValueError, match="equal shards"):
        shard_range(0, 3, 64)
