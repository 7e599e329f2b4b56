"""GPU: the data-parallel learner (slimdqn/networks/parallel.py::DataParallelLearner) and the native entry points under it.

Two ranks on one card over gloo (RCCL refuses two ranks per GPU): each rank holds a replica of the same replay, draws the same
global batch of 64 itself, learns on its 32-sample shard staged from its own frame ring (the Python factored schedule fed by the
replay-sourced split step), and -- prioritized -- writes the gathered |TD| back into its replica of the sum tree.  Both ranks
must land on the single-device 64-sample step and stay bit-identical to each other.

One rank on RCCL: ``idqn_dp_learn_on_replay`` (host and device slots) against ``idqn_dp_step`` on the gathered shard, the split
steps of ``idqn_learn_on_replay`` against the same split on the gathered batch, ``per_priorities_from_td_gathered`` against
``per_priorities_from_td``, and the refused combinations.
"""
import ctypes as C
import hashlib
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OBS, A, K, FEATS, B, LR = (84, 84, 4), 18, 2, [32, 64, 64, 512], 64, 6.25e-5


def _paths():
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "i-dqn_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)


def _agent():
    from slimdqn.networks.idqn import iDQN

    return iDQN(0, OBS, A, K, FEATS, "cnn", LR, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)


def _replay(kind, batch_size=B):
    """The same synthetic transitions on every call: ring and slots have wrapped, episode starts (zero frames) included."""
    from slimdqn.sample_collection.per import SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    cap = 300
    sampler = UniformSamplingDistribution(5) if kind == "uniform" else SlotPrioritizedSampler(5, cap, 0.6)
    rb = ReplayBuffer(sampler, batch_size=batch_size, max_capacity=cap, stack_size=4, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(9)
    for i in range(450):
        tr = TransitionElement(rng.integers(0, 256, OBS[:2], dtype=np.uint8), int(rng.integers(A)), float(rng.normal()),
                               bool(i % 37 == 36), bool(i % 91 == 90))
        rb.add(tr, **({"priority": float(rng.random() + 0.1)} if kind == "prioritized" else {}))
    return rb


def _sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


# ---- two ranks on one card over gloo -------------------------------------------------------------------------------------
def _worker(rank, world, port, kind, out):
    _paths()
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from slimdqn.networks.parallel import DataParallelLearner

        agent, rb = _agent(), _replay(kind)
        learner = DataParallelLearner(agent, rb)
        assert learner.prioritized == (kind == "prioritized") and learner.batch == B // world
        learner.update_online_params(0)
        torch.cuda.synchronize()
        first = dict(losses=agent._losses.cpu().numpy().copy(), online=agent._online.cpu().numpy())
        if kind == "prioritized":
            bf = learner._bufs
            first.update(leaves=bf["leaves"].cpu().numpy(), weights=bf["weights"].cpu().numpy(),
                         priorities=bf["priorities"].cpu().numpy())
        for step in range(1, 20):
            learner.update_online_params(step)
        torch.cuda.synchronize()
        digest = learner.replicas_digest()
        last = dict(online=agent._online.cpu().numpy(), mu=agent._mu.cpu().numpy(), nu=agent._nu.cpu().numpy(),
                    count=agent._count.cpu().numpy(), cum=agent._cum.cpu().numpy(), digest=np.asarray(digest, np.int64))
        if kind == "prioritized":
            t = rb._sampling_distribution._sum_tree
            last.update(nodes_sha=np.frombuffer(_sha(t._nodes_dev).encode(), np.uint8),
                        online_sha=np.frombuffer(_sha(agent._online).encode(), np.uint8),
                        max_priority=rb._sampling_distribution._max_priority_dev.cpu().numpy())
        np.savez(f"{out}/first{rank}.npz", **first)
        np.savez(f"{out}/last{rank}.npz", **last)
    finally:
        dist.destroy_process_group()


def _spawn(kind, out):
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, kind, out), nprocs=2, join=True)
    return ([np.load(f"{out}/first{r}.npz") for r in range(2)], [np.load(f"{out}/last{r}.npz") for r in range(2)])


def _close_to(got, ref, what):
    """The tolerances of tests/test_gpu_dp_two_ranks.py (two shards sum their blocks in another order than one 64-sample step)."""
    assert np.abs(got["losses"] - ref["losses"]).max() <= 1e-5, what
    err = np.abs(got["online"] - ref["online"])
    assert (err <= 3e-7).mean() >= 0.98 and err.max() <= 2 * LR, (what, float(err.max()))


def _bit_identical(last, keys):
    for k in keys:
        np.testing.assert_array_equal(last[0][k], last[1][k], err_msg=f"ranks diverged in {k}")


def test_two_ranks_uniform(tmp_path):
    import torch

    first, last = _spawn("uniform", str(tmp_path))
    agent, rb = _agent(), _replay("uniform")
    agent.update_online_params(0, rb)  # the single-device update_online_params, B = 64, the same keys
    torch.cuda.synchronize()
    ref = dict(losses=agent._losses.cpu().numpy(), online=agent._online.cpu().numpy())
    for r in range(2):
        _close_to(first[r], ref, f"rank {r}, step 1")
    _bit_identical(last, ("online", "mu", "nu", "count", "cum"))
    assert last[0]["count"].tolist() == [20] * K
    assert len(set(last[0]["digest"].tolist())) == 1


def test_two_ranks_prioritized(tmp_path):
    import torch

    from slimdqn.sample_collection.per import PrioritizedLearner

    first, last = _spawn("prioritized", str(tmp_path))
    agent, rb = _agent(), _replay("prioritized")
    pl = PrioritizedLearner(agent, rb)
    pl.step()
    torch.cuda.synchronize()
    ref = dict(losses=agent._losses.cpu().numpy(), online=agent._online.cpu().numpy())
    for r in range(2):
        np.testing.assert_array_equal(first[r]["leaves"], pl._leaves.cpu().numpy())  # the same leaves drawn
        np.testing.assert_array_equal(first[r]["weights"], pl._weights.cpu().numpy())  # global-batch weights, bit for bit
        np.testing.assert_allclose(first[r]["priorities"], pl._priorities.cpu().numpy(), rtol=1e-5, atol=1e-5)
        _close_to(first[r], ref, f"rank {r}, step 1")
    np.testing.assert_array_equal(first[0]["priorities"], first[1]["priorities"])
    _bit_identical(last, ("nodes_sha", "online_sha", "online", "mu", "nu", "count", "cum", "max_priority"))
    assert len(set(last[0]["digest"].tolist())) == 1


# ---- one rank on RCCL ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rccl_group():
    import torch
    import torch.distributed as dist

    owns = not dist.is_initialized()
    if owns:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    if owns:
        dist.destroy_process_group()


def _ring(rb):
    from slimdqn import _hip

    frames, n_frames, frame_bytes, rows, stack, _, _ = rb.ring_view()
    return (_hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows)), int(stack)


def _state(agent):
    return {n: getattr(agent, n).cpu().numpy() for n in ("_online", "_mu", "_nu", "_losses", "_cum", "_count")}


def _assert_same(a, b):
    sa, sb = _state(a), _state(b)
    for n in sa:
        np.testing.assert_array_equal(sa[n], sb[n], err_msg=n)


@pytest.mark.parametrize("slots_on", ["host", "device"])
def test_dp_learn_on_replay_is_dp_step_on_the_gathered_shard(rccl_group, slots_on):
    import torch

    from slimdqn import _hip
    from slimdqn.networks.parallel import _native_handle, data_parallel_step

    lib = _hip.lib()
    rb = _replay("uniform")
    a, b = _agent(), _agent()
    ring, stack = _ring(rb)
    for _ in range(3):
        slots = rb.sample_slots(B)
        data_parallel_step(a, rb._gather(slots), B, mode="native")  # idqn_dp_step on the materialised shard
        b._ensure_handle(B)
        dp = _native_handle(b, None)
        if slots_on == "host":
            hs = np.ascontiguousarray(slots, np.int32)
            rc = lib.idqn_dp_learn_on_replay(dp, *ring, stack, hs.ctypes.data, None, B, B, None, 0, _hip.current_stream())
        else:
            ds = torch.from_numpy(slots.astype(np.int32)).cuda()
            rc = lib.idqn_dp_learn_on_replay(dp, *ring, stack, None, _hip.ptr(ds), B, B, None, 0, _hip.current_stream())
        _hip.check(rc, "idqn_dp_learn_on_replay")
    torch.cuda.synchronize()
    _assert_same(a, b)
    assert b._count.cpu().tolist() == [3] * K


@pytest.mark.parametrize("flag", ["stop_after_dense0", "stop_before_dense0_wgrad"])
@pytest.mark.parametrize("slots_on", ["host", "device"])
def test_split_steps_on_the_replay_source(rccl_group, flag, slots_on):
    """idqn_learn_on_replay(_dev) with an IDQN_F_STOP_* flag, finished by the existing calls, against idqn_learn_on_batch on the
    gathered batch with the same flag finished the same way: bit for bit (the replay source is dropped when the call returns)."""
    import torch

    from slimdqn import _hip
    from slimdqn.networks.parallel import _factored_step

    lib, q = _hip.lib(), _hip.current_stream
    rb = _replay("uniform")
    a, b = _agent(), _agent()
    ring, stack = _ring(rb)
    for _ in range(2):
        slots = np.ascontiguousarray(rb.sample_slots(B), np.int32)
        batch = rb._gather(slots)
        for x in (a, b):
            x._ensure_handle(B)
        ds = torch.from_numpy(slots).cuda()

        def replay(flags):
            if slots_on == "host":
                rc = lib.idqn_learn_on_replay(b._handle, *ring, slots.ctypes.data, B, stack, B, flags, q())
            else:
                rc = lib.idqn_learn_on_replay_dev(b._handle, *ring, _hip.ptr(ds), B, stack, B, flags, q())
            _hip.check(rc, "idqn_learn_on_replay")

        if flag == "stop_after_dense0":
            a._learn(batch, flags=_hip.F_STOP_AFTER_DENSE0, mean_divisor=B)
            replay(_hip.F_STOP_AFTER_DENSE0)
            for x in (a, b):
                _hip.check(lib.idqn_backward_rest(x._handle, q()), "idqn_backward_rest")
                x._apply_adam()
        else:
            _factored_step(a, batch, B, None, 0)
            _factored_step(b, None, B, None, 0, forward=replay, batch=B)
    torch.cuda.synchronize()
    _assert_same(a, b)


def test_gathered_priorities_kernel(rccl_group):
    import torch

    from slimdqn import _hip
    from slimdqn.networks.parallel import global_order

    lib, q = _hip.lib(), _hip.current_stream()
    g = torch.Generator().manual_seed(3)
    for reduce_max in (0, 1):
        # W = 1: bit-identical to per_priorities_from_td, running maximum included
        td = (torch.rand((K, 96), generator=g) * 3).cuda()
        outs = []
        for fn in ("per_priorities_from_td", "per_priorities_from_td_gathered"):
            pr = torch.empty(96, dtype=torch.float64, device="cuda")
            mx = torch.ones(1, dtype=torch.float64, device="cuda")
            args = (K, 96) if fn == "per_priorities_from_td" else (1, K, 96)
            _hip.check(getattr(lib, fn)(_hip.ptr(td), *args, reduce_max, 1e-6, 0.6, _hip.ptr(pr), _hip.ptr(mx), q), fn)
            outs.append((pr, mx))
        torch.cuda.synchronize()
        for x, y in zip(*outs):
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
        # W = 3: the [W][K][b] layout gives what the single-device kernel gives on the same errors in global order
        td_all = (torch.rand((3, K, 32), generator=g) * 3).cuda()
        flat = global_order(td_all).contiguous()
        p1, p2 = (torch.empty(96, dtype=torch.float64, device="cuda") for _ in range(2))
        _hip.check(lib.per_priorities_from_td(_hip.ptr(flat), K, 96, reduce_max, 1e-6, 0.6, _hip.ptr(p1), None, q), "p")
        _hip.check(lib.per_priorities_from_td_gathered(_hip.ptr(td_all), 3, K, 32, reduce_max, 1e-6, 0.6, _hip.ptr(p2), None, q), "p")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(p1.cpu().numpy(), p2.cpu().numpy())


def test_invalid_combinations_are_refused(rccl_group):
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN
    from slimdqn.networks.parallel import _native_handle

    lib = _hip.lib()
    rb = _replay("uniform")
    agent = _agent()
    agent._ensure_handle(B)
    dp = _native_handle(agent, None)
    ring, stack = _ring(rb)
    hs = np.ascontiguousarray(rb.sample_slots(B), np.int32)
    ds = torch.from_numpy(hs).cuda()
    td_all = torch.zeros((1, K, B), dtype=torch.float32, device="cuda")

    def call(sh, sd, batch, gb, td=None):
        return _hip.check(lib.idqn_dp_learn_on_replay(dp, *ring, stack, sh, sd, batch, gb, td, 0, _hip.current_stream()), "dp")

    with pytest.raises(_hip.HipExtensionError, match="is not 1 ranks x 32 samples"):
        call(hs.ctypes.data, None, 32, B)
    with pytest.raises(_hip.HipExtensionError, match="exactly one of slots_host / slots_dev must be set .got both"):
        call(hs.ctypes.data, _hip.ptr(ds), B, B)
    with pytest.raises(_hip.HipExtensionError, match="exactly one of slots_host / slots_dev must be set .got neither"):
        call(None, None, B, B)
    with pytest.raises(_hip.HipExtensionError, match="td_all_dev is set but the handle writes no"):
        call(hs.ctypes.data, None, B, B, _hip.ptr(td_all))
    w, td = torch.ones(B, dtype=torch.float32, device="cuda"), torch.zeros((K, B), dtype=torch.float32, device="cuda")
    _hip.check(lib.idqn_set_per_buffers(agent._handle, _hip.ptr(w), _hip.ptr(td)), "idqn_set_per_buffers")
    try:
        with pytest.raises(_hip.HipExtensionError, match="td_all_dev is null"):
            call(hs.ctypes.data, None, B, B)
    finally:
        _hip.check(lib.idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    torch.cuda.synchronize()
    assert agent._count.cpu().tolist() == [0] * K  # nothing of a refused call was enqueued
    # a non-cnn arch and the general-shape conv path: no data-parallel step object comes up on their handles, and the replay
    # source refuses them
    uid = (C.c_ubyte * _hip.DP_UNIQUE_ID_BYTES)()
    for other in (iDQN(0, 8, 4, 2, [16, 16], "fc", 1e-3, 0.99, 1, 1, 10**9, 10**9),
                  iDQN(0, OBS, 6, 1, [2, 3, 1, 15], "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9)):
        other._ensure_handle(B)
        h = C.c_void_p()
        with pytest.raises(_hip.HipExtensionError, match="built for the MFMA cnn path"):
            _hip.check(lib.idqn_dp_create(other._handle, uid, 0, 1, 0, C.byref(h)), "idqn_dp_create")
        with pytest.raises(_hip.HipExtensionError, match="needs the cnn arch on the plane conv path"):
            _hip.check(lib.idqn_learn_on_replay_dev(other._handle, *ring, _hip.ptr(ds), B, stack, B, 0, _hip.current_stream()), "r")


def test_learner_on_rccl_one_rank_runs_the_native_step(rccl_group):
    """DataParallelLearner on RCCL goes through idqn_dp_learn_on_replay and equals the direct call bit for bit (uniform), and
    its prioritized step keeps the tree's root and the running maximum finite and moving."""
    import torch

    from slimdqn import _hip
    from slimdqn.networks.parallel import DataParallelLearner, _native_handle

    lib = _hip.lib()
    rb_a, rb_b = _replay("uniform"), _replay("uniform")
    a, b = _agent(), _agent()
    learner = DataParallelLearner(a, rb_a)
    ring, stack = _ring(rb_b)
    for step in range(3):
        learner.update_online_params(step)
        b._ensure_handle(B)
        hs = np.ascontiguousarray(rb_b.sample_slots(B), np.int32)
        _hip.check(lib.idqn_dp_learn_on_replay(_native_handle(b, None), *ring, stack, hs.ctypes.data, None, B, B, None, 0,
                                               _hip.current_stream()), "idqn_dp_learn_on_replay")
    torch.cuda.synchronize()
    assert a.__dict__.get("_dp") is not None and not getattr(a, "_native_dp_failed", False)
    _assert_same(a, b)
    rb = _replay("prioritized")
    c = _agent()
    pl = DataParallelLearner(c, rb)
    root0 = rb._sampling_distribution._sum_tree.root
    for step in range(3):
        pl.update_online_params(step)
    torch.cuda.synchronize()
    root1 = rb._sampling_distribution._sum_tree.root
    assert np.isfinite(root1) and root1 != root0
    assert np.isfinite(c._losses.cpu().numpy()).all() and c._count.cpu().tolist() == [3] * K
    assert len(pl.replicas_digest()) == 1
