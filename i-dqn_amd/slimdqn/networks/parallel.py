"""Data-parallel i-DQN step over the GPUs of one node (one process per GPU, RCCL over xGMI).

The reference is single-device; the loss is a plain mean over the minibatch (``slimdqn/networks/idqn.py:111-112``),
so the gradient of a global batch of ``B * world`` samples is the SUM of the shard gradients when every shard
divides by the global batch size.  The gradients are all-reduced, then the identical Adam update runs on every
rank, which keeps the replicas bit-identical.  ``torch.distributed`` is plumbing here: backend "nccl" is RCCL on
ROCm; the CPU tests drive the same function over "gloo".

Overlap (GPU, cnn path): 98 % of the 80.9 MB of gradients is Dense_0/kernel, and the backward pass produces it
FIRST.  The step is therefore issued as two C calls: ``idqn_learn_on_batch(..., IDQN_F_STOP_AFTER_DENSE0)`` queues
everything up to the Dense_0 weight gradient, the K contiguous Dense_0 slices are all-reduced asynchronously (RCCL
runs them on its own stream, ordered behind that point of the compute stream), and ``idqn_backward_rest`` queues
the conv backward, which then runs concurrently with the collective.  The gradient arena is laid out as two
contiguous regions for exactly this: ``[all heads' small leaves + the K losses][all heads' Dense_0 slices]`` -- two
collectives per step, no packing.  xGMI is point-to-point (7 links per GPU), so a few large collectives beat many
small ones.  ``IDQN_DP_OVERLAP=0`` falls back to one all-reduce of the whole arena after the backward pass.

Factored mode (GPU, cnn path, the default): the Dense_0/kernel gradient is the outer product ``a3^T . dh`` over the
samples, i.e. of rank <= global batch, far below its 7744 x 512 shape.  Ranks therefore ALL-GATHER the two factors
(``a3``: K x 7744 x 32 floats, ``dh``: K x 512 x 32 floats -- 5.3 MB per rank at K=5, one contiguous run inside the
library: nothing is copied before the collective) instead of all-reducing the
79.3 MB product, and every rank runs the fused weight-gradient + Adam kernel over the gathered global batch: 4x
(8 ranks) to 15x (2 ranks) fewer bytes over xGMI, the gradient is never materialised, and Adam stays fused.  The
gather runs while ``idqn_backward_rest`` computes the conv backward; the 1.6 MB of small leaves (and the K losses)
are all-reduced under the fused Dense_0 update, which needs only the gathered factors.  Every rank sums the same blocks in the same order, so replicas stay bit-identical.
``IDQN_DP_MODE=allreduce`` selects the all-reduce variants above.

Native mode (GPU, cnn path, RCCL backend: the default there): the SAME factored schedule issued by ONE C call,
``idqn_dp_step`` (``include/idqn_hip.h``, ``csrc/dp.hip``) -- the library owns an RCCL communicator (``idqn_dp_create``: rank 0's
``ncclGetUniqueId`` bytes are broadcast over this process group once) and enqueues forward -> ``ncclAllGather`` of the factor
run -> conv backward -> ``ncclAllReduce`` of the small region -> fused update itself, with the collectives on a side stream of
its own ordered by events (``IDQN_DP_STREAMS=inline``: on the compute stream).  The Python schedule below stays as the
oracle of that call (``tests/test_gpu_configs.py``: bit-identical) and as the path of the gloo tests.
``IDQN_DP_MODE=factored`` selects it on RCCL too.
"""
import ctypes as C
import os

import torch.distributed as dist

from slimdqn import _hip


def _factored_step(agent, shard, global_batch, group, extra_flags, serial=False, forward=None, batch=None):
    """``forward`` (optional): enqueues this rank's step up to the Dense_0 weight gradient for a shard of ``batch`` samples in
    place of ``agent._learn(shard, IDQN_F_STOP_BEFORE_DENSE0_WGRAD)`` (the replay-sourced step of DataParallelLearner)."""
    import torch

    lib, q = _hip.lib(), _hip.current_stream
    world = dist.get_world_size(group)
    K = agent._K
    F, J = next(shape for name, _, shape in agent._leaves if name == "Dense_0/kernel")
    nb = -(-(len(shard.action) if batch is None else int(batch)) // 32)  # 32-sample blocks of this rank's shard
    X, Y = F * 32, J * 32
    n_a3, n_dh = K * nb * X, K * nb * Y
    key = (world, nb)
    if getattr(agent, "_factor_key", None) != key:  # gathered factors, allocated once per (world, shard blocks)
        agent._fact_all = torch.empty(world * (n_a3 + n_dh), dtype=torch.float32, device=agent._grad.device)  # [rank][dh | a3]
        agent._factor_key, agent._fact_send = key, None
    gathered = agent._fact_all
    if forward is None:
        agent._learn(shard, flags=_hip.F_STOP_BEFORE_DENSE0_WGRAD | extra_flags, mean_divisor=global_batch)
    else:
        forward(_hip.F_STOP_BEFORE_DENSE0_WGRAD | extra_flags)
    # this rank's factors: dL/dh directly in front of the online nets' a3 inside the library -- one contiguous run, no copy
    p, c_dh, c_a3 = C.c_void_p(), C.c_int64(), C.c_int64()
    _hip.check(lib.idqn_dense0_factors(agent._handle, C.byref(p), C.byref(c_dh), C.byref(c_a3)), "idqn_dense0_factors")
    assert (c_dh.value, c_a3.value) == (n_dh, n_a3)
    if agent._fact_send is None or agent._fact_send.data_ptr() != p.value:
        agent._fact_send = _hip.device_view(p.value, n_dh + n_a3)
    send = agent._fact_send
    work = dist.all_gather_into_tensor(gathered, send, group=group, async_op=True)  # ONE collective for both factors
    if serial:  # test mode: no collective overlaps any kernel (the stream-race stress compares the two bit for bit)
        work.wait()
        torch.cuda.synchronize()
    _hip.check(lib.idqn_backward_rest(agent._handle, q()), "idqn_backward_rest")  # conv backward, under the gather
    if serial:
        torch.cuda.synchronize()
    small = dist.all_reduce(agent._grad_small, op=dist.ReduceOp.SUM, group=group, async_op=True)  # small leaves + K losses
    if serial:
        small.wait()
        torch.cuda.synchronize()
    work.wait()
    args = (agent._handle, _hip.ptr(gathered[n_dh:]), _hip.ptr(gathered), world * nb, nb, n_a3 + n_dh, nb * X, X,
            n_a3 + n_dh, nb * Y, Y)
    # the 80 us Dense_0 update needs only the gather: it runs while the small all-reduce is still in flight
    _hip.check(lib.idqn_finish_step_factored(*args, _hip.FACTORED_DENSE0, q()), "idqn_finish_step_factored")
    small.wait()
    _hip.check(lib.idqn_finish_step_factored(*args, _hip.FACTORED_REST, q()), "idqn_finish_step_factored")
    return agent._losses


def _native_handle(agent, group, streams=None):
    """The library-side RCCL communicator of this agent's handle (``idqn_dp_create``), created on first use: collective."""
    import torch

    dp = agent.__dict__.get("_dp")
    if dp is not None and dp[1] == agent._handle.value:
        return dp[0]
    if dp is not None:  # the handle was re-created for a larger batch: its dp object went with it (DeviceAgent._destroy_handle)
        agent.__dict__.pop("_dp", None)
    lib = _hip.lib()
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    uid = (C.c_ubyte * _hip.DP_UNIQUE_ID_BYTES)()
    if rank == 0:
        _hip.check(lib.idqn_dp_unique_id(uid), "idqn_dp_unique_id")
    box = [bytes(uid)]
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if streams is None:
        streams = os.environ.get("IDQN_DP_STREAMS", "side")
    flags = _hip.DP_SIDE_STREAM if streams == "side" else 0
    h = C.c_void_p()
    torch.cuda.synchronize()
    rc = lib.idqn_dp_create(agent._handle, box[0], rank, world, flags, C.byref(h))
    # every rank has to agree on the outcome: a communicator that came up on some ranks only would hang the first collective
    ok = torch.tensor([1 if rc == 0 else 0], dtype=torch.int32, device=agent._grad.device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
    if int(ok.item()) == 0:
        msg = lib.idqn_last_error().decode(errors="replace") if rc else "another rank failed"
        if rc == 0:
            lib.idqn_dp_destroy(h)
        raise _NativeUnavailable(f"idqn_dp_create: {msg}")
    agent._dp = (h, agent._handle.value)
    return h


class _NativeUnavailable(RuntimeError):
    """The library-side RCCL communicator could not be created on every rank (the Python schedule over torch.distributed runs instead)."""


def _native_step(agent, shard, global_batch, group, extra_flags, streams=None):
    B, ptrs = agent._prepare(shard)
    dp = _native_handle(agent, group, streams)
    _hip.check(_hip.lib().idqn_dp_step(dp, *ptrs, B, int(global_batch), int(extra_flags), _hip.current_stream()), "idqn_dp_step")
    return agent._losses


def data_parallel_step(agent, shard, global_batch: int, group=None, extra_flags: int = 0, overlap=None, mode=None,
                       serial: bool = False, streams=None):
    """One global gradient step; ``shard`` is this rank's ReplayElement-like slice of the global batch."""
    on_gpu_cnn = agent._grad.is_cuda and getattr(agent, "_arch", "") == "cnn"
    if mode is None:
        rccl = on_gpu_cnn and dist.get_backend(group) == "nccl"  # one rank per GPU: the library's own communicator works
        mode = os.environ.get("IDQN_DP_MODE", "native" if rccl else "factored")
    if mode == "native" and on_gpu_cnn and overlap is None and not serial and not getattr(agent, "_native_dp_failed", False):
        try:
            return _native_step(agent, shard, global_batch, group, extra_flags, streams)
        except _NativeUnavailable as e:  # agreed on by all ranks (see _native_handle): the same HIP kernels, collectives issued from Python
            import sys

            agent._native_dp_failed = True
            print(f"[idqn] native data-parallel step unavailable ({e}); using the Python schedule over torch.distributed", file=sys.stderr, flush=True)
    if mode == "native":
        mode = "factored"
    if mode == "factored" and on_gpu_cnn and overlap is None:
        return _factored_step(agent, shard, global_batch, group, extra_flags, serial)
    if overlap is None:
        overlap = (os.environ.get("IDQN_DP_OVERLAP", "1") != "0" and agent._grad.is_cuda
                   and getattr(agent, "_arch", "") == "cnn")
    if not overlap:
        agent._learn(shard, flags=_hip.F_GRADS_ONLY | extra_flags, mean_divisor=global_batch)
        dist.all_reduce(agent._grad, op=dist.ReduceOp.SUM, group=group)  # the whole arena in one collective
        if not getattr(agent, "_losses_in_grad", False):  # the device agent keeps its losses inside the arena
            dist.all_reduce(agent._losses, op=dist.ReduceOp.SUM, group=group)
        agent._apply_adam()  # Adam from the summed gradient, count += 1, cumulated_losses += losses
        return agent._losses
    # forward, head, Dense_0 data + weight gradient are queued; the conv backward is not yet
    agent._learn(shard, flags=_hip.F_STOP_AFTER_DENSE0 | extra_flags, mean_divisor=global_batch)
    big = dist.all_reduce(agent._grad_w0, op=dist.ReduceOp.SUM, group=group, async_op=True)  # 79.3 MB, 98 %
    if serial:
        import torch

        big.wait()
        torch.cuda.synchronize()
    _hip.check(_hip.lib().idqn_backward_rest(agent._handle, _hip.current_stream()), "idqn_backward_rest")
    dist.all_reduce(agent._grad_small, op=dist.ReduceOp.SUM, group=group)  # 1.6 MB of small leaves + the K losses
    big.wait()  # the compute stream waits for the Dense_0 region
    agent._apply_adam()
    return agent._losses


def shard_of(batch, rank: int, world: int):
    """Contiguous shard ``rank`` of ``world`` of every field of a ReplayElement-like batch."""
    n = len(batch.action)
    assert n % world == 0, f"global batch {n} is not divisible by {world} ranks"
    lo, hi = rank * (n // world), (rank + 1) * (n // world)
    return type(batch)(*[getattr(f, "tensor", f)[lo:hi] for f in batch])


# ---- the data-parallel learner: replay sampling, sharded step, priority write-back ------------------------------------------
def shard_range(rank: int, world: int, global_batch: int):
    """``[lo, hi)`` of rank ``rank``'s contiguous shard of a global batch (equal shards only)."""
    if world < 1 or global_batch % world:
        raise ValueError(f"global batch {global_batch} is not divisible by {world} ranks (equal shards only)")
    b = global_batch // world
    return rank * b, (rank + 1) * b


def global_order(td_gathered):
    """``[W][K][b]`` (every rank's |TD| as all-gathered) -> ``[K][W * b]`` in global-batch order, column ``r * b + j`` being
    rank r's sample j: the layout ``per_priorities_from_td_gathered`` reads directly (numpy array or torch tensor)."""
    W, K, b = td_gathered.shape
    t = td_gathered.transpose(0, 1) if hasattr(td_gathered, "permute") else td_gathered.transpose(1, 0, 2)
    return t.reshape(K, W * b)


def replica_digest(add_count: int, rng_state, root: float) -> int:
    """63-bit digest of what a replica's next draw depends on: add count, sampler generator state, sum-tree root bits."""
    import hashlib
    import json
    import struct

    blob = json.dumps([int(add_count), rng_state], sort_keys=True, default=str).encode() + struct.pack("<d", float(root))
    return int.from_bytes(hashlib.sha256(blob).digest()[:8], "little") >> 1


class DataParallelLearner:
    """``update_online_params`` (idqn.py:65-72: ``replay_buffer.sample()`` + ``learn_on_batch``) over the ranks of ``group``.

    Protocol (replicated replay): every rank's ``ReplayBuffer`` gets the same ``add`` calls and the same sampler seed, so every
    rank draws the SAME global batch of ``B = replay_buffer._batch_size`` keys itself -- nothing about the keys travels.  Rank r
    learns on the contiguous shard ``[r b, (r + 1) b)``, ``b = B / W``, staged straight from its own frame ring inside the step,
    every shard dividing by B; the factored data-parallel step (module docstring) keeps the replicas bit-identical.
    Prioritized (``SlotPrioritizedSampler``): B PCG64 uniforms -> ``per_sample_leaves`` -> ``per_importance_weights`` over all B
    leaves (the max-normalisation is the global batch's) -> the shard's weights and |TD| [K][b] -> all-gathered [W][K][b] ->
    ``per_priorities_from_td_gathered`` in global order -> ONE ``sumtree_set`` on the B global leaves on every rank (running
    maximum included), so the replica trees stay bit-identical too.

    RCCL with one rank per GPU: ``idqn_dp_learn_on_replay`` (the whole step, collectives included, one C call).  Otherwise
    (gloo, several ranks on a card): the Python factored schedule fed by ``idqn_learn_on_replay(_dev)``'s split step.
    Both stage from the frame ring, so they need what ``idqn_learn_on_replay`` needs: Atari-shaped uint8 frames and the plane
    conv path (``IDQN_CONV=bf16x3``, the default); anything else is refused with the library's message (HipExtensionError).
    """

    def __init__(self, agent, replay_buffer, group=None, prioritized=None, beta: float = 0.4, eps: float = 1e-6,
                 reduce: str = "mean", stratified: bool = True):
        from slimdqn.sample_collection.per import SlotPrioritizedSampler

        assert reduce in ("mean", "max")
        self.agent, self.rb, self.group = agent, replay_buffer, group
        self.sampler = replay_buffer._sampling_distribution
        if prioritized is None:
            prioritized = isinstance(self.sampler, SlotPrioritizedSampler)
        if prioritized and not isinstance(self.sampler, SlotPrioritizedSampler):
            raise ValueError("prioritized=True needs a SlotPrioritizedSampler (tree leaf == replay slot)")
        self.prioritized = bool(prioritized)
        self.beta, self.eps, self.reduce_max, self.stratified = float(beta), float(eps), int(reduce == "max"), int(stratified)
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.global_batch = int(replay_buffer._batch_size)
        self.lo, self.hi = shard_range(self.rank, self.world, self.global_batch)
        self.batch = self.hi - self.lo
        self._bufs = None  # device buffers, allocated by the first prioritized step

    # ---- protocol pieces (host) ----------------------------------------------------------------------------------------
    def shard(self, x):
        """This rank's slice of a global-batch array (slots, leaves, weights: numpy or torch, leading axis = B)."""
        assert len(x) == self.global_batch, (len(x), self.global_batch)
        return x[self.lo : self.hi]

    def gather_td(self, td_local, out=None):
        """All-gathers this rank's |TD| ``[K][b]`` into ``[W][K][b]`` (``out``, allocated when None) over the group."""
        import torch

        if out is None:
            out = torch.empty((self.world,) + tuple(td_local.shape), dtype=td_local.dtype, device=td_local.device)
        dist.all_gather_into_tensor(out.view(-1), td_local.contiguous().view(-1), group=self.group)
        return out

    def add(self, transition, **kwargs) -> None:
        """Rank 0's ``transition`` is broadcast over the group and added to every replica (other ranks may pass None)."""
        box = [(transition, kwargs) if self.rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
        tr, kw = box[0]
        self.rb.add(tr, **kw)

    def replicas_digest(self):
        """Every rank's ``replica_digest`` of its replay (add count, sampler RNG state, tree root bits), in rank order.  The
        replicas agree iff all entries are equal.  Collective; reads the tree root (a device read) on a device sampler."""
        import torch

        s = self.sampler
        tree = getattr(s, "_sum_tree", None)
        root = float(tree.root) if tree is not None else 0.0
        d = replica_digest(self.rb.add_count, s._rng_key.bit_generator.state, root)
        dev = "cuda" if dist.get_backend(self.group) == "nccl" else "cpu"
        mine = torch.tensor([d], dtype=torch.int64, device=dev)
        every = torch.empty(self.world, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(every, mine, group=self.group)
        return [int(x) for x in every.cpu()]

    # ---- the step ------------------------------------------------------------------------------------------------------
    def update_online_params(self, step: int) -> None:
        """idqn.py:65-72: one global gradient step every ``update_to_data`` steps; ``cumulated_losses`` grows on the device."""
        if step % self.agent.update_to_data == 0:
            self.step()

    def update_target_params(self, step: int):
        return self.agent.update_target_params(step)  # identical on every rank: the replicas stay equal

    def _native(self):
        return (dist.get_backend(self.group) == "nccl" and os.environ.get("IDQN_DP_MODE", "native") == "native"
                and not getattr(self.agent, "_native_dp_failed", False))

    def _alloc(self):
        import torch

        B, b, K, W = self.global_batch, self.batch, self.agent._K, self.world
        self._bufs = dict(
            u_pin=torch.empty(B, dtype=torch.float64).pin_memory(), u_ev=None,
            u=torch.empty(B, dtype=torch.float64, device="cuda"),
            leaves=torch.empty(B, dtype=torch.int32, device="cuda"),
            weights=torch.empty(B, dtype=torch.float32, device="cuda"),
            td=torch.zeros((K, b), dtype=torch.float32, device="cuda"),
            td_all=torch.zeros((W, K, b), dtype=torch.float32, device="cuda"),
            priorities=torch.empty(B, dtype=torch.float64, device="cuda"))

    def _draw_prioritized(self):
        """B uniforms from the sampler's PCG64 stream -> tree descent -> clamped leaves + global-batch weights (device)."""
        import torch

        lib, q = _hip.lib(), _hip.current_stream()
        if self._bufs is None:
            self._alloc()
        bf, tree, B = self._bufs, self.sampler._sum_tree, self.global_batch
        if bf["u_ev"] is not None:
            bf["u_ev"].synchronize()  # the previous step's upload has left the pinned staging buffer
        bf["u_pin"].copy_(torch.from_numpy(self.sampler._rng_key.random(B)))
        bf["u"].copy_(bf["u_pin"], non_blocking=True)
        bf["u_ev"] = torch.cuda.Event()
        bf["u_ev"].record()
        _hip.check(lib.per_sample_leaves(_hip.ptr(tree._nodes_dev), tree._depth, _hip.ptr(bf["u"]), B, self.stratified,
                                         _hip.ptr(bf["leaves"]), q), "per_sample_leaves")
        _hip.check(lib.per_importance_weights(_hip.ptr(tree._nodes_dev), tree._depth, _hip.ptr(bf["leaves"]), B, len(self.sampler),
                                              self.beta, _hip.ptr(bf["weights"]), q), "per_importance_weights")

    def step(self):
        """One global gradient step; returns the per-head losses of the global batch (device, not synchronised)."""
        import numpy as np

        agent, rb, lib = self.agent, self.rb, _hip.lib()
        assert rb.add_count, "No samples in replay buffer!"
        B, b = self.global_batch, self.batch
        if self.prioritized:
            self._draw_prioritized()
            slots_host, slots_dev = None, self.shard(self._bufs["leaves"])  # (a contiguous device slice: a pointer offset)
        else:
            slots_host = np.ascontiguousarray(self.shard(rb.sample_slots(B)), np.int32)  # the same B keys on every rank
            slots_dev = None
        frames, n_frames, frame_bytes, rows, stack, _, _ = rb.ring_view()
        agent._ensure_handle(b)
        if self.prioritized:
            _hip.check(lib.idqn_set_per_buffers(agent._handle, _hip.ptr(self.shard(self._bufs["weights"])),
                                                _hip.ptr(self._bufs["td"])), "idqn_set_per_buffers")
        try:
            self._learn(frames, n_frames, frame_bytes, rows, stack, slots_host, slots_dev)
        finally:
            if self.prioritized:
                _hip.check(lib.idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
        if self.prioritized:
            bf, tree, q = self._bufs, self.sampler._sum_tree, _hip.current_stream()
            _hip.check(lib.per_priorities_from_td_gathered(_hip.ptr(bf["td_all"]), self.world, agent._K, b, self.reduce_max,
                                                           self.eps, self.sampler._alpha, _hip.ptr(bf["priorities"]),
                                                           _hip.ptr(self.sampler._max_priority_dev), q),
                       "per_priorities_from_td_gathered")
            _hip.check(lib.sumtree_set(_hip.ptr(tree._nodes_dev), tree._depth, _hip.ptr(bf["leaves"]), _hip.ptr(bf["priorities"]),
                                       B, _hip.ptr(tree._scratch), q), "sumtree_set")
        return agent._losses

    def _learn(self, frames, n_frames, frame_bytes, rows, stack, slots_host, slots_dev):
        agent, lib, B, b = self.agent, _hip.lib(), self.global_batch, self.batch
        ring = (_hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows))
        sh = None if slots_host is None else slots_host.ctypes.data
        sd = None if slots_dev is None else _hip.ptr(slots_dev)
        td_all = _hip.ptr(self._bufs["td_all"]) if self.prioritized else None
        if self._native():
            try:
                dp = _native_handle(agent, self.group)
            except _NativeUnavailable as e:
                import sys

                agent._native_dp_failed = True
                print(f"[idqn] native data-parallel step unavailable ({e}); using the Python schedule over torch.distributed",
                      file=sys.stderr, flush=True)
            else:
                _hip.check(lib.idqn_dp_learn_on_replay(dp, *ring, int(stack), sh, sd, b, B, td_all, 0, _hip.current_stream()),
                           "idqn_dp_learn_on_replay")
                return

        def forward(flags):
            if sd is not None:
                rc = lib.idqn_learn_on_replay_dev(agent._handle, *ring, sd, b, int(stack), B, flags, _hip.current_stream())
            else:
                rc = lib.idqn_learn_on_replay(agent._handle, *ring, sh, b, int(stack), B, flags, _hip.current_stream())
            _hip.check(rc, "idqn_learn_on_replay")
            if self.prioritized:  # |TD| of the shard is final once the forward half is queued: gather it under the backward
                self.gather_td(self._bufs["td"], self._bufs["td_all"])

        _factored_step(agent, None, B, self.group, 0, forward=forward, batch=b)
