"""Prioritized experience replay wired end to end on the device -- an EXTENSION.

The reference ships ``PrioritizedSamplingDistribution`` but cannot use it for learning: ``ReplayBuffer.sample``
drops the sampled keys (``replay_buffer.py:222-230``), ``collect_single_sample`` passes no priority
(``slimdqn/sample_collection/utils.py:27-35``) and the loss has no importance weights (``idqn.py:111-112``).
There is therefore no reference behaviour to match here; the pieces are checked against the oracle's weighted loss /
TD errors and against numpy restatements of the formulas (parity unpinned, by construction).

Design (Schaul et al. 2016, proportional variant), all on the GPU, no host synchronisation in the loop:

* ``SlotPrioritizedSampler``: the sum-tree leaf of an element IS its replay slot (``key % max_capacity``), so FIFO
  eviction is the overwrite of that leaf by the newcomer and no key <-> index map is needed on either side;
  newcomers enter with the running maximum priority, which lives in device memory.
* ``PrioritizedLearner.step()``: host draws B uniforms (PCG64) -> ``per_sample_leaves`` (tree descent, stratified)
  -> ``per_importance_weights`` -> ``replay_gather_stacked`` -> ``idqn_learn_on_batch`` with the weights, which also
  emits |TD| per head and sample -> ``per_priorities_from_td`` (mean or max over the K heads, ``(.+eps)^alpha``)
  -> ``sumtree_set`` on the same leaves.
* An ``iIQN`` agent takes the same loop: the quantile loss is weighted per sample and emits the mean absolute pairwise TD
  error per head and sample as its |TD| (``iIQN._learn``).  On a buffer with Atari-shaped uint8 frames the gather is
  skipped: the leaves go straight to ``idqn_iqn_learn_on_replay_dev``, bit-identical to the gathered step.  MLP agents (and
  general-shape cnn agents) skip it the same way through ``idqn_learn_on_replay_fc_dev``.
* Where the agent's replay-sourced conditions hold, the whole chain is ONE C call, ``idqn_per_learn_on_replay`` (two fused
  kernels around the replay-sourced step), byte-identical to the chain; ``fuse_per_step`` / ``fuse_per_family`` below.
* n steps are ONE C call as well, ``idqn_per_learn_steps_on_replay`` (``PrioritizedLearner.steps``): the write-back of a step and
  the draw of the next are one launch (``k_per_turn``), the uniforms of all steps one upload; byte-identical to n ``step()`` calls.
  ``PrioritizedLearner.update_params_many`` is the trainer-side loop over it (``VectorTrainer(..., learner=...)``).
* ``PrioritizedGroupLearner``: the prioritized step of the S MLP agents of an ``AgentGroup`` as ONE C call,
  ``idqn_group_per_learn_on_replay_fc`` (three launches for all members), byte-identical per member to the member's own step;
  n steps of all members as ONE C call, ``idqn_group_per_learn_steps_on_replay_fc`` (``PrioritizedGroupLearner.steps``: the S
  write-backs of a step and the S draws of the next are one launch, ``k_per_group_turn``), byte-identical to n ``step()`` calls.
  ``PrioritizedGroupLearner.update_params_many`` is the trainer-side loop over it (``SeedVectorTrainer(..., learner=...)``).
"""
import ctypes as C
import os

import numpy as np

from slimdqn import _hip
from slimdqn.networks._agent import DeviceAgent, plan_step_runs
from slimdqn.sample_collection import sum_tree


class SlotPrioritizedSampler:
    """Sampler protocol of ``ReplayBuffer`` (add / remove / update / sample) with tree index == replay slot."""

    def __init__(self, seed: int, max_capacity: int, priority_exponent: float = 0.6):
        import torch

        self._max_capacity, self._alpha = max_capacity, priority_exponent
        self._sum_tree = sum_tree.SumTree(max_capacity)
        self._rng_key = np.random.default_rng(seed)
        self._key_of_slot = np.full(max_capacity, -1, np.int64)
        self._max_priority_dev = torch.ones(1, dtype=torch.float64, device="cuda")  # max_recorded_priority starts at 1
        self._size = 0

    def _set_one(self, slot: int, value: float = 0.0, value_dev=None) -> None:
        t = self._sum_tree
        _hip.check(_hip.lib().sumtree_set_one(_hip.ptr(t._nodes_dev), t._depth, int(slot), float(value), _hip.ptr(value_dev),
                                              _hip.current_stream()), "sumtree_set_one")

    def add(self, key, priority=None) -> None:
        slot = int(key) % self._max_capacity
        if self._key_of_slot[slot] < 0:
            self._size += 1
        self._key_of_slot[slot] = int(key)
        if priority is None:
            self._set_one(slot, value_dev=self._max_priority_dev)  # newcomers are sampled at least once soon
        else:
            self._set_one(slot, 0.0 if priority == 0.0 else float(priority) ** self._alpha)

    def remove(self, key) -> None:
        slot = int(key) % self._max_capacity
        if self._key_of_slot[slot] == int(key):  # not yet overwritten by its successor in the FIFO
            self._key_of_slot[slot] = -1
            self._size -= 1
            self._set_one(slot, 0.0)

    def update(self, keys, priorities) -> None:
        keys = np.atleast_1d(np.asarray(keys, np.int64))
        pr = np.atleast_1d(np.asarray(priorities, np.float64))
        self._sum_tree.set((keys % self._max_capacity).astype(np.int32), np.where(pr == 0.0, 0.0, pr**self._alpha))

    def sample(self, size: int):
        """Host-visible variant (synchronises): keys of ``size`` elements drawn in proportion to priority."""
        root = self._sum_tree.root
        slots = self._sum_tree.query(self._rng_key.uniform(0.0, root, size=size))
        return self._key_of_slot[slots].astype(np.int32)

    def __len__(self) -> int:
        return self._size


class PrioritizedLearner:
    """sample -> weights -> gather -> learn -> priorities -> tree update, queued on the stream without a host sync."""

    def __init__(self, agent, replay_buffer, beta: float = 0.4, eps: float = 1e-6, reduce: str = "mean",
                 stratified: bool = True):
        import torch

        assert isinstance(replay_buffer._sampling_distribution, SlotPrioritizedSampler)
        assert reduce in ("mean", "max")
        self.agent, self.rb, self.sampler = agent, replay_buffer, replay_buffer._sampling_distribution
        self.beta, self.eps, self.reduce_max, self.stratified = beta, eps, int(reduce == "max"), int(stratified)
        B, K = replay_buffer._batch_size, agent._K
        self._u_pin = torch.empty(B, dtype=torch.float64).pin_memory()
        self._u_ev = None
        self._u_dev = torch.empty(B, dtype=torch.float64, device="cuda")
        # (zeros, not empty: a step of fewer than B samples leaves the lanes past it unwritten, and what they hold must not
        # depend on what the allocator handed out before -- tests/test_gpu_group_per.py::test_ragged_and_minimal_batches compares
        # the whole rows of two learners after a batch of 16 in rows of 17)
        self._leaves = torch.zeros(B, dtype=torch.int32, device="cuda")
        self._weights = torch.zeros(B, dtype=torch.float32, device="cuda")
        self._td_abs = torch.zeros((K, B), dtype=torch.float32, device="cuda")
        self._priorities = torch.zeros(B, dtype=torch.float64, device="cuda")

    def _replay_sourced(self):
        """The buffer's ring view for an i-IQN agent whose replay-sourced step can read it (the agent's own conditions, its
        switches included), else None."""
        from slimdqn.networks.iiqn import iIQN

        agent, rb = self.agent, self.rb
        if not (isinstance(agent, iIQN) and agent._replay_fusable(rb)):
            return None
        view = rb.ring_view()
        return view if agent._ring_fusable(view) else None

    # The whole step as ONE C call (``idqn_per_learn_on_replay``: uniforms -> k_per_draw -> the agent's replay-sourced step ->
    # k_per_write_back), byte-identical to the chain below.  Taken when the agent's own replay-sourced conditions hold (its
    # switches included) and its ``_learn`` is the stock one; a plain plane-path ``iDQN`` / ``DQN`` agent, which the chain
    # gathers for, qualifies too.  ``IDQN_PER_FUSED=0`` and the attribute switch it off; ``fuse_per_family`` holds the default
    # per agent family, set from the measurements in profiles/per_step_fused.json.  ``_fused_ok`` (unset: not tried; False: the
    # entry refused this handle the first time, the chain from then on; True: it served).
    # Defaults by the rule "the one call stays the default where its median lies below the parent chain's minimum": MLP (47.8
    # against 50.4 us on the LunarLander net, 341.7 against 342.1 on [520]) and plane-path cnn (292.0 against 297.8 us at B = 32,
    # 1140.8 against 1144.4 at B = 256) on; general-shape cnn (5386 against 5365 us) and i-IQN (1553.4 against 1551.2 us) off.
    fuse_per_step = True
    fuse_per_family = {"plane": True, "fc": True, "gcnn": False, "iqn": False}

    @staticmethod
    def _general_shape(agent):
        """Whether a cnn agent's handle runs the general-shape conv path: the plane entry said so, or the library's shape rule
        restated (``cnn_fast_shape``, csrc/qnet.hip).  Only the default depends on it: both routes leave the same bytes."""
        if agent.__dict__.get("_replay_fused_ok") is False or os.environ.get("IDQN_CNN_GENERAL", "0") not in ("", "0"):
            return True
        net = getattr(agent, "network", None)
        if net is None:
            return False
        f = list(net.features)
        return not (len(f) == 4 and agent._obs[2] == 4 and min(agent._obs[:2]) >= 8 and net.n_actions <= 32
                    and all(x in (32, 64) for x in f[:3]) and f[3] % 128 == 0 and 128 <= f[3] <= 512)

    def _fused_route(self, defaults=None):
        """``(ring view, family)`` when this step goes through ``idqn_per_learn_on_replay``, else None; read on every call.
        ``defaults``: the per-family switches that apply (``fuse_per_family``; ``steps`` passes ``fuse_per_steps_family``)."""
        from slimdqn.networks.iiqn import iIQN

        defaults = self.fuse_per_family if defaults is None else defaults

        agent, rb = self.agent, self.rb
        if not self.fuse_per_step or os.environ.get("IDQN_PER_FUSED", "1") == "0" or self.__dict__.get("_fused_ok") is False:
            return None
        if rb._batch_size > 256:
            return None
        if isinstance(agent, iIQN):
            view = self._replay_sourced() if type(agent)._learn is iIQN._learn else None
            return (view, "iqn") if view is not None and defaults.get("iqn") else None
        if type(agent)._learn is not DeviceAgent._learn:
            return None
        if agent._arch == "impala":
            return None  # the one-call forms refuse impala handles: the chain, through the agent's replay-sourced entry
        family = "fc" if agent._arch == "fc" else ("gcnn" if self._general_shape(agent) else "plane")
        if not defaults.get(family):
            return None
        if agent._replay_fusable(rb):
            view = rb.ring_view()
            if agent._ring_fusable(view):
                return view, family
        if agent._replay_fc_route(rb):
            view = rb.ring_view()
            if agent._ring_fc_fusable(view):
                return view, family
        return None

    @staticmethod
    def _vp(t):
        return None if t is None else int(t.data_ptr())

    def _fill_sampler_args(self, p, u, leaves, weights, td_abs, priorities):
        """The fields ``_hip.PerStep`` and ``_hip.PerSteps`` have in common, written into ``p``: the tree, the sampler's settings,
        host uniforms ``u`` and the four output tensors."""
        tree, vp = self.sampler._sum_tree, self._vp
        p.nodes_dev, p.depth, p.n_items = vp(tree._nodes_dev), tree._depth, len(self.sampler)
        p.uniforms_host = u.ctypes.data
        p.stratified, p.reduce_max, p.beta, p.eps, p.alpha = self.stratified, self.reduce_max, self.beta, self.eps, self.sampler._alpha
        p.max_priority_dev = vp(self.sampler._max_priority_dev)
        p.leaves_dev, p.weights_dev, p.td_abs_dev, p.priorities_dev = vp(leaves), vp(weights), vp(td_abs), vp(priorities)
        p.tree_scratch_dev = vp(tree._scratch)

    def _step_fused(self, view, u, taus):
        """The library's code for the one-call step on ring ``view`` with uniforms ``u`` (float64 [B], host)."""
        rb, agent = self.rb, self.agent
        B = rb._batch_size
        frames, n_frames, frame_bytes, rows, stack = view[:5]
        if taus is not None:
            agent._upload_fractions(B, taus)
        agent._ensure_handle(B)
        p = self.__dict__.get("_per_args")
        if p is None:
            p = self._per_args = _hip.PerStep()
        self._fill_sampler_args(p, u, self._leaves, self._weights, self._td_abs, self._priorities)
        p.tau_dev = self._vp(agent._tau_dev) if taus is not None else None
        return _hip.lib().idqn_per_learn_on_replay(agent._handle, C.byref(p), _hip.ptr(frames), int(n_frames), int(frame_bytes),
                                                   _hip.ptr(rows), B, int(stack), B, 0, _hip.current_stream())

    def step(self):
        """One prioritized gradient step; returns the per-head losses (device tensor, not synchronised)."""
        rb = self.rb
        B = rb._batch_size
        assert rb.add_count, "No samples in replay buffer!"
        return self.step_with_uniforms(self.sampler._rng_key.random(B))  # the one draw from the sampler's generator, whichever route runs

    def step_with_uniforms(self, u):
        """``step()`` on uniforms ``u`` (float64 [B] in [0, 1)) that the caller has drawn from the sampler's generator already --
        what ``PrioritizedGroupLearner`` runs per member where the group call does not serve."""
        rb, agent = self.rb, self.agent
        B = rb._batch_size
        route, taus = self._fused_route(), None
        if route is not None:
            view, family = route
            taus = agent.sample_fractions(B) if family == "iqn" else None
            rc = self._step_fused(view, u, taus)
            if rc == _hip.E_INVALID and self.__dict__.get("_fused_ok") is None:
                self._fused_ok = False  # not this handle: the chain from now on -- same uniforms (and fractions) for this step
                self.fused_refusal = _hip.lib().idqn_last_error().decode(errors="replace")
            else:
                _hip.check(rc, "idqn_per_learn_on_replay")
                self._fused_ok = True
                if family == "iqn":  # the agent's replay-sourced entry served (the flags its own routes keep)
                    agent._replay_fused_ok = True
                elif family == "fc":
                    agent._replay_fc_ok = True
                return agent._losses
        return self._step_chain(u, taus)

    # n steps as ONE C call per ``MAX_STEPS_PER_CALL`` rows of uniforms (``idqn_per_learn_steps_on_replay``: one upload, k_per_draw,
    # then step / k_per_turn alternating, k_per_write_back), byte-identical to n ``step_with_uniforms`` calls on the same rows.
    # Taken where the one-call step would be (``_fused_route``'s conditions, under ``fuse_per_steps_family`` instead of
    # ``fuse_per_family``; i-IQN agents are not served) for runs of at least ``per_steps_min`` steps at batches of at most
    # ``per_steps_max_batch`` samples; ``IDQN_PER_STEPS=0`` switches
    # it off.  ``_steps_ok`` (unset: not tried; False: the entry refused this handle the first time -- text in ``steps_refusal`` --
    # the rows go through ``step_with_uniforms`` one by one from then on; True: it served).
    # Defaults by the rule "the call is a family's default at the n where its median lies below the minimum of the chain of n
    # ``idqn_per_learn_on_replay`` calls on the same commit" (tools/bench_per_steps.py -> profiles/per_steps.json; B = 32, us per
    # gradient step, call against chain).  n = 1 is SLOWER everywhere (LunarLander net 51.2 against 47.6, [520] 342.9 against
    # 341.6, Atari shape K = 5 277.8 against 277.4): ``per_steps_min`` = 2.  From n = 2 on the call wins: LunarLander net 43.9 /
    # 41.5 / 40.8 / 40.6 at n = 2 / 5 / 10 / 32 against 47.6; [520] 336.6 ... 333.4 against 341.6; Atari shape 272.4 ... 269.5
    # against 277.3: MLP and plane-path cnn on.  General-shape cnn: not measured, off.  k_per_turn alone beats the launch pair at
    # n = 32 (14.4 against 16.1 us) and is SLOWER at n = 256 (61.5 against 31.1 us: 16 descents in turn per wave where k_per_draw
    # spreads them over 64 workgroups), and no whole step was measured past B = 32: ``per_steps_max_batch`` keeps larger batches on
    # the single steps.
    per_steps_min = 2
    per_steps_max_batch = 32
    fuse_per_steps_family = {"plane": True, "fc": True, "gcnn": False}

    def _steps_route(self, n):
        """``(ring view, family)`` when a run of ``n`` steps goes through ``idqn_per_learn_steps_on_replay``, else None."""
        if n < self.per_steps_min or os.environ.get("IDQN_PER_STEPS", "1") == "0" or self.__dict__.get("_steps_ok") is False:
            return None
        if self.rb._batch_size > self.per_steps_max_batch:
            return None
        return self._fused_route(self.fuse_per_steps_family)

    def _ensure_steps_rows(self):
        """The row buffers of the n-step calls (this learner's and ``PrioritizedGroupLearner``'s), one row per step:
        ``(leaves, weights, |TD|, priorities)`` of ``[MAX_STEPS_PER_CALL][...]``, made on first use."""
        rows_out = self.__dict__.get("_steps_rows")
        if rows_out is None:
            import torch

            M, B, K = _hip.MAX_STEPS_PER_CALL, self.rb._batch_size, self.agent._K
            rows_out = self._steps_rows = (torch.empty((M, B), dtype=torch.int32, device="cuda"),
                                           torch.empty((M, B), dtype=torch.float32, device="cuda"),
                                           torch.zeros((M, K, B), dtype=torch.float32, device="cuda"),
                                           torch.empty((M, B), dtype=torch.float64, device="cuda"))
        return rows_out

    def _steps_fused(self, view, U):
        """The library's code for the n-step call on ring ``view`` with uniforms ``U`` (float64 [m][B], host, contiguous)."""
        rb, agent = self.rb, self.agent
        B, m = rb._batch_size, U.shape[0]
        frames, n_frames, frame_bytes, rows, stack = view[:5]
        agent._ensure_handle(B)
        rows_out = self._ensure_steps_rows()
        p = self.__dict__.get("_per_steps_args")
        if p is None:
            p = self._per_steps_args = _hip.PerSteps()
        self._fill_sampler_args(p, U, *rows_out)
        rc = _hip.lib().idqn_per_learn_steps_on_replay(agent._handle, C.byref(p), _hip.ptr(frames), int(n_frames), int(frame_bytes),
                                                       _hip.ptr(rows), m, B, int(stack), B, 0, _hip.current_stream())
        if rc == 0:  # the learner's own buffers are the last step's rows, as m ``step()`` calls leave them
            self._leaves, self._weights, self._td_abs, self._priorities = (t[m - 1] for t in rows_out)
        return rc

    def steps_with_uniforms(self, U):
        """``step_with_uniforms`` on every row of ``U`` (float64 [n][B] in [0, 1)), in order; returns the per-head losses of the
        last step (device tensor, not synchronised).  Every row goes through exactly one route."""
        U = np.ascontiguousarray(U, np.float64)
        n, i = U.shape[0], 0
        route = self._steps_route(n)
        while route is not None and i < n:
            m = min(_hip.MAX_STEPS_PER_CALL, n - i)
            rc = self._steps_fused(route[0], U[i : i + m])
            if rc == _hip.E_INVALID and self.__dict__.get("_steps_ok") is None:
                self._steps_ok = False  # not this handle: single steps from now on -- the same rows, nothing more drawn
                self.steps_refusal = _hip.lib().idqn_last_error().decode(errors="replace")
                break
            _hip.check(rc, "idqn_per_learn_steps_on_replay")
            self._steps_ok = True
            if route[1] == "fc":  # the agent's replay-sourced entry served (the flag its own routes keep)
                self.agent._replay_fc_ok = True
            i += m
        for u in U[i:]:
            self.step_with_uniforms(u)
        return self.agent._losses

    def steps(self, n):
        """``n`` prioritized gradient steps: the sampler's generator is drawn n times first, in order -- the state n ``step()``
        calls leave (a prioritized draw takes uniforms only, so it does not depend on the steps between) -- then the steps run,
        as one call where ``steps_with_uniforms`` allows it."""
        n = int(n)
        if n <= 0:
            return self.agent._losses
        assert self.rb.add_count, "No samples in replay buffer!"
        B = self.rb._batch_size
        return self.steps_with_uniforms(np.stack([self.sampler._rng_key.random(B) for _ in range(n)]))

    def update_params_many(self, first_step, n_steps):
        """``[(step, logs)]`` of the target updates of the loop ``if s % update_to_data == 0: step(); update_target_params(s)``
        over ``n_steps`` steps from ``first_step``, with the same effect and order: ``plan_step_runs`` with the agent's schedule,
        every run's gradient steps through ``steps``, the target operation the agent's own.  The losses reach the agent's
        ``cumulated_losses`` as ``step()`` adds them: on the device, inside the step."""
        agent, out = self.agent, []
        for n_grad, op, last in plan_step_runs(first_step, n_steps, agent.update_to_data, agent.target_update_frequency,
                                               getattr(agent, "target_sync_frequency", None)):
            self.steps(n_grad)
            if op is not None:
                updated, logs = agent.update_target_params(last)
                if updated:
                    out.append((last, logs))
        return out

    def _step_chain(self, u, taus=None):
        """The step as a chain of calls on uniforms ``u`` (and, for an i-IQN agent, fractions ``taus`` already drawn)."""
        import torch

        lib, q = _hip.lib(), _hip.current_stream()
        rb, tree, agent = self.rb, self.sampler._sum_tree, self.agent
        B = rb._batch_size
        if self._u_ev is not None:
            self._u_ev.synchronize()  # the previous step's upload has left the pinned staging buffer
        self._u_pin.copy_(torch.from_numpy(u))
        self._u_dev.copy_(self._u_pin, non_blocking=True)
        self._u_ev = torch.cuda.Event()
        self._u_ev.record()
        _hip.check(lib.per_sample_leaves(_hip.ptr(tree._nodes_dev), tree._depth, _hip.ptr(self._u_dev), B, self.stratified,
                                         _hip.ptr(self._leaves), q), "per_sample_leaves")
        _hip.check(lib.per_importance_weights(_hip.ptr(tree._nodes_dev), tree._depth, _hip.ptr(self._leaves), B,
                                              len(self.sampler), self.beta, _hip.ptr(self._weights), q),
                   "per_importance_weights")
        # i-IQN on a fused-capable buffer: the leaves (== replay slots, already in device memory) go to the replay-sourced step
        view = self._replay_sourced()
        # ... and so do those of an MLP / general-shape cnn agent (DeviceAgent._learn_on_replay_fc, its own flag and switches)
        fc_route = view is None and type(agent)._learn is DeviceAgent._learn and agent._replay_fc_route(rb)
        batch = rb._gather_device(self._leaves) if view is None and not fc_route else None
        agent._ensure_handle(B)
        _hip.check(lib.idqn_set_per_buffers(agent._handle, _hip.ptr(self._weights), _hip.ptr(self._td_abs)),
                   "idqn_set_per_buffers")
        try:
            if fc_route:
                losses = agent._learn_on_replay_fc(rb, rb.ring_view(), slots_dev=self._leaves,
                                                   gather=lambda: rb._gather_device(self._leaves))
            elif view is None:
                losses = agent._learn(batch)
            else:
                taus = agent.sample_fractions(B) if taus is None else taus
                rc = agent._learn_on_replay(view, slots_dev=self._leaves, taus=taus)
                if rc == _hip.E_INVALID and agent.__dict__.get("_replay_fused_ok") is None:
                    agent._replay_fused_ok = False  # another conv path: gathered steps from now on, same leaves and fractions
                    losses = agent._learn(rb._gather_device(self._leaves), taus=taus)
                else:
                    _hip.check(rc, "idqn_iqn_learn_on_replay_dev")
                    agent._replay_fused_ok = True
                    losses = agent._losses
        finally:
            _hip.check(lib.idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
        _hip.check(lib.per_priorities_from_td(_hip.ptr(self._td_abs), agent._K, B, self.reduce_max, self.eps,
                                              self.sampler._alpha, _hip.ptr(self._priorities),
                                              _hip.ptr(self.sampler._max_priority_dev), q), "per_priorities_from_td")
        _hip.check(lib.sumtree_set(_hip.ptr(tree._nodes_dev), tree._depth, _hip.ptr(self._leaves),
                                   _hip.ptr(self._priorities), B, _hip.ptr(tree._scratch), q), "sumtree_set")
        return losses


class PrioritizedGroupLearner:
    """``PrioritizedLearner.step`` for every member of an ``AgentGroup`` at once: one ``idqn_group_per_learn_on_replay_fc`` call
    (S draws and weights, the group step on the leaves, S write-backs: three launches) leaves on every member, its tree and
    its learner's buffers the bytes the member's own ``PrioritizedLearner.step`` leaves.

    It owns one ``PrioritizedLearner`` per member: they supply the buffers and the fallback.  ``step()`` draws every member's
    uniforms from the member's own sampler generator, once per member, in member order, whichever route runs -- a member's
    sampler stream is what it would be alone.  The group call is taken when the group is stock (``AgentGroup._stock``), every
    member's ring serves the replay-sourced MLP step, B <= 32, the group's size is in ``group_per_sizes`` and
    ``IDQN_PER_FUSED`` is not 0; otherwise every member's own learner steps on the uniforms already drawn.
    ``_group_per_ok`` (unset: not tried; False: the entry refused these members the first time -- text in
    ``group_per_refusal`` -- the members' own steps from then on; True: it served)."""

    # The sizes S at which the group call is taken by default: those where its median lay below the minimum of the S solo
    # steps (tools/bench_group_per.py -> profiles/group_per.json), the rule of ``AgentGroup.group_sizes``.  LunarLander net,
    # B = 32, us per step of all members: S = 1 50.7 against 48.1 (SLOWER: a group of one runs its member's own step),
    # S = 2 52.7 against 95.6, 4 52.5 against 191.5, 8 67.2 against 384.7, 16 115.0 against 779.1, 32 207.2 against 1562.1.
    group_per_sizes = frozenset(range(2, 33))

    def __init__(self, group, replay_buffers, beta: float = 0.4, eps: float = 1e-6, reduce: str = "mean", stratified: bool = True):
        rbs = list(replay_buffers)
        assert len(rbs) == len(group.agents)
        per_member = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * len(rbs)  # noqa: E731
        self.group, self.rbs = group, rbs
        self.learners = [PrioritizedLearner(a, rb, beta=b, eps=e, reduce=r, stratified=s) for a, rb, b, e, r, s in
                         zip(group.agents, rbs, per_member(beta), per_member(eps), per_member(reduce), per_member(stratified))]

    def _group_route(self, sizes=None):
        """The members' ring views when this step goes through the group call, else None; read on every call.  ``sizes``: the
        size set that applies (``group_per_sizes``; ``steps`` passes ``group_per_steps_sizes``)."""
        group = self.group
        if os.environ.get("IDQN_PER_FUSED", "1") == "0" or self.__dict__.get("_group_per_ok") is False:
            return None
        if len(group.agents) not in (self.group_per_sizes if sizes is None else sizes) or not group._stock():
            return None
        if len({rb._batch_size for rb in self.rbs}) != 1 or self.rbs[0]._batch_size > 32:
            return None
        if not all(a._replay_fc_route(rb) for a, rb in zip(group.agents, self.rbs)):
            return None
        views = [rb.ring_view() for rb in self.rbs]
        return views if all(a._ring_fc_fusable(v) for a, v in zip(group.agents, views)) else None

    def _step_group(self, views, us):
        """The library's code for the group call on ring ``views`` with uniforms ``us`` ([S] float64 arrays of [B], host), or
        None when ``idqn_group_create`` refused the members."""
        B = self.rbs[0]._batch_size
        g = self.group._ensure_group(B)
        if g is None:
            return None
        per = self.__dict__.get("_per_args")
        if per is None:
            per = self._per_args = (_hip.PerStep * len(self.learners))()
        for p, lr, u in zip(per, self.learners, us):
            lr._fill_sampler_args(p, u, lr._leaves, lr._weights, lr._td_abs, lr._priorities)
            p.tau_dev = None
        return _hip.lib().idqn_group_per_learn_on_replay_fc(g, self.group._rings(views), per, B, B, 0, _hip.current_stream())

    def step(self):
        """One prioritized gradient step of every member; returns the members' per-head losses (device tensors, not
        synchronised)."""
        for rb in self.rbs:
            assert rb.add_count, "No samples in replay buffer!"
        return self.step_with_uniforms([lr.sampler._rng_key.random(lr.rb._batch_size) for lr in self.learners])  # member order

    def step_with_uniforms(self, us):
        """``step()`` on uniforms ``us`` ([S] float64 arrays of [B] in [0, 1)) that the caller has drawn from the members' sampler
        generators already -- what ``steps_with_uniforms`` runs per row where the n-step group call does not serve."""
        us = [np.ascontiguousarray(u, np.float64) for u in us]
        views = self._group_route()
        if views is not None:
            rc = self._step_group(views, us)
            if rc is None or (rc == _hip.E_INVALID and self.__dict__.get("_group_per_ok") is None):
                self._group_per_ok = False  # not these members: their own steps from now on -- same uniforms for this step
                self.group_per_refusal = "idqn_group_create refused the members" if rc is None else \
                    _hip.lib().idqn_last_error().decode(errors="replace")
            else:
                _hip.check(rc, "idqn_group_per_learn_on_replay_fc")
                self._group_per_ok = True
                for a in self.group.agents:
                    a._replay_fc_ok = True
                return [a._losses for a in self.group.agents]
        return [lr.step_with_uniforms(u) for lr, u in zip(self.learners, us)]

    # n steps of every member as ONE C call per ``MAX_STEPS_PER_CALL`` rows (``idqn_group_per_learn_steps_on_replay_fc``: one
    # upload, k_per_group_draw, then the group step / k_per_group_turn alternating, k_per_group_write_back), byte-identical per
    # member to n ``step_with_uniforms`` calls on the same rows.  Taken under ``_group_route``'s conditions with the size set
    # ``group_per_steps_sizes`` for runs of at least ``group_per_steps_min`` steps; ``IDQN_PER_STEPS=0`` switches it off.
    # ``_group_per_steps_ok`` (unset: not tried; False: the entry refused these members the first time -- text in
    # ``group_per_steps_refusal`` -- the rows go through ``step_with_uniforms`` one by one from then on; True: it served).
    # Defaults by the standing rule "a size (S, n) is on only where the call's median lies below the minimum of the chain of n
    # ``idqn_group_per_learn_on_replay_fc`` calls on the same commit" (tools/bench_group_per_steps.py ->
    # profiles/group_per_steps.json; LunarLander net, B = 32, us per gradient step of all S members, call against chain).  n = 1
    # is SLOWER at every S >= 2 (S = 2 51.3 against 50.0, 8 111.7 against 66.8, 32 378.2 against 211.1: the same launches behind
    # more host work per call): ``group_per_steps_min`` = 2.  From n = 2 on the call wins at every measured S: S = 2 45.8 / 43.2 /
    # 42.5 / 43.9 at n = 2 / 5 / 8 / 32 against 49.8; S = 4 46.5 ... 43.9 against 49.8; S = 8 62.5 ... 46.5 against 66.2; S = 16
    # 106.3 ... 50.3 against 112.9; S = 32 199.3 / 96.6 / 71.0 / 54.1 against 206.5 ... 209.0.  Sizes that were not measured stay
    # off; S = 1 is no group (``AgentGroup._stock``).
    group_per_steps_sizes = frozenset({2, 4, 8, 16, 32})
    group_per_steps_min = 2

    def _group_steps_route(self, n):
        """The members' ring views when a run of ``n`` steps goes through the n-step group call, else None."""
        if n < self.group_per_steps_min or os.environ.get("IDQN_PER_STEPS", "1") == "0" or self.__dict__.get("_group_per_steps_ok") is False:
            return None
        return self._group_route(self.group_per_steps_sizes)

    def _steps_group(self, views, Us):
        """The library's code for the n-step group call on ring ``views`` with uniforms ``Us`` ([S] float64 arrays of [m][B],
        host, contiguous), or None when ``idqn_group_create`` refused the members."""
        B, m = self.rbs[0]._batch_size, Us[0].shape[0]
        g = self.group._ensure_group(B)
        if g is None:
            return None
        per = self.__dict__.get("_per_steps_args")
        if per is None:
            per = self._per_steps_args = (_hip.PerSteps * len(self.learners))()
        rows = [lr._ensure_steps_rows() for lr in self.learners]
        for p, lr, U, r in zip(per, self.learners, Us, rows):
            lr._fill_sampler_args(p, U, *r)
        rc = _hip.lib().idqn_group_per_learn_steps_on_replay_fc(g, self.group._rings(views), per, m, B, B, 0, _hip.current_stream())
        if rc == 0:  # the member learners' own buffers are the last step's rows, as m ``step()`` calls leave them
            for lr, r in zip(self.learners, rows):
                lr._leaves, lr._weights, lr._td_abs, lr._priorities = (t[m - 1] for t in r)
        return rc

    def steps_with_uniforms(self, Us):
        """``step_with_uniforms`` on every row of ``Us`` ([S] float64 arrays of [n][B] in [0, 1)), in order; returns the members'
        per-head losses of the last step.  Every row goes through exactly one route."""
        Us = [np.ascontiguousarray(U, np.float64) for U in Us]
        n, i = Us[0].shape[0], 0
        views = self._group_steps_route(n)
        while views is not None and i < n:
            m = min(_hip.MAX_STEPS_PER_CALL, n - i)
            rc = self._steps_group(views, [U[i : i + m] for U in Us])
            if rc is None or (rc == _hip.E_INVALID and self.__dict__.get("_group_per_steps_ok") is None):
                self._group_per_steps_ok = False  # not these members: single steps from now on -- the same rows, nothing more drawn
                self.group_per_steps_refusal = "idqn_group_create refused the members" if rc is None else \
                    _hip.lib().idqn_last_error().decode(errors="replace")
                break
            _hip.check(rc, "idqn_group_per_learn_steps_on_replay_fc")
            self._group_per_steps_ok = True
            for a in self.group.agents:
                a._replay_fc_ok = True
            i += m
        for j in range(i, n):
            self.step_with_uniforms([U[j] for U in Us])
        return [a._losses for a in self.group.agents]

    def steps(self, n):
        """``n`` prioritized gradient steps of every member: every member's sampler generator is drawn n times first, member by
        member -- the state n ``step()`` calls leave, since a member's generator is its own -- then the steps run, as one call
        where ``steps_with_uniforms`` allows it."""
        n = int(n)
        if n <= 0:
            return [a._losses for a in self.group.agents]
        for rb in self.rbs:
            assert rb.add_count, "No samples in replay buffer!"
        return self.steps_with_uniforms([np.stack([lr.sampler._rng_key.random(lr.rb._batch_size) for _ in range(n)]) for lr in self.learners])

    def update_params_many(self, first_step, n_steps):
        """Per member ``[(step, logs)]`` of the target updates of the loop ``if s % update_to_data == 0: step();
        update_target_params(s)`` over ``n_steps`` steps from ``first_step``, as ``AgentGroup.update_params_many`` runs it: one
        ``plan_step_runs`` on the shared schedule, every run's gradient steps through ``steps``, the target operations the
        members' own.  Members whose schedules differ, or a group that is not stock: every member learner's own
        ``update_params_many``."""
        agents = self.group.agents
        schedule = lambda a: (a.update_to_data, a.target_update_frequency, getattr(a, "target_sync_frequency", None))  # noqa: E731
        if not self.group._stock() or any(schedule(a) != schedule(agents[0]) for a in agents):
            return [lr.update_params_many(first_step, n_steps) for lr in self.learners]
        out = [[] for _ in agents]
        for n_grad, op, last in plan_step_runs(first_step, n_steps, *schedule(agents[0])):
            self.steps(n_grad)
            if op is not None:
                for o, a in zip(out, agents):
                    updated, logs = a.update_target_params(last)
                    if updated:
                        o.append((last, logs))
        return out
