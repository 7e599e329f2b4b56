"""Device state shared by ``iDQN`` and ``DQN``: parameter arenas in HBM + the C-ABI handle.

All arithmetic of the gradient step runs in ``libidqn_hip.so``; torch tensors are storage.
Arenas are ``[K][head_stride]`` float32; ``params`` / ``target_params`` / ``optimizer_state`` are
pytrees of VIEWS into them with the flax leaf names of the reference
(``{"params": {"Conv_0": {"kernel", "bias"}, ...}}``, leading K axis for iDQN -- idqn.py:48-50).
"""
import ctypes as C

import os

import numpy as np
import torch

from slimdqn import _hip, prng
from slimdqn.networks.architectures.dqn import DQNNet
from slimdqn.networks.architectures.impala import ImpalaNet

PIXEL_ARCHS = ("cnn", "impala")  # uint8 (H, W, C) states; everything else is a flat float32 vector


def _obs_triplet(observation_dim, arch):
    if isinstance(observation_dim, (int, np.integer)):
        return (int(observation_dim), 1, 1)
    dims = tuple(int(d) for d in observation_dim)
    if arch in PIXEL_ARCHS:
        assert len(dims) == 3, f"{arch} expects observation_dim = (H, W, C)"
        return dims
    return (int(np.prod(dims)), 1, 1)


def plan_step_runs(first_step, n_steps, update_to_data, target_update_frequency, target_sync_frequency=None):
    """Cuts the steps ``first_step .. first_step + n_steps - 1`` of the loop ``update_online_params(s, rb);
    update_target_params(s)`` into runs ``(n_gradient_steps, target_op, last_step)``: the gradient steps of a run (steps with
    ``s % update_to_data == 0``) may be issued together, then the target operation due at the run's last step -- ``"update"``
    (``s % target_update_frequency == 0``), ``"sync"`` (``s % target_sync_frequency == 0`` on a step that is no update;
    ``None`` for ``DQN``, which has no sync) or ``None`` at the end of the range.  Replaying the runs in order is the loop.
    ``update_to_data`` may be a float, as the parser passes it.  Pure host arithmetic."""
    runs, n_grad = [], 0
    for s in range(int(first_step), int(first_step) + int(n_steps)):
        if s % update_to_data == 0:
            n_grad += 1
        op = None
        if s % target_update_frequency == 0:
            op = "update"
        elif target_sync_frequency is not None and s % target_sync_frequency == 0:
            op = "sync"
        if op is not None:
            runs.append((n_grad, op, s))
            n_grad = 0
    if n_grad:
        runs.append((n_grad, None, int(first_step) + int(n_steps) - 1))
    return runs


class _HostAction(int):
    """The greedy action as a host integer that still answers ``.item()`` like the device scalar the reference returns
    (``select_action`` calls ``.item()`` on it, slimdqn/sample_collection/utils.py:21)."""

    def item(self):
        return int(self)


class _PendingHostAction:
    """A greedy action whose launch is in flight (``idqn_act_host_begin``): ``.item()`` waits for it.  The trainer's
    ``collect_single_sample`` runs the replay bookkeeping of the previous transition between the two."""

    __slots__ = ("_agent", "_value")

    def __init__(self, agent):
        self._agent, self._value = agent, None

    def item(self):
        if self._value is None:
            a = self._agent
            try:
                _hip.check(_hip.lib().idqn_act_host_end(a._handle, C.c_void_p(a._act_out.data_ptr()), _hip.current_stream()),
                           "idqn_act_host_end")
                self._value = int(a._act_out_np[0])
            finally:  # the library has dropped its pending launch either way: a failure must not wedge every later call
                a._act_in_flight = None
        return self._value

    __int__ = __index__ = item


class DeviceAgent:
    lazy_host_actions = False  # True (the trainer of this build sets it): best_action on a host state returns a pending action
    # n for which an impala agent's ``_best_actions`` asks idqn_act_host_many_impala: the sizes whose one call measured a median
    # below the MINIMUM of the loop of n idqn_act_host calls, on both shapes and both head assignments
    # (tools/bench_impala_act_many.py -> profiles/impala_act_many.json).  Sizes that lost and sizes not measured stay on the loop.
    act_many_imp_sizes = frozenset({1, 2, 3, 4, 8, 16, 32})

    def __init__(self, key, observation_dim, n_actions, n_heads, features, architecture_type, learning_rate, gamma,
                 update_horizon, adam_eps, stacked, init_heads=None):
        self.network = (ImpalaNet(features, n_actions) if architecture_type == "impala"
                        else DQNNet(features, architecture_type, n_actions))
        self._K = int(n_heads)
        self._stacked = stacked  # iDQN leaves carry a leading K axis, DQN leaves do not
        self._arch = architecture_type
        self._pixels = architecture_type in PIXEL_ARCHS
        self._obs = _obs_triplet(observation_dim, architecture_type)
        self._lr, self._eps = float(learning_rate), float(adam_eps)
        self.gamma, self.update_horizon = gamma, update_horizon
        self._gamma_n = float(gamma) ** update_horizon  # a Python double, folded like idqn.py:122
        _hip.lib()  # fail loudly (HipExtensionError) before any allocation if the extension is missing
        if not torch.cuda.is_available():
            raise _hip.HipExtensionError("no HIP device visible: the i-DQN step has no CPU path")
        self._leaves, self._P = _hip.layout(self._config(32))
        K, P = self._K, self._P
        dev = "cuda"
        self._online = torch.zeros((K, P), dtype=torch.float32, device=dev)
        self._target = torch.zeros((K, P), dtype=torch.float32, device=dev)
        self._mu = torch.zeros((K, P), dtype=torch.float32, device=dev)
        self._nu = torch.zeros((K, P), dtype=torch.float32, device=dev)
        # gradient arena (include/idqn_hip.h): [K][gP] small leaves | 64 reserved floats (the K losses live there, so
        # that one collective covers them) | [K][w0n] Dense_0/kernel gradients of the cnn
        names = [n for n, _, _ in self._leaves]
        self._w0 = (0, 0)
        if architecture_type == "cnn":  # (impala: one region, like fc)
            i = names.index("Dense_0/kernel")
            self._w0 = (self._leaves[i][1], self._leaves[i + 1][1])
        self._gP = P - (self._w0[1] - self._w0[0])
        self._grad = torch.zeros(K * P + 64, dtype=torch.float32, device=dev)
        self._grad_small = self._grad[: K * self._gP + 64]
        self._grad_w0 = self._grad[K * self._gP + 64 :]
        self._losses = self._grad[K * self._gP : K * self._gP + K]
        self._losses_in_grad = True
        self._count = torch.zeros(K, dtype=torch.int32, device=dev)
        self._cum = torch.zeros(K, dtype=torch.float64, device=dev)
        self._handle, self._handle_batch = None, 0
        self._q_out = torch.zeros((32, n_actions), dtype=torch.float32, device=dev)
        # initial parameters (idqn.py:48-50 / dqn.py:29); target starts equal to online (idqn.py:56)
        rng = prng.generator(key)
        # init_heads = (K_global, first): this agent holds heads [first, first + K) of a K_global-head i-DQN and must
        # start from exactly the parameters the single-device agent gives those heads (head-parallel mode)
        k_all, first = init_heads if init_heads is not None else (K, 0)
        host = np.zeros((K, P), np.float32)
        for name, off, shape in self._leaves:
            leaf = self.network.init_leaf(rng, name, shape, k_all).reshape(k_all, -1)
            host[:, off : off + int(np.prod(shape))] = leaf[first : first + K]
        self._online.copy_(torch.from_numpy(host))
        self._target.copy_(self._online)
        self.params = self._tree(self._online)
        self.target_params = self._tree(self._target)
        self.optimizer_state = {"mu": self._tree(self._mu), "nu": self._tree(self._nu), "count": self._count}

    # ---- plumbing ----------------------------------------------------------------------------------
    def _config(self, max_batch):
        return _hip.make_config(self._arch, self._K, self.network.n_actions, self._obs, self.network.features,
                                max_batch, self._lr, self._eps, self._gamma_n,
                                n_quantiles=getattr(self, "_n_quantiles", 0))  # > 0: i-IQN heads (slimdqn/networks/iiqn.py)

    def _tree(self, arena):
        tree = {}
        for name, off, shape in self._leaves:
            *mods, leaf = name.split("/")  # "Conv_0/kernel", or "Stack_0/Conv_0/kernel": nested as flax nests submodules
            view = arena[:, off : off + int(np.prod(shape))].view((self._K,) + tuple(shape))
            node = tree
            for mod in mods:
                node = node.setdefault(mod, {})
            node[leaf] = view if self._stacked else view[0]
        return {"params": tree}

    def _ensure_handle(self, batch):
        if self._handle is not None and batch <= self._handle_batch:
            return
        self._destroy_handle()
        cfg = self._config(max(batch, 32))
        h = C.c_void_p()
        _hip.check(_hip.lib().idqn_create(C.byref(cfg), _hip.ptr(self._online), _hip.ptr(self._target),
                                          _hip.ptr(self._mu), _hip.ptr(self._nu), _hip.ptr(self._grad),
                                          _hip.ptr(self._count), _hip.ptr(self._losses), _hip.ptr(self._cum),
                                          C.byref(h)), "idqn_create")
        self._handle, self._handle_batch = h, max(batch, 32)

    def _destroy_handle(self):
        pending = getattr(self, "_act_in_flight", None)
        if pending is not None and getattr(self, "_handle", None) is not None:  # collect before the handle goes away
            try:
                pending.item()
            except Exception:
                self._act_in_flight = None
        dp = self.__dict__.pop("_dp", None)  # (slimdqn/networks/parallel.py: the RCCL side of this handle goes first)
        if dp is not None:
            _hip.lib().idqn_dp_destroy(dp[0])
        if getattr(self, "_handle", None) is not None:
            _hip.lib().idqn_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy_handle()
        except Exception:
            pass

    @staticmethod
    def _dev(x, dtype):
        t = getattr(x, "tensor", x)
        if not isinstance(t, torch.Tensor):
            a = np.ascontiguousarray(np.asarray(t))
            t = torch.from_numpy(a if a.flags.writeable else a.copy())  # (a read-only view, e.g. an environment's state table)
        return t.to(device="cuda", dtype=dtype).contiguous()

    # ---- the step ------------------------------------------------------------------------------------
    def _prepare(self, batch):
        """``(B, pointers)`` of a ReplayElement-like batch on the device: state, next_state, action, reward, terminal."""
        # The replay buffer hands out the SAME ReplayElement object (views of a staging set) every other sample: its
        # converted tensors and argument pointers are kept per object (a handful of entries; the entry holds the object).
        cache = self.__dict__.setdefault("_learn_cache", {})
        hit = cache.get(id(batch))
        if hit is not None and hit[0] is batch and self._handle is not None and hit[1] <= self._handle_batch:
            return hit[1], hit[2]
        if self._pixels:
            s, s2 = self._dev(batch.state, torch.uint8), self._dev(batch.next_state, torch.uint8)
            assert tuple(s.shape[1:]) == self._obs, f"state shape {tuple(s.shape)} vs observation_dim {self._obs}"
        else:
            s, s2 = self._dev(batch.state, torch.float32), self._dev(batch.next_state, torch.float32)
            assert int(np.prod(s.shape[1:])) == self._obs[0], f"state shape {tuple(s.shape)} vs dim {self._obs[0]}"
        B = int(s.shape[0])
        a = self._dev(batch.action, torch.int32)
        r = self._dev(batch.reward, torch.float32)
        t = self._dev(batch.is_terminal, torch.uint8)
        assert a.numel() == B and r.numel() == B and t.numel() == B
        self._ensure_handle(B)
        self._keep = (s, s2, a, r, t)  # keep inputs alive until the stream has consumed them
        ptrs = (_hip.ptr(s), _hip.ptr(s2), _hip.ptr(a), _hip.ptr(r), _hip.ptr(t))
        if type(batch).__name__ == "ReplayElement" and all(hasattr(f, "tensor") for f in (batch.state, batch.action)):
            if len(cache) >= 8:
                cache.clear()
            if all(x.data_ptr() == getattr(f, "tensor", f).data_ptr() for x, f in
                   ((s, batch.state), (s2, batch.next_state), (a, batch.action), (r, batch.reward), (t, batch.is_terminal))):
                cache[id(batch)] = (batch, B, ptrs)
        return B, ptrs

    def _learn(self, batch, flags=0, mean_divisor=None):
        """One gradient step on a ReplayElement-like batch; returns the per-head losses (device, [K])."""
        B, ptrs = self._prepare(batch)
        _hip.check(_hip.lib().idqn_learn_on_batch(self._handle, *ptrs, B, int(mean_divisor or B), int(flags),
                                                  _hip.current_stream()), "idqn_learn_on_batch")
        return self._losses

    # ``update_online_params`` = ``replay_buffer.sample()`` + ``learn_on_batch`` (idqn.py:65-72, dqn.py:41-47).  On this package's
    # ReplayBuffer with Atari-shaped uint8 frames the two halves are ONE C call (``idqn_learn_on_replay``): the sampler draws the
    # same keys from the same generator, the stacked gather happens inside the step's staging launch and the minibatch is never
    # materialised.  MLP agents and the general-shape cnn take ``idqn_learn_on_replay_fc`` the same way (below).  Anything else
    # (other buffers, other frame dtypes, the f32 conv mode) samples, gathers and learns as two calls.
    fuse_replay_sampling = True

    def _replay_fusable(self, rb):
        """Buffer-side conditions of the replay-sourced step (the ring's shape is checked once the slots are drawn:
        ``_ring_fusable``); read on every call, the environment switch included."""
        return (self.fuse_replay_sampling and self._arch == "cnn" and hasattr(rb, "sample_slots") and hasattr(rb, "ring_view")
                and getattr(self, "_replay_fused_ok", True) and rb._batch_size <= 256 and os.environ.get("IDQN_LEARN_ON_REPLAY", "1") != "0")

    def _ring_fusable(self, ring_view):
        _, _, frame_bytes, _, stack, fshape, fdt = ring_view
        return (stack == 4 and self._obs[2] == 4 and tuple(fshape) == tuple(self._obs[:2]) and np.dtype(fdt) == np.uint8
                and frame_bytes % 16 == 0)

    # MLP ("fc") agents, and cnn agents whose handle the plane entry refused (the general shapes), take the same one-call route
    # through ``idqn_learn_on_replay_fc`` under a flag of their own, ``_replay_fc_ok`` (unset: not tried yet; False: this handle or
    # this buffer's ring is outside the entry's domain, gather and learn from then on; True: it served).
    def _replay_fc_route(self, rb):
        """Buffer-side conditions of ``idqn_learn_on_replay_fc``, read on every call (the switches included)."""
        return (self.fuse_replay_sampling and hasattr(rb, "sample_slots") and hasattr(rb, "ring_view")
                and getattr(self, "_replay_fc_ok", True) and os.environ.get("IDQN_LEARN_ON_REPLAY", "1") != "0"
                and (self._arch in ("fc", "impala") or (self._arch == "cnn" and self.__dict__.get("_replay_fused_ok") is False)))

    def _ring_fc_fusable(self, ring_view):
        _, _, frame_bytes, _, stack, fshape, fdt = ring_view
        if self._arch == "fc":
            return (np.dtype(fdt) == np.float32 and 1 <= stack <= 8 and int(np.prod(fshape, dtype=np.int64)) * stack == self._obs[0]
                    and frame_bytes * stack == 4 * self._obs[0])
        return np.dtype(fdt) == np.uint8 and tuple(fshape) == tuple(self._obs[:2]) and stack == self._obs[2]

    def _learn_on_replay_fc(self, rb, view, slots=None, slots_dev=None, gather=None):
        """One step through ``idqn_learn_on_replay_fc`` (host ``slots``) or ``_dev`` (``slots_dev``); ``gather()`` is the batch
        of the same slots for the two-call form this falls back to when the entry answers "not this handle" the first time."""
        frames, n_frames, frame_bytes, rows, stack = view[:5]
        if not self._ring_fc_fusable(view):
            self._replay_fc_ok = False
            return self._learn(gather())
        B = int(slots.size if slots_dev is None else slots_dev.numel())
        self._ensure_handle(B)
        lib = _hip.lib()
        if slots_dev is None:
            name = "idqn_learn_on_replay_fc"
            rc = lib.idqn_learn_on_replay_fc(self._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                             slots.ctypes.data, B, int(stack), B, 0, _hip.current_stream())
        else:
            name = "idqn_learn_on_replay_fc_dev"
            rc = lib.idqn_learn_on_replay_fc_dev(self._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                 _hip.ptr(slots_dev), B, int(stack), B, 0, _hip.current_stream())
        if rc == _hip.E_INVALID and self.__dict__.get("_replay_fc_ok") is None:
            self._replay_fc_ok = False  # not this handle (the f32 conv mode, ...): same slots, two calls, from now on
            return self._learn(gather())
        _hip.check(rc, name)
        self._replay_fc_ok = True
        return self._losses

    def _sample_and_learn(self, replay_buffer):
        rb = replay_buffer
        if type(self)._learn is not DeviceAgent._learn:
            return self._learn(rb.sample())
        if self._replay_fusable(rb):
            slots = rb.sample_slots()
            frames, n_frames, frame_bytes, rows, stack, fshape, fdt = view = rb.ring_view()
            if not self._ring_fusable(view):
                self._replay_fused_ok = False
            else:
                B = int(slots.size)
                self._ensure_handle(B)
                slots = np.ascontiguousarray(slots, np.int32)
                rc = _hip.lib().idqn_learn_on_replay(self._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                     slots.ctypes.data, B, int(stack), B, 0, _hip.current_stream())
                if rc == _hip.E_INVALID and self.__dict__.get("_replay_fused_ok") is None:
                    # this handle runs another conv path (IDQN_CONV=f32 / the general shapes): not the plane entry, from now on
                    self._replay_fused_ok = False
                else:
                    _hip.check(rc, "idqn_learn_on_replay")
                    self._replay_fused_ok = True
                    return self._losses
            if not self._replay_fc_route(rb):
                return self._learn(rb._gather(slots))
        elif self._replay_fc_route(rb):
            slots = rb.sample_slots()
            view = rb.ring_view()
        else:
            return self._learn(rb.sample())
        slots = np.ascontiguousarray(slots, np.int32)
        return self._learn_on_replay_fc(rb, view, slots=slots, gather=lambda: rb._gather(slots))

    # n gradient steps of ``update_online_params`` as one C call per ``MAX_STEPS_PER_CALL`` draws (``idqn_learn_steps_on_replay_fc``):
    # the sampler is drawn n times first -- a uniform sampler's draws do not depend on the learner, so these are the generator
    # draws of n ``_sample_and_learn`` calls -- and the library runs the steps back to back, MLP nets of the one-launch step inside
    # one launch.  Flag ``_learn_steps_ok`` (unset: not tried; False: the entry refused this handle / ring, single steps on the
    # slots already drawn from then on).
    learn_steps_min = 5  # fewer steps than this go one by one: the call's slot staging costs more than it saves (profiles/fc_learn_steps.json)

    def _sample_and_learn_many(self, rb, n):
        n = int(n)
        if n <= 0:
            return self._losses
        if (type(self)._learn is not DeviceAgent._learn or type(self)._sample_and_learn is not DeviceAgent._sample_and_learn
                or not self._replay_fc_route(rb) or n < self.learn_steps_min):
            for _ in range(n):
                self._sample_and_learn(rb)
            return self._losses
        draws = [np.ascontiguousarray(rb.sample_slots(), np.int32) for _ in range(n)]
        view = rb.ring_view()
        frames, n_frames, frame_bytes, rows, stack = view[:5]
        B = int(draws[0].size)
        i = 0
        while i < n and getattr(self, "_learn_steps_ok", True) and self._ring_fc_fusable(view) and all(d.size == B for d in draws):
            m = min(_hip.MAX_STEPS_PER_CALL, n - i)
            block = np.ascontiguousarray(np.stack(draws[i : i + m]), np.int32)
            self._ensure_handle(B)
            rc = _hip.lib().idqn_learn_steps_on_replay_fc(self._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                          block.ctypes.data, m, B, int(stack), B, 0, _hip.current_stream())
            if rc == _hip.E_INVALID and self.__dict__.get("_learn_steps_ok") is None:
                self._learn_steps_ok = False  # not this handle: the drawn slots go through the single step, one set at a time
                break
            _hip.check(rc, "idqn_learn_steps_on_replay_fc")
            self._learn_steps_ok = True
            self._replay_fc_ok = True
            i += m
        for slots in draws[i:]:
            if self._replay_fc_route(rb):
                self._learn_on_replay_fc(rb, view, slots=slots, gather=lambda slots=slots: rb._gather(slots))
            else:
                self._learn(rb._gather(slots))
        return self._losses

    def _update_params_many(self, base, first_step, n_steps, replay_buffer, target_sync_frequency):
        """``[(step, logs)]`` of the target updates of ``for s in steps: update_online_params(s, rb); update_target_params(s)``,
        with the same effect, generator stream, cumulated-loss logs and order.  The gradient steps between two target operations
        go through ``_sample_and_learn_many`` when ``type(self)`` leaves the four methods of the loop (and the target hooks) as
        ``base`` defines them; subclasses and wrappers with a step of their own get the plain loop."""
        cls, out = type(self), []
        stock = (cls.update_online_params is base.update_online_params and cls.update_target_params is base.update_target_params
                 and cls._learn is DeviceAgent._learn and cls._sample_and_learn is DeviceAgent._sample_and_learn
                 and all(getattr(cls, h, None) is getattr(base, h, None) for h in ("_target_update", "_target_sync")))
        if not stock:
            for s in range(int(first_step), int(first_step) + int(n_steps)):
                self.update_online_params(s, replay_buffer)
                updated, logs = self.update_target_params(s)
                if updated:
                    out.append((s, logs))
            return out
        for n_grad, op, last in plan_step_runs(first_step, n_steps, self.update_to_data, self.target_update_frequency, target_sync_frequency):
            self._sample_and_learn_many(replay_buffer, n_grad)
            if op is not None:
                updated, logs = self.update_target_params(last)  # (the step is due for `op`: the method does exactly that)
                if updated:
                    out.append((last, logs))
        return out

    def _local_target_update(self):
        """target <- online (real copy), then online[k] <- online[k+1] over THIS agent's heads (idqn.py:78-80)."""
        self._ensure_handle(32)
        _hip.check(_hip.lib().idqn_target_update(self._handle, _hip.current_stream()), "idqn_target_update")

    def _local_target_sync(self):
        """target[k] <- online[k-1], k >= 1, over THIS agent's heads (idqn.py:20-24)."""
        self._ensure_handle(32)
        _hip.check(_hip.lib().idqn_target_sync(self._handle, _hip.current_stream()), "idqn_target_sync")

    def _apply_adam(self):
        _hip.check(_hip.lib().idqn_apply_adam(self._handle, _hip.current_stream()), "idqn_apply_adam")

    def _q_values(self, which, head, state):
        """Q-values [n, A] (device) of one head for <= 32 states."""
        dt = torch.uint8 if self._pixels else torch.float32
        s = self._dev(state, dt)
        n = 1 if s.numel() == int(np.prod(self._obs)) else int(s.shape[0])
        self._ensure_handle(32)
        self._keep_q = s
        _hip.check(_hip.lib().idqn_q_values(self._handle, int(which), int(head), _hip.ptr(s), n, _hip.ptr(self._q_out),
                                            _hip.current_stream()), "idqn_q_values")
        return self._q_out[:n]

    def _best_action(self, which, head, state):
        """Greedy action (device int32 scalar, first maximum on ties) of one head for one state: one C call.
        A host state goes through a pinned staging buffer (a pageable 28 KB upload costs ~100 us, this ~10)."""
        dt = torch.uint8 if self._pixels else torch.float32
        st = getattr(state, "tensor", state)
        if isinstance(st, torch.Tensor) and st.is_cuda:
            s = self._dev(st, dt)
        else:
            # a host state: ONE C call uploads it from pinned memory, runs the single-state path, brings the action back
            # and synchronises (what the reference's select_action does with its blocking `.item()`)
            if not hasattr(self, "_act_pin"):
                n = int(np.prod(self._obs))
                self._act_pin = torch.empty(n, dtype=dt).pin_memory()
                self._act_pin_np = self._act_pin.numpy()
                self._act_out = torch.zeros(4, dtype=torch.int32).pin_memory()
                self._act_out_np = self._act_out.numpy()
            src = np.asarray(getattr(state, "tensor", state))
            assert src.size == self._act_pin_np.size, "best_action takes a single state"
            pending = getattr(self, "_act_in_flight", None)
            if pending is not None:  # (a lazy action nobody collected: finish it before the staging buffer is rewritten)
                pending.item()
            self._act_pin_np[:] = src.reshape(-1)  # casts like the array conversion of the reference's jit would
            self._ensure_handle(32)
            if self.lazy_host_actions:
                _hip.check(_hip.lib().idqn_act_host_begin(self._handle, int(which), int(head), C.c_void_p(self._act_pin.data_ptr()),
                                                          _hip.ptr(self._q_out), C.c_void_p(self._act_out.data_ptr()),
                                                          _hip.current_stream()), "idqn_act_host_begin")
                self._act_in_flight = _PendingHostAction(self)
                return self._act_in_flight
            _hip.check(_hip.lib().idqn_act_host(self._handle, int(which), int(head), C.c_void_p(self._act_pin.data_ptr()),
                                                _hip.ptr(self._q_out), C.c_void_p(self._act_out.data_ptr()),
                                                _hip.current_stream()), "idqn_act_host")
            return _HostAction(int(self._act_out_np[0]))
        assert s.numel() == int(np.prod(self._obs)), "best_action takes a single state"
        self._ensure_handle(32)
        self._keep_q = s
        if not hasattr(self, "_action_out"):
            self._action_out = torch.zeros(32, dtype=torch.int32, device="cuda")
        _hip.check(_hip.lib().idqn_best_action(self._handle, int(which), int(head), _hip.ptr(s), 1, _hip.ptr(self._q_out),
                                               _hip.ptr(self._action_out), _hip.current_stream()), "idqn_best_action")
        return self._action_out[0]

    def _best_actions(self, which, heads, states):
        """Greedy actions (host int array [n], first maximum on ties) of n <= 32 host states, state i on head ``heads[i]``:
        the states are staged into one pinned block and ONE C call uploads them, runs the single-state arithmetic per state
        and brings the n actions back; the Q rows are left in ``self._q_out[:n]``.  ``idqn_act_host_many`` serves the MFMA
        cnn handles (the Dense_0 stream shared among the states of a head); a handle outside its domain answers
        ``E_INVALID`` once and ``idqn_act_host_many_fc`` (MLP, general-shape cnn) is tried under a flag of its own.  A
        handle both refuse (quantile heads, ...) acts through a loop of ``_best_action`` from then on: same actions, same
        Q rows.  An impala agent -- both refuse it -- asks ``idqn_act_host_many_impala`` third, under ``_act_many_imp_ok`` and
        by the same protocol, for the n in ``act_many_imp_sizes``; every other n stays on the loop."""
        heads = np.ascontiguousarray(np.asarray(heads, np.int32).reshape(-1))
        n = int(heads.size)
        if not 1 <= n <= 32 or len(states) != n:
            raise ValueError(f"best_actions takes 1..32 states and as many heads, got {len(states)} and {n}")
        if heads.min() < 0 or heads.max() >= self._K:
            raise ValueError(f"best_actions: heads {heads.tolist()} outside [0, {self._K})")
        pending = getattr(self, "_act_in_flight", None)
        if pending is not None:  # (a lazy single-state action nobody collected, as in _best_action)
            pending.item()
        size = int(np.prod(self._obs))
        srcs = [np.asarray(getattr(s, "tensor", s)) for s in states]
        assert all(a.size == size for a in srcs), "best_actions takes single states"
        self._ensure_handle(32)
        staged = False
        entries = [("_act_many_ok", "idqn_act_host_many"), ("_act_many_fc_ok", "idqn_act_host_many_fc")]
        if getattr(self, "_arch", None) == "impala" and n in self.act_many_imp_sizes:
            entries.append(("_act_many_imp_ok", "idqn_act_host_many_impala"))
        for flag, entry in entries:
            if not getattr(self, flag, True):
                continue
            if not staged:
                if not hasattr(self, "_acts_pin"):
                    dt = torch.uint8 if self._pixels else torch.float32  # the arch's dtype: pixels or features
                    self._acts_pin = torch.empty((32, size), dtype=dt).pin_memory()
                    self._acts_pin_np = self._acts_pin.numpy()
                    self._acts_out = torch.zeros(32, dtype=torch.int32).pin_memory()
                    self._acts_out_np = self._acts_out.numpy()
                for i, a in enumerate(srcs):
                    self._acts_pin_np[i] = a.reshape(-1)  # casts like the array conversion of the reference's jit would
                staged = True
            rc = getattr(_hip.lib(), entry)(self._handle, int(which), heads.ctypes.data, C.c_void_p(self._acts_pin.data_ptr()), n,
                                            _hip.ptr(self._q_out), C.c_void_p(self._acts_out.data_ptr()), _hip.current_stream())
            if rc != _hip.E_INVALID or self.__dict__.get(flag) is not None:
                _hip.check(rc, entry)
                setattr(self, flag, True)
                return self._acts_out_np[:n].astype(np.int64)
            setattr(self, flag, False)  # this entry does not serve the handle, from now on
        actions, rows = np.empty(n, np.int64), []
        for i in range(n):
            actions[i] = int(self._best_action(which, int(heads[i]), srcs[i]).item())
            rows.append(self._q_out[0].clone())
        self._q_out[:n] = torch.stack(rows)
        return actions

    def _debug(self, name):
        """Internal activation buffer as a flat float32 device tensor (tests only)."""
        p, nbytes = C.c_void_p(), C.c_int64()
        _hip.check(_hip.lib().idqn_debug_buffer(self._handle, name.encode(), C.byref(p), C.byref(nbytes)), name)
        out = torch.empty(nbytes.value // 4, dtype=torch.float32, device="cuda")
        C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(out.data_ptr()), p, C.c_size_t(nbytes.value), 3)
        return out

    def _numpy_tree(self, arena):
        host = arena.cpu().numpy()
        tree = {}
        for name, off, shape in self._leaves:
            *mods, leaf = name.split("/")
            v = host[:, off : off + int(np.prod(shape))].reshape((self._K,) + tuple(shape)).copy()
            node = tree
            for mod in mods:
                node = node.setdefault(mod, {})
            node[leaf] = v if self._stacked else v[0]
        return {"params": tree}

    def _load_flat(self, arena, flat):
        """flat: {"Conv_0/kernel": array [K, ...]} -> arena (fixture injection in tests)."""
        host = arena.cpu().numpy()
        for name, off, shape in self._leaves:
            v = np.asarray(flat[name], np.float32)
            if not self._stacked and v.shape == tuple(shape):
                v = v[None]
            host[:, off : off + int(np.prod(shape))] = v.reshape(self._K, -1)
        arena.copy_(torch.from_numpy(host))

    def _flat(self, arena):
        host = arena.cpu().numpy()
        return {name: host[:, off : off + int(np.prod(shape))].reshape((self._K,) + tuple(shape)).copy()
                for name, off, shape in self._leaves}

    def _flat_grad(self):
        """{"Conv_0/kernel": array [K, ...]} read from the two-region gradient arena (tests)."""
        host = self._grad.cpu().numpy()
        K, gP, (w0b, w0e) = self._K, self._gP, self._w0
        out = {}
        for name, off, shape in self._leaves:
            n = int(np.prod(shape))
            if w0e > w0b and off == w0b:
                base = K * gP + 64
                v = np.stack([host[base + k * (w0e - w0b) : base + k * (w0e - w0b) + n] for k in range(K)])
            else:
                o = off if off < w0b or w0e == w0b else off - (w0e - w0b)
                v = np.stack([host[k * gP + o : k * gP + o + n] for k in range(K)])
            out[name] = v.reshape((K,) + tuple(shape)).copy()
        return out

    def get_model(self):
        """Picklable ``{"params": self.params}`` with numpy leaves (idqn.py:133-134, experiments/base/utils.py:134).
        ``self.params`` is already the flax variables dict ``{"params": {"Conv_0": ...}}``, so the pickle holds
        ``model["params"]["params"]["Dense_0"]["kernel"]`` -- exactly what the reference's checkpoints hold."""
        return {"params": self._numpy_tree(self._online)}
