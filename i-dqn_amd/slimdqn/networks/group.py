"""Seed groups: S independent MLP agents (``iDQN`` / ``DQN``) whose learner steps and greedy actions are ONE device call each;
S Atari-shaped (cnn) agents share the acting call only (``idqn_act_group_host``, ``act_group_sizes``).

The reference runs its seeds as N processes on one device (``launch_job/*/train.sh``).  The one-launch MLP step uses one
workgroup per head, so S agents are a grid of (K, S) workgroups (``csrc/fc_group_kernels.h``) and every member's parameters,
moments, counters and losses after a group call are, byte for byte, what the member's own call leaves.  The members keep
their arenas, handles and hyper-parameters; a member may be driven alone between two group calls.

Prioritized samplers: ``AgentGroup`` itself steps such members through their own calls; their one-call group step is
``slimdqn.sample_collection.per.PrioritizedGroupLearner`` (``idqn_group_per_learn_on_replay_fc``), which takes this group's
C object (``_ensure_group``), its ring records (``_rings``) and its ``_stock`` rule.

Every member's buffer draws its own keys with the host protocol of ``DeviceAgent._sample_and_learn`` -- the sampler stream
of a member is what it would be alone -- and the drawn slots travel in one block.  Where the group entry refuses (agents
that are not MLPs, batches of more than 32 samples, prioritized samplers, ...) the members' own methods run on the slots
already drawn, under flags of the pattern of ``DeviceAgent._replay_fc_ok`` (unset: not tried; False: refused, the members'
own route from then on; True: it served).
"""
import ctypes as C

import numpy as np

from slimdqn import _hip, prng
from slimdqn.networks._agent import DeviceAgent, plan_step_runs

GROUP_MAX = 32  # members of a group: the acting slot holds 32 states (include/idqn_hip.h)


class AgentGroup:
    # The sizes S at which a group learner call is taken by default: those where its median lay below the minimum of the S
    # solo calls (tools/bench_seed_group.py -> profiles/seed_group.json).  Other sizes run the members one by one.
    group_sizes = frozenset(range(2, GROUP_MAX + 1))
    # The sizes S at which Atari-shaped (cnn) members act through ONE ``idqn_act_group_host`` call by default: those where its
    # median lay below the minimum of the loop of S ``idqn_act_host`` calls (tools/bench_act_group.py -> profiles/act_group.json).
    # Measured: S = 1, 2, 4, 8, 16, 32; S = 1 was SLOWER (42.7 against 40.8 us).  Sizes that were not measured are off.
    act_group_sizes = frozenset({2, 4, 8, 16, 32})

    def __init__(self, agents):
        self.agents = list(agents)
        if not 1 <= len(self.agents) <= GROUP_MAX:
            raise ValueError(f"a group holds 1..{GROUP_MAX} agents, got {len(self.agents)}")
        self._group, self._group_handles = None, None
        self._act_group, self._act_group_handles = None, None

    # ---- plumbing ----------------------------------------------------------------------------------
    def _destroy_group(self):
        if getattr(self, "_group", None) is not None:
            _hip.lib().idqn_group_destroy(self._group)
            self._group = None
        if getattr(self, "_act_group", None) is not None:
            _hip.lib().idqn_act_group_destroy(self._act_group)
            self._act_group = None

    def close(self):
        """Destroys the group object (before its members' handles go away)."""
        self._destroy_group()

    def __del__(self):
        try:
            self._destroy_group()
        except Exception:
            pass

    def _stock(self):
        """The members run the step and the acting rule of ``DeviceAgent`` itself and a group of this size is wanted."""
        return (len(self.agents) in self.group_sizes and getattr(self, "_group_ok", True)
                and all(isinstance(a, DeviceAgent) and a._arch == "fc" and type(a)._learn is DeviceAgent._learn
                        and type(a)._sample_and_learn is DeviceAgent._sample_and_learn for a in self.agents))

    def _ensure_group(self, batch):
        """The group over the members' current handles, or None once ``idqn_group_create`` has refused them."""
        if self.__dict__.get("_group_ok") is False:
            return None
        for a in self.agents:
            a._ensure_handle(batch)
        handles = tuple(a._handle.value for a in self.agents)
        if self._group is not None and handles == self._group_handles:
            return self._group
        self._destroy_group()  # (a member re-created its handle for a larger batch)
        arr = (C.c_void_p * len(handles))(*handles)
        g = C.c_void_p()
        rc = _hip.lib().idqn_group_create(arr, len(handles), C.byref(g))
        if rc == _hip.E_INVALID and self.__dict__.get("_group_ok") is None:
            self._group_ok = False  # not these handles (a wide net, different shapes, ...): the members' own calls from now on
            return None
        _hip.check(rc, "idqn_group_create")
        self._group, self._group_handles, self._group_ok = g, handles, True
        return g

    def _stock_act_cnn(self):
        """The members are Atari-shaped agents of one shape that act as ``DeviceAgent`` itself does, and an acting group of this
        size is wanted (the learner routes have a rule of their own, ``_stock``)."""
        a0 = self.agents[0]
        return (len(self.agents) in self.act_group_sizes and getattr(self, "_group_act_cnn_ok", True)
                and all(isinstance(a, DeviceAgent) and a._arch == "cnn" and not getattr(a, "_n_quantiles", 0)
                        and type(a)._best_action is DeviceAgent._best_action and type(a)._best_actions is DeviceAgent._best_actions
                        and a._obs == a0._obs and a._K == a0._K and a.network.n_actions == a0.network.n_actions
                        and list(a.network.features) == list(a0.network.features) for a in self.agents))

    def _ensure_act_group(self):
        """The acting group over the members' current handles, or None once ``idqn_act_group_create`` has refused them."""
        if self.__dict__.get("_group_act_cnn_ok") is False:
            return None
        for a in self.agents:
            a._ensure_handle(32)
        handles = tuple(a._handle.value for a in self.agents)
        if self._act_group is not None and handles == self._act_group_handles:
            return self._act_group
        if self._act_group is not None:  # (a member re-created its handle for a larger batch)
            _hip.lib().idqn_act_group_destroy(self._act_group)
            self._act_group = None
        arr = (C.c_void_p * len(handles))(*handles)
        g = C.c_void_p()
        rc = _hip.lib().idqn_act_group_create(arr, len(handles), C.byref(g))
        if rc == _hip.E_INVALID and self.__dict__.get("_group_act_cnn_ok") is None:
            self._group_act_cnn_ok = False  # not these handles (general shapes, J > 512, ...): the members' own calls from now on
            return None
        _hip.check(rc, "idqn_act_group_create")
        self._act_group, self._act_group_handles = g, handles
        return g

    @staticmethod
    def _rings(views):
        rings = (_hip.GroupRing * len(views))()
        for r, (frames, n_frames, frame_bytes, rows, stack) in zip(rings, (v[:5] for v in views)):
            r.frames_dev, r.n_frames, r.frame_bytes = frames.data_ptr(), int(n_frames), int(frame_bytes)
            r.rows_dev, r.stack = rows.data_ptr(), int(stack)
        return rings

    def _learn_route(self, rbs):
        return (self._stock() and getattr(self, "_group_learn_ok", True) and len(rbs) == len(self.agents)
                and all(a._replay_fc_route(rb) for a, rb in zip(self.agents, rbs)))

    # ---- the learner step ----------------------------------------------------------------------------
    def _sample_and_learn(self, rbs):
        """One gradient step of every member: S draws, one call."""
        if not self._learn_route(rbs):
            for a, rb in zip(self.agents, rbs):
                a._sample_and_learn(rb)
            return
        draws = [np.ascontiguousarray(rb.sample_slots(), np.int32) for rb in rbs]
        views = [rb.ring_view() for rb in rbs]
        if not self._learn_group(draws, views, rbs, None):
            self._learn_members(draws, views, rbs)

    def _learn_members(self, draws, views, rbs):
        """The members' own single step on slots that are already drawn."""
        for a, rb, slots, view in zip(self.agents, rbs, draws, views):
            a._learn_on_replay_fc(rb, view, slots=slots, gather=lambda rb=rb, slots=slots: rb._gather(slots))

    def _learn_group(self, draws, views, rbs, n_steps):
        """The group call on the drawn slots ([S] arrays of [B], or of [n_steps][B]); False: refused, nothing was done."""
        B = int(draws[0].shape[-1])
        if (B > 32 or any(d.shape != draws[0].shape for d in draws)
                or not all(a._ring_fc_fusable(v) for a, v in zip(self.agents, views))):
            return False
        group = self._ensure_group(B)
        if group is None:
            return False
        block = np.ascontiguousarray(np.stack(draws), np.int32)
        lib, rings = _hip.lib(), self._rings(views)
        if n_steps is None:
            flag, name = "_group_learn_ok", "idqn_group_learn_on_replay_fc"
            rc = lib.idqn_group_learn_on_replay_fc(group, rings, block.ctypes.data, B, B, 0, _hip.current_stream())
        else:
            flag, name = "_group_steps_ok", "idqn_group_learn_steps_on_replay_fc"
            rc = lib.idqn_group_learn_steps_on_replay_fc(group, rings, block.ctypes.data, int(n_steps), B, B, 0, _hip.current_stream())
        if rc == _hip.E_INVALID and self.__dict__.get(flag) is None:
            setattr(self, flag, False)  # e.g. a member with prioritized-replay buffers: not this group, from now on
            return False
        _hip.check(rc, name)
        setattr(self, flag, True)
        for a in self.agents:
            a._replay_fc_ok = True
        return True

    def _sample_and_learn_many(self, rbs, n):
        """n gradient steps of every member: each buffer is drawn n times first (the draws of n single steps), then one call
        per ``MAX_STEPS_PER_CALL`` steps."""
        n = int(n)
        if n <= 0:
            return
        if n < min(a.learn_steps_min for a in self.agents if hasattr(a, "learn_steps_min")) or not self._learn_route(rbs) \
                or not getattr(self, "_group_steps_ok", True):
            for _ in range(n):
                self._sample_and_learn(rbs)
            return
        draws = [[np.ascontiguousarray(rb.sample_slots(), np.int32) for _ in range(n)] for rb in rbs]
        views = [rb.ring_view() for rb in rbs]
        i = 0
        while i < n and getattr(self, "_group_steps_ok", True):
            m = min(_hip.MAX_STEPS_PER_CALL, n - i)
            if len({d.size for ds in draws for d in ds[i : i + m]}) != 1 or \
                    not self._learn_group([np.stack(ds[i : i + m]) for ds in draws], views, rbs, m):
                break
            i += m
        for j in range(i, n):  # refused: single steps on the slots already drawn, as a group where that serves
            step = [ds[j] for ds in draws]
            if not (getattr(self, "_group_learn_ok", True) and self._learn_group(step, views, rbs, None)):
                self._learn_members(step, views, rbs)

    def update_online_params(self, step, replay_buffers):
        due = [step % a.update_to_data == 0 for a in self.agents]
        if all(due):
            self._sample_and_learn(list(replay_buffers))
        else:  # (a sweep over update_to_data: the members that are due step alone)
            for a, rb, d in zip(self.agents, replay_buffers, due):
                if d:
                    a._sample_and_learn(rb)

    def update_target_params(self, step):
        """``[(updated, logs)]`` of the members' own ``update_target_params(step)``."""
        return [a.update_target_params(step) for a in self.agents]

    def update_params_many(self, first_step, n_steps, replay_buffers):
        """The loop ``update_online_params(s, rbs); update_target_params(s)`` over ``n_steps`` steps; per member the list
        ``[(step, logs)]`` of its target updates, as the member's own ``update_params_many`` returns it."""
        rbs, a0 = list(replay_buffers), self.agents[0]
        schedule = lambda a: (a.update_to_data, a.target_update_frequency, getattr(a, "target_sync_frequency", None))
        if not self._stock() or any(schedule(a) != schedule(a0) for a in self.agents):
            return [a.update_params_many(first_step, n_steps, rb) for a, rb in zip(self.agents, rbs)]
        out = [[] for _ in self.agents]
        for n_grad, op, last in plan_step_runs(first_step, n_steps, *schedule(a0)):
            self._sample_and_learn_many(rbs, n_grad)
            if op is not None:
                for o, (updated, logs) in zip(out, self.update_target_params(last)):
                    if updated:
                        o.append((last, logs))
        return out

    # ---- acting ----------------------------------------------------------------------------------------
    def best_actions(self, which, heads, states, members=None):
        """Greedy actions (host int array [n]) of n <= 32 host states: state i on head ``heads[i]`` of member ``members[i]``
        (default: one state per member, in order) of the online (``which`` = 0) or target (1) parameters, one device call;
        the Q rows are left in ``self.q_out[:n]``.  A member's lazy action that nobody collected is collected first."""
        heads = np.ascontiguousarray(np.asarray(heads, np.int32).reshape(-1))
        n = int(heads.size)
        members = np.ascontiguousarray(np.arange(n) if members is None else np.asarray(members), np.int32).reshape(-1)
        if not 1 <= n <= 32 or len(states) != n or members.size != n:
            raise ValueError(f"best_actions takes 1..32 states, as many heads and members, got {len(states)}, {n}, {members.size}")
        if members.min() < 0 or members.max() >= len(self.agents):
            raise ValueError(f"best_actions: members {members.tolist()} outside [0, {len(self.agents)})")
        for a in self.agents:
            pending = getattr(a, "_act_in_flight", None)
            if pending is not None:
                pending.item()
        group = self._ensure_group(32) if self._stock() and getattr(self, "_group_act_ok", True) else None
        if group is not None:
            import torch

            a0 = self.agents[0]
            size = int(np.prod(a0._obs))
            if not hasattr(self, "_pin"):
                self._pin = torch.empty((32, size), dtype=torch.float32).pin_memory()
                self._pin_np = self._pin.numpy()
                self._out = torch.zeros(32, dtype=torch.int32).pin_memory()
                self._out_np = self._out.numpy()
                self.q_out = torch.zeros((32, a0.network.n_actions), dtype=torch.float32, device="cuda")
            for i, s in enumerate(states):
                self._pin_np[i] = np.asarray(getattr(s, "tensor", s)).reshape(-1)
            rc = _hip.lib().idqn_group_act_host_fc(group, int(which), members.ctypes.data, heads.ctypes.data,
                                                   C.c_void_p(self._pin.data_ptr()), n, _hip.ptr(self.q_out),
                                                   C.c_void_p(self._out.data_ptr()), _hip.current_stream())
            if rc != _hip.E_INVALID or self.__dict__.get("_group_act_ok") is not None:
                _hip.check(rc, "idqn_group_act_host_fc")
                self._group_act_ok = True
                return self._out_np[:n].astype(np.int64)
            self._group_act_ok = False
        group = self._ensure_act_group() if self._stock_act_cnn() else None
        if group is not None:
            import torch

            a0 = self.agents[0]
            if not hasattr(self, "_pin_u8"):
                self._pin_u8 = torch.empty((32, int(np.prod(a0._obs))), dtype=torch.uint8).pin_memory()
                self._pin_u8_np = self._pin_u8.numpy()
                self._out = torch.zeros(32, dtype=torch.int32).pin_memory()
                self._out_np = self._out.numpy()
                self.q_out = torch.zeros((32, a0.network.n_actions), dtype=torch.float32, device="cuda")
            for i, s in enumerate(states):
                self._pin_u8_np[i] = np.asarray(getattr(s, "tensor", s)).reshape(-1)  # casts as DeviceAgent._best_action does
            rc = _hip.lib().idqn_act_group_host(group, int(which), members.ctypes.data, heads.ctypes.data,
                                                C.c_void_p(self._pin_u8.data_ptr()), n, _hip.ptr(self.q_out),
                                                C.c_void_p(self._out.data_ptr()), _hip.current_stream())
            if rc != _hip.E_INVALID or self.__dict__.get("_group_act_cnn_ok") is not None:
                _hip.check(rc, "idqn_act_group_host")
                self._group_act_cnn_ok = True
                return self._out_np[:n].astype(np.int64)
            self._group_act_cnn_ok = False
        return np.array([int(self.agents[m]._best_action(int(which), int(h), s).item()) for m, h, s in zip(members, heads, states)],
                        np.int64)

    def select_heads(self, keys, members=None):
        """The head each member's ``best_action`` would draw from its key (``idqn.py:126-131``; 0 for ``DQN``)."""
        members = range(len(keys)) if members is None else members
        return [prng.randint(k, 0, self.agents[m].n_networks) if hasattr(self.agents[m], "n_networks") else 0
                for k, m in zip(keys, members)]
