"""i-IQN agent on the HIP path -- BASELINE config 3, a LABELLED EXTENSION (parity unpinned).

The reference snapshot has no quantile code: its README names i-IQN and points at another repository
(``/root/reference/README.md:3,10``).  This class keeps the reference's iDQN protocol (constructor arguments, chain of
K heads, ``update_online_params`` / ``update_target_params`` / ``best_action``, ``slimdqn/networks/idqn.py:27-134``) and
swaps the head for an implicit quantile network (Dabney et al. 2018) -- the algorithm and its sources are written down
in ``oracle/iqn_ref.py``, which is also what the parity tests compare against.

Quantile fractions are drawn on the host from numpy's PCG64 (the sampler's generator family, ``samplers.py:17``) and
handed to the library as data: a step is a deterministic function of (parameters, batch, fractions).  They travel through
two pinned staging buffers used in turn (asynchronous copies: the host does not wait for the stream each step).
Acting: ``argmax_a mean_l Z(s, tau_l)[a]`` over ``n_quantiles`` fractions, for a uniformly drawn head -- head AND
fractions are functions of the ``key`` the trainer passes, like ``iDQN.best_action`` (``idqn.py:126-131``).
"""
import ctypes as C

import numpy as np
import torch

from slimdqn import _hip, prng
from slimdqn.networks._agent import _HostAction, _PendingHostAction
from slimdqn.networks.idqn import iDQN


class iIQN(iDQN):
    def __init__(self, key, observation_dim, n_actions, n_networks: int, features: list, architecture_type: str,
                 learning_rate: float, gamma: float, update_horizon: int, update_to_data: int,
                 target_update_frequency: int, target_sync_frequency: int, adam_eps: float = 1e-8,
                 n_quantiles: int = 32):
        assert architecture_type == "cnn", "the quantile heads are built on the cnn trunk"
        assert 1 <= n_quantiles <= 64
        self._n_quantiles = int(n_quantiles)  # read by DeviceAgent._config: the layout gains Embed_0/{kernel,bias}
        super().__init__(key, observation_dim, n_actions, n_networks, features, architecture_type, learning_rate, gamma,
                         update_horizon, update_to_data, target_update_frequency, target_sync_frequency, adam_eps)
        self._tau_rng = np.random.Generator(np.random.PCG64(prng.randint(key, 0, 2**31 - 1)))
        self._tau_dev = None
        self._tau_act = torch.zeros(self._n_quantiles * 32, dtype=torch.float32, device="cuda")
        self._pins = {}  # name -> [two pinned host tensors, their numpy views, the events behind their last copies, turn]

    def _upload(self, name, host: np.ndarray, dst: torch.Tensor):
        """host -> dst[: host.size] through one of two pinned buffers used in turn; a buffer is written again only after the
        event recorded behind its previous copy (the copy itself is asynchronous: no stream synchronisation per step)."""
        ent = self._pins.get(name)
        if ent is None or ent[0][0].numel() < host.size or ent[0][0].dtype != dst.dtype:
            pins = [torch.empty(max(host.size, 1), dtype=dst.dtype).pin_memory() for _ in range(2)]
            ent = self._pins[name] = [pins, [p.numpy() for p in pins], [None, None], 0]
        pins, views, events, turn = ent
        if events[turn] is not None:
            events[turn].synchronize()
        views[turn][: host.size] = host.reshape(-1)
        dst[: host.size].copy_(pins[turn][: host.size], non_blocking=True)
        ev = events[turn] or torch.cuda.Event()
        ev.record()
        events[turn] = ev
        ent[3] = turn ^ 1

    def sample_fractions(self, batch_size: int) -> np.ndarray:
        """tau [K][3][N][B] in (0, 1): online, action-selection and target fractions of every head."""
        return self._tau_rng.random((self._K, 3, self._n_quantiles, batch_size)).astype(np.float32)

    def _upload_fractions(self, B, taus=None):
        """The step's fractions [K][3][N][B] -> ``self._tau_dev`` (drawn from ``_tau_rng`` unless given)."""
        if taus is None:
            taus = self.sample_fractions(B)
        taus = np.ascontiguousarray(taus, np.float32)
        assert taus.shape == (self._K, 3, self._n_quantiles, B), taus.shape
        if self._tau_dev is None or self._tau_dev.numel() != taus.size:
            self._tau_dev = torch.empty(taus.size, dtype=torch.float32, device="cuda")
        self._upload("tau", taus, self._tau_dev)

    def _learn_on_replay(self, view, slots_host=None, slots_dev=None, taus=None):
        """The step on the buffer's frame ring (``idqn_iqn_learn_on_replay`` / ``_dev``): the fractions are drawn exactly as
        ``_learn`` draws them.  Returns the library's code; ``E_INVALID`` = this handle runs another conv path, nothing was
        enqueued and the drawn fractions are still in ``self._tau_dev`` for the two-call step."""
        frames, n_frames, frame_bytes, rows, stack = view[:5]
        B = int(slots_host.size if slots_dev is None else slots_dev.numel())
        self._upload_fractions(B, taus)
        self._ensure_handle(B)
        lib = _hip.lib()
        if slots_dev is None:
            slots_host = np.ascontiguousarray(slots_host, np.int32)
            return lib.idqn_iqn_learn_on_replay(self._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                slots_host.ctypes.data, _hip.ptr(self._tau_dev), B, int(stack), 0,
                                                _hip.current_stream())
        return lib.idqn_iqn_learn_on_replay_dev(self._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                _hip.ptr(slots_dev), _hip.ptr(self._tau_dev), B, int(stack), 0,
                                                _hip.current_stream())

    def _sample_and_learn(self, replay_buffer):
        """``update_online_params``'s step: one C call on the frame ring where the buffer and the shapes allow it (the
        conditions of ``DeviceAgent._sample_and_learn``), else sample, gather and ``_learn``."""
        rb = replay_buffer
        if not self._replay_fusable(rb):
            return self._learn(rb.sample())
        slots = rb.sample_slots()
        view = rb.ring_view()
        if not self._ring_fusable(view):
            self._replay_fused_ok = False
            return self._learn(rb._gather(slots))
        B = int(slots.size)
        taus = self.sample_fractions(B)
        rc = self._learn_on_replay(view, slots_host=slots, taus=taus)
        if rc == _hip.E_INVALID and self.__dict__.get("_replay_fused_ok") is None:
            # this handle runs another conv path (IDQN_CONV=f32): same slots, same fractions, two calls, from now on
            self._replay_fused_ok = False
            return self._learn(rb._gather(slots), taus=taus)
        _hip.check(rc, "idqn_iqn_learn_on_replay")
        self._replay_fused_ok = True
        return self._losses

    def _learn(self, batch, flags=0, mean_divisor=None, taus=None):
        """One gradient step of the K quantile heads on a device-resident batch.

        With prioritized-replay buffers set on the handle (``idqn_set_per_buffers``, what ``PrioritizedLearner`` does):
        weights ``w`` [B] make the loss of head k ``(1 / B) sum_b w_b l_kb`` with ``l_kb = (1 / N) sum_ij rho_ij`` the per-sample
        quantile Huber loss (``oracle/iqn_ref.py``'s ``aux["per_sample"]``), the gradient of sample b is scaled by ``w_b``, and
        ``td_abs[k][b] = (1 / N^2) sum_ij |delta_ij|`` -- the mean absolute pairwise TD error, |TD| for N = 1 -- is written as
        the priority signal.  Without them the step is the plain one, bit for bit.  ``mean_divisor`` (sharded minibatches) is
        refused: there is no data-parallel i-IQN."""
        assert mean_divisor is None, "the quantile heads have no sharded-minibatch mode"
        s, s2 = self._dev(batch.state, torch.uint8), self._dev(batch.next_state, torch.uint8)
        assert tuple(s.shape[1:]) == self._obs, f"state shape {tuple(s.shape)} vs observation_dim {self._obs}"
        B = int(s.shape[0])
        assert 1 <= B <= 256, "the quantile heads take minibatches of 1 to 256 samples"
        a = self._dev(batch.action, torch.int32)
        r = self._dev(batch.reward, torch.float32)
        t = self._dev(batch.is_terminal, torch.uint8)
        self._upload_fractions(B, taus)
        self._ensure_handle(B)
        self._keep = (s, s2, a, r, t)
        _hip.check(_hip.lib().idqn_iqn_learn_on_batch(self._handle, _hip.ptr(s), _hip.ptr(s2), _hip.ptr(a), _hip.ptr(r),
                                                      _hip.ptr(t), _hip.ptr(self._tau_dev), B, int(flags),
                                                      _hip.current_stream()), "idqn_iqn_learn_on_batch")
        return self._losses

    def _iqn_q(self, which, head, state, taus=None, want_action=False, key=None):
        st = getattr(state, "tensor", state)
        E = int(np.prod(self._obs))
        if isinstance(st, torch.Tensor) and st.is_cuda:
            s = self._dev(st, torch.uint8)
        else:  # a host state (the trainer's acting path): pinned staging like iDQN._best_action, no pageable upload
            src = np.ascontiguousarray(np.asarray(st)).astype(np.uint8, copy=False)
            if not hasattr(self, "_state_dev") or self._state_dev.numel() < src.size:
                self._state_dev = torch.empty(max(src.size, E), dtype=torch.uint8, device="cuda")
            self._upload("state", src, self._state_dev)
            s = self._state_dev[: src.size]
        assert s.numel() % E == 0, f"state of {s.numel()} bytes vs observation_dim {self._obs}"
        n = s.numel() // E
        if taus is None:
            # acting is a function of the key (idqn.py:128 draws the head from it; the fractions come from a child of it)
            rng = prng.generator(prng.split(key, 2)[1]) if key is not None else self._tau_rng
            taus = rng.random((self._n_quantiles, n)).astype(np.float32)
        taus = np.ascontiguousarray(taus, np.float32)
        assert taus.shape == (self._n_quantiles, n), taus.shape
        assert 1 <= n <= 256, "the quantile heads take 1 to 256 states per call"
        if self._tau_act.numel() < taus.size:
            self._tau_act = torch.zeros(taus.size, dtype=torch.float32, device="cuda")
        self._upload("tau_act", taus, self._tau_act)
        self._ensure_handle(n)  # (a handle holds Q-values of up to its max_batch states)
        self._keep_q = s
        q_out = self._q_out  # (more than its 32 rows: a buffer of this class, grown on demand)
        if q_out.shape[0] < n:
            if getattr(self, "_q_out_n", None) is None or self._q_out_n.shape[0] < n:
                self._q_out_n = torch.zeros((n, q_out.shape[1]), dtype=torch.float32, device="cuda")
            q_out = self._q_out_n
        if not hasattr(self, "_action_out") or self._action_out.numel() < n:
            self._action_out = torch.zeros(max(n, 32), dtype=torch.int32, device="cuda")
        _hip.check(_hip.lib().idqn_iqn_q_values(self._handle, int(which), int(head), _hip.ptr(s), n, _hip.ptr(self._tau_act),
                                                _hip.ptr(q_out), _hip.ptr(self._action_out) if want_action else None,
                                                _hip.current_stream()), "idqn_iqn_q_values")
        return q_out[:n]

    def q_values(self, params, state, idx_params: int, taus=None):
        """Mean over the fractions of Z(s, tau) of head ``idx_params``: device tensor [n, A]."""
        assert params is self.params or params is self.target_params
        return self._iqn_q(0 if params is self.params else 1, idx_params, state, taus)

    def _act_host(self, which, head, src, taus, key):
        """``best_action`` for ONE state in host memory (the trainer's case): ``idqn_iqn_act_host`` -- the state and the N
        fractions go through pinned buffers of this agent, the single-state chain is replayed as one graph and the action
        comes back through the mailbox (a ``_PendingHostAction`` with ``lazy_host_actions``, like ``DeviceAgent._best_action``)."""
        if taus is None:  # drawn as _iqn_q draws them: a function of the key, _tau_rng untouched unless there is none
            rng = prng.generator(prng.split(key, 2)[1]) if key is not None else self._tau_rng
            taus = rng.random((self._n_quantiles, 1)).astype(np.float32)
        taus = np.ascontiguousarray(taus, np.float32)
        assert taus.size == self._n_quantiles, taus.shape
        if not hasattr(self, "_act_pin"):
            self._act_pin = torch.empty(int(np.prod(self._obs)), dtype=torch.uint8).pin_memory()
            self._act_pin_np = self._act_pin.numpy()
            self._act_tau_pin = torch.empty(self._n_quantiles, dtype=torch.float32).pin_memory()
            self._act_tau_np = self._act_tau_pin.numpy()
            self._act_out = torch.zeros(4, dtype=torch.int32).pin_memory()
            self._act_out_np = self._act_out.numpy()
        pending = getattr(self, "_act_in_flight", None)
        if pending is not None:  # (a lazy action nobody collected: finish it before the staging buffers are rewritten)
            pending.item()
        self._act_pin_np[:] = src.reshape(-1)
        self._act_tau_np[:] = taus.reshape(-1)
        self._ensure_handle(32)
        args = (self._handle, int(which), int(head), C.c_void_p(self._act_pin.data_ptr()), C.c_void_p(self._act_tau_pin.data_ptr()),
                _hip.ptr(self._q_out), C.c_void_p(self._act_out.data_ptr()), _hip.current_stream())
        if self.lazy_host_actions:
            _hip.check(_hip.lib().idqn_iqn_act_host_begin(*args), "idqn_iqn_act_host_begin")
            self._act_in_flight = _PendingHostAction(self)
            return self._act_in_flight
        _hip.check(_hip.lib().idqn_iqn_act_host(*args), "idqn_iqn_act_host")
        return _HostAction(int(self._act_out_np[0]))

    def best_action(self, params, state, key, taus=None):
        idx_params = prng.randint(key, 0, self.n_networks)
        assert params is self.params or params is self.target_params
        which = 0 if params is self.params else 1
        st = getattr(state, "tensor", state)
        if not (isinstance(st, torch.Tensor) and st.is_cuda):
            src = np.asarray(st)
            if src.size == int(np.prod(self._obs)):  # one state on the host: the latency path
                return self._act_host(which, idx_params, src, taus, key)
        self._iqn_q(which, idx_params, state, taus, want_action=True, key=key)
        return self._action_out[0]

    def best_actions(self, params, states, keys, taus=None):
        """``[best_action(params, states[i], keys[i]).item() for i]`` as a host int64 array, for 1..32 host states: head i is
        ``prng.randint(keys[i], 0, K)`` and fraction row i is what ``_act_host`` draws from ``keys[i]`` (``_tau_rng`` is left
        alone; ``taus`` [n][N] overrides the draw).  States and fractions are staged into pinned blocks of this agent and ONE
        C call (``idqn_iqn_act_host_many``) evaluates them all: row i of ``self._q_out[:n]`` and action i are, byte for
        byte, the single-state call's.  A handle that answers ``E_INVALID`` once on an otherwise valid call makes this the
        loop of single-state calls from then on: same actions, same rows."""
        assert params is self.params or params is self.target_params
        n = len(states)
        if not 1 <= n <= 32 or len(keys) != n:
            raise ValueError(f"best_actions takes 1..32 states and as many keys, got {n} and {len(keys)}")
        N = self._n_quantiles
        heads = [prng.randint(k, 0, self.n_networks) for k in keys]
        if taus is None:
            taus = np.stack([prng.generator(prng.split(k, 2)[1]).random((N, 1)).astype(np.float32)[:, 0] for k in keys])
        return self._act_host_many(0 if params is self.params else 1, heads, states, taus)

    def _act_host_many(self, which, heads, states, taus):
        """Greedy actions (host int64 array [n]) of n <= 32 host states, state i on head ``heads[i]`` with the fractions
        ``taus[i]`` [N]: ONE ``idqn_iqn_act_host_many`` call, or -- after that entry has refused this handle once -- the loop
        of ``_act_host`` calls; the Q rows are left in ``self._q_out[:n]`` either way."""
        heads = np.ascontiguousarray(np.asarray(heads, np.int32).reshape(-1))
        n, N = int(heads.size), self._n_quantiles
        if not 1 <= n <= 32 or len(states) != n:
            raise ValueError(f"best_actions takes 1..32 states and as many heads, got {len(states)} and {n}")
        if heads.min() < 0 or heads.max() >= self._K:
            raise ValueError(f"best_actions: heads {heads.tolist()} outside [0, {self._K})")
        taus = np.ascontiguousarray(taus, np.float32)
        if taus.shape != (n, N):
            raise ValueError(f"best_actions: fractions of shape {taus.shape}, expected {(n, N)}")
        pending = getattr(self, "_act_in_flight", None)
        if pending is not None:  # (a lazy single-state action nobody collected, as in _best_actions)
            pending.item()
        size = int(np.prod(self._obs))
        srcs = [np.asarray(getattr(s, "tensor", s)) for s in states]
        assert all(a.size == size for a in srcs), "best_actions takes single states"
        self._ensure_handle(32)
        if getattr(self, "_iqn_act_many_ok", True):
            if not hasattr(self, "_iacts_pin"):
                self._iacts_pin = torch.empty((32, size), dtype=torch.uint8).pin_memory()
                self._iacts_pin_np = self._iacts_pin.numpy()
                self._iacts_tau_pin = torch.empty((32, N), dtype=torch.float32).pin_memory()
                self._iacts_tau_np = self._iacts_tau_pin.numpy()
                self._iacts_out = torch.zeros(32, dtype=torch.int32).pin_memory()
                self._iacts_out_np = self._iacts_out.numpy()
            for i, a in enumerate(srcs):
                self._iacts_pin_np[i] = a.reshape(-1)
            self._iacts_tau_np[:n] = taus
            rc = self._iqn_act_many_call(which, heads, n)
            if rc != _hip.E_INVALID or self.__dict__.get("_iqn_act_many_ok") is not None:
                _hip.check(rc, "idqn_iqn_act_host_many")
                self._iqn_act_many_ok = True
                return self._iacts_out_np[:n].astype(np.int64)
            self._iqn_act_many_ok = False  # this handle acts one state at a time, from now on
        actions, rows = np.empty(n, np.int64), []
        for i in range(n):
            actions[i] = int(self._act_host(which, int(heads[i]), srcs[i], taus[i], None).item())
            rows.append(self._q_out[0].clone())
        self._q_out[:n] = torch.stack(rows)
        return actions

    def _iqn_act_many_call(self, which, heads, n):
        """The one C call of ``best_actions`` on the staged blocks: the library's return code."""
        return _hip.lib().idqn_iqn_act_host_many(self._handle, int(which), heads.ctypes.data, C.c_void_p(self._iacts_pin.data_ptr()),
                                                 C.c_void_p(self._iacts_tau_pin.data_ptr()), n, _hip.ptr(self._q_out),
                                                 C.c_void_p(self._iacts_out.data_ptr()), _hip.current_stream())
