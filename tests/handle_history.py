"""Handle-history harness: every entry on a USED handle must give the bits it gives on a FRESH one.

The fp tests tie a fresh ``idqn_create`` handle to the fp64 oracle.  A handle in use is another thing: scratch is addressed with
the active number of 32-sample blocks of each call, the launch routes change with that number, pad lanes of a ragged block keep
what the previous batch left there, and the handle keeps sticky settings, plan maps, graph caches, gate words and last-arriver
counters between calls.  The steps are deterministic (ordered sums), so no tolerance is needed: ``run_script`` drives a list of
ops through ONE agent whose handle is sized once, and after each op repeats that op on a newly created agent that was given the
used agent's state from just before the op.  Everything the op returns or writes, and every state arena after it, must be equal
byte for byte.

A plain helper module like ``tests/kat_int_path.py``: ``tests/test_gpu_handle_history.py`` runs it on the library's agents,
``tests/test_handle_history_host.py`` on numpy stubs (one of which leaks a pad lane on purpose: the harness can fail).

What an agent has to offer: the state arenas ``_online _target _mu _nu _count _cum`` (torch tensors or numpy arrays, copied in
place), ``_ensure_handle`` / ``_handle`` / ``_destroy_handle``, ``_obs _arch _K network.n_actions`` for the synthetic inputs, and
the entry each op of its script calls (``OPS`` below).  ``max_batch`` is the same for the used and the fresh handle, and so is the
environment: independence from ``max_batch`` is not claimed here.
"""
import os
from collections import namedtuple

import numpy as np

ARENAS = ("_online", "_target", "_mu", "_nu", "_count", "_cum")
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
Op = namedtuple("Op", "kind args")
TD_PAD, TD_SENTINEL = 64, -7.0  # the priority output is followed by this many sentinels: nothing past [K][B] may be written


# ---- the ops a script is made of -----------------------------------------------------------------------------------------
def learn(B, seed, flags=0):
    """One gradient step (``_learn``) on the synthetic batch of ``seed``."""
    return Op("learn", dict(B=B, seed=seed, flags=flags))


def grads_then_adam(B, seed):
    """``F_GRADS_ONLY`` (losses and the whole gradient arena are compared), then ``_apply_adam``."""
    return Op("grads_then_adam", dict(B=B, seed=seed))


def q_values(which, head, n, seed):
    return Op("q_values", dict(which=which, head=head, n=n, seed=seed))


def act_host(which, head, seed, lazy=False):
    """Greedy action for one state in host memory; ``lazy``: the begin / end form (``lazy_host_actions``)."""
    return Op("act_host", dict(which=which, head=head, seed=seed, lazy=lazy))


def act_dev(which, head, seed):
    """Greedy action for one state in device memory."""
    return Op("act_dev", dict(which=which, head=head, seed=seed))


def target_update():
    return Op("target_update", {})


def target_sync():
    return Op("target_sync", {})


def weighted_learn(B, seed):
    """``idqn_set_per_buffers(weights, td_abs)``, the step, both buffers back to null."""
    return Op("weighted_learn", dict(B=B, seed=seed))


def learn_on_replay(B, seed):
    """The replay-sourced step on the script's shared ReplayBuffer, the slots drawn once and passed explicitly."""
    return Op("learn_on_replay", dict(B=B, seed=seed))


BATCH_OPS = ("learn", "grads_then_adam", "weighted_learn", "learn_on_replay")   # they run a minibatch of args["B"] samples
SYNTHETIC_BATCH_OPS = ("learn", "grads_then_adam", "weighted_learn")            # ... that the harness builds itself
MOVES_STATE = BATCH_OPS + ("target_update", "target_sync")                      # the others must leave every arena untouched


def describe(op):
    return "%s(%s)" % (op.kind, ", ".join("%s=%r" % kv for kv in op.args.items()))


# ---- torch tensors and numpy arrays alike ------------------------------------------------------------------------------
def _host(x):
    """A detached host copy (numpy) of a tensor, an array or a scalar."""
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy().copy()
    return np.array(x, copy=True)


def _clone(x):
    return x.clone() if hasattr(x, "clone") else np.array(x, copy=True)


def _assign(dst, src):
    if hasattr(dst, "copy_"):
        dst.copy_(src)
    else:
        dst[...] = src


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _where(agent, name, idx):
    """Flat index of a state arena -> 'head k, leaf[i]' through the agent's leaf table."""
    leaves = getattr(agent, "_leaves", None)
    P = getattr(agent, "_P", None)
    if name not in ("_online", "_target", "_mu", "_nu") or not leaves or not P:
        return ""
    k, off = divmod(int(idx), int(P))
    for leaf, lo, shape in leaves:
        if lo <= off < lo + int(np.prod(shape)):
            return " = head %d, %s[%d]" % (k, leaf, off - lo)
    return " = head %d, offset %d" % (k, off)


def _compare(i, script, name, got, want, agent):
    """``got`` (used handle) against ``want`` (fresh handle), byte for byte; the message names everything needed to start looking."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (i, describe(script[i]), name, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() == want.tobytes():
        return
    diff = np.flatnonzero(_bits(got) != _bits(want))
    first = int(diff[0])
    before = describe(script[i - 1]) if i else "(nothing: the first op of the script)"
    raise AssertionError(
        "op %d %s after %s: %s differs between the used and the fresh handle in %d of %d elements, first at flat index %d%s "
        "(used %r, fresh %r)" % (i, describe(script[i]), before, name, diff.size, got.size, first, _where(agent, name, first),
                                 got.reshape(-1)[first], want.reshape(-1)[first]))


# ---- inputs: built once per op, shared by the used and the fresh agent ------------------------------------------------------
def _shape(agent):
    obs = tuple(agent._obs) if agent._arch == "cnn" else int(agent._obs[0])
    return obs, int(agent.network.n_actions), agent._arch


def _states(agent, seed, n):
    from oracle import qnet_ref as Q

    obs, A, arch = _shape(agent)
    return Q.synthetic_batch(seed, n, obs, A, arch)[0]


def _fractions(agent, seed, shape):
    """Quantile fractions in (0.01, 0.99) from the op's seed (agents with quantile heads only)."""
    return (np.random.default_rng([seed, 77]).random(shape) * 0.98 + 0.01).astype(np.float32)


def make_replay(agent, capacity=64, n=150):
    """A small package ReplayBuffer filled the way test_learn_on_replay_is_sample_then_learn fills its own: more transitions
    than the ring holds (slots and frames have wrapped), episode ends (zero frames in the stacks behind them) every 37."""
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    H, W, _ = agent._obs
    A = int(agent.network.n_actions)
    rb = ReplayBuffer(UniformSamplingDistribution(5), batch_size=32, max_capacity=capacity, stack_size=4, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(9)
    for i in range(n):
        rb.add(TransitionElement(rng.integers(0, 256, (H, W), dtype=np.uint8), int(rng.integers(A)), float(rng.normal()),
                                 bool(i % 37 == 36), False))
    assert rb.add_count > capacity
    return rb


def _prepare(agent, op, boosted, ctx):
    """The op's inputs as host arrays.  ``boosted``: the batch in front of a ragged one -- rewards x 1000 and no terminals,
    so that a pad lane leaking into the next step cannot hide under rounding."""
    from oracle import qnet_ref as Q

    a, N = op.args, int(getattr(agent, "_n_quantiles", 0))
    K = int(agent._K)
    inp = {}
    if op.kind in SYNTHETIC_BATCH_OPS:
        obs, A, arch = _shape(agent)
        s, ac, r, s2, t = Q.synthetic_batch(a["seed"], a["B"], obs, A, arch)
        if boosted:
            r, t = r * np.float32(1000.0), np.zeros_like(t)
        inp["batch"] = Batch(s, ac, r, s2, t)
    if op.kind == "weighted_learn":
        inp["weights"] = np.random.default_rng([a["seed"], 3]).uniform(0.05, 1.0, a["B"]).astype(np.float32)
    if op.kind == "learn_on_replay":
        if "replay" not in ctx:
            ctx["replay"] = make_replay(agent)
        # the sampler's own draw, made once: the used and the fresh agent both get these slots (the op's seed decides the
        # fractions of an agent with quantile heads only)
        inp["slots"] = np.ascontiguousarray(ctx["replay"].sample_slots(a["B"]), np.int32)
    if op.kind in ("q_values", "act_host", "act_dev"):
        n = a.get("n", 1)
        st = _states(agent, a["seed"], n)
        inp["states"] = st if op.kind == "q_values" else st[0]
        if N:
            inp["taus"] = _fractions(agent, a["seed"], (N, n))
    if N and op.kind in BATCH_OPS:
        inp["taus"] = _fractions(agent, a["seed"], (K, 3, N, a["B"]))
    return inp


# ---- running one op on one agent: thin calls into what DeviceAgent / iDQN / iIQN expose -------------------------------
def _kw(inp):
    return {"taus": inp["taus"]} if "taus" in inp else {}


def _op_learn(agent, a, inp, ctx):
    kw = _kw(inp)
    if a["flags"]:
        kw["flags"] = a["flags"]
    out = {"losses": _host(agent._learn(inp["batch"], **kw))}
    if a["flags"] & 1:  # F_GRADS_ONLY: the gradient arena is the result
        out["_grad"] = _host(agent._grad)
    return out


def _op_grads_then_adam(agent, a, inp, ctx):
    from slimdqn import _hip

    out = {"losses": _host(agent._learn(inp["batch"], flags=_hip.F_GRADS_ONLY)), "_grad": _host(agent._grad)}
    out["_count before Adam"] = _host(agent._count)
    agent._apply_adam()
    return out


def _op_q_values(agent, a, inp, ctx):
    if "taus" in inp:
        return {"q": _host(agent._iqn_q(a["which"], a["head"], inp["states"], inp["taus"]))}
    return {"q": _host(agent._q_values(a["which"], a["head"], inp["states"]))}


def _op_act_host(agent, a, inp, ctx):
    agent.lazy_host_actions = bool(a["lazy"])
    try:
        if "taus" in inp:
            act = agent._act_host(a["which"], a["head"], np.asarray(inp["states"]), inp["taus"], None)
        else:
            act = agent._best_action(a["which"], a["head"], np.asarray(inp["states"]))
        assert (type(act).__name__ == "_PendingHostAction") == bool(a["lazy"]), type(act)
        return {"action": np.asarray([int(act.item())], np.int32), "q": _host(agent._q_out[0])}
    finally:
        agent.lazy_host_actions = False


def _op_act_dev(agent, a, inp, ctx):
    import torch

    st = torch.from_numpy(np.ascontiguousarray(inp["states"])).cuda()
    if "taus" in inp:
        q = agent._iqn_q(a["which"], a["head"], st, inp["taus"], want_action=True)
        return {"action": _host(agent._action_out[:1]), "q": _host(q)}
    act = agent._best_action(a["which"], a["head"], st)
    return {"action": _host(act).reshape(1), "q": _host(agent._q_out[0])}


def _op_target_update(agent, a, inp, ctx):
    agent._local_target_update()
    return {}


def _op_target_sync(agent, a, inp, ctx):
    agent._local_target_sync()
    return {}


def _op_weighted_learn(agent, a, inp, ctx):
    import torch

    from slimdqn import _hip

    K, B = int(agent._K), a["B"]
    w = torch.from_numpy(inp["weights"]).cuda()
    td = torch.full((K * B + TD_PAD,), TD_SENTINEL, dtype=torch.float32, device="cuda")
    agent._ensure_handle(B)
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w), _hip.ptr(td)), "idqn_set_per_buffers")
    try:
        losses = _host(agent._learn(inp["batch"], **_kw(inp)))
    finally:
        _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    td = _host(td)
    assert (td[K * B :] == TD_SENTINEL).all(), "td_abs entries past [K][batch] were written"
    return {"losses": losses, "td_abs": td}


def _op_learn_on_replay(agent, a, inp, ctx):
    """``idqn_learn_on_replay`` / ``idqn_iqn_learn_on_replay``.  The entry is built for the plane conv path and refuses every
    other handle before it enqueues anything; with ``IDQN_CONV=f32`` the op is therefore what ``_sample_and_learn`` makes of
    it there -- the same slots gathered, then ``_learn`` -- and the refusal itself is asserted.  Nowhere else is a refusal accepted."""
    from slimdqn import _hip

    rb, slots, B = ctx["replay"], inp["slots"], a["B"]
    view = rb.ring_view()
    if "taus" in inp:
        _hip.check(agent._learn_on_replay(view, slots_host=slots, taus=inp["taus"]), "idqn_iqn_learn_on_replay")
        return {"losses": _host(agent._losses)}
    frames, n_frames, frame_bytes, rows, stack = view[:5]
    agent._ensure_handle(B)
    rc = _hip.lib().idqn_learn_on_replay(agent._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                         slots.ctypes.data, B, int(stack), B, 0, _hip.current_stream())
    if os.environ.get("IDQN_CONV") == "f32":
        assert rc == _hip.E_INVALID, rc
        agent._learn(rb._gather(slots))
    else:
        _hip.check(rc, "idqn_learn_on_replay")
    return {"losses": _host(agent._losses)}


OPS = {"learn": _op_learn, "grads_then_adam": _op_grads_then_adam, "q_values": _op_q_values, "act_host": _op_act_host,
       "act_dev": _op_act_dev, "target_update": _op_target_update, "target_sync": _op_target_sync,
       "weighted_learn": _op_weighted_learn, "learn_on_replay": _op_learn_on_replay}


def _execute(agent, op, inp, ctx):
    """(outputs, state after) of one op on one agent, everything on the host."""
    out = OPS[op.kind](agent, op.args, inp, ctx)
    return out, {name: _host(getattr(agent, name)) for name in ARENAS}


def _boosted(script):
    """Indices of the synthetic batches that get rewards x 1000 and no terminals: the batch-carrying op in front of each
    ragged one (``B`` no multiple of the 32-sample block) -- directly in front of it, or with only calls that carry no
    minibatch (acting, Q-values, target ops) in between."""
    marks, last = set(), None
    for i, op in enumerate(script):
        if op.kind in BATCH_OPS:
            if op.args["B"] % 32 and last is not None and script[last].kind in SYNTHETIC_BATCH_OPS:
                marks.add(last)
            last = i
    return marks


def run_script(make_agent, max_batch, script, on_op=None):
    """Drive ``script`` through one agent whose handle is created once for ``max_batch``; after every op, repeat the op on a
    newly created agent holding the state the used one had before it, and require equal bytes in every output and in every
    state arena.  Returns the number of ops compared.  ``on_op(i, op, outputs)`` (optional) sees the used agent's outputs."""
    script = list(script)
    for op in script:
        assert op.kind in OPS, op
        assert op.args.get("B", 1) <= max_batch and op.args.get("n", 1) <= max_batch, \
            "%s exceeds max_batch %d: the handle would be rebuilt" % (describe(op), max_batch)
    boosted = _boosted(script)
    used = make_agent()
    used._ensure_handle(max_batch)
    handle = used._handle
    assert handle is not None
    ctx = {}
    try:
        for i, op in enumerate(script):
            inp = _prepare(used, op, i in boosted, ctx)
            before = {name: _clone(getattr(used, name)) for name in ARENAS}
            before_host = {name: _host(v) for name, v in before.items()}
            got_out, got_state = _execute(used, op, inp, ctx)
            assert used._handle is handle, "op %d %s rebuilt the used handle" % (i, describe(op))
            moved = [name for name in ARENAS if got_state[name].tobytes() != before_host[name].tobytes()]
            if op.kind in MOVES_STATE:
                assert moved, "op %d %s left every state arena as it was: the script does not move the parameters" % (i, describe(op))
            else:
                assert not moved, "op %d %s changed %s" % (i, describe(op), moved)
            fresh = make_agent()
            try:
                fresh._ensure_handle(max_batch)
                fresh_handle = fresh._handle
                for name in ARENAS:
                    _assign(getattr(fresh, name), before[name])
                want_out, want_state = _execute(fresh, op, inp, ctx)
                assert fresh._handle is fresh_handle, "op %d %s rebuilt the fresh handle" % (i, describe(op))
            finally:
                fresh._destroy_handle()
            assert sorted(got_out) == sorted(want_out)
            for name in got_out:
                _compare(i, script, name, got_out[name], want_out[name], used)
            for name in ARENAS:
                _compare(i, script, name, got_state[name], want_state[name], used)
            if on_op is not None:
                on_op(i, op, got_out)
            del fresh
    finally:
        used._destroy_handle()
    return len(script)
