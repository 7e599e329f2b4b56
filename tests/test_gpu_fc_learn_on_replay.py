"""GPU: the replay-sourced learner step of MLP ("fc") and general-shape cnn handles -- ``idqn_learn_on_replay_fc`` / ``_dev`` and
the route ``DeviceAgent._sample_and_learn`` takes through them (flag ``_replay_fc_ok``).

The contract is bit identity with the two-call form (``replay_buffer.sample()`` = ``replay_gather_stacked``, then
``idqn_learn_on_batch``): parameters, Adam moments, losses, running loss sums, step counts and the sampler's generator state,
byte for byte, on ``ReplayBuffer`` and ``VectorReplayBuffer`` rings that have wrapped, with sampled elements whose stack crosses
an episode start (zero frames; only a stack of more than one frame can) and terminal elements.  Every MLP step kernel is
reached: ``k_fc_step_par`` with the ring as its minibatch source (B <= 32, widths <= 128), ``k_fc_step_mfma`` / ``k_fc_step_lds``
behind the staging launch (B = 64, the [520] net); the general-shape cnn runs behind the same staging launch.

The sampler seed of a case is CHOSEN at run time: the first generator seed whose draws contain the elements the case is about
(the draw is host arithmetic on the filled buffer, so the choice is deterministic), and the property is asserted again on the
slots the fused agent really drew.
"""
import numpy as np
import pytest

import fc_shapes as F

pytestmark = pytest.mark.gpu

#        kind   frame shape  dtype     stack  obs dim / shape  features          K  A  B   agent
CONFIGS = {
    "lunar_par": ("fc", (8,), np.float32, 1, 8, [100, 100], 3, 4, 32, "iDQN"),
    "lunar_b64": ("fc", (8,), np.float32, 1, 8, [100, 100], 3, 4, 64, "iDQN"),
    "fc_520": ("fc", (8,), np.float32, 1, 8, [520], 3, 4, 32, "iDQN"),
    "dqn_ragged": ("fc", (3,), np.float32, 2, 6, [7], 1, 2, 3, "DQN"),
    "gcnn_12x10x2": ("cnn", (12, 10), np.uint8, 2, (12, 10, 2), [2, 3, 1, 15], 2, 3, 5, "iDQN"),
    "gcnn_20x20x4": ("cnn", (20, 20), np.uint8, 4, (20, 20, 4), [8, 8, 8, 30, 20], 2, 6, 8, "iDQN"),
}
# Rows of the one-launch step's shape table (tests/fc_shapes.py) as ring-sourced cases "shape_<row>": odd din, 33- and 128-wide
# layers, A = 1, d0 = 128, B = 1, the net within 2 KB of the LDS budget and the one that fits fc_par_plan but not fc_steps_plan
SHAPE_CASES = ["shape_" + rid for rid in F.DESCENDANT_ROWS + (F.DESCENDANT_LOOP_ROW,)]
CONFIGS.update({"shape_" + rid: ("fc", (F.BY_ID[rid].d0,), np.float32, 1, F.BY_ID[rid].d0, list(F.BY_ID[rid].feats), F.BY_ID[rid].K,
                                 F.BY_ID[rid].A, F.BY_ID[rid].B, "iDQN") for rid in F.DESCENDANT_ROWS + (F.DESCENDANT_LOOP_ROW,)})
STATE = ("_online", "_mu", "_nu", "_losses", "_cum", "_count")
STEPS, HORIZON, CAPACITY = 3, 2, 40


def _agent(name, fuse=True):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.idqn import iDQN

    arch, _, _, _, obs, feats, K, A, _, cls = CONFIGS[name]
    if cls == "DQN":
        agent = DQN(0, obs, A, feats, arch, 1e-3, 0.99, HORIZON, 1, 10**9)
    else:
        agent = iDQN(0, obs, A, K, feats, arch, 1e-3, 0.99, HORIZON, 1, 10**9, 10**9)
    agent.fuse_replay_sampling = fuse
    return agent


def _frame(rng, shape, dtype):
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.standard_normal(shape).astype(np.float32)


def _buffer(name, seed=0):
    """A ``ReplayBuffer`` of 40 elements fed 150 transitions (slots and frame ring have wrapped), episodes of 7 steps."""
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    _, shape, dtype, stack, _, _, _, A, B, _ = CONFIGS[name]
    rb = ReplayBuffer(UniformSamplingDistribution(seed), batch_size=B, max_capacity=CAPACITY, stack_size=stack, update_horizon=HORIZON,
                      gamma=0.99)
    rng = np.random.default_rng(11)
    for i in range(150):
        rb.add(TransitionElement(_frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), i % 7 == 6, i % 7 == 6))
    rb.reuse_sample_buffers = True
    assert rb.add_count > CAPACITY and rb._t > rb._n_frames
    return rb


def _vector_buffer(name, seed=0):
    """E = 3 time lines in segments of 24 main slots, fed past the capacity and around the segments."""
    from slimdqn.sample_collection.replay_buffer import TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    _, shape, dtype, stack, _, _, _, A, B, _ = CONFIGS[name]
    rb = VectorReplayBuffer(UniformSamplingDistribution(seed), B, CAPACITY, stack_size=stack, update_horizon=HORIZON, gamma=0.99, n_envs=3,
                            segment=24)
    rng, lengths, n = np.random.default_rng(13), (7, 5, 9), [0, 0, 0]
    for _ in range(24 * 3 + 3):
        row = []
        for e in range(3):
            n[e] += 1
            last = n[e] >= lengths[e]
            n[e] = 0 if last else n[e]
            row.append(TransitionElement(_frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), last, last))
        rb.add_many(row)
    rb.reuse_sample_buffers = True
    assert rb._plan.n_growths == 0 and rb.add_count > CAPACITY and min(rb._plan.frame_count) > 3 * 24
    return rb


def _rows(rb, slots):
    return (rb._plan.rows if hasattr(rb, "_plan") else rb._meta)[np.asarray(slots)]


def _covers(rb, draws, stack, first_slot=False):
    """The draws hold a terminal element, (stack > 1) an element with zero frames in front of an episode start, and on the vector
    ring an element whose stack ends at its segment's FIRST main slot (stack > 1: its other frames are the mirror slots)."""
    rows = _rows(rb, np.concatenate(draws))
    ok = bool((rows[:, 6] == 1).any()) and (stack == 1 or bool((rows[:, 1] < stack).any() or (rows[:, 3] < stack).any()))
    if first_slot:
        p = rb._plan
        ok = ok and bool(((rows[:, 0] % p.segment_slots == stack - 1) | (rows[:, 2] % p.segment_slots == stack - 1)).any())
    return ok


def _choose_seed(rb, stack, first_slot=False):
    for seed in range(400):
        rb._sampling_distribution._rng_key = np.random.default_rng(seed)
        if _covers(rb, [rb.sample_slots() for _ in range(STEPS)], stack, first_slot):
            return seed
    raise AssertionError("no sampler seed below 400 draws the elements this case is about")


def _assert_same(a, b, names=STATE):
    for name in names:
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert x.tobytes() == y.tobytes(), f"{name} differs"


def _identity(name, make_buffer, first_slot=False):
    import torch

    stack = CONFIGS[name][3]
    rb_a, rb_b = make_buffer(name), make_buffer(name)
    seed = _choose_seed(rb_a, stack, first_slot)
    for rb in (rb_a, rb_b):
        rb._sampling_distribution._rng_key = np.random.default_rng(seed)
    fused, plain = _agent(name), _agent(name, fuse=False)
    drawn, real = [], rb_a.sample_slots
    rb_a.sample_slots = lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1]
    for step in range(STEPS):
        fused.update_online_params(step, rb_a)
        plain.update_online_params(step, rb_b)
    torch.cuda.synchronize()
    assert len(drawn) == STEPS and _covers(rb_a, drawn, stack, first_slot), "the drawn slots miss the elements this case is about"
    assert fused.__dict__.get("_replay_fc_ok") is True, "the replay-sourced route did not run"
    assert plain.__dict__.get("_replay_fc_ok") is None
    _assert_same(fused, plain)
    assert np.isfinite(fused._losses.cpu().numpy()).all() and (fused._count.cpu().numpy() == STEPS).all()
    assert rb_a._sampling_distribution._rng_key.bit_generator.state == rb_b._sampling_distribution._rng_key.bit_generator.state
    return fused


@pytest.mark.parametrize("name", list(CONFIGS))
def test_update_online_params_is_sample_then_learn(name):
    """Three ``update_online_params`` calls on the new route against ``fuse_replay_sampling = False``: every byte of the agent's
    state and the sampler's generator state.  (On the parent commit the fused agent gathers too and ``_replay_fc_ok`` is unset.)"""
    fused = _identity(name, _buffer)
    if CONFIGS[name][0] == "cnn":  # the plane entry's own flag says what it said before: not its handle / not its ring
        assert fused.__dict__.get("_replay_fused_ok") is False
    if name in SHAPE_CASES:  # inside fc_par_plan: the ring was the one-launch step's own minibatch source
        import ctypes as C

        from slimdqn import _hip

        mean_ms, n_l, kernel = C.c_double(), C.c_int32(), C.create_string_buffer(64)
        _hip.check(_hip.lib().idqn_profile_read(fused._handle, C.byref(mean_ms), C.byref(n_l), kernel), "idqn_profile_read")
        assert kernel.value.decode() == "k_fc_step_par<ring>"


@pytest.mark.parametrize("name", ["lunar_par", "gcnn_12x10x2"])
def test_same_identity_on_the_vector_ring(name):
    """``VectorReplayBuffer``, E = 3: a sampled element ends at its segment's first main slot, so for a stack of two its older
    frame is the segment's mirror slot."""
    _identity(name, _vector_buffer, first_slot=True)


def _call(agent, rb, slots, dev=False, flags=0, B=None, **over):
    """The C entry on ``rb``'s ring with explicit slots; ``over`` replaces arguments by name (refusal tests)."""
    import torch

    from slimdqn import _hip

    frames, n_frames, frame_bytes, rows, stack = rb.ring_view()[:5]
    B = int(len(slots)) if B is None else B
    agent._ensure_handle(max(B, 32))
    host = np.ascontiguousarray(slots, np.int32)
    agent._keep_slots = torch.from_numpy(host).cuda() if dev else host
    a = dict(ring=_hip.ptr(frames), n_frames=int(n_frames), frame_bytes=int(frame_bytes), rows=_hip.ptr(rows),
             slots_ptr=_hip.ptr(agent._keep_slots) if dev else host.ctypes.data, stack=int(stack), div=B)
    a.update(over)
    fn = _hip.lib().idqn_learn_on_replay_fc_dev if dev else _hip.lib().idqn_learn_on_replay_fc
    return fn(agent._handle, a["ring"], a["n_frames"], a["frame_bytes"], a["rows"], a["slots_ptr"], B, a["stack"], a["div"], flags,
              _hip.current_stream())


def _slots(rb, n, seed):
    lo = max(0, rb.add_count - CAPACITY)
    return (np.random.default_rng(seed).integers(lo, rb.add_count, n) % CAPACITY).astype(np.int32)


@pytest.mark.parametrize("name", ["lunar_par", "lunar_b64", "gcnn_12x10x2"])
def test_device_slots_equal_host_slots(name):
    import torch

    from slimdqn import _hip

    rb, B = _buffer(name), CONFIGS[name][8]
    host, dev = _agent(name), _agent(name)
    for step in range(2):
        slots = _slots(rb, B, 20 + step)
        _hip.check(_call(host, rb, slots), "idqn_learn_on_replay_fc")
        _hip.check(_call(dev, rb, slots, dev=True), "idqn_learn_on_replay_fc_dev")
    torch.cuda.synchronize()
    _assert_same(host, dev)
    assert (host._count.cpu().numpy() == 2).all()


def test_prioritized_learner_takes_the_dev_entry():
    """``PrioritizedLearner.step()`` with an MLP agent hands its leaves to ``idqn_learn_on_replay_fc_dev``: losses, parameters,
    Adam state, |TD| and the tree equal those of the gathered two-call form."""
    import torch

    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement

    name = "lunar_par"
    _, shape, dtype, stack, _, _, _, A, B, _ = CONFIGS[name]

    def make(fuse):
        rb = ReplayBuffer(SlotPrioritizedSampler(4, CAPACITY), batch_size=B, max_capacity=CAPACITY, stack_size=stack, update_horizon=HORIZON,
                          gamma=0.99)
        rng = np.random.default_rng(17)
        for i in range(150):
            rb.add(TransitionElement(_frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), i % 7 == 6, i % 7 == 6))
        rb.reuse_sample_buffers = True
        return PrioritizedLearner(_agent(name, fuse=fuse), rb)

    a, b = make(True), make(False)
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert a.agent.__dict__.get("_replay_fc_ok") is True and b.agent.__dict__.get("_replay_fc_ok") is None
    _assert_same(a.agent, b.agent)
    assert a._td_abs.cpu().numpy().tobytes() == b._td_abs.cpu().numpy().tobytes()
    assert a._leaves.cpu().numpy().tobytes() == b._leaves.cpu().numpy().tobytes()
    assert a.sampler._sum_tree._nodes_dev.cpu().numpy().tobytes() == b.sampler._sum_tree._nodes_dev.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["lunar_par", "lunar_b64", "gcnn_12x10x2"])
def test_grads_only_then_apply_adam_is_the_plain_step(name):
    import torch

    from slimdqn import _hip

    rb, B = _buffer(name), CONFIGS[name][8]
    plain, split = _agent(name), _agent(name)
    for step in range(2):
        slots = _slots(rb, B, 30 + step)
        _hip.check(_call(plain, rb, slots), "idqn_learn_on_replay_fc")
        _hip.check(_call(split, rb, slots, flags=_hip.F_GRADS_ONLY), "idqn_learn_on_replay_fc")
        split._apply_adam()
    torch.cuda.synchronize()
    _assert_same(plain, split, ("_online", "_mu", "_nu", "_losses", "_grad"))


def _snapshot(agent):
    return {n: getattr(agent, n).cpu().numpy().tobytes() for n in ("_online", "_target", "_mu", "_nu", "_count", "_cum", "_grad")}


def test_refusals_enqueue_nothing():
    """Every documented refusal answers ``E_INVALID`` with a message, and parameters, Adam state, count and a sentinel-filled
    gradient arena (the losses live in it) are untouched."""
    import torch

    from slimdqn import _hip
    from slimdqn.networks.iiqn import iIQN
    from slimdqn.networks.idqn import iDQN

    rb_fc, rb_cnn = _buffer("lunar_par"), _buffer("gcnn_20x20x4")
    fc, gcnn = _agent("lunar_par"), _agent("gcnn_20x20x4")
    plane = iDQN(0, (20, 20, 4), 5, 2, [32, 32, 32, 128], "cnn", 6.25e-5, 0.99, HORIZON, 1, 10**9, 10**9, adam_eps=1.5e-4)
    quant = iIQN(3, (20, 20, 4), 5, 2, [32, 32, 32, 256], "cnn", 6.25e-5, 0.99, HORIZON, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=4)
    s32, s8 = _slots(rb_fc, 32, 1), _slots(rb_cnn, 8, 2)
    cases = [
        ("a plane-path handle", plane, rb_cnn, s8, {}),
        ("a quantile handle", quant, rb_cnn, s8, {}),
        ("batch 0", fc, rb_fc, s32, dict(B=0)),
        ("batch max_batch + 1", fc, rb_fc, np.resize(s32, 33), {}),
        ("a wrong frame_bytes (fc)", fc, rb_fc, s32, dict(frame_bytes=28)),
        ("a wrong stack (fc)", fc, rb_fc, s32, dict(stack=2)),
        ("null slots (fc)", fc, rb_fc, s32, dict(slots_ptr=None)),
        ("null slots (fc, device)", fc, rb_fc, s32, dict(slots_ptr=None, dev=True)),
        ("a wrong frame_bytes (cnn)", gcnn, rb_cnn, s8, dict(frame_bytes=399)),
        ("a wrong stack (cnn)", gcnn, rb_cnn, s8, dict(stack=3)),
        ("null slots (cnn)", gcnn, rb_cnn, s8, dict(slots_ptr=None)),
        ("a null ring", gcnn, rb_cnn, s8, dict(ring=None)),
        ("a null row table", fc, rb_fc, s32, dict(rows=None)),
        ("a mean divisor below the batch", fc, rb_fc, s32, dict(div=31)),
    ]
    for agent in (fc, gcnn, plane, quant):
        agent._ensure_handle(32)
        agent._grad.fill_(-7.25)
        agent._mu.fill_(0.5)
    torch.cuda.synchronize()
    for what, agent, rb, slots, over in cases:
        before = _snapshot(agent)
        B, dev = over.pop("B", None), over.pop("dev", False)
        if what == "batch max_batch + 1":
            assert agent._handle_batch == 32
            frames, n_frames, frame_bytes, rows, stack = rb.ring_view()[:5]
            rc = _hip.lib().idqn_learn_on_replay_fc(agent._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                    slots.ctypes.data, 33, int(stack), 33, 0, _hip.current_stream())
        else:
            rc = _call(agent, rb, slots, dev=dev, B=B, **over)
        torch.cuda.synchronize()
        assert rc == _hip.E_INVALID, f"{what}: answered {rc}"
        assert _hip.lib().idqn_last_error(), what
        assert _snapshot(agent) == before, f"{what}: the refused call changed the agent's state"


# ---- handle history: every call on a used handle equals the same call on a fresh one ----------------------------------------
def _run_op(agent, op, rb, name):
    """Runs one operation; returns the bytes it produced besides the agent's state."""
    import torch

    from slimdqn import _hip

    kind, arg = op
    arch, shape, dtype, stack, obs, _, K, A, _, _ = CONFIGS[name]
    rng = np.random.default_rng(1000 + arg)
    size = int(np.prod(agent._obs))
    state = lambda: (rng.integers(0, 256, size, dtype=np.uint8) if arch == "cnn" else rng.standard_normal(size).astype(np.float32))
    out = b""
    if kind in ("replay", "replay_dev"):
        B = arg
        _hip.check(_call(agent, rb, _slots(rb, B, arg), dev=kind == "replay_dev"), "idqn_learn_on_replay_fc")
    elif kind == "learn":
        agent._learn(rb._gather(_slots(rb, arg, 77 + arg)))
    elif kind == "q":
        out = agent._q_values(arg % 2, arg % K, np.stack([state() for _ in range(3)])).cpu().numpy().tobytes()
    elif kind == "act":
        out = bytes([int(agent._best_action(arg % 2, arg % K, state()))]) + agent._q_out[0].cpu().numpy().tobytes()
    elif kind == "act_many":
        heads = [int(h) for h in rng.integers(0, K, 5)]
        acts = agent._best_actions(arg % 2, heads, [state() for _ in heads])
        assert agent.__dict__.get("_act_many_fc_ok") is True
        out = np.asarray(acts).tobytes() + agent._q_out[:5].cpu().numpy().tobytes()
    elif kind == "target_update":
        agent._local_target_update()
    elif kind == "target_sync":
        agent._local_target_sync()
    torch.cuda.synchronize()
    return out


HISTORY = [("replay", 32), ("q", 1), ("learn", 32), ("replay", 64), ("act", 2), ("replay_dev", 32), ("act_many", 3), ("replay", 7),
           ("target_update", 0), ("replay", 32), ("target_sync", 0), ("learn", 64), ("replay_dev", 64), ("q", 4), ("replay", 32)]


@pytest.mark.parametrize("name", ["lunar_par", "gcnn_12x10x2"])
def test_handle_history(name):
    """One handle (max_batch 64) takes the new entry -- one-launch route, staging route, host and device slots, a short batch --
    interleaved with plain steps, Q-values, acting, target update and sync; after each call its state and the call's outputs
    equal those of a freshly created handle that was given the state before the call."""
    import torch

    rb = _buffer(name)
    used = _agent(name)
    used._ensure_handle(64)
    handle = used._handle.value
    arenas = ("_online", "_target", "_mu", "_nu", "_count", "_cum", "_grad")
    for op in HISTORY:
        fresh = _agent(name)
        fresh._ensure_handle(64)
        for n in arenas:
            getattr(fresh, n).copy_(getattr(used, n))
        torch.cuda.synchronize()
        got, want = _run_op(used, op, rb, name), _run_op(fresh, op, rb, name)
        assert got == want, f"{op}: outputs differ from a fresh handle's"
        after_used, after_fresh = _snapshot(used), _snapshot(fresh)
        for n in arenas:
            assert after_used[n] == after_fresh[n], f"{op}: {n} differs from a fresh handle's"
        assert used._handle.value == handle, "the handle was rebuilt"
