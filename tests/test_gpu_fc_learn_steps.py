"""GPU: n replay-sourced learner steps in one C call -- ``idqn_learn_steps_on_replay_fc`` / ``_dev``, the persistent kernel
``k_fc_steps_par`` behind them, and the agent / trainer layers on top (``update_params_many``, ``VectorTrainer``).

The contract is byte identity with n consecutive ``idqn_learn_on_replay_fc`` calls on the same slots: parameters, Adam moments,
losses, running loss sums, counts, the last gradient; the target arena untouched.  Buffers are capacity-40 rings that have
wrapped (7-step episodes, horizon 2); the sampler seed of a case is chosen at run time so that the draws hold a terminal element
and, for a stack of two, a stack with zero frames in front of an episode start -- asserted again on the slots used.
"""
import numpy as np
import pytest

import fc_shapes as F

pytestmark = pytest.mark.gpu

#        arch  frame shape  dtype     stack  obs         features      K  A  B   agent
CONFIGS = {
    "lunar": ("fc", (8,), np.float32, 1, 8, [100, 100], 3, 4, 32, "iDQN"),
    "dqn_ragged": ("fc", (3,), np.float32, 2, 6, [7], 1, 2, 3, "DQN"),
    "odd_tiles": ("fc", (5,), np.float32, 1, 5, [128, 33], 2, 3, 17, "iDQN"),
    "lunar_b64": ("fc", (8,), np.float32, 1, 8, [100, 100], 3, 4, 64, "iDQN"),
    "fc_520": ("fc", (8,), np.float32, 1, 8, [520], 3, 4, 32, "iDQN"),
    "gcnn": ("cnn", (12, 10), np.uint8, 2, (12, 10, 2), [2, 3, 1, 15], 2, 3, 5, "iDQN"),
}
PERSISTENT = ("lunar", "dqn_ragged", "odd_tiles")
# Rows of the one-launch step's shape table (tests/fc_shapes.py: odd din, 33- and 128-wide layers, A = 1, d0 = 128, B = 1, the net
# within 2 KB of the LDS budget), as "shape_<row>"; the net that fits fc_par_plan but not fc_steps_plan goes to the loop route.


def _shape_config(rid):
    r = F.BY_ID[rid]
    return ("fc", (r.d0,), np.float32, 1, r.d0, list(r.feats), r.K, r.A, r.B, "iDQN")


CONFIGS.update({"shape_" + rid: _shape_config(rid) for rid in F.DESCENDANT_ROWS + (F.DESCENDANT_LOOP_ROW,)})
PERSISTENT += tuple("shape_" + rid for rid in F.DESCENDANT_ROWS)
SHAPE_LOOP = "shape_" + F.DESCENDANT_LOOP_ROW
STATE = ("_online", "_mu", "_nu", "_losses", "_cum", "_count", "_grad", "_target")
HORIZON, CAPACITY = 2, 40


def _agent(name, **kw):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.idqn import iDQN

    arch, _, _, _, obs, feats, K, A, _, cls = CONFIGS[name]
    if cls == "DQN":
        return DQN(0, obs, A, feats, arch, 1e-3, 0.99, HORIZON, kw.get("utd", 1), kw.get("tuf", 10**9))
    return iDQN(0, obs, A, K, feats, arch, 1e-3, 0.99, HORIZON, kw.get("utd", 1), kw.get("tuf", 10**9), kw.get("tsf", 10**9))


def _frame(rng, shape, dtype):
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.standard_normal(shape).astype(np.float32)


def _buffer(name, seed=0):
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
    assert rb.add_count > CAPACITY
    return rb


def _rows(rb, slots):
    return (rb._plan.rows if hasattr(rb, "_plan") else rb._meta)[np.asarray(slots).reshape(-1)]


def _covers(rb, slots, stack):
    rows = _rows(rb, slots)
    return bool((rows[:, 6] == 1).any()) and (stack == 1 or bool((rows[:, 1] < stack).any() or (rows[:, 3] < stack).any()))


def _draws(rb, n, stack, head=None):
    """``n`` sampler draws [n][B] from the first generator seed whose draws hold the elements the cases are about (``head``: and
    whose first ``head`` draws already do -- the small batches of the shape-table rows)."""
    for seed in range(400):
        rb._sampling_distribution._rng_key = np.random.default_rng(seed)
        slots = np.stack([np.ascontiguousarray(rb.sample_slots(), np.int32) for _ in range(n)])
        if _covers(rb, slots, stack) and (head is None or _covers(rb, slots[:head], stack)):
            return slots
    raise AssertionError("no sampler seed below 400 draws the elements this case is about")


def _single(agent, rb, slots, dev=False):
    import torch

    from slimdqn import _hip

    frames, n_frames, frame_bytes, rows, stack = rb.ring_view()[:5]
    B = int(slots.size)
    agent._ensure_handle(max(B, 32))
    host = np.ascontiguousarray(slots, np.int32)
    keep = torch.from_numpy(host).cuda() if dev else host
    agent.__dict__.setdefault("_keep_all", []).append(keep)
    fn = _hip.lib().idqn_learn_on_replay_fc_dev if dev else _hip.lib().idqn_learn_on_replay_fc
    _hip.check(fn(agent._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows), _hip.ptr(keep) if dev else host.ctypes.data,
                  B, int(stack), B, 0, _hip.current_stream()), "idqn_learn_on_replay_fc")


def _many(agent, rb, slots, dev=False, check=True, **over):
    """The new entry on ``rb``'s ring with slots [n][B]; ``over`` replaces arguments by name (refusal tests)."""
    import torch

    from slimdqn import _hip

    frames, n_frames, frame_bytes, rows, stack = rb.ring_view()[:5]
    n, B = slots.shape
    agent._ensure_handle(max(B, 32))
    host = np.ascontiguousarray(slots, np.int32)
    keep = torch.from_numpy(host).cuda() if dev else host
    agent.__dict__.setdefault("_keep_all", []).append(keep)
    a = dict(ring=_hip.ptr(frames), n_frames=int(n_frames), frame_bytes=int(frame_bytes), rows=_hip.ptr(rows),
             slots_ptr=_hip.ptr(keep) if dev else host.ctypes.data, n_steps=n, B=B, stack=int(stack), div=B, flags=0)
    a.update(over)
    fn = _hip.lib().idqn_learn_steps_on_replay_fc_dev if dev else _hip.lib().idqn_learn_steps_on_replay_fc
    rc = fn(agent._handle, a["ring"], a["n_frames"], a["frame_bytes"], a["rows"], a["slots_ptr"], a["n_steps"], a["B"], a["stack"], a["div"],
            a["flags"], _hip.current_stream())
    if check:
        _hip.check(rc, "idqn_learn_steps_on_replay_fc")
    return rc


def _snapshot(agent, names=STATE):
    import torch

    torch.cuda.synchronize()
    return {n: getattr(agent, n).cpu().numpy().tobytes() for n in names}


def _assert_same(a, b, what=""):
    sa, sb = _snapshot(a), _snapshot(b)
    for n in STATE:
        assert sa[n] == sb[n], f"{what}: {n} differs"


def _warm(agents, rb, name):
    """Five single steps and a target sync: non-zero moments and counts, a target that differs from online."""
    B = CONFIGS[name][8]
    for agent in agents:
        for i in range(5):
            _single(agent, rb, (np.random.default_rng(90 + i).integers(0, CAPACITY, B)).astype(np.int32))
        agent._local_target_sync()
        if agent._K == 1:  # (no sync between heads: make the target differ from online some other way)
            agent._target.mul_(0.5)


_DRAWS = {}


def _case_draws(name, ring, n=32):
    """The slots of a case, drawn once per (shape, ring) and shared by its tests."""
    key = (name, ring)
    if key not in _DRAWS:
        rb = (_buffer if ring == "ring" else _vector_buffer)(name)
        _DRAWS[key] = _draws(rb, n, CONFIGS[name][3], head=7 if name.startswith("shape_") else None)
    return _DRAWS[key]


@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("ring", ["ring", "vector"])
@pytest.mark.parametrize("name", PERSISTENT)
def test_identity_persistent_route(name, ring, warm):
    """One many-call against n single calls on a twin, n in {1, 2, 7, 32}, host and device slots (cases 1 and 4)."""
    stack = CONFIGS[name][3]
    rb = (_buffer if ring == "ring" else _vector_buffer)(name)
    draws = _case_draws(name, ring)
    for n in (1, 2, 7, 32):
        slots = draws[:n] if n > 2 else draws[-n:]
        if n >= 7:
            assert _covers(rb, slots, stack), "the slots used miss the elements this case is about"
        many, many_dev, twin = _agent(name), _agent(name), _agent(name)
        if warm:
            _warm((many, many_dev, twin), rb, name)
        before = _snapshot(twin, ("_target",))["_target"]
        _many(many, rb, slots)
        _many(many_dev, rb, slots, dev=True)
        for i in range(n):
            _single(twin, rb, slots[i])
        _assert_same(many, twin, f"n = {n}")
        _assert_same(many_dev, twin, f"n = {n}, device slots")
        assert _snapshot(many, ("_target",))["_target"] == before
        assert (many._count.cpu().numpy() == n + (5 if warm else 0)).all() and np.isfinite(many._losses.cpu().numpy()).all()
        assert many._handle.value and many.__dict__.get("_replay_fc_ok") is None
        if name.startswith("shape_"):  # the launch is the persistent kernel, the twin's the ring-sourced single step
            assert _route(many) == _route(many_dev) == "k_fc_steps_par" and _route(twin) == "k_fc_step_par<ring>"


def _route(agent):
    """The kernel the handle's last MLP step launched (idqn_profile_read)."""
    import ctypes as C

    from slimdqn import _hip

    mean_ms, n_l, kernel = C.c_double(), C.c_int32(), C.create_string_buffer(64)
    _hip.check(_hip.lib().idqn_profile_read(agent._handle, C.byref(mean_ms), C.byref(n_l), kernel), "idqn_profile_read")
    return kernel.value.decode()


@pytest.mark.parametrize("name", ["lunar_b64", "fc_520", "gcnn", SHAPE_LOOP])
def test_identity_loop_route(name):
    """Handles and batches outside the one-launch plan: the entry loops over the single step (case 2)."""
    rb = _buffer(name)
    slots = _draws(rb, 3, CONFIGS[name][3])
    assert _covers(rb, slots, CONFIGS[name][3])
    many, many_dev, twin = _agent(name), _agent(name), _agent(name)
    _many(many, rb, slots)
    _many(many_dev, rb, slots, dev=True)
    for i in range(3):
        _single(twin, rb, slots[i])
    _assert_same(many, twin)
    _assert_same(many_dev, twin, "device slots")
    assert (many._count.cpu().numpy() == 3).all()
    if name == SHAPE_LOOP:  # inside fc_par_plan, 1 KB short for fc_steps_plan: every step of the loop is the one-launch step on the ring
        assert _route(many) == _route(many_dev) == _route(twin) == "k_fc_step_par<ring>"


def test_staging_blocks_are_reused_safely():
    """Twelve many-calls of 4 steps, different slots, no synchronisation in between = 48 single steps (case 3)."""
    from slimdqn import _hip

    assert _hip.STEPS_STAGING_DEPTH == 4 and 12 >= 2 * _hip.STEPS_STAGING_DEPTH + 2
    name = "lunar"
    rb = _buffer(name)
    rng = np.random.default_rng(5)
    blocks = [rng.integers(0, CAPACITY, (4, 32)).astype(np.int32) for _ in range(12)]
    many, twin = _agent(name), _agent(name)
    for b in blocks:
        host = b.copy()
        _many(many, rb, host)
        host[:] = -(2**30)  # the host slots were read before the call returned
    for b in blocks:
        for i in range(4):
            _single(twin, rb, b[i])
    _assert_same(many, twin)
    assert (many._count.cpu().numpy() == 48).all()


def test_interleaved_with_the_other_entries():
    """many-call, vectorised acting, Q-values, single step, target sync, many-call on one handle against a twin that runs the
    same sequence with single steps: state after every call, the Q rows and the actions (case 5)."""
    name = "lunar"
    rb = _buffer(name)
    draws = _case_draws(name, "ring")
    a, b = _agent(name), _agent(name)
    rng = np.random.default_rng(3)
    states = [rng.standard_normal(8).astype(np.float32) for _ in range(5)]
    heads = [0, 2, 1, 1, 0]

    def steps(agent, slots, many):
        if many:
            _many(agent, rb, slots)
        else:
            for s in slots:
                _single(agent, rb, s)

    for agent, many in ((a, True), (b, False)):
        agent.out = []
        steps(agent, draws[:5], many)
        agent.out.append(_snapshot(agent))
        acts = agent._best_actions(0, heads, states)
        agent.out.append((np.asarray(acts).tobytes(), agent._q_out[:5].cpu().numpy().tobytes(), _snapshot(agent)))
        agent.out.append((agent._q_values(1, 1, np.stack(states[:3])).cpu().numpy().tobytes(), _snapshot(agent)))
        _single(agent, rb, draws[5])
        agent.out.append(_snapshot(agent))
        agent._local_target_sync()
        agent.out.append(_snapshot(agent))
        steps(agent, draws[6:13], many)
        agent.out.append(_snapshot(agent))
    for i, (x, y) in enumerate(zip(a.out, b.out)):
        assert x == y, f"call {i} of the sequence differs"
    assert (a._count.cpu().numpy() == 13).all()


def test_eight_steps_against_the_oracle():
    """8 steps from a fresh K = 3 [100, 100] agent in one call against ``oracle/qnet_ref`` stepping the same gathered minibatches
    (case 6).  Tolerances: those ``tests/test_gpu_fp_path.py::test_ragged_batches_and_shapes_against_oracle`` applies to this net
    -- ``LOSS_ATOL`` = 1e-5 on a loss (times the number of steps on the running sum, as that file's cumulated-loss checks do)
    and 2e-5 on a parameter."""
    from oracle import qnet_ref as Q

    LOSS_ATOL, PARAM_ATOL, n = 1e-5, 2e-5, 8
    name = "lunar"
    _, _, _, _, obs, feats, K, A, B, _ = CONFIGS[name]
    rb = _buffer(name)
    slots = _case_draws(name, "ring")[:n]
    agent = _agent(name)
    p = {k: v.astype(np.float64) for k, v in agent._flat(agent._online).items()}
    pt = agent._flat(agent._target)
    mu = {k: np.zeros(v.shape, np.float64) for k, v in p.items()}
    nu = {k: np.zeros(v.shape, np.float64) for k, v in p.items()}
    count, cum, losses = np.zeros(K, np.int64), np.zeros(K), None
    for i in range(n):
        el = rb._gather(slots[i])
        batch = tuple(np.asarray(getattr(f, "tensor", f).cpu() if hasattr(getattr(f, "tensor", f), "cpu") else getattr(f, "tensor", f))
                      for f in (el.state, el.action, el.reward, el.next_state, el.is_terminal))
        batch = (batch[0].reshape(B, -1).astype(np.float32), batch[1].astype(np.int64), batch[2].astype(np.float32),
                 batch[3].reshape(B, -1).astype(np.float32), batch[4].astype(bool))
        p, mu, nu, count, losses = Q.learn_on_batch(p, pt, mu, nu, count, batch, "fc", 0.99 ** HORIZON, 1e-3, 1e-8)
        cum += losses
    _many(agent, rb, slots)
    got_l, got_c = agent._losses.cpu().numpy(), agent._cum.cpu().numpy()
    got = agent._flat(agent._online)
    perr = max(float(np.abs(got[leaf] - p[leaf]).max()) for leaf in p)
    print(f"loss err {np.abs(got_l - losses).max():.3e}, cum err {np.abs(got_c - cum).max():.3e}, param err {perr:.3e}")
    assert np.abs(got_l - losses).max() <= LOSS_ATOL
    assert np.abs(got_c - cum).max() <= LOSS_ATOL * n
    assert perr <= PARAM_ATOL
    assert (agent._count.cpu().numpy() == n).all()


def test_refusals_enqueue_nothing():
    """Every documented refusal answers ``E_INVALID`` with a message and leaves every state array's bytes unchanged (case 7)."""
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN
    from slimdqn.networks.iiqn import iIQN

    rb_fc, rb_cnn = _buffer("lunar"), _buffer("gcnn")
    fc, per, gcnn = _agent("lunar"), _agent("lunar"), _agent("gcnn")
    plane = iDQN(0, (20, 20, 4), 5, 2, [32, 32, 32, 128], "cnn", 6.25e-5, 0.99, HORIZON, 1, 10**9, 10**9, adam_eps=1.5e-4)
    quant = iIQN(3, (20, 20, 4), 5, 2, [32, 32, 32, 256], "cnn", 6.25e-5, 0.99, HORIZON, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=4)
    rng = np.random.default_rng(1)
    s32, s5 = rng.integers(0, CAPACITY, (3, 32)).astype(np.int32), rng.integers(0, CAPACITY, (3, 5)).astype(np.int32)
    for agent in (fc, per, gcnn, plane, quant):
        agent._ensure_handle(32)
        agent._grad.fill_(-7.25)
        agent._mu.fill_(0.5)
    w, td = torch.ones(32, device="cuda"), torch.zeros(3 * 32, device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(per._handle, _hip.ptr(w), _hip.ptr(td)), "idqn_set_per_buffers")
    cases = [
        ("n_steps 0", fc, rb_fc, s32, dict(n_steps=0)),
        ("n_steps 33", fc, rb_fc, s32, dict(n_steps=33)),
        ("flags", fc, rb_fc, s32, dict(flags=_hip.F_GRADS_ONLY)),
        ("profile flag", fc, rb_fc, s32, dict(flags=_hip.F_PROFILE)),
        ("prioritized-replay buffers", per, rb_fc, s32, {}),
        ("null slots", fc, rb_fc, s32, dict(slots_ptr=None)),
        ("null slots (device)", fc, rb_fc, s32, dict(slots_ptr=None, dev=True)),
        ("a null ring", fc, rb_fc, s32, dict(ring=None)),
        ("a null row table", gcnn, rb_cnn, s5, dict(rows=None)),
        ("batch 0", fc, rb_fc, s32, dict(B=0)),
        ("batch max_batch + 1", fc, rb_fc, s32, dict(B=33, div=33)),
        ("a mean divisor below the batch", fc, rb_fc, s32, dict(div=31)),
        ("a wrong frame_bytes (fc)", fc, rb_fc, s32, dict(frame_bytes=28)),
        ("a wrong stack (fc)", fc, rb_fc, s32, dict(stack=2)),
        ("a wrong stack (cnn)", gcnn, rb_cnn, s5, dict(stack=3)),
        ("a wrong frame_bytes (cnn)", gcnn, rb_cnn, s5, dict(frame_bytes=119)),
        ("a plane-path handle", plane, rb_cnn, s5, {}),
        ("a quantile handle", quant, rb_cnn, s5, {}),
    ]
    for what, agent, rb, slots, over in cases:
        assert agent._handle_batch == 32
        before = _snapshot(agent)
        dev = over.pop("dev", False)
        rc = _many(agent, rb, slots, dev=dev, check=False, **over)
        assert rc == _hip.E_INVALID, f"{what}: answered {rc}"
        assert _hip.lib().idqn_last_error(), what
        assert _snapshot(agent) == before, f"{what}: the refused call changed the agent's state"


def test_update_params_many_is_the_loop():
    """``update_params_many(first, 40, rb)`` with update_to_data 2, target update every 12, sync every 5 against the loop on a
    twin: state, target, returned logs and the sampler generator's state (case 8)."""
    name = "lunar"
    rb_a, rb_b = _buffer(name, seed=4), _buffer(name, seed=4)
    a, b = _agent(name, utd=2, tuf=12, tsf=5), _agent(name, utd=2, tuf=12, tsf=5)
    a.learn_steps_min = 1  # (runs of 2 and 3 gradient steps: below the default threshold of the one-call route)
    first = 7
    got = a.update_params_many(first, 40, rb_a)
    want = []
    for s in range(first, first + 40):
        b.update_online_params(s, rb_b)
        updated, logs = b.update_target_params(s)
        if updated:
            want.append((s, logs))
    assert a.__dict__.get("_learn_steps_ok") is True, "the one-call route did not run"
    _assert_same(a, b)
    assert [s for s, _ in got] == [s for s, _ in want] == [12, 24, 36]
    for (_, x), (_, y) in zip(got, want):
        assert x.keys() == y.keys() and all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x)
    assert rb_a._sampling_distribution._rng_key.bit_generator.state == rb_b._sampling_distribution._rng_key.bit_generator.state
    assert (a._count.cpu().numpy() == 20).all()


def test_vector_trainer_fused_equals_loop():
    """``VectorTrainer`` on the synthetic environment, E = 4, two short epochs, ``fuse_gradient_steps`` True and False: returns,
    lengths, logged records and final state (case 8)."""
    from experiments.base.dqn import VectorTrainer
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    class Log:
        def __init__(self):
            self.records = []

        def log(self, d):
            self.records.append({k: np.asarray(v).tobytes() for k, v in d.items()})

    def run(fuse):
        envs = [SyntheticVector(e, dim=8, n_actions=4, episode_length=(9, 6, 11, 7)[e]) for e in range(4)]
        agent = iDQN(1, 8, 4, 3, [100, 100], "fc", 1e-3, 0.99, 1, 1, 24, 5)
        agent.learn_steps_min = 1  # (E = 4: runs of at most 4 gradient steps, below the default threshold of the one-call route)
        rb = VectorReplayBuffer(UniformSamplingDistribution(2), 32, 4000, stack_size=1, update_horizon=1, gamma=0.99, n_envs=4)
        p = dict(epsilon_end=0.05, epsilon_duration=30, n_epochs=2, n_training_steps_per_epoch=80, n_initial_samples=40, horizon=1000,
                 wandb=Log(), fuse_gradient_steps=fuse)
        t = VectorTrainer(prng.PRNGKey(1), p, agent, envs, rb)
        out = t.run()
        return out, p["wandb"].records, _snapshot(agent), t.total_steps, agent

    (out_a, rec_a, st_a, n_a, ag), (out_b, rec_b, st_b, n_b, _) = run(True), run(False)
    assert ag.__dict__.get("_learn_steps_ok") is True, "the one-call route did not run"
    assert out_a == out_b and n_a == n_b and rec_a == rec_b and st_a == st_b
    assert sum("loss" in r for r in rec_a) >= 3

