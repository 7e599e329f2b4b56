"""GPU: n prioritized learner steps as one call -- ``idqn_per_learn_steps_on_replay`` and the layers on top of it
(``PrioritizedLearner.steps`` / ``update_params_many``, ``VectorTrainer(learner=...)``).

Every comparison is ``tobytes()`` equality against n calls of ``idqn_per_learn_on_replay`` on a twin built from the same bytes
(the same arenas, the same tree, the same rows of uniforms): parameters, both moments, count, losses, ``cum_losses``, the node
array, the running maximum and EVERY step's row of leaves, weights, |TD| and priorities.  On the parent commit the entry and
the methods do not exist.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#          arch   frame shape  dtype      stack obs            features            K  A  N
FAMILIES = {
    "lunar": ("fc", (8,), np.float32, 1, 8, [100, 100], 3, 4, 0),              # the LunarLander net
    "fc520": ("fc", (8,), np.float32, 1, 8, [520], 3, 4, 0),
    "gcnn": ("cnn", (20, 20), np.uint8, 4, (20, 20, 4), [2, 3, 1, 15], 2, 6, 0),  # general-shape conv path
    "plane": ("cnn", (84, 84), np.uint8, 4, (84, 84, 4), [32, 64, 64, 512], 2, 6, 0),
    "plane_small": ("cnn", (20, 20), np.uint8, 4, (20, 20, 4), [32, 32, 32, 128], 2, 5, 0),
    "iqn": ("cnn", (20, 20), np.uint8, 4, (20, 20, 4), [32, 32, 32, 256], 2, 5, 4),
}
CAPACITY = 64  # small: a step resamples leaves the step before it rewrote
AGENT_STATE = ("_online", "_mu", "_nu", "_count", "_losses", "_cum")
LEARNER_STATE = ("_leaves", "_weights", "_td_abs", "_priorities")


def _agent(family):
    from slimdqn.networks.idqn import iDQN
    from slimdqn.networks.iiqn import iIQN

    arch, _, _, _, obs, feats, K, A, N = FAMILIES[family]
    if N:
        return iIQN(0, obs, A, K, feats, "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9, adam_eps=1e-8, n_quantiles=N)
    return iDQN(0, obs, A, K, feats, arch, 1e-3, 0.99, 1, 1, 10**9, 10**9)


def _frame(rng, shape, dtype):
    return rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else rng.standard_normal(shape).astype(np.float32)


def _learner(family, B):
    """A ``PrioritizedLearner`` on a wrapped ring of 64 elements with episode ends, priorities included."""
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement

    _, shape, dtype, stack, _, _, _, A, _ = FAMILIES[family]
    rng = np.random.default_rng(17)
    rb = ReplayBuffer(SlotPrioritizedSampler(4, CAPACITY), batch_size=B, max_capacity=CAPACITY, stack_size=stack, update_horizon=1, gamma=0.99)
    for i in range(150):
        rb.add(TransitionElement(_frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), i % 7 == 6, i % 7 == 6),
               **({"priority": float(rng.random() + 0.1)} if i % 3 else {}))
    rb.reuse_sample_buffers = True
    learner = PrioritizedLearner(_agent(family), rb, beta=0.5, eps=1e-3)
    learner.agent._ensure_handle(B)
    return learner


class _Rows:
    """The per-step output rows of one side: leaves, weights, |TD|, priorities, [n] of each."""

    def __init__(self, n, K, B):
        import torch

        self.leaves = torch.full((n, B), -7, dtype=torch.int32, device="cuda")
        self.weights = torch.full((n, B), -7.0, dtype=torch.float32, device="cuda")
        self.td = torch.full((n, K, B), -7.0, dtype=torch.float32, device="cuda")
        self.pri = torch.full((n, B), -7.0, dtype=torch.float64, device="cuda")

    def all(self):
        return {"leaves": self.leaves, "weights": self.weights, "td": self.td, "priorities": self.pri}


def _fill(p, learner, rows, i=None, with_pri=True):
    tree = learner.sampler._sum_tree
    pick = (lambda t: t) if i is None else (lambda t: t[i])
    p.nodes_dev, p.depth, p.n_items = tree._nodes_dev.data_ptr(), tree._depth, len(learner.sampler)
    p.stratified, p.reduce_max, p.beta, p.eps, p.alpha = 1, 0, learner.beta, learner.eps, learner.sampler._alpha
    p.max_priority_dev = learner.sampler._max_priority_dev.data_ptr()
    p.leaves_dev, p.weights_dev, p.td_abs_dev = pick(rows.leaves).data_ptr(), pick(rows.weights).data_ptr(), pick(rows.td).data_ptr()
    p.priorities_dev = pick(rows.pri).data_ptr() if with_pri else None
    p.tree_scratch_dev = tree._scratch.data_ptr()


def _steps_call(learner, U, rows, B, flags=0, handle=None, n_steps=None, stack=None, with_pri=True, **fields):
    """``idqn_per_learn_steps_on_replay`` on the rows of ``U``; arguments replaced by name for the refusal tests."""
    from slimdqn import _hip

    frames, n_frames, frame_bytes, ring_rows, stk = learner.rb.ring_view()[:5]
    p = _hip.PerSteps()
    _fill(p, learner, rows, with_pri=with_pri)
    p.uniforms_host = U.ctypes.data
    for k, v in fields.items():
        setattr(p, k, v)
    return _hip.lib().idqn_per_learn_steps_on_replay(learner.agent._handle if handle is None else handle, C.byref(p), _hip.ptr(frames),
                                                     int(n_frames), int(frame_bytes), _hip.ptr(ring_rows), len(U) if n_steps is None else n_steps,
                                                     B, int(stk if stack is None else stack), B, flags, _hip.current_stream())


def _single_calls(learner, U, rows, B, with_pri=True):
    """n calls of ``idqn_per_learn_on_replay``, call i on row i of ``U`` and of the outputs."""
    from slimdqn import _hip

    frames, n_frames, frame_bytes, ring_rows, stk = learner.rb.ring_view()[:5]
    for i in range(len(U)):
        p = _hip.PerStep()
        _fill(p, learner, rows, i, with_pri)
        p.uniforms_host, p.tau_dev = U[i].ctypes.data, None
        _hip.check(_hip.lib().idqn_per_learn_on_replay(learner.agent._handle, C.byref(p), _hip.ptr(frames), int(n_frames), int(frame_bytes),
                                                       _hip.ptr(ring_rows), B, int(stk), B, 0, _hip.current_stream()), "idqn_per_learn_on_replay")


def _state(learner, rows=None):
    """Device-side copies (no host synchronisation) of everything the contract names."""
    out = {n: getattr(learner.agent, n).clone() for n in AGENT_STATE}
    out["nodes"] = learner.sampler._sum_tree._nodes_dev.clone()
    out["max_priority"] = learner.sampler._max_priority_dev.clone()
    if rows is not None:
        out.update({k: v.clone() for k, v in rows.all().items()})
    return out


def _assert_equal(a, b, tag):
    assert a.keys() == b.keys()
    for n in a:
        assert a[n].cpu().numpy().tobytes() == b[n].cpu().numpy().tobytes(), (tag, n)


def _uniforms(rng, n, B):
    U = rng.random((n, B))
    U[rng.integers(n), rng.integers(B)] = 0.0
    U[rng.integers(n), rng.integers(B)] = np.nextafter(1.0, 0.0)
    return U


@pytest.mark.parametrize("family,B,ns", [("lunar", 1, (1, 2, 5, 32)), ("lunar", 5, (1, 2, 5, 32)), ("lunar", 32, (1, 2, 5, 32)),
                                         ("fc520", 32, (3,)), ("lunar", 33, (2,)), ("gcnn", 4, (3,)), ("plane", 32, (2,))])
def test_the_call_equals_n_single_calls(family, B, ns):
    """One pair of twins per row of the table; the calls for the n of a row follow each other on the state the one before left,
    with no synchronisation between them on the side of the new call."""
    import torch

    K = FAMILIES[family][6]
    one, chain = _learner(family, B), _learner(family, B)
    rng = np.random.default_rng(100 * B + len(ns))
    draws = [_uniforms(rng, n, B) for n in ns]
    got = []
    for U in draws:
        rows = _Rows(len(U), K, B)
        _steps_call_checked(one, U, rows, B)
        got.append(_state(one, rows))
    rewritten = False
    for U, want in zip(draws, got):
        rows = _Rows(len(U), K, B)
        _single_calls(chain, U, rows, B)
        torch.cuda.synchronize()
        _assert_equal(_state(chain, rows), want, (family, B, len(U)))
        leaves = rows.leaves.cpu().numpy()
        rewritten |= any(np.isin(leaves[i + 1], leaves[i]).any() for i in range(len(U) - 1))
        assert (rows.td.cpu().numpy() >= 0).all() and (rows.pri.cpu().numpy() > 0).all() and (rows.weights.cpu().numpy() <= 1).all()
    total = sum(ns)
    assert (chain.agent._count.cpu().numpy() == total).all() and np.isfinite(chain.agent._losses.cpu().numpy()).all()
    if B * max(ns) >= CAPACITY:
        assert rewritten, "no step resampled a leaf the step before it rewrote"


def _steps_call_checked(learner, U, rows, B, **kw):
    from slimdqn import _hip

    _hip.check(_steps_call(learner, U, rows, B, **kw), "idqn_per_learn_steps_on_replay")


def test_priorities_may_be_null():
    import torch

    one, chain = _learner("lunar", 32), _learner("lunar", 32)
    U = _uniforms(np.random.default_rng(2), 3, 32)
    ra, rb = _Rows(3, 3, 32), _Rows(3, 3, 32)
    _steps_call_checked(one, U, ra, 32, with_pri=False)
    _single_calls(chain, U, rb, 32, with_pri=False)
    torch.cuda.synchronize()
    _assert_equal(_state(one, ra), _state(chain, rb), "no priorities")
    assert (ra.pri == -7.0).all().item()


def test_the_profile_table_lists_the_launches():
    """n steps of the one-launch MLP step: n step launches, n - 1 k_per_turn, one k_per_draw, one k_per_write_back."""
    import torch

    from slimdqn import _hip

    n, B = 5, 32
    one, chain = _learner("lunar", B), _learner("lunar", B)
    U = _uniforms(np.random.default_rng(8), n, B)
    ra, rb = _Rows(n, 3, B), _Rows(n, 3, B)
    _steps_call_checked(one, U, ra, B, flags=_hip.F_PROFILE_ALL)
    buf = C.create_string_buffer(8192)
    _hip.check(_hip.lib().idqn_profile_table(one.agent._handle, buf, 8192), "idqn_profile_table")
    table = {ln.split("\t")[0]: int(ln.split("\t")[2]) for ln in buf.value.decode().splitlines()}
    per = {k: v for k, v in table.items() if k.startswith("k_per_")}
    step = {k: v for k, v in table.items() if not k.startswith("k_per_")}
    assert per == {"k_per_draw": 1, "k_per_turn": n - 1, "k_per_write_back": 1}, table
    assert list(step.values()) == [n] and next(iter(step)).startswith("k_fc_step_par"), table
    _single_calls(chain, U, rb, B)
    torch.cuda.synchronize()
    _assert_equal(_state(one, ra), _state(chain, rb), "profiled")


def test_staging_blocks_are_reused_safely():
    """More calls than staging blocks on one handle with no synchronisation between them, the caller's uniforms overwritten
    right after each return."""
    import torch

    from slimdqn import _hip

    n, B = 3, 32
    one, chain = _learner("lunar", B), _learner("lunar", B)
    rng = np.random.default_rng(9)
    draws = [_uniforms(rng, n, B) for _ in range(2 * _hip.STEPS_STAGING_DEPTH + 1)]
    ra, rb = _Rows(n, 3, B), _Rows(n, 3, B)
    U = np.empty((n, B))
    for d in draws:
        U[:] = d
        _steps_call_checked(one, U, ra, B)
        U[:] = 0.5
    for d in draws:
        _single_calls(chain, d, rb, B)
    torch.cuda.synchronize()
    _assert_equal(_state(one, ra), _state(chain, rb), "staging")


def test_refusals_leave_everything_untouched():
    import torch

    from slimdqn import _hip

    B, n = 32, 3
    one, chain, iqn = _learner("lunar", B), _learner("lunar", B), _learner("iqn", B)
    U = _uniforms(np.random.default_rng(4), n, B)
    rows, rows_iqn = _Rows(n, 3, B), _Rows(n, 2, B)
    before = _state(one, rows)
    lib = _hip.lib()
    cases = [
        (dict(n_steps=0), "n_steps 0"), (dict(n_steps=_hip.MAX_STEPS_PER_CALL + 1), "n_steps 33"),
        (dict(stack=3), "stack 3"),                                  # what the dispatched entry refuses
        (dict(weights_dev=None), "null pointer"), (dict(td_abs_dev=None), "null pointer"),
        (dict(nodes_dev=None), "null pointer"), (dict(uniforms_host=None), "null pointer"), (dict(leaves_dev=None), "null pointer"),
        (dict(tree_scratch_dev=None), "null pointer"),
        (dict(B=0), "batch 0"), (dict(B=257), "batch 257"),
        (dict(depth=0), "depth"), (dict(depth=32), "depth"),
        (dict(n_items=0), "n_items"),
        (dict(flags=_hip.F_GRADS_ONLY), "profile flags"), (dict(flags=_hip.F_STOP_AFTER_DENSE0 | _hip.F_PROFILE), "profile flags"),
    ]
    for kw, match in cases:
        kw = dict(kw)
        rc = _steps_call(one, U, rows, kw.pop("B", B), **kw)
        msg = lib.idqn_last_error().decode()
        assert rc == _hip.E_INVALID and msg.startswith("idqn_per_learn_steps_on_replay:") and match in msg, (kw, rc, msg)
    rc = _steps_call(iqn, U, rows_iqn, B)  # quantile heads
    msg = lib.idqn_last_error().decode()
    assert rc == _hip.E_INVALID and msg.startswith("idqn_per_learn_steps_on_replay:") and "quantile heads" in msg, (rc, msg)
    _hip.check(lib.idqn_set_per_buffers(one.agent._handle, _hip.ptr(one._weights), _hip.ptr(one._td_abs)), "idqn_set_per_buffers")
    assert _steps_call(one, U, rows, B) == _hip.E_INVALID and "idqn_set_per_buffers" in lib.idqn_last_error().decode()
    _hip.check(lib.idqn_set_per_buffers(one.agent._handle, None, None), "idqn_set_per_buffers")
    torch.cuda.synchronize()
    _assert_equal(before, _state(one, rows), "after the refusals")
    # the next valid call gives the single calls' result
    _steps_call_checked(one, U, rows, B)
    rows_chain = _Rows(n, 3, B)
    _single_calls(chain, U, rows_chain, B)
    torch.cuda.synchronize()
    _assert_equal(_state(one, rows), _state(chain, rows_chain), "after a valid call")


# ---- the Python layers ---------------------------------------------------------------------------------------------------
def _snapshot(learner):
    out = {n: getattr(learner.agent, n).clone() for n in AGENT_STATE}
    out.update({n: getattr(learner, n).clone() for n in LEARNER_STATE})
    out["nodes"] = learner.sampler._sum_tree._nodes_dev.clone()
    out["max_priority"] = learner.sampler._max_priority_dev.clone()
    return out


def _on(learner):
    """The n-step route, whatever defaults the measurements gave its family."""
    learner.fuse_per_family = dict.fromkeys(learner.fuse_per_family, True)
    learner.fuse_per_steps_family = dict.fromkeys(learner.fuse_per_steps_family, True)
    learner.per_steps_min = 2
    return learner


@pytest.mark.parametrize("family", ["lunar", "plane_small"])
def test_learner_steps_equals_seven_step_calls(family):
    import torch

    many, single = _on(_learner(family, 32)), _on(_learner(family, 32))
    many.steps(7)
    for _ in range(7):
        single.step()
    torch.cuda.synchronize()
    assert many.__dict__.get("_steps_ok") is True and single.__dict__.get("_steps_ok") is None, "the wrong route ran"
    _assert_equal(_snapshot(many), _snapshot(single), family)
    assert many.sampler._rng_key.bit_generator.state == single.sampler._rng_key.bit_generator.state
    assert (many.agent._count.cpu().numpy() == 7).all()
    # a single step after the call goes on from the call's rows, and a run past MAX_STEPS_PER_CALL splits
    many.step(), single.step()
    many.steps(35)
    for _ in range(35):
        single.step()
    torch.cuda.synchronize()
    _assert_equal(_snapshot(many), _snapshot(single), (family, "continued"))
    assert many.sampler._rng_key.bit_generator.state == single.sampler._rng_key.bit_generator.state


def test_vector_trainer_with_a_learner_fused_equals_loop():
    """``VectorTrainer(learner=...)`` on the synthetic environment, E = 4, two short epochs, ``fuse_gradient_steps`` True and
    False: returns, lengths, logged records, parameters, moments and the tree."""
    from experiments.base.dqn import VectorTrainer
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    class Log:
        def __init__(self):
            self.records = []

        def log(self, d):
            self.records.append({k: np.asarray(v).tobytes() for k, v in d.items()})

    def run(fuse):
        envs = [SyntheticVector(e, dim=8, n_actions=4, episode_length=(9, 6, 11, 7)[e]) for e in range(4)]
        agent = iDQN(1, 8, 4, 3, [100, 100], "fc", 1e-3, 0.99, 1, 1, 24, 5)
        rb = VectorReplayBuffer(SlotPrioritizedSampler(2, 4096), 32, 4096, stack_size=1, update_horizon=1, gamma=0.99, n_envs=4)
        learner = _on(PrioritizedLearner(agent, rb, beta=0.5, eps=1e-3))
        p = dict(epsilon_end=0.05, epsilon_duration=30, n_epochs=2, n_training_steps_per_epoch=150, n_initial_samples=40, horizon=1000,
                 wandb=Log(), fuse_gradient_steps=fuse)
        t = VectorTrainer(prng.PRNGKey(1), p, agent, envs, rb, learner=learner)
        out = t.run()
        state = {k: v.cpu().numpy().tobytes() for k, v in _snapshot(learner).items()}
        return out, p["wandb"].records, state, t.total_steps, learner

    (out_a, rec_a, st_a, n_a, la), (out_b, rec_b, st_b, n_b, lb) = run(True), run(False)
    assert la.__dict__.get("_steps_ok") is True and lb.__dict__.get("_steps_ok") is None, "the wrong route ran"
    assert n_a == n_b >= 300 and out_a == out_b and rec_a == rec_b
    assert st_a.keys() == st_b.keys() and all(st_a[k] == st_b[k] for k in st_a), [k for k in st_a if st_a[k] != st_b[k]]
    assert la.sampler._rng_key.bit_generator.state == lb.sampler._rng_key.bit_generator.state
    assert sum("loss" in r for r in rec_a) >= 3
