"""GPU: the prioritized learner step as one call -- ``per_draw``, ``per_write_back`` and ``idqn_per_learn_on_replay``.

Every comparison is ``tobytes()`` equality against the entries the chain of ``PrioritizedLearner`` issues (``per_sample_leaves``
+ ``per_importance_weights``; ``per_priorities_from_td`` + ``sumtree_set``; the whole chain) on a twin tree / twin handle built
from the same bytes.  On the parent commit the three entries do not exist.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPACITIES = [1, 2, 5, 37, 1024, 2**16]
NS = [1, 31, 32, 33, 64, 255, 256]
U_EDGE = [0.0, np.nextafter(1.0, 0.0)]


def _depth(capacity):
    return int(np.ceil(np.log2(capacity))) + 1


def _host_tree(capacity, kind, seed=0):
    """Node array (host, float64) of a tree of ``capacity`` leaves and the item count the draws are clamped to."""
    from oracle.sumtree_ref import SumTreeRef

    rng = np.random.default_rng(1000 * seed + capacity)
    ref = SumTreeRef(capacity)
    val = rng.random(capacity) + 0.05
    n_items = capacity
    if kind == "zero_leaves":
        val[rng.random(capacity) < 0.4] = 0.0
    elif kind == "all_zero":
        val[:] = 0.0
    elif kind == "mass_past_items":  # live leaves hold little, the leaves at and past n_items the rest: the clamp
        n_items = max(1, capacity // 2)
        val[:n_items] *= 1e-3
    for lo in range(0, capacity, 4096):
        ref.set(np.arange(lo, min(lo + 4096, capacity), dtype=np.int32), val[lo : lo + 4096])
    return np.ascontiguousarray(ref.nodes, np.float64), n_items


def _uniforms(rng, n):
    u = rng.random(n)
    u[rng.integers(n)] = U_EDGE[0]
    u[rng.integers(n)] = U_EDGE[1]
    return u


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_per_draw_equals_sample_then_weights(capacity):
    import torch

    from slimdqn import _hip

    lib, q, depth = _hip.lib(), _hip.current_stream(), _depth(capacity)
    rng = np.random.default_rng(capacity)
    clamped = False
    for kind in ("random", "zero_leaves", "all_zero", "mass_past_items"):
        nodes_h, n_items = _host_tree(capacity, kind)
        nodes = _dev(nodes_h)
        for n in NS:
            for stratified in (1, 0):
                u = _dev(_uniforms(rng, n))
                la, wa = torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
                lb, wb = la.clone(), wa.clone()
                _hip.check(lib.per_sample_leaves(_hip.ptr(nodes), depth, _hip.ptr(u), n, stratified, _hip.ptr(la), q), "per_sample_leaves")
                raw = la.clone()
                _hip.check(lib.per_importance_weights(_hip.ptr(nodes), depth, _hip.ptr(la), n, n_items, 0.4, _hip.ptr(wa), q),
                           "per_importance_weights")
                _hip.check(lib.per_draw(_hip.ptr(nodes), depth, _hip.ptr(u), n, stratified, n_items, 0.4, _hip.ptr(lb), _hip.ptr(wb), q),
                           "per_draw")
                torch.cuda.synchronize()
                tag = (capacity, kind, n, stratified)
                assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes(), tag
                assert wa.cpu().numpy().tobytes() == wb.cpu().numpy().tobytes(), tag
                assert nodes.cpu().numpy().tobytes() == nodes_h.tobytes(), tag
                clamped |= bool((raw != la).any().item())
                if kind == "all_zero":
                    assert (lb == 0).all().item() and (wb == 1.0).all().item(), tag
                if capacity <= 37 and n > capacity:
                    assert len(set(lb.cpu().numpy().tolist())) < n  # duplicate leaves
    if capacity >= 5:
        assert clamped, "no draw landed at or past the item count: the clamp was not reached"


def _leaf_sets(rng, capacity, n):
    yield "unsorted", rng.integers(0, capacity, n)  # duplicates once n approaches the capacity
    yield "with_duplicates", np.concatenate([rng.integers(0, capacity, n - n // 2), rng.integers(0, capacity, 1).repeat(n // 2)])
    yield "all_equal", np.full(n, rng.integers(0, capacity))


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_per_write_back_equals_priorities_then_set(capacity):
    import torch

    from slimdqn import _hip

    lib, q, depth = _hip.lib(), _hip.current_stream(), _depth(capacity)
    rng = np.random.default_rng(7 * capacity + 1)
    nodes_h, _ = _host_tree(capacity, "zero_leaves", seed=1)
    scratch_a, scratch_b = (torch.empty(8192, dtype=torch.float64, device="cuda") for _ in range(2))
    case = 0
    for n in NS:
        for name, leaves_h in _leaf_sets(rng, capacity, n):
            case += 1
            K = (1, 3, 5)[case % 3]
            reduce_max, with_max, with_out = case % 2, (case // 2) % 2, (case // 3) % 2 if case > 4 else 1
            td_h = (rng.random((K, n)) * 3.0).astype(np.float32)
            td_h[:, rng.integers(n)] = 0.0
            td_h[rng.integers(K), rng.integers(n)] = 0.0
            leaves, td = _dev(leaves_h.astype(np.int32)), _dev(td_h)
            na, nb = _dev(nodes_h), _dev(nodes_h)
            ma, mb = (torch.full((1,), 1.0, dtype=torch.float64, device="cuda") for _ in range(2))
            pa, pb = (torch.full((n,), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
            _hip.check(lib.per_priorities_from_td(_hip.ptr(td), K, n, reduce_max, 1e-3, 0.6, _hip.ptr(pa), _hip.ptr(ma) if with_max else None, q),
                       "per_priorities_from_td")
            _hip.check(lib.sumtree_set(_hip.ptr(na), depth, _hip.ptr(leaves), _hip.ptr(pa), n, _hip.ptr(scratch_a), q), "sumtree_set")
            _hip.check(lib.per_write_back(_hip.ptr(nb), depth, _hip.ptr(leaves), _hip.ptr(td), K, n, reduce_max, 1e-3, 0.6,
                                          _hip.ptr(pb) if with_out else None, _hip.ptr(mb) if with_max else None, _hip.ptr(scratch_b), q),
                       "per_write_back")
            torch.cuda.synchronize()
            tag = (capacity, n, name, K, reduce_max, with_max, with_out)
            assert na.cpu().numpy().tobytes() == nb.cpu().numpy().tobytes(), tag
            assert ma.cpu().numpy().tobytes() == mb.cpu().numpy().tobytes(), tag
            if with_out:
                assert pa.cpu().numpy().tobytes() == pb.cpu().numpy().tobytes(), tag
            else:
                assert (pb == -1.0).all().item(), tag
            assert na.cpu().numpy().tobytes() != nodes_h.tobytes(), tag  # the set changed the tree


# ---- the whole call ------------------------------------------------------------------------------------------------------
#         kind     frame shape  dtype       stack obs             features            K  A   N
FAMILIES = {
    "mlp": ("fc", (8,), np.float32, 1, 8, [16, 16], 2, 4, 0),
    "gcnn": ("cnn", (20, 20), np.uint8, 1, (20, 20, 1), [8, 8, 8], 3, 40, 0),
    "plane": ("cnn", (20, 20), np.uint8, 4, (20, 20, 4), [32, 32, 32, 128], 2, 5, 0),
    "iqn": ("cnn", (20, 20), np.uint8, 4, (20, 20, 4), [32, 32, 32, 256], 2, 5, 4),
}
CAPACITY = 40
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


def _learner(family, B, vector=False, n_add=150, **kw):
    """A ``PrioritizedLearner`` on a wrapped ring of 40 elements with episode ends, priorities included."""
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    _, shape, dtype, stack, _, _, _, A, _ = FAMILIES[family]
    rng = np.random.default_rng(17)
    if vector:
        rb = VectorReplayBuffer(SlotPrioritizedSampler(4, CAPACITY), B, CAPACITY, stack_size=stack, update_horizon=1, gamma=0.99, n_envs=3,
                                segment=24)
        for i in range(24 * 3 + 3):
            rb.add_many([TransitionElement(_frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), (i + e) % 7 == 6, (i + e) % 7 == 6)
                         for e in range(3)])
    else:
        rb = ReplayBuffer(SlotPrioritizedSampler(4, CAPACITY), batch_size=B, max_capacity=CAPACITY, stack_size=stack, update_horizon=1, gamma=0.99)
        for i in range(n_add):
            rb.add(TransitionElement(_frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), i % 7 == 6, i % 7 == 6),
                   **({"priority": float(rng.random() + 0.1)} if i % 3 else {}))
    rb.reuse_sample_buffers = True
    assert rb.add_count > CAPACITY
    return PrioritizedLearner(_agent(family), rb, beta=0.5, eps=1e-3, **kw)


def _snapshot(learner):
    """Device-side copies (no host synchronisation) of everything the contract names."""
    out = {n: getattr(learner.agent, n).clone() for n in AGENT_STATE}
    out.update({n: getattr(learner, n).clone() for n in LEARNER_STATE})
    out["nodes"] = learner.sampler._sum_tree._nodes_dev.clone()
    out["max_priority"] = learner.sampler._max_priority_dev.clone()
    return out


def _assert_snapshots_equal(a, b, tag):
    for n in a:
        assert a[n].cpu().numpy().tobytes() == b[n].cpu().numpy().tobytes(), (tag, n)


def _fused(learner, u, taus=None):
    from slimdqn import _hip

    _hip.check(learner._step_fused(learner.rb.ring_view(), u, taus), "idqn_per_learn_on_replay")


def _draws(family, B, steps, seed=3):
    rng = np.random.default_rng(seed)
    K, N = FAMILIES[family][6], FAMILIES[family][8]
    return [(rng.random(B), rng.random((K, 3, N, B)).astype(np.float32) * 0.98 + 0.01 if N else None) for _ in range(steps)]


@pytest.mark.parametrize("family,B,vector", [("mlp", 32, False), ("mlp", 32, True), ("mlp", 33, False), ("gcnn", 33, False),
                                             ("plane", 32, False), ("plane", 33, False), ("iqn", 32, False)])
def test_whole_call_equals_the_chain(family, B, vector):
    import torch

    fused, chain = _learner(family, B, vector), _learner(family, B, vector)
    draws = _draws(family, B, 3)
    got = []
    for u, taus in draws:  # back to back: nothing here waits for the device
        _fused(fused, u, taus)
        got.append(_snapshot(fused))
    for step, (u, taus) in enumerate(draws):
        chain._step_chain(u.copy(), taus)
        torch.cuda.synchronize()
        _assert_snapshots_equal(_snapshot(chain), got[step], (family, B, vector, step))
    assert (chain.agent._count.cpu().numpy() == 3).all() and np.isfinite(chain.agent._losses.cpu().numpy()).all()
    assert (got[2]["_td_abs"] > 0).any().item()


def test_staging_blocks_are_reused_safely():
    """More calls than staging blocks, the caller's uniforms overwritten right after each return."""
    import torch

    from slimdqn import _hip

    fused, chain = _learner("mlp", 32), _learner("mlp", 32)
    draws = _draws("mlp", 32, 2 * _hip.STEPS_STAGING_DEPTH + 1)
    u = np.empty(32)
    for d, _ in draws:
        u[:] = d
        _fused(fused, u)
        u[:] = 0.5
    for d, _ in draws:
        chain._step_chain(d)
    torch.cuda.synchronize()
    _assert_snapshots_equal(_snapshot(chain), _snapshot(fused), "staging")


def _raw_call(learner, u, B, taus_dev=None, handle=None, flags=0, stack=None, **fields):
    """``idqn_per_learn_on_replay`` with arguments replaced by name (refusal tests)."""
    from slimdqn import _hip

    rb, tree, agent = learner.rb, learner.sampler._sum_tree, learner.agent
    frames, n_frames, frame_bytes, rows, stk = rb.ring_view()[:5]
    p = _hip.PerStep()
    p.nodes_dev, p.depth, p.n_items = tree._nodes_dev.data_ptr(), tree._depth, len(learner.sampler)
    p.uniforms_host = u.ctypes.data
    p.stratified, p.reduce_max, p.beta, p.eps, p.alpha = 1, 0, learner.beta, learner.eps, learner.sampler._alpha
    p.max_priority_dev = learner.sampler._max_priority_dev.data_ptr()
    p.leaves_dev, p.weights_dev, p.td_abs_dev = learner._leaves.data_ptr(), learner._weights.data_ptr(), learner._td_abs.data_ptr()
    p.priorities_dev, p.tree_scratch_dev = learner._priorities.data_ptr(), tree._scratch.data_ptr()
    p.tau_dev = None if taus_dev is None else taus_dev.data_ptr()
    for k, v in fields.items():
        setattr(p, k, v)
    return _hip.lib().idqn_per_learn_on_replay(agent._handle if handle is None else handle, C.byref(p), _hip.ptr(frames), int(n_frames),
                                               int(frame_bytes), _hip.ptr(rows), B, int(stk if stack is None else stack), B, flags,
                                               _hip.current_stream())


def test_refusals_leave_everything_untouched():
    import torch

    from slimdqn import _hip

    B = 32
    fused, chain, iqn = _learner("mlp", B), _learner("mlp", B), _learner("iqn", B)
    for lr in (fused, chain, iqn):
        lr.agent._ensure_handle(B)
    (u, _), = _draws("mlp", B, 1)
    tau = torch.full((2 * 3 * 4 * B,), 0.5, dtype=torch.float32, device="cuda")
    before = _snapshot(fused)
    lib = _hip.lib()
    cases = [
        (dict(stack=3), "stack 3"),                                  # what the dispatched entry refuses
        (dict(weights_dev=None), "null pointer"),
        (dict(nodes_dev=None), "null pointer"),
        (dict(uniforms_host=None), "null pointer"),
        (dict(B=0), "batch 0"), (dict(B=257), "batch 257"),
        (dict(depth=0), "depth"), (dict(depth=32), "depth"),
        (dict(n_items=0), "n_items"),
        (dict(taus_dev=tau), "tau_dev"),                             # fractions for a handle without quantile heads
        (dict(flags=_hip.F_GRADS_ONLY), "profile flags"),
    ]
    for kw, match in cases:
        kw = dict(kw)
        rc = _raw_call(fused, u, kw.pop("B", B), **kw)
        msg = lib.idqn_last_error().decode()
        assert rc == _hip.E_INVALID and msg.startswith("idqn_per_learn_on_replay:") and match in msg, (kw, rc, msg)
    assert _raw_call(iqn, u, B) == _hip.E_INVALID and "tau_dev" in lib.idqn_last_error().decode()  # quantile heads without fractions
    _hip.check(lib.idqn_set_per_buffers(fused.agent._handle, _hip.ptr(fused._weights), _hip.ptr(fused._td_abs)), "idqn_set_per_buffers")
    assert _raw_call(fused, u, B) == _hip.E_INVALID and "idqn_set_per_buffers" in lib.idqn_last_error().decode()
    _hip.check(lib.idqn_set_per_buffers(fused.agent._handle, None, None), "idqn_set_per_buffers")
    torch.cuda.synchronize()
    _assert_snapshots_equal(before, _snapshot(fused), "after the refusals")
    # the next valid call gives the chain's result
    _hip.check(_raw_call(fused, u, B), "idqn_per_learn_on_replay")
    chain._step_chain(u.copy())
    torch.cuda.synchronize()
    _assert_snapshots_equal(_snapshot(chain), _snapshot(fused), "after a valid call")


@pytest.mark.parametrize("family", ["mlp", "plane"])
def test_prioritized_learner_fused_equals_chain(family):
    import torch

    from slimdqn.sample_collection.replay_buffer import TransitionElement

    _, shape, dtype, _, _, _, _, A, _ = FAMILIES[family]
    out = {}
    for fuse in (True, False):
        learner = _learner(family, 32)
        learner.fuse_per_step = fuse
        gathers, real = [], learner.rb._gather_device
        learner.rb._gather_device = lambda *a, **k: gathers.append(1) or real(*a, **k)
        rng, losses = np.random.default_rng(23), []
        for i in range(6):
            losses.append(learner.step().clone())
            learner.rb.add(TransitionElement(_frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), i == 3, i == 3))
        torch.cuda.synchronize()
        assert learner.__dict__.get("_fused_ok") is (True if fuse else None), "the wrong route ran"
        if fuse:
            assert not gathers, "the fused route gathered"
        elif family == "plane":
            assert len(gathers) == 6
        out[fuse] = (torch.stack(losses).cpu().numpy(), _snapshot(learner), learner.sampler._rng_key.bit_generator.state)
    assert out[True][0].tobytes() == out[False][0].tobytes() and np.isfinite(out[True][0]).all()
    _assert_snapshots_equal(out[True][1], out[False][1], family)
    assert out[True][2] == out[False][2]
