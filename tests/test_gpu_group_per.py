"""GPU: prioritized seed groups -- ``idqn_group_per_learn_on_replay_fc`` and ``PrioritizedGroupLearner``.

Every comparison is ``tobytes()`` equality, no tolerance, against TWINS: a second set of agents, rings, trees and learner
buffers built by the same code from the same seeds (so with the same initial bytes), stepped member by member through
``idqn_per_learn_on_replay`` with the same uniforms.  Compared after a call, for every member: online parameters, moments,
count, losses, cum_losses, tree nodes, max_priority_dev, leaves, weights, |TD| and priorities.

Nets are tiny (obs 8, features [16, 12], A 4, K 3; one K = 1 ``DQN`` case; obs 6 = frames of 3 x stack 2).  Rings come from
``ReplayBuffer`` with ``SlotPrioritizedSampler``, filled with scripted transitions (terminals every 7th step, an episode start
at the front, so short stacks occur) whose priorities differ, so the members' descents differ.  The stack-2 case has one
``VectorReplayBuffer`` ring (E = 2): its sampler protocol is ``ReplayBuffer``'s, so it takes a ``SlotPrioritizedSampler``.
On the parent commit the entry and the class do not exist.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FEATS, A = [16, 12], 4
HYPER = [(1e-3, 1e-8, 0.99), (3e-4, 1.5e-4, 0.9), (2e-3, 1e-6, 0.95), (5e-4, 1e-7, 0.999)]  # lr, Adam eps, gamma per member
AGENT_STATE = ("_online", "_mu", "_nu", "_count", "_losses", "_cum")
LEARNER_STATE = ("_leaves", "_weights", "_td_abs", "_priorities")


def _agent(g, K=3, obs=8):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.idqn import iDQN

    lr, eps, gamma = HYPER[g % len(HYPER)]
    if K == 1:
        a = DQN(100 + g, obs, A, FEATS, "fc", lr, gamma, 1, 1, 10**9, adam_eps=eps)
    else:
        a = iDQN(100 + g, obs, A, K, FEATS, "fc", lr, gamma, 1, 1, 10**9, 10**9, adam_eps=eps)
    a._target.copy_(a._online * 0.5 + 0.01 * (g + 1))  # a target net that is not the online net
    return a


def _learner(g, B=32, capacity=64, n_items=None, K=3, frame=8, stack=1, vector=False, alpha=0.6, **kw):
    """Member g: agent, ring (wrapped unless ``n_items`` asks for a partly filled one) and ``PrioritizedLearner``."""
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    rng = np.random.default_rng(50 + g)
    tr = lambda last: TransitionElement(rng.standard_normal((frame,)).astype(np.float32), int(rng.integers(A)), float(rng.normal()), last, last)
    sampler = SlotPrioritizedSampler(7 + g, capacity, alpha)
    if vector:
        rb = VectorReplayBuffer(sampler, B, capacity, stack_size=stack, update_horizon=1, gamma=0.99, n_envs=2, segment=24)
        for i in range(24 * 2 + 3):
            rb.add_many([tr((i + 2 * e) % 7 == 6) for e in range(2)])
    else:
        rb = ReplayBuffer(sampler, batch_size=B, max_capacity=capacity, stack_size=stack, update_horizon=1, gamma=0.99)
        i = 0
        while (len(sampler) < n_items) if n_items else (i < 2 * capacity + 22):
            rb.add(tr(i % 7 == 6), **({"priority": float(rng.random() * 3.0 + 0.05)} if i % 3 else {}))
            i += 1
    rb.reuse_sample_buffers = True
    if n_items:
        assert len(sampler) == n_items
    lr = PrioritizedLearner(_agent(g, K, frame * stack), rb, **kw)
    lr.agent._ensure_handle(32)
    return lr


def _snapshot(learners):
    """Device-side copies (no host synchronisation) of everything the contract names, per member."""
    out = []
    for lr in learners:
        d = {n: getattr(lr.agent, n).clone() for n in AGENT_STATE}
        d.update({n: getattr(lr, n).clone() for n in LEARNER_STATE})
        d["nodes"] = lr.sampler._sum_tree._nodes_dev.clone()
        d["max_priority"] = lr.sampler._max_priority_dev.clone()
        out.append(d)
    return out


def _assert_equal(a, b, tag):
    for g, (x, y) in enumerate(zip(a, b)):
        for n in x:
            assert x[n].cpu().numpy().tobytes() == y[n].cpu().numpy().tobytes(), (tag, f"member {g}", n)


def _per(p, lr, u, **fields):
    """``idqn_per_step_t`` of learner ``lr`` on uniforms ``u``, fields replaced by name."""
    tree = lr.sampler._sum_tree
    p.nodes_dev, p.depth, p.n_items = tree._nodes_dev.data_ptr(), tree._depth, len(lr.sampler)
    p.uniforms_host = u.ctypes.data
    p.stratified, p.reduce_max, p.beta, p.eps, p.alpha = lr.stratified, lr.reduce_max, lr.beta, lr.eps, lr.sampler._alpha
    p.max_priority_dev = lr.sampler._max_priority_dev.data_ptr()
    p.leaves_dev, p.weights_dev, p.td_abs_dev = lr._leaves.data_ptr(), lr._weights.data_ptr(), lr._td_abs.data_ptr()
    p.priorities_dev, p.tree_scratch_dev, p.tau_dev = lr._priorities.data_ptr(), tree._scratch.data_ptr(), None
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _solo(lr, u, B=None, **fields):
    """The comparison target: ``idqn_per_learn_on_replay`` on one member."""
    from slimdqn import _hip

    B = lr.rb._batch_size if B is None else B
    frames, n_frames, frame_bytes, rows, stack = lr.rb.ring_view()[:5]
    p = _per(_hip.PerStep(), lr, u, **fields)
    _hip.check(_hip.lib().idqn_per_learn_on_replay(lr.agent._handle, C.byref(p), _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                   B, int(stack), B, 0, _hip.current_stream()), "idqn_per_learn_on_replay")


class _Group:
    """The C group over the learners' handles."""

    def __init__(self, learners):
        from slimdqn import _hip

        self.learners, self.g = learners, C.c_void_p()
        arr = (C.c_void_p * len(learners))(*[lr.agent._handle.value for lr in learners])
        _hip.check(_hip.lib().idqn_group_create(arr, len(learners), C.byref(self.g)), "idqn_group_create")

    def rings(self):
        from slimdqn.networks.group import AgentGroup

        self._views = [lr.rb.ring_view() for lr in self.learners]
        return AgentGroup._rings(self._views)

    def call(self, us, B=None, flags=0, fields=None, rings=None, per=None, div=None):
        """The entry's return code; ``fields``: {member: {field: value}} replacements in the members' records."""
        from slimdqn import _hip

        B = self.learners[0].rb._batch_size if B is None else B
        if per is None:
            per = (_hip.PerStep * len(self.learners))()
            for g, (lr, u) in enumerate(zip(self.learners, us)):
                _per(per[g], lr, u, **(fields or {}).get(g, {}))
        return _hip.lib().idqn_group_per_learn_on_replay_fc(self.g, self.rings() if rings is None else rings, per, B, B if div is None else div, flags,
                                                            _hip.current_stream())

    def step(self, us, **kw):
        from slimdqn import _hip

        _hip.check(self.call(us, **kw), "idqn_group_per_learn_on_replay_fc")

    def plain(self, slots):
        from slimdqn import _hip

        slots = np.ascontiguousarray(slots, np.int32)
        _hip.check(_hip.lib().idqn_group_learn_on_replay_fc(self.g, self.rings(), slots.ctypes.data, slots.shape[1], slots.shape[1], 0,
                                                            _hip.current_stream()), "idqn_group_learn_on_replay_fc")

    def close(self):
        from slimdqn import _hip

        if self.g:
            _hip.lib().idqn_group_destroy(self.g)
            self.g = C.c_void_p()


def _sets(S, **kw):
    """(members, twins): two sets of S learners with the same initial bytes."""
    per_member = kw.pop("per_member", None) or [{}] * S
    make = lambda: [_learner(g, **{**kw, **per_member[g]}) for g in range(S)]
    return make(), make()


def _uniforms(rng, S, B):
    us = [rng.random(B) for _ in range(S)]
    us[0][rng.integers(B)] = 0.0
    us[-1][rng.integers(B)] = np.nextafter(1.0, 0.0)
    return us


def _run(members, twins, B_seq, each, tag, seed=3, group=None):
    """Group calls of batches ``B_seq`` back to back (no synchronisation between them) against the solo calls on the twins,
    compared after the last call or -- ``each`` -- after every call."""
    import torch

    rng = np.random.default_rng(seed)
    draws = [_uniforms(rng, len(members), B) for B in B_seq]
    own = group is None
    group = _Group(members) if own else group
    got = []
    for B, us in zip(B_seq, draws):
        group.step(us, B=B)
        if each:
            got.append(_snapshot(members))
    if not each:
        got.append(_snapshot(members))
    want = []
    for B, us in zip(B_seq, draws):
        for t, u in zip(twins, us):
            _solo(t, u, B=B)
        if each:
            want.append(_snapshot(twins))
    if not each:
        want.append(_snapshot(twins))
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        _assert_equal(a, b, (tag, f"call {i if each else len(B_seq) - 1}"))
    if own:
        group.close()
    return got[-1]


@pytest.mark.parametrize("K,each", [(3, False), (3, True), (1, True)])
def test_base_four_calls_back_to_back(K, each):
    members, twins = _sets(3, K=K)
    last = _run(members, twins, [32] * 4, each, ("base", K))
    for g, d in enumerate(last):
        assert (d["_count"].cpu().numpy() == 4).all() and np.isfinite(d["_losses"].cpu().numpy()).all()
        assert (d["_td_abs"] > 0).any().item() and (d["_weights"] >= 0).all().item() and (d["_weights"] <= 1).all().item()
    assert len({d["_online"].cpu().numpy().tobytes() for d in last}) == 3, "the members were meant to differ"
    assert len({d["_leaves"].cpu().numpy().tobytes() for d in last}) == 3, "the members' descents were meant to differ"


@pytest.mark.parametrize("B_seq", [[5, 5], [1, 1], [32, 5, 32], [16, 17]])
def test_ragged_and_minimal_batches(B_seq):
    """Pad lanes and the workgroup shape: batches that fill no wave round, and a small batch after a full one on one group."""
    members, twins = _sets(2, B=max(B_seq))
    _run(members, twins, B_seq, True, ("ragged", tuple(B_seq)))


def test_duplicate_leaves_first_occurrence_wins():
    """8 items, 32 draws: duplicates by pigeonhole.  Byte equality with the solo call pins the order of the adds per node; the
    leaf values are checked on the CPU as well: a leaf holds the priority of its FIRST occurrence in the batch."""
    members, twins = _sets(2, n_items=8)
    last = _run(members, twins, [32, 32], True, "duplicates")
    for g, d in enumerate(last):
        leaves, pri, nodes = d["_leaves"].cpu().numpy(), d["_priorities"].cpu().numpy(), d["nodes"].cpu().numpy()
        assert leaves.min() >= 0 and leaves.max() <= 7
        assert len(set(leaves.tolist())) < 32, "duplicates are present"
        first_leaf = 2 ** (members[g].sampler._sum_tree._depth - 1) - 1
        for leaf in set(leaves.tolist()):
            assert nodes[first_leaf + leaf] == pri[np.flatnonzero(leaves == leaf)[0]], (g, leaf)


def test_partly_filled_tree():
    members, twins = _sets(2, n_items=5)
    last = _run(members, twins, [32, 32], True, "partly filled")
    for d in last:
        leaves = d["_leaves"].cpu().numpy()
        assert leaves.min() >= 0 and leaves.max() <= 4


def test_heterogeneous_members():
    """Capacities 64 and 256 (depths 7 and 9), different item counts, beta, alpha, eps, reduce, stratified -- and, by ``HYPER``,
    different learning rate, Adam epsilon and gamma."""
    per_member = [dict(capacity=64, beta=0.4, eps=1e-6, reduce="mean", stratified=True, alpha=0.6),
                  dict(capacity=256, n_items=100, beta=0.7, eps=1e-3, reduce="max", stratified=False, alpha=0.9),
                  dict(capacity=256, beta=1.0, eps=1e-2, reduce="max", stratified=True, alpha=0.3)]
    members, twins = _sets(3, per_member=per_member)
    assert [lr.sampler._sum_tree._depth for lr in members] == [7, 9, 9] and [len(lr.sampler) for lr in members] == [64, 100, 256]
    _run(members, twins, [32] * 3, True, "heterogeneous")


def test_stack_two_with_a_vector_ring():
    """obs 6 = frames of 3 x stack 2: sampled elements whose stack crosses an episode start; member 1 draws from a
    ``VectorReplayBuffer`` (E = 2)."""
    per_member = [dict(), dict(vector=True), dict()]
    members, twins = _sets(3, capacity=40, frame=3, stack=2, per_member=per_member)
    rows = np.asarray(members[0].rb._meta)
    assert ((rows[:, 1] < 2) | (rows[:, 3] < 2)).any(), "the ring holds no element whose stack crosses an episode start"
    _run(members, twins, [32] * 3, True, "stack 2")


def test_largest_grid():
    members, twins = _sets(32)
    _run(members, twins, [32], False, "S = 32")


def test_interleaved_with_solo_and_plain_group_calls():
    """Group PER call, a solo PER call on member 1, a plain group step, a group PER call -- the same script on the twins.  The
    weights travel in the table: none may leak into the plain step, and the members' own buffers stay unset."""
    import torch

    from slimdqn import _hip

    members, twins = _sets(3)
    group, twin_group = _Group(members), _Group(twins)
    rng = np.random.default_rng(11)
    us = [_uniforms(rng, 3, 32) for _ in range(3)]
    slots = np.stack([rng.choice(np.flatnonzero(lr.sampler._key_of_slot >= 0), 32) for lr in members]).astype(np.int32)  # live slots
    group.step(us[0])
    _solo(members[1], us[1][1])
    group.plain(slots)
    after_plain = _snapshot(members)
    group.step(us[2])
    got = _snapshot(members)
    for t, u in zip(twins, us[0]):
        _solo(t, u)
    _solo(twins[1], us[1][1])
    for t, s in zip(twins, slots):  # the plain step through the solo entry: no weights, no |TD|
        frames, n_frames, frame_bytes, rows, stack = t.rb.ring_view()[:5]
        _hip.check(_hip.lib().idqn_learn_on_replay_fc(t.agent._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                      s.ctypes.data, 32, int(stack), 32, 0, _hip.current_stream()), "idqn_learn_on_replay_fc")
    want_plain = _snapshot(twins)
    for t, u in zip(twins, us[2]):
        _solo(t, u)
    torch.cuda.synchronize()
    _assert_equal(after_plain, want_plain, "after the plain group step")
    _assert_equal(got, _snapshot(twins), "after the last group call")
    # h->is_weight is still NULL: the plain group entry, which refuses members with buffers set, serves
    group.plain(slots)
    twin_group.plain(slots)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(members), _snapshot(twins), "a plain group step afterwards")
    group.close(), twin_group.close()


def test_null_outputs():
    """``priorities_dev`` and ``max_priority_dev`` NULL for member 1: its buffers keep their bytes, everything else matches."""
    import torch

    members, twins = _sets(3)
    group = _Group(members)
    us = _uniforms(np.random.default_rng(5), 3, 32)
    null = dict(priorities_dev=None, max_priority_dev=None)
    for lr in (members[1], twins[1]):
        lr._priorities.fill_(-1.0)
    before_max = members[1].sampler._max_priority_dev.clone()
    group.step(us, fields={1: null})
    for g, (t, u) in enumerate(zip(twins, us)):
        _solo(t, u, **(null if g == 1 else {}))
    torch.cuda.synchronize()
    _assert_equal(_snapshot(members), _snapshot(twins), "null outputs")
    assert (members[1]._priorities == -1.0).all().item() and members[1].sampler._max_priority_dev.equal(before_max)
    assert (members[0]._priorities > 0).all().item()
    group.close()


def test_refusals_leave_everything_untouched():
    import torch

    from slimdqn import _hip

    members, twins = _sets(3)
    group = _Group(members)
    us = _uniforms(np.random.default_rng(9), 3, 32)
    before = _snapshot(members)
    lib = _hip.lib()
    tau = torch.full((8,), 0.5, dtype=torch.float32, device="cuda")
    other = members[0]
    cases = [
        (dict(per="null"), "null pointer"), (dict(rings="null"), "null pointer"),
        (dict(B=0), "batch 0"), (dict(B=33), "batch 33"),
        (dict(flags=_hip.F_GRADS_ONLY), "takes no flags"), (dict(flags=_hip.F_PROFILE), "takes no flags"),
        (dict(div=31), "mean divisor"),
    ]
    cases += [(dict(fields={1: {f: None}}), "null pointer")
              for f in ("nodes_dev", "uniforms_host", "leaves_dev", "weights_dev", "td_abs_dev", "tree_scratch_dev")]
    cases += [
        (dict(fields={2: dict(tau_dev=tau.data_ptr())}), "tau_dev"),
        (dict(fields={1: dict(depth=0)}), "depth"), (dict(fields={1: dict(depth=32)}), "depth"),
        (dict(fields={2: dict(n_items=0)}), "n_items"),
        (dict(fields={1: dict(nodes_dev=other.sampler._sum_tree._nodes_dev.data_ptr())}), "same nodes_dev"),
        (dict(fields={1: dict(leaves_dev=other._leaves.data_ptr())}), "same leaves_dev"),
        (dict(fields={2: dict(weights_dev=other._weights.data_ptr())}), "same weights_dev"),
        (dict(fields={2: dict(td_abs_dev=members[1]._td_abs.data_ptr())}), "same td_abs_dev"),
        (dict(fields={1: dict(tree_scratch_dev=other.sampler._sum_tree._scratch.data_ptr())}), "same tree_scratch_dev"),
        (dict(fields={1: dict(priorities_dev=other._priorities.data_ptr())}), "same priorities_dev"),
        (dict(fields={2: dict(max_priority_dev=other.sampler._max_priority_dev.data_ptr())}), "same max_priority_dev"),
    ]
    for kw, match in cases:
        kw = dict(kw)
        if kw.get("per") == "null":
            rc = lib.idqn_group_per_learn_on_replay_fc(group.g, group.rings(), None, 32, 32, 0, _hip.current_stream())
        elif kw.get("rings") == "null":
            per = (_hip.PerStep * 3)()
            for g in range(3):
                _per(per[g], members[g], us[g])
            rc = lib.idqn_group_per_learn_on_replay_fc(group.g, None, per, 32, 32, 0, _hip.current_stream())
        else:
            rc = group.call(us, **kw)
        msg = lib.idqn_last_error().decode()
        assert rc == _hip.E_INVALID and msg.startswith("idqn_group_per_learn_on_replay_fc:") and match in msg, (kw, rc, msg)
    # what replay_fc_check refuses for a member's ring
    rings = group.rings()
    rings[1].stack = 3
    assert group.call(us, rings=rings) == _hip.E_INVALID and "stack 3" in lib.idqn_last_error().decode()
    # a member with idqn_set_per_buffers set
    _hip.check(lib.idqn_set_per_buffers(members[1].agent._handle, _hip.ptr(members[1]._weights), _hip.ptr(members[1]._td_abs)), "idqn_set_per_buffers")
    assert group.call(us) == _hip.E_INVALID and "idqn_set_per_buffers" in lib.idqn_last_error().decode()
    _hip.check(lib.idqn_set_per_buffers(members[1].agent._handle, None, None), "idqn_set_per_buffers")
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(members), "after the refusals")
    # the next valid call gives the twins' result
    group.step(us)
    for t, u in zip(twins, us):
        _solo(t, u)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(members), _snapshot(twins), "after a valid call")
    group.close()


@pytest.mark.parametrize("fused_env", ["1", "0"])
def test_prioritized_group_learner_equals_the_members_learners(monkeypatch, fused_env):
    """Three ``PrioritizedGroupLearner.step`` rounds against three rounds of ``PrioritizedLearner.step`` on the twins: generator
    states, trees, learner buffers and agents.  With ``IDQN_PER_FUSED=0`` the members' route runs and gives the same bytes."""
    import torch

    from slimdqn.networks.group import AgentGroup
    from slimdqn.sample_collection.per import PrioritizedGroupLearner

    monkeypatch.setenv("IDQN_PER_FUSED", fused_env)
    members, twins = _sets(3, beta=0.5, eps=1e-3)
    group = AgentGroup([lr.agent for lr in members])
    gl = PrioritizedGroupLearner(group, [lr.rb for lr in members], beta=0.5, eps=1e-3)
    gl.group_per_sizes = frozenset({3})  # (the shipped default follows the measurements: the route is what is under test)
    losses = [[x.clone() for x in gl.step()] for _ in range(3)]
    want = [[t.step().clone() for t in twins] for _ in range(3)]
    torch.cuda.synchronize()
    assert gl.__dict__.get("_group_per_ok") is (True if fused_env == "1" else None), "the wrong route ran"
    for a, b in zip(losses, want):
        for x, y in zip(a, b):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    _assert_equal(_snapshot(gl.learners), _snapshot(twins), ("group learner", fused_env))
    for lr, t in zip(gl.learners, twins):
        assert lr.sampler._rng_key.bit_generator.state == t.sampler._rng_key.bit_generator.state
    assert (members[0].agent._count.cpu().numpy() == 3).all()
    group.close()
