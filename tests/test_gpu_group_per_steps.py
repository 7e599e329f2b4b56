"""GPU: prioritized seed groups, n steps per call -- ``idqn_group_per_learn_steps_on_replay_fc`` (``k_per_group_turn``),
``PrioritizedGroupLearner.steps`` / ``update_params_many`` and ``SeedVectorTrainer(..., learner=)``.

Every comparison is ``tobytes()`` equality, no tolerance, against TWINS: a second set of agents, rings, trees and row buffers
built by the same code from the same seeds (so with the same initial bytes), driven through n calls of
``idqn_group_per_learn_on_replay_fc`` on the rows of the same uniforms (or, where a test says so, through
``idqn_per_learn_steps_on_replay`` member by member).  Compared after a call, for every member: online parameters, both
moments, count, losses, cum_losses, tree nodes, max_priority_dev and ALL n rows of leaves, weights, |TD| and priorities.

Nets are tiny (obs 8, features [16, 12], A 4, K 3; one K = 1 ``DQN`` case).  Members differ in capacity (so in depth), beta,
alpha, eps, reduce, stratification; one has a partly filled ring, one a ``VectorReplayBuffer`` ring of stack 2 (frames of 4, so
its observations are 8 wide like the others').  On the parent commit the entry and the methods do not exist.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAME = "idqn_group_per_learn_steps_on_replay_fc"
FEATS, A = [16, 12], 4
HYPER = [(1e-3, 1e-8, 0.99), (3e-4, 1.5e-4, 0.9), (2e-3, 1e-6, 0.95), (5e-4, 1e-7, 0.999)]  # lr, Adam eps, gamma per member
AGENT_STATE = ("_online", "_mu", "_nu", "_count", "_losses", "_cum")
ROWS = ("leaves", "weights", "td_abs", "priorities")
# member g of a set (the first S are taken): base; vector ring of stack 2; partly filled, max, not stratified; deep and full; shallow
MEMBERS = [dict(capacity=64, beta=0.4, eps=1e-6, reduce="mean", stratified=True, alpha=0.6),
           dict(capacity=40, vector=True, frame=4, stack=2, beta=0.5, eps=1e-4, reduce="max", stratified=True, alpha=0.7),
           dict(capacity=256, n_items=100, beta=0.7, eps=1e-3, reduce="max", stratified=False, alpha=0.9),
           dict(capacity=256, beta=1.0, eps=1e-2, reduce="mean", stratified=True, alpha=0.3),
           dict(capacity=32, beta=0.2, eps=1e-5, reduce="mean", stratified=False, alpha=0.5)]


def _agent(g, K=3, obs=8, shift=None, schedule=(10**9, 10**9)):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.idqn import iDQN

    lr, eps, gamma = HYPER[g % len(HYPER)]
    if K == 1:
        a = DQN(100 + g, obs, A, FEATS, "fc", lr, gamma, 1, 1, schedule[0], adam_eps=eps)
    else:
        a = iDQN(100 + g, obs, A, K, FEATS, "fc", lr, gamma, 1, 1, schedule[0], schedule[1], adam_eps=eps)
    a._target.copy_(a._online * 0.5 + (0.01 * (g + 1) if shift is None else shift))  # a target net that is not the online net
    return a


def _learner(g, B=32, capacity=64, n_items=None, K=3, frame=8, stack=1, vector=False, alpha=0.6, shift=None, schedule=(10**9, 10**9), **kw):
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
    lr = PrioritizedLearner(_agent(g, K, frame * stack, shift, schedule), rb, **kw)
    lr.agent._ensure_handle(32)
    return lr


def _sets(S, **kw):
    """(members, twins): two sets of S learners with the same initial bytes; member g is ``MEMBERS[g]`` unless ``per_member``."""
    per_member = kw.pop("per_member", None) or MEMBERS[:S]
    make = lambda: [_learner(g, **{**kw, **per_member[g]}) for g in range(S)]
    return make(), make()


class _Rows:
    """The row buffers of one member for calls of at most n steps of B samples, with the same start bytes on both sides."""

    def __init__(self, lr, n, B):
        import torch

        K = lr.agent._K
        self.n, self.B, self.K = n, B, K
        self.leaves = torch.full((n, B), -1, dtype=torch.int32, device="cuda")
        self.weights = torch.full((n, B), -1.0, dtype=torch.float32, device="cuda")
        self.td_abs = torch.full((n, K, B), -1.0, dtype=torch.float32, device="cuda")
        self.priorities = torch.full((n, B), -1.0, dtype=torch.float64, device="cuda")


def _snapshot(learners, rows):
    """Device-side copies (no host synchronisation) of everything the contract names, per member."""
    out = []
    for lr, r in zip(learners, rows):
        d = {n: getattr(lr.agent, n).clone() for n in AGENT_STATE}
        d.update({n: getattr(r, n).clone() for n in ROWS})
        d["nodes"] = lr.sampler._sum_tree._nodes_dev.clone()
        d["max_priority"] = lr.sampler._max_priority_dev.clone()
        out.append(d)
    return out


def _assert_equal(a, b, tag):
    for g, (x, y) in enumerate(zip(a, b)):
        for n in x:
            assert x[n].cpu().numpy().tobytes() == y[n].cpu().numpy().tobytes(), (tag, f"member {g}", n)


def _per(p, lr, U, r, row=None, **fields):
    """``idqn_per_steps_t`` of learner ``lr`` on uniforms ``U`` and rows ``r`` -- or, with ``row``, the ``idqn_per_step_t`` of that
    row; fields replaced by name."""
    tree = lr.sampler._sum_tree
    at = lambda t: t.data_ptr() if row is None else t[row].data_ptr()
    p.nodes_dev, p.depth, p.n_items = tree._nodes_dev.data_ptr(), tree._depth, len(lr.sampler)
    p.uniforms_host = U.ctypes.data if row is None else U[row].ctypes.data
    p.stratified, p.reduce_max, p.beta, p.eps, p.alpha = lr.stratified, lr.reduce_max, lr.beta, lr.eps, lr.sampler._alpha
    p.max_priority_dev = lr.sampler._max_priority_dev.data_ptr()
    p.leaves_dev, p.weights_dev, p.td_abs_dev, p.priorities_dev = at(r.leaves), at(r.weights), at(r.td_abs), at(r.priorities)
    p.tree_scratch_dev = tree._scratch.data_ptr()
    if row is not None:
        p.tau_dev = None
    for k, v in fields.items():
        setattr(p, k, v)
    return p


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

    def call(self, Us, rows, n=None, B=None, flags=0, fields=None, rings=None, div=None):
        """The n-step entry's return code; ``fields``: {member: {field: value}} replacements in the members' records."""
        from slimdqn import _hip

        n, B = Us[0].shape[0] if n is None else n, rows[0].B if B is None else B
        per = (_hip.PerSteps * len(self.learners))()
        for g, (lr, U, r) in enumerate(zip(self.learners, Us, rows)):
            _per(per[g], lr, U, r, **(fields or {}).get(g, {}))
        return getattr(_hip.lib(), NAME)(self.g, self.rings() if rings is None else rings, per, n, B, B if div is None else div, flags,
                                         _hip.current_stream())

    def steps(self, Us, rows, **kw):
        from slimdqn import _hip

        _hip.check(self.call(Us, rows, **kw), NAME)

    def singles(self, Us, rows):
        """The comparison target: one ``idqn_group_per_learn_on_replay_fc`` call per row."""
        from slimdqn import _hip

        B = rows[0].B
        for i in range(Us[0].shape[0]):
            per = (_hip.PerStep * len(self.learners))()
            for g, (lr, U, r) in enumerate(zip(self.learners, Us, rows)):
                _per(per[g], lr, U, r, row=i)
            _hip.check(_hip.lib().idqn_group_per_learn_on_replay_fc(self.g, self.rings(), per, B, B, 0, _hip.current_stream()),
                       "idqn_group_per_learn_on_replay_fc")

    def close(self):
        from slimdqn import _hip

        if self.g:
            _hip.lib().idqn_group_destroy(self.g)
            self.g = C.c_void_p()


def _uniforms(rng, S, n, B):
    Us = [np.ascontiguousarray(rng.random((n, B))) for _ in range(S)]
    Us[0][0, rng.integers(B)] = 0.0
    Us[-1][n - 1, rng.integers(B)] = np.nextafter(1.0, 0.0)
    return Us


def _solo_steps(lr, U, r):
    """``idqn_per_learn_steps_on_replay`` on one member."""
    from slimdqn import _hip

    frames, n_frames, frame_bytes, ring_rows, stack = lr.rb.ring_view()[:5]
    p = _per(_hip.PerSteps(), lr, U, r)
    _hip.check(_hip.lib().idqn_per_learn_steps_on_replay(lr.agent._handle, C.byref(p), _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(ring_rows),
                                                         U.shape[0], r.B, int(stack), r.B, 0, _hip.current_stream()), "idqn_per_learn_steps_on_replay")


def _parity(S, n_seq, B, tag, seed=3, each=True, **kw):
    """Calls of ``n_seq`` steps back to back (no host synchronisation between them) against the single group calls on the twins,
    compared after every call (``each``) or after the last; returns (members, twins, the rows of both, the uniforms, the groups)."""
    import torch

    members, twins = _sets(S, B=max(B, 2), **kw)  # (a ring's own batch size is not the call's)
    rng = np.random.default_rng(seed)
    draws = [_uniforms(rng, S, n, B) for n in n_seq]
    rows, twin_rows = [_Rows(lr, max(n_seq), B) for lr in members], [_Rows(lr, max(n_seq), B) for lr in twins]
    group, twin_group = _Group(members), _Group(twins)
    got, want = [], []
    for Us in draws:
        group.steps(Us, rows)
        if each:
            got.append(_snapshot(members, rows))
    for Us in draws:
        twin_group.singles(Us, twin_rows)
        if each:
            want.append(_snapshot(twins, twin_rows))
    if not each:
        got.append(_snapshot(members, rows)), want.append(_snapshot(twins, twin_rows))
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        _assert_equal(a, b, (tag, f"call {i}"))
    return members, twins, rows, twin_rows, draws, group, twin_group


@pytest.mark.parametrize("B", [1, 7, 32])
@pytest.mark.parametrize("n", [1, 2, 3, 32])
@pytest.mark.parametrize("S", [1, 2, 5])
def test_parity_with_n_single_group_calls(S, n, B):
    """Two calls of n steps each.  Seven samples are no power of two (m = 8 != n in the set); the members are ``MEMBERS``."""
    members, twins, rows, _, _, group, twin_group = _parity(S, [n, n], B, ("parity", S, n, B))
    if S == 5:
        assert [lr.sampler._sum_tree._depth for lr in members] == [7, 7, 9, 9, 6] and len(members[2].sampler) == 100
        assert members[1].rb.ring_view()[4] == 2, "member 1 draws from a ring of stack 2"
    for lr, r in zip(members, rows):
        assert (lr.agent._count.cpu().numpy() == 2 * n).all() and np.isfinite(lr.agent._losses.cpu().numpy()).all()
        leaves, w = r.leaves[:n].cpu().numpy(), r.weights[:n].cpu().numpy()
        assert leaves.min() >= 0 and leaves.max() < len(lr.sampler) and (w >= 0).all() and (w <= 1).all()
        assert (r.td_abs[:n] >= 0).all().item() and (r.priorities[:n] > 0).all().item()
    group.close(), twin_group.close()


def test_parity_single_head():
    """The K = 1 ``DQN`` members."""
    _, _, _, _, _, group, twin_group = _parity(3, [3, 2], 32, "K = 1", per_member=[dict(m, K=1) for m in MEMBERS[:3]])
    group.close(), twin_group.close()


def test_parity_with_the_solo_n_step_call_and_the_draw_sees_the_write_back():
    """S = 2, n = 3 against ``idqn_per_learn_steps_on_replay`` on each member alone -- and the condition on the inputs without which
    a kernel that drew every row on the tree of the call's start would pass: on the twins alone, rows 1 .. n - 1 drawn on the INITIAL
    tree (the oracle's descent on the nodes downloaded before the call) differ from the rows the steps produced.  The target nets
    are far from the online nets, so the first write-back moves the priorities of the sampled leaves by a lot."""
    import torch

    from oracle.sumtree_ref import SumTreeRef

    S, n, B = 2, 3, 32
    per_member = [dict(MEMBERS[0], shift=2.0), dict(MEMBERS[2], shift=-1.5)]
    members, twins = _sets(S, per_member=per_member)
    Us = _uniforms(np.random.default_rng(17), S, n, B)
    rows, twin_rows = [_Rows(lr, n, B) for lr in members], [_Rows(lr, n, B) for lr in twins]
    initial = [lr.sampler._sum_tree._nodes_dev.cpu().numpy().copy() for lr in twins]
    group = _Group(members)
    group.steps(Us, rows)
    for t, U, r in zip(twins, Us, twin_rows):
        _solo_steps(t, U, r)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(members, rows), _snapshot(twins, twin_rows), "against the solo n-step call")
    for g, (t, U, r, nodes) in enumerate(zip(twins, Us, twin_rows, initial)):  # the condition, on the twin alone
        ref = SumTreeRef(t.sampler._max_capacity)
        assert ref.depth == t.sampler._sum_tree._depth and ref.nodes.shape == nodes.shape
        ref.nodes[:] = nodes
        stale = []
        for i in range(1, n):
            targets = (np.arange(B) + U[i]) / B * ref.root if t.stratified else U[i] * ref.root
            stale.append(np.clip(ref.query(np.minimum(targets, np.nextafter(ref.root, 0.0))), 0, len(t.sampler) - 1))
        drawn = r.leaves[1:n].cpu().numpy()
        assert (np.stack(stale) != drawn).any(), f"member {g}: rows 1.. do not depend on the write-backs before them; choose other inputs"
        assert not np.array_equal(t.sampler._sum_tree._nodes_dev.cpu().numpy(), nodes)
    group.close()


def test_duplicate_leaves_first_occurrence_wins_through_the_turn():
    """Member 1 holds 3 items and draws 32: every batch repeats leaves.  Byte equality pins the order of the adds per node through
    ``k_per_group_turn``; on the CPU as well: after the call a leaf holds the priority of its FIRST occurrence in the LAST row that
    names it."""
    per_member = [MEMBERS[0], dict(MEMBERS[2], n_items=3)]
    members, _, rows, _, _, group, twin_group = _parity(2, [3, 3], 32, "duplicates", per_member=per_member)
    r, lr = rows[1], members[1]
    leaves, pri, nodes = r.leaves.cpu().numpy(), r.priorities.cpu().numpy(), lr.sampler._sum_tree._nodes_dev.cpu().numpy()
    assert leaves.min() >= 0 and leaves.max() <= 2
    first_leaf = 2 ** (lr.sampler._sum_tree._depth - 1) - 1
    for leaf in range(3):
        last_row = max(i for i in range(3) if (leaves[i] == leaf).any())
        assert nodes[first_leaf + leaf] == pri[last_row][np.flatnonzero(leaves[last_row] == leaf)[0]], leaf
    group.close(), twin_group.close()


def test_six_calls_back_to_back_then_a_member_alone():
    """Six calls without a host synchronisation between them (more than ``IDQN_STEPS_STAGING_DEPTH``: a block is reused), compared
    after the last; then one solo ``idqn_per_learn_on_replay`` on member 1 of both sides: members remain drivable alone."""
    import torch

    from slimdqn import _hip

    assert 6 > _hip.STEPS_STAGING_DEPTH
    members, twins, rows, twin_rows, _, group, twin_group = _parity(3, [3, 2, 32, 1, 3, 2], 32, "back to back", each=False)
    u = np.random.default_rng(23).random((1, 32))
    for lr, r in ((members[1], rows[1]), (twins[1], twin_rows[1])):
        frames, n_frames, frame_bytes, ring_rows, stack = lr.rb.ring_view()[:5]
        p = _per(_hip.PerStep(), lr, u, r, row=0)
        _hip.check(_hip.lib().idqn_per_learn_on_replay(lr.agent._handle, C.byref(p), _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(ring_rows),
                                                       32, int(stack), 32, 0, _hip.current_stream()), "idqn_per_learn_on_replay")
    torch.cuda.synchronize()
    _assert_equal(_snapshot(members, rows), _snapshot(twins, twin_rows), "a solo step afterwards")
    assert (members[1].agent._count.cpu().numpy() == 44).all()
    group.close(), twin_group.close()


def test_the_four_group_learner_entries_share_one_ring():
    """S = 2, B = 7: eight learner calls back to back, no host synchronisation between them, through the four group learner
    entries -- the prioritized single call, the plain n-step call (n = 3), the prioritized n-step call (n = 3), the plain single
    call -- against the same calls on the twins with a ``torch.cuda.synchronize()`` after each.  Eight is twice
    ``IDQN_STEPS_STAGING_DEPTH``: every block of the group's staging ring is written a second time while earlier calls may still be
    running.  The second round starts one entry later than the first, so on a ring of four blocks a block's second writer is
    another entry, with another layout, than its first.  The plain calls take the slots a prioritized draw could have given
    (any index below the member's item count)."""
    import torch

    from slimdqn import _hip

    S, B, n, calls = 2, 7, 3, 8
    assert calls > _hip.STEPS_STAGING_DEPTH
    assert _hip.STEPS_STAGING_DEPTH == 4, "the schedule below is worked out for a ring of four blocks: two rounds of the four entries"
    members, twins = _sets(S, B=B)
    rng = np.random.default_rng(29)
    rows, twin_rows = [_Rows(lr, n, B) for lr in members], [_Rows(lr, n, B) for lr in twins]
    group, twin_group = _Group(members), _Group(twins)
    script = []  # (entry, its uniforms [S] x [steps][B] or slots [S][steps][B]), the same for both sides
    for c in range(calls):
        entry = (c + c // _hip.STEPS_STAGING_DEPTH) % 4
        steps = n if entry in (1, 2) else 1
        if entry in (0, 2):
            script.append((entry, _uniforms(rng, S, steps, B)))
        else:
            script.append((entry, np.stack([rng.integers(0, len(lr.sampler), (steps, B)) for lr in members]).astype(np.int32)))
    assert sorted(e for e, _ in script) == [0, 0, 1, 1, 2, 2, 3, 3]

    def run(grp, rws, sync):
        lib, q = _hip.lib(), _hip.current_stream()
        for entry, x in script:
            if entry == 0:
                grp.singles(x, rws)
            elif entry == 2:
                grp.steps(x, rws)
            elif entry == 1:
                _hip.check(lib.idqn_group_learn_steps_on_replay_fc(grp.g, grp.rings(), x.ctypes.data, n, B, B, 0, q), "idqn_group_learn_steps_on_replay_fc")
            else:
                _hip.check(lib.idqn_group_learn_on_replay_fc(grp.g, grp.rings(), x.ctypes.data, B, B, 0, q), "idqn_group_learn_on_replay_fc")
            if sync:
                torch.cuda.synchronize()

    run(group, rows, False)
    run(twin_group, twin_rows, True)
    torch.cuda.synchronize()
    _assert_equal(_snapshot(members, rows), _snapshot(twins, twin_rows), "four entries on one ring")
    for lr in members:
        assert (lr.agent._count.cpu().numpy() == 2 * (1 + n + n + 1)).all() and np.isfinite(lr.agent._losses.cpu().numpy()).all()
    group.close(), twin_group.close()


def test_refusals_leave_everything_untouched():
    import torch

    from slimdqn import _hip

    S, n, B = 3, 3, 32
    members, twins = _sets(S)
    group = _Group(members)
    Us = _uniforms(np.random.default_rng(9), S, n, B)
    rows, twin_rows = [_Rows(lr, n, B) for lr in members], [_Rows(lr, n, B) for lr in twins]
    before = _snapshot(members, rows)
    lib, fn = _hip.lib(), getattr(_hip.lib(), NAME)
    other, tree = rows[0], lambda g: members[g].sampler._sum_tree
    cases = [
        (dict(n=0), "n_steps 0"), (dict(n=33), "n_steps 33"), (dict(n=-1), "n_steps -1"),
        (dict(B=0), "batch 0"), (dict(B=33), "batch 33"),
        (dict(flags=_hip.F_GRADS_ONLY), "takes no flags"), (dict(flags=_hip.F_PROFILE), "takes no flags"),
        (dict(div=31), "mean divisor"),
    ]
    cases += [(dict(fields={1: {f: None}}), "member 1: null pointer")
              for f in ("nodes_dev", "uniforms_host", "leaves_dev", "weights_dev", "td_abs_dev", "tree_scratch_dev")]
    cases += [
        (dict(fields={1: dict(depth=0)}), "member 1: depth"), (dict(fields={1: dict(depth=32)}), "member 1: depth"),
        (dict(fields={2: dict(n_items=0)}), "member 2: n_items"),
        (dict(fields={1: dict(nodes_dev=tree(0)._nodes_dev.data_ptr())}), "members 0 and 1: two members name the same nodes_dev"),
        (dict(fields={1: dict(leaves_dev=other.leaves.data_ptr())}), "members 0 and 1: two members name the same leaves_dev"),
        (dict(fields={2: dict(weights_dev=other.weights.data_ptr())}), "members 0 and 2: two members name the same weights_dev"),
        (dict(fields={2: dict(td_abs_dev=rows[1].td_abs.data_ptr())}), "members 1 and 2: two members name the same td_abs_dev"),
        (dict(fields={1: dict(tree_scratch_dev=tree(0)._scratch.data_ptr())}), "members 0 and 1: two members name the same tree_scratch_dev"),
        (dict(fields={1: dict(priorities_dev=other.priorities.data_ptr())}), "members 0 and 1: two members name the same priorities_dev"),
        (dict(fields={2: dict(max_priority_dev=members[0].sampler._max_priority_dev.data_ptr())}),
         "members 0 and 2: two members name the same max_priority_dev"),
    ]
    for kw, match in cases:
        rc = group.call(Us, rows, **kw)
        msg = lib.idqn_last_error().decode()
        assert rc == _hip.E_INVALID and msg.startswith(NAME + ":") and match in msg, (kw, rc, msg)
    per = (_hip.PerSteps * S)()
    for g in range(S):
        _per(per[g], members[g], Us[g], rows[g])
    for args in ((group.g, group.rings(), None), (group.g, None, per), (None, group.rings(), per)):
        assert fn(*args, n, B, B, 0, _hip.current_stream()) == _hip.E_INVALID
        assert lib.idqn_last_error().decode() == NAME + ": null pointer"
    # what idqn_learn_on_replay_fc_dev refuses for a member's ring
    rings = group.rings()
    rings[1].stack = 3
    assert group.call(Us, rows, rings=rings) == _hip.E_INVALID
    assert lib.idqn_last_error().decode().startswith(NAME + ":") and "stack 3" in lib.idqn_last_error().decode()
    rings = group.rings()
    rings[2].rows_dev = None
    assert group.call(Us, rows, rings=rings) == _hip.E_INVALID and lib.idqn_last_error().decode().startswith(NAME + ":")
    # a member with idqn_set_per_buffers set
    _hip.check(lib.idqn_set_per_buffers(members[1].agent._handle, _hip.ptr(rows[1].weights), _hip.ptr(rows[1].td_abs)), "idqn_set_per_buffers")
    assert group.call(Us, rows) == _hip.E_INVALID
    msg = lib.idqn_last_error().decode()
    assert msg.startswith(NAME + ": member 1") and "idqn_set_per_buffers" in msg
    _hip.check(lib.idqn_set_per_buffers(members[1].agent._handle, None, None), "idqn_set_per_buffers")
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(members, rows), "after the refusals")
    # the next valid call gives the twins' result; the optional outputs of member 1 NULL on both sides
    null = dict(priorities_dev=None, max_priority_dev=None)
    before_max = members[1].sampler._max_priority_dev.clone()
    group.steps(Us, rows, fields={1: null})
    for g, (t, U, r) in enumerate(zip(twins, Us, twin_rows)):
        frames, n_frames, frame_bytes, ring_rows, stack = t.rb.ring_view()[:5]
        p = _per(_hip.PerSteps(), t, U, r, **(null if g == 1 else {}))
        _hip.check(lib.idqn_per_learn_steps_on_replay(t.agent._handle, C.byref(p), _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(ring_rows), n,
                                                      B, int(stack), B, 0, _hip.current_stream()), "idqn_per_learn_steps_on_replay")
    torch.cuda.synchronize()
    _assert_equal(_snapshot(members, rows), _snapshot(twins, twin_rows), "after a valid call")
    assert (rows[1].priorities == -1.0).all().item() and members[1].sampler._max_priority_dev.equal(before_max)
    group.close()


# ---- PrioritizedGroupLearner ----------------------------------------------------------------------------------------------
LEARNER_STATE = ("_leaves", "_weights", "_td_abs", "_priorities")


def _learner_snapshot(learners):
    out = []
    for lr in learners:
        d = {n: getattr(lr.agent, n).clone() for n in AGENT_STATE + ("_target",)}
        d.update({n: getattr(lr, n).clone() for n in LEARNER_STATE})
        d["nodes"] = lr.sampler._sum_tree._nodes_dev.clone()
        d["max_priority"] = lr.sampler._max_priority_dev.clone()
        out.append(d)
    return out


def _group_learner(members, **kw):
    from slimdqn.networks.group import AgentGroup
    from slimdqn.sample_collection.per import PrioritizedGroupLearner

    group = AgentGroup([lr.agent for lr in members])
    gl = PrioritizedGroupLearner(group, [lr.rb for lr in members], **kw)
    gl.learners = members  # (the learners under test: their settings differ per member)
    gl.group_per_steps_sizes, gl.group_per_steps_min = frozenset({len(members)}), 2  # the route is what is under test, whatever ships
    return group, gl


@pytest.mark.parametrize("steps_env", ["1", "0"])
def test_group_learner_steps_equal_n_steps_of_the_members_learners(monkeypatch, steps_env):
    """``steps(3)`` then ``steps(34)`` (two chunks: 32 + 2) against 37 ``PrioritizedLearner.step`` calls per twin, member by member:
    agents, trees, the learners' buffers (the last step's rows) and the sampler generators.  With ``IDQN_PER_STEPS=0`` the single
    group steps run and give the same bytes."""
    import torch

    monkeypatch.setenv("IDQN_PER_STEPS", steps_env)
    members, twins = _sets(3)
    group, gl = _group_learner(members)
    gl.group_per_sizes = frozenset({3})
    for n in (3, 34):
        losses = [x.clone() for x in gl.steps(n)]
    for t in twins:  # (a member's generator and tree are its own: member by member is the same script)
        for _ in range(37):
            want = t.step()
    torch.cuda.synchronize()
    assert gl.__dict__.get("_group_per_steps_ok") is (True if steps_env == "1" else None), "the wrong route ran"
    assert gl.__dict__.get("_group_per_ok") is (None if steps_env == "1" else True)
    _assert_equal(_learner_snapshot(gl.learners), _learner_snapshot(twins), ("group learner", steps_env))
    assert losses[2].cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    for lr, t in zip(gl.learners, twins):
        assert lr.sampler._rng_key.bit_generator.state == t.sampler._rng_key.bit_generator.state
    assert (members[0].agent._count.cpu().numpy() == 37).all()
    group.close()


def test_group_learner_update_params_many_across_target_operations():
    """Steps 1 .. 13 with a target update every 6 and a target sync every 4 steps inside the run: against the loop ``step();
    update_target_params(s)`` on every twin."""
    import torch

    per_member = [dict(m, schedule=(6, 4)) for m in (MEMBERS[0], MEMBERS[2], MEMBERS[3])]
    members, twins = _sets(3, per_member=per_member)
    group, gl = _group_learner(members)
    got = gl.update_params_many(1, 13)
    want = []
    for t in twins:
        logs = []
        for s in range(1, 14):
            t.step()
            updated, rec = t.agent.update_target_params(s)
            if updated:
                logs.append((s, rec))
        want.append(logs)
    torch.cuda.synchronize()
    assert gl._group_per_steps_ok is True
    assert [[s for s, _ in m] for m in got] == [[s for s, _ in m] for m in want] and all(len(m) >= 2 for m in got)
    assert [[sorted(r) for _, r in m] for m in got] == [[sorted(r) for _, r in m] for m in want]
    _assert_equal(_learner_snapshot(gl.learners), _learner_snapshot(twins), "update_params_many")
    for lr, t in zip(gl.learners, twins):
        assert lr.sampler._rng_key.bit_generator.state == t.sampler._rng_key.bit_generator.state
    group.close()


# ---- SeedVectorTrainer(..., learner=) -----------------------------------------------------------------------------------------
def _trainer_side(S, E, initial):
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    out = []
    for g in range(S):
        p = dict(seed=g, epsilon_end=0.05, epsilon_duration=80, n_epochs=2, n_training_steps_per_epoch=70 + 10 * g, n_initial_samples=initial[g],
                 horizon=30, wandb=NullLogger())
        agent = iDQN(prng.PRNGKey(200 + g), 8, 4, 2, [16], "fc", 1e-3, 0.99, 1, 1, 20, 5, adam_eps=1e-8)
        envs = [SyntheticVector(10 * g + e, episode_length=(13, 9)[e % 2]) for e in range(E)]
        rb = VectorReplayBuffer(SlotPrioritizedSampler(g, 150, 0.6), 32, 150, stack_size=1, update_horizon=1, gamma=0.99, n_envs=E)
        rb.reuse_sample_buffers = True
        out.append((prng.PRNGKey(300 + g), p, agent, envs, rb, PrioritizedLearner(agent, rb, beta=0.5)))
    return out


@pytest.mark.parametrize("initial", [(40, 40, 40), (40, 52, 40)])
def test_seed_vector_trainer_with_a_learner_equals_vector_trainers(initial):
    """S = 3, E = 2, two epochs per seed (a few hundred lock-step iterations): per seed, returns and lengths, parameters, moments,
    counters, replay rows, tree nodes, sampler generator and log records against ``VectorTrainer(..., learner=)`` alone on the
    same key.  With different ``n_initial_samples`` the seeds' runs differ for a while: the per-member path runs."""
    import torch

    from experiments.base.dqn import VectorTrainer
    from experiments.base.seeds import SeedVectorTrainer
    from slimdqn.networks.group import AgentGroup
    from slimdqn.sample_collection.per import PrioritizedGroupLearner

    S, E = 3, 2
    solo, together = _trainer_side(S, E, initial), _trainer_side(S, E, initial)
    want = [VectorTrainer(*side[:5], learner=side[5]).run() for side in solo]
    keys, ps, agents, envs, rbs, learners = (list(x) for x in zip(*together))
    group = AgentGroup(agents)
    gl = PrioritizedGroupLearner(group, rbs, beta=0.5)
    gl.group_per_steps_sizes, gl.group_per_steps_min = frozenset({S}), 2  # a vector step owes E = 2 gradient steps
    member_calls = []
    for i, lr in enumerate(gl.learners):
        real = lr.update_params_many
        lr.update_params_many = lambda first, n, i=i, real=real: member_calls.append(i) or real(first, n)
    got = SeedVectorTrainer(keys, ps, agents, envs, rbs, group=group, learner=gl).run()
    torch.cuda.synchronize()
    assert gl.__dict__.get("_group_per_steps_ok") is True, "the n-step group call never ran"
    assert member_calls, "a seed that outlives the others learns alone at the end"
    if len(set(initial)) > 1:
        assert member_calls[0] in (0, 2), "seeds 0 and 2 learn before seed 1 does: their own learners"
    for g in range(S):
        a, b = agents[g], solo[g][2]
        for name in AGENT_STATE + ("_target",):
            assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), (g, name)
        ra, rb = rbs[g], solo[g][4]
        assert ra._add_count == rb._add_count > 100 and np.array_equal(ra._plan.rows, rb._plan.rows)
        assert np.array_equal(ra._meta_dev.cpu().numpy(), rb._meta_dev.cpu().numpy())
        sa, sb = ra._sampling_distribution, rb._sampling_distribution
        assert sa._sum_tree._nodes_dev.cpu().numpy().tobytes() == sb._sum_tree._nodes_dev.cpu().numpy().tobytes(), (g, "tree nodes")
        assert sa._max_priority_dev.cpu().numpy().tobytes() == sb._max_priority_dev.cpu().numpy().tobytes()
        assert sa._rng_key.bit_generator.state == sb._rng_key.bit_generator.state
        assert ps[g]["wandb"].records == solo[g][1]["wandb"].records
        assert int(a._count[0].item()) > 50
        assert [list(x) for x in got[g]] == [list(x) for x in want[g]]
