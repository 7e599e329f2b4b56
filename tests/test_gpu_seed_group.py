"""GPU: seed groups -- S independent MLP handles learn and act in one launch (``idqn_group_*``, ``slimdqn.networks.group``).

Every comparison is WITHOUT a tolerance, against twins: fresh agents created with the member's hyper-parameters, given the
member's state (parameters, target, moments, gradient arena, counters, running loss sums) as it was before the call, and driven
through the existing single-handle entries (``idqn_learn_on_replay_fc``, ``idqn_target_update``, ``idqn_act_host``) with the same
slots.  Members of a group differ in parameters, rings, learning rate, Adam epsilon and gamma.

Shapes: the LunarLander net (obs 8, [100, 100], A 4, K 3, B 32) and a ragged one ([33, 70], A 3, K 2, B 7: edge tiles, rows
past the batch end) at obs 5 / stack 1 and -- a stack of two needs an even feature count, frame_bytes * stack == 4 * obs -- at
obs 6 = frames of 3 x stack 2, with sampled elements whose stack crosses an episode start (valid frames < stack).
"""
import ctypes as C

import numpy as np
import pytest

import fc_shapes as F

pytestmark = pytest.mark.gpu

#         frame  stack  obs  features    K  A  B
SHAPES = {
    "lunar": ((8,), 1, 8, [100, 100], 3, 4, 32),
    "ragged": ((5,), 1, 5, [33, 70], 2, 3, 7),
    "ragged_stack2": ((3,), 2, 6, [33, 70], 2, 3, 7),
}
# Rows of the one-launch step's shape table (tests/fc_shapes.py) as member shapes "shape_<row>": odd din, 33- and 128-wide layers,
# A = 1, d0 = 128, B = 1 and the net within 2 KB of the LDS budget, two members each
SHAPES.update({"shape_" + rid: ((F.BY_ID[rid].d0,), 1, F.BY_ID[rid].d0, list(F.BY_ID[rid].feats), F.BY_ID[rid].K, F.BY_ID[rid].A, F.BY_ID[rid].B)
               for rid in F.DESCENDANT_ROWS})
TABLE_SHAPES = ["shape_" + rid for rid in F.DESCENDANT_ROWS]
HYPER = [(1e-3, 1e-8, 0.99), (3e-4, 1.5e-4, 0.9), (2e-3, 1e-6, 0.95), (5e-4, 1e-7, 0.999)]  # lr, Adam eps, gamma per member
ARENAS = ("_online", "_target", "_mu", "_nu", "_grad", "_count", "_cum")
CAPACITY = 40


def _agent(shape, g, feats=None, arch="fc", max_tsf=10**9):
    from slimdqn.networks.idqn import iDQN

    _, _, obs, f, K, A, _ = SHAPES[shape]
    lr, eps, gamma = HYPER[g % len(HYPER)]
    a = iDQN(100 + g, obs, A, K, feats or f, arch, lr, gamma, 2, 1, 10**9, max_tsf, adam_eps=eps)
    a._target.copy_(a._online * 0.5 + 0.01 * (g + 1))  # a target net that is not the online net
    return a


def _twin(shape, g, member, **kw):
    """A freshly created agent in the member's state."""
    t = _agent(shape, g, **kw)
    for name in ARENAS:
        getattr(t, name).copy_(getattr(member, name))
    return t


def _same(a, b, what=""):
    for name in ARENAS:
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert x.tobytes() == y.tobytes(), f"{what}: {name} differs"


def _snapshot(agents):
    return [{n: getattr(a, n).cpu().numpy().tobytes() for n in ARENAS} for a in agents]


def _buffer(shape, g, vector=False):
    """A ring that has wrapped, episodes of 7 (vector: 5 and 9) steps, its own data and sampler seed per member."""
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    frame, stack, _, _, _, A, B = SHAPES[shape]
    rng = np.random.default_rng(50 + g)
    tr = lambda last: TransitionElement(rng.standard_normal(frame).astype(np.float32), int(rng.integers(A)), float(rng.normal()), last, last)
    if vector:
        rb = VectorReplayBuffer(UniformSamplingDistribution(g), B, CAPACITY, stack_size=stack, update_horizon=2, gamma=0.99, n_envs=2, segment=24)
        n = [0, 0]
        for _ in range(24 * 2 + 3):
            row = []
            for e, length in enumerate((5, 9)):
                n[e] = (n[e] + 1) % length
                row.append(tr(n[e] == 0))
            rb.add_many(row)
    else:
        rb = ReplayBuffer(UniformSamplingDistribution(g), batch_size=B, max_capacity=CAPACITY, stack_size=stack, update_horizon=2, gamma=0.99)
        for i in range(150):
            rb.add(tr(i % 7 == 6))
    rb.reuse_sample_buffers = True
    return rb


def _rows(rb, slots):
    return (rb._plan.rows if hasattr(rb, "_plan") else rb._meta)[np.asarray(slots)]


def _draw(rb, shape, n=1):
    """[n][B] live slots; for a stack of two every draw holds an element with fewer valid frames than the stack."""
    stack = SHAPES[shape][1]
    draws = np.stack([np.asarray(rb.sample_slots(), np.int32) for _ in range(n)])
    if stack > 1:
        live = np.unique(np.concatenate([np.asarray(rb.sample_slots(), np.int32) for _ in range(40)]))
        rows = _rows(rb, live)
        short = live[(rows[:, 1] < stack) | (rows[:, 3] < stack)]
        assert short.size, "the ring holds no element whose stack crosses an episode start"
        draws[:, 0] = short[0]
        draws[:, -1] = short[-1]
    return np.ascontiguousarray(draws, np.int32)


def _solo(agent, rb, slots, flags=0):
    from slimdqn import _hip

    frames, n_frames, frame_bytes, rows, stack = rb.ring_view()[:5]
    slots = np.ascontiguousarray(slots, np.int32)
    agent._ensure_handle(32)
    _hip.check(_hip.lib().idqn_learn_on_replay_fc(agent._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                                  slots.ctypes.data, int(slots.size), int(stack), int(slots.size), flags,
                                                  _hip.current_stream()), "idqn_learn_on_replay_fc")


class _Group:
    """The C group over agents' handles."""

    def __init__(self, agents, check=True):
        from slimdqn import _hip

        for a in agents:
            a._ensure_handle(32)
        self.agents, self.g = agents, C.c_void_p()
        arr = (C.c_void_p * len(agents))(*[a._handle.value for a in agents])
        self.rc = _hip.lib().idqn_group_create(arr, len(agents), C.byref(self.g))
        if check:
            _hip.check(self.rc, "idqn_group_create")

    def rings(self, rbs):
        from slimdqn.networks.group import AgentGroup

        self._views = [rb.ring_view() for rb in rbs]
        return AgentGroup._rings(self._views)

    def learn(self, rbs, slots, flags=0, B=None):
        """slots [S][B]"""
        from slimdqn import _hip

        slots = np.ascontiguousarray(slots, np.int32)
        B = slots.shape[-1] if B is None else B
        return _hip.lib().idqn_group_learn_on_replay_fc(self.g, self.rings(rbs), slots.ctypes.data, B, B, flags, _hip.current_stream())

    def learn_steps(self, rbs, slots):
        """slots [S][n][B]"""
        from slimdqn import _hip

        slots = np.ascontiguousarray(slots, np.int32)
        return _hip.lib().idqn_group_learn_steps_on_replay_fc(self.g, self.rings(rbs), slots.ctypes.data, slots.shape[1], slots.shape[2],
                                                              slots.shape[2], 0, _hip.current_stream())

    def close(self):
        from slimdqn import _hip

        if self.g:
            _hip.lib().idqn_group_destroy(self.g)
            self.g = C.c_void_p()


def _last_error():
    from slimdqn import _hip

    return _hip.lib().idqn_last_error().decode()


def _members(shape, S, vector_member=None):
    agents = [_agent(shape, g) for g in range(S)]
    rbs = [_buffer(shape, g, vector=(g == vector_member)) for g in range(S)]
    return agents, rbs


@pytest.mark.parametrize("shape,S,vector_member", [("lunar", 3, None), ("ragged", 2, 1), ("ragged_stack2", 2, 1), ("lunar", 1, None)]
                         + [(name, 2, None) for name in TABLE_SHAPES])
@pytest.mark.parametrize("flags", [0, 1])  # 1: IDQN_F_GRADS_ONLY
def test_group_step_equals_solo_steps(shape, S, vector_member, flags):
    """Two group calls (the second on warm moments); after each, every member equals its twin stepped alone."""
    import torch

    from slimdqn import _hip

    agents, rbs = _members(shape, S, vector_member)
    group = _Group(agents)
    for call in range(2):
        twins = [_twin(shape, g, a) for g, a in enumerate(agents)]
        slots = np.stack([_draw(rb, shape)[0] for rb in rbs])
        _hip.check(group.learn(rbs, slots, flags), "idqn_group_learn_on_replay_fc")
        for t, rb, s in zip(twins, rbs, slots):
            _solo(t, rb, s, flags)
        torch.cuda.synchronize()
        for g, (a, t) in enumerate(zip(agents, twins)):
            _same(a, t, f"call {call}, member {g}")
            assert np.isfinite(a._losses.cpu().numpy()).all()
            assert (a._count.cpu().numpy() == (call if flags else call + 1)).all()
        if flags:  # (a gradient-only step changes no parameter: make the second call's state differ anyway)
            for rb, a, s in zip(rbs, agents, slots):
                _solo(a, rb, s)
    assert len({a._online.cpu().numpy().tobytes() for a in agents}) == S, "the members were meant to differ"
    group.close()


def test_history_of_group_and_solo_calls():
    """Five group steps with a solo step on member 0 and a target update on member 1 in between: after EVERY call each member
    equals a freshly created twin given the member's state before the call and the same operation through the solo entries."""
    import torch

    from slimdqn import _hip

    shape, S = "lunar", 3
    agents, rbs = _members(shape, S)
    group = _Group(agents)
    ops = ["group", "solo0", "group", "target1", "group", "group", "solo0", "group"]
    for i, op in enumerate(ops):
        twins = [_twin(shape, g, a) for g, a in enumerate(agents)]
        slots = np.stack([_draw(rb, shape)[0] for rb in rbs])
        if op == "group":
            _hip.check(group.learn(rbs, slots), "idqn_group_learn_on_replay_fc")
            for t, rb, s in zip(twins, rbs, slots):
                _solo(t, rb, s)
        elif op == "solo0":
            _solo(agents[0], rbs[0], slots[0])
            _solo(twins[0], rbs[0], slots[0])
        else:
            agents[1]._local_target_update()
            twins[1]._local_target_update()
        torch.cuda.synchronize()
        for g, (a, t) in enumerate(zip(agents, twins)):
            _same(a, t, f"after call {i} ({op}), member {g}")
    assert [int(a._count[0].item()) for a in agents] == [7, 5, 5]
    group.close()


@pytest.mark.parametrize("n", [1, 2, 5, 7])
@pytest.mark.parametrize("shape,S,vector_member", [("lunar", 3, None), ("ragged_stack2", 2, 1)] + [(name, 2, None) for name in TABLE_SHAPES])
def test_group_n_steps_equal_n_group_steps_and_n_solo_steps(n, shape, S, vector_member):
    import torch

    from slimdqn import _hip

    agents, rbs = _members(shape, S, vector_member)
    singles = [_twin(shape, g, a) for g, a in enumerate(agents)]
    solos = [_twin(shape, g, a) for g, a in enumerate(agents)]
    many, single = _Group(agents), _Group(singles)
    for call in range(2):  # (the second call starts from warm moments and a count > 0)
        slots = np.stack([_draw(rb, shape, n) for rb in rbs])  # [S][n][B]
        _hip.check(many.learn_steps(rbs, slots), "idqn_group_learn_steps_on_replay_fc")
        for i in range(n):
            _hip.check(single.learn(rbs, slots[:, i]), "idqn_group_learn_on_replay_fc")
            for t, rb, s in zip(solos, rbs, slots[:, i]):
                _solo(t, rb, s)
        torch.cuda.synchronize()
        for g in range(S):
            _same(agents[g], solos[g], f"call {call}: n-step group call vs n solo steps, member {g}")
            _same(singles[g], solos[g], f"call {call}: n group steps vs n solo steps, member {g}")
            assert (agents[g]._count.cpu().numpy() == n * (call + 1)).all()
    many.close(), single.close()


@pytest.mark.parametrize("n", [1, 3, 32])
@pytest.mark.parametrize("shape,S", [("lunar", 3), ("ragged", 2)] + [(name, 2) for name in TABLE_SHAPES])
def test_group_acting_equals_act_host_on_the_member(n, shape, S):
    """Members in shuffled order, several states on one member with different heads, both parameter sets; the single-state
    reference runs blocking and as a begin / end pair (``lazy_host_actions``)."""
    import torch

    from slimdqn import _hip

    obs, K, A = SHAPES[shape][2], SHAPES[shape][4], SHAPES[shape][5]
    agents, _ = _members(shape, S)
    group = _Group(agents)
    rng = np.random.default_rng(n)
    pin = torch.zeros((33, obs), dtype=torch.float32).pin_memory()
    q_out = torch.empty((33, A), dtype=torch.float32, device="cuda")
    acts = torch.empty(40, dtype=torch.int32).pin_memory()
    for which in (0, 1):
        for rep in range(2):  # (the second call replays the captured graph with another assignment)
            states = rng.standard_normal((n, obs)).astype(np.float32)
            member = np.ascontiguousarray(rng.permutation(np.arange(n) % S), np.int32)
            heads = np.ascontiguousarray((np.arange(n) // S + rep) % K, np.int32)
            if n >= 3:
                member[:3], heads[:3] = S - 1, [0, K - 1, 0]  # several states on one member, different heads
            pin[:n] = torch.from_numpy(states)
            q_out.fill_(-7.0), acts.fill_(-9)
            torch.cuda.synchronize()
            _hip.check(_hip.lib().idqn_group_act_host_fc(group.g, which, member.ctypes.data, heads.ctypes.data, C.c_void_p(pin.data_ptr()), n,
                                                         _hip.ptr(q_out), C.c_void_p(acts.data_ptr()), _hip.current_stream()),
                       "idqn_group_act_host_fc")
            got_a = acts.numpy().copy()  # (the call has returned: the actions are there without a synchronisation)
            got_q = q_out.cpu().numpy()
            assert (got_q[n:] == -7.0).all() and (got_a[n:] == -9).all()
            for e in range(n):
                a = agents[member[e]]
                a.lazy_host_actions = bool((e + rep) % 2)
                want_a = int(a._best_action(which, int(heads[e]), states[e]).item())
                a.lazy_host_actions = False
                want_q = a._q_out[0].cpu().numpy()
                assert got_q[e].tobytes() == want_q.tobytes(), (which, rep, e)
                assert got_a[e] == want_a, (which, rep, e)
    group.close()


def test_agent_group_is_the_agents_alone():
    """``AgentGroup`` on real buffers against the same agents driven alone: state bytes and every sampler's generator state, for
    single steps, ``update_params_many`` (runs cut by target syncs and an update) and acting with a lazy action pending."""
    import torch

    from slimdqn import prng
    from slimdqn.networks.group import AgentGroup

    shape, S = "lunar", 3
    mk = lambda: ([_agent(shape, g, max_tsf=6) for g in range(S)], [_buffer(shape, g) for g in range(S)])
    (ga, grb), (sa, srb) = mk(), mk()
    for a in ga + sa:
        a.target_update_frequency = 18
    group = AgentGroup(ga)
    for step in range(3):
        group.update_online_params(step, grb)
        for a, rb in zip(sa, srb):
            a.update_online_params(step, rb)
    got = group.update_params_many(3, 30, grb)
    want = [a.update_params_many(3, 30, rb) for a, rb in zip(sa, srb)]
    torch.cuda.synchronize()
    assert group.__dict__.get("_group_learn_ok") is True and group.__dict__.get("_group_steps_ok") is True
    assert [[s for s, _ in o] for o in got] == [[s for s, _ in o] for o in want] and got[0], "a target update was due"
    for o, w in zip(got, want):
        for (_, a), (_, b) in zip(o, w):
            assert a == b
    for g in range(S):
        _same(ga[g], sa[g], f"member {g}")
        assert grb[g]._sampling_distribution._rng_key.bit_generator.state == srb[g]._sampling_distribution._rng_key.bit_generator.state
    states = np.random.default_rng(3).standard_normal((S, SHAPES[shape][2])).astype(np.float32)
    keys = [prng.PRNGKey(40 + g) for g in range(S)]
    ga[1].lazy_host_actions = True
    pending = ga[1]._best_action(0, 0, states[1])  # nobody collected it: the group call does
    ga[1].lazy_host_actions = False
    got = group.best_actions(0, group.select_heads(keys), list(states))
    assert ga[1]._act_in_flight is None and isinstance(pending.item(), int)
    want = [int(a.best_action(a.params, s, k).item()) for a, s, k in zip(sa, states, keys)]
    assert got.tolist() == want and group.__dict__.get("_group_act_ok") is True
    group.close()


def test_refusals_leave_every_member_unchanged():
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    shape = "lunar"
    agents, rbs = _members(shape, 3)
    before = _snapshot(agents)
    slots = np.stack([_draw(rb, shape)[0] for rb in rbs])

    def refused(rc, text):
        assert rc == _hip.E_INVALID and text in _last_error(), (rc, text, _last_error())

    cnn = iDQN(0, (12, 10, 2), 3, 3, [2, 3, 1, 15], "cnn", 1e-3, 0.99, 2, 1, 10**9, 10**9)
    g = _Group([agents[0], cnn], check=False)
    refused(g.rc, "not an MLP")
    g = _Group([agents[0], _agent(shape, 1, feats=[100, 90])], check=False)
    refused(g.rc, "differs from member 0")
    g = _Group([agents[0], agents[1], agents[0]], check=False)
    refused(g.rc, "same handle")
    wide = [_agent(shape, g, feats=[520]) for g in range(2)]
    g = _Group(wide, check=False)
    refused(g.rc, "outside the one-launch step")
    out = C.c_void_p()
    refused(_hip.lib().idqn_group_create((C.c_void_p * 33)(*[agents[0]._handle.value] * 33), 33, C.byref(out)), "33 members")
    # B = 33: members that take such batches, a group that does not
    big = [_agent(shape, g) for g in range(2)]
    for a in big:
        a._ensure_handle(64)
    g = _Group.__new__(_Group)
    g.agents, g.g = big, C.c_void_p()
    arr = (C.c_void_p * 2)(*[a._handle.value for a in big])
    _hip.check(_hip.lib().idqn_group_create(arr, 2, C.byref(g.g)), "idqn_group_create")
    big_before = _snapshot(big)
    s33 = np.stack([np.resize(_draw(rb, shape)[0], 33) for rb in rbs[:2]])
    refused(g.learn(rbs[:2], s33), "batch 33")
    torch.cuda.synchronize()
    assert _snapshot(big) == big_before
    g.close()
    # a member with prioritized-replay buffers set; a flag the group does not take
    group = _Group(agents)
    w, td = torch.ones(32, device="cuda"), torch.zeros((3, 32), device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(agents[1]._handle, _hip.ptr(w), _hip.ptr(td)), "idqn_set_per_buffers")
    refused(group.learn(rbs, slots), "prioritized-replay buffers")
    refused(group.learn_steps(rbs, np.stack([slots] * 2, axis=1)), "prioritized-replay buffers")
    _hip.check(_hip.lib().idqn_set_per_buffers(agents[1]._handle, None, None), "idqn_set_per_buffers")
    refused(group.learn(rbs, slots, flags=2), "IDQN_F_GRADS_ONLY only")
    torch.cuda.synchronize()
    assert _snapshot(agents) == before
    _hip.check(group.learn(rbs, slots), "idqn_group_learn_on_replay_fc")  # ... and the group still serves
    torch.cuda.synchronize()
    assert _snapshot(agents) != before
    group.close()


def test_seeds_entry_point_equals_single_seed_runs(tmp_path):
    """``experiments/lunar_lander/idqn_seeds.py`` on seeds 3..5 against ``experiments/lunar_lander/idqn.py`` once per seed: every
    agent's bytes and every log record."""
    import torch

    from experiments.lunar_lander import idqn, idqn_seeds

    flags = ["-en", "seeds", "-ne", "2", "-ntspe", "90", "-nis", "40", "-ed", "60", "-tuf", "20", "-tsf", "5", "-rbc", "150", "-horizon", "25"]
    ps, agents = idqn_seeds.run(flags + ["--first_seed", "3", "--last_seed", "5"], save_root=str(tmp_path / "group"))
    assert [p["seed"] for p in ps] == [3, 4, 5]
    for p, a in zip(ps, agents):
        p1, a1 = idqn.run(flags + ["-s", str(p["seed"])], save_root=str(tmp_path / "solo"))
        torch.cuda.synchronize()
        _same(a, a1, f"seed {p['seed']}")
        assert p["wandb"].records == p1["wandb"].records and any("loss" in r for r in p1["wandb"].records)
        assert int(a._count[0].item()) > 100
