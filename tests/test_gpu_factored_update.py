"""The factored Dense_0 update (``idqn_finish_step_factored``) on the device, at every block count, geometry and factor layout
of tests/factored_shapes.py.

Kernel level: a handle is armed by the first half of a step on a batch of ONE sample (IDQN_F_STOP_BEFORE_DENSE0_WGRAD), then
the update runs on synthetic factors.  Every element of Dense_0/kernel's theta, mu and nu is compared with the fp64 reference;
the three layouts must agree bit for bit; the two phases one after the other must equal both at once; the launches the profile
table lists must be the ones the restated rule names.

End to end: several ranks emulated on one GPU (factored_shapes.emulate_ranks) against the fp64 oracle on the concatenated
batch, ragged shards and importance weights included, and a second chained step.

Bars (factored_shapes.bars): gradient recovered from mu' within 2e-5 max |G[k]|, theta' within 3e-7 at the goldens' learning
rate, nu' within what that gradient bar and float32 storage allow.  A figure that misses its bar is held to 4 x the float32
reference's own error on that row instead; the test prints which rows needed that.
"""
import numpy as np
import pytest

import factored_shapes as FS

pytestmark = pytest.mark.gpu


def _agent(geom, K, J, lr=FS.LR, eps=FS.EPS):
    from slimdqn.networks.idqn import iDQN

    obs, convs = FS.GEOMS[geom]
    return iDQN(0, obs, FS.N_ACTIONS, K, convs + [J], "cnn", lr, 0.99, 1, 1, 10**9, 10**9, adam_eps=eps)


def _one_sample(geom):
    from collections import namedtuple

    from oracle import qnet_ref as Q

    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    return Batch(*Q.synthetic_batch(11, 1, FS.GEOMS[geom][0], FS.N_ACTIONS, "cnn"))


def _profile_rows(agent):
    import ctypes as C

    from slimdqn import _hip

    buf = C.create_string_buffer(8192)
    _hip.check(_hip.lib().idqn_profile_table(agent._handle, buf, 8192), "idqn_profile_table")
    rows = {}
    for line in buf.value.decode().splitlines():
        name, _, count = line.split("\t")
        rows[name] = int(count)
    return rows


class _Run:
    """One armed handle; ``update(layout, phases)`` restores the arenas, arms the handle and runs the update."""

    def __init__(self, case):
        import torch

        self.case, self.agent = case, _agent(case.geom, case.K, case.J)
        ag = self.agent
        self.one = _one_sample(case.geom)
        off, shape = next((o, s) for n, o, s in ag._leaves if n == "Dense_0/kernel")
        assert tuple(shape) == (FS.F_OF[case.geom], case.J)
        self.sl = slice(off, off + shape[0] * shape[1])
        theta, mu, nu, count = FS.state(case)
        K = case.K
        for arena, v in ((ag._online, theta), (ag._mu, mu), (ag._nu, nu)):
            arena[:, self.sl] = torch.from_numpy(v.reshape(K, -1)).cuda()
        ag._count.copy_(torch.from_numpy(count.astype(np.int32)))
        self.start = [t.clone() for t in (ag._online, ag._mu, ag._nu, ag._count, ag._cum)]
        self.mu_old = mu

    def update(self, lay, phases=(3,), flags=0):
        import torch

        from slimdqn import _hip

        ag, lib, q = self.agent, _hip.lib(), _hip.current_stream
        for dst, src in zip((ag._online, ag._mu, ag._nu, ag._count, ag._cum), self.start):
            dst.copy_(src)
        # (the bias corrections of the step are written by the first half: it has to see the count of this state)
        ag._learn(self.one, flags=_hip.F_STOP_BEFORE_DENSE0_WGRAD | flags)
        _hip.check(lib.idqn_backward_rest(ag._handle, q()), "rest")
        dev = torch.from_numpy(lay.buf).cuda()
        base = dev.data_ptr()
        assert base % 16 == 0
        for ph in phases:
            _hip.check(lib.idqn_finish_step_factored(ag._handle, base + 4 * lay.a3_off, base + 4 * lay.dh_off, self.case.nb_total,
                                                     self.case.nb_inner, *lay.a3_strides, *lay.dh_strides, ph, q()), "finish")
        torch.cuda.synchronize()
        return [t.clone() for t in (ag._online, ag._mu, ag._nu)]

    def dense0(self, arenas):
        K, F, J = self.case.K, FS.F_OF[self.case.geom], self.case.J
        return [a[:, self.sl].cpu().numpy().reshape(K, F, J) for a in arenas]


def _same_bytes(a, b):
    import torch

    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _check(case, got, want, mu_old, f32):
    """Every element against fp64 under the bars in force; prints the measured maxima and the rows on the fallback bar."""
    errs = FS.errors(got, want, mu_old)
    primary, inforce = FS.bars(want, mu_old, f32)
    fallback = [q for q in errs if (errs[q] > primary[q]).any()]
    print("[factored] %s  grad/max|G| %.3g  theta %.3g  nu/allowance %.3g  (float32 reference: %.3g, %.3g, %.3g)%s" % (
        FS.case_id(case), (errs["grad"] / (primary["grad"] / FS.GRAD_BAR)).max(), errs["theta"].max(), errs["nu"].max(),
        (f32["grad"] / (primary["grad"] / FS.GRAD_BAR)).max(), f32["theta"].max(), f32["nu"].max(),
        "  FALLBACK BAR: " + ", ".join(fallback) if fallback else ""))
    for q in errs:
        assert (errs[q] <= inforce[q]).all(), (FS.case_id(case), q, errs[q], primary[q], inforce[q])


@pytest.mark.parametrize("case", FS.CASES, ids=FS.case_id)
def test_update_against_fp64_at_every_row(case):
    import torch

    from slimdqn import _hip

    a3, dh = FS.factors(case)
    ref = FS.reference(case)
    run = _Run(case)
    lays = {name: build(a3, dh, case.nb_inner) for name, build in FS.LAYOUTS.items()}
    out = run.update(lays["packed"], flags=_hip.F_PROFILE_ALL)
    rows = _profile_rows(run.agent)
    # route: the plane split appears exactly where the restated rule says, the update as ONE line (its one or two launches --
    # one per cache policy of theta' -- share it)
    assert ("factor planes" in rows) == FS.bf3(case.nb_total, case.J), rows
    assert rows.get("factor planes", 1) == 1 and rows.get("dense0 wgrad + adam") == 1, rows
    assert "dense0 wgrad" not in rows and "dense0 wgrad + dgrad + adam" not in rows, rows
    kernels = FS.update_kernels(case.K, FS.F_OF[case.geom], case.J, case.nb_total)
    assert sum(h for _, h in kernels) == case.K and len(kernels) == 1  # (no table row splits the heads between two policies)
    assert (kernels[0][0] == "k_dense0_wgrad_alds<1, true>") == (case.geom == "GA")
    _check(case, run.dense0(out), ref["want"], run.mu_old, ref["f32"])
    assert run.agent._count.cpu().numpy().tolist() == [int(c) + 1 for c in FS.state(case)[3]]
    # layouts: same blocks in the same order -> the same bytes in the three arenas; no NaN of the gaps reaches the output
    for name in ("split", "gapped"):
        other = run.update(lays[name])
        assert _same_bytes(other, out), name
        if name == "gapped":
            assert not any(bool(torch.isnan(t).any()) for t in other)
    # phases: Dense_0 then the rest == both at once
    assert _same_bytes(run.update(lays["packed"], phases=(1, 2)), out)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _e2e_agent(J, R, b):
    from collections import namedtuple

    obs, feats, p, pt, batch = FS.e2e_inputs(J, R, b)
    agent = _agent("G1", FS.E2E_K, J, FS.E2E_LR, FS.E2E_EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    return agent, Batch(*batch), p


def _finish(agent, g, phases=3):
    from slimdqn import _hip

    _hip.check(_hip.lib().idqn_finish_step_factored(*g.finish_args, phases, _hip.current_stream()), "finish")


def _leaf_bars(name, got, want, grad_bar=FS.GRAD_BAR):
    return np.abs(got - want).max() <= grad_bar * np.abs(want).max()


@pytest.mark.parametrize("J", [256, 128])
@pytest.mark.parametrize("R,b", FS.E2E_SHARDS)
def test_emulated_ranks_against_the_oracle(J, R, b):
    """Losses, every leaf's gradient (recovered from mu') and theta' of the step N ranks take together == the fp64 oracle's step on
    the concatenated batch; then a second step from the result, whose theta depends on the first gradient's magnitude."""
    agent, batch, p = _e2e_agent(J, R, b)
    want = FS.e2e_oracle(J, R, b, steps=2)
    f32 = FS.e2e_oracle(J, R, b, dtype=np.float32, steps=2)
    for s in range(2):
        g = FS.emulate_ranks(agent, batch, R)
        assert (g.nb_total, g.nb_inner) == (R * -(-b // 32), -(-b // 32))
        _finish(agent, g)
        wp, wm, _, wl, wg = want[s]
        fp, fm, _, _, fg = f32[s]
        assert np.abs(agent._losses.cpu().numpy() - wl).max() <= 1e-5, (s, wl)
        theta, mu = agent._flat(agent._online), agent._flat(agent._mu)
        for n in wp:
            for k in range(FS.E2E_K):
                if s == 0:  # from zero moments: mu' = (1 - b1) g
                    scale = np.abs(wg[n][k]).max()
                    e, e32 = np.abs(mu[n][k] / (1 - FS.B1) - wg[n][k]).max(), np.abs(fg[n][k] - wg[n][k]).max()
                    assert e <= max(FS.GRAD_BAR * scale, 4 * e32), (n, k, e / scale, e32 / scale)
                e, e32 = np.abs(theta[n][k] - wp[n][k]).max(), np.abs(fp[n][k] - wp[n][k]).max()
                bar = FS.THETA_BAR * (s + 1)
                if e > bar:
                    print("[factored e2e] J %d %dx%d step %d %s head %d: theta %.3g on the fallback bar (float32 oracle %.3g)" % (J, R, b, s, n, k, e, e32))
                assert e <= max(bar, 4 * e32), (s, n, k, e, e32)
        assert agent._count.cpu().numpy().tolist() == [s + 1] * FS.E2E_K


def test_emulated_ranks_with_importance_weights():
    """2 x 40 (ragged) with importance weights through idqn_set_per_buffers: |TD|, losses, gradients and theta' against the oracle's
    ``weights=`` path."""
    from oracle import qnet_ref as Q

    J, R, b = 256, 2, 40
    agent, batch, p = _e2e_agent(J, R, b)
    w = np.random.default_rng(9).uniform(0.05, 1.0, R * b).astype(np.float32)
    (wp, wm, _, wl, wg), = FS.e2e_oracle(J, R, b, weights=w)
    (fp, _, _, _, fg), = FS.e2e_oracle(J, R, b, dtype=np.float32, weights=w)
    _, _, _, pt, raw = FS.e2e_inputs(J, R, b)
    g = FS.emulate_ranks(agent, batch, R, weights=w)
    _finish(agent, g)
    assert np.abs(agent._losses.cpu().numpy() - wl).max() <= 1e-5
    for k in range(FS.E2E_K):
        td = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), raw, "cnn", FS.E2E_GAMMA, weights=w)[2]["td"]
        np.testing.assert_allclose(g.td_abs[k], np.abs(td), rtol=2e-5, atol=2e-6)
    theta, mu = agent._flat(agent._online), agent._flat(agent._mu)
    for n in wp:
        for k in range(FS.E2E_K):
            scale = np.abs(wg[n][k]).max()
            assert np.abs(mu[n][k] / (1 - FS.B1) - wg[n][k]).max() <= max(FS.GRAD_BAR * scale, 4 * np.abs(fg[n][k] - wg[n][k]).max()), (n, k)
            assert np.abs(theta[n][k] - wp[n][k]).max() <= max(FS.THETA_BAR, 4 * np.abs(fp[n][k] - wp[n][k]).max()), (n, k)
