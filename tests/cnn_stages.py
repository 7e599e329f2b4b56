"""Stage-by-stage comparison of one cnn gradient step on the matrix-core conv path against the fp64 oracle.

A plain helper module like ``tests/kat_int_path.py``: ``tests/test_gpu_fp_path.py`` runs it on the golden cases,
``tests/test_gpu_conv_geometry.py`` on a table of frame geometries.  Everything here derives the layer geometry from
``oracle.qnet_ref.same_pad`` (the rules of csrc/qnet.hip: cnn_setup), so it holds for any frame the path accepts.

``stage_errors`` reads the handle's internal buffers after an ``F_GRADS_ONLY`` step: activations a1, a2, a3, Q-values of the
online and the target net, dL/dh, the data gradients da3, da2, da1 and every leaf gradient -- for every head and every
32-sample block (slot ``net * nb + block``, ragged lanes cut at B).  ``border_report`` reads the WHOLE padded buffers and
reports what lies outside the interiors (the zero borders are written once, at allocation, and never again).
"""
import numpy as np


def relerr(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


def unpack_act(buf, n_slots, slot, H, W, C, lo_h, lo_w, Hp, Wp):
    """device [slot][Hp*Wp*C][32] -> numpy [32, H, W, C]"""
    a = buf.cpu().numpy()[: n_slots * Hp * Wp * C * 32].reshape(n_slots, Hp, Wp, C, 32)[slot]
    return a[lo_h : lo_h + H, lo_w : lo_w + W].transpose(3, 0, 1, 2)


def unpack_planes(buf, n_slots, slot, H, W, C, lo_h, lo_w, Hp, Wp):
    """device [slot][Hp][Wp][3 planes][C][32] bf16 (read through a float32 view) -> numpy [32, H, W, C] = sum of planes"""
    raw = buf.cpu().numpy().view(np.uint16)[: n_slots * Hp * Wp * 3 * C * 32].reshape(n_slots, Hp, Wp, 3, C, 32)[slot]
    f = (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(axis=2).astype(np.float32)
    return f[lo_h : lo_h + H, lo_w : lo_w + W].transpose(3, 0, 1, 2)


def dgrad_pad(I, O, K, S, PL):
    mn, mx = 0, O - 1
    for i in range(I):
        for k in range(K):
            t = i + PL - k
            if t % S:
                continue
            o = t // S
            mn, mx = min(mn, o), max(mx, o)
    return -mn, mx - (O - 1)


def geometry(obs, feats):
    """Per conv layer: input / output extents and the SAME padding (same rules as csrc/qnet.hip)."""
    from oracle import qnet_ref as Q

    H, W, C = obs
    geo = []
    for (k, s), f in zip(Q.CNN_GEOM, feats[:3]):
        oh, lh, hh = Q.same_pad(H, k, s)
        ow, lw, hw = Q.same_pad(W, k, s)
        geo.append(dict(IH=H, IW=W, CI=C, OH=oh, OW=ow, CO=f, lo_h=lh, hi_h=hh, lo_w=lw, hi_w=hw, k=k, s=s))
        H, W, C = oh, ow, f
    return geo


def padded_buffers(obs, feats):
    """{buffer stem: (H, W, C, lo_h, lo_w, Hp, Wp)} of the buffers that carry a zero border: the inputs of Conv_1 / Conv_2
    (SAME padding) and the output gradients of Conv_2 / Conv_1 (the border the data-gradient loop reads)."""
    geo = geometry(obs, feats)
    out = {}
    for name, gi in (("a1", geo[1]), ("a2", geo[2])):
        out[name] = (gi["IH"], gi["IW"], gi["CI"], gi["lo_h"], gi["lo_w"], gi["IH"] + gi["lo_h"] + gi["hi_h"],
                     gi["IW"] + gi["lo_w"] + gi["hi_w"])
    for name, g in (("da3", geo[2]), ("da2", geo[1])):
        lh, hh = dgrad_pad(g["IH"], g["OH"], g["k"], g["s"], g["lo_h"])
        lw, hw = dgrad_pad(g["IW"], g["OW"], g["k"], g["s"], g["lo_w"])
        out[name] = (g["OH"], g["OW"], g["CO"], lh, lw, g["OH"] + lh + hh, g["OW"] + lw + hw)
    return out


def oracle_heads(p, pt, batch, K, gamma_hat, arch="cnn"):
    """[(loss, grads, aux)] of every head from the fp64 oracle."""
    from oracle import qnet_ref as Q

    return [Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), tuple(batch), arch, gamma_hat) for k in range(K)]


def stage_errors(agent, p, pt, batch, obs, feats, A, K, B, gamma_hat, conv_mode, oracle=None):
    """Relative error (max |got - want| / max |want|) of every stage of the step ``agent`` has just run with ``F_GRADS_ONLY``
    on ``batch``: {"h{k}_{stage}": error}.  Every 32-sample block of every net is compared.  ``oracle``: what ``oracle_heads``
    returned for these inputs (computed here if not given)."""
    if oracle is None:
        oracle = oracle_heads(p, pt, batch, K, gamma_hat)
    nb = (B + 31) // 32
    lanes = [min(32, B - 32 * bb) for bb in range(nb)]
    geo = geometry(obs, feats)
    pad = padded_buffers(obs, feats)
    planes = conv_mode == "bf16x3"
    unpack = unpack_planes if planes else unpack_act
    sfx = "p" if planes else ""
    J = feats[3]

    def blocks(fn):  # fn(bb) -> [32, ...] of sample block bb; all blocks, ragged lanes cut, as [B, ...]
        return np.concatenate([fn(bb)[: lanes[bb]] for bb in range(nb)], axis=0)

    bufs = {n: agent._debug(n) for n in ("a1" + sfx, "a2" + sfx, "a3", "da3" + sfx, "da2" + sfx, "da1" + sfx)}
    q = agent._debug("q").cpu().numpy().reshape(2 * K, nb, 32, 32)
    dh = agent._debug("dh").cpu().numpy()[: K * nb * J * 32].reshape(K, nb, J, 32)
    G = agent._flat_grad()
    errs = {}
    for k in range(K):
        loss, grads, aux = oracle[k]
        tape = aux["tape"]
        # forward activations of the online net k (slots k * nb + bb)
        for li, name in enumerate(["a1", "a2"]):
            Hh, Ww, Cc, lh, lw, Hp, Wp = pad[name]
            got = blocks(lambda bb: unpack(bufs[name + sfx], 2 * K * nb, k * nb + bb, Hh, Ww, Cc, lh, lw, Hp, Wp))
            errs[f"h{k}_{name}"] = relerr(got, tape[li][4])
        go = geo[2]
        got = blocks(lambda bb: unpack_act(bufs["a3"], 2 * K * nb, k * nb + bb, go["OH"], go["OW"], go["CO"], 0, 0,
                                           go["OH"], go["OW"]))
        errs[f"h{k}_a3"] = relerr(got, tape[2][4])
        errs[f"h{k}_q"] = relerr(blocks(lambda bb: q[k, bb, :A].T), aux["q"])
        errs[f"h{k}_qnext"] = relerr(blocks(lambda bb: q[K + k, bb, :A].T), aux["q_next"])
        # backward intermediates
        errs[f"h{k}_dh"] = relerr(blocks(lambda bb: dh[k, bb].T), aux["trace"]["d_dense0"])
        for name, key in (("da3", "d_conv2"), ("da2", "d_conv1")):
            Hh, Ww, Cc, lh, lw, Hp, Wp = pad[name]
            got = blocks(lambda bb: unpack(bufs[name + sfx], K * nb, k * nb + bb, Hh, Ww, Cc, lh, lw, Hp, Wp))
            errs[f"h{k}_{name}"] = relerr(got, aux["trace"][key])
        g0 = geo[0]
        got = blocks(lambda bb: unpack(bufs["da1" + sfx], K * nb, k * nb + bb, g0["OH"], g0["OW"], g0["CO"], 0, 0,
                                       g0["OH"], g0["OW"]))
        errs[f"h{k}_da1"] = relerr(got, aux["trace"]["d_conv0"])
        # leaf gradients
        for leaf in grads:
            errs[f"h{k}_grad_{leaf}"] = relerr(G[leaf][k], grads[leaf])
    return errs


def print_stage_errors(errs):
    print("\nstage relative errors (max |got - want| / max |want|):")
    for n_, e in errs.items():
        print(f"  {n_:32s} {e:.3e}")


def border_report(agent, obs, feats, K, B, conv_mode):
    """After a step of B samples: for each padded buffer, (largest |element| outside the interiors over every slot the step
    used and all 32 lanes, smallest over the used slots of the largest |element| inside the interior).  The first must be
    exactly 0.0, the second non-zero."""
    nb = (B + 31) // 32
    planes = conv_mode == "bf16x3"
    report = {}
    for name, (H, W, C, lh, lw, Hp, Wp) in padded_buffers(obs, feats).items():
        n_slots = (2 if name.startswith("a") else 1) * K * nb
        raw = agent._debug(name + ("p" if planes else "")).cpu().numpy()
        if planes:
            raw = raw.view(np.uint16)[: n_slots * Hp * Wp * 3 * C * 32].reshape(n_slots, Hp, Wp, 3 * C, 32)
            a = np.abs((raw.astype(np.uint32) << 16).view(np.float32))
        else:
            a = np.abs(raw[: n_slots * Hp * Wp * C * 32].reshape(n_slots, Hp, Wp, C, 32))
        assert a.shape[0] == n_slots, (name, a.shape, n_slots)
        inside = np.zeros((Hp, Wp), bool)
        inside[lh : lh + H, lw : lw + W] = True
        outside = a[:, ~inside]
        interior = a[:, inside].reshape(n_slots, -1).max(axis=1)
        report[name] = (float(outside.max()) if outside.size else 0.0, float(interior.min()))
    return report


# ---- the i-IQN heads: one step against oracle/iqn_ref.py ------------------------------------------------------------------
def iqn_record(p, pt, batch, taus, hyper):
    """What oracle/make_golden.py's capture_iqn records for one i-IQN step, computed live and over EVERY element of every leaf
    (the committed goldens keep probe indices only): losses, head 0's quantile values and greedy target actions, and per
    leaf the gradient, its largest entry per head and the parameters after the Adam step."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    K = next(iter(p.values())).shape[0]
    gamma_n = hyper["gamma"] ** hyper["n"]
    mu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
    nu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
    _, _, aux0 = I.loss_and_grads(Q.head(p, 0), Q.head(pt, 0), batch, tuple(taus[0]), gamma_n)
    p64, _, _, _, losses, grads = I.learn_on_batch(p, pt, mu, nu, np.zeros(K, np.int64), batch, taus, gamma_n, hyper["lr"],
                                                   hyper["eps"], np.float64, return_grads=True)
    rec = {"hyper": hyper, "losses": losses, "z_online_head0": aux0["z_a"], "z_target_head0": aux0["z_t"],
           "a_star_head0": aux0["a_star"], "q_select_head0": aux0["q_sel"], "leaves": {}}
    for leaf in p64:
        flat_g, flat_p = grads[leaf].reshape(K, -1), p64[leaf].reshape(K, -1)
        rec["leaves"][leaf] = {"idx": np.arange(flat_g.shape[1]), "grad": flat_g, "param": flat_p,
                               "grad_absmax": np.abs(flat_g).max(1)}
    return rec


def check_iqn_step(agent, losses, rec, A, K, B, N):
    """The comparisons of tests/test_gpu_iqn.py::test_iqn_step_against_golden, after ``agent`` has run ONE full step from a
    zero optimizer state and returned ``losses``: per-head loss within 1e-5 (relative to max(1, |loss|)), quantile values
    within 2e-5, every leaf gradient within 3e-5 of its largest entry, greedy target actions identical."""
    want = np.asarray(rec["losses"])
    assert np.abs(losses - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (losses, want)
    # quantile values of head 0, greedy target action (the library records sample block 0: the first 32 samples)
    n = min(B, 32)
    dbg = agent._debug("iqn_dbg").cpu().numpy().reshape(K, 2 * N + 33, 32)[0]
    z_on, z_tg, q_sel, a_star = dbg[:N, :n], dbg[N : 2 * N, :n], dbg[2 * N : 2 * N + A, :n].T, dbg[2 * N + 32, :n]
    assert np.array_equal(a_star.astype(np.int64), np.asarray(rec["a_star_head0"])[:n])
    for got, key in ((z_on, "z_online_head0"), (z_tg, "z_target_head0"), (q_sel, "q_select_head0")):
        w = np.asarray(rec[key])
        w = w[:n] if key == "q_select_head0" else w[:, :n]
        assert np.abs(got - w).max() <= 2e-5 * max(1.0, np.abs(w).max()), key
    # first step from zero Adam state: mu = (1 - b1) g, so every leaf's gradient is read off mu
    mu = agent._flat(agent._mu)
    par = agent._flat(agent._online)
    for leaf, r in rec["leaves"].items():
        idx = np.asarray(r["idx"])
        g = mu[leaf].reshape(K, -1)[:, idx] / (1.0 - 0.9)
        wg, scale = np.asarray(r["grad"]), np.asarray(r["grad_absmax"])[:, None]
        assert (np.abs(g - wg) <= 3e-5 * scale + 1e-12).all(), (leaf, np.abs(g - wg).max(), scale.max())
        # post-Adam parameters: one step moves a parameter by at most lr; the update direction is sign-like for tiny
        # gradients, so the bar is a fraction of lr wherever the gradient is not negligible
        wp = np.asarray(r["param"])
        big = np.abs(wg) > 1e-3 * scale
        assert (np.abs(par[leaf].reshape(K, -1)[:, idx] - wp)[big] <= 0.02 * rec["hyper"]["lr"] + 2e-7 * np.abs(wp[big])).all(), leaf
    assert (agent._count.cpu().numpy() == 1).all()
    assert np.allclose(agent.cumulated_losses, want, rtol=2e-6, atol=1e-5)
