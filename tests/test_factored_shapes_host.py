"""CPU side of the factored Dense_0 update's shape table (tests/factored_shapes.py): the table reaches every bound it names,
the layout builders are right, the float32 reference meets the bars the device is held to, the fp64 reference catches wrong
restatements of the block addressing and of the chunk loop, and the emulation of several ranks is an identity in fp64."""
import numpy as np
import pytest

import factored_shapes as FS


def test_table_reaches_every_bound():
    # the rules of launch_dense0_wgrad / dense0_wgrad_body this table is built around, restated
    assert FS.CH == 8
    assert [FS.nq(J) for J in (128, 256, 384, 512)] == [1, 2, 1, 2]
    assert [FS.n_jt(J) for J in (128, 256, 384, 512)] == [1, 1, 3, 2]
    assert FS.keep_heads(5, 7744, 512) == 5 and FS.keep_heads(6, 7744, 512) == 0   # 5 x 15.9 MB <= 84 MiB < 6 x 15.9 MB
    assert FS.KEEP_BYTES == 84 * 1024 * 1024
    assert FS.chunks(9) == [(0, 8), (8, 1)] and FS.chunks(10) == [(0, 8), (8, 2)] and FS.chunks(17) == [(0, 8), (8, 8), (16, 1)]
    assert FS.update_kernels(6, 7744, 512, 9) == [("k_dense0_wgrad_alds<1, true>", 6)]
    assert FS.update_kernels(3, 576, 512, 9) == [("k_dense0_wgrad_alds<1, false>", 3)]
    assert FS.update_kernels(3, 576, 384, 9) == [("k_dense0_wgrad<true, 1>", 3)]
    assert FS.update_kernels(3, 576, 256, 1) == [("k_dense0_wgrad<true, 2>", 3)]
    reached = {}
    for c in FS.CASES:
        assert c.nb_total % c.nb_inner == 0 and c.J % 128 == 0 and 128 <= c.J <= 512
        for b in FS.bounds(c):
            reached.setdefault(b, []).append(c)
    for b in ("one block, fused f32 update", "bo > 0 and bi > 0", "outer term alone", "inner term alone", "exactly one full chunk",
              "c0 > 0", "last chunk of one block", "ragged later chunk of several blocks", "two full chunks", "third chunk", "odd nc > 1",
              "bf3, n_jt = 1", "bf3, n_jt = 2", "non-temporal theta store", "f32 route over more than two strided blocks, n_jt = 1",
              "f32 route over more than two strided blocks, n_jt = 3", "F / 32 = 1"):
        assert reached.get(b), b
    # every row of the table on G1 at both bf16-plane widths, the f32 subset at both f32 widths
    plain = {(c.geom, c.J, c.nb_total, c.nb_inner) for c in FS.CASES if c.family == "plain"}
    assert all(("G1", J, nb, ni) in plain for J in (256, 512) for nb, ni in FS.ROWS)
    assert all(("G1", J, nb, ni) in plain for J in (128, 384) for nb, ni in FS.F32_ROWS)
    assert {("G0", 256, 9, 3), ("GA", 512, 2, 1), ("GA", 512, 9, 3)} <= plain
    # bo and bi both nonzero together with a second chunk, and the non-temporal store with a second chunk
    assert any("bo > 0 and bi > 0" in FS.bounds(c) and "c0 > 0" in FS.bounds(c) for c in FS.CASES)
    assert any("non-temporal theta store" in FS.bounds(c) and "c0 > 0" in FS.bounds(c) for c in FS.CASES)
    assert {c.family for c in FS.CASES} == {"plain", "dead", "warm"}
    assert len(set(FS.CASES)) == len(FS.CASES)


def _small(case):
    """The case with F cut to 64 rows: the layout and restatement checks do not depend on F."""
    a3, dh = FS.factors(case)
    return a3[:, :, :64], dh


@pytest.mark.parametrize("case", [c for c in FS.CASES if c.geom != "GA"], ids=FS.case_id)
def test_layout_builders(case):
    a3, dh = _small(case)
    nb, K = a3.shape[:2]
    for name, build in FS.LAYOUTS.items():
        lay = build(a3, dh, case.nb_inner)
        assert lay.name == name and lay.buf.dtype == np.float32
        assert all(s % 4 == 0 for s in lay.a3_strides + lay.dh_strides + (lay.a3_off, lay.dh_off)), (name, lay.a3_strides, lay.dh_strides)
        covered = np.zeros(lay.buf.size, bool)
        for bb in range(nb):
            for k in range(K):
                for which, src in (("a3", a3), ("dh", dh)):
                    v = FS.block_of(lay, which, bb, k)
                    assert v.base is lay.buf or v.base is lay.buf.base
                    assert v.size == src[bb, k].size and np.array_equal(v, src[bb, k].reshape(-1)), (name, which, bb, k)
                    o = FS.block_offset(lay, which, bb, k)
                    assert not covered[o : o + v.size].any(), "blocks overlap"
                    covered[o : o + v.size] = True
        assert not np.isnan(lay.buf[covered]).any()
        if name == "gapped":
            assert np.isnan(lay.buf[~covered]).all() and (~covered).sum() >= 4 * (nb + K)
            so, sh, si = lay.a3_strides
            assert si > lay.X and sh > case.nb_inner * si and so > K * sh
            assert len({si - lay.X, sh - case.nb_inner * si, so - K * sh}) == 3  # three different gaps
        else:
            assert covered.all()
    p = FS.packed(a3, dh, case.nb_inner)   # [rank][dh | a3], the strides parallel._factored_step passes
    n_a3, n_dh = K * case.nb_inner * p.X, K * case.nb_inner * p.Y
    assert (p.a3_off, p.dh_off) == (n_dh, 0)
    assert p.a3_strides == (n_a3 + n_dh, case.nb_inner * p.X, p.X) and p.dh_strides == (n_a3 + n_dh, case.nb_inner * p.Y, p.Y)


@pytest.mark.parametrize("case", FS.CASES, ids=FS.case_id)
def test_float32_reference_meets_the_bars(case):
    """Block-ordered float32 accumulation stays inside the primary bars on every row and every element: the device test
    therefore excludes nothing, and its fallback bar (4 x these figures) is never the looser one by accident of the inputs."""
    ref = FS.reference(case)
    for q in ("grad", "theta", "nu"):
        assert (ref["f32"][q] <= ref["primary"][q]).all(), (q, ref["f32"][q], ref["primary"][q])
    G = ref["want"][3]
    assert (np.abs(G).max(axis=(1, 2)) > 0).all()
    if case.family == "warm":
        _, mu, nu, count = FS.state(case)
        assert (count == FS.WARM_COUNT).all() and np.abs(mu).max() > 0 and nu.min() > 0


def _through_layout(lay, nb_total, K, F, J, blocks=None, exchange=()):
    """fp64 G from the blocks as the address rule finds them in the buffer; ``exchange``: the factors whose outer and inner
    strides the restatement swaps.  (Swapping them for BOTH factors on a square block grid only permutes the blocks of a sum:
    the three addressing sites of the kernels can go wrong one by one, and so do these restatements.)"""
    blocks = range(nb_total) if blocks is None else blocks
    a3 = np.stack([np.stack([FS.block_of(lay, "a3", bb, k, "a3" in exchange).reshape(F, 32) for k in range(K)]) for bb in blocks])
    dh = np.stack([np.stack([FS.block_of(lay, "dh", bb, k, "dh" in exchange).reshape(J, 32) for k in range(K)]) for bb in blocks])
    return FS.gradient(a3, dh)


def _misses(G_wrong, G):
    """True for every head: the wrong gradient lies outside the gradient bar somewhere (NaN counts as outside)."""
    return [not (np.abs(G_wrong[k] - G[k]).max() <= FS.GRAD_BAR * np.abs(G[k]).max()) for k in range(G.shape[0])]


@pytest.mark.parametrize("case", [c for c in FS.CASES if c.geom == "G1" and c.J == 256], ids=FS.case_id)
def test_reference_catches_wrong_restatements(case):
    a3, dh = _small(case)
    nb, K, F = a3.shape[:3]
    J = dh.shape[2]
    G = FS.gradient(a3, dh)
    for build in FS.LAYOUTS.values():  # right restatement: exact
        assert np.array_equal(_through_layout(build(a3, dh, case.nb_inner), nb, K, F, J), G)
    n_outer = nb // case.nb_inner
    if "bo > 0 and bi > 0" in FS.bounds(case) and n_outer == case.nb_inner:  # (square: the exchanged rule stays inside the buffer)
        for name in ("packed", "split"):
            lay = FS.LAYOUTS[name](a3, dh, case.nb_inner)
            for which in (("a3",), ("dh",)):
                assert all(_misses(_through_layout(lay, nb, K, F, J, exchange=which), G)), (name, which)
            assert not any(_misses(_through_layout(lay, nb, K, F, J, exchange=("a3", "dh")), G))  # only a permutation of the sum
    if nb >= 2:
        for drop in {0, nb - 1, nb // 2}:
            assert all(_misses(FS.gradient(a3, dh, blocks=[b for b in range(nb) if b != drop]), G)), drop
    if nb > FS.CH:  # the second chunk started one block early: block 7 twice (and, equally wrong, block 8 twice)
        assert all(_misses(FS.gradient(a3, dh, blocks=list(range(8)) + list(range(7, nb))), G))
        assert all(_misses(FS.gradient(a3, dh, blocks=list(range(9)) + list(range(8, nb))), G))
        assert all(_misses(FS.gradient(a3, dh, blocks=list(range(8)) + list(range(7, nb - 1))), G))  # c0 - 1 with the same count
    if case.family == "dead":
        live = dh.copy()
        rng = np.random.default_rng(3)
        for bb in range(nb):
            if bb % case.nb_inner == case.nb_inner - 1:
                assert not live[bb, :, :, FS.LIVE_IN_DEAD_BLOCK:].any() and (a3[bb, :, :, FS.LIVE_IN_DEAD_BLOCK:] > 0).all()
                live[bb, :, :, FS.LIVE_IN_DEAD_BLOCK:] = 1e-3 * rng.standard_normal(live[bb, :, :, FS.LIVE_IN_DEAD_BLOCK:].shape)
        assert all(_misses(FS.gradient(a3, live), G))


@pytest.mark.parametrize("R,b", [(3, 32), (2, 40)])
def test_emulation_identity_in_fp64(R, b):
    """Sum over the shards of the per-shard loss and gradients taken with the GLOBAL batch as mean divisor == the loss and
    gradients of the global batch, to 1e-12 relative."""
    from oracle import qnet_ref as Q

    obs, feats, p, pt, batch = FS.e2e_inputs(128, R, b)
    B = R * b
    for k in range(FS.E2E_K):
        want_loss, want, _ = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", FS.E2E_GAMMA)
        loss, total = 0.0, None
        for r in range(R):
            shard = tuple(f[b * r : b * (r + 1)] for f in batch)
            l, g, _ = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), shard, "cnn", FS.E2E_GAMMA)  # mean over b ...
            loss += l * b / B                                                                       # ... -> divisor B
            total = {n: v * b / B for n, v in g.items()} if total is None else {n: total[n] + v * b / B for n, v in g.items()}
        assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
        for n in want:
            assert np.abs(total[n] - want[n]).max() <= 1e-12 * np.abs(want[n]).max(), (k, n)


@pytest.mark.parametrize("J", [256, 128])
@pytest.mark.parametrize("R,b", FS.E2E_SHARDS)
def test_float32_oracle_meets_the_end_to_end_bars(J, R, b):
    """The inputs of the end-to-end rows are such that the float32 run of the oracle meets every bar on every element of
    every leaf, first and second step: the device test leaves nothing out."""
    want = FS.e2e_oracle(J, R, b, steps=2)
    got = FS.e2e_oracle(J, R, b, dtype=np.float32, steps=2)
    for s in range(2):
        wp, wm, _, wl, wg = want[s]
        gp, gm, _, gl, gg = got[s]
        assert np.abs(gl - wl).max() <= 1e-5
        for n in wp:
            for k in range(FS.E2E_K):
                if s == 0:
                    assert np.abs(gg[n][k] - wg[n][k]).max() <= FS.GRAD_BAR * np.abs(wg[n][k]).max(), (n, k)
                assert np.abs(gp[n][k] - wp[n][k]).max() <= FS.THETA_BAR * (s + 1), (s, n, k, np.abs(gp[n][k] - wp[n][k]).max())
