"""CPU (no GPU): the impala architecture's layout, descriptor and shape table (tests/impala_shapes.py).

The layout query names flax's leaves in creation order on 256-byte boundaries, meaningless shapes are refused, ``ImpalaNet``
draws each leaf from the reference's initialiser family, the parameter tree nests as flax nests submodules -- and the table
itself is worth running: both pad classes of the pool on both axes, an extent of 1, a non-zero oracle gradient on every
leaf of every row, float32 autograd within the device bars, a tie row that tells the pool's two tie rules apart.
"""
import numpy as np
import pytest

import impala_shapes as S

NAMES = list(S.ROWS)


@pytest.mark.parametrize("name", NAMES)
def test_layout_matches_the_flax_pytree(name):
    from oracle import qnet_ref as Q
    from slimdqn import _hip

    obs, feats, A, K, B = S.ROWS[name]
    leaves, stride = _hip.layout(_hip.make_config("impala", K, A, obs, feats, max(B, 32), 1e-3, 1e-8, 0.99))
    assert [(n, tuple(s)) for n, _, s in leaves] == [(n, tuple(s)) for n, s in Q.leaf_shapes("impala", obs, A, feats)]
    assert stride % 64 == 0 and all(off % 64 == 0 for _, off, _ in leaves)
    ends = [off + int(np.prod(s)) for _, off, s in leaves]
    assert all(e <= nxt for e, nxt in zip(ends, [off for _, off, _ in leaves][1:] + [stride]))


def test_meaningless_shapes_are_refused():
    from slimdqn import _hip

    cfg = lambda obs, feats, **kw: _hip.make_config("impala", 2, 4, obs, feats, 32, 1e-3, 1e-8, 0.99, **kw)  # noqa: E731
    _hip.layout(cfg((84, 84, 4), [32, 64, 64, 512]))
    _hip.layout(cfg((84, 84, 4), [1, 1, 1, 2, 3, 4, 5, 6]))  # the most leaves a config can ask for
    for obs, feats, kw in (((84, 84, 4), [32, 64], {}), ((84, 84, 4), [32, 0, 64, 512], {}), ((84, 84, 4), [32, 64, 64, -1], {}),
                           ((0, 84, 4), [32, 64, 64], {}), ((84, 84, 0), [32, 64, 64], {}), ((84, 84, 4), [32, 64, 64, 512], {"n_quantiles": 8})):
        with pytest.raises(_hip.HipExtensionError):
            _hip.layout(cfg(obs, feats, **kw))


def test_dqnnet_still_refuses_and_points_at_the_new_class():
    from slimdqn.networks.architectures.dqn import DQNNet

    with pytest.raises(NotImplementedError, match="ImpalaNet"):
        DQNNet([32, 64, 64, 512], "impala", 6)


def test_init_leaf_families():
    from oracle import qnet_ref as Q
    from slimdqn.networks.architectures.impala import ImpalaNet

    net = ImpalaNet([32, 64, 64, 512], 6)
    assert (net.features, net.n_actions, net.architecture_type) == ([32, 64, 64, 512], 6, "impala")
    rng = np.random.default_rng(0)
    for name, shape in Q.leaf_shapes("impala", (21, 21, 4), 6, [32, 64, 64, 512]):
        v = net.init_leaf(rng, name, shape, 3)
        assert v.shape == (3,) + tuple(shape) and v.dtype == np.float32
        if name.endswith("bias"):
            assert not v.any()
            continue
        rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
        fan_in, fan_out = rf * shape[-2], rf * shape[-1]
        if "/Conv_0/" in name or name.startswith("Dense_"):  # xavier_uniform: inside the bound, filling it, variance lim^2 / 3
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            assert np.abs(v).max() <= lim and np.abs(v).max() >= 0.9 * lim, name
            assert abs(v.std() / (lim / np.sqrt(3.0)) - 1) < 0.1, name
        else:  # lecun_normal: standard deviation sqrt(1 / fan_in), truncated at 2 sigma of the untruncated normal
            sig = np.sqrt(1.0 / fan_in) / 0.87962566103423978
            assert np.abs(v).max() <= 2 * sig * (1 + 1e-6) and np.abs(v).max() >= 1.8 * sig, name
            assert abs(v.std() / np.sqrt(1.0 / fan_in) - 1) < 0.05, name
    with pytest.raises(ValueError):
        ImpalaNet([32, 64], 6)


def test_nested_tree_has_flax_structure():
    """DeviceAgent._tree on an object that carries only what it reads (no device)."""
    import torch

    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent, _obs_triplet

    assert _obs_triplet((84, 84, 4), "impala") == (84, 84, 4)
    leaves, P = _hip.layout(_hip.make_config("impala", 2, 4, (8, 8, 1), [2, 3, 4, 5], 32, 1e-3, 1e-8, 0.99))
    for stacked in (True, False):
        a = object.__new__(DeviceAgent)
        a._leaves, a._K, a._stacked = leaves, 2, stacked
        arena = torch.arange(2 * P, dtype=torch.float32).reshape(2, P)
        for tree in (a._tree(arena)["params"], a._numpy_tree(arena)["params"]):
            assert list(tree) == ["Stack_0", "Stack_1", "Stack_2", "Dense_0", "Dense_1"]
            assert list(tree["Stack_1"]) == [f"Conv_{i}" for i in range(5)] and list(tree["Stack_1"]["Conv_3"]) == ["kernel", "bias"]
            assert tuple(tree["Stack_1"]["Conv_0"]["kernel"].shape) == ((2,) if stacked else ()) + (3, 3, 2, 3)
            assert tuple(tree["Dense_1"]["bias"].shape) == ((2,) if stacked else ()) + (4,)
            off = dict((n, o) for n, o, _ in leaves)["Stack_2/Conv_4/bias"]
            assert float(np.asarray(tree["Stack_2"]["Conv_4"]["bias"]).reshape(-1)[0]) == float(off)


def test_table_covers_the_pool_pad_classes():
    from oracle.qnet_ref import same_pad

    seen = {0: set(), 1: set()}
    ones = False
    for obs, *_ in S.ROWS.values():
        for axis in (0, 1):
            e = obs[axis]
            for _ in range(3):
                out, lo, hi = same_pad(e, 3, 2)
                seen[axis].add((lo, hi))
                e = out
                ones = ones or e == 1
    assert seen[0] >= {(0, 1), (1, 1)} and seen[1] >= {(0, 1), (1, 1)} and ones


@pytest.mark.parametrize("name", NAMES)
def test_every_leaf_has_a_gradient_and_float32_meets_the_bars(name):
    obs, feats, A, K, B, p, pt, batch = S.case(name)
    for k, (want, (loss_err, leaf_err)) in enumerate(zip(S.oracle(name), S.f32_errors(name))):
        assert set(want["grads"]) == set(p)
        for leaf, g in want["grads"].items():
            assert np.abs(g).max() > 0, (name, k, leaf)
        print(name, k, "f32 loss error", loss_err, "worst leaf", max(leaf_err.values()))
        assert loss_err <= 1e-5 * max(1.0, abs(want["loss"]))
        assert max(leaf_err.values()) <= 2e-5, (name, k, max(leaf_err, key=leaf_err.get))


def test_tie_row_tells_the_tie_rules_apart():
    want = S.oracle("tie")[0]["grads"]["Stack_0/Conv_0/kernel"]
    last = S.last_max_pool_conv0_grad("tie", 0)
    assert np.abs(want).max() > 0.01
    assert np.abs(last - want).max() > 1e-3 * np.abs(want).max()
    # the same replacement on a head without ties changes nothing: the model differs from the oracle in the tie rule only
    assert np.abs(S.last_max_pool_conv0_grad("tie", 1) - S.oracle("tie")[1]["grads"]["Stack_0/Conv_0/kernel"]).max() <= 1e-12
