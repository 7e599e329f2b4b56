"""GPU: ``per_turn`` -- the write-back of one prioritized step and the draw of the next as one launch (``k_per_turn``).

Every comparison is ``tobytes()`` equality against ``per_write_back`` followed by ``per_draw`` on a twin tree built from the same
bytes: the node array, the running maximum, the priorities, the next leaves (clamped) and the next weights.  On the parent commit
the entry does not exist.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 4, 5, 16, 17, 32, 33, 256]  # 16, 17: a full round of the 16 waves, and one descent into the second round
EPS, ALPHA, BETA = 1e-3, 0.6, 0.4


def _depth(capacity):
    return int(np.ceil(np.log2(capacity))) + 1


def _nodes(values):
    """Node array (host, float64) of the tree whose leaves are ``values`` (a power of two of them)."""
    from oracle.sumtree_ref import SumTreeRef

    ref = SumTreeRef(len(values))
    ref.set(np.arange(len(values), dtype=np.int32), np.asarray(values, np.float64))
    return np.ascontiguousarray(ref.nodes, np.float64)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(nodes_h, depth, leaves_h, td_h, u_h, n_items, stratified=1, reduce_max=0, with_out=True, with_max=True, eps=EPS):
    """``per_turn`` on one copy of the tree, ``per_write_back`` then ``per_draw`` on a twin; asserts the bytes and returns the
    turn's host results ``(nodes, next leaves, next weights, priorities, maximum)``."""
    import torch

    from slimdqn import _hip

    lib, q = _hip.lib(), _hip.current_stream()
    K, n = td_h.shape
    leaves, td, u = _dev(leaves_h.astype(np.int32)), _dev(td_h.astype(np.float32)), _dev(u_h.astype(np.float64))
    out = []
    for turn in (False, True):
        nodes = _dev(nodes_h)
        mx = torch.full((1,), 1.0, dtype=torch.float64, device="cuda")
        pr = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        nl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        nw = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        scratch = torch.empty(8192, dtype=torch.float64, device="cuda")
        p_pr, p_mx = _hip.ptr(pr) if with_out else None, _hip.ptr(mx) if with_max else None
        if turn:
            _hip.check(lib.per_turn(_hip.ptr(nodes), depth, _hip.ptr(leaves), _hip.ptr(td), K, n, reduce_max, eps, ALPHA, p_pr, p_mx,
                                    _hip.ptr(scratch), _hip.ptr(u), stratified, n_items, BETA, _hip.ptr(nl), _hip.ptr(nw), q), "per_turn")
        else:
            _hip.check(lib.per_write_back(_hip.ptr(nodes), depth, _hip.ptr(leaves), _hip.ptr(td), K, n, reduce_max, eps, ALPHA, p_pr, p_mx,
                                          _hip.ptr(scratch), q), "per_write_back")
            _hip.check(lib.per_draw(_hip.ptr(nodes), depth, _hip.ptr(u), n, stratified, n_items, BETA, _hip.ptr(nl), _hip.ptr(nw), q),
                       "per_draw")
        torch.cuda.synchronize()
        out.append(tuple(t.cpu().numpy() for t in (nodes, nl, nw, pr, mx)))
    tag = (depth, n, stratified, reduce_max, with_out, with_max)
    for name, a, b in zip(("nodes", "next leaves", "next weights", "priorities", "maximum"), *out):
        assert a.tobytes() == b.tobytes(), (tag, name)
    nodes, nl, nw, pr, mx = out[1]
    assert nodes.tobytes() != nodes_h.tobytes(), tag  # the write-back changed the tree
    assert ((0 <= nl) & (nl < n_items)).all() and np.isfinite(nw).all() and nw.max() == 1.0, tag
    assert (pr == -1.0).all() if not with_out else (pr > 0).all(), tag
    assert mx[0] == (max(1.0, pr.max()) if with_max and with_out else mx[0]) and (with_max or mx[0] == 1.0), tag
    return out[1]


@pytest.mark.parametrize("capacity", [8, 64])
def test_per_turn_equals_write_back_then_draw(capacity):
    from slimdqn import _hip

    lib, q, depth = _hip.lib(), _hip.current_stream(), _depth(capacity)
    rng = np.random.default_rng(capacity)
    # live leaves hold little, the leaves at and past n_items most of the mass: descents land there and the clamp pulls them back
    n_items = capacity // 2 + 1
    values = rng.random(capacity) + 0.05
    values[:n_items] *= 1e-2
    values[rng.integers(n_items)] = 0.0
    nodes_h = _nodes(values)
    clamped, case = False, 0
    for n in NS:
        for stratified in (1, 0):
            for reduce_max in (0, 1):
                for with_out, with_max in ((True, True), (False, False)) if case % 2 else ((False, True), (True, False)):
                    case += 1
                    K = (1, 3, 5)[case % 3]
                    leaves_h = rng.integers(0, n_items, n)
                    td_h = (rng.random((K, n)) * 3.0).astype(np.float32)
                    td_h[:, rng.integers(n)] = 0.0
                    u_h = rng.random(n)
                    u_h[rng.integers(n)], u_h[rng.integers(n)] = 0.0, np.nextafter(1.0, 0.0)
                    nodes, nl, _, _, _ = _run(nodes_h, depth, leaves_h, td_h, u_h, n_items, stratified, reduce_max, with_out, with_max)
                    # the unclamped leaves of the same draw on the tree the turn left
                    raw = _dev(np.zeros(n, np.int32))
                    _hip.check(lib.per_sample_leaves(_hip.ptr(_dev(nodes)), depth, _hip.ptr(_dev(u_h)), n, stratified, _hip.ptr(raw), q),
                               "per_sample_leaves")
                    clamped |= bool((raw.cpu().numpy() != nl).any())
    assert clamped, "no draw landed at or past the item count: the clamp was not reached"


@pytest.mark.parametrize("n", [4, 32, 256])
def test_duplicate_leaves_first_occurrence_wins(n):
    capacity, depth = 64, _depth(64)
    rng = np.random.default_rng(n)
    nodes_h = _nodes(rng.random(capacity) + 0.05)
    first_leaf = capacity - 1
    pairs = rng.permutation(capacity)[: n // 2] if n // 2 <= capacity else rng.integers(0, capacity, n // 2)
    for name, leaves_h in (("all equal", np.full(n, 17)), ("pairs", rng.permutation(np.concatenate([pairs, pairs])))):
        td_h = (rng.random((3, n)) * 3.0 + 0.1).astype(np.float32)
        nodes, _, _, pr, _ = _run(nodes_h, depth, leaves_h, td_h, rng.random(n), capacity)
        for leaf in np.unique(leaves_h):
            first = int(np.flatnonzero(leaves_h == leaf)[0])
            # (the set adds new - old to the leaf, so the leaf is the priority up to rounding; the occurrences' priorities differ widely)
            assert np.isclose(nodes[first_leaf + leaf], pr[first], rtol=1e-9, atol=0.0), (name, n, leaf)
        assert len(np.unique(pr)) > n // 2  # (the occurrences had priorities of their own to win with)


@pytest.mark.parametrize("n", [4, 256])
def test_the_draw_reads_the_tree_the_write_back_left(n):
    """Visibility: the write-back raises one leaf of an 8-leaf tree from about nothing to almost the whole mass, so every next
    target lands on it -- a stale read of any node on its path gives another leaf.  n = 256: every wave descends, 16 times."""
    depth, hot = _depth(8), 5
    nodes_h = _nodes(np.full(8, 1e-9))
    td_h = np.full((2, n), 1e6, np.float32)
    u_h = np.random.default_rng(n).random(n) * 0.98 + 0.01
    for stratified in (0, 1):
        nodes, nl, nw, _, mx = _run(nodes_h, depth, np.full(n, hot), td_h, u_h, 8, stratified=stratified)
        assert (nl == hot).all(), (n, stratified, nl)
        assert (nw == 1.0).all() and nodes[0] > 1e3 and np.isclose(mx[0], nodes[7 + hot], rtol=1e-9, atol=0.0)


def test_the_mass_moves_away_from_the_leaves_written_back():
    """The write-back sets the sampled leaves to eps^alpha: the next draw lands on the others."""
    capacity, depth, n = 64, _depth(64), 32
    rng = np.random.default_rng(5)
    nodes_h = _nodes(rng.random(capacity) + 0.5)
    written = rng.permutation(capacity)[:n]
    u_h = rng.random(n) * 0.98 + 0.01
    for stratified in (0, 1):
        nodes, nl, _, pr, _ = _run(nodes_h, depth, written, np.zeros((3, n), np.float32), u_h, capacity, stratified=stratified, eps=1e-12)
        assert np.allclose(pr, 1e-12 ** ALPHA, rtol=1e-9, atol=0.0) and not np.isin(nl, written).any(), (stratified, nl)


def test_refusals():
    import torch

    from slimdqn import _hip

    lib, q = _hip.lib(), _hip.current_stream()
    nodes = _dev(_nodes(np.ones(8)))
    before = nodes.clone()
    i32, f32, f64 = (torch.zeros(512, dtype=d, device="cuda") for d in (torch.int32, torch.float32, torch.float64))
    ok = dict(nodes=_hip.ptr(nodes), depth=4, leaves=_hip.ptr(i32), td=_hip.ptr(f32), K=2, n=4, scratch=_hip.ptr(f64.clone()),
              u=_hip.ptr(f64), n_items=8, nl=_hip.ptr(i32.clone()), nw=_hip.ptr(f32.clone()))
    for change, match in ((dict(n=0), "n not in"), (dict(n=257), "n not in"), (dict(depth=0), "depth"), (dict(depth=32), "depth"),
                          (dict(K=0), "n_heads"), (dict(n_items=0), "n_items"), (dict(nodes=None), "null pointer"),
                          (dict(u=None), "null pointer"), (dict(nl=None), "null pointer"), (dict(scratch=None), "null pointer")):
        a = dict(ok, **change)
        rc = lib.per_turn(a["nodes"], a["depth"], a["leaves"], a["td"], a["K"], a["n"], 0, EPS, ALPHA, None, None, a["scratch"], a["u"], 1,
                          a["n_items"], BETA, a["nl"], a["nw"], q)
        msg = lib.idqn_last_error().decode()
        assert rc == _hip.E_INVALID and msg.startswith("per_turn:") and match in msg, (change, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(nodes, before)
