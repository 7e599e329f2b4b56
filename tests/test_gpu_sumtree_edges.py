"""GPU: the sum-tree and prioritized-replay kernels against the reference's captured bytes and against fp64 numpy models, at
every edge of their plans (the table, the input scripts and the models: tests/sumtree_edges.py; what the table is held to:
tests/test_sumtree_edges_host.py).  Everything goes through the C ABI.

``sumtree_set`` rows: node bytes == the digest the reference's own ``sum_tree.py`` left (tests/golden/int_path_sumtree_edges.npz),
root, and ``sumtree_query`` on the result == the reference's ``query``.

Prioritized rows: the separate launches (``per_sample_leaves`` + ``per_importance_weights``, ``per_priorities_from_td`` +
``sumtree_set``) AND the fused entries (``per_draw``, ``per_write_back``, ``per_turn``) run on twin trees, and EACH side is compared
with the model, not only with the other side:

* leaves, raw and clamped: exact;
* priorities: rtol 1e-12 (the bound tests/test_gpu_per_extension.py uses for the same ``pow``), exactly 1.0 where alpha = 0;
* running maximum: the bits of max(start, max(device priorities)); untouched where ``max_dev`` is NULL;
* tree after a write-back: the bytes of ``SumTreeRef.set(leaves, device priorities)`` on the same start tree (feeding the oracle
  the device's own priorities separates the set from ``pow``);
* weights: relative difference to the fp64 model <= 2^-23, one float32 ulp (an fp64 quotient rounded once to float32 is half an
  ulp off, 2^-24; the fp64 ``pow`` error is eight orders smaller; the factor 2 is the margin); the batch maximum exactly 1.0f, a
  zero-priority leaf exactly 0.0f, beta = 0 exactly 1.0f on every positive leaf, an empty tree leaves 0 and weights 1.0f;
* ``per_turn``: its next draw against the model's draw on the model's tree after the write-back -- the first independent check of
  the read-after-write inside that kernel.

Largest differences observed on an MI355X over the whole table: priorities 2.21e-16 relative (one fp64 ulp), weights 5.81e-8
relative (just under 2^-24 = 5.96e-8, the rounding to float32).
"""
import hashlib
import os

import numpy as np
import pytest

import sumtree_edges as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "int_path_sumtree_edges.npz")
PRI_RTOL = 1e-12
W_RTOL = 2.0 ** -23
OBSERVED = {"priority": 0.0, "weight": 0.0}  # largest relative differences seen so far (printed by every test: run with -s)


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # (the shared start trees are read-only arrays)


def _same_bits(a, b):
    import torch

    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def _first_difference(got, want):
    g, w = got.view(np.uint64), want.view(np.uint64)
    at = int(np.flatnonzero(g != w)[0])
    return f"first differing node {at} of {len(got)}: device {got[at]!r}, expected {want[at]!r} ({int((g != w).sum())} nodes differ)"


# ---------------------------------------------------------------------------------------------------------------
# sumtree_set
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", range(1, 22))
def test_sumtree_set_leaves_the_bytes_of_the_reference(depth):
    import torch

    from slimdqn import _hip

    lib, q = _hip.lib(), _hip.current_stream()
    z = np.load(GOLDEN)
    scratch = torch.empty(2 * E.ST_MAX_N, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows = [(i, r) for i, r in enumerate(E.SET_ROWS) if E.depth_of(r.capacity) == depth]
    assert rows
    start, start_cap = None, None
    for i, row in rows:
        assert tuple(z["rows"][i]) == (row.capacity, row.n, E.LEAF_KINDS.index(row.kind), row.salt)
        if start_cap != row.capacity:
            start, start_cap = _dev(E.set_start_nodes(row.capacity)), row.capacity  # one upload per capacity
        idx, val = E.set_row_inputs(row)
        nodes, idx_dev, val_dev = start.clone(), _dev(idx), _dev(val.astype(np.float64))  # (named: alive until the launch has run)
        _hip.check(lib.sumtree_set(_hip.ptr(nodes), depth, _hip.ptr(idx_dev), _hip.ptr(val_dev), row.n, _hip.ptr(scratch), q),
                   "sumtree_set")
        got = nodes.cpu().numpy()
        if hashlib.sha256(got.tobytes()).digest() != z["digests"][i].tobytes():
            pytest.fail(f"{row}: " + _first_difference(got, E.model_set_row(row).nodes))
        assert got[0] == z["roots"][i], row
        targets = E.query_targets(row, float(got[0]))
        if targets.size:
            out, targets_dev = torch.full((E.N_QUERY,), -7, dtype=torch.int32, device="cuda"), _dev(targets)
            _hip.check(lib.sumtree_query(_hip.ptr(nodes), depth, _hip.ptr(targets_dev), E.N_QUERY, _hip.ptr(out), _hip.ptr(status), q),
                       "sumtree_query")
            np.testing.assert_array_equal(out.cpu().numpy(), z["q_out"][i], err_msg=str(row))
    assert int(status.item()) == 0


def test_sumtree_set_refuses_4097_and_leaves_the_tree():
    import torch

    from slimdqn import _hip

    lib, q = _hip.lib(), _hip.current_stream()
    cap, n = 4096, E.ST_MAX_N + 1
    start = _dev(E.set_start_nodes(cap))
    nodes = start.clone()
    idx = _dev(np.arange(n, dtype=np.int32) % cap)
    val = _dev(np.full(n, 7.0))
    scratch = torch.empty(2 * E.ST_MAX_N + 64, dtype=torch.float64, device="cuda")
    rc = lib.sumtree_set(_hip.ptr(nodes), E.depth_of(cap), _hip.ptr(idx), _hip.ptr(val), n, _hip.ptr(scratch), q)
    torch.cuda.synchronize()
    assert rc == _hip.E_INVALID and "sumtree_set" in lib.idqn_last_error().decode()
    assert _same_bits(nodes, start)


# ---------------------------------------------------------------------------------------------------------------
# prioritized rows
# ---------------------------------------------------------------------------------------------------------------
def _check_leaves(tag, got, want):
    np.testing.assert_array_equal(got, want.astype(np.int32), err_msg=str(tag))


def _check_weights(tag, got, want):
    """``got``: the device's float32 weights; ``want``: the fp64 model's."""
    assert got.dtype == np.float32 and np.isfinite(got).all(), tag
    diff = np.abs(got.astype(np.float64) - want)
    pos = want > 0.0
    if pos.any():
        OBSERVED["weight"] = max(OBSERVED["weight"], float((diff[pos] / want[pos]).max()))
    assert (diff <= W_RTOL * want).all(), (tag, float((diff[pos] / want[pos]).max()) if pos.any() else None)
    assert (got[want == 0.0] == 0.0).all(), tag  # zero-priority leaves
    assert (got[want == 1.0] == 1.0).all() and got.max() == np.float32(1.0), tag  # the batch maximum; beta = 0; the empty tree


def _check_priorities(tag, got, want, alpha):
    rel = np.abs(got - want) / np.where(want > 0.0, want, 1.0)
    OBSERVED["priority"] = max(OBSERVED["priority"], float(rel.max()))
    np.testing.assert_allclose(got, want, rtol=PRI_RTOL, atol=0.0, err_msg=str(tag))
    if alpha == 0.0:
        assert (got == 1.0).all(), tag


class _Side:
    """The buffers of one side (separate launches, or a fused entry) of a prioritized row on its own copy of the tree."""

    def __init__(self, start, n, max_start):
        import torch

        self.nodes = start.clone()
        self.pri = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        self.mx = torch.full((1,), max_start, dtype=torch.float64, device="cuda")
        self.leaves = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.raw = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.w = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        self.scratch = torch.empty(2 * E.ST_MAX_N, dtype=torch.float64, device="cuda")


def _chain_draw(lib, q, H, nodes, depth, u, row, side):
    n = row.n
    H.check(lib.per_sample_leaves(H.ptr(nodes), depth, H.ptr(u), n, row.stratified, H.ptr(side.raw), q), "per_sample_leaves")
    side.leaves.copy_(side.raw)
    H.check(lib.per_importance_weights(H.ptr(nodes), depth, H.ptr(side.leaves), n, row.n_items, row.beta, H.ptr(side.w), q),
            "per_importance_weights")
    return side.raw.cpu().numpy(), side.leaves.cpu().numpy(), side.w.cpu().numpy()


def _fused_draw(lib, q, H, nodes, depth, u, row, side):
    H.check(lib.per_draw(H.ptr(nodes), depth, H.ptr(u), row.n, row.stratified, row.n_items, row.beta, H.ptr(side.leaves), H.ptr(side.w), q),
            "per_draw")
    return side.leaves.cpu().numpy(), side.w.cpu().numpy()


def _run_per_row(row, start):
    import torch

    from slimdqn import _hip as H

    lib, q = H.lib(), H.current_stream()
    n, depth = row.n, E.depth_of(row.capacity)
    nodes_h, inp = E.per_tree(row.capacity, row.tree), E.per_row_inputs(row)
    u, u2, wb, td = _dev(inp["u"]), _dev(inp["u2"]), _dev(inp["leaves"]), _dev(inp["td"])
    chain, fused, turn = (_Side(start, n, inp["max_start"]) for _ in range(3))

    # ---- the draw on the start tree: separate launches, per_draw
    raw_m, leaves_m = E.model_draw(nodes_h, inp["u"], row.stratified, row.n_items)
    w_m = E.model_weights(nodes_h, leaves_m, row.n_items, row.beta)
    raw, leaves, w = _chain_draw(lib, q, H, start, depth, u, row, chain)
    _check_leaves((row, "chain raw leaves"), raw, raw_m)
    _check_leaves((row, "chain clamped leaves"), leaves, leaves_m)
    _check_weights((row, "chain weights"), w, w_m)
    leaves, w = _fused_draw(lib, q, H, start, depth, u, row, fused)
    _check_leaves((row, "per_draw leaves"), leaves, leaves_m)
    _check_weights((row, "per_draw weights"), w, w_m)
    if nodes_h[0] == 0.0:
        assert (leaves == 0).all() and (w == 1.0).all(), row  # the empty tree

    # ---- the write-back: separate launches, per_write_back, per_turn (which also draws with u2)
    p_mx = [H.ptr(s.mx) if row.with_max else None for s in (chain, fused, turn)]
    p_pr = [H.ptr(s.pri) if row.with_out else None for s in (fused, turn)]
    wbargs = (row.K, n, row.reduce_max, row.eps, row.alpha)
    H.check(lib.per_priorities_from_td(H.ptr(td), row.K, n, row.reduce_max, row.eps, row.alpha, H.ptr(chain.pri), p_mx[0], q), "pri")
    H.check(lib.sumtree_set(H.ptr(chain.nodes), depth, H.ptr(wb), H.ptr(chain.pri), n, H.ptr(chain.scratch), q), "sumtree_set")
    H.check(lib.per_write_back(H.ptr(fused.nodes), depth, H.ptr(wb), H.ptr(td), *wbargs, p_pr[0], p_mx[1], H.ptr(fused.scratch), q),
            "per_write_back")
    H.check(lib.per_turn(H.ptr(turn.nodes), depth, H.ptr(wb), H.ptr(td), *wbargs, p_pr[1], p_mx[2], H.ptr(turn.scratch), H.ptr(u2),
                         row.stratified, row.n_items, row.beta, H.ptr(turn.leaves), H.ptr(turn.w), q), "per_turn")
    pri_m = E.model_priorities(inp["td"], row.reduce_max, row.eps, row.alpha)
    chain_pri = chain.pri.cpu().numpy()
    expected = {}  # priorities' bytes -> (the oracle's tree after the set, the same on the device)
    for name, side in (("chain", chain), ("per_write_back", fused), ("per_turn", turn)):
        pri = side.pri.cpu().numpy()
        if side is chain or row.with_out:
            _check_priorities((row, name, "priorities"), pri, pri_m, row.alpha)
        else:
            assert (pri == -1.0).all(), (row, name)
            pri = chain_pri  # (not handed out: the tree below shows whether this side computed the same ones)
        mx = side.mx.cpu().numpy()
        want_mx = np.float64(max(inp["max_start"], pri.max()) if row.with_max else inp["max_start"])
        assert mx.tobytes() == np.asarray([want_mx]).tobytes(), (row, name, "running maximum", mx, want_mx)
        key = pri.tobytes()
        if key not in expected:
            post_h, _ = E.model_write_back(row.capacity, nodes_h, inp["leaves"], pri, inp["max_start"])
            at = E.touched_nodes(nodes_h, inp["leaves"])
            post = start.clone()
            post[_dev(at)] = _dev(post_h[at])
            rest = np.ones(len(nodes_h), bool)
            rest[at] = False
            assert depth > 12 or (post_h[rest] == nodes_h[rest]).all()  # (the oracle changes touched nodes only)
            expected[key] = (post_h, post)
        post_h, post = expected[key]
        if not _same_bits(side.nodes, post):
            pytest.fail(f"{row}, {name}, tree after the write-back: " + _first_difference(side.nodes.cpu().numpy(), post_h))

    # ---- the next draw on the tree the write-back left: separate launches, per_draw, per_turn's own
    raw_m, leaves_m = E.model_draw(post_h, inp["u2"], row.stratified, row.n_items)
    w_m = E.model_weights(post_h, leaves_m, row.n_items, row.beta)
    turn_leaves, turn_w = turn.leaves.cpu().numpy(), turn.w.cpu().numpy()
    _check_leaves((row, "per_turn next leaves"), turn_leaves, leaves_m)
    _check_weights((row, "per_turn next weights"), turn_w, w_m)
    raw, leaves, w = _chain_draw(lib, q, H, chain.nodes, depth, u2, row, chain)
    _check_leaves((row, "chain next raw leaves"), raw, raw_m)
    _check_leaves((row, "chain next clamped leaves"), leaves, leaves_m)
    _check_weights((row, "chain next weights"), w, w_m)
    leaves, w = _fused_draw(lib, q, H, fused.nodes, depth, u2, row, fused)
    _check_leaves((row, "per_draw next leaves"), leaves, leaves_m)
    _check_weights((row, "per_draw next weights"), w, w_m)
    torch.cuda.synchronize()


@pytest.mark.parametrize("depth", range(1, 22))
def test_prioritized_entries_against_the_models(depth):
    rows = [r for r in E.PER_ROWS if E.depth_of(r.capacity) == depth]
    assert rows
    key, start = None, None
    for row in sorted(rows, key=lambda r: (r.capacity, E.TREE_KINDS.index(r.tree))):
        if key != (row.capacity, row.tree):
            key, start = (row.capacity, row.tree), _dev(E.per_tree(row.capacity, row.tree))  # one upload per start tree
        _run_per_row(row, start)
    print(f"depth {depth}: {len(rows)} rows; largest relative differences so far: {OBSERVED}")


def test_fused_entries_refuse_257_and_write_nothing():
    import torch

    from slimdqn import _hip as H

    lib, q = H.lib(), H.current_stream()
    cap, n = 512, E.PER_MAX_N + 1
    depth = E.depth_of(cap)
    start = _dev(E.per_tree(cap, "wide"))
    nodes = start.clone()
    rng = np.random.default_rng(257)
    u, wb, td = _dev(rng.random(n)), _dev(rng.integers(cap, size=n).astype(np.int32)), _dev(rng.random((3, n)).astype(np.float32))
    pri = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    mx = torch.full((1,), 0.5, dtype=torch.float64, device="cuda")
    leaves = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    scratch = torch.full((2 * E.ST_MAX_N,), -3.0, dtype=torch.float64, device="cuda")
    calls = (
        ("per_draw", lambda: lib.per_draw(H.ptr(nodes), depth, H.ptr(u), n, 1, cap, 0.4, H.ptr(leaves), H.ptr(w), q)),
        ("per_write_back", lambda: lib.per_write_back(H.ptr(nodes), depth, H.ptr(wb), H.ptr(td), 3, n, 0, 1e-3, 0.6, H.ptr(pri),
                                                      H.ptr(mx), H.ptr(scratch), q)),
        ("per_turn", lambda: lib.per_turn(H.ptr(nodes), depth, H.ptr(wb), H.ptr(td), 3, n, 0, 1e-3, 0.6, H.ptr(pri), H.ptr(mx),
                                          H.ptr(scratch), H.ptr(u), 1, cap, 0.4, H.ptr(leaves), H.ptr(w), q)),
    )
    for name, call in calls:
        rc = call()
        msg = lib.idqn_last_error().decode()
        assert rc == H.E_INVALID and msg.startswith(name + ":") and "n not in" in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert _same_bits(nodes, start)
    assert (pri == -1.0).all() and mx.item() == 0.5 and (leaves == -7).all() and (w == -7.0).all() and (scratch == -3.0).all()
