"""CPU: the edge table of tests/sumtree_edges.py can tell a subtly wrong sum-tree / prioritized-replay kernel from a right one.

1. coverage -- the table reaches every branch of the kernels' plans that it was laid out along;
2. the oracle (``SumTreeRef``) reproduces every digest, root, maximum and query the reference's own ``sum_tree.py`` left in
   ``tests/golden/int_path_sumtree_edges.npz`` for the ``sumtree_set`` rows;
3. every ``sumtree_set`` row with two distinct leaves is sensitive to the accumulation order;
4. ten deliberately wrong models each disagree with the right one on at least one row (the test names the first).
"""
import hashlib
import os

import numpy as np
import pytest

import sumtree_edges as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "int_path_sumtree_edges.npz")
F32_MIN_NORMAL = 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------
# the right models on every prioritized row, once
# ---------------------------------------------------------------------------------------------------------------
def _per_model(row):
    nodes, inp = E.per_tree(row.capacity, row.tree), E.per_row_inputs(row)
    raw, leaves = E.model_draw(nodes, inp["u"], row.stratified, row.n_items)
    pri = E.model_priorities(inp["td"], row.reduce_max, row.eps, row.alpha)
    post, mx = E.model_write_back(row.capacity, nodes, inp["leaves"], pri, inp["max_start"])
    raw2, leaves2 = E.model_draw(post, inp["u2"], row.stratified, row.n_items)
    return dict(nodes=nodes, inp=inp, raw=raw, leaves=leaves, w=E.model_weights(nodes, leaves, row.n_items, row.beta), pri=pri,
                post=post, mx=mx, raw2=raw2, leaves2=leaves2, w2=E.model_weights(post, leaves2, row.n_items, row.beta))


@pytest.fixture(scope="module")
def per_models():
    return [_per_model(row) for row in E.PER_ROWS]


# ---------------------------------------------------------------------------------------------------------------
# 1. coverage
# ---------------------------------------------------------------------------------------------------------------
def test_set_rows_cover_the_plan_of_the_batched_set():
    rows = E.SET_ROWS
    assert len(set(rows)) == len(rows)
    have = {(E.depth_of(r.capacity), r.n, r.kind) for r in rows}
    for n in E.SET_NS:
        for depth in E.SET_MAIN_DEPTHS:
            kinds = {k for d, nn, k in have if (d, nn) == (depth, n)}
            assert kinds >= ({"all_equal"} if depth == 1 else {"unsorted", "half_duplicates"} if n >= 2 else {"unsorted"}), (n, depth)
    for depth in range(1, 22):
        for n in (33, 1025):
            assert any((d, nn) == (depth, n) for d, nn, _ in have), (depth, n)
    ms = {E.pow2_at_least(r.n) for r in rows}
    assert min(ms) <= E.ST_THREADS // 2 and {512, 1024} <= ms  # both sort routes, and both sides of the switch between them
    for m in (1024, 2048, 4096):  # the bitonic network at each size: a ragged n, and duplicate leaves with different values
        ragged = [r for r in rows if E.pow2_at_least(r.n) == m and r.n != m and r.kind == "half_duplicates" and r.capacity > 1]
        assert ragged, m
        idx, val = E.set_row_inputs(ragged[0])
        dup = idx[: ragged[0].n // 2]
        assert len(np.unique(idx)) < len(idx) and (val[: len(dup)] != val[::-1][: len(dup)]).any()
    assert any(r.n > E.ST_THREADS for r in rows)  # register slots q >= 1
    assert any(r.n * E.depth_of(r.capacity) > 8 * E.ST_THREADS for r in rows)  # more than one round of phase 4
    assert any(r.n * E.depth_of(r.capacity) > 64 * E.ST_THREADS for r in rows)  # (and more than eight)
    assert {r.kind for r in rows} == set(E.LEAF_KINDS)
    dtypes = {E.set_row_inputs(r)[1].dtype for r in rows}
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any((E.set_row_inputs(r)[1] == 0.0).any() for r in rows)
    for r in rows:
        idx, val = E.set_row_inputs(r)
        assert idx.dtype == np.int32 and len(idx) == len(val) == r.n and 0 <= idx.min() and idx.max() < r.capacity and r.n <= E.ST_MAX_N


def test_per_rows_cover_the_plans_of_the_draw_the_write_back_and_the_turn(per_models):
    rows = E.PER_ROWS
    have = {(E.depth_of(r.capacity), r.n) for r in rows}
    assert all((d, n) in have for d in E.PER_MAIN_DEPTHS for n in E.PER_NS)
    assert all((d, n) in have for d in range(1, 22) for n in (1, 33, 256))
    assert all(1 <= r.n <= E.PER_MAX_N and 1 <= r.n_items <= r.capacity for r in rows)
    # wave_descend: all five sizes of the last round trip, each on a tree with many non-zero leaves and both target forms
    for residue in range(5):
        for stratified in (0, 1):
            assert any((E.depth_of(r.capacity) - 1) % 5 == residue and r.stratified == stratified and r.tree in ("wide", "exact", "mass_past_items")
                       and (r.capacity >= 9 or residue < 3) for r in rows), (residue, stratified)
    groups = {min((r.n + 3) // 4, 3) for r in rows}
    assert groups == {1, 2, 3}  # one, two and many k_per_draw workgroups
    assert any(r.n == 16 for r in rows) and any(r.n == 17 for r in rows) and any(r.n < 16 for r in rows)  # k_per_turn's rounds of 16
    for name, values in (("tree", E.TREE_KINDS), ("stratified", (0, 1)), ("beta", (0.0, 0.4, 1.0)), ("alpha", (0.0, 0.6, 1.0)),
                         ("eps", (0.0, 1e-3)), ("K", (1, 3, 5)), ("reduce_max", (0, 1)), ("td", E.TD_KINDS), ("with_out", (False, True)),
                         ("with_max", (False, True)), ("max_above", (False, True)), ("wb_kind", E.LEAF_KINDS)):
        assert {getattr(r, name) for r in rows} == set(values), name
    assert {(r.with_out, r.with_max) for r in rows} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(r.n_items == 1 and r.capacity > 1 for r in rows) and any(r.n_items == r.capacity > 1 for r in rows)
    assert any(1 < r.n_items < r.capacity for r in rows)
    clamped = zero_drawn = empty = dup_diff = boundary = below = above = zero_pri = 0
    dup_ns = set()
    for r, m in zip(rows, per_models):
        first_leaf = E.first_leaf_of(m["nodes"])
        clamped += bool((m["raw"] != m["leaves"]).any())
        zero_drawn += bool(m["nodes"][0] > 0.0 and (m["nodes"][first_leaf + m["leaves"]] == 0.0).any() and (m["w"] == 0.0).any())
        empty += bool(m["nodes"][0] == 0.0)
        if r.tree == "exact":  # targets exactly on a boundary between two leaves
            prefix = np.cumsum(m["nodes"][first_leaf : first_leaf + r.capacity])
            boundary += bool(np.isin(E.model_targets(m["inp"]["u"], m["nodes"][0], r.stratified), prefix).any())
        wb = m["inp"]["leaves"]
        for leaf in np.unique(wb):
            at = np.flatnonzero(wb == leaf)
            if len(at) > 1 and (m["pri"][at] != m["pri"][at[0]]).any():
                dup_diff += 1
                dup_ns.add(r.n)
                break
        below += bool(m["inp"]["max_start"] < m["pri"].max() and r.with_max)
        above += bool(m["inp"]["max_start"] > m["pri"].max() and r.with_max)
        zero_pri += bool((m["pri"] == 0.0).any())
        # the one-float32-ulp bound on the weights means something only on float32 normals
        for w in (m["w"], m["w2"]):
            assert (w[w > 0.0] >= 2 * F32_MIN_NORMAL).all() and np.isfinite(w).all() and np.isfinite(m["post"]).all(), r
        if r.td == "huge":
            assert m["inp"]["td"].max() > 1e29 and np.isfinite(m["inp"]["td"]).all()
    assert min(clamped, zero_drawn, empty, dup_diff, boundary, below, above, zero_pri) >= 2, (
        clamped, zero_drawn, empty, dup_diff, boundary, below, above, zero_pri)
    # duplicates are written back at every n >= 2 (capacity 1 has one leaf, so they are there at every n by construction)
    assert all(any(r.n == n and len(np.unique(m["inp"]["leaves"])) < n for r, m in zip(rows, per_models)) for n in E.PER_NS if n >= 2)
    assert len(dup_ns) >= 10


# ---------------------------------------------------------------------------------------------------------------
# 2. the oracle against what the reference left
# ---------------------------------------------------------------------------------------------------------------
def test_the_oracle_reproduces_the_reference_on_every_set_row():
    z = np.load(GOLDEN)
    want_rows = np.asarray([(r.capacity, r.n, E.LEAF_KINDS.index(r.kind), r.salt) for r in E.SET_ROWS], np.int64)
    np.testing.assert_array_equal(z["rows"], want_rows)  # (the file was made from this table)
    assert os.path.getsize(GOLDEN) < 100_000
    queried = 0
    for i, row in enumerate(E.SET_ROWS):
        ref = E.model_set_row(row)
        assert hashlib.sha256(ref.nodes.tobytes()).digest() == z["digests"][i].tobytes(), row
        assert ref.root == z["roots"][i] and float(ref.max_recorded_priority) == z["maxp"][i], row
        targets = E.query_targets(row, float(ref.root))
        if targets.size:
            np.testing.assert_array_equal(ref.query(targets), z["q_out"][i], err_msg=str(row))
            np.testing.assert_array_equal(E.model_descend(ref.nodes, targets), z["q_out"][i], err_msg=str(row))
            queried += 1
    assert queried >= len(E.SET_ROWS) - 4  # (a capacity-1 row whose one value is zero leaves an empty tree: nothing to query)


# ---------------------------------------------------------------------------------------------------------------
# 3., 4. wrong models
# ---------------------------------------------------------------------------------------------------------------
def set_variant(nodes, idx, val, keep="first", order="ascending", against="start"):
    """SumTree.set restated with its three decisions open, on the touched nodes only: ``{heap index: value}``.
    keep: which occurrence of a duplicate leaf counts; order: the order the kept deltas are added in at every node;
    against: deltas against the leaves at the start, or each occurrence against the leaf as the occurrences before it left it
    (every occurrence applied)."""
    leaves = (E.first_leaf_of(nodes) + idx.astype(np.int64)).tolist()
    vals = val.astype(np.float64).tolist()
    if against == "running":
        leaf_now, seq = {}, []
        for leaf, v in zip(leaves, vals):
            seq.append((leaf, v - leaf_now.get(leaf, float(nodes[leaf]))))
            leaf_now[leaf] = v
        seq.sort(key=lambda e: e[0])  # (stable: ascending leaves, occurrences in their order)
    else:
        pos = {}
        for p, leaf in enumerate(leaves):
            if keep == "last" or leaf not in pos:
                pos[leaf] = p
        seq = [(leaf, vals[pos[leaf]] - float(nodes[leaf])) for leaf in sorted(pos, reverse=order == "descending")]
    out = {}
    cur = [leaf for leaf, _ in seq]
    while True:
        for c, (_, d) in zip(cur, seq):
            out[c] = out.get(c, float(nodes[c])) + d
        if cur[0] == 0:
            return out
        cur = [(c - 1) // 2 for c in cur]


def test_set_variant_right_is_the_oracle():
    for row in E.SET_ROWS[::7]:
        idx, val = E.set_row_inputs(row)
        got, ref = set_variant(E.set_start_nodes(row.capacity), idx, val), E.model_set_row(row)
        assert all(ref.nodes[k] == v for k, v in got.items()), row
        rest = np.ones(len(ref.nodes), bool)
        rest[list(got)] = False
        assert (ref.nodes[rest] == E.set_start_nodes(row.capacity)[rest]).all(), row


def test_every_set_row_is_order_sensitive():
    checked = 0
    for row in E.SET_ROWS:
        idx, val = E.set_row_inputs(row)
        if len(np.unique(idx)) < 2:
            # one leaf: nothing to order.  Only the rows that are so by their kind, never by the luck of a script
            assert row.salt == 0 and (row.capacity == 1 or row.kind == "all_equal" or row.n == 1
                                      or (row.n == 2 and row.kind == "half_duplicates")), row
            continue
        start = E.set_start_nodes(row.capacity)
        assert set_variant(start, idx, val) != set_variant(start, idx, val, order="descending"), row
        checked += 1
    assert checked >= 200


def _first_set_row_that_differs(**mutation):
    for row in E.SET_ROWS:
        if row.capacity > 4096:
            continue
        idx, val = E.set_row_inputs(row)
        start = E.set_start_nodes(row.capacity)
        if set_variant(start, idx, val) != set_variant(start, idx, val, **mutation):
            return row
    return None


def _descend_le(nodes, targets):  # MUTANT: t <= left
    first_leaf, out = E.first_leaf_of(nodes), []
    for t in np.asarray(targets, np.float64).tolist():
        node = 0
        while node < first_leaf:
            left_sum = float(nodes[2 * node + 1])
            if t <= left_sum:
                node = 2 * node + 1
            else:
                t, node = t - left_sum, 2 * node + 2
        out.append(node - first_leaf)
    return np.asarray(out, np.int64)


def _first_per_row_that_differs(per_models, wrong):
    """``wrong(row, m)`` returns (the mutant's result, the right model's result) or None when the row does not apply."""
    for row, m in zip(E.PER_ROWS, per_models):
        pair = wrong(row, m)
        if pair is not None and not np.array_equal(np.asarray(pair[0]), np.asarray(pair[1])):
            return row
    return None


def test_every_mutant_is_caught_by_a_row(per_models):
    caught = {}
    caught["last occurrence wins"] = _first_set_row_that_differs(keep="last")
    caught["descending accumulation order"] = _first_set_row_that_differs(order="descending")
    caught["deltas against leaves after earlier duplicates were applied"] = _first_set_row_that_differs(against="running")

    def le(row, m):
        if not m["nodes"][0] > 0.0:
            return None
        return _descend_le(m["nodes"], E.model_targets(m["inp"]["u"], m["nodes"][0], row.stratified)), m["raw"]

    def no_clamp(row, m):
        return m["raw"], m["leaves"]

    def no_plus_i(row, m):
        if not (row.stratified and m["nodes"][0] > 0.0):
            return None
        root = m["nodes"][0]
        t = np.minimum(m["inp"]["u"] / np.float64(row.n) * root, np.nextafter(root, 0.0))
        return E.model_descend(m["nodes"], t), m["raw"]

    def sum_normalised(row, m):
        w = E.model_raw_weights(m["nodes"], m["leaves"], row.n_items, row.beta)
        return (w / w.sum() if w.sum() > 0.0 else np.ones(len(w))), m["w"]

    def reductions_swapped(row, m):
        return E.model_priorities(m["inp"]["td"], 1 - row.reduce_max, row.eps, row.alpha), m["pri"]

    def eps_after_power(row, m):
        td = m["inp"]["td"].astype(np.float64)
        acc = td.max(0) if row.reduce_max else E.model_priorities(td, 0, 0.0, 1.0)
        return acc ** row.alpha + row.eps, m["pri"]

    def maximum_overwritten(row, m):
        return float(m["pri"].max()), m["mx"]

    for name, wrong in (("t <= left", le), ("no clamp", no_clamp), ("stratified targets without the + i", no_plus_i),
                        ("weights normalised by the sum", sum_normalised), ("mean and max swapped", reductions_swapped),
                        ("eps added after the power", eps_after_power), ("running maximum overwritten", maximum_overwritten)):
        caught[name] = _first_per_row_that_differs(per_models, wrong)
    for name, row in caught.items():
        print(f"mutant '{name}': caught by {row}")
    assert all(row is not None for row in caught.values()), [name for name, row in caught.items() if row is None]
    # the boundary mutant shows on the rows made for it, at the depth whose last round trip has four levels too
    exact = [r for r, m in zip(E.PER_ROWS, per_models) if r.tree == "exact" and le(r, m) is not None
             and not np.array_equal(*le(r, m))]
    assert any((E.depth_of(r.capacity) - 1) % 5 == 4 for r in exact) and {r.stratified for r in exact} == {0, 1}, exact
