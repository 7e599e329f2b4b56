"""Edge table, seeded input scripts and fp64 numpy models for the sum-tree and prioritized-replay kernels.

No GPU and no ``slimdqn`` import: ``tests/test_sumtree_edges_host.py`` (CPU), ``tests/test_gpu_sumtree_edges.py`` (GPU) and
``oracle/make_golden.py --int-edges`` all import this file, so the three agree on every input by construction.

Two families of rows:

* ``SET_ROWS``  ``(capacity, n, kind, salt)`` -- one measured ``sumtree_set`` of ``n`` leaves on a pre-filled tree.  The expected
  node bytes are captured from the reference's own ``sum_tree.py`` (``tests/golden/int_path_sumtree_edges.npz``).
* ``PER_ROWS``  one draw, one write-back and one turn (write-back, then the next draw) of the prioritized extension, which the
  reference does not have: the expectations are the fp64 models at the end of this file.

The kernels' plan, as far as the table is laid out along it (csrc/sumtree_device.h, csrc/per_step_args.h):
``m`` = n rounded up to a power of two; m <= 512 sorts by rank counting, m >= 1024 by the bitonic network; phase 4 of the set
takes 8 * 1024 (leaf, level) pairs per round; ``wave_descend`` takes min(5, levels left) levels per round trip; ``k_per_draw``
runs 4 descents per workgroup and ``k_per_turn`` 16 per round of its one workgroup.
"""
import collections
import functools
import math

import numpy as np

from oracle.sumtree_ref import SumTreeRef

ST_THREADS, ST_MAX_N, PER_MAX_N = 1024, 4096, 256
LEAF_KINDS = ("unsorted", "half_duplicates", "all_equal", "ascending", "descending")
TREE_KINDS = ("wide", "exact", "zero_leaves", "all_zero", "mass_past_items")
TD_KINDS = ("plain", "zero_columns", "huge")
N_QUERY = 64  # targets of the captured query per set row

SetRow = collections.namedtuple("SetRow", "capacity n kind salt")
PerRow = collections.namedtuple(
    "PerRow", "capacity n tree n_items stratified beta alpha eps K reduce_max td with_out with_max max_above wb_kind")


def depth_of(capacity):
    return int(math.ceil(math.log2(capacity))) + 1


def pow2_at_least(n):
    m = 1
    while m < n:
        m <<= 1
    return m


def capacity_at_depth(depth):
    """A capacity whose tree has ``depth`` levels: the full tree at the depths the main rows use and at even depths, the
    smallest capacity of that depth (2^(depth-2) + 1 leaves in use, the right part of the tree empty) at the other odd ones."""
    if depth == 1:
        return 1
    if depth in (5, 13, 21) or depth % 2 == 0:
        return 1 << (depth - 1)
    return (1 << (depth - 2)) + 1


def wide(rng, n):
    """Values over nine binades: with values in [0, 1) alone the accumulation order often leaves no trace in the sums."""
    return rng.random(n) * 10.0 ** rng.uniform(-6, 3, n)


def leaf_set(rng, kind, n, hi):
    """``n`` leaf indices in [0, hi) of one of LEAF_KINDS (int32)."""
    if kind == "unsorted":
        out = rng.integers(hi, size=n)
    elif kind == "half_duplicates":  # the second half repeats the first, reversed (the values differ: first occurrence must win)
        h = n // 2
        a = rng.integers(hi, size=n - h)
        out = np.concatenate([a, a[:h][::-1]])
    elif kind == "all_equal":
        out = np.full(n, rng.integers(hi))
    else:
        out = np.sort(rng.choice(hi, n, replace=False) if hi >= n else rng.integers(hi, size=n))
        if kind == "descending":
            out = out[::-1]
    return np.ascontiguousarray(out, np.int32)


# ------------------------------------------------------------------------------------------------------------------
# sumtree_set rows
# ------------------------------------------------------------------------------------------------------------------
SET_NS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
SET_MAIN_DEPTHS = (1, 5, 13, 21)
# Rows whose first script (salt 0) happened to give the same node bytes in ascending and in descending accumulation order
# (few distinct leaves: one or two shared ancestors) carry the first salt at which the order shows
# (test_sumtree_edges_host.py::test_every_set_row_is_order_sensitive holds the table to it).
SET_SALTS = {
    (16, 2, "unsorted"): 2, (16, 3, "unsorted"): 5, (16, 3, "half_duplicates"): 3, (4096, 2, "unsorted"): 85,
    (4096, 3, "unsorted"): 8, (4096, 3, "half_duplicates"): 117, (4096, 3, "ascending"): 33, (4096, 3, "descending"): 27,
    (4096, 63, "half_duplicates"): 1, (4096, 64, "half_duplicates"): 1, (1048576, 2, "unsorted"): 337,
    (1048576, 3, "half_duplicates"): 38, (1048576, 3, "ascending"): 54, (1048576, 3, "descending"): 89,
    (1048576, 63, "half_duplicates"): 2, (1048576, 64, "half_duplicates"): 1, (1048576, 65, "ascending"): 1,
    (2, 33, "half_duplicates"): 1, (3, 33, "unsorted"): 2, (3, 33, "half_duplicates"): 4, (3, 1025, "half_duplicates"): 3,
    (2048, 33, "unsorted"): 1, (2048, 33, "half_duplicates"): 2, (4096, 33, "unsorted"): 1, (4096, 33, "half_duplicates"): 1,
    (8192, 33, "unsorted"): 1, (8192, 33, "half_duplicates"): 1, (8193, 33, "half_duplicates"): 4,
    (32768, 33, "half_duplicates"): 4, (32769, 33, "unsorted"): 1, (32769, 33, "half_duplicates"): 1,
    (131072, 33, "unsorted"): 2, (131072, 33, "half_duplicates"): 1, (131073, 33, "unsorted"): 1,
    (131073, 33, "half_duplicates"): 5, (524288, 33, "half_duplicates"): 1, (1048576, 33, "half_duplicates"): 2,
}


def _set_rows():
    rows = []
    for depth in SET_MAIN_DEPTHS:
        cap = capacity_at_depth(depth)
        for n in SET_NS:
            if cap == 1:  # one leaf: every kind is the same set, n copies of leaf 0 (the sort sees equal leaves only)
                rows.append((cap, n, "all_equal"))
                continue
            rows.append((cap, n, "unsorted"))
            if n >= 2:
                rows.append((cap, n, "half_duplicates"))
            if n in (3, 65, 513, 1025, 4096):
                rows += [(cap, n, k) for k in ("all_equal", "ascending", "descending")]
    for depth in range(1, 22):
        cap = capacity_at_depth(depth)
        for n in (33, 1025):
            for kind in ("all_equal",) if cap == 1 else ("unsorted", "half_duplicates"):
                if (cap, n, kind) not in rows:
                    rows.append((cap, n, kind))
    return tuple(SetRow(c, n, k, SET_SALTS.get((c, n, k), 0)) for c, n, k in rows)


def prefill_script(capacity):
    """The sets that fill the tree before the measured one: up to three chunks of 4096 distinct leaves, some values zero."""
    rng = np.random.default_rng([11, capacity])
    idx = rng.permutation(capacity)[: min(capacity, 3 * ST_MAX_N)].astype(np.int32)
    val = wide(rng, idx.size)
    val[rng.random(idx.size) < 0.1] = 0.0
    return [(idx[i : i + ST_MAX_N], val[i : i + ST_MAX_N]) for i in range(0, idx.size, ST_MAX_N)]


def set_row_inputs(row):
    """``(leaves int32, values)`` of the measured set: some values zero, float32-typed on every third script."""
    seed = [13, row.capacity, row.n, LEAF_KINDS.index(row.kind), row.salt]
    rng = np.random.default_rng(seed)
    idx = leaf_set(rng, row.kind, row.n, row.capacity)
    val = wide(rng, row.n)
    val[rng.random(row.n) < 0.1] = 0.0
    if sum(seed) % 3 == 2:
        val = val.astype(np.float32)
    return idx, val


def query_targets(row, root):
    """The seeded in-range targets of the captured query on the tree the measured set left (none on an empty tree)."""
    if not root > 0.0:
        return np.zeros(0, np.float64)
    rng = np.random.default_rng([17, row.capacity, row.n, LEAF_KINDS.index(row.kind)])
    t = rng.random(N_QUERY) * root
    t[0] = 0.0
    return np.minimum(t, np.nextafter(root, 0.0))


def run_set_row(make_tree, row):
    """Pre-fill, then the measured set, on ``make_tree(capacity)`` (the reference's SumTree or the oracle's): the tree."""
    tree = make_tree(row.capacity)
    for idx, val in prefill_script(row.capacity):
        tree.set(idx, val)
    tree.set(*set_row_inputs(row))
    return tree


@functools.lru_cache(maxsize=4)
def _set_start(capacity):
    tree = SumTreeRef(capacity)
    for idx, val in prefill_script(capacity):
        tree.set(idx, val)
    tree.nodes.setflags(write=False)
    return tree.nodes, tree.max_recorded_priority


def set_start_nodes(capacity):
    """The oracle's node array after the pre-fill (read-only, shared between the rows of one capacity)."""
    return _set_start(capacity)[0]


def ref_on(capacity, nodes, max_recorded=1.0):
    """A SumTreeRef that continues from a copy of ``nodes``."""
    ref = SumTreeRef(capacity)
    assert ref.nodes.shape == nodes.shape
    ref.nodes = np.array(nodes, np.float64)
    ref.max_recorded_priority = max_recorded
    return ref


def model_set_row(row):
    """The oracle's tree after the measured set of ``row``."""
    nodes, maxp = _set_start(row.capacity)
    ref = ref_on(row.capacity, nodes, maxp)
    ref.set(*set_row_inputs(row))
    return ref


# ------------------------------------------------------------------------------------------------------------------
# prioritized rows
# ------------------------------------------------------------------------------------------------------------------
PER_NS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
PER_MAIN_DEPTHS = (1, 5, 10, 21)


def mass_past_items_count(capacity):
    """n_items of the ``mass_past_items`` tree: leaf n_items - 1 holds nothing, the leaves from n_items on hold most of the mass."""
    return capacity // 2 + 1


def _per_rows():
    rows, seen = [], set()
    pairs = [(capacity_at_depth(d), n) for d in PER_MAIN_DEPTHS for n in PER_NS]
    pairs += [(capacity_at_depth(d), n) for d in range(1, 22) for n in (1, 33, 256)]
    for i, (cap, n) in enumerate(pairs):
        if (cap, n) in seen:
            continue
        seen.add((cap, n))
        rng = np.random.default_rng([19, cap, n])
        kinds = [k for k in TREE_KINDS if (k != "mass_past_items" or cap >= 4) and (k != "zero_leaves" or cap >= 2)]
        tree = kinds[i % len(kinds)] if rng.random() < 0.8 else "wide"
        if depth_of(cap) == 10 and n % 2 == 1:
            tree = "exact" if n % 4 == 1 else "mass_past_items"  # the residue-4 depth gets the two kinds a wrong walk shows on
        td = TD_KINDS[int(rng.choice(3, p=[0.5, 0.4, 0.1]))]
        beta = float(rng.choice([0.0, 0.4, 1.0]))
        if td == "huge":
            beta = min(beta, 0.4)  # (weights of the next draw stay float32 normals: the one-ulp bound means something)
        if tree == "mass_past_items":
            n_items = mass_past_items_count(cap) - int(rng.integers(2))
        else:
            n_items = int(rng.choice([1, cap, 1 + rng.integers(cap)], p=[0.15, 0.45, 0.4]))
        rows.append(PerRow(cap, n, tree, n_items, int(rng.integers(2)), beta, float(rng.choice([0.0, 0.6, 1.0])),
                           float(rng.choice([0.0, 1e-3])), int(rng.choice([1, 3, 5])), int(rng.integers(2)), td,
                           bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2)),
                           "half_duplicates" if depth_of(cap) in (5, 10) and i % 2 else LEAF_KINDS[int(rng.integers(5))]))
    # the one very large |TD| at the deepest tree and the largest batch, both outputs given
    rows.append(PerRow(1 << 20, 256, "zero_leaves", 1 << 20, 1, 0.4, 1.0, 1e-3, 5, 0, "huge", True, True, False, "half_duplicates"))
    return tuple(rows)


def tree_from_leaves(depth, leaves):
    """A node array whose inner nodes are the pairwise sums of their children, bottom-up."""
    nodes = np.zeros((1 << depth) - 1, np.float64)
    first_leaf = (1 << (depth - 1)) - 1
    nodes[first_leaf : first_leaf + len(leaves)] = leaves
    for level in range(depth - 2, -1, -1):
        lo, hi = (1 << level) - 1, (1 << (level + 1)) - 1
        nodes[lo:hi] = nodes[2 * lo + 1 : 2 * hi + 1 : 2] + nodes[2 * lo + 2 : 2 * hi + 2 : 2]
    return nodes


@functools.lru_cache(maxsize=6)
def per_tree(capacity, kind):
    """The start tree of every row with this capacity and tree kind (read-only)."""
    rng = np.random.default_rng([23, capacity, TREE_KINDS.index(kind)])
    if kind == "wide":
        leaves = wide(rng, capacity) + 1e-9
    elif kind == "exact":  # small integers, zeros among them: every sum in the tree is exact
        leaves = rng.integers(0, 4, capacity).astype(np.float64)
        leaves[capacity // 2] = 3.0
    elif kind == "zero_leaves":
        leaves = wide(rng, capacity) * (rng.random(capacity) < 0.6)
        leaves[rng.integers(capacity)] = 0.0
        leaves[(capacity - 1) // 3] = 0.75
    elif kind == "all_zero":
        leaves = np.zeros(capacity)
    else:
        t = mass_past_items_count(capacity)
        leaves = wide(rng, capacity) + 0.5
        leaves[:t] *= 1e-4
        leaves[t - 1] = 0.0
    nodes = tree_from_leaves(depth_of(capacity), leaves)
    nodes.setflags(write=False)
    return nodes


def first_leaf_of(nodes):
    return (len(nodes) + 1) // 2 - 1


def _exact_uniforms(rng, u, nodes, capacity, stratified):
    """Replaces every second uniform by one whose target is EXACTLY a prefix sum of the leaves (the boundary between two
    leaves: the walk must go right there), where the model confirms the equality in fp64."""
    n, root = len(u), nodes[0]
    fl = first_leaf_of(nodes)
    cs = np.cumsum(nodes[fl : fl + capacity])
    for i in range(0, n, 2):
        if stratified:
            k0 = int(np.searchsorted(cs, i * root / n, "left"))
            cand = cs[k0 : k0 + 4]
        else:
            cand = cs[rng.integers(capacity, size=4)]
        for c in cand:
            v = c * n / root - i if stratified else c / root
            if 0.0 <= v < 1.0 and c < root:
                t = (np.float64(i) + v) / np.float64(n) * root if stratified else v * root
                if t == c:
                    u[i] = v
                    break
    return u


def per_row_inputs(row):
    """Everything a prioritized row feeds the device: uniforms of the draw and of the draw after the write-back, the leaves
    and |TD| of the write-back, the value the running maximum starts at."""
    rng = np.random.default_rng([29, row.capacity, row.n, TREE_KINDS.index(row.tree)])
    n, nodes = row.n, per_tree(row.capacity, row.tree)
    u, u2 = rng.random(n), rng.random(n)
    for v in (u, u2):
        v[rng.integers(n)] = np.nextafter(1.0, 0.0)
        v[rng.integers(n)] = 0.0
    if row.tree == "exact":
        u = _exact_uniforms(rng, u, nodes, row.capacity, row.stratified)
    td = rng.random((row.K, n)) * 10.0 ** rng.uniform(-4, 2, (row.K, n))
    if row.td == "zero_columns":
        td[:, rng.random(n) < 0.25] = 0.0
        td[:, rng.integers(n)] = 0.0
    elif row.td == "huge":
        td = (rng.random((row.K, n)) + 0.5) * 1e30
    return dict(u=u, u2=u2, leaves=leaf_set(rng, row.wb_kind, n, row.n_items), td=np.ascontiguousarray(td, np.float32),
                max_start=1e35 if row.max_above else 2.0 ** -40)


# ------------------------------------------------------------------------------------------------------------------
# fp64 models (numpy, as plain as they go)
# ------------------------------------------------------------------------------------------------------------------
def model_targets(u, root, stratified):
    """u * root, or the stratified (i + u) / n * root; clamped below the root."""
    n = len(u)
    t = (np.arange(n, dtype=np.float64) + u) / np.float64(n) * root if stratified else u * root
    return np.minimum(t, np.nextafter(root, 0.0))


def model_descend(nodes, targets):
    """Left when t < left sum, else subtract it and go right; no per-level assertion (the device ignores that bit for draws)."""
    first_leaf = first_leaf_of(nodes)
    out = np.zeros(len(targets), np.int64)
    for i, t in enumerate(np.asarray(targets, np.float64).tolist()):
        node = 0
        while node < first_leaf:
            left = 2 * node + 1
            left_sum = float(nodes[left])
            if t < left_sum:
                node = left
            else:
                t = t - left_sum
                node = left + 1
        out[i] = node - first_leaf
    return out


def model_draw(nodes, u, stratified, n_items):
    """``(raw leaves, clamped leaves)``: an empty tree answers leaf 0; leaves are clamped to [0, n_items - 1]."""
    root = nodes[0]
    raw = model_descend(nodes, model_targets(u, root, stratified)) if root > 0.0 else np.zeros(len(u), np.int64)
    return raw, np.clip(raw, 0, n_items - 1)


def model_raw_weights(nodes, leaves, n_items, beta):
    root = nodes[0]
    p = nodes[first_leaf_of(nodes) + np.asarray(leaves, np.int64)]
    w = np.zeros(len(p), np.float64)
    ok = (p > 0.0) & (root > 0.0)
    w[ok] = (np.float64(n_items) * p[ok] / root) ** (-beta)
    return w


def model_weights(nodes, leaves, n_items, beta):
    """(n_items p / root)^(-beta), 0 where p == 0 or the tree is empty, over the batch maximum; all 1 where that is 0."""
    w = model_raw_weights(nodes, leaves, n_items, beta)
    return w / w.max() if w.max() > 0.0 else np.ones(len(w), np.float64)


def model_priorities(td, reduce_max, eps, alpha):
    """(mean_k |td| + eps)^alpha or (max_k |td| + eps)^alpha, the reduction ascending in k."""
    td = np.asarray(td, np.float32).astype(np.float64)
    acc = np.zeros(td.shape[1], np.float64)
    for k in range(td.shape[0]):
        acc = np.maximum(acc, td[k]) if reduce_max else acc + td[k]
    if not reduce_max:
        acc = acc / np.float64(td.shape[0])
    return (acc + eps) ** alpha


def model_write_back(capacity, nodes, leaves, priorities, max_start):
    """``(node array, running maximum)``: SumTreeRef.set (first occurrence of a leaf wins) and a plain maximum."""
    ref = ref_on(capacity, nodes)
    ref.set(np.asarray(leaves, np.int32), np.asarray(priorities, np.float64))
    return ref.nodes, max(float(max_start), float(np.max(priorities)))


def touched_nodes(nodes, leaves):
    """Heap indices of every node a set of ``leaves`` may change (the leaves and all their ancestors), ascending."""
    cur = np.unique(first_leaf_of(nodes) + np.asarray(leaves, np.int64))
    out = [cur]
    while cur[0] > 0:
        cur = np.unique((cur - 1) // 2)
        out.append(cur)
    return np.sort(np.concatenate(out))


SET_ROWS = _set_rows()
PER_ROWS = _per_rows()
