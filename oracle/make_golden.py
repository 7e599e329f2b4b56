"""Generates the committed golden vectors under tests/golden/ (run in the BUILD container only).

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden [--int] [--int-edges] [--replay] [--fp]

--replay  imports the reference's ``slimdqn/sample_collection/replay_buffer.py`` and ``samplers.py`` as-is.  The three
       modules replay_buffer.py imports at its top and that are not installed (``jax``, ``flax.struct``, ``snappy``) are
       stand-ins written here (``install_replay_standins``: dataclass plumbing only, no reference behaviour).  Scripted,
       seeded streams (``REPLAY_STREAMS``; tests/replay_pinned.py lists their corners, which this mode ASSERTS while it
       records) go through ``ReplayBuffer(..., compress=False)`` with the reference's uniform and prioritized samplers;
       written are the stream, at checkpoints ``add_count`` / the live keys / every field of every live element (rewards
       as float64), the sampler's drawn keys and the stacked batches of a few ``sample()`` calls.  Only data is written;
       the file is written without time stamps, so a second run gives the same bytes.
       -> tests/golden/int_path_replay.npz
--int  imports the reference's ``slimdqn/sample_collection/sum_tree.py`` as-is and its
       ``samplers.py`` (whose only obstacle is an unused ``import jax`` at samplers.py:7; an empty
       placeholder module object is put in ``sys.modules`` for that name -- no jax functionality is
       stood in for, nothing in samplers.py ever touches the name) from ``/root/reference`` and
       records operation traces: inputs AND the reference's outputs (node arrays, roots, query
       results, sampled keys, index maps).  Only data is written; no reference source travels.
       -> tests/golden/int_path_sumtree.npz, int_path_samplers.npz
--int-edges  imports the reference's ``sum_tree.py`` the same way and runs every ``sumtree_set`` row of the edge table
       (tests/sumtree_edges.py: pre-fill, then the measured set) through it.  Per row: the sha256 of the node array, the root,
       ``max_recorded_priority`` and the reference's ``query`` output for seeded in-range targets.  The inputs are regenerated
       from the table, so only results are written; written without time stamps, so a second run gives the same bytes.
       -> tests/golden/int_path_sumtree_edges.npz
--iqn  the same for the i-IQN extension (``oracle/iqn_ref.py``; the reference has no quantile code at all).
       -> tests/golden/fp_path_iqn_*.json
--fp   writes expected losses / gradient / post-Adam probes of the fp64 numpy restatement
       (``oracle/qnet_ref.py``) for seeded inputs.  NOT reference-captured (jax is not installed):
       "parity unpinned" for this part, see oracle/__init__.py.
       -> tests/golden/fp_path_*.json

The GPU box never has /root/reference: tests only read the files written here.
"""
import argparse
import collections
import hashlib
import json
import os
import sys
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
REFERENCE = "/root/reference"


# ----------------------------------------------------------------------------------------------
# integer / fp64 path: captured from the reference
# ----------------------------------------------------------------------------------------------
def sumtree_op_script(seed, capacity, n_ops, max_batch):
    """A seeded script of set() calls: duplicates, float32-typed values, zeros, scalars."""
    rng = np.random.default_rng(seed)
    ops = []
    for j in range(n_ops):
        kind = j % 5
        if kind == 4:  # scalar form
            ops.append((int(rng.integers(capacity)), float(rng.random() * 3)))
            continue
        n = int(rng.integers(1, max_batch + 1))
        idx = rng.integers(capacity, size=n).astype(np.int32)
        if kind == 1 and n > 2:  # force duplicates with DIFFERENT values: first occurrence must win
            idx[1:] = idx[: n - 1]
        val = rng.random(n) * (10.0 ** rng.integers(-3, 3))
        if kind == 2:
            val = val.astype(np.float32)
        if kind == 3:
            val[rng.random(n) < 0.3] = 0.0
        ops.append((idx, val))
    return ops


def capture_sumtree():
    from slimdqn.sample_collection import sum_tree  # the reference, imported as-is

    out = {}
    cases = [(1, 6, 1), (4, 12, 4), (8, 16, 8), (100, 60, 32), (1000, 80, 64), (1 << 20, 40, 256), (3000, 30, 1024)]
    meta = []
    for ci, (cap, n_ops, max_batch) in enumerate(cases):
        tree = sum_tree.SumTree(cap)
        ops = sumtree_op_script(100 + ci, cap, n_ops, max_batch)
        roots, maxp, digests = [], [], []
        for j, (idx, val) in enumerate(ops):
            tree.set(idx, val)
            out[f"c{ci}_op{j}_idx"] = np.asarray(idx)
            out[f"c{ci}_op{j}_val"] = np.asarray(val)
            roots.append(tree.root)
            maxp.append(tree.max_recorded_priority)
            digests.append(hashlib.sha256(tree._nodes.tobytes()).hexdigest())
        rng = np.random.default_rng(7 + ci)
        targets = rng.uniform(0.0, tree.root, size=257)
        targets[0] = 0.0
        targets[1] = tree.root * (1.0 - 1e-6)
        out[f"c{ci}_roots"] = np.asarray(roots, np.float64)
        out[f"c{ci}_maxp"] = np.asarray(maxp, np.float64)
        out[f"c{ci}_q_targets"] = targets
        out[f"c{ci}_q_out"] = tree.query(targets)
        if cap <= 3000:
            out[f"c{ci}_nodes"] = tree._nodes.copy()
        probe = rng.integers(tree._nodes.size, size=64)
        out[f"c{ci}_probe_idx"] = probe
        out[f"c{ci}_probe_val"] = tree._nodes[probe]
        meta.append({"capacity": cap, "n_ops": len(ops), "depth": tree._depth, "n_nodes": int(tree._nodes.size),
                     "first_leaf": int(tree._first_leaf_offset), "digests": digests})
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(GOLDEN, "int_path_sumtree.npz"), **out)
    print("wrote int_path_sumtree.npz", len(out), "arrays")


def capture_sumtree_edges():
    from slimdqn.sample_collection import sum_tree  # the reference, imported as-is

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import sumtree_edges as E

    rows = E.SET_ROWS
    out = {"rows": np.asarray([(r.capacity, r.n, E.LEAF_KINDS.index(r.kind), r.salt) for r in rows], np.int64),
           "digests": np.zeros((len(rows), 32), np.uint8), "roots": np.zeros(len(rows), np.float64),
           "maxp": np.zeros(len(rows), np.float64), "q_out": np.full((len(rows), E.N_QUERY), -1, np.int32)}
    for i, row in enumerate(rows):
        tree = E.run_set_row(sum_tree.SumTree, row)
        out["digests"][i] = np.frombuffer(hashlib.sha256(tree._nodes.tobytes()).digest(), np.uint8)
        out["roots"][i] = tree.root
        out["maxp"][i] = tree.max_recorded_priority
        targets = E.query_targets(row, float(tree.root))
        if targets.size:
            out["q_out"][i] = tree.query(targets)
    write_npz_deterministic(os.path.join(GOLDEN, "int_path_sumtree_edges.npz"), out)
    print("wrote int_path_sumtree_edges.npz", len(rows), "rows")


def capture_samplers():
    sys.modules.setdefault("jax", types.ModuleType("jax"))  # unused import at samplers.py:7
    from slimdqn.sample_collection import samplers  # the reference

    out, meta = {}, []
    # uniform: interleaved add / remove / sample; op codes 0=add 1=remove 2=sample(n)
    for ci, (seed, n_ops) in enumerate([(0, 200), (1, 400), (12345, 300)]):
        rng = np.random.default_rng(900 + ci)
        u = samplers.UniformSamplingDistribution(seed)
        live, next_key, script, samples = [], 0, [], []
        for j in range(n_ops):
            c = rng.random()
            if c < 0.5 or len(live) < 3:
                u.add(next_key); live.append(next_key); script.append((0, next_key)); next_key += 1
            elif c < 0.7:
                k = live.pop(int(rng.integers(len(live)))); u.remove(k); script.append((1, k))
            else:
                n = int(rng.integers(1, 40)); s = u.sample(n); script.append((2, n)); samples.append(s)
        out[f"u{ci}_script"] = np.asarray(script, np.int64)
        out[f"u{ci}_samples"] = np.concatenate(samples)
        out[f"u{ci}_final_index_to_key"] = np.asarray(u._index_to_key, np.int64)
        meta.append({"kind": "uniform", "seed": seed})
    # prioritized: 0=add(key,prio) 1=remove(key) 2=sample(n) 3=update(keys,prios)
    for ci, (seed, cap, alpha, n_ops) in enumerate([(0, 10, 1.0, 120), (3, 64, 0.6, 300), (5, 1000, 0.5, 400)]):
        rng = np.random.default_rng(700 + ci)
        p = samplers.PrioritizedSamplingDistribution(seed, cap, alpha)
        live, next_key, recs = [], 0, []
        for j in range(n_ops):
            c = rng.random()
            if (c < 0.45 or len(live) < 3) and len(live) < cap:
                pr = 0.0 if rng.random() < 0.15 else float(rng.random() * 5)
                p.add(next_key, priority=pr); live.append(next_key)
                recs.append({"op": 0, "key": next_key, "prio": pr}); next_key += 1
            elif c < 0.6 and len(live) > 3:
                k = live.pop(int(rng.integers(len(live)))); p.remove(k); recs.append({"op": 1, "key": k})
            elif c < 0.8:
                n = int(rng.integers(1, min(len(live), 16) + 1))
                ks = rng.choice(np.asarray(live), size=n, replace=bool(rng.random() < 0.3)).astype(np.int32)
                pr = rng.random(n) * 4
                pr[rng.random(n) < 0.2] = 0.0
                p.update(ks, pr); recs.append({"op": 3, "keys": ks.tolist(), "prios": pr.tolist()})
            else:
                if p._sum_tree.root == 0.0:
                    continue
                n = int(rng.integers(1, 40)); s = p.sample(n)
                recs.append({"op": 2, "n": n, "out": s.tolist(), "root": float(p._sum_tree.root)})
        meta.append({"kind": "prioritized", "seed": seed, "cap": cap, "alpha": alpha, "recs": recs,
                     "final_index_to_key": [int(k) for k in p._index_to_key],
                     "final_digest": hashlib.sha256(p._sum_tree._nodes.tobytes()).hexdigest()})
        out[f"p{ci}_final_nodes"] = p._sum_tree._nodes.copy()
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(GOLDEN, "int_path_samplers.npz"), **out)
    print("wrote int_path_samplers.npz")


# ----------------------------------------------------------------------------------------------
# replay buffer: captured from the reference's replay_buffer.py (compress=False)
# ----------------------------------------------------------------------------------------------
def install_replay_standins():
    """Stand-in modules for the three imports at the top of the reference's replay_buffer.py.  They are this project's
    own and stand in for NO reference behaviour beyond dataclass plumbing: ``flax.struct.PyTreeNode`` makes a subclass
    a frozen dataclass with ``.replace``, ``jax.tree_util.tree_map`` maps a function over the dataclass fields of its
    arguments (what ``sample()`` uses to stack elements), ``snappy`` is empty (``compress=False`` never touches it)."""
    import dataclasses

    class PyTreeNode:
        def __init_subclass__(cls, **kwargs):
            super().__init_subclass__(**kwargs)
            dataclasses.dataclass(frozen=True)(cls)

        def replace(self, **changes):
            return dataclasses.replace(self, **changes)

    def tree_map(f, *trees):
        fields = [fld.name for fld in dataclasses.fields(trees[0])]
        return type(trees[0])(**{n: f(*[getattr(t, n) for t in trees]) for n in fields})

    jax, tree_util = types.ModuleType("jax"), types.ModuleType("jax.tree_util")
    flax, struct = types.ModuleType("flax"), types.ModuleType("flax.struct")
    tree_util.tree_map, jax.tree_util = tree_map, tree_util
    struct.PyTreeNode, flax.struct = PyTreeNode, struct
    sys.modules.update({"jax": jax, "jax.tree_util": tree_util, "flax": flax, "flax.struct": struct,
                        "snappy": types.ModuleType("snappy")})


#  name      frame shape  dtype  stack n  gamma cap  sampler        T    longest episode / extras
REPLAY_STREAMS = [
    # frame sizes 4, 6, 36, 63, 64 bytes: the byte path, the packed uint8 x 4 path and the 16-byte path of replay.hip
    dict(name="u8x4", shape=(4,), dtype="uint8", stack=4, n=1, gamma=0.97, cap=16, sampler="uniform", T=300, longest=9),
    dict(name="u8x6", shape=(2, 3), dtype="uint8", stack=3, n=2, gamma=1.0, cap=2, sampler="uniform", T=120, longest=6),
    # the ring of cap + n + stack + 64 = 79 frames has to grow: 40 truncated episodes of n transitions make no element
    dict(name="u8x36", shape=(6, 6), dtype="uint8", stack=4, n=3, gamma=0.97, cap=8, sampler="uniform", T=300, longest=9,
         elementless=40),
    dict(name="u8x63", shape=(7, 9), dtype="uint8", stack=2, n=5, gamma=0.97, cap=1, sampler="uniform", T=120, longest=8),
    # n >= the longest episode (every element comes out of a terminal flush) and cap < n + stack
    dict(name="u8x64", shape=(8, 8), dtype="uint8", stack=4, n=7, gamma=1.0, cap=5, sampler="prioritized", alpha=0.6, T=160,
         longest=7),
    dict(name="u8x84x84", shape=(84, 84), dtype="uint8", stack=4, n=1, gamma=0.97, cap=3, sampler="uniform", T=24, longest=6,
         blocky=7, every=0, batch=2),
    dict(name="i64x3", shape=(3,), dtype="int64", stack=3, n=5, gamma=0.97, cap=16, sampler="prioritized", alpha=1.0, T=150,
         longest=9),
    # the learner cases of tests/test_gpu_replay_pinned.py: MLP on float32 frames (stack 1 and 2), plane-path cnn on 20 x 20
    dict(name="f32s1", shape=(8,), dtype="float32", stack=1, n=2, gamma=0.97, cap=40, sampler="uniform", T=150, longest=7),
    dict(name="f32s2", shape=(9,), dtype="float32", stack=2, n=2, gamma=0.97, cap=40, sampler="uniform", T=150, longest=7),
    dict(name="u8x20x20", shape=(20, 20), dtype="uint8", stack=4, n=1, gamma=0.97, cap=48, sampler="uniform", T=130, longest=9,
         every=0, batch=3),
    # three time lines of one frame shape and unequal episode lengths for the E = 3 vector ring; nothing is evicted, so
    # the last checkpoint holds every element they ever made
    dict(name="vec0", shape=(3, 5), dtype="uint8", stack=4, n=3, gamma=0.97, cap=256, sampler="uniform", T=130, longest=5),
    dict(name="vec1", shape=(3, 5), dtype="uint8", stack=4, n=3, gamma=0.97, cap=256, sampler="uniform", T=130, longest=7),
    dict(name="vec2", shape=(3, 5), dtype="uint8", stack=4, n=3, gamma=0.97, cap=256, sampler="uniform", T=130, longest=11),
]


def replay_stream_script(spec, seed):
    """``[(terminal, episode_end)]`` per transition.  Episodes are scripted: every trajectory length 1 .. n + 1 (as far as
    the stream's longest episode allows) ends once in a terminal and once in a truncation; a transition with both flags; two
    terminals on consecutive transitions; the element-less run, if asked for; seeded episodes fill the rest.  The units are
    shuffled (seeded) and the stream is cut at T transitions."""
    rng = np.random.default_rng(seed)
    n, longest = spec["n"], spec["longest"]
    corner = range(1, min(n + 1, longest) + 1)
    units = [[(L, kind)] for L in corner for kind in ("terminal", "truncated")]
    units += [[(2, "terminal"), (1, "terminal"), (1, "terminal")], [(min(3, longest), "both")], [(1, "both")]]
    room = spec["T"] - sum(L for u in units for L, _ in u) - (n * spec["elementless"] + longest if spec.get("elementless") else 0)
    assert room >= 0, "the scripted corners alone are longer than the stream"
    while True:
        L, kind = int(rng.integers(1, longest + 1)), ("terminal", "terminal", "truncated", "both")[int(rng.integers(4))]
        if L > room:
            break  # (the stream ends inside an unfinished episode)
        units.append([(L, kind)])
        room -= L
    order = rng.permutation(len(units))
    units = [units[i] for i in order]
    if spec.get("elementless"):  # after a stretch that made elements, with more of them behind it
        at = len(units) // 3
        units[at:at] = [[(longest, "terminal")], [(n, "truncated")] * spec["elementless"]]
    flags = []
    for unit in units:
        for L, kind in unit:
            flags += [(False, False)] * (L - 1) + [(kind != "truncated", kind != "terminal")]
    assert len(flags) <= spec["T"]
    return flags + [(False, False)] * (spec["T"] - len(flags))


def replay_frame(rng, spec):
    """A frame without a zero in it (so a zero channel of a stack is padding, never data)."""
    shape, dtype = spec["shape"], np.dtype(spec["dtype"])
    if spec.get("blocky"):  # the one large frame: blocks of equal pixels, so that the file stays small
        b = spec["blocky"]
        return np.kron(rng.integers(1, 256, (shape[0] // b, shape[1] // b)), np.ones((b, b), np.int64)).astype(dtype)
    if dtype == np.float32:
        f = rng.standard_normal(shape).astype(np.float32)
        return np.where(f == 0, np.float32(1), f)
    if dtype == np.uint8:
        return rng.integers(1, 256, shape).astype(np.uint8)
    return rng.integers(1, 1 << 40, shape).astype(dtype) * np.where(rng.random(shape) < 0.5, -1, 1).astype(dtype)


def write_npz_deterministic(path, arrays):
    """``np.savez_compressed`` without the clock: fixed member dates, so the same arrays give the same bytes."""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, value in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(value), allow_pickle=False)


ELEMENT_FIELDS = ("state", "action", "reward", "next_state", "is_terminal", "episode_end")
ELEMENT_DTYPES = dict(action=np.int64, reward=np.float64, is_terminal=np.bool_, episode_end=np.bool_)


def _stacked(elements, field, like, dtype):
    """One field of a list of elements as an array (frame stacks keep their dtype; an empty list keeps the shape)."""
    if field in ELEMENT_DTYPES:
        return np.asarray([getattr(e, field) for e in elements], ELEMENT_DTYPES[field])
    if not elements:
        return np.zeros((0,) + like, dtype)
    return np.stack([getattr(e, field) for e in elements])


def capture_replay():
    install_replay_standins()
    from slimdqn.sample_collection import replay_buffer, samplers  # the reference, imported as-is

    out, meta, seen = {}, [], collections.defaultdict(set)
    for si, spec in enumerate(REPLAY_STREAMS):
        name, n, stack, cap, T = spec["name"], spec["n"], spec["stack"], spec["cap"], spec["T"]
        rng = np.random.default_rng(4000 + si)
        flags = replay_stream_script(spec, 5000 + si)
        assert len(flags) == T
        batch = spec.get("batch", 8)
        if spec["sampler"] == "uniform":
            sampler = samplers.UniformSamplingDistribution(si)
        else:  # (the key is added before the oldest one leaves: the tree holds cap + 1 leaves for a moment)
            sampler = samplers.PrioritizedSamplingDistribution(si, cap + 8, spec["alpha"])
        rb = replay_buffer.ReplayBuffer(sampler, batch_size=batch, max_capacity=cap, stack_size=stack, update_horizon=n,
                                        gamma=spec["gamma"], compress=False)
        drawn, real_sample = [], sampler.sample
        sampler.sample = lambda size: drawn.append(real_sample(size)) or drawn[-1]
        every = spec.get("every", 37)
        obs, action, reward, priority, checkpoints = [], [], [], [], []
        # elements of all checkpoints / batches of all draws / updates, each concatenated in order (the counts are in `meta`)
        live, batches, updates = (collections.defaultdict(list) for _ in range(3))
        quiet, cover = 0, seen[name]
        for t, (terminal, episode_end) in enumerate(flags):
            obs.append(replay_frame(rng, spec))
            action.append(int(rng.integers(0, 6)))
            reward.append(float(rng.normal()))
            priority.append(0.0 if rng.random() < 0.15 else float(rng.random() * 5))
            length = min(len(rb._trajectory) + 1, n + stack)  # the trajectory length this transition makes
            before = rb.add_count
            kwargs = {"priority": priority[-1]} if spec["sampler"] == "prioritized" else {}
            rb.add(replay_buffer.TransitionElement(obs[-1], action[-1], reward[-1], terminal, episode_end), **kwargs)
            made = rb.add_count - before
            # ---- what this transition covered (asserted below, per stream and per file)
            kind = "both" if terminal and episode_end else "terminal" if terminal else "truncated" if episode_end else None
            if kind:
                cover.add((kind, length))
                if terminal and t and flags[t - 1][0]:
                    cover.add("back-to-back terminals")
                if terminal and 2 <= length <= n:
                    assert made == length - 1  # one element per popleft, horizons length - 1 ... 1
                    cover.add("early-terminal flush")
                if not terminal:
                    assert len(rb._trajectory) == 0
            if made > cap:
                cover.add("an element made and evicted in one add")
            if made > 1 and rb.add_count > cap and cap < n + stack:
                cover.add("eviction inside a flush, capacity below n + stack")
            quiet = 0 if made or not before else quiet + 1
            if quiet >= cap + n + stack + max(64, cap // 16) and len(rb._memory) == cap:
                cover.add("element-less run longer than the frame ring")  # (ReplayBuffer._allocate's ring size)
            if (every and t % every == every - 1) or t == T - 1:
                cp = {"t": t, "add_count": int(rb.add_count), "samples": []}
                keys = [int(k) for k in rb._memory]
                els = [rb._memory[k] for k in keys]
                cp["n_live"] = len(keys)
                live["keys"].append(np.asarray(keys, np.int64))
                for field in ELEMENT_FIELDS:
                    live[field].append(_stacked(els, field, tuple(spec["shape"]) + (stack,), np.dtype(spec["dtype"])))
                if any(np.float64(np.float32(e.reward)) != e.reward for e in els):
                    cover.add("a reward that is no f32")
                for j, size in enumerate((None, 3) if keys else ()):
                    got = rb.sample() if size is None else rb.sample(size)
                    ks = drawn.pop()
                    assert not drawn
                    batches["keys"].append(np.asarray(ks, np.int32))
                    for field in ELEMENT_FIELDS:
                        batches[field].append(np.asarray(getattr(got, field)))
                    cp["samples"].append(int(len(ks)))
                    if stack > 1:
                        st, nx = np.asarray(got.state), np.asarray(got.next_state)
                        flat = lambda a: a.reshape(len(a), -1, stack)
                        if (flat(st)[:, :, 0] == 0).all(1).any():
                            cover.add("a sampled state stack crosses an episode start")
                        if ((flat(nx)[:, :, 0] == 0).all(1) & (flat(nx)[:, :, -1] != 0).all(1)).any():
                            cover.add("a sampled next_state stack crosses an episode start")
                    if len(set(ks.tolist())) < len(ks):
                        cover.add("a batch with a repeated key")
                if spec["sampler"] == "prioritized" and keys:  # an update between two checkpoints' draws
                    uk = np.asarray(keys[: min(4, len(keys))], np.int32)
                    up = rng.random(len(uk)) * 4
                    rb.update(uk, priorities=up)
                    updates["keys"].append(uk)
                    updates["priorities"].append(up)
                    cp["n_update"] = len(uk)
                    assert sampler._sum_tree.root > 0.0
                checkpoints.append(cp)
        for group, arrays in (("live", live), ("drawn", batches), ("update", updates)):
            for field, parts in arrays.items():
                out[f"{name}_{group}_{field}"] = np.concatenate(parts)
        out[name + "_observation"] = np.stack(obs)
        out[name + "_action"] = np.asarray(action, np.int64)
        out[name + "_reward"] = np.asarray(reward, np.float64)
        out[name + "_priority"] = np.asarray(priority, np.float64)
        out[name + "_is_terminal"] = np.asarray([f[0] for f in flags], np.bool_)
        out[name + "_episode_end"] = np.asarray([f[1] for f in flags], np.bool_)
        meta.append(dict({k: v for k, v in spec.items() if k not in ("blocky", "every", "elementless", "T", "longest")},
                         sampler_seed=si, tree_capacity=cap + 8, batch=batch, n_transitions=T, checkpoints=checkpoints))
        # ---- per stream: every corner length of its script happened
        for L in range(1, min(n + 1, spec["longest"]) + 1):
            assert ("terminal", L) in cover and ("truncated", L) in cover, (name, L)
        assert any(c[0] == "both" for c in cover if isinstance(c, tuple)) and "back-to-back terminals" in cover, name
        assert rb.add_count > 0 and checkpoints[-1]["samples"], name
    # ---- per file: the corners of the table in tests/replay_pinned.py's docstring
    by = {s["name"]: s for s in REPLAY_STREAMS}
    everything = set().union(*seen.values())
    for what in ("early-terminal flush", "an element made and evicted in one add", "eviction inside a flush, capacity below n + stack",
                 "element-less run longer than the frame ring", "a reward that is no f32", "a batch with a repeated key",
                 "a sampled state stack crosses an episode start", "a sampled next_state stack crosses an episode start"):
        assert what in everything, what
    assert "element-less run longer than the frame ring" in seen["u8x36"]
    assert {s["stack"] for s in REPLAY_STREAMS} >= {1, 2, 3, 4} and {s["n"] for s in REPLAY_STREAMS} >= {1, 2, 3, 5, 7}
    assert {s["dtype"] for s in REPLAY_STREAMS} >= {"uint8", "float32", "int64"} and {s["gamma"] for s in REPLAY_STREAMS} >= {0.97, 1.0}
    assert {s["cap"] for s in REPLAY_STREAMS} >= {1, 2} and {s["sampler"] for s in REPLAY_STREAMS} == {"uniform", "prioritized"}
    sizes = {int(np.prod(s["shape"])) * np.dtype(s["dtype"]).itemsize for s in REPLAY_STREAMS}
    assert sizes >= {4, 6, 36, 63, 64, 84 * 84}, sizes
    assert any(s["n"] > s["stack"] for s in REPLAY_STREAMS) and any(s["n"] >= s["longest"] for s in REPLAY_STREAMS)
    for s in REPLAY_STREAMS:  # a terminal at every trajectory length 1 .. n + 1, wherever episodes get that long
        if s["longest"] > s["n"]:
            assert {("terminal", L) for L in range(1, s["n"] + 2)} <= seen[s["name"]], s["name"]
    # (ReplayBuffer._allocate: cap + n + stack + max(64, cap // 16) frames) a ring that wraps several times
    assert by["u8x4"]["T"] > 3 * (16 + 1 + 4 + 64)
    assert len({(s["shape"], s["stack"], s["n"], s["gamma"]) for s in REPLAY_STREAMS if s["name"].startswith("vec")}) == 1
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(GOLDEN, "int_path_replay.npz")
    write_npz_deterministic(path, out)
    print("wrote int_path_replay.npz", len(out), "arrays,", os.path.getsize(path), "bytes")


# ----------------------------------------------------------------------------------------------
# fp path: from the fp64 restatement (not reference-captured)
# ----------------------------------------------------------------------------------------------
FP_CASES = {
    # name: (arch, obs_dim, n_actions, features, K, B, steps)
    "cnn_small": ("cnn", (20, 20, 4), 5, [32, 32, 32, 128], 2, 32, 2),
    "cnn_atari_k5": ("cnn", (84, 84, 4), 6, [32, 64, 64, 512], 5, 32, 2),
    "cnn_atari_a18_b64": ("cnn", (84, 84, 4), 18, [32, 64, 64, 512], 2, 64, 1),
    "fc_lunar_k3": ("fc", 8, 4, [100, 100], 3, 32, 3),
    # BASELINE configs 4 and 5 at their full single-device workload (one step each; probe indices keep the fixtures small)
    "cnn_atari_k5_b256": ("cnn", (84, 84, 4), 6, [32, 64, 64, 512], 5, 256, 1),
    "cnn_atari_k64": ("cnn", (84, 84, 4), 6, [32, 64, 64, 512], 64, 32, 1),
}
FP_HYPER = {"gamma": 0.99, "n": 1, "lr": 6.25e-5, "eps": 1.5e-4}


def fp_case_inputs(name):
    from . import qnet_ref as Q

    arch, obs, A, feats, K, B, steps = FP_CASES[name]
    seed = sum(name.encode())
    p = Q.init_params(seed, arch, obs, A, feats, K, np.float32)
    pt = Q.init_params(seed + 1, arch, obs, A, feats, K, np.float32)
    rng = np.random.default_rng(seed + 2)
    for n in p:  # non-zero biases so that bias handling is exercised
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batches = []
    for s in range(steps):
        st, a, r, s2, term = Q.synthetic_batch(seed + 10 + s, B, obs, A, arch)
        term[s % B] = True
        batches.append((st, a, r, s2, term))
    return p, pt, batches


def probe_indices(name, leaf, size, n=24):
    rng = np.random.default_rng(sum((name + leaf).encode()))
    return np.sort(rng.choice(size, size=min(n, size), replace=False))


def capture_fp(names=None):
    from . import qnet_ref as Q

    for name in names or FP_CASES:
        arch, obs, A, feats, K, B, steps = FP_CASES[name]
        p, pt, batches = fp_case_inputs(name)
        mu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
        nu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
        p64 = {n: a.astype(np.float64) for n, a in p.items()}
        count = np.zeros(K, np.int64)
        rec = {"case": name, "hyper": FP_HYPER, "steps": []}
        gamma_n = FP_HYPER["gamma"] ** FP_HYPER["n"]
        for s, batch in enumerate(batches):
            # forward probes for head 0 (first step only): q, q_next
            if s == 0:
                _, _, aux = Q.loss_and_grads(Q.head(p64, 0), Q.head(pt, 0), batch, arch, gamma_n)
                rec["q_head0"] = aux["q"].tolist()
                rec["q_next_head0"] = aux["q_next"].tolist()
            p64, mu, nu, count, losses, grads = Q.learn_on_batch(
                p64, pt, mu, nu, count, batch, arch, gamma_n, FP_HYPER["lr"], FP_HYPER["eps"], np.float64,
                return_grads=True)
            step = {"losses": losses.tolist(), "leaves": {}}
            for leaf in p64:
                flat_g = grads[leaf].reshape(K, -1)
                flat_p = p64[leaf].reshape(K, -1)
                idx = probe_indices(name, leaf, flat_g.shape[1])
                step["leaves"][leaf] = {
                    "idx": idx.tolist(),
                    "grad": flat_g[:, idx].tolist(),
                    "param": flat_p[:, idx].tolist(),
                    "grad_l2": np.sqrt((flat_g**2).sum(1)).tolist(),
                    "grad_absmax": np.abs(flat_g).max(1).tolist(),
                }
            rec["steps"].append(step)
        with open(os.path.join(GOLDEN, f"fp_path_{name}.json"), "w") as f:
            json.dump(rec, f)
        print("wrote", name, [s["losses"] for s in rec["steps"]])


# ----------------------------------------------------------------------------------------------
# i-IQN extension (oracle/iqn_ref.py; no reference code exists for it): fp64 restatement -> probes
# ----------------------------------------------------------------------------------------------
IQN_CASES = {  # name: (obs, A, features, K, B, N)
    "iqn_small": ((20, 20, 4), 5, [32, 32, 32, 256], 2, 32, 4),
    "iqn_small_ragged": ((20, 20, 4), 5, [32, 64, 32, 256], 2, 20, 5),
    "iqn_atari_k5": ((84, 84, 4), 6, [32, 64, 64, 512], 5, 32, 32),
}


def iqn_case_inputs(name):
    from . import iqn_ref as I
    from . import qnet_ref as Q

    obs, A, feats, K, B, N = IQN_CASES[name]
    seed = sum(name.encode())
    p = I.init_params(seed, obs, A, feats, K)
    pt = I.init_params(seed + 1, obs, A, feats, K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    st, a, r, s2, term = Q.synthetic_batch(seed + 10, B, obs, A, "cnn")
    term[0] = True
    taus = I.synthetic_taus(seed + 20, K, N, B)
    return p, pt, (st, a, r, s2, term), taus


def capture_iqn(names=None):
    from . import iqn_ref as I
    from . import qnet_ref as Q

    for name in names or IQN_CASES:
        obs, A, feats, K, B, N = IQN_CASES[name]
        p, pt, batch, taus = iqn_case_inputs(name)
        gamma_n = FP_HYPER["gamma"] ** FP_HYPER["n"]
        mu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
        nu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
        _, _, aux0 = I.loss_and_grads(Q.head(p, 0), Q.head(pt, 0), batch, tuple(taus[0]), gamma_n)
        p64, mu, nu, count, losses, grads = I.learn_on_batch(p, pt, mu, nu, np.zeros(K, np.int64), batch, taus, gamma_n,
                                                             FP_HYPER["lr"], FP_HYPER["eps"], np.float64, return_grads=True)
        rec = {"case": name, "hyper": FP_HYPER, "losses": losses.tolist(), "z_online_head0": aux0["z_a"].tolist(),
               "z_target_head0": aux0["z_t"].tolist(), "a_star_head0": aux0["a_star"].tolist(),
               "q_select_head0": aux0["q_sel"].tolist(), "leaves": {}}
        for leaf in p64:
            flat_g, flat_p = grads[leaf].reshape(K, -1), p64[leaf].reshape(K, -1)
            idx = probe_indices(name, leaf, flat_g.shape[1])
            rec["leaves"][leaf] = {"idx": idx.tolist(), "grad": flat_g[:, idx].tolist(), "param": flat_p[:, idx].tolist(),
                                   "grad_l2": np.sqrt((flat_g**2).sum(1)).tolist(), "grad_absmax": np.abs(flat_g).max(1).tolist()}
        with open(os.path.join(GOLDEN, f"fp_path_{name}.json"), "w") as f:
            json.dump(rec, f)
        print("wrote", name, rec["losses"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--int", action="store_true")
    ap.add_argument("--int-edges", action="store_true")
    ap.add_argument("--fp", action="store_true")
    ap.add_argument("--iqn", action="store_true")
    ap.add_argument("--replay", action="store_true")
    ap.add_argument("--cases", nargs="*")
    args = ap.parse_args()
    os.makedirs(GOLDEN, exist_ok=True)
    if args.int:
        sys.path.insert(0, REFERENCE)
        capture_sumtree()
        capture_samplers()
    if args.int_edges:
        sys.path.insert(0, REFERENCE)
        capture_sumtree_edges()
    if args.replay:
        sys.path.insert(0, REFERENCE)
        capture_replay()
    if args.fp:
        capture_fp(args.cases)
    if args.iqn:
        capture_iqn(args.cases)
