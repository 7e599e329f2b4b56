"""What ``PrioritizedLearner.step`` costs as one C call (``idqn_per_learn_on_replay``: k_per_draw, the replay-sourced step,
k_per_write_back) against the chain of calls (``fuse_per_step = False``) on the same commit and against the chain of the parent
commit's library, and what the two fused kernels cost alone against the launch pairs they replace.

  lunar       fc, obs 8, [100, 100], A = 4, K = 3, B = 32 (the LunarLander experiment)
  fc_520      fc, obs 8, [520], A = 4, K = 3, B = 32
  gcnn_smoke  cnn, (84, 84, 4), [2, 3, 1, 15], A = 6, K = 1, B = 32
  atari_b32   cnn, (84, 84, 4), [32, 64, 64, 512], A = 6, K = 5, B = 32  (plane path: the chain gathers, the call does not)
  atari_b256  the same at B = 256
  iiqn_n32    i-IQN on the Atari shape, K = 5, N = 32, B = 32

``--leg step:<config>`` (one process): two learners of the same seeds, ``fuse_per_step`` on and off; regions of ``--calls`` steps
alternate between them, ``--rounds`` times after a warm-up region each, timed on the host clock with a device synchronisation at
both ends.  With ``--tree DIR`` (a built checkout of the parent commit) only the chain exists and only it is measured.
``--leg kernels``: ``per_draw`` against ``per_sample_leaves`` + ``per_importance_weights`` and ``per_write_back`` against
``per_priorities_from_td`` + ``sumtree_set`` at n = 32 and 256 on a 2^20-leaf tree, regions of ``--calls`` launches between two
events.  Without ``--leg`` this is the driver: every leg in a fresh process under its own time limit, nothing started after a
failure; per measurement the median and [min, max] over the regions.  Writes ``profiles/per_step_fused.json``.
Usage: ``python tools/bench_per_step.py [--parent DIR] [--out profiles/per_step_fused.json]``.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT  # before the imports
sys.path[:0] = [TREE, os.path.join(TREE, "i-dqn_amd")]
ATARI = ("cnn", (84, 84), "uint8", 4, (84, 84, 4), 6)
CONFIGS = {  # name: (arch, frame shape, dtype, stack, obs, A, K, features, B, N)
    "lunar": ("fc", (8,), "float32", 1, 8, 4, 3, [100, 100], 32, 0),
    "fc_520": ("fc", (8,), "float32", 1, 8, 4, 3, [520], 32, 0),
    "gcnn_smoke": ATARI + (1, [2, 3, 1, 15], 32, 0),
    "atari_b32": ATARI + (5, [32, 64, 64, 512], 32, 0),
    "atari_b256": ATARI + (5, [32, 64, 64, 512], 256, 0),
    "iiqn_n32": ATARI + (5, [32, 64, 64, 512], 32, 32),
}


def step_leg(name, calls, rounds):
    import numpy as np
    import torch

    from slimdqn.networks.idqn import iDQN
    from slimdqn.networks.iiqn import iIQN
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement

    arch, shape, dtype, stack, obs, A, K, feats, B, N = CONFIGS[name]
    parent = TREE != ROOT

    def side(fuse):
        rb = ReplayBuffer(SlotPrioritizedSampler(0, 2000), batch_size=B, max_capacity=2000, stack_size=stack, update_horizon=1, gamma=0.99)
        rng = np.random.default_rng(1)
        for i in range(2500):
            frame = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == "uint8" else rng.standard_normal(shape).astype(np.float32)
            rb.add(TransitionElement(frame, int(rng.integers(A)), float(rng.normal()), i % 200 == 199, i % 200 == 199))
        rb.reuse_sample_buffers = True
        if N:
            agent = iIQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
        else:
            agent = iDQN(0, obs, A, K, feats, arch, 3e-4, 0.99, 1, 1, 10**9, 10**9)
        learner = PrioritizedLearner(agent, rb, beta=0.4, eps=1e-3, reduce="mean")
        learner.fuse_per_step = fuse
        if fuse:  # the route itself, whatever default the family has been given
            learner.fuse_per_family = dict.fromkeys(learner.fuse_per_family, True)
        return learner

    sides = {"chain": side(False)} if parent else {"fused": side(True), "chain": side(False)}

    def region(learner):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            learner.step()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / calls

    for learner in sides.values():
        region(learner)
    if not parent:
        assert sides["fused"].__dict__.get("_fused_ok") is True, "the one-call step did not run"
        assert sides["chain"].__dict__.get("_fused_ok") is None
        for n in ("_online", "_mu", "_nu"):  # the same steps on both sides, bit for bit
            assert torch.equal(getattr(sides["fused"].agent, n), getattr(sides["chain"].agent, n)), n
        assert torch.equal(sides["fused"].sampler._sum_tree._nodes_dev, sides["chain"].sampler._sum_tree._nodes_dev)
    reg = {k: [] for k in sides}
    for _ in range(rounds):
        for k, learner in sides.items():
            reg[k].append(region(learner))
    print("RESULT" + json.dumps({"leg": "step", "config": name, "tree": "parent" if parent else "this", "regions": reg}), flush=True)


def kernels_leg(calls, rounds):
    import numpy as np
    import torch

    from slimdqn import _hip
    from slimdqn.sample_collection.sum_tree import SumTree

    lib, q = _hip.lib(), _hip.current_stream()
    cap = 2**20
    tree = SumTree(cap)
    rng = np.random.default_rng(0)
    for lo in range(0, cap, 4096):
        tree.set(np.arange(lo, lo + 4096, dtype=np.int32), rng.random(4096) + 0.05)
    nodes, depth, scratch = _hip.ptr(tree._nodes_dev), tree._depth, _hip.ptr(tree._scratch)
    out = {}
    for n in (32, 256):
        u = torch.from_numpy(rng.random(n)).cuda()
        leaves = torch.zeros(n, dtype=torch.int32, device="cuda")
        w = torch.zeros(n, dtype=torch.float32, device="cuda")
        td = torch.from_numpy(rng.random((5, n)).astype(np.float32)).cuda()
        pri = torch.zeros(n, dtype=torch.float64, device="cuda")
        mx = torch.ones(1, dtype=torch.float64, device="cuda")

        def draw_pair():
            lib.per_sample_leaves(nodes, depth, _hip.ptr(u), n, 1, _hip.ptr(leaves), q)
            lib.per_importance_weights(nodes, depth, _hip.ptr(leaves), n, cap, 0.4, _hip.ptr(w), q)

        def draw_fused():
            lib.per_draw(nodes, depth, _hip.ptr(u), n, 1, cap, 0.4, _hip.ptr(leaves), _hip.ptr(w), q)

        def back_pair():
            lib.per_priorities_from_td(_hip.ptr(td), 5, n, 0, 1e-3, 0.6, _hip.ptr(pri), _hip.ptr(mx), q)
            lib.sumtree_set(nodes, depth, _hip.ptr(leaves), _hip.ptr(pri), n, scratch, q)

        def back_fused():
            lib.per_write_back(nodes, depth, _hip.ptr(leaves), _hip.ptr(td), 5, n, 0, 1e-3, 0.6, _hip.ptr(pri), _hip.ptr(mx), scratch, q)

        def region(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / calls

        fns = {"draw_pair": draw_pair, "draw_fused": draw_fused, "write_back_pair": back_pair, "write_back_fused": back_fused}
        for fn in fns.values():
            region(fn)
        reg = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                reg[k].append(region(fn))
        out[f"n{n}"] = reg
    print("RESULT" + json.dumps({"leg": "kernels", "regions": out}), flush=True)


def summary(values):
    s = sorted(values)
    return {"median": s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]), "min": s[0], "max": s[-1], "n": len(s)}


def driver(a):
    def run(leg, tree=None):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(a.calls), "--rounds", str(a.rounds)]
        if tree:
            cmd += ["--tree", tree, "--out", a.out]  # (--tree is read from the middle of the argument list)
        out = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
        if out.returncode or not line:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"leg {leg} failed with status {out.returncode}: nothing more is started")
        return json.loads(line[0][6:])

    res = {"method": {"calls": a.calls, "rounds": a.rounds, "parent_leg": "measured" if a.parent else "unmeasured"}, "step_us": {}}
    for name in CONFIGS:
        r = run(f"step:{name}")["regions"]
        row = {"fused": summary(r["fused"]), "chain": summary(r["chain"])}
        if a.parent:
            row["parent_chain"] = summary(run(f"step:{name}", tree=a.parent)["regions"]["chain"])
            row["fused_stays_default"] = row["fused"]["median"] < row["parent_chain"]["min"]  # the decision rule
        row["chain_over_fused"] = row["chain"]["median"] / row["fused"]["median"]
        res["step_us"][name] = row
        print(name, json.dumps(row), flush=True)
    k = run("kernels")["regions"]
    res["kernels_us"] = {n: {leg: summary(v) for leg, v in legs.items()} for n, legs in k.items()}
    print("kernels", json.dumps(res["kernels_us"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout whose package and library a leg measures (default: this one)")
    ap.add_argument("--parent", default=None, help="driver: a built checkout of the parent commit for the parent-chain leg")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_step_fused.json"))
    a = ap.parse_args()
    if a.leg is None:
        return driver(a)
    kind, _, rest = a.leg.partition(":")
    return step_leg(rest, a.calls, a.rounds) if kind == "step" else kernels_leg(a.calls, a.rounds)


if __name__ == "__main__":
    main()
