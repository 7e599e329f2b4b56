"""What n prioritized learner steps cost as one C call (``PrioritizedLearner.steps(n)`` -> ``idqn_per_learn_steps_on_replay``:
one upload, k_per_draw, then step / k_per_turn alternating, k_per_write_back) against the chain of n ``idqn_per_learn_on_replay``
calls (n ``step()``) on the same commit, and what ``per_turn`` costs alone against ``per_write_back`` + ``per_draw``.

  lunar      fc, obs 8, [100, 100], A = 4, K = 3, B = 32 (the LunarLander experiment)
  fc_520     fc, obs 8, [520], A = 4, K = 3, B = 32
  atari_b32  cnn, (84, 84, 4), [32, 64, 64, 512], A = 6, K = 5, B = 32 (plane path)

``--leg steps:<config>`` (one process): two learners of the same seeds; for every n in 1, 2, 5, 10, 32 regions of about
``--steps`` gradient steps alternate between ``steps(n)`` and n x ``step()``, ``--rounds`` times after a warm-up region each, timed
on the host clock with a device synchronisation at both ends; us per gradient step.  ``--leg kernels``: ``per_turn`` against
``per_write_back`` + ``per_draw`` at n = 32 and 256 on a 2^20-leaf tree, regions of ``--steps`` turns between two events.
Without ``--leg`` this is the driver: every leg in a fresh process under its own time limit, nothing started after a failure;
per measurement the median and [min, max] over the regions, and per config and n the decision rule of the README -- the call
is the default where its median lies below the chain's minimum.  Writes ``profiles/per_steps.json``.
Usage: ``python tools/bench_per_steps.py [--out profiles/per_steps.json]``.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
NS = (1, 2, 5, 10, 32)
CONFIGS = {  # name: (arch, frame shape, dtype, stack, obs, A, K, features, B)
    "lunar": ("fc", (8,), "float32", 1, 8, 4, 3, [100, 100], 32),
    "fc_520": ("fc", (8,), "float32", 1, 8, 4, 3, [520], 32),
    "atari_b32": ("cnn", (84, 84), "uint8", 4, (84, 84, 4), 6, 5, [32, 64, 64, 512], 32),
}


def steps_leg(name, steps, rounds):
    import numpy as np
    import torch

    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement

    arch, shape, dtype, stack, obs, A, K, feats, B = CONFIGS[name]

    def side():
        rb = ReplayBuffer(SlotPrioritizedSampler(0, 2000), batch_size=B, max_capacity=2000, stack_size=stack, update_horizon=1, gamma=0.99)
        rng = np.random.default_rng(1)
        for i in range(2500):
            frame = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == "uint8" else rng.standard_normal(shape).astype(np.float32)
            rb.add(TransitionElement(frame, int(rng.integers(A)), float(rng.normal()), i % 200 == 199, i % 200 == 199))
        rb.reuse_sample_buffers = True
        learner = PrioritizedLearner(iDQN(0, obs, A, K, feats, arch, 3e-4, 0.99, 1, 1, 10**9, 10**9), rb, beta=0.4, eps=1e-3, reduce="mean")
        # the routes themselves, whatever defaults the families have been given
        learner.fuse_per_family = dict.fromkeys(learner.fuse_per_family, True)
        learner.fuse_per_steps_family = dict.fromkeys(learner.fuse_per_steps_family, True)
        learner.per_steps_min = 1
        return learner

    call, chain = side(), side()

    def run_call(n):
        call.steps(n)

    def run_chain(n):
        for _ in range(n):
            chain.step()

    def region(fn, n):
        reps = max(1, steps // n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(n)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / (reps * n)

    out = {}
    for n in NS:
        region(run_call, n), region(run_chain, n)
        assert call.__dict__.get("_steps_ok") is True and chain.__dict__.get("_steps_ok") is None, "the wrong route ran"
        for a in ("_online", "_mu", "_nu"):  # the same steps on both sides, bit for bit
            assert torch.equal(getattr(call.agent, a), getattr(chain.agent, a)), a
        assert torch.equal(call.sampler._sum_tree._nodes_dev, chain.sampler._sum_tree._nodes_dev)
        reg = {"call": [], "chain": []}
        for _ in range(rounds):
            reg["call"].append(region(run_call, n))
            reg["chain"].append(region(run_chain, n))
        out[f"n{n}"] = reg
    print("RESULT" + json.dumps({"leg": "steps", "config": name, "regions": out}), flush=True)


def kernels_leg(steps, rounds):
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
        leaves = torch.from_numpy(rng.integers(0, cap, n).astype(np.int32)).cuda()
        nxt = torch.zeros(n, dtype=torch.int32, device="cuda")
        w = torch.zeros(n, dtype=torch.float32, device="cuda")
        td = torch.from_numpy(rng.random((5, n)).astype(np.float32)).cuda()
        pri = torch.zeros(n, dtype=torch.float64, device="cuda")
        mx = torch.ones(1, dtype=torch.float64, device="cuda")

        def pair():
            lib.per_write_back(nodes, depth, _hip.ptr(leaves), _hip.ptr(td), 5, n, 0, 1e-3, 0.6, _hip.ptr(pri), _hip.ptr(mx), scratch, q)
            lib.per_draw(nodes, depth, _hip.ptr(u), n, 1, cap, 0.4, _hip.ptr(nxt), _hip.ptr(w), q)

        def turn():
            lib.per_turn(nodes, depth, _hip.ptr(leaves), _hip.ptr(td), 5, n, 0, 1e-3, 0.6, _hip.ptr(pri), _hip.ptr(mx), scratch, _hip.ptr(u), 1,
                         cap, 0.4, _hip.ptr(nxt), _hip.ptr(w), q)

        def region(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / steps

        fns = {"write_back_then_draw": pair, "per_turn": turn}
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
    def run(leg):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--leg", leg, "--steps", str(a.steps), "--rounds", str(a.rounds)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
        if out.returncode or not line:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"leg {leg} failed with status {out.returncode}: nothing more is started")
        return json.loads(line[0][6:])

    res = {"method": {"steps_per_region": a.steps, "rounds": a.rounds, "unit": "us per gradient step", "rule": "call median < chain minimum"},
           "steps_us": {}}
    for name in CONFIGS:
        rows = {}
        for n, r in run(f"steps:{name}")["regions"].items():
            row = {"call": summary(r["call"]), "chain": summary(r["chain"])}
            row["call_is_default"] = row["call"]["median"] < row["chain"]["min"]  # the decision rule
            row["chain_over_call"] = row["chain"]["median"] / row["call"]["median"]
            rows[n] = row
        res["steps_us"][name] = rows
        print(name, json.dumps(rows), flush=True)
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
    ap.add_argument("--steps", type=int, default=320)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_steps.json"))
    a = ap.parse_args()
    if a.leg is None:
        return driver(a)
    kind, _, rest = a.leg.partition(":")
    return steps_leg(rest, a.steps, a.rounds) if kind == "steps" else kernels_leg(a.steps, a.rounds)


if __name__ == "__main__":
    main()
