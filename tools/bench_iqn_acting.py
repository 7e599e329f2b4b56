"""What one greedy i-IQN action costs: ``iIQN.best_action(host state)`` through ``.item()`` on the single-state path
(``idqn_iqn_act_host``, csrc/iqn_act_kernels.h) against a checkout of the PARENT commit (``--parent ROOT``, built), whose
``best_action`` runs the batched route (``idqn_iqn_q_values``) -- K = 5, A = 6, [32, 64, 64, 512], 84 x 84 x 4, N = 32 / 64.

  (a) median wall time per action, in regions of ``--calls`` calls; parent and this tree run in alternating child processes
      (process-level interleaving: both see the same clocks), the spread is the range of the region medians;
  (b) ``iDQN``'s ``idqn_act_host`` time in the same run, and the per-launch durations of the new chain from a
      ``rocprofv3 --kernel-trace --stats`` run of its own; beside the Dense_0 kernel's time, the time its W0 + We stream
      would take at the copy rate DESIGN quotes (6.2 TB/s) -- the floor it is judged against;
  (c) the Atari-shaped synthetic i-IQN trainer loop in env-steps/s, parent against this tree, alternating.
The driver never opens the GPU; every child runs under its own ``timeout`` and the driver stops at the first that fails.
Usage: ``python tools/bench_iqn_acting.py --parent ROOT [--out profiles/iiqn_acting.json] [--rounds 3] [--loop-steps 3000]``.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS, A, FEATS, K = (84, 84, 4), 6, [32, 64, 64, 512], 5


def _child_act(root, algo, N, regions, calls):
    sys.path[:0] = [root, os.path.join(root, "i-dqn_amd")]
    import numpy as np

    if algo == "iiqn":
        from slimdqn.networks.iiqn import iIQN

        agent = iIQN(0, OBS, A, K, FEATS, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
    else:
        from slimdqn.networks.idqn import iDQN

        agent = iDQN(0, OBS, A, K, FEATS, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
    rng = np.random.default_rng(0)
    states = [rng.integers(0, 256, size=OBS, dtype=np.uint8) for _ in range(8)]
    for i in range(50):
        agent.best_action(agent.params, states[i % 8], i).item()
    med = []
    for r in range(regions):
        ts = []
        for i in range(calls):
            t0 = time.perf_counter()
            agent.best_action(agent.params, states[i % 8], 1000 * r + i).item()
            ts.append(time.perf_counter() - t0)
        med.append(1e6 * float(np.median(ts)))
    print("RESULT" + json.dumps(med))


def _child_loop(root, steps):
    sys.path[:0] = [root, os.path.join(root, "i-dqn_amd")]
    from experiments.atari.iiqn import run

    argv = ["-en", "b", "-s", "1", "-ne", "1", "-ntspe", str(steps), "-nis", "200", "-rbc", "4000", "-nn", str(K), "-at", "cnn",
            "-tuf", "200", "-tsf", "50", "-f"] + [str(f) for f in FEATS] + ["-horizon", "500", "-bs", "32", "-nq", "32", "-ed", "500"]
    t0 = time.perf_counter()
    run(argv, save_root=tempfile.mkdtemp())
    print("RESULT" + json.dumps(steps / (time.perf_counter() - t0)))


def _spawn(args, limit, prefix=()):
    env = dict(os.environ)
    env.pop("IDQN_HIP_LIB", None)  # every tree loads the library it was built with
    out = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__)] + args,
                         capture_output=True, text=True, env=env)
    if out.returncode != 0:
        sys.exit(f"child {args} ended with {out.returncode}:\n{out.stderr[-1500:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit, built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iiqn_acting.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--loop-steps", type=int, default=3000)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "act":
            return _child_act(a.child[1], a.child[2], int(a.child[3]), a.regions, a.calls)
        return _child_loop(a.child[1], int(a.child[2]))
    import numpy as np

    trees = {"new": ROOT}
    if a.parent:
        trees["parent"] = os.path.abspath(a.parent)
    common = ["--regions", str(a.regions), "--calls", str(a.calls)]
    res = {"config": {"K": K, "A": A, "features": FEATS, "obs": OBS, "regions": a.regions, "calls": a.calls, "rounds": a.rounds},
           "acting_us": {}, "loop_env_steps_per_s": {}}
    for N in (32, 64):
        reg = {t: [] for t in trees}
        for _ in range(a.rounds):
            for t, root in trees.items():
                reg[t] += _spawn(common + ["--child", "act", root, "iiqn", str(N)], a.limit)
        res["acting_us"][f"N{N}"] = {t: {"median": float(np.median(v)), "min": min(v), "max": max(v), "regions": v} for t, v in reg.items()}
        print(json.dumps({f"N{N}": {t: res["acting_us"][f"N{N}"][t]["median"] for t in trees}}), flush=True)
    v = _spawn(common + ["--child", "act", ROOT, "idqn", "0"], a.limit)
    res["acting_us"]["idqn_act_host"] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "regions": v}
    # (b) the chain's launches, in a traced run of its own
    rocprof = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    for N in (32, 64):
        d = tempfile.mkdtemp()
        _spawn(["--regions", "2", "--calls", "200", "--child", "act", ROOT, "iiqn", str(N)], a.limit,
               prefix=[rocprof, "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--"])
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            import csv

            for row in csv.DictReader(open(f)):
                name = row["Name"].split("(")[0]
                if "k_iqn_act" in name or "k_act_conv" in name:
                    rows[name] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3}
        res[f"kernels_N{N}"] = rows
    n_feat = -(-OBS[0] // 8) * -(-OBS[1] // 8) * FEATS[2]  # SAME convs of stride 4, 2, 1: 84 -> 21 -> 11 -> 11
    stream_mb = (n_feat * FEATS[3] + 64 * n_feat) * 4 / 1e6  # Dense_0/kernel + Embed_0/kernel
    res["dense0_floor"] = {"stream_MB": stream_mb, "us_at_6.2TBps": stream_mb / 6.2}
    # (c) the trainer loop
    loops = {t: [] for t in trees}
    for _ in range(2):
        for t, root in trees.items():
            loops[t].append(_spawn(["--child", "loop", root, str(a.loop_steps)], 2 * a.limit))
    res["loop_env_steps_per_s"] = {t: {"median": float(np.median(v)), "runs": v} for t, v in loops.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"acting_us": {k: {t: x["median"] for t, x in v.items()} if "median" not in v else v["median"]
                                    for k, v in res["acting_us"].items()}, "loop": res["loop_env_steps_per_s"]}))


if __name__ == "__main__":
    main()
