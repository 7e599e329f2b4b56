"""A/B of the impala matrix-core weight gradient (IDQN_IMP_WGRAD=bf16x3, csrc/impala_mx_wgrad_kernels.h); writes
profiles/impala_mx_wgrad.json.

    python tools/bench_impala_mx_wgrad.py --parent-lib <libidqn_hip.so of the parent commit> [--regions 5] [--steps 10] [--out ...]

The harness of tools/bench_impala_mx.py (its child process, its configurations, its alternating regions): five legs, each a
child process of its own that lives for the whole run -- ``parent_conv`` = the parent commit's library (built into a second
directory, loaded through IDQN_HIP_LIB) with IDQN_IMP_CONV=bf16x3, the yardstick; ``off`` = this tree, both variables unset;
``conv`` = this tree, IDQN_IMP_CONV=bf16x3; ``both`` = this tree, both on; ``wgrad`` = this tree, IDQN_IMP_WGRAD=bf16x3 alone.
ms per learner step as median [min, max] of alternating regions.  Verdicts by the standing rule -- a gain only where the
median lies below the yardstick's minimum, SLOWER in capitals where it lies above its maximum: ``both`` against
``parent_conv``, ``conv`` against ``parent_conv`` (the old path did not move), and ``wgrad`` against ``off`` (this tree's own
legs; the parent has no such leg).  Also the per-launch tables of ``both`` and ``conv`` from idqn_profile_table, whose
averages are per kernel NAME: k_imp_wgrad_mx over its 14 launches against k_imp_wgrad over its 15 (the 42 x 42, 21 x 21 and
11 x 11 layers are not separated by the table).  bench.py is not involved.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd"), os.path.join(ROOT, "tools")]

import bench_impala_mx as H  # noqa: E402  the child process, ask() and the configurations

VARS = ("IDQN_IMP_CONV", "IDQN_IMP_WGRAD", "IDQN_HIP_LIB")
LEGS = {
    "parent_conv": "the parent commit's library, IDQN_IMP_CONV=bf16x3 (the yardstick)",
    "off": "this tree, both variables unset",
    "conv": "this tree, IDQN_IMP_CONV=bf16x3",
    "both": "this tree, IDQN_IMP_CONV=bf16x3 and IDQN_IMP_WGRAD=bf16x3",
    "wgrad": "this tree, IDQN_IMP_WGRAD=bf16x3 alone",
}


def verdict(leg, yard):
    if leg["median"] < yard["min"]:
        return "FASTER: the median lies below the yardstick's minimum (%.3fx on the medians)" % (yard["median"] / leg["median"])
    if leg["median"] > yard["max"]:
        return "SLOWER: the median lies above the yardstick's maximum (%.3fx on the medians)" % (leg["median"] / yard["median"])
    return "inside the spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impala_mx_wgrad.json"))
    args = ap.parse_args()
    assert args.regions >= 5
    envs = {"off": {}, "conv": {"IDQN_IMP_CONV": "bf16x3"}, "both": {"IDQN_IMP_CONV": "bf16x3", "IDQN_IMP_WGRAD": "bf16x3"},
            "wgrad": {"IDQN_IMP_WGRAD": "bf16x3"}}
    if args.parent_lib:
        envs = {"parent_conv": {"IDQN_HIP_LIB": os.path.abspath(args.parent_lib), "IDQN_IMP_CONV": "bf16x3"}, **envs}
    legs = {}
    for leg, extra in envs.items():
        env = {k: v for k, v in os.environ.items() if k not in VARS}
        env.update(extra)
        legs[leg] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "bench_impala_mx.py"), "--leg"], env=env, stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, text=True)
    result = {"what": "impala learner step, ms per step, median [min, max] of alternating regions (" + ", ".join(envs) + ", ...)",
              "legs": {leg: (txt if leg in envs else "NOT RUN: no --parent-lib") for leg, txt in LEGS.items()},
              "regions": args.regions, "steps_per_region": args.steps, "configs": {}}
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    try:
        for name, (obs, feats, A, K, B) in H.CONFIGS.items():
            ms = {leg: [] for leg in legs}
            for leg, p in legs.items():
                H.ask(p, "region %s 3" % name)  # warm-up
            for _ in range(args.regions):
                for leg, p in legs.items():
                    ms[leg].append(H.ask(p, "region %s %d" % (name, args.steps)))
            st = {leg: stat(v) for leg, v in ms.items()}
            yard = "parent_conv" if "parent_conv" in legs else "conv"
            row = {"obs": obs, "features": feats, "A": A, "K": K, "B": B, "ms_per_step": st, "yardstick": yard,
                   "verdict_both": verdict(st["both"], st[yard]), "verdict_conv": verdict(st["conv"], st[yard]),
                   "verdict_wgrad_against_off": verdict(st["wgrad"], st["off"]),
                   "launches_both": H.ask(legs["both"], "table %s" % name), "launches_conv": H.ask(legs["conv"], "table %s" % name)}
            result["configs"][name] = row
            print(name, json.dumps(st), "| both:", row["verdict_both"], "| conv:", row["verdict_conv"], "| wgrad against off:",
                  row["verdict_wgrad_against_off"], flush=True)
            for leg in ("both", "conv"):
                print(name, leg, [ln for ln in row["launches_" + leg] if ln.startswith(("k_imp_wgrad", "k_imp_wreduce"))], flush=True)
    finally:
        for p in legs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
