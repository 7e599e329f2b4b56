"""A/B of the impala matrix-core conv mode (IDQN_IMP_CONV=bf16x3, csrc/impala_mx_kernels.h); writes profiles/impala_mx.json.

    python tools/bench_impala_mx.py --parent-lib <libidqn_hip.so of the parent commit> [--regions 5] [--steps 10] [--out ...]

Three legs, each a child process of its own that lives for the whole run (a library is loaded once per process, and the mode is
read when a handle is created): ``parent`` = the parent commit's library (built into a second directory, passed with
--parent-lib, loaded through IDQN_HIP_LIB), ``off`` = this tree's library with the variable unset, ``on`` = this tree's
library with IDQN_IMP_CONV=bf16x3.  Per configuration of tools/bench_impala.py the learner step is timed in alternating
regions (parent, off, on, parent, ...), each ``steps`` steps between two stream synchronisations after a warm-up region:
ms per step as median [min, max].  The yardstick is the parent's leg; ``off`` only shows that the old path did not move.  A
gain is claimed only where the mode-on median lies below the parent's minimum; otherwise the verdict is SLOWER or "inside the
spread".  Also: the per-launch table of the mode-on (and mode-off) step from idqn_profile_table, and us per call of
idqn_act_host and idqn_act_host_many_impala at n = 1, 8, 32 with the mode on against off (workload configuration).
bench.py is not involved.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]

CONFIGS = {
    "workload": ((84, 84, 4), [32, 64, 64, 512], 6, 5, 32),
    "reference_test": ((84, 84, 4), [3, 7, 5, 9], 4, 2, 32),
}
Batch = namedtuple("Batch", "state action reward next_state is_terminal")


def child():
    """One leg: answers ``region <config> <steps>``, ``table <config>``, ``act <calls>`` and ``quit`` on stdin, one JSON line each."""
    import numpy as np
    import torch

    from oracle import qnet_ref as Q
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    agents = {}

    def get(name):
        if name not in agents:
            obs, feats, A, K, B = CONFIGS[name]
            agent = iDQN(0, obs, A, K, feats, "impala", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
            agent._load_flat(agent._online, Q.init_params(0, "impala", obs, A, feats, K))
            agent._load_flat(agent._target, Q.init_params(1, "impala", obs, A, feats, K))
            batch = Q.synthetic_batch(2, B, obs, A, "cnn")
            agents[name] = (agent, Batch(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch]), batch)
        return agents[name]

    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "region":
            agent, dev, _ = get(cmd[1])
            n = int(cmd[2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                agent._learn(dev)
            torch.cuda.synchronize()
            out = (time.perf_counter() - t0) * 1e3 / n
        elif cmd[0] == "table":
            agent, dev, _ = get(cmd[1])
            for _ in range(3):
                agent._learn(dev, flags=_hip.F_PROFILE_ALL)
            torch.cuda.synchronize()
            table = C.create_string_buffer(1 << 16)
            _hip.check(_hip.lib().idqn_profile_table(agent._handle, table, len(table)), "idqn_profile_table")
            out = table.value.decode(errors="replace").splitlines()
        elif cmd[0] == "act":
            agent, _, batch = get("workload")
            calls, K = int(cmd[1]), CONFIGS["workload"][3]
            states = [np.asarray(s) for s in batch[0]]
            agent.act_many_imp_sizes = (1, 8, 32)
            out = {}
            for label, n in (("act_host", 0), ("many_1", 1), ("many_8", 8), ("many_32", 32)):
                run = (lambda: agent._best_action(0, 1, states[0]).item()) if n == 0 else \
                      (lambda: agent._best_actions(0, [e % K for e in range(n)], states[:n]))
                for _ in range(5):
                    run()
                regions = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        run()
                    regions.append((time.perf_counter() - t0) * 1e6 / calls)
                out[label + "_us_per_call"] = {"median": statistics.median(regions), "min": min(regions), "max": max(regions)}
            assert agent.__dict__.get("_act_many_imp_ok") is True
        print("RESULT" + json.dumps(out), flush=True)


def ask(proc, text):
    proc.stdin.write(text + "\n")
    proc.stdin.flush()
    while True:
        line = proc.stdout.readline()
        if not line:
            raise RuntimeError("a leg ended: rc %s" % proc.poll())
        if line.startswith("RESULT"):
            return json.loads(line[len("RESULT"):])


def verdict(on, parent):
    if on["median"] < parent["min"]:
        return "FASTER: the mode-on median lies below the parent's minimum (%.2fx on the medians)" % (parent["median"] / on["median"])
    if on["median"] > parent["max"]:
        return "SLOWER: the mode-on median lies above the parent's maximum (%.2fx on the medians)" % (on["median"] / parent["median"])
    return "inside the spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--act-calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impala_mx.json"))
    args = ap.parse_args()
    if args.leg:
        return child()
    assert args.regions >= 5
    legs = {}
    envs = {"off": {}, "on": {"IDQN_IMP_CONV": "bf16x3"}}
    if args.parent_lib:
        envs = {"parent": {"IDQN_HIP_LIB": os.path.abspath(args.parent_lib)}, **envs}
    for leg, extra in envs.items():
        env = {k: v for k, v in os.environ.items() if k not in ("IDQN_IMP_CONV", "IDQN_HIP_LIB")}
        env.update(extra)
        legs[leg] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--leg"], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                     text=True)
    result = {"what": "impala learner step, ms per step, median [min, max] of alternating regions (parent, off, on, parent, ...)",
              "legs": {"parent": "the parent commit's library" if args.parent_lib else "NOT RUN: no --parent-lib", "off": "this tree, IDQN_IMP_CONV unset",
                       "on": "this tree, IDQN_IMP_CONV=bf16x3"},
              "regions": args.regions, "steps_per_region": args.steps, "configs": {}}
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    try:
        for name, (obs, feats, A, K, B) in CONFIGS.items():
            ms = {leg: [] for leg in legs}
            for leg, p in legs.items():
                ask(p, "region %s 3" % name)  # warm-up
            for _ in range(args.regions):
                for leg, p in legs.items():
                    ms[leg].append(ask(p, "region %s %d" % (name, args.steps)))
            row = {"obs": obs, "features": feats, "A": A, "K": K, "B": B, "ms_per_step": {leg: stat(v) for leg, v in ms.items()}}
            yard = "parent" if "parent" in legs else "off"
            row["yardstick"] = yard
            row["verdict"] = verdict(row["ms_per_step"]["on"], row["ms_per_step"][yard])
            row["launches_on"] = ask(legs["on"], "table %s" % name)
            row["launches_off"] = ask(legs["off"], "table %s" % name)
            result["configs"][name] = row
            print(name, json.dumps(row["ms_per_step"]), row["verdict"], flush=True)
        result["acting_workload"] = {leg: ask(legs[leg], "act %d" % args.act_calls) for leg in ("off", "on")}
        print("acting", json.dumps(result["acting_workload"]), flush=True)
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
