"""Times the impala learner step (csrc/impala_kernels.h) beside the 16-thread float32 torch-CPU restatement of the same net on the
same box, and writes profiles/impala.json.  bench.py is not involved: its headline run is "no change claimed" for this path.

    python tools/bench_impala.py [--regions 5] [--steps 10] [--out profiles/impala.json]

Per configuration: ms per step as median [min, max] over alternating regions (HIP region, CPU region, HIP region, ...), each HIP
region `steps` steps between two stream synchronisations after a warm-up region; the per-launch table of idqn_profile_table from
separate IDQN_F_PROFILE_ALL steps.  The pool backward recomputes its argmax from Conv_0's output; a stored-byte variant was not
built, so no A/B stands behind that choice.
"""
import argparse
import ctypes as C
import json
import os
import statistics
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


def main():
    import numpy as np
    import torch

    from oracle import qnet_ref as Q
    from oracle import torch_ref as T
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impala.json"))
    args = ap.parse_args()
    torch.set_num_threads(16)
    result = {"what": "impala learner step, ms per step, median [min, max] of alternating regions", "bench_py_headline": "no change claimed",
              "pool_backward_argmax": "recomputed from c0; no A/B against a stored byte was run", "cpu_threads": 16, "configs": {}}
    for name, (obs, feats, A, K, B) in CONFIGS.items():
        p = Q.init_params(0, "impala", obs, A, feats, K)
        pt = Q.init_params(1, "impala", obs, A, feats, K)
        batch = Q.synthetic_batch(2, B, obs, A, "cnn")
        agent = iDQN(0, obs, A, K, feats, "impala", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
        agent._load_flat(agent._online, p)
        agent._load_flat(agent._target, pt)
        dev = Batch(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch])

        def hip_region(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                agent._learn(dev)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def cpu_region(n):
            t0 = time.perf_counter()
            for _ in range(n):
                for k in range(K):
                    T.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "impala", 0.99, dtype=torch.float32)
            return (time.perf_counter() - t0) * 1e3 / n

        hip_region(3)
        cpu_region(1)
        hip, cpu = [], []
        for _ in range(args.regions):
            hip.append(hip_region(args.steps))
            cpu.append(cpu_region(1))
        for _ in range(3):
            agent._learn(dev, flags=_hip.F_PROFILE_ALL)
        torch.cuda.synchronize()
        table = C.create_string_buffer(1 << 16)
        _hip.check(_hip.lib().idqn_profile_table(agent._handle, table, len(table)), "idqn_profile_table")
        stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
        result["configs"][name] = {"obs": obs, "features": feats, "A": A, "K": K, "B": B, "hip_ms_per_step": stat(hip),
                                   "cpu_f32_torch_ms_per_step": stat(cpu), "cpu_over_hip": statistics.median(cpu) / statistics.median(hip),
                                   "launches": table.value.decode(errors="replace").splitlines()}
        print(name, result["configs"][name]["hip_ms_per_step"], result["configs"][name]["cpu_f32_torch_ms_per_step"], flush=True)
        del agent
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({n: c["cpu_over_hip"] for n, c in result["configs"].items()}))


if __name__ == "__main__":
    main()
