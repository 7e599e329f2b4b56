"""i-IQN step time against the minibatch size: BASELINE config 3 (K = 5, N = 32, A = 6, [32, 64, 64, 512], synthetic Atari
batches) as bench.py's ``iiqn_bench`` times it, for B in {32, 64, 128, 256}.

One JSON line per batch size: ms/step (median of 5 regions), the per-launch table of ``idqn_profile_table`` and the issued
MFMA rate of the Dense_0 GEMMs (six bf16 products per f32 product, against the dense bf16 peak).  bench.py is not touched.
Usage: ``python tools/bench_iiqn_batch.py [--batches 32 64 128 256] [--steps 20] [--warmup 5] [--out FILE]``.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "i-dqn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench import FEATURES, K_HEADS, MFMA_BF16_PEAK, OBS, synthetic  # noqa: E402

Batch = namedtuple("Batch", "state action reward next_state is_terminal")


def run(B, steps, warmup, regions, A=6, N=32):
    import torch

    from slimdqn import _hip
    from slimdqn.networks.iiqn import iIQN

    agent = iIQN(0, OBS, A, K_HEADS, FEATURES, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
    batches = [Batch(*(torch.from_numpy(x).cuda() for x in synthetic(1000 + i, A, B))) for i in range(8)]
    it = [0]

    def step(flags=0):
        agent._learn(batches[it[0] % 8], flags=flags)
        it[0] += 1

    for _ in range(warmup):
        step()
    times = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    for _ in range(10):
        step(_hip.F_PROFILE_ALL)
    torch.cuda.synchronize()
    buf = C.create_string_buffer(8192)
    _hip.check(_hip.lib().idqn_profile_table(agent._handle, buf, 8192), "idqn_profile_table")
    kernels = []
    for ln in buf.value.decode().splitlines():
        nm, us, cnt = ln.split("\t")
        kernels.append({"launch": nm, "us": float(us), "n": int(cnt)})
    losses = agent._losses.cpu().numpy()
    assert np.isfinite(losses).all(), losses
    F, J = 7744, FEATURES[3]  # trunk features of the 84 x 84 x 4 Nature-CNN (as bench.py prices them)
    gemm = 2.0 * K_HEADS * N * B * F * J  # f32-equivalent FLOPs of one Dense_0 contraction over the online nets
    flops = {"iqn dense0 fwd": 3 * gemm, "iqn dense0 dgrad": gemm, "iqn dense0 wgrad": gemm, "iqn dense0 dgrad + wgrad": 2 * gemm,
             "iqn dense0 dgrad + wgrad + adam": 2 * gemm}
    gemm_us = gemm_flops = 0.0
    for kr in kernels:
        if kr["launch"] in flops:
            kr["mfma_issued_tflops"] = 6 * flops[kr["launch"]] / (kr["us"] * 1e-6) / 1e12
            kr["mfma_frac"] = kr["mfma_issued_tflops"] / (MFMA_BF16_PEAK / 1e12)
            gemm_us += kr["us"]
            gemm_flops += flops[kr["launch"]]
    del agent
    torch.cuda.empty_cache()
    return {"batch": B, "ms_per_step": float(np.median(times)), "ms_per_step_all": times, "steps_per_region": steps,
            "regions": regions, "heads": K_HEADS, "quantiles": N, "actions": A, "features": FEATURES,
            "dense0_gemm_us": gemm_us,
            "dense0_gemm_mfma_issued_tflops": 6 * gemm_flops / (gemm_us * 1e-6) / 1e12 if gemm_us else None,
            "dense0_gemm_mfma_frac": 6 * gemm_flops / (gemm_us * 1e-6) / MFMA_BF16_PEAK if gemm_us else None,
            "kernels": kernels, "final_losses": [float(x) for x in losses]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[32, 64, 128, 256])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for B in args.batches:
        rec = run(B, args.steps, args.warmup, args.regions)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
