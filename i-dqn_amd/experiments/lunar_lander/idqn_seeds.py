"""`python experiments/lunar_lander/idqn_seeds.py -en NAME --first_seed A --last_seed B ...` -- the seeds A .. B of
`experiments/lunar_lander/idqn.py` in ONE process (the reference's `launch_job/lunar_lander/train.sh` starts one process per
seed): one acting call and one learner call per step for all of them (experiments/base/seeds.py).  Every other flag is the
single-seed entry point's, unchanged; `-s` is set per seed.  ``envs`` defaults to the synthetic stand-in environment."""
import argparse
import sys

from experiments.base.launch import ENVIRONMENTS, default_environment, make_agent, observation_dim
from experiments.base.seeds import train_seeds
from experiments.base.utils import prepare_logs, save_data
from slimdqn import prng
from slimdqn.sample_collection.replay_buffer import ReplayBuffer
from slimdqn.sample_collection.samplers import UniformSamplingDistribution


def run(argvs=sys.argv[1:], envs=None, save_root=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--first_seed", type=int, required=True)
    ap.add_argument("--last_seed", type=int, required=True)
    own, rest = ap.parse_known_args(argvs)
    seeds = list(range(own.first_seed, own.last_seed + 1))
    if not 1 <= len(seeds) <= 32:
        raise SystemExit(f"--first_seed .. --last_seed must name 1..32 seeds, got {len(seeds)}")
    consts = ENVIRONMENTS["lunar_lander"]
    ps, keys, agents, rbs = [], [], [], []
    envs = list(envs) if envs is not None else [default_environment("lunar_lander", s) for s in seeds]
    for seed, env in zip(seeds, envs):  # the wiring of experiments/base/launch.py, per seed
        p = prepare_logs("lunar_lander", "idqn", list(rest) + ["-s", str(seed)], save_root)
        agent_key, train_key = prng.split(prng.PRNGKey(p["seed"]))
        rb = ReplayBuffer(UniformSamplingDistribution(p["seed"]), batch_size=p["batch_size"], max_capacity=p["replay_buffer_capacity"],
                          stack_size=consts["stack_size"], update_horizon=p["update_horizon"], gamma=p["gamma"],
                          clipping=consts["clipping"], compress=True)
        rb.reuse_sample_buffers = True
        agents.append(make_agent("idqn", agent_key, observation_dim("lunar_lander", env), env.n_actions, p, consts["adam_eps"]))
        ps.append(p), keys.append(train_key), rbs.append(rb)
    train_seeds(keys, ps, agents, envs, rbs, save_fn=save_data)
    return ps, agents


if __name__ == "__main__":
    run()
