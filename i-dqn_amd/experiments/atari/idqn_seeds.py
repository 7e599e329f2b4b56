"""`python experiments/atari/idqn_seeds.py -en NAME --first_seed A --last_seed B ...` -- the seeds A .. B of
`experiments/atari/idqn.py` in ONE process (the reference's `launch_job/atari/train.sh` starts one process per seed): the
greedy states of all seeds go through one acting call per step (`AgentGroup.best_actions` -> `idqn_act_group_host`, at the
sizes in `AgentGroup.act_group_sizes`) and their replay adds through one collector call; every seed's learner step is its own
plane-path step, which fills the chip alone (experiments/base/seeds.py).  Every other flag is the single-seed entry point's,
unchanged; `-s` is set per seed.  ``envs`` defaults to the synthetic stand-in environment.
`--n_envs E` (default 1) gives every seed E environments and a `VectorReplayBuffer`: S x E time lines per lock-step iteration
(`SeedVectorTrainer`), the S x E greedy states in chunks of at most 32; ``envs`` is then a list of E environments per seed."""
import argparse
import os
import sys

from experiments.base.launch import ENVIRONMENTS, default_environment, make_agent, observation_dim
from experiments.base.seeds import SeedTrainer, train_seeds_vector
from experiments.base.utils import prepare_logs, save_data
from slimdqn import prng
from slimdqn.sample_collection.replay_buffer import ReplayBuffer
from slimdqn.sample_collection.samplers import UniformSamplingDistribution
from slimdqn.sample_collection.vector_replay_buffer import MAX_ENVS, VectorReplayBuffer


def run(argvs=sys.argv[1:], envs=None, save_root=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--first_seed", type=int, required=True)
    ap.add_argument("--last_seed", type=int, required=True)
    ap.add_argument("--n_envs", type=int, default=1)
    own, rest = ap.parse_known_args(argvs)
    seeds = list(range(own.first_seed, own.last_seed + 1))
    if not 1 <= len(seeds) <= 32:
        raise SystemExit(f"--first_seed .. --last_seed must name 1..32 seeds, got {len(seeds)}")
    E = own.n_envs
    if not 1 <= E <= MAX_ENVS:
        raise SystemExit(f"--n_envs must be in 1..{MAX_ENVS}, got {E}")
    os.environ.setdefault("IDQN_STEP_GRAPH", "1")  # as experiments/base/launch.py: every seed steps the same buffer sets over and over
    consts = ENVIRONMENTS["atari"]
    ps, keys, agents, rbs = [], [], [], []
    if envs is not None:
        envs = list(envs)
    elif E == 1:
        envs = [default_environment("atari", s) for s in seeds]
    else:  # environment e of seed s: a stream of its own
        envs = [[default_environment("atari", 1000 * e + s) for e in range(E)] for s in seeds]
    for seed, env in zip(seeds, envs):  # the wiring of experiments/base/launch.py, per seed
        p = prepare_logs("atari", "idqn", list(rest) + ["-s", str(seed)], save_root)
        agent_key, train_key = prng.split(prng.PRNGKey(p["seed"]))
        shared = dict(batch_size=p["batch_size"], max_capacity=p["replay_buffer_capacity"], stack_size=consts["stack_size"],
                      update_horizon=p["update_horizon"], gamma=p["gamma"], clipping=consts["clipping"], compress=True)
        sampler = UniformSamplingDistribution(p["seed"])
        rb = ReplayBuffer(sampler, **shared) if E == 1 else VectorReplayBuffer(sampler, n_envs=E, **shared)
        rb.reuse_sample_buffers = True
        env0 = env if E == 1 else env[0]
        agents.append(make_agent("idqn", agent_key, observation_dim("atari", env0), env0.n_actions, p, consts["adam_eps"]))
        ps.append(p), keys.append(train_key), rbs.append(rb)
    if E == 1:
        SeedTrainer(keys, ps, agents, envs, rbs, save_data).run()
    else:
        train_seeds_vector(keys, ps, agents, envs, rbs, save_fn=save_data)
    return ps, agents


if __name__ == "__main__":
    run()
