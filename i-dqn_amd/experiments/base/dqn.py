"""Trainer loop of the HIP build.

Interface and event order follow the reference's ``experiments/base/dqn.py:12-69`` -- per environment step: split the
key, collect one sample, and once ``n_initial_samples`` are in, ``update_online_params`` then
``update_target_params``; a log record on every target update and at every epoch end; the model saved per epoch -- but
the loop is organised as a small state machine (``EpochStats`` + ``Trainer``) instead of one nested loop.

``p["wandb"]`` only needs ``.log(dict)``; ``experiments.base.utils.NullLogger`` stands in when wandb is absent.
"""
import numpy as np

from slimdqn import prng
from slimdqn.sample_collection.utils import collect_single_sample, linear_schedule


class EpochStats:
    """Returns and lengths of the episodes of one epoch; the last entry is the episode in progress."""

    def __init__(self):
        self.returns, self.lengths = [0], [0]

    def record(self, reward):
        self.returns[-1] += reward
        self.lengths[-1] += 1

    def open_episode(self):
        self.returns.append(0)
        self.lengths.append(0)

    def summary(self):
        return float(np.mean(self.returns)), float(np.mean(self.lengths)), len(self.lengths)


class Trainer:
    def __init__(self, key, p, agent, env, rb, save_fn=None):
        self.key, self.p, self.agent, self.env, self.rb, self.save_fn = key, p, agent, env, rb, save_fn
        self.epsilon = linear_schedule(1.0, p["epsilon_end"], p["epsilon_duration"])
        self.total_steps = 0
        self.history = []  # one EpochStats per epoch

    def _environment_step(self):
        self.key, explore_key = prng.split(self.key)
        return collect_single_sample(explore_key, self.env, self.agent, self.rb, self.p, self.epsilon, self.total_steps)

    def _gradient_step(self):
        self.agent.update_online_params(self.total_steps, self.rb)
        updated, logs = self.agent.update_target_params(self.total_steps)
        if updated:
            self.p["wandb"].log({"n_training_steps": self.total_steps, **logs})

    def run_epoch(self, index):
        stats, budget, done, just_reset = EpochStats(), self.p["n_training_steps_per_epoch"], 0, False
        self.history.append(stats)
        # an epoch always ends on an episode boundary (experiments/base/dqn.py:29)
        while done < budget or not just_reset:
            reward, just_reset = self._environment_step()
            done += 1
            self.total_steps += 1
            stats.record(reward)
            if just_reset and done < budget:
                stats.open_episode()
            if self.total_steps > self.p["n_initial_samples"]:
                self._gradient_step()
        if hasattr(self.rb, "flush_deferred"):
            self.rb.flush_deferred()  # (a postponed add of the last step: the buffer is complete at every epoch end)
        avg_return, avg_length, n_episodes = stats.summary()
        print(f"\nEpoch {index}: Return {avg_return} averaged on {n_episodes} episodes.\n", flush=True)
        self.p["wandb"].log({"epoch": index, "n_training_steps": self.total_steps, "avg_return": avg_return,
                             "avg_length_episode": avg_length})
        if self.save_fn is not None:
            self.save_fn(self.p, [s.returns for s in self.history], [s.lengths for s in self.history],
                         self.agent.get_model())

    def run(self):
        self.env.reset()
        for index in range(self.p["n_epochs"]):
            self.run_epoch(index)
        return [s.returns for s in self.history], [s.lengths for s in self.history]


def train(key, p: dict, agent, env, rb, save_fn=None):
    """Same call as the reference's ``train`` (``experiments/base/dqn.py:12``); returns (returns, lengths) per epoch."""
    return Trainer(key, p, agent, env, rb, save_fn).run()


from slimdqn.sample_collection.utils import collect_vector_samples  # noqa: E402


class VectorTrainer:
    """``Trainer`` over a list of E environments stepped together: one vectorised acting call and one replay call per
    vector step.  Every environment step still counts as one step of the schedule: ``total_steps`` advances once per
    environment that stepped and ``update_online_params`` / ``update_target_params`` run at every one of those values
    (after ``n_initial_samples``), so the gradient-step and target-update schedule per environment step is the single
    trainer's.  Once an epoch's budget is spent, an environment that ends its episode waits (it is passed to the buffer as
    ``None``) until all have: an epoch ends with every environment on an episode boundary.

    ``learner``: a ``PrioritizedLearner`` on ``agent`` and ``rb`` (slimdqn/sample_collection/per.py).  The gradient step of the
    schedule is then ``learner.step()`` -- the vector step's run of them ``learner.update_params_many`` -- and the target
    operations stay the agent's own."""

    def __init__(self, key, p, agent, envs, rb, save_fn=None, learner=None):
        self.key, self.p, self.agent, self.envs, self.rb, self.save_fn = key, p, agent, list(envs), rb, save_fn
        self.learner = learner
        self.epsilon = linear_schedule(1.0, p["epsilon_end"], p["epsilon_duration"])
        self.total_steps = 0
        self.history = []  # one list of per-environment EpochStats per epoch

    def _environment_step(self, active):
        keys = []
        for _ in range(sum(active)):  # the key is split once per environment that steps
            self.key, explore_key = prng.split(self.key)
            keys.append(explore_key)
        return collect_vector_samples(keys, self.envs, self.agent, self.rb, self.p, self.epsilon, self.total_steps, active)

    def _gradient_step(self):
        if self.learner is None:
            self.agent.update_online_params(self.total_steps, self.rb)
        elif self.total_steps % self.agent.update_to_data == 0:
            self.learner.step()
        updated, logs = self.agent.update_target_params(self.total_steps)
        if updated:
            self.p["wandb"].log({"n_training_steps": self.total_steps, **logs})

    def _update_params_many(self, first, n_steps):
        if self.learner is not None:
            return self.learner.update_params_many(first, n_steps)
        return self.agent.update_params_many(first, n_steps, self.rb)

    def run_epoch(self, index):
        n_envs, budget, done = len(self.envs), self.p["n_training_steps_per_epoch"], 0
        stats, active = [EpochStats() for _ in range(n_envs)], [True] * n_envs
        self.history.append(stats)
        while any(active):
            rewards, ended = self._environment_step(active)
            stepped = sum(active)
            done += stepped
            for i in range(n_envs):
                if not active[i]:
                    continue
                stats[i].record(rewards[i])
                if ended[i]:
                    if done < budget:
                        stats[i].open_episode()
                    else:
                        active[i] = False
            if (self.learner is not None or hasattr(self.agent, "update_params_many")) and self.p.get("fuse_gradient_steps", True):
                # the vector step's gradient steps as one call; a target update's record follows the run that call closes
                first = max(self.total_steps, self.p["n_initial_samples"]) + 1
                self.total_steps += stepped
                if self.total_steps >= first:
                    for step, logs in self._update_params_many(first, self.total_steps - first + 1):
                        self.p["wandb"].log({"n_training_steps": step, **logs})
            else:
                for _ in range(stepped):
                    self.total_steps += 1
                    if self.total_steps > self.p["n_initial_samples"]:
                        self._gradient_step()
        if hasattr(self.rb, "flush_deferred"):
            self.rb.flush_deferred()
        returns, lengths = [r for s in stats for r in s.returns], [n for s in stats for n in s.lengths]
        avg_return, avg_length = float(np.mean(returns)), float(np.mean(lengths))
        print(f"\nEpoch {index}: Return {avg_return} averaged on {len(lengths)} episodes.\n", flush=True)
        self.p["wandb"].log({"epoch": index, "n_training_steps": self.total_steps, "avg_return": avg_return,
                             "avg_length_episode": avg_length})
        if self.save_fn is not None:
            self.save_fn(self.p, self._per_epoch("returns"), self._per_epoch("lengths"), self.agent.get_model())

    def _per_epoch(self, field):
        return [[x for s in epoch for x in getattr(s, field)] for epoch in self.history]

    def run(self):
        for env in self.envs:
            env.reset()
        for index in range(self.p["n_epochs"]):
            self.run_epoch(index)
        return self._per_epoch("returns"), self._per_epoch("lengths")


def train_vector(key, p: dict, agent, envs, rb, save_fn=None, learner=None):
    """``train`` for a list of environments and a ``VectorReplayBuffer``; returns (returns, lengths) per epoch, the
    environments' episodes concatenated in environment order."""
    return VectorTrainer(key, p, agent, envs, rb, save_fn, learner=learner).run()
