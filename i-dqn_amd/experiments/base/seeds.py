"""Trainer loop for S seeds at once: the reference starts one process per seed on one device (``launch_job/*/train.sh``); here S
(agent, environment, replay buffer) triples advance in lock step inside one process, with ONE acting call and ONE learner
call per step for all of them (``slimdqn.networks.group.AgentGroup``).

Every triple runs the loop of ``experiments.base.dqn.Trainer`` -- its own key stream, epsilon schedule, epochs that end on its
own episode boundaries, log records and saved model -- so a seed sees what it would see trained alone.  All unfinished seeds
share the step counter (each advances one environment step per iteration); a seed whose last epoch has ended stops stepping,
and from then on the remaining ones are driven through their own agents' calls.
"""
import numpy as np

from experiments.base.dqn import EpochStats
from slimdqn import prng
from slimdqn.networks.group import AgentGroup
from slimdqn.sample_collection.group_replay import GroupCollector, GroupVectorCollector
from slimdqn.sample_collection.replay_buffer import TransitionElement
from slimdqn.sample_collection.utils import _best_actions_fn, linear_schedule, select_actions


class _Seed:
    """The loop state ``Trainer`` keeps, for one triple."""

    def __init__(self, key, p, agent, env, rb):
        self.key, self.p, self.agent, self.env, self.rb = key, p, agent, env, rb
        self.epsilon = linear_schedule(1.0, p["epsilon_end"], p["epsilon_duration"])
        self.history, self.epoch, self.done, self.finished = [], 0, 0, p["n_epochs"] <= 0
        if not self.finished:
            self.history.append(EpochStats())


class SeedTrainer:
    def __init__(self, keys, p, agents, envs, replay_buffers, save_fn=None, group=None, learner=None, collector=None):
        """``learner``: a ``slimdqn.sample_collection.per.PrioritizedGroupLearner`` over the same agents and buffers -- the
        gradient step of a step at which every seed learns is then ``learner.step()`` (one prioritized group call) in place
        of ``group.update_online_params``; where only some seeds learn, their own ``learner.learners[i].step()``.  None: every
        line behaves as without the argument.  ``collector``: a ``slimdqn.sample_collection.group_replay.GroupCollector`` over the
        same buffers (default: one with the measured default sizes) -- the replay adds of an iteration are its ``add_many``."""
        ps = list(p) if isinstance(p, (list, tuple)) else [p] * len(agents)
        assert len(keys) == len(ps) == len(agents) == len(envs) == len(replay_buffers)
        self.seeds = [_Seed(*t) for t in zip(keys, ps, agents, envs, replay_buffers)]
        self.group = group if group is not None else AgentGroup(agents)
        self.learner, self.save_fn, self.total_steps = learner, save_fn, 0
        self.collector = collector if collector is not None else GroupCollector(replay_buffers)

    def _select_actions(self, live):
        """``select_action`` of every live seed on its own key; the greedy ones share one acting call."""
        actions, greedy, greedy_keys = {}, [], []
        for i in live:
            s = self.seeds[i]
            s.key, key = prng.split(s.key)
            explore_key, random_action_key, greedy_key = prng.split(key, 3)
            if prng.uniform(explore_key) <= s.epsilon(self.total_steps):
                actions[i] = prng.randint(random_action_key, 0, s.env.n_actions)
            else:
                greedy.append(i)
                greedy_keys.append(greedy_key)
        if greedy:  # (any subset of the members: the acting call names the member of every state)
            heads = self.group.select_heads(greedy_keys, greedy)
            best = self.group.best_actions(0, heads, [self.seeds[i].env.state for i in greedy], greedy)
            for i, a in zip(greedy, best):
                actions[i] = int(a)
        return actions

    def _environment_steps(self, live):
        observations = {i: self.seeds[i].env.observation for i in live}  # the frame BEFORE the action goes with it
        actions = self._select_actions(live)
        out, transitions = {}, []
        for i in live:
            s = self.seeds[i]
            reward, absorbing = s.env.step(actions[i])
            ended = bool(absorbing) or s.env.n_steps >= s.p["horizon"]
            stored = s.rb._clipping(reward) if s.rb._clipping is not None else reward
            transitions.append(TransitionElement(observations[i], actions[i], stored, absorbing, ended))
            if ended:
                s.env.reset()
            out[i] = (reward, ended)
        # the adds of all live seeds in one go (one call where the collector takes that route, else every buffer's own add);
        # `observations` are the environments' own copies of the frames before the step, which a reset does not touch
        self.collector.add_many(transitions, live)
        return out

    def _gradient_steps(self, live):
        learners = [i for i in live if self.total_steps > self.seeds[i].p["n_initial_samples"]]
        if not learners:
            return
        if len(learners) == len(self.seeds):
            if self.learner is not None:
                self._prioritized_steps(learners)
            else:
                self.group.update_online_params(self.total_steps, [s.rb for s in self.seeds])
            results = self.group.update_target_params(self.total_steps)
        else:
            results = []
            for i in learners:
                s = self.seeds[i]
                if self.learner is not None:
                    self._prioritized_steps([i])
                else:
                    s.agent.update_online_params(self.total_steps, s.rb)
                results.append(s.agent.update_target_params(self.total_steps))
        for i, (updated, logs) in zip(learners, results):
            if updated:
                self.seeds[i].p["wandb"].log({"n_training_steps": self.total_steps, **logs})

    def _prioritized_steps(self, learners):
        """``update_online_params`` of seeds ``learners`` through the prioritized learner: a gradient step where
        ``total_steps % update_to_data == 0`` (``idqn.py:65-66``) -- one group call when that holds for every seed."""
        due = [i for i in learners if self.total_steps % getattr(self.seeds[i].agent, "update_to_data", 1) == 0]
        if len(due) == len(self.seeds):
            self.learner.step()
        else:
            for i in due:
                self.learner.learners[i].step()

    def _end_epoch(self, s):
        if hasattr(s.rb, "flush_deferred"):
            s.rb.flush_deferred()
        avg_return, avg_length, n_episodes = s.history[-1].summary()
        print(f"\nSeed {s.p.get('seed')} epoch {s.epoch}: Return {avg_return} averaged on {n_episodes} episodes.\n", flush=True)
        s.p["wandb"].log({"epoch": s.epoch, "n_training_steps": self.total_steps, "avg_return": avg_return,
                          "avg_length_episode": avg_length})
        if self.save_fn is not None:
            self.save_fn(s.p, [e.returns for e in s.history], [e.lengths for e in s.history], s.agent.get_model())
        s.epoch, s.done = s.epoch + 1, 0
        if s.epoch >= s.p["n_epochs"]:
            s.finished = True
        else:
            s.history.append(EpochStats())

    def run(self):
        for s in self.seeds:
            s.env.reset()
        while True:
            live = [i for i, s in enumerate(self.seeds) if not s.finished]
            if not live:
                break
            stepped = self._environment_steps(live)
            self.total_steps += 1
            closing = []
            for i in live:
                s, (reward, ended) = self.seeds[i], stepped[i]
                s.done += 1
                s.history[-1].record(reward)
                budget = s.p["n_training_steps_per_epoch"]
                if ended and s.done < budget:
                    s.history[-1].open_episode()
                if ended and s.done >= budget:  # an epoch always ends on an episode boundary
                    closing.append(s)
            self._gradient_steps(live)
            for s in closing:
                self._end_epoch(s)
        self.group.close()
        return [([e.returns for e in s.history], [e.lengths for e in s.history]) for s in self.seeds]


def train_seeds(keys, p, agents, envs, replay_buffers, save_fn=None, learner=None):
    """``experiments.base.dqn.train`` for S seeds in one process; returns ``(returns, lengths)`` per epoch, per seed."""
    return SeedTrainer(keys, p, agents, envs, replay_buffers, save_fn, learner=learner).run()


class _VectorSeed:
    """The loop state ``experiments.base.dqn.VectorTrainer`` keeps, for one (agent, environments, buffer) triple."""

    def __init__(self, key, p, agent, envs, rb):
        self.key, self.p, self.agent, self.envs, self.rb = key, p, agent, list(envs), rb
        self.epsilon = linear_schedule(1.0, p["epsilon_end"], p["epsilon_duration"])
        self.total_steps, self.history, self.epoch, self.finished = 0, [], 0, p["n_epochs"] <= 0
        if not self.finished:
            self.open_epoch()

    def open_epoch(self):
        self.stats, self.active, self.done = [EpochStats() for _ in self.envs], [True] * len(self.envs), 0
        self.history.append(self.stats)

    def per_epoch(self, field):
        return [[x for s in epoch for x in getattr(s, field)] for epoch in self.history]

    def fused(self, learner=None):
        return (learner is not None or hasattr(self.agent, "update_params_many")) and self.p.get("fuse_gradient_steps", True)


class SeedVectorTrainer:
    """S seeds x E time lines: every seed runs the loop of ``VectorTrainer`` on its own key stream, step counter, epsilon schedule,
    epoch boundaries, logs and ``save_fn``, and the S vector steps of a lock-step iteration share their device calls -- the
    greedy states of all seeds go through ``AgentGroup.best_actions`` (at most 32 states per call, in (seed, environment)
    order), the S ``add_many`` are ONE ``GroupVectorCollector.add_many``, and where every seed learns over the same run of
    steps the E gradient steps of all of them are ONE ``AgentGroup.update_params_many`` (the persistent group kernel).  A seed
    whose last epoch has ended stops stepping; from then on, and wherever the seeds' runs differ, every seed is driven through
    its own agent.

    ``learner``: a ``slimdqn.sample_collection.per.PrioritizedGroupLearner`` over the same agents (the same ``group``) and
    buffers.  The gradient steps of a run that every seed owes are then ``learner.update_params_many`` (the n-step prioritized
    group call, ``idqn_group_per_learn_steps_on_replay_fc``, where its sizes allow); where the runs differ, every seed's own
    ``learner.learners[i].update_params_many``; the non-fused path steps ``learner.learners[i].step()``.  The target operations
    stay the agents' own.  None: every line behaves as without the argument."""

    def __init__(self, keys, p, agents, envs, replay_buffers, save_fn=None, group=None, collector=None, learner=None):
        ps = list(p) if isinstance(p, (list, tuple)) else [p] * len(agents)
        assert len(keys) == len(ps) == len(agents) == len(envs) == len(replay_buffers)
        self.seeds = [_VectorSeed(*t) for t in zip(keys, ps, agents, envs, replay_buffers)]
        self.group = group if group is not None else AgentGroup(agents)
        self.collector = collector if collector is not None else GroupVectorCollector(replay_buffers)
        self.save_fn, self.learner = save_fn, learner

    def _select_actions(self, live):
        """``select_actions`` of every live seed on its own keys (one split per environment that steps); the greedy states of
        all seeds share the acting calls.  ``{seed: (stepping environments, their actions)}``."""
        # (else -- i-IQN, general-shape cnn or head-parallel members -- every seed's own acting call)
        shared = self.group._stock() or self.group._stock_act_cnn()
        out, greedy = {}, []
        for i in live:
            s = self.seeds[i]
            idx = [e for e, on in enumerate(s.active) if on]
            keys = []
            for _ in idx:
                s.key, explore_key = prng.split(s.key)
                keys.append(explore_key)
            states, n_actions = [s.envs[e].state for e in idx], s.envs[idx[0]].n_actions
            if not shared:
                out[i] = (idx, select_actions(_best_actions_fn(s.agent), s.agent.params, states, keys, n_actions, s.epsilon, s.total_steps))
                continue
            epsilon, actions = s.epsilon(s.total_steps), [None] * len(idx)
            for j, key in enumerate(keys):
                explore_key, random_action_key, greedy_key = prng.split(key, 3)
                if prng.uniform(explore_key) <= epsilon:
                    actions[j] = prng.randint(random_action_key, 0, n_actions)
                else:
                    greedy.append((i, j, greedy_key, states[j]))
            out[i] = (idx, actions)
        for lo in range(0, len(greedy), 32):
            chunk = greedy[lo:lo + 32]
            members = [i for i, _, _, _ in chunk]
            heads = self.group.select_heads([k for _, _, k, _ in chunk], members)
            best = self.group.best_actions(0, heads, [x for _, _, _, x in chunk], members)
            for (i, j, _, _), a in zip(chunk, best):
                out[i][1][j] = int(a)
        return out

    def _environment_steps(self, live):
        """``collect_vector_samples`` of every live seed; ``{seed: (rewards, ended)}``, lists over all its environments."""
        observations = {i: {e: env.observation for e, env in enumerate(self.seeds[i].envs) if self.seeds[i].active[e]} for i in live}
        chosen = self._select_actions(live)
        out, entries = {}, []
        for i in live:
            s, (idx, actions) = self.seeds[i], chosen[i]
            n = len(s.envs)
            rewards, ended, transitions = [None] * n, [False] * n, [None] * n
            for e, action in zip(idx, actions):
                env = s.envs[e]
                reward, absorbing = env.step(int(action))
                ended[e] = bool(absorbing) or env.n_steps >= s.p["horizon"]
                rewards[e] = reward
                stored = s.rb._clipping(reward) if s.rb._clipping is not None else reward
                transitions[e] = TransitionElement(observations[i][e], int(action), stored, absorbing, ended[e])
            entries.append(transitions)
            out[i] = (rewards, ended)
        self.collector.add_many(entries, live)  # (one call where the collector takes that route, else every buffer's own add_many)
        for i in live:
            for e, env in enumerate(self.seeds[i].envs):
                if out[i][1][e]:
                    env.reset()
        return out

    def _gradient_step(self, i):
        s = self.seeds[i]
        if self.learner is None:
            s.agent.update_online_params(s.total_steps, s.rb)
        elif s.total_steps % s.agent.update_to_data == 0:
            self.learner.learners[i].step()
        updated, logs = s.agent.update_target_params(s.total_steps)
        if updated:
            s.p["wandb"].log({"n_training_steps": s.total_steps, **logs})

    def _gradient_runs(self, runs):
        """``runs[seed] = (first step, n steps)``: the gradient steps a vector step owes, as one group call where every seed owes
        the same run."""
        if not runs:
            return
        if len(runs) == len(self.seeds) and len(set(runs.values())) == 1:
            first, n = next(iter(runs.values()))
            if self.learner is not None:
                results = self.learner.update_params_many(first, n)
            else:
                results = self.group.update_params_many(first, n, [s.rb for s in self.seeds])
        elif self.learner is not None:
            results = [self.learner.learners[i].update_params_many(*runs[i]) for i in sorted(runs)]
        else:
            results = [self.seeds[i].agent.update_params_many(*runs[i], self.seeds[i].rb) for i in sorted(runs)]
        for i, result in zip(sorted(runs), results):
            for step, logs in result:
                self.seeds[i].p["wandb"].log({"n_training_steps": step, **logs})

    def _end_epoch(self, s):
        if hasattr(s.rb, "flush_deferred"):
            s.rb.flush_deferred()
        returns, lengths = [r for st in s.stats for r in st.returns], [n for st in s.stats for n in st.lengths]
        avg_return, avg_length = float(np.mean(returns)), float(np.mean(lengths))
        print(f"\nSeed {s.p.get('seed')} epoch {s.epoch}: Return {avg_return} averaged on {len(lengths)} episodes.\n", flush=True)
        s.p["wandb"].log({"epoch": s.epoch, "n_training_steps": s.total_steps, "avg_return": avg_return, "avg_length_episode": avg_length})
        if self.save_fn is not None:
            self.save_fn(s.p, s.per_epoch("returns"), s.per_epoch("lengths"), s.agent.get_model())
        s.epoch += 1
        if s.epoch >= s.p["n_epochs"]:
            s.finished = True
        else:
            s.open_epoch()

    def run(self):
        for s in self.seeds:
            for env in s.envs:
                env.reset()
        while True:
            live = [i for i, s in enumerate(self.seeds) if not s.finished]
            if not live:
                break
            stepped = self._environment_steps(live)
            runs = {}
            for i in live:
                s, (rewards, ended) = self.seeds[i], stepped[i]
                n_stepped, budget = sum(s.active), s.p["n_training_steps_per_epoch"]
                s.done += n_stepped
                for e in range(len(s.envs)):
                    if not s.active[e]:
                        continue
                    s.stats[e].record(rewards[e])
                    if ended[e]:
                        if s.done < budget:
                            s.stats[e].open_episode()
                        else:  # the budget is spent: this environment waits for the others' episode ends
                            s.active[e] = False
                if s.fused(self.learner):
                    first = max(s.total_steps, s.p["n_initial_samples"]) + 1
                    s.total_steps += n_stepped
                    if s.total_steps >= first:
                        runs[i] = (first, s.total_steps - first + 1)
                else:
                    for _ in range(n_stepped):
                        s.total_steps += 1
                        if s.total_steps > s.p["n_initial_samples"]:
                            self._gradient_step(i)
            self._gradient_runs(runs)
            for i in live:
                if not any(self.seeds[i].active):
                    self._end_epoch(self.seeds[i])
        self.group.close()
        return [(s.per_epoch("returns"), s.per_epoch("lengths")) for s in self.seeds]


def train_seeds_vector(keys, p, agents, envs, replay_buffers, save_fn=None, learner=None):
    """``experiments.base.dqn.train_vector`` for S seeds in one process: ``envs[i]`` is seed i's list of E environments and
    ``replay_buffers[i]`` its ``VectorReplayBuffer(n_envs=E)``; returns ``(returns, lengths)`` per epoch, per seed.  ``learner``:
    a ``PrioritizedGroupLearner`` over the same agents and buffers; the trainer then runs on the learner's ``AgentGroup``."""
    group = learner.group if learner is not None else None
    return SeedVectorTrainer(keys, p, agents, envs, replay_buffers, save_fn, group=group, learner=learner).run()
