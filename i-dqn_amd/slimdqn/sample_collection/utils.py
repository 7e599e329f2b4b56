"""Acting and sample collection -- the other device call of an environment step.

Same entry points as the reference's ``slimdqn/sample_collection/utils.py:8-40`` (``select_action``,
``collect_single_sample``): the key is split three ways (exploration draw, random action, key handed to
``best_action``); the greedy branch is one batch-1 forward of a head on the HIP path (``idqn_best_action``) whose
``.item()`` is the device -> host sync the reference has at ``utils.py:21``.
"""
from slimdqn import prng
from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement


class HostAction(int):
    """A host-side action that answers ``.item()`` like the device scalar of the greedy branch."""

    def item(self):
        return int(self)


def linear_schedule(init_value: float, end_value: float, transition_steps):
    """optax.linear_schedule (experiments/base/dqn.py:19): linear from init to end over transition_steps, then flat."""
    span = init_value - end_value

    def value_at(count):
        if transition_steps <= 0:  # optax.linear_schedule: a constant schedule at init_value
            return init_value
        progress = min(max(count, 0), transition_steps) / transition_steps
        return end_value + span * (1.0 - progress)

    return value_at


def select_action(best_action_fn, params, state, key, n_actions, epsilon_fn, n_training_steps):
    explore_key, random_action_key, greedy_key = prng.split(key, 3)
    exploring = prng.uniform(explore_key) <= epsilon_fn(n_training_steps)
    if exploring:
        return HostAction(prng.randint(random_action_key, 0, n_actions))
    return best_action_fn(params, state, key=greedy_key)  # device scalar


def select_actions(best_actions_fn, params, states, keys, n_actions, epsilon_fn, n_training_steps):
    """``select_action`` for E environments at once: host int list ``[E]`` equal to
    ``[select_action(best_action_fn, params, states[i], keys[i], ...).item() for i]``.  Every environment splits its key
    three ways as ``select_action`` does; the exploring ones get their random action on the host, all the others go
    through ONE ``best_actions_fn(params, greedy states, greedy keys)`` call (none if every environment explores)."""
    assert len(states) == len(keys)
    epsilon = epsilon_fn(n_training_steps)
    actions, greedy, greedy_keys = [None] * len(keys), [], []
    for i, key in enumerate(keys):
        explore_key, random_action_key, greedy_key = prng.split(key, 3)
        if prng.uniform(explore_key) <= epsilon:
            actions[i] = prng.randint(random_action_key, 0, n_actions)
        else:
            greedy.append(i)
            greedy_keys.append(greedy_key)
    if greedy:
        best = best_actions_fn(params, [states[i] for i in greedy], greedy_keys)
        for i, a in zip(greedy, best):
            actions[i] = int(a)
    return actions


def collect_single_sample(key, env, agent, rb: ReplayBuffer, p, epsilon_schedule, n_training_steps: int):
    """One environment step into the replay buffer; returns ``(reward, episode_ended)``.

    ``p["overlap_replay_add"]`` (set by this build's launcher, absent = off): the greedy action is launched without waiting
    (``DeviceAgent.lazy_host_actions``), the replay bookkeeping of the PREVIOUS transition runs while the GPU computes it,
    and this step's ``rb.add`` is postponed the same way (``add_deferred``: flushed before anything reads the buffer) --
    same transitions in the same order, ~20 us of host time per step moved under the ~40 us of the acting launch."""
    overlap = bool(p.get("overlap_replay_add", False)) and hasattr(rb, "add_deferred")
    observation = env.observation  # the frame BEFORE the action goes with it (utils.py:27-35)
    pending = select_action(agent.best_action, agent.params, env.state, key, env.n_actions, epsilon_schedule, n_training_steps)
    if overlap:
        rb.flush_deferred()
    action = pending.item()
    reward, absorbing = env.step(action)
    ended = bool(absorbing) or env.n_steps >= p["horizon"]
    stored_reward = rb._clipping(reward) if rb._clipping is not None else reward
    (rb.add_deferred if overlap else rb.add)(TransitionElement(observation, action, stored_reward, absorbing, ended))
    if ended:
        env.reset()
    return reward, ended


def _best_actions_fn(agent):
    """``agent.best_actions``; an agent without one (no vectorised acting path) acts one state at a time: same actions."""
    if hasattr(agent, "best_actions"):
        return agent.best_actions
    return lambda params, states, keys: [int(agent.best_action(params, s, key=k).item()) for s, k in zip(states, keys)]


def collect_vector_samples(keys, envs, agent, rb, p, epsilon_schedule, n_training_steps: int, active=None):
    """One step of every active environment into a ``VectorReplayBuffer``: ONE ``select_actions`` call, the E host steps, ONE
    ``rb.add_many``; returns ``(rewards, ended)``, lists over all environments (``None`` / ``False`` for an inactive one, which
    neither acts nor steps and is passed to ``add_many`` as ``None``).  ``keys`` holds one key per ACTIVE environment, in
    order; environment ``i`` sees exactly what ``collect_single_sample(keys[i], envs[i], ...)`` would show it."""
    idx = [i for i in range(len(envs)) if active is None or active[i]]
    assert len(keys) == len(idx), "one key per active environment"
    rewards, ended, transitions = [None] * len(envs), [False] * len(envs), [None] * len(envs)
    if not idx:
        return rewards, ended
    observations = [envs[i].observation for i in idx]  # the frame BEFORE the action goes with it (utils.py:27-35)
    actions = select_actions(_best_actions_fn(agent), agent.params, [envs[i].state for i in idx], keys, envs[idx[0]].n_actions,
                             epsilon_schedule, n_training_steps)
    for i, observation, action in zip(idx, observations, actions):
        env = envs[i]
        reward, absorbing = env.step(int(action))
        ended[i] = bool(absorbing) or env.n_steps >= p["horizon"]
        rewards[i] = reward
        stored_reward = rb._clipping(reward) if rb._clipping is not None else reward
        transitions[i] = TransitionElement(observation, int(action), stored_reward, absorbing, ended[i])
    rb.add_many(transitions)
    for i in idx:
        if ended[i]:
            envs[i].reset()
    return rewards, ended
