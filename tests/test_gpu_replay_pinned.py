"""GPU: the HBM replay path against traces captured from the reference's OWN replay buffer (tests/replay_pinned.py describes the
file; this module reads nothing else).  Every comparison is exact.

* elements: ``ReplayBuffer`` on the frame ring (``replay_add_frame``, ``replay_gather_stacked``) -- at every checkpoint of every
  stream ``add_count``, the live keys in order and every live element: stacks in bytes, dtype and shape, action, terminal,
  ``episode_end``, and the reward as ``np.float32(captured double)``;
* batches: the sampler must draw the captured keys and ``sample()`` must return the captured stacked batch, repeated slots included;
* the vector ring: ``VectorReplayBuffer`` (``replay_add_step``) for one environment on every stream, and for three environments
  fed three captured time lines at once;
* in-kernel gathers: ``idqn_learn_on_replay`` / ``idqn_learn_on_replay_fc`` on slots of the HIP ring against ``idqn_learn_on_batch``
  on a twin handle whose batch is put together ON THE HOST FROM THE CAPTURED ELEMENTS of the same keys -- the library's gather has
  no part in the twin's input, so the kernels' slot -> row -> frame resolution is tied to the reference itself.
"""
import numpy as np
import pytest

import replay_pinned as rp

pytestmark = pytest.mark.gpu


def _classes():
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import PrioritizedSamplingDistribution, UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    return ReplayBuffer, VectorReplayBuffer, TransitionElement, UniformSamplingDistribution, PrioritizedSamplingDistribution


def _gathered(rb, keys):
    """The elements of ``keys`` as the DEVICE holds them: one stacked gather of their slots, copied back."""
    got = rb._gather((np.asarray(keys, np.int64) % rb._max_capacity).astype(np.int32))
    cols = [np.asarray(getattr(got, f)) for f in rp.FIELDS]
    assert cols[2].dtype == np.float32
    return [rp.Element(*[c[i] for c in cols]) for i in range(len(keys))]


def _host_view(rb, cp):
    """``_memory[key]`` (the mapping callers read; its reward is the host's double) for the oldest and the newest live key."""
    for key in {cp.keys[0], cp.keys[-1]} if cp.keys else ():
        rp.assert_element(rb._memory[key], cp.elements[key], "f64", f"_memory[{key}]")
    assert len(rb._memory) == len(cp.keys) and (not cp.keys or cp.keys[0] - 1 not in rb._memory)


def _buffer(s, vector=False):
    ReplayBuffer, VectorReplayBuffer, Transition, Uniform, Prioritized = _classes()
    args = dict(batch_size=s.batch, max_capacity=s.cap, stack_size=s.stack, update_horizon=s.n, gamma=s.gamma, compress=False)
    if vector:
        return VectorReplayBuffer(rp.make_sampler(s, Uniform, Prioritized), n_envs=1, **args), Transition
    return ReplayBuffer(rp.make_sampler(s, Uniform, Prioritized), **args), Transition


@pytest.mark.parametrize("name", rp.NAMES)
def test_frame_ring_equals_the_reference(name):
    s = rp.load()[name]
    rb, Transition = _buffer(s)
    rp.replay(s, rb, Transition, "f32", _gathered, on_checkpoint=_host_view)
    n0 = s.cap + s.n + s.stack + max(64, s.cap // 16)  # the ring the buffer starts with
    if name == "u8x4":
        assert rb._n_frames == n0 and rb._t > 3 * rb._n_frames  # around the ring several times
    if name == "u8x36":
        assert rb._n_frames > n0  # the element-less run made the ring grow


@pytest.mark.parametrize("name", rp.NAMES)
def test_vector_ring_of_one_environment_equals_the_reference(name):
    s = rp.load()[name]
    rb, Transition = _buffer(s, vector=True)
    rp.replay(s, rb, Transition, "f32", _gathered, on_checkpoint=_host_view)
    if name == "u8x36":
        assert rb._plan.n_growths > 0
    if name == "u8x4":
        assert rb._plan.n_growths == 0 and rb._plan.frame_count[0] > 3 * rb._plan.segment


def test_vector_ring_of_three_environments_equals_three_captures():
    """Three captured time lines of one frame shape and unequal episode lengths, one vector step per transition index
    (``replay_add_step``); tests/replay_pinned.py, ``replay_three_lines``, says what is compared and what must be covered."""
    _, VectorReplayBuffer, Transition, Uniform, _ = _classes()
    s = rp.load()[rp.VECTOR_LINES[0]]
    rb = VectorReplayBuffer(Uniform(0), 8, rp.VECTOR_CAPACITY, stack_size=s.stack, update_horizon=s.n, gamma=s.gamma, n_envs=3,
                            segment=rp.VECTOR_SEGMENT)
    covered = rp.replay_three_lines(Transition, rb.add_many, lambda: rb._plan, lambda keys: _gathered(rb, keys), "f32")
    rp.assert_three_lines_covered(covered, rb._plan)
    assert rb.add_count == rb._plan.add_count and rb._n_frames == rb._plan.n_frames == rb._frames.shape[0]


# ---- in-kernel gathers ------------------------------------------------------------------------------------------------------------
#  case              stream      arch   observation  features            K  B   entry
LEARNERS = {
    "plane_20x20": ("u8x20x20", "cnn", (20, 20, 4), [32, 32, 32, 128], 2, 32, "idqn_learn_on_replay"),  # the plane path's staging launch
    "mlp_stack1_b32": ("f32s1", "fc", 8, [100, 100], 3, 32, "idqn_learn_on_replay_fc"),  # k_fc_step_par reads the ring itself
    "mlp_stack2_b32": ("f32s2", "fc", 18, [100, 100], 3, 32, "idqn_learn_on_replay_fc"),
    "mlp_stack2_b64": ("f32s2", "fc", 18, [100, 100], 3, 64, "idqn_learn_on_replay_fc"),  # behind k_rps_stage
}
STATE = ("_online", "_mu", "_nu", "_count", "_losses", "_cum")
STEPS, N_ACTIONS = 3, 6


def _draws(s, B):
    """``STEPS`` draws of ``B`` live keys (seeded, with repeats).  Every draw holds, twice each, a terminal element and the short
    stacks the stream's geometry allows: a stack of one frame is never short; ``state`` can be from two frames on (the element's
    state ends at the episode's first frames); ``next_state`` ends at trajectory position >= 1, so it is short only from three
    frames on."""
    live, els = s.last.keys, s.last.elements
    zero_first = lambda a: not a.reshape(-1, s.stack)[:, 0].any()
    short_s = [k for k in live if s.stack >= 2 and zero_first(els[k].state) and not zero_first(els[k].next_state)]
    short_n = [k for k in live if s.stack >= 3 and zero_first(els[k].next_state)]
    terminal = [k for k in live if els[k].is_terminal]
    assert terminal and (s.stack < 2 or short_s) and (s.stack < 3 or short_n), "the last checkpoint lacks the elements this case is about"
    rng, out = np.random.default_rng(B + s.stack), []
    for step in range(STEPS):
        keys = rng.choice(live, size=B, replace=True)
        must = [terminal[step % len(terminal)]] + [group[step % len(group)] for group in (short_s, short_n) if group]
        keys[: 2 * len(must)] = must + must
        out.append(keys)
    return out


@pytest.mark.parametrize("case", list(LEARNERS))
def test_learner_on_the_ring_equals_learner_on_the_captured_elements(case):
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    stream, arch, obs, feats, K, B, entry = LEARNERS[case]
    s = rp.load()[stream]
    rb, Transition = _buffer(s)
    for t in range(s.n_transitions):
        rb.add(rp.transition(s, t, Transition))
    assert rb.add_count == s.last.add_count and list(rb._memory.keys()) == s.last.keys
    fused, twin = (iDQN(0, obs, N_ACTIONS, K, feats, arch, 1e-3, s.gamma, s.n, 1, 10**9, 10**9, adam_eps=1.5e-4) for _ in range(2))
    fused._ensure_handle(B)
    for keys in _draws(s, B):
        slots = np.ascontiguousarray(keys % s.cap, np.int32)
        frames, n_frames, frame_bytes, rows, stack = rb.ring_view()[:5]
        _hip.check(getattr(_hip.lib(), entry)(fused._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                                              slots.ctypes.data, B, int(stack), B, 0, _hip.current_stream()), entry)
        els = [s.last.elements[int(k)] for k in keys]  # the reference's elements: nothing below comes out of the ring
        twin._learn(rp.Element(state=np.stack([e.state for e in els]), action=np.asarray([e.action for e in els], np.int32),
                               reward=np.asarray([e.reward for e in els], np.float64).astype(np.float32),
                               next_state=np.stack([e.next_state for e in els]),
                               is_terminal=np.asarray([e.is_terminal for e in els], np.uint8),
                               episode_end=np.asarray([e.episode_end for e in els], np.uint8)))
    torch.cuda.synchronize()
    for name in STATE:
        a, b = getattr(fused, name).cpu().numpy(), getattr(twin, name).cpu().numpy()
        assert a.tobytes() == b.tobytes(), f"{name} differs"
    assert np.isfinite(fused._losses.cpu().numpy()).all() and (fused._count.cpu().numpy() == STEPS).all()
