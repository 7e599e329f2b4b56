"""Network descriptor of the reference's third architecture, ``DQNNet(..., "impala", ...)``
(``slimdqn/networks/architectures/dqn.py:7-29,54-60``): three residual Stacks of widths ``features[0..2]``, a ReLU, a
flatten, ``Dense + relu`` for every ``features[3:]`` and ``Dense(n_actions)``.

Execution is the HIP path (``csrc/impala_kernels.h``); like ``DQNNet`` this class only carries the architecture and
initialises parameters with the reference's initialiser families: ``xavier_uniform`` for each Stack's ``Conv_0`` and for
every Dense layer, flax's default ``lecun_normal`` for ``Conv_1..4``, zero biases.
"""
from typing import Sequence

import numpy as np


class ImpalaNet:
    architecture_type = "impala"

    def __init__(self, features: Sequence[int], n_actions: int):
        self.features = [int(f) for f in features]
        if len(self.features) < 3:
            raise ValueError(f"impala needs at least 3 features (the three Stacks), got {self.features}")
        self.n_actions = int(n_actions)

    def init_leaf(self, rng: np.random.Generator, name: str, shape, n_heads: int) -> np.ndarray:
        if name.endswith("bias"):
            return np.zeros((n_heads,) + tuple(shape), np.float32)
        receptive = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
        fan_in, fan_out = receptive * shape[-2], receptive * shape[-1]
        if "/Conv_0/" in name or name.startswith("Dense_"):  # xavier_uniform
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            return rng.uniform(-lim, lim, size=(n_heads,) + tuple(shape)).astype(np.float32)
        std = np.sqrt(1.0 / fan_in) / 0.87962566103423978  # lecun_normal: truncated normal, variance 1/fan_in
        z = rng.standard_normal((n_heads,) + tuple(shape))
        bad = np.abs(z) > 2
        while bad.any():
            z[bad] = rng.standard_normal(int(bad.sum()))
            bad = np.abs(z) > 2
        return (z * std).astype(np.float32)
