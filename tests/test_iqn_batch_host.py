"""Host-side checks of i-IQN minibatches above 32 samples: the parameter layout of a quantile-head config is built for any
max_batch up to 256 (the heads deal the batch's 32-sample blocks to their kernels), and refused above.  No GPU needed."""
import pytest

from slimdqn import _hip

FEATS = [32, 64, 64, 512]


def _layout(max_batch):
    return _hip.layout(_hip.make_config("cnn", 5, 6, (84, 84, 4), FEATS, max_batch, 1e-4, 1e-8, 0.99, n_quantiles=32))


def test_iqn_layout_accepts_batches_up_to_256():
    leaves32, stride32 = _layout(32)
    names = [name for name, _, _ in leaves32]
    assert "Embed_0/kernel" in names and "Embed_0/bias" in names
    for B in (33, 64, 256):
        leaves, stride = _layout(B)
        assert leaves == leaves32, B
        assert stride == stride32, B


def test_iqn_layout_refuses_batches_above_256():
    with pytest.raises(_hip.HipExtensionError, match="256"):
        _layout(257)
