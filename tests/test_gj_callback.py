"""HMC with batched gradient callbacks: what the sampler refuses before any engine or GPU is involved (no GPU needed)."""
import numpy as np
import pytest


def _cb(X):
    return X.sum(-1), X


def test_batched_gradients_refuse_nuts_before_the_engine(tmp_path):
    """NUTS is not built for batched gradient callbacks: initialize() says so, names NUTS and NUTSweight=0, and builds no engine."""
    from ptmcmcsampler_amd.sampler import PTSampler
    d = 3
    s = PTSampler(d, lambda X: X.sum(-1), lambda X: X.sum(-1), np.eye(d), logl_grad=_cb, logp_grad=_cb, batched=True,
                  outDir=str(tmp_path), verbose=False)
    with pytest.raises(NotImplementedError, match="NUTS") as err:
        s.sample(np.zeros(d), 100, NUTSweight=20, HMCweight=20)
    assert "NUTSweight=0" in str(err.value)
    assert s.engine is None
