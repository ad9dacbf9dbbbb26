"""NUTS with batched gradient callbacks (PTSampler(batched_nuts=True)): what the sampler refuses before any engine or GPU is involved
(no GPU needed)."""
import numpy as np
import pytest


def _cb(X):
    return X.sum(-1), X


def test_batched_nuts_needs_batched_gradient_callbacks(tmp_path):
    """batched_nuts=True builds the NUTS trees from batched gradient callbacks: without batched=True and both of them, __init__ refuses."""
    from ptmcmcsampler_amd.sampler import PTSampler
    d = 3
    with pytest.raises(ValueError, match="batched_nuts"):
        PTSampler(d, lambda X: X.sum(-1), lambda X: X.sum(-1), np.eye(d), logl_grad=_cb, logp_grad=_cb, outDir=str(tmp_path),
                  verbose=False, batched_nuts=True)
    with pytest.raises(ValueError, match="batched_nuts"):
        PTSampler(d, lambda X: X.sum(-1), lambda X: X.sum(-1), np.eye(d), batched=True, outDir=str(tmp_path), verbose=False,
                  batched_nuts=True)
    with pytest.raises(ValueError, match="batched_nuts"):
        PTSampler(d, lambda X: X.sum(-1), lambda X: X.sum(-1), np.eye(d), logl_grad=_cb, batched=True, outDir=str(tmp_path),
                  verbose=False, batched_nuts=True)
    with pytest.raises(ValueError, match="batched_nuts"):
        PTSampler(d, ("iso",), ("flat",), np.eye(d), logl_grad=True, logp_grad=True, batched=True, outDir=str(tmp_path), verbose=False,
                  batched_nuts=True)


def test_the_refusal_without_the_flag_names_it(tmp_path):
    """Without batched_nuts, NUTSweight > 0 on batched gradient callbacks is still refused in initialize(), before any engine is
    built; the message names NUTS, NUTSweight=0 and the way in, batched_nuts=True."""
    from ptmcmcsampler_amd.sampler import PTSampler
    d = 3
    s = PTSampler(d, lambda X: X.sum(-1), lambda X: X.sum(-1), np.eye(d), logl_grad=_cb, logp_grad=_cb, batched=True,
                  outDir=str(tmp_path), verbose=False)
    with pytest.raises(NotImplementedError, match="NUTS") as err:
        s.sample(np.zeros(d), 100, NUTSweight=20, HMCweight=20)
    assert "NUTSweight=0" in str(err.value) and "batched_nuts=True" in str(err.value)
    assert s.engine is None
