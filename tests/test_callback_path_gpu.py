"""The one value that takes another route since the callback path's stages share their conversion (``CallbackPath._dev_f64``,
ptmcmcsampler_amd/callback_path.py): a custom jump's ``qxy`` that comes back as a strided view used to be copied into the stage's buffer
as it was, and is now made contiguous first (the auxiliary stage always did that).  Two engines, one seed; on the first the function
returns ``qxy`` as a contiguous ``[n]`` tensor, on the second the same values as every other element of a ``[2 n]`` buffer: the chains
are the same bit for bit.  The same pair with the function among the auxiliary jumps.

Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads the reference tree."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

D, NT, W, ITERS = 3, 2, 4, 6


def _run(PTEngine, stage, strided):
    """6 iterations (tskip = 3: two swaps) of 4 walkers x 2 temperatures x 3-d on the built-in row kernels with a box prior, one batched
    function in ``stage`` ("jumps" or "aux") whose qxy is contiguous or a stride-2 view.  Returns the engine and the calls' (n, contiguous)."""
    import torch
    calls = []

    def term(beta):
        qxy = -0.1 * beta
        if strided:
            buf = torch.full((2 * qxy.numel(),), float("nan"), dtype=torch.float64, device=beta.device)   # NaN between the values: a copy
            buf[::2] = qxy                                                                                # that took them would show
            qxy = buf[::2]
        calls.append((qxy.numel(), qxy.is_contiguous()))
        return qxy

    def kickJump(X, it, beta):
        return X * 0.5 + (0.05 * beta)[:, None], term(beta)

    def halfway(X, Q, it, beta):
        return X + 0.5 * (Q - X), term(beta)

    rs = np.random.RandomState(11)
    lo, hi = -2.0 * np.ones(D), 2.0 * np.ones(D)
    kw = dict(logl=("iso",), logp=("box", lo, hi), weights=(2, 1, 0), cov_update=1000, burn=10000, tskip=3, seed=17, rows_logl=True)
    if stage == "jumps":
        g = PTEngine(D, NT, W, np.eye(D) * 0.3, jumps=[(kickJump, 3)], **kw)
    else:
        g = PTEngine.with_stages(D, NT, W, np.eye(D) * 0.3, aux=[halfway], **kw)
    g.init_state(rs.randn(W, NT, D) * 0.3)
    logl, logp = g._rows_callbacks()[:2]
    assert logp is not None
    g.run_callback(ITERS, logl, logp)
    g.sync()
    assert g.iter == ITERS and g.swap_proposed == 2
    return g, calls


@pytest.mark.parametrize("stage", ("jumps", "aux"))
def test_a_strided_qxy_gives_the_same_chains_bit_for_bit(mods, stage):
    PTEngine = mods[2]
    a, calls_a = _run(PTEngine, stage, False)
    b, calls_b = _run(PTEngine, stage, True)
    # the same calls on both engines; the first saw contiguous terms only, the second a strided one wherever a view of n > 1 values is
    assert [n for n, _ in calls_a] == [n for n, _ in calls_b] and all(c for _, c in calls_a)
    assert all(c == (n == 1) for n, c in calls_b) and any(n > 1 for n, _ in calls_b)
    if stage == "aux":
        assert [n for n, _ in calls_b] == [W * NT] * ITERS            # every chain, once per iteration
    names = ["X", "lnL", "lp", "jstat", "nacc", "slot_of"] + (["cjstat"] if stage == "jumps" else [])
    for name in names:
        assert_same(a.get(name), b.get(name), "%s: %s" % (stage, name))
    assert np.isfinite(b.get("X")).all() and np.isfinite(b.get("lnL")).all()      # none of the buffer's NaN got in
    nacc = b.get("nacc").astype(np.int64)
    assert 0 < nacc.sum() < W * NT * ITERS                            # the term decided something: not all accepted, not none
    if stage == "jumps":
        cj = b.get("cjstat").astype(np.int64)
        assert cj[..., 0].sum() == sum(n for n, _ in calls_b) > 0     # every listed chain was counted as proposed
