"""Gradient jumps together with parameter groups (PTMCMCSampler.py:129-145 with :225-258; oracle/ptmcmc_oracle.c mh_one): SCAM / AM /
DE move one group's parameters with that group's eigenvectors, a NUTS / HMC pick moves every parameter with the whitening tables of
the full initial covariance and draws no group.  Held to the oracle bit for bit
  * in the fused kernels (mh_steps_gj_kernel<..., GRP = true>: whole-wave layout at 4 lanes per chain, per-chain at 16 and 64),
  * on the callback path (split_rows_kernel + ptmi_gj_begin / ptmi_gj_step), through callback_segment and split_step,
  * with the built-in likelihood as row kernels (rows_logl=True),
and at the sampler's surface.  One oracle run per case, shared by the tests that need it.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import os
import types

import numpy as np
import pytest

from test_gj_callback_gpu import _oracle_callbacks
from test_gpu_parity import _compare, assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

PIECES = (60, 7, 63, 130)                # uneven pieces through covariance epochs, DE activation and swaps: 260 iterations
_BOX20 = ("box", -10 * np.ones(20), 10 * np.ones(20))
_CURVED20 = dict(logl=("curved",), logp=_BOX20, weights=(10, 0, 10), grad_weights=(10, 10), hmc=(0.08, 2, 50),
                 groups=[list(range(10)), list(range(10, 20))], p0=np.tile(np.array([-0.1, -0.5] * 10), (3, 3, 1)))
_DENSE40 = dict(logl="dense", groups=[list(range(16)), list(range(16, 40))], weights=(20, 20, 20), hmc=(0.1, 2, 20))
_POOLED12 = dict(cov_mode="pooled", groups=[list(range(5)), list(range(5, 12))], weights=(20, 20, 20))

CASES = {
    # name: (d, nt, W, keywords)        what it reaches
    "iso6": (6, 3, 4, dict(groups=[[0, 2, 4], [1, 3, 5]], weights=(20, 20, 20), grad_weights=(10, 10))),   # 4 lanes, interleaved embedding, AM ahead of the launch at 4 lanes
    "iso7_overlap": (7, 3, 4, dict(groups=[list(range(7)), [3, 1], [2]], weights=(20, 20, 20), grad_weights=(0, 20))),   # odd d, overlapping groups, a group of one
    "curved20_box": (20, 3, 3, dict(_CURVED20, cov0=np.eye(20))),
    "curved20_box_diag": (20, 3, 3, dict(_CURVED20, cov0="diag")),                  # the handle that would take the pair layout without groups
    "dense40": (40, 2, 3, dict(_DENSE40, grad_weights=(0, 20))),                    # 16 lanes
    "dense40_diag": (40, 2, 3, dict(_DENSE40, grad_weights=(10, 10), cov0="diag")),  # the handle that would take the wide-16 layout
    "iso130": (130, 2, 2, dict(groups=[list(range(65)), list(range(65, 130))], weights=(10, 0, 10), grad_weights=(5, 10), hmc=(0.1, 2, 10))),   # 64 lanes
    "pooled12_walker_pick": (12, 3, 4, dict(_POOLED12, am_mode="rows", pick_mode="walker", grad_weights=(10, 10))),
    "pooled12_ql": (12, 3, 4, dict(_POOLED12, eig_mode="ql", grad_weights=(0, 20))),      # groups factorized by the device solver
}
CALLBACK_CASES = ("iso6", "iso7_overlap", "dense40", "pooled12_walker_pick")
SNAP = ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM", "gj", "Ut", "S")
_ref = {}


def _setup(name):
    """The case's (d, nt, W, cov0, p0, engine keywords), the same for every engine of the case."""
    d, nt, W, kw = CASES[name]
    kw = dict(kw)
    rs = np.random.RandomState(sorted(CASES).index(name))
    A = rs.randn(d, d)
    cov0 = kw.pop("cov0", None)
    full = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    if cov0 is None:
        cov0 = full
    elif isinstance(cov0, str):
        cov0 = np.diag(np.diag(full)) if kw["logl"] == "dense" else np.diag(rs.uniform(0.5, 1.5, d))     # (the curved family starts from a unit-scale covariance)
    p0 = kw.pop("p0", None)
    if p0 is None:
        p0 = rs.randn(W, nt, d) * 0.3
    if kw.get("logl") == "dense":
        P = rs.randn(d, d)
        kw["logl"] = ("dense", rs.randn(d) * 0.1, P @ P.T / d + np.eye(d))
        p0 = p0 * 0.1
    kw.update(cov_update=50, burn=100, tskip=10, seed=4000 + d)
    return d, nt, W, cov0, p0, kw


def _oracle(mods, name):
    """The oracle's run of a case, once: the live engine (its cfg serves the oracle callbacks) and its state after every piece."""
    if name not in _ref:
        orc, _lib, _ = mods
        d, nt, W, cov0, p0, kw = _setup(name)
        o = orc.OracleEngine(d, nt, W, cov0, **kw)
        assert o.lanes == _lib.lanes_for(d, grad=True)
        o.init_state(p0)
        snaps = []
        for n in PIECES:
            o.run(n)
            snaps.append(types.SimpleNamespace(**{k: np.array(getattr(o, k)) for k in SNAP}))
        # no case passes idle: every chain made one proposal per iteration, every weighted jump was proposed, the gradient jumps, DE and
        # AM accepted, swaps were accepted
        js = o.jstat.astype(np.int64)
        gw, w = kw["grad_weights"], kw["weights"]
        assert (js[..., 0].sum(-1) == sum(PIECES)).all()
        if gw[0]:
            assert js[..., 3, 0].sum() > 0 and js[..., 3, 0].sum() == js[..., 3, 1].sum()       # NUTS proposals are built to be accepted
        else:
            assert js[..., 3, 0].sum() == 0
        if gw[1]:
            assert js[..., 4, 0].sum() > 0 and js[..., 4, 1].sum() > 0
        if w[2]:
            assert js[..., 2, 0].sum() > 0
        if w[1]:
            assert js[..., 1, 1].sum() > 0
        assert js[..., 0, 0].sum() > 0 and o.nswap.sum() > 0
        assert all(np.isfinite(getattr(o, k)).all() for k in ("X", "lnL", "gj"))
        _ref[name] = (o, snaps)
    return _ref[name]


def _compare_all(g, snap, what):
    _compare(g, snap, what)
    assert_same(g.get("gj"), snap.gj, what + "gj")
    assert_same(g.get("Ut"), snap.Ut, what + "Ut")
    assert_same(g.get("S"), snap.S, what + "S")


@pytest.mark.parametrize("name", list(CASES))
def test_fused_kernels_equal_the_oracle(mods, name):
    """PTEngine.run through the fused gradient-jump kernel's group instantiation against OracleEngine.run, after every piece."""
    _, _lib, PTEngine = mods
    o, snaps = _oracle(mods, name)
    d, nt, W, cov0, p0, kw = _setup(name)
    g = PTEngine(d, nt, W, cov0, **kw)
    g.init_state(p0)
    for n, snap in zip(PIECES, snaps):
        g.run(n)
        _compare_all(g, snap, "%s fused it=%d " % (name, g.iter))
    flags, lanes, _ = g.last_variant()
    assert flags & _lib.VAR_GRADJUMP and lanes == _lib.lanes_for(d, grad=True)
    # the GRP instantiation ran, in the one layout of its lane width -- also for the handles that would take the pair layout
    # (curved20_box_diag) or the wide-16 one (dense40_diag) without groups; with an AM entry behind ptmi_am_prepare's pieces
    layout, levels, nbytes, nslots = g.last_gj_launch()
    diag = not np.count_nonzero(cov0 - np.diag(np.diag(cov0)))        # (curved20_box starts from the identity: diagonal tables too)
    want = ((_lib.GJL_WAVE if lanes == 4 else _lib.GJL_CHAIN) | _lib.GJL_GRP | (_lib.GJL_DIAG if diag else 0) |
            (_lib.GJL_BOX_LDS if kw.get("logp", ("flat",))[0] == "box" else 0) | (_lib.GJL_ORDERED if kw["grad_weights"][0] else 0) |
            (_lib.GJL_AM_AHEAD if kw["weights"][1] else 0))
    assert layout == want, "%s launched 0x%x, the case means 0x%x" % (name, layout, want)
    cpw = 64 // lanes
    assert nslots == (-(-(nt * W) // cpw) * cpw if kw["grad_weights"][0] else nt * W) and levels >= 1 and nbytes > 0


@pytest.mark.parametrize("name", CALLBACK_CASES)
def test_callback_path_equals_the_oracle(mods, name):
    """The split path's row kernels with the gradient stage (HMC, and NUTS through split_nuts=True), the callbacks handing back the
    oracle's own values and gradients: callback_segment and split_step both equal the oracle."""
    orc, _, PTEngine = mods
    o, snaps = _oracle(mods, name)
    d, nt, W, cov0, p0, kw = _setup(name)
    nuts = kw["grad_weights"][0] > 0
    seg, step = [PTEngine(d, nt, W, cov0, split=True, split_nuts=nuts, **kw) for _ in range(2)]
    logl, logp, logl_grad, logp_grad = _oracle_callbacks(orc, o)
    for g in (seg, step):
        g.init_state(p0)
    for n, snap in zip(PIECES, snaps):
        seg.run_callback(n, logl, logp, logl_grad=logl_grad, logp_grad=logp_grad)
        step.run_callback(n, logl, logp, fused=False, logl_grad=logl_grad, logp_grad=logp_grad)
        _compare_all(seg, snap, "%s callback_segment it=%d " % (name, seg.iter))
        _compare_all(step, snap, "%s split_step it=%d " % (name, step.iter))


def test_rows_logl_equals_the_oracle_and_the_fused_run(mods):
    """Dense 40-d with groups and HMC as PTEngine(rows_logl=True): the built-in likelihood and its gradient as row kernels over the
    launch's proposals -- the oracle's bits, and the fused run's in every buffer."""
    _, _, PTEngine = mods
    name = "dense40"
    o, snaps = _oracle(mods, name)
    d, nt, W, cov0, p0, kw = _setup(name)
    r = PTEngine(d, nt, W, cov0, rows_logl=True, **kw)
    f = PTEngine(d, nt, W, cov0, **kw)
    for g in (r, f):
        g.init_state(p0)
    for n, snap in zip(PIECES, snaps):
        r.run(n)
        f.run(n)
        _compare_all(r, snap, "rows_logl it=%d " % r.iter)
        f.sync()
        for buf in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM", "gj", "cov", "Ut", "S", "DE"):
            assert_same(r.get(buf), f.get(buf), "rows_logl vs fused it=%d %s" % (r.iter, buf))


SAMPLER_GROUPS = [[0, 2, 4], [1, 3, 5]]
SAMPLER_RUN = dict(burn=100, covUpdate=50, thin=1, isave=100, Tskip=10, SCAMweight=20, AMweight=20, DEweight=20)


def _sampler_cov():
    A = np.random.RandomState(6).randn(6, 6)
    return (A @ A.T / 6 + 0.5 * np.eye(6)) * 0.05


def test_sampler_with_a_device_likelihood(mods, tmp_path):
    """PTSampler(groups=, logl_grad=True, logp_grad=True): all five jumps in the statistics and files, a table per group, and the
    engine's state equal to an oracle engine of the same seed and settings."""
    from ptmcmcsampler_amd.sampler import PTSampler
    orc = mods[0]
    d, nt, W, N = 6, 3, 2, 300
    cov = _sampler_cov()
    p0 = np.random.RandomState(7).randn(W, nt, d) * 0.3
    s = PTSampler(d, ("iso",), ("flat",), np.copy(cov), groups=SAMPLER_GROUPS, logl_grad=True, logp_grad=True, ntemps=nt, nwalkers=W,
                  seed=21, outDir=str(tmp_path), verbose=False)
    s.sample(p0, N, NUTSweight=10, HMCweight=10, **SAMPLER_RUN)
    names = {"covarianceJumpProposalSCAM", "covarianceJumpProposalAM", "DEJump", "NUTSJUMP", "HMCJump"}
    listed = open(tmp_path / "jumps.txt").read()
    for n in names:
        assert n in listed and os.path.isfile(tmp_path / (n + "_jump.txt")), n
    assert names <= set(s.jumpDict) and sum(v[0] for v in s.jumpDict.values()) == N
    assert len(s.U) == 2 and all(np.shape(u) == (3, 3) for u in s.U)
    o = orc.OracleEngine(d, nt, W, cov, ladder=s.ladder, groups=SAMPLER_GROUPS, weights=(20, 20, 20), grad_weights=(10, 10), hmc=(0.1, 2, 300),
                         cov_update=50, burn=100, tskip=10, seed=s.seed)
    o.init_state(p0)
    o.run(N)
    _compare(s.engine, o, "sampler ")
    assert_same(s.engine.get("gj"), o.gj, "sampler gj")
    assert o.jstat.astype(np.int64)[..., 3:, 0].sum(axis=(0, 1)).min() > 0


def test_sampler_with_batched_callbacks(tmp_path):
    """The same target as batched torch callbacks with torch gradients (HMC): two runs of one seed write the same files."""
    from ptmcmcsampler_amd.sampler import PTSampler
    d, nt, W, N = 6, 3, 2, 300
    p0 = np.random.RandomState(7).randn(W, nt, d) * 0.3

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    def logp(X):
        return X.new_zeros(X.shape[0])

    runs = []
    for out in ("a", "b"):
        s = PTSampler(d, logl, logp, _sampler_cov(), groups=SAMPLER_GROUPS, batched=True, logl_grad=lambda X: (logl(X), -X),
                      logp_grad=lambda X: (logp(X), X.new_zeros(X.shape)), ntemps=nt, nwalkers=W, seed=21, outDir=str(tmp_path / out),
                      verbose=False)
        s.sample(p0, N, NUTSweight=0, HMCweight=10, **SAMPLER_RUN)
        runs.append(s)
    a, b = runs
    assert a.jumpDict["HMCJump"][0] > 0 and a.jumpDict == b.jumpDict
    assert sum(v[0] for v in a.jumpDict.values()) == N
    files = sorted(f for f in os.listdir(tmp_path / "a") if f.startswith("chain_") or f.endswith("_jump.txt") or f == "jumps.txt")
    assert "HMCJump_jump.txt" in files and any(f.startswith("chain_") for f in files)
    for f in files:
        assert open(tmp_path / "a" / f).read() == open(tmp_path / "b" / f).read(), f
