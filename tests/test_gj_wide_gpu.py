"""HMC with batched gradient callbacks beyond 512 parameters (csrc/ptmi_gjcb_wide.hip: the whitening products on the matrix cores,
one wave per listed chain in the step; ptmi_gj_begin / ptmi_gj_step, PTEngine.gradient_stage, PTSampler).

Bit for bit against the ORACLE (hmc_call of oracle/ptmcmc_oracle.c inside its MH step), the callbacks handing back the oracle's own
values and gradients, through callback_segment and split_step -- the pattern of tests/test_gj_callback_gpu.py at the smallest shapes
at which each mechanism of the wide stage can go wrong; then the built-in row kernels as callbacks (rows_logl=True), a custom jump
beside HMC, the launch shapes, the refusals and the sampler's surface.  On the parent every engine here is refused at construction.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gj_callback_gpu import _build, _compare_all
from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


def _p0_with_zeros(d, nt, W, scale):
    p0 = np.random.RandomState(77).randn(W, nt, d) * scale
    p0[..., ::7] = 0.0                                  # exact zeros: -0.0 gradients of the iso family go through `+ 0.0`
    return p0


def _full_cov(d, seed=0):
    A = np.random.RandomState(seed).randn(d, d)         # (what _build draws for its default, without the 0.01)
    return A @ A.T / d + 0.5 * np.eye(d)


P0_520 = np.random.RandomState(78).randn(3, 2, 520) * 0.3           # (the dense case of _build starts from a tenth of it)
BOX_520 = float(np.abs(0.1 * P0_520).max()) + 0.002

WIDE_CASES = [
    # name, d, nt, W, pieces, engine keywords
    # ninth lane slot with one element; 3 padded k-steps; a 1-column last tile; full tables
    ("iso513", 513, 2, 2, (60, 7, 63, 130), dict(weights=(10, 0, 10), grad_weights=(0, 20), hmc=(0.1, 2, 10), p0=_p0_with_zeros(513, 2, 2, 0.3))),
    # the prior's gradient operand, -inf prior rows, AM increments beside the stage
    # (the box ends a hair outside the start's extreme elements: jumps put rows outside from the first iterations on)
    ("dense520_box_am", 520, 2, 3, (60, 7, 63, 130), dict(logl="dense", p0=P0_520, logp=("box", -BOX_520 * np.ones(520), BOX_520 * np.ones(520)),
                                                          weights=(20, 20, 20), grad_weights=(0, 20), hmc=(0.1, 2, 20))),
    # diagonal tables: d multiplications; exact multiples of 64 and 16
    ("diag640", 640, 2, 2, (60, 70), dict(cov0=np.eye(640) * 0.5, weights=(10, 0, 10), grad_weights=(0, 20), hmc=(0.1, 2, 10))),
    # 17 slots, ndim > 1024 (no AM: its split stops at 1024), pooled covariance, one pick per walker
    ("iso1030_pooled_walker", 1030, 2, 2, (40,), dict(weights=(10, 0, 10), grad_weights=(0, 20), hmc=(0.1, 2, 10), cov_mode="pooled",
                                                      am_mode="rows", pick_mode="walker")),
    # the upper limit
    ("iso2048", 2048, 2, 1, (30,), dict(weights=(10, 0, 10), grad_weights=(0, 20), hmc=(0.1, 2, 10))),
]


@pytest.mark.parametrize("name,d,nt,W,pieces,kw", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_wide_hmc_through_gradient_callbacks_equals_the_oracle(mods, name, d, nt, W, pieces, kw):
    """callback_segment (accept + next proposal in one launch, the gradient stage behind every proposal launch) and split_step (two
    launches per iteration) both equal the oracle: every buffer and the jump state, after every piece."""
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, d, nt, W, kw)
    assert o.lanes == 64 and seg.de_ld == d and seg.am_epl == 0
    outside = [0, 0]                                                  # rows with a prior of -inf: proposals, rows of the gradient stage

    def seg_logp(X):
        lp = logp(X)
        outside[0] += int(lp.isinf().sum())
        return lp

    def seg_logp_grad(X):
        lp, g = logp_grad(X)
        outside[1] += int(lp.isinf().sum())
        return lp, g

    for n in pieces:
        seg.run_callback(n, logl, seg_logp if logp else None, logl_grad=logl_grad, logp_grad=seg_logp_grad if logp else None)
        step.run_callback(n, logl, logp, fused=False, logl_grad=logl_grad, logp_grad=logp_grad)
        o.run(n)
        _compare_all(seg, o, "%s callback_segment it=%d " % (name, seg.iter))
        _compare_all(step, o, "%s split_step it=%d " % (name, step.iter))
    js = o.jstat.astype(np.int64)
    assert js[..., 4, 0].sum() > 0 and js[..., 4, 1].sum() > 0                     # HMC proposed and accepted
    assert js[..., 3, 0].sum() == 0 and (js[..., 0].sum(-1) == sum(pieces)).all()
    assert o.nswap.sum() > 0
    if logp is not None:
        assert outside[0] > 0, outside                                # the box prior refused proposals
    if kw["weights"][1]:
        assert js[..., 1, 1].sum() > 0
    if kw["weights"][2] and sum(pieces) > 100:
        assert js[..., 2, 0].sum() > 0                                                # DE joined after burn


FAR = dict(weights=(10, 0, 0), grad_weights=(0, 30), hmc=(1.0, 2, 300))


def test_wide_multi_round_trajectories_equal_the_oracle(mods):
    """40 chains far from the mode with a long step and full tables, HMC-dominated: more than two row tiles and a partial one, rounds
    whose lists shrink, chains that finish in different rounds."""
    d, nt, W = 513, 2, 20
    kw = dict(cov0=_full_cov(d), p0=np.full((W, nt, d), 30.0), **FAR)
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, d, nt, W, kw)
    counts = []

    def count_grad(X):
        counts.append(X.shape[0])
        return logl_grad(X)

    seg.run_callback(12, logl, None, logl_grad=count_grad)
    step.run_callback(12, logl, None, fused=False, logl_grad=logl_grad)
    o.run(12)
    _compare_all(seg, o, "far start callback_segment ")
    _compare_all(step, o, "far start split_step ")
    _lib = mods[1]
    calls, leaps = o.gj[..., _lib.GJ_HITER], o.gj[..., _lib.GJ_NLEAP]
    assert (calls > 0).all() and (leaps[calls > 0] / calls[calls > 0]).max() >= 3.0   # some call took three rounds or more
    assert max(counts) > 32 and 0 < min(counts) < 16                                # three row tiles at the start; a partial one alone later
    assert len(set(counts)) > 3                                                     # the lists shrink


def test_launch_shapes_give_the_same_bits(mods):
    """The product kernel runs two row tiles per wave once a launch lists 32768 chains and one below: 49152 walkers of the far-start
    case (no ladder, one pooled table that no epoch touches) against 48 of them run alone (walker0: the same streams) -- every
    launch of the big batch takes the two-tile shape, every launch of the small one the one-tile shape."""
    orc, _lib, PTEngine = mods
    d, W, n, k0, kn = 513, 49152, 6, 20000, 48
    rs = np.random.RandomState(3)
    p0 = np.full((W, 1, d), 30.0)
    p0[k0:k0 + kn] += rs.randn(kn, 1, d)
    kw = dict(cov_mode="pooled", am_mode="rows", cov_update=n + 1, burn=100, tskip=10, seed=7, split=True, **FAR)
    big = PTEngine(d, 1, W, _full_cov(d), **kw)
    small = PTEngine(d, 1, kn, _full_cov(d), walker0=k0, **kw)
    counts = []
    for g, p in ((big, p0), (small, p0[k0:k0 + kn])):
        bl = g.builtin_logl()

        def logl_grad(X, bl=bl, big=g is big):
            if big:
                counts.append(X.shape[0])
            return bl(X), -X

        g.init_state_callback(p, bl, None)
        g.run_callback(n, bl, None, logl_grad=logl_grad)
        g.sync()
    assert len(counts) > n and min(counts) >= 32768                                 # rounds beyond the first; all in the two-tile shape
    for name in ("X", "lnL", "lp", "nacc", "jstat", "gj"):
        assert_same(big.get(name)[k0:k0 + kn], small.get(name), "two-tile vs one-tile launches: %s" % name)
    js = small.get("jstat").astype(np.int64)
    assert js[..., 4, 0].sum() > 0 and (small.get("gj")[..., _lib.GJ_NLEAP] > small.get("gj")[..., _lib.GJ_HITER]).any()


def _dense_target(d, seed):
    rs = np.random.RandomState(seed)
    B = rs.randn(d, d)
    P = np.linalg.inv(B @ B.T / d + 0.5 * np.eye(d))
    A = rs.randn(d, d)
    return rs, ("dense", rs.randn(d) * 0.05, (P + P.T) / 2.0), (A @ A.T / d + 0.5 * np.eye(d)) * 0.01


def test_rows_logl_with_hmc_equals_the_oracle(mods):
    """PTEngine(600, logl=('dense', mu, P), rows_logl=True, grad_weights=(0, 20)): the library's own row kernels (ptmi_rows_logl,
    ptmi_rows_logl_grad) serve the wide stage; every buffer equals the oracle's run."""
    orc, _lib, PTEngine = mods
    d, nt, W = 600, 2, 2
    rs, logl, cov0 = _dense_target(d, 5)
    p0 = rs.randn(W, nt, d) * 0.05
    kw = dict(logl=logl, weights=(20, 20, 20), grad_weights=(0, 20), hmc=(0.1, 2, 10), cov_update=50, burn=100, tskip=10, seed=12,
              am_mode="rows")
    o = orc.OracleEngine(d, nt, W, cov0, **kw)
    g = PTEngine(d, nt, W, cov0, rows_logl=True, **kw)
    o.init_state(p0)
    g.init_state(p0)
    cbs = g._rows_callbacks()
    for n in (60, 70):
        o.run(n)
        g.run_callback(n, cbs[0], cbs[1], logl_grad=cbs[2], logp_grad=cbs[3])
        _compare_all(g, o, "rows_logl it=%d " % g.iter)
    js = o.jstat.astype(np.int64)
    assert js[..., 4, 1].sum() > 0 and js[..., 1, 0].sum() > 0 and js[..., 2, 0].sum() > 0


def test_custom_jump_beside_wide_hmc_equals_the_oracle(mods):
    """One boxDrawJump beside HMC at 520-d (with_stages(jumps=..., jumps_with_grad=True)) equals the oracle's mixed cycle, as
    tests/test_cycle_mixed_gpu.py does at small d."""
    from ptmcmcsampler_amd.engine import box_draw_jump
    from test_cycle_mixed_gpu import _compare as compare_mixed
    orc, _lib, PTEngine = mods
    d, nt, W, grad = 520, 2, 3, (0, 4)
    rs = np.random.RandomState(8)
    lo, hi = -0.4 - 0.1 * rs.rand(d), 0.4 + 0.1 * rs.rand(d)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.05
    kw = dict(weights=(3, 2, 2), cov_update=20, burn=40, tskip=7, seed=31, logp=("box", lo, hi), am_mode="rows", hmc=(0.1, 2, 10))
    o = orc.OracleEngine(d, nt, W, cov0, jumps=[(("box", lo, hi), 1)], lanes=orc.lanes_for(d, grad=True), **kw)
    o.grad_weights = grad                                             # (the constructor refuses the mix; the C step defines it)
    o.gj_tab = orc.gj_tables(cov0)
    o.cfg.w_nuts, o.cfg.w_hmc = grad
    o.cfg.gj_tab = orc._p(o.gj_tab)
    o.init_state(p0)
    g = PTEngine.with_stages(d, nt, W, cov0, rows_logl=True, jumps=[(box_draw_jump(lo, hi), 1)], grad_weights=grad, jumps_with_grad=True, **kw)
    g.init_state(p0)
    cbs = g._rows_callbacks()
    for n in (25, 3, 32):
        o.run(n)
        g.run_callback(n, cbs[0], cbs[1], logl_grad=cbs[2], logp_grad=cbs[3])
        compare_mixed(g, o, "box draw beside HMC at iteration %d" % g.iter)
    js, cj = o.jstat.astype(np.int64), o.cjstat.astype(np.int64)
    assert cj[..., 0].sum() > 0 and js[..., 4, 0].sum() > 0 and js[..., 4, 1].sum() > 0


def test_work_area_and_refusals(mods):
    """The work area is the header's HMC-only formula at 512 (unchanged) and at 513; NUTS beyond 512-d is refused before anything is
    built, the fused launch of a wide handle by the library."""
    orc, _lib, PTEngine = mods
    nt, W = 2, 3
    for d in (512, 513):
        g = PTEngine(d, nt, W, np.eye(d) * 0.1, weights=(1, 0, 0), grad_weights=(0, 5), hmc=(0.1, 2, 5), split=True)
        nb = C.c_size_t(0)
        _lib.check(g.lib.ptmi_gj_work_bytes(g.h, C.byref(nb)))
        nch, al = nt * W, lambda b: (b + 15) // 16 * 16               # noqa: E731
        assert nb.value == al(8 * nch * d) * 3 + al(8 * nch) + al(16 * nch) + al(4 * nch) + al(4 * ((nch + 1023) // 1024)) + 16, d
    assert g.lib.ptmi_mh_steps(g.h, 1, 1) == -3 and b"ndim <= 512" in g.lib.ptmi_last_error()   # PTMI_EUNSUPPORTED: the 513-d handle
    with pytest.raises(ValueError, match="512"):
        PTEngine(513, nt, W, np.eye(513), grad_weights=(5, 5), split=True, split_nuts=True)
    with pytest.raises(ValueError, match="512"):
        PTEngine(513, nt, W, np.eye(513), grad_weights=(0, 5), split=True, split_nuts=True)
    with pytest.raises(ValueError, match="512"):
        PTEngine(513, nt, W, np.eye(513), grad_weights=(0, 5))          # the fused kernels stay at 512
    with pytest.raises(ValueError, match="2048"):
        PTEngine(2049, nt, W, np.eye(2049), grad_weights=(0, 5), split=True)


def test_sampler_facade_wide_hmc_on_the_row_path(tmp_path):
    """PTSampler(600, ('dense', mu, P), ('box', lo, hi), logl_grad=True, logp_grad=True): the row path by itself, HMCJump in the jump
    files, and the chain of the same sampler built with batched=True callbacks that wrap the library's row kernels."""
    from ptmcmcsampler_amd.sampler import PTSampler
    d, nt, W, N = 600, 2, 2, 300
    rs, logl, cov = _dense_target(d, 21)
    lo, hi = -0.5 * np.ones(d), 0.5 * np.ones(d)
    p0 = rs.randn(W, nt, d) * 0.05
    run = dict(SCAMweight=20, AMweight=20, DEweight=20, HMCweight=20, NUTSweight=0, MALAweight=0, HMCstepsize=0.1, HMCsteps=10,
               burn=100, covUpdate=50, Tskip=10, thin=10, isave=100)
    common = dict(ntemps=nt, nwalkers=W, keep_walkers=W, verbose=False, seed=4)
    s = PTSampler(d, logl, ("box", lo, hi), np.copy(cov), logl_grad=True, logp_grad=True, outDir=str(tmp_path / "a"), **common)
    assert s.rows_logl is True
    with pytest.raises(NotImplementedError, match="NUTSweight=0"):
        s.sample(p0, N, **dict(run, NUTSweight=20))
    s.sample(p0, N, **run)
    assert s.engine.rows_logl and s.engine.grad_weights == (0, 20)
    hmc = s.jumpDict["HMCJump"]
    assert hmc[0] > 0 and 0 < hmc[1] <= hmc[0]
    last = np.loadtxt(tmp_path / "a" / "HMCJump_jump.txt", ndmin=1)[-1]
    assert 0.0 < float(last) <= 1.0
    assert "NUTSJUMP" not in s.jumpDict and not os.path.exists(tmp_path / "a" / "NUTSJUMP_jump.txt")
    cb_logl, cb_logp, cb_logl_grad, cb_logp_grad = s.engine._rows_callbacks()
    b = PTSampler(d, lambda X: cb_logl(X), lambda X: cb_logp(X), np.copy(cov), logl_grad=lambda X: cb_logl_grad(X),
                  logp_grad=lambda X: cb_logp_grad(X), batched=True, outDir=str(tmp_path / "b"), **common)
    b.sample(p0, N, **run)
    assert not b.rows_logl and b.engine.grad_weights == (0, 20)
    assert_same(b._chains, s._chains, "batched callbacks vs the row path: chains")
    assert_same(b.engine.get("X"), s.engine.get("X"), "batched callbacks vs the row path: X")
    assert_same(b.engine.get("gj"), s.engine.get("gj"), "batched callbacks vs the row path: gj")
    assert b.jumpDict == s.jumpDict
    with pytest.raises(ValueError, match="512"):
        PTSampler(d, lambda X: cb_logl(X), lambda X: cb_logp(X), np.copy(cov), logl_grad=lambda X: cb_logl_grad(X),
                  logp_grad=lambda X: cb_logp_grad(X), batched=True, batched_nuts=True, outDir=str(tmp_path / "c"), **common)
