"""NUTS on the split path with BATCHED gradient callbacks (csrc/ptmi_gjcb.hip nuts_round: a per-chain state machine that stops at every
leapfrog's gradient and resumes in the next round; PTEngine(split=True, split_nuts=True); PTSampler(batched_nuts=True)).

NUTSJump of the reference (nutsjump.py:379-840) with the user's gradients, pinned bit for bit:
  * against the ORACLE (nuts_call / hmc_call of oracle/ptmcmc_oracle.c inside its MH step), the callbacks handing back the oracle's own
    values and gradients, through callback_segment and split_step -- NUTS alone and NUTS + HMC, binding caps, deep trees, the
    step-size search's halving loop;
  * against the FUSED device NUTS (GradJump::nuts, ptmi_mh_steps) at a size the host oracle does not reach, the callbacks being the
    built-in isotropic Gaussian's bits (ptmi_rows_logl, gradient -X);
and at the sampler's surface: acceptance, jump files, the target's moments, checkpoint + resume, and the full-size invariants.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gj_callback_gpu import LB, ORACLE_CASES, _case, _compare_all, _halfnormal_start, _interval_torch, _oracle_callbacks, _split_equals_fused
from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


def _build(mods, d, nt, W, kw, seed=0):
    """test_gj_callback_gpu._build with split_nuts=True on the two engines (the oracle takes the same keywords otherwise)."""
    orc, _lib, PTEngine = mods
    kw = dict(kw)
    rs, kw = _case(d, seed, **kw)
    cov0 = kw.pop("cov0")
    scale = kw.pop("p0_scale")
    center = kw.pop("p0_center", 0.0)
    p0 = kw.pop("p0", None)
    if p0 is None:
        p0 = center + rs.randn(W, nt, d) * scale
    if kw.get("logl") == "dense":
        P = rs.randn(d, d)
        P = P @ P.T / d + np.eye(d)
        kw["logl"] = ("dense", rs.randn(d) * 0.1, P)
        p0 = p0 * 0.1
    kw.setdefault("cov_update", 50)
    kw.setdefault("burn", 100)
    kw.setdefault("tskip", 10)
    kw["seed"] = 1000 + seed
    o = orc.OracleEngine(d, nt, W, cov0, **kw)
    assert o.lanes == _lib.lanes_for(d, grad=True)
    engines = [PTEngine(d, nt, W, cov0, split=True, split_nuts=True, **kw) for _ in range(2)]
    o.init_state(p0)
    for g in engines:
        g.init_state(p0)
    box = (kw["logp"][1], kw["logp"][2]) if kw.get("logp", ("flat",))[0] == "box" else None
    return o, engines, _oracle_callbacks(orc, o, box)


def _nuts_cases():
    """ORACLE_CASES of the HMC tests with NUTS in the cycle: NUTS alone (its weight in HMC's place) and NUTS + HMC."""
    out = []
    for name, d, nt, W, kw in ORACLE_CASES:
        w = kw["grad_weights"][1]
        out.append((name + "-nuts", d, nt, W, dict(kw, grad_weights=(w, 0))))
        out.append((name + "-nuts+hmc", d, nt, W, dict(kw, grad_weights=(w, w))))
    return out


NUTS_CASES = _nuts_cases()


def _assert_nuts_ran(o, _lib):
    js = o.jstat.astype(np.int64)
    assert js[..., _lib.J_NUTS, 0].sum() > 0 and js[..., _lib.J_NUTS, 1].sum() > 0                # NUTS proposed and accepted
    called = o.gj[..., _lib.GJ_NITER] > 0
    assert called.any()
    assert (o.gj[..., _lib.GJ_HAVE_EPS][called] == 1.0).all()                                      # every chain that made a call searched its step
    return js


@pytest.mark.parametrize("name,d,nt,W,kw", NUTS_CASES, ids=[c[0] for c in NUTS_CASES])
def test_nuts_through_gradient_callbacks_equals_the_oracle(mods, name, d, nt, W, kw):
    """260 iterations through covariance and DE epochs, DE activation, swaps and the gj_nburn boundary (burn = 100): callback_segment
    and split_step both equal the oracle in every buffer and in the jump state gj."""
    _lib = mods[1]
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, d, nt, W, kw)
    for n in (60, 7, 63, 130):
        seg.run_callback(n, logl, logp, logl_grad=logl_grad, logp_grad=logp_grad)
        step.run_callback(n, logl, logp, fused=False, logl_grad=logl_grad, logp_grad=logp_grad)
        o.run(n)
        _compare_all(seg, o, "%s callback_segment it=%d " % (name, seg.iter))
        _compare_all(step, o, "%s split_step it=%d " % (name, step.iter))
    js = _assert_nuts_ran(o, _lib)
    assert (js[..., 0].sum(-1) == 260).all()
    assert o.nswap.sum() > 0
    if kw["grad_weights"][1]:
        assert js[..., _lib.J_HMC, 0].sum() > 0
    if kw["weights"][2]:
        assert js[..., 2, 0].sum() > 0                                                # DE joined after burn


@pytest.mark.parametrize("maxdepth", [0, 1, 2, 3])
def test_binding_tree_caps_equal_the_oracle(mods, maxdepth):
    """nuts_maxdepth 0..3 stop the doublings of most calls (heights 0..maxdepth only): the cap and its stack heights against the oracle."""
    _lib = mods[1]
    kw = dict(weights=(10, 0, 10), grad_weights=(30, 0), nuts_maxdepth=maxdepth, nuts_delta=0.9)
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, 12, 2, 4, kw, seed=maxdepth)
    for n in (70, 50):
        seg.run_callback(n, logl, logp, logl_grad=logl_grad, logp_grad=logp_grad)
        step.run_callback(n, logl, logp, fused=False, logl_grad=logl_grad, logp_grad=logp_grad)
        o.run(n)
        _compare_all(seg, o, "maxdepth=%d callback_segment it=%d " % (maxdepth, seg.iter))
        _compare_all(step, o, "maxdepth=%d split_step it=%d " % (maxdepth, step.iter))
    _assert_nuts_ran(o, _lib)
    # a call takes at most 2^(maxdepth + 1) - 1 leaves, plus its first call's step-size search
    assert (o.gj[..., _lib.GJ_NLEAP] <= o.gj[..., _lib.GJ_NITER] * (2 ** (maxdepth + 1) - 1) + 201).all()


def _round_counter(logl, logl_grad):
    rounds = [0]

    def count_logl(X):
        rounds.append(0)
        return logl(X)

    def count_grad(X):
        rounds[-1] += 1
        return logl_grad(X)

    return rounds, count_logl, count_grad


def test_deep_trees_equal_the_oracle(mods):
    """A small target acceptance (nuts_delta = 0.99: small steps) on 40-d: trees of height >= 5, i.e. >= 32 callback rounds in one
    iteration and stack heights >= 4 in use, against the oracle."""
    _lib = mods[1]
    kw = dict(cov0=np.eye(40), weights=(10, 0, 0), grad_weights=(30, 0), nuts_delta=0.99, p0_scale=1.0)
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, 40, 2, 4, kw, seed=3)
    rounds, count_logl, count_grad = _round_counter(logl, logl_grad)
    seg.run_callback(40, count_logl, None, logl_grad=count_grad)
    step.run_callback(40, logl, None, fused=False, logl_grad=logl_grad)
    o.run(40)
    _compare_all(seg, o, "deep trees callback_segment ")
    _compare_all(step, o, "deep trees split_step ")
    _assert_nuts_ran(o, _lib)
    assert max(rounds) >= 32, max(rounds)


def test_step_size_search_halves_out_of_a_tight_box(mods):
    """A box prior of half-width 0.3 around the start: the search's first leapfrog at eps = 1 leaves the support (logp = -inf), so its
    halving loop runs (NJ:449-452) before the doubling-or-halving one -- against the oracle."""
    _lib = mods[1]
    d = 8
    kw = dict(cov0=np.eye(d), logp=("box", -0.3 * np.ones(d), 0.3 * np.ones(d)), weights=(10, 0, 0), grad_weights=(30, 10),
              p0_scale=0.02)
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, d, 3, 4, kw, seed=4)
    for n in (3, 47):
        seg.run_callback(n, logl, logp, logl_grad=logl_grad, logp_grad=logp_grad)
        step.run_callback(n, logl, logp, fused=False, logl_grad=logl_grad, logp_grad=logp_grad)
        o.run(n)
        _compare_all(seg, o, "tight box callback_segment it=%d " % seg.iter)
        _compare_all(step, o, "tight box split_step it=%d " % step.iter)
    _assert_nuts_ran(o, _lib)
    # the search's step is 0.5 k with k = 1/2, 1/4, ... after the halving loop, then doubled or halved: at most 0.5 once it halved
    called = o.gj[..., _lib.GJ_NITER] > 0
    assert np.isfinite(o.gj[..., _lib.GJ_EPS][called]).all()


@pytest.mark.parametrize("d,diag", [(40, False), (20, True)], ids=["40d-full-tables", "20d-diag-tables"])
def test_nuts_through_callbacks_equals_the_fused_device_nuts(mods, d, diag):
    """W = 256, 8 temperatures, SCAM + AM + DE + NUTS + HMC: the split path with the built-in likelihood's bits as callbacks
    (ptmi_rows_logl, gradient -X) against the fused kernels' own NUTS and HMC -- every buffer.  40-d with full whitening tables, 20-d
    with diagonal ones (the fused kernels' two-chains-per-wave layout)."""
    orc, _lib, PTEngine = mods
    nt, W = 8, 256
    rs = np.random.RandomState(6 + d)
    if diag:
        cov0 = np.diag(rs.uniform(0.5, 1.5, d)) * 0.05
    else:
        A = rs.randn(d, d)
        cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.05
    p0 = rs.randn(W, nt, d) * 0.5
    kw = dict(weights=(20, 20, 20), grad_weights=(20, 20), hmc=(0.2, 2, 20), cov_update=50, burn=100, tskip=10, seed=77)
    f = PTEngine(d, nt, W, cov0, **kw)
    s = PTEngine(d, nt, W, cov0, split=True, split_nuts=True, **kw)
    f.init_state(p0)
    s.init_state(p0)
    bl = s.builtin_logl()

    def logl_grad(X):
        return bl(X), -X

    for n in (60, 7, 63, 130):
        f.run(n)
        s.run_callback(n, bl, None, logl_grad=logl_grad)
        f.sync()
        s.sync()
        for name in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM", "gj", "cov", "Ut", "S", "DE"):
            assert_same(s.get(name), f.get(name), "split vs fused %dd it=%d %s" % (d, s.iter, name))
    js = s.get("jstat").astype(np.int64)
    assert js[..., _lib.J_NUTS, 1].sum() > 0 and js[..., _lib.J_HMC, 1].sum() > 0 and js[..., 1, 1].sum() > 0 and js[..., 2, 0].sum() > 0


def test_nuts_listing_beyond_one_wave_of_blocks(mods):
    """7 x 10 007 = 70 049 chains, 4-d, SCAM + DE + NUTS with trees of height <= 3: 69 listing blocks, so gj_fill_kernel's part[1] (the
    counts of blocks 64 .. 127, held by wave 1) is non-zero for the blocks 65 .. 68 -- test_hmc_listing_beyond_one_wave_of_blocks.
    Unlike HMC's fixed trajectory, a tree ends when it turns or is full, and the first call of every chain searches its step: the set
    of listed chains thins out from round to round, down to a few, so the blocks' counts are sparse and uneven (many of them zero).
    Against the fused kernels' NUTS, every buffer; swaps (3), covariance epochs (4), DE activation and the end of the step-size
    adaptation (8) inside."""
    _lib = mods[1]
    kw = dict(weights=(20, 0, 20), grad_weights=(20, 0), nuts_maxdepth=3, cov_update=4, burn=8, tskip=3, seed=77, cov_mode="pooled", am_mode="rows")
    s, rounds = _split_equals_fused(mods, 4, 7, 10007, kw, (5, 6), nblk=69, beyond=65, split_nuts=True)
    js = s.get("jstat").astype(np.int64)
    assert js[..., _lib.J_NUTS, 0].sum() > 0 and js[..., _lib.J_NUTS, 1].sum() > 0 and js[..., 2, 0].sum() > 0
    # the chains whose search and tree took longest are alone in an iteration's last rounds: fewer rows than blocks, so empty blocks
    assert 0 < min(rounds) < -(-7 * 10007 // LB) < LB < max(rounds) and len(rounds) > s.iter


def test_accept_refuses_an_open_nuts_stage_and_the_flag_alone_changes_nothing(mods):
    """ptmi_accept / ptmi_accept_propose refuse while NUTS chains wait for their gradient rounds; split_nuts=True with w_nuts = 0 gives
    the bits of the engine without the flag."""
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 2, 3
    g = PTEngine(d, nt, W, np.eye(d) * 0.1, weights=(1, 0, 0), grad_weights=(50, 0), split=True, split_nuts=True, tskip=0)
    g.init_state(np.zeros(d))
    z = torch.zeros((W, nt), dtype=torch.float64, device=g.device)
    _lib.check(g.lib.ptmi_propose(g.h, 1))
    assert g.lib.ptmi_accept(g.h, 1, z.data_ptr(), z.data_ptr()) == -1                       # PTMI_EINVAL
    assert b"ptmi_gj_begin" in g.lib.ptmi_last_error()
    assert g.lib.ptmi_accept_propose(g.h, 1, z.data_ptr(), z.data_ptr()) == -1
    assert b"ptmi_gj_begin" in g.lib.ptmi_last_error()
    bl = g.builtin_logl()
    assert g.gradient_stage(1, lambda X: (bl(X), -X)) >= 1                                   # the stage runs its rounds ...
    out = torch.empty((W, nt), dtype=torch.float64, device=g.device)
    _lib.check(g.lib.ptmi_rows_logl(g.h, g.proposals().data_ptr(), W * nt, out.data_ptr()))
    _lib.check(g.lib.ptmi_accept(g.h, 1, out.data_ptr(), z.data_ptr()))                     # ... then the accept test takes the proposals
    with pytest.raises(ValueError):
        PTEngine(d, nt, W, np.eye(d), grad_weights=(5, 5), split_nuts=True)                  # split_nuts is the callback path's
    # the flag with w_nuts = 0: the HMC engine's bits
    kw = dict(weights=(20, 0, 20), grad_weights=(0, 20), hmc=(0.1, 2, 30), cov_update=50, burn=100, tskip=10, seed=5)
    p0 = np.random.RandomState(5).randn(4, 3, 5) * 0.3
    a = PTEngine(5, 3, 4, np.eye(5) * 0.05, split=True, **kw)
    b = PTEngine(5, 3, 4, np.eye(5) * 0.05, split=True, split_nuts=True, **kw)
    for e in (a, b):
        e.init_state(p0)
        bl = e.builtin_logl()
        e.run_callback(120, bl, None, logl_grad=lambda X, bl=bl: (bl(X), -X))
        e.sync()
    for name in ("X", "lnL", "nacc", "jstat", "gj", "Ut", "DE"):
        assert_same(b.get(name), a.get(name), "split_nuts with w_nuts = 0: " + name)


def test_sampler_facade_nuts_with_batched_torch_gradients(tmp_path):
    """PTSampler(batched=True, logl_grad=, logp_grad=, batched_nuts=True) with sample()'s default weights (SCAM = AM = DE = NUTS = HMC
    = 20) on the 40-d interval-transformed Gaussian: NUTSJUMP accepts nearly always and writes its jump file, the moments match the
    same sampler on the device family, and checkpoint + resume equals an uninterrupted run."""
    from ptmcmcsampler_amd.sampler import PTSampler
    d, W, N = 40, 256, 300
    logl, logp, logl_grad, logp_grad = _interval_torch(d)
    cov = np.eye(d) * 0.5
    p0 = _halfnormal_start(np.random.RandomState(1), (W, 1, d))
    run = dict(HMCstepsize=0.4, HMCsteps=50, burn=100, covUpdate=100, thin=10, isave=100)

    def sampler(out, **kw):
        return PTSampler(d, logl, logp, np.copy(cov), logl_grad=logl_grad, logp_grad=logp_grad, batched=True, batched_nuts=True,
                         nwalkers=W, ntemps=1, keep_walkers=W, outDir=str(out), verbose=False, seed=11, **kw)

    s = sampler(tmp_path / "a", checkpoint=True)
    s.sample(p0, 2 * N, **run)
    prop, acc = s.jumpDict["NUTSJUMP"]
    assert prop > 0 and acc / prop > 0.97, (prop, acc)
    assert os.path.isfile(tmp_path / "a" / "NUTSJUMP_jump.txt") and os.path.isfile(tmp_path / "a" / "HMCJump_jump.txt")
    assert sum(v[0] for v in s.jumpDict.values()) == 2 * N
    js = s.engine.get("jstat").astype(np.int64)
    assert js[..., 3, 0].sum() > 0 and js[..., 4, 0].sum() > 0
    # The moments of the back-transformed parameters, held to the SAME sampler on the device's built-in copy of this likelihood with
    # its analytic gradient (logl=("interval", 0, 10), logl_grad=True: the fused kernels' NUTS and HMC, the same cycle and rules) with
    # the tolerance of test_the_references_nuts_test_on_the_device_family: 0.03 on the mean, 0.06 on the second moment.  (HMC's qxy
    # pulls either sampler off the target itself, tests/test_gj_callback_gpu.py; the comparison is between the two.)
    f = PTSampler(d, ("interval", 0.0, 10.0), ("flat",), np.copy(cov), logl_grad=True, logp_grad=True, nwalkers=W, ntemps=1,
                  keep_walkers=W, outDir=str(tmp_path / "f"), verbose=False, seed=11)
    f.sample(p0, 2 * N, **run)
    x = 10.0 / (1.0 + np.exp(-s._chains[:, 20:]))
    xf = 10.0 / (1.0 + np.exp(-f._chains[:, 20:]))
    assert abs(x.mean() - xf.mean()) < 0.03 and abs((x * x).mean() - (xf * xf).mean()) < 0.06, (x.mean(), xf.mean(), (x * x).mean(),
                                                                                                   (xf * xf).mean())
    # N + resume + N equals 2N: the step-size state (gj) is in the checkpoint
    b = sampler(tmp_path / "b", checkpoint=True)
    b.sample(p0, N, **run)
    r = sampler(tmp_path / "b", checkpoint=True, resume=True)
    r.sample(p0, 2 * N, **run)
    assert_same(r.engine.get("X"), s.engine.get("X"), "resumed X")
    assert_same(r.engine.get("gj"), s.engine.get("gj"), "resumed gj")
    assert_same(r._chains, s._chains, "resumed chains")
    assert r.jumpDict == s.jumpDict
    assert open(tmp_path / "b" / "chain_1.txt").read() == open(tmp_path / "a" / "chain_1.txt").read()


def test_full_size_invariants(mods):
    """64 x 1024 x 40-d, SCAM + NUTS, a torch callback with autograd gradients, past every chain's first NUTS call: lnL is the
    callback's value of the held row, every chain made one proposal per iteration, nothing is NaN, NUTS accepts nearly always."""
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W, n = 40, 64, 1024, 40
    logl, logp, logl_grad, logp_grad = _interval_torch(d)
    g = PTEngine(d, nt, W, np.eye(d) * 0.5, weights=(20, 0, 0), grad_weights=(20, 0), cov_update=1000, burn=10000, tskip=100, seed=3,
                 split=True, split_nuts=True, cov_mode="pooled", am_mode="rows")
    g.init_state_callback(_halfnormal_start(np.random.RandomState(2), (W, nt, d)), logl, None)
    g.run_callback(n, logl, None, logl_grad=logl_grad)
    g.sync()
    X, lnL = g.get("X"), g.get("lnL")
    assert np.isfinite(X).all() and np.isfinite(lnL).all() and np.isfinite(g.get("gj")).all()
    again = logl(torch.from_numpy(X.reshape(-1, d)).to(g.device)).cpu().numpy().reshape(W, nt)
    assert np.allclose(again, lnL, rtol=1e-13, atol=1e-10)
    js = g.get("jstat").astype(np.int64)
    assert js[..., 0].sum() == W * nt * n
    assert (g.get("gj")[..., _lib.GJ_NITER] > 0).mean() > 0.99                                # (nearly) every chain is past its first call
    acc = js[..., 3, 1].sum() / js[..., 3, 0].sum()
    assert acc > 0.97, acc
