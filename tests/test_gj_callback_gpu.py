"""HMC on the split path with BATCHED gradient callbacks (csrc/ptmi_gjcb.hip: ptmi_gj_begin / ptmi_gj_step between the proposal
launch and the likelihood callback; PTEngine.gradient_stage; PTSampler(batched=True, logl_grad=, logp_grad=)).

HMCJump of the reference (nutsjump.py:238-291) with the user's gradients, pinned bit for bit:
  * against the ORACLE (hmc_call of oracle/ptmcmc_oracle.c inside its MH step), the callbacks handing back the oracle's own values and
    gradients (orc_logl / orc_logl_grad), through callback_segment and split_step;
  * against the FUSED device HMC (GradJump::hmc, ptmi_mh_steps) at a size the host oracle does not reach, the callbacks being the
    built-in isotropic Gaussian's bits (ptmi_rows_logl, gradient -X);
and at the sampler's surface: jump statistics and files, the target's moments, checkpoint + resume.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_parity import _compare, assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


def _oracle_callbacks(orc, o, box=None):
    """logl, logp, logl_grad, logp_grad as batched device callbacks that return the ORACLE's bits row by row."""
    import torch
    L = orc.lib()

    def rows(X):
        return np.ascontiguousarray(X.detach().cpu().numpy())

    def logl(X):
        q = rows(X)
        v = np.array([L.orc_logl(C.byref(o.cfg), q[i].ctypes.data_as(orc._dp)) for i in range(len(q))])
        return torch.from_numpy(v).to(X.device)

    def logl_grad(X):
        q = rows(X)
        g = np.zeros_like(q)
        v = np.array([L.orc_logl_grad(C.byref(o.cfg), q[i].ctypes.data_as(orc._dp), g[i].ctypes.data_as(orc._dp)) for i in range(len(q))])
        return torch.from_numpy(v).to(X.device), torch.from_numpy(g).to(X.device)

    if box is None:
        return logl, None, logl_grad, None
    lo, hi = box

    def logp(X):
        q = rows(X)
        return torch.from_numpy(np.where(((q >= lo) & (q <= hi)).all(-1), 0.0, -np.inf)).to(X.device)

    def logp_grad(X):
        return logp(X), torch.zeros_like(X)

    return logl, logp, logl_grad, logp_grad


def _case(d, seed, **kw):
    rs = np.random.RandomState(seed)
    A = rs.randn(d, d)
    kw.setdefault("cov0", (A @ A.T / d + 0.5 * np.eye(d)) * 0.01)
    kw.setdefault("p0_scale", 0.3)
    return rs, kw


ORACLE_CASES = [
    # name, d, nt, W, engine keywords
    ("iso5", 5, 3, 4, dict(weights=(20, 0, 20), grad_weights=(0, 20), hmc=(0.1, 2, 30))),
    ("curved20_box", 20, 3, 3, dict(logl=("curved",), logp=("box", -10 * np.ones(20), 10 * np.ones(20)), cov0=np.eye(20),
                                    weights=(10, 0, 10), grad_weights=(0, 10), hmc=(0.08, 2, 50),
                                    p0=np.tile(np.array([-0.1, -0.5] * 10), (3, 3, 1)))),
    ("dense40", 40, 2, 3, dict(logl="dense", weights=(20, 0, 20), grad_weights=(0, 20), hmc=(0.1, 2, 20))),
    ("interval40_diag", 40, 2, 3, dict(logl=("interval", 0.0, 10.0), cov0=np.eye(40) * 0.5, weights=(10, 0, 10), grad_weights=(0, 10),
                                       hmc=(0.4, 2, 100), p0_center=-2.4)),
    ("iso130", 130, 2, 2, dict(weights=(10, 0, 10), grad_weights=(0, 10), hmc=(0.1, 2, 10))),
    ("pooled", 20, 3, 4, dict(weights=(20, 0, 20), grad_weights=(0, 20), cov_mode="pooled", am_mode="rows")),
    ("walker_pick", 12, 3, 4, dict(weights=(20, 0, 20), grad_weights=(0, 20), pick_mode="walker")),
    ("with_am", 40, 2, 3, dict(weights=(20, 20, 20), grad_weights=(0, 20), hmc=(0.1, 2, 20))),
]


def _build(mods, d, nt, W, kw, seed=0):
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
    kw.update(cov_update=50, burn=100, tskip=10, seed=1000 + seed)
    okw = {k: v for k, v in kw.items()}
    o = orc.OracleEngine(d, nt, W, cov0, **okw)
    assert o.lanes == _lib.lanes_for(d, grad=True)
    engines = [PTEngine(d, nt, W, cov0, split=True, **kw) for _ in range(2)]
    o.init_state(p0)
    for g in engines:
        g.init_state(p0)
    box = (kw["logp"][1], kw["logp"][2]) if kw.get("logp", ("flat",))[0] == "box" else None
    return o, engines, _oracle_callbacks(orc, o, box)


def _compare_all(g, o, what):
    _compare(g, o, what)
    assert_same(g.get("gj"), o.gj, what + "gj")


@pytest.mark.parametrize("name,d,nt,W,kw", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_hmc_through_gradient_callbacks_equals_the_oracle(mods, name, d, nt, W, kw):
    """260 iterations through covariance and DE epochs, DE activation and swaps: callback_segment (accept + next proposal in one
    launch, the gradient stage behind every proposal launch) and split_step (two launches per iteration) both equal the oracle."""
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, d, nt, W, kw)
    for n in (60, 7, 63, 130):
        seg.run_callback(n, logl, logp, logl_grad=logl_grad, logp_grad=logp_grad)
        step.run_callback(n, logl, logp, fused=False, logl_grad=logl_grad, logp_grad=logp_grad)
        o.run(n)
        _compare_all(seg, o, "%s callback_segment it=%d " % (name, seg.iter))
        _compare_all(step, o, "%s split_step it=%d " % (name, step.iter))
    js = o.jstat.astype(np.int64)
    assert js[..., 4, 0].sum() > 0 and js[..., 4, 1].sum() > 0                     # HMC proposed and accepted
    assert (js[..., 0].sum(-1) == 260).all()
    assert o.nswap.sum() > 0
    if kw["weights"][2]:
        assert js[..., 2, 0].sum() > 0                                                # DE joined after burn
    if kw["weights"][1]:
        assert js[..., 1, 1].sum() > 0


def test_multi_round_trajectories_equal_the_oracle(mods):
    """Chains far from the mode with a long step: the energy soars, the guard (joint1 - 1000 < joint0) lets trajectories run
    several leapfrogs, so the stage takes several callback rounds per iteration."""
    d, nt, W = 40, 2, 8
    kw = dict(cov0=np.eye(d), weights=(10, 0, 0), grad_weights=(0, 30), hmc=(1.0, 2, 300), p0=np.full((W, nt, d), 30.0))
    o, (seg, step), (logl, logp, logl_grad, logp_grad) = _build(mods, d, nt, W, kw)
    rounds = [0]

    def count_logl(X):
        rounds.append(0)
        return logl(X)

    def count_grad(X):
        rounds[-1] += 1
        return logl_grad(X)

    seg.run_callback(20, count_logl, None, logl_grad=count_grad)
    step.run_callback(20, logl, None, fused=False, logl_grad=logl_grad)
    o.run(20)
    _compare_all(seg, o, "multi-round callback_segment ")
    _compare_all(step, o, "multi-round split_step ")
    _lib = mods[1]
    assert (o.gj[..., _lib.GJ_NLEAP] > o.gj[..., _lib.GJ_HITER]).any()                  # some calls took more than one leapfrog
    assert max(rounds) >= 3                                                             # some iteration's stage took three rounds or more


def test_hmc_through_callbacks_equals_the_fused_device_hmc(mods):
    """W = 256, 8 temperatures, 40-d iso, SCAM + AM + DE + HMC: the split path with the built-in likelihood's bits as callbacks
    (ptmi_rows_logl, gradient -X) against the fused kernels' own HMC (GradJump::hmc) -- every buffer."""
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 40, 8, 256
    rs = np.random.RandomState(5)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.05
    p0 = rs.randn(W, nt, d) * 0.5
    kw = dict(weights=(20, 20, 20), grad_weights=(0, 20), hmc=(0.2, 2, 20), cov_update=50, burn=100, tskip=10, seed=99)
    f = PTEngine(d, nt, W, cov0, **kw)
    s = PTEngine(d, nt, W, cov0, split=True, **kw)
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
            assert_same(s.get(name), f.get(name), "split vs fused it=%d %s" % (s.iter, name))
    js = s.get("jstat").astype(np.int64)
    assert js[..., 4, 1].sum() > 0 and js[..., 1, 1].sum() > 0 and js[..., 2, 0].sum() > 0
    assert torch.is_tensor(s._gj_rows)


LB = 1024                                                             # chain slots per block of the stage's listing (GJ_LB, csrc/ptmi_gjcb.h)
BUFFERS = ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM", "gj", "cov", "Ut", "S", "DE")


def _listing_blocks(_lib, g, want):
    """The listing's block count from W x T -- and, for an HMC-only handle, from the library's own work area, which holds one int32
    per block (work_layout of csrc/ptmi_gjcb.h): another LB fails here and does not quietly make the case a small one.  A handle with
    NUTS has no such check: its work area also holds the trees' stacks, whose sizes are the library's own, so there ``want`` is held
    to this file's LB alone."""
    n = g.W * g.nt
    nblk = -(-n // LB)
    assert nblk == want
    if g.grad_weights[0] == 0 and not g.split_nuts:
        al16 = lambda v: (v + 15) & ~15                               # noqa: E731
        nb = C.c_size_t(0)
        _lib.check(g.lib.ptmi_gj_work_bytes(g.h, C.byref(nb)))
        assert nb.value == 3 * al16(8 * n * g.d) + al16(8 * n) + al16(16 * n) + al16(4 * n) + al16(4 * nblk) + 16   # q, p, xs, joint0, ist, list, bcnt, n
    return nblk


def _split_equals_fused(mods, d, nt, W, kw, segments, nblk, beyond, absent=(), **split_kw):
    """Two engines from one start, the fused kernels' own gradient jumps and the callback path with the built-in likelihood's bits as
    callbacks (ptmi_rows_logl, gradient -X): every buffer bit for bit after every segment; ``absent`` names the buffers neither
    engine has in this configuration.  ``nblk``: the listing's block count, ``beyond``: the count it must exceed for the case's term to be live.  Returns the callback engine and the
    number of rows of every gradient round."""
    orc, _lib, PTEngine = mods
    rs = np.random.RandomState(W + d)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.05
    p0 = rs.randn(W, nt, d) * 0.5
    f = PTEngine(d, nt, W, cov0, **kw)
    s = PTEngine(d, nt, W, cov0, split=True, **split_kw, **kw)
    assert _listing_blocks(_lib, s, nblk) > beyond
    f.init_state(p0)
    s.init_state(p0)
    bl, rounds = s.builtin_logl(), []

    def logl_grad(X):
        rounds.append(X.shape[0])
        return bl(X), -X

    for n in segments:
        f.run(n)
        s.run_callback(n, bl, None, logl_grad=logl_grad)
        f.sync()
        s.sync()
        for name in BUFFERS:
            if name in absent:
                assert s.t.get(name) is None and f.t.get(name) is None, name
            else:
                assert_same(s.get(name), f.get(name), "split vs fused, %d chains, it=%d: %s" % (W * nt, s.iter, name))
    assert s.get("nswap").sum() > 0 and not np.array_equal(s.get("slot_of"), np.tile(np.arange(nt, dtype=np.int32), (W, 1)))
    return s, rounds


def test_hmc_listing_beyond_one_wave_of_blocks(mods):
    """7 x 10 007 = 70 049 chains, 4-d, SCAM + DE + HMC with 2 leapfrogs: 69 listing blocks.  gj_fill_kernel's start of block b is the
    sum of bcnt[0 .. b) over a block's 16 waves, wave k holding part[k] = the counts of blocks 64 k .. 64 k + 63: for the blocks
    65 .. 68 part[1] is non-zero -- up to 64 x 1024 chains (test_full_size_invariants) every part[k], k >= 1, is zero.  A wrong start
    hands the gradients of one chain to another: against the fused kernels' HMC, every buffer.  Swaps (3), covariance epochs (4) and the
    DE activation (8) inside."""
    kw = dict(weights=(20, 0, 20), grad_weights=(0, 20), hmc=(0.2, 2, 3), cov_update=4, burn=8, tskip=3, seed=99, cov_mode="pooled", am_mode="rows")
    s, rounds = _split_equals_fused(mods, 4, 7, 10007, kw, (5, 6), nblk=69, beyond=65)
    js = s.get("jstat").astype(np.int64)
    assert js[..., 4, 0].sum() > 0 and 0 < js[..., 4, 1].sum() < js[..., 4, 0].sum() and js[..., 2, 0].sum() > 0
    assert len(rounds) >= 2 * s.iter and min(rounds) > 0              # a round per leapfrog at the least


def test_hmc_listing_beyond_1024_blocks(mods):
    """16 x 65 601 = 1 049 616 chains, 2-d, SCAM + HMC at equal weights: 1026 listing blocks.  In gj_fill_kernel thread tid sums
    bcnt[tid], bcnt[tid + 1024], ... below its block: for block 1025 thread 0 takes a second step (bcnt[1024]), and every part[k] is
    non-zero from block 960 on.  Four iterations with swaps at 2 and 4; no covariance epoch (cov_update = 8: an AM ring of 8 MB)."""
    kw = dict(weights=(20, 0, 0), grad_weights=(0, 20), hmc=(0.2, 2, 3), cov_update=8, burn=8, tskip=2, seed=7, cov_mode="pooled", am_mode="rows")
    s, rounds = _split_equals_fused(mods, 2, 16, 65601, kw, (3, 1), nblk=1026, beyond=1025, absent=("DE",))
    js = s.get("jstat").astype(np.int64)
    assert js[..., 4, 0].sum() > 0 and 0 < js[..., 4, 1].sum() < js[..., 4, 0].sum()
    assert len(rounds) >= 2 * s.iter and min(rounds) > 0
    assert 0.45 < js[..., 4, 0].sum() / (16 * 65601.0 * s.iter) < 0.55   # half the chains pick HMC (4.2 million picks: a standard error of 0.00024)


def test_accept_refuses_an_unfinished_gradient_stage_and_shapes_are_checked(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 2, 3
    g = PTEngine(d, nt, W, np.eye(d) * 0.1, weights=(1, 0, 0), grad_weights=(0, 50), hmc=(0.1, 2, 5), split=True, tskip=0)
    g.init_state(np.zeros(d))
    z = torch.zeros((W, nt), dtype=torch.float64, device=g.device)
    _lib.check(g.lib.ptmi_propose(g.h, 1))
    assert g.lib.ptmi_accept(g.h, 1, z.data_ptr(), z.data_ptr()) == -1                       # PTMI_EINVAL
    assert b"ptmi_gj_begin" in g.lib.ptmi_last_error()
    n = C.c_int64(0)
    assert g.lib.ptmi_gj_step(g.h, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, z.data_ptr(), C.byref(n)) == -1   # out of sequence
    bl = g.builtin_logl()
    with pytest.raises(ValueError, match="gradient"):
        g.gradient_stage(1, lambda X: (bl(X), -X[:, :-1]))
    with pytest.raises(ValueError):
        PTEngine(d, nt, W, np.eye(d), grad_weights=(5, 5), split=True)                        # NUTS is not served on the split path


def _interval_torch(d, a=0.0, b=10.0):
    """The reference's own gradient workload (tests/test_nuts.py: GaussianLikelihood behind intervalTransform, 40-d on (0, 10)) as a
    batched torch expression in the transformed coordinates p, with its gradient by autograd."""
    import torch
    c = 0.5 * np.log(2 * np.pi)
    lw = float(np.log(b - a))

    def logl(X):
        x = a + (b - a) * torch.sigmoid(X)
        return (-0.5 * x * x - c).sum(-1) + (lw + torch.nn.functional.logsigmoid(X) + torch.nn.functional.logsigmoid(-X)).sum(-1)

    def logl_grad(X):
        Xg = X.detach().requires_grad_(True)
        with torch.enable_grad():
            ll = logl(Xg)
            g, = torch.autograd.grad(ll.sum(), Xg)
        return ll.detach(), g

    def logp(X):
        return torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)

    def logp_grad(X):
        return logp(X), torch.zeros_like(X)

    return logl, logp, logl_grad, logp_grad


def _halfnormal_start(rs, shape):
    x = np.clip(np.abs(rs.randn(*shape)), 1e-6, 9.999)                 # the target itself: a unit Gaussian on (0, 10)
    return np.log(x / 10.0) - np.log1p(-x / 10.0)


def test_sampler_facade_hmc_with_batched_torch_gradients(tmp_path):
    """PTSampler(batched=True, logl_grad=, logp_grad=) with SCAM + HMC on the 40-d interval-transformed Gaussian: HMCJump in the
    jump statistics and files, the target's moments, and checkpoint + resume equal to an uninterrupted run."""
    from ptmcmcsampler_amd.sampler import PTSampler
    d, W, N = 40, 384, 400
    logl, logp, logl_grad, logp_grad = _interval_torch(d)
    cov = np.eye(d) * 0.5
    p0 = _halfnormal_start(np.random.RandomState(1), (W, 1, d))
    run = dict(SCAMweight=20, AMweight=0, DEweight=0, HMCweight=20, NUTSweight=0, MALAweight=0, HMCstepsize=0.4, HMCsteps=50,
               burn=100, covUpdate=100, thin=10, isave=100)

    def sampler(out, **kw):
        return PTSampler(d, logl, logp, np.copy(cov), logl_grad=logl_grad, logp_grad=logp_grad, batched=True, nwalkers=W, ntemps=1,
                         keep_walkers=W, outDir=str(out), verbose=False, seed=11, **kw)

    s = sampler(tmp_path / "a", checkpoint=True)
    s.sample(p0, 2 * N, **run)
    hmc = s.jumpDict["HMCJump"]
    assert hmc[0] > 0 and 0 < hmc[1] < hmc[0]
    assert sum(v[0] for v in s.jumpDict.values()) == 2 * N                 # walker 0's T = 1 chain: one proposal per iteration
    assert os.path.isfile(tmp_path / "a" / "HMCJump_jump.txt")
    rows = np.loadtxt(tmp_path / "a" / "chain_1.txt")
    assert rows.shape == (2 * N // 10 + 1, d + 4)
    js = s.engine.get("jstat").astype(np.int64)
    assert js[..., 4, 0].sum() > 0 and js[..., 3, 0].sum() == 0
    # the cold chains' pooled moments of the back-transformed parameters, from starts drawn from the target itself (a unit Gaussian on
    # (0, 10): half-normal, mean sqrt(2 / pi), variance 1 - 2 / pi); 384 walkers x 40 parameters x 61 kept rows.  The reference's HMC
    # hands qxy = joint1 - joint0 to the Hastings test (NJ:290), which adds it to the posterior difference (PT:615): the posterior
    # change is counted twice, and the cycle's stationary law is not the target but is pulled from it (measured: mean 0.853 against
    # 0.798, variance 0.221 against 0.363).  So the moments are held to the SAME sampler with the device's built-in copy of this
    # likelihood and its analytic gradient (logl=("interval", 0, 10), logl_grad=True: the fused kernels' HMC, the same rule) within
    # 0.02, and to the target within the reference rule's pull: 0.1 on the mean, 0.2 on the variance.
    f = PTSampler(d, ("interval", 0.0, 10.0), ("flat",), np.copy(cov), logl_grad=True, logp_grad=True, nwalkers=W, ntemps=1, keep_walkers=W,
                  outDir=str(tmp_path / "f"), verbose=False, seed=11)
    f.sample(p0, 2 * N, **run)
    x = 10.0 / (1.0 + np.exp(-s._chains[:, 20:]))
    xf = 10.0 / (1.0 + np.exp(-f._chains[:, 20:]))
    assert abs(x.mean() - xf.mean()) < 0.02 and abs(x.var() - xf.var()) < 0.02, (x.mean(), xf.mean(), x.var(), xf.var())
    assert abs(x.mean() - np.sqrt(2 / np.pi)) < 0.1 and abs(x.var() - (1 - 2 / np.pi)) < 0.2, (x.mean(), x.var())
    # N + resume + N equals 2N
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
    """64 x 1024 x 40-d, SCAM + HMC, a torch callback with autograd gradients, 200 iterations: lnL is the callback's value of the
    held row, every chain made one proposal per iteration, nothing is NaN, HMC accepts some and refuses some."""
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W, n = 40, 64, 1024, 200
    logl, logp, logl_grad, logp_grad = _interval_torch(d)
    g = PTEngine(d, nt, W, np.eye(d) * 0.5, weights=(20, 0, 0), grad_weights=(0, 20), hmc=(0.4, 2, 50), cov_update=1000, burn=10000,
                 tskip=100, seed=3, split=True, cov_mode="pooled", am_mode="rows")
    g.init_state_callback(_halfnormal_start(np.random.RandomState(2), (W, nt, d)), logl, None)
    g.run_callback(n, logl, None, logl_grad=logl_grad)
    g.sync()
    X, lnL = g.get("X"), g.get("lnL")
    assert np.isfinite(X).all() and np.isfinite(lnL).all()
    again = logl(torch.from_numpy(X.reshape(-1, d)).to(g.device)).cpu().numpy().reshape(W, nt)
    assert np.allclose(again, lnL, rtol=1e-13, atol=1e-10)
    js = g.get("jstat").astype(np.int64)
    assert js[..., 0].sum() == W * nt * n
    acc = js[..., 4, 1].sum() / js[..., 4, 0].sum()
    assert 0 < acc < 1
