"""Custom jump proposals in the cycle as batched device callbacks on the split path (csrc/ptmi_cj.hip; include/ptmi.h ptmi_cj_*;
PTEngine(jumps=...), PTEngine.jump_stage, PTSampler.addProposalToCycle(..., batched=True)): the reference's addProposalToCycle
(PTMCMCSampler.py:988-1014, dispatched at :1058-1059) for every chain of the batch at once.

  1. a sampler with the jump as a batched torch callback equals, bit for bit, the sampler that calls the same arithmetic per chain in
     NumPy on the host;
  2. row kernels (one launch, two launches) and the shape kernels give the same buffers with the stage between their launches;
  3. the library's box draw holds lo + (hi - lo) u with u from the oracle's Philox at the documented counter;
  4. the reference's own test cycle (tests/test_simple.py:94-97: SCAM/AM/DE 20/20/20 + a uniform jump of weight 5) samples its target.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

NAMES = ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "cjstat", "nswap", "Q", "qaux", "AM", "AMaux", "AMflag", "cov", "Ut", "S", "DE")
SLOT_CJ = 0x4000000


# ----------------------------------------------------------------------------------------------------------- 1. the sampler
def test_batched_jump_equals_the_per_chain_jump(tmp_path):
    """Two samplers, one seed, a custom jump of weight 3 beside SCAM / AM / DE, swaps, covariance and DE epochs inside: (a) calls
    logl / logp / the jump per chain in NumPy on the host, (b) is batched=True with the same arithmetic in torch -- element-wise IEEE
    operations only, the sum spelled out column by column, so that both give the same bits."""
    import torch
    from ptmcmcsampler_amd import PTSampler
    d = 4
    kw = dict(burn=100, thin=1, covUpdate=50, isave=100, Tskip=10, SCAMweight=20, AMweight=20, DEweight=20)

    def logl_np(x):
        return -0.5 * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3])

    def logp_np(x):
        return 0.0 if np.all((x >= -3.0) & (x <= 3.0)) else -np.inf

    def logl_t(X):
        return -0.5 * (X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1] + X[:, 2] * X[:, 2] + X[:, 3] * X[:, 3])

    def logp_t(X):
        return torch.where(((X >= -3.0) & (X <= 3.0)).all(-1), 0.0, -float("inf")).to(torch.float64)

    def make_np():
        def shrinkJump(x, it, beta):
            c = 0.01 * float((it % 7) - 3)
            return x * 0.5 + (0.25 * beta + c), -0.1 * beta
        return shrinkJump

    seen = []

    def make_t():
        def shrinkJump(X, it, beta):
            assert X.is_cuda and X.dtype == torch.float64 and X.shape[1] == d and beta.shape == (X.shape[0],) and X.shape[0] > 0
            seen.append(X.shape[0])
            c = 0.01 * float((it % 7) - 3)
            return X * 0.5 + (0.25 * beta + c)[:, None], -0.1 * beta
        return shrinkJump

    a = PTSampler(d, logl_np, logp_np, np.eye(d) * 0.5, outDir=str(tmp_path / "a"), verbose=False, seed=4, ntemps=3, nwalkers=4, keep_walkers=4)
    a.addProposalToCycle(make_np(), 3)
    a.sample(np.full(d, 0.1), 300, **kw)
    b = PTSampler(d, logl_t, logp_t, np.eye(d) * 0.5, outDir=str(tmp_path / "b"), verbose=False, seed=4, ntemps=3, nwalkers=4, keep_walkers=4,
                  batched=True)
    b.addProposalToCycle(make_t(), 3, batched=True)
    b.sample(np.full(d, 0.1), 300, **kw)
    for name in ("X", "lnL", "lp", "slot_of", "nacc", "jstat", "nswap", "Ut"):
        assert_same(a.engine.get(name), b.engine.get(name), name)
    assert np.array_equal(a._chains, b._chains) and np.array_equal(a._lnlikes, b._lnlikes) and np.array_equal(a._lnprobs, b._lnprobs)
    files = ["chain_1.0.txt"] + ["chain_1.0_w%d.txt" % k for k in range(1, 4)]
    for f in files + ["jumps.txt", "shrinkJump_jump.txt"]:
        assert open(tmp_path / "a" / f).read() == open(tmp_path / "b" / f).read(), f
    assert a.jumpDict == b.jumpDict
    prop, acc = b.jumpDict["shrinkJump"]
    assert 0 <= acc <= prop and prop > 0 and sum(v[0] for v in b.jumpDict.values()) == 300
    cj = b.engine.get("cjstat").astype(np.int64)
    assert cj.shape == (4, 3, 3, 2) and cj[..., 0].sum() == sum(seen)               # every listed chain went through the callback once
    assert (b.engine.get("jstat").astype(np.int64)[..., 0].sum(-1) + cj[..., 0].sum(-1) == 300).all()
    # the row kernels serve (b) although its cycle has AM entries beside the custom ones
    v = C.c_int32(0)
    assert b.engine.lib.ptmi_split_am_piece(b.engine.h, C.byref(v)) == 0 and v.value > 0


# ------------------------------------------------------------------------------------------------------------ 2. the engine
def _snapshot(g):
    g.sync()
    out = {k: g.t[k].cpu().numpy().copy() for k in NAMES if g.t.get(k) is not None}
    out["Q"] = g.proposals().cpu().numpy().copy()
    assert not g.t["sloc"].any()
    return out


def _jumps(torch, probe):
    """Two batched jumps: deterministic functions of (x, iter, beta), one with a qxy that depends on beta, one without.  ``probe``
    (a dict) names the engine being run: the first call of every run asks ptmi_accept from INSIDE the stage."""
    def stretchJump(X, it, beta):
        assert X.shape[0] > 0 and beta.shape == (X.shape[0],)
        g = probe.get("engine")
        if g is not None and probe.get("rc") is None:
            probe["rc"] = g.lib.ptmi_accept(g.h, it, g.t["lnL"].data_ptr(), g.t["lp"].data_ptr())
        return X * 0.5 + (0.05 * beta)[:, None], -0.1 * beta

    def shiftJump(X, it, beta):
        assert X.shape[0] > 0
        X += 0.01 * float((it % 5) - 2)                       # in place: the same rows come back
        return X, None

    return stretchJump, shiftJump


ENGINE_CASES = [
    # d, nt, W, weights, extra
    (20, 4, 37, (3, 0, 2), {}),                               # 148 chains: 2.3 tiles
    (20, 4, 37, (3, 2, 2), {}),                               # AM entries beside the custom ones: the increments' scratch from ptmi_cj_attach
    (21, 3, 5, (3, 0, 2), {}),                                # odd ndim: 8-byte pieces
    (21, 3, 5, (3, 2, 2), {}),
    (20, 4, 6, (3, 2, 2), dict(pick_mode="walker")),
    # 1400 chains: two blocks of the listing -- a second block's start, no more: cj_gather_kernel's strided sums over the blocks
    # (32 partial sums per function, block b in partial b % 32) take their second step from 33 blocks on, which
    # test_listing_beyond_one_stride_of_blocks reaches
    (6, 2, 700, (3, 2, 2), dict(cov_mode="pooled")),
]


@pytest.mark.parametrize("d,nt,W,weights,extra", ENGINE_CASES)
def test_stage_between_row_kernels_and_between_shape_kernels(mods, d, nt, W, weights, extra, monkeypatch):
    import torch
    orc, _lib, PTEngine = mods
    probe = {}
    f1, f2 = _jumps(torch, probe)

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    rs = np.random.RandomState(d + nt)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.05
    kw = dict(weights=weights, cov_update=20, burn=40, tskip=7, seed=31, split=True, w_host=3, jumps=[(f1, 2), (f2, 1)], **extra)
    engines = []
    for mode in ("rows fused", "rows two launches", "shape kernels"):
        g = PTEngine(d, nt, W, cov0, **kw)
        g.init_state_callback(p0, logl, None)
        engines.append((mode, g))
    if weights[1] > 0:
        v = C.c_int32(0)
        _lib.check(engines[0][1].lib.ptmi_split_am_piece(engines[0][1].h, C.byref(v)))
        assert v.value > 0                                    # the row kernels serve the handle
    snaps = {}
    for n in (25, 3, 1, 46, 30):
        for mode, g in engines:
            if mode == "shape kernels":
                monkeypatch.setenv("PTMI_SPLIT_ROWS", "0")
            else:
                monkeypatch.delenv("PTMI_SPLIT_ROWS", raising=False)
            probe.update(engine=g, rc=None)
            g.run_callback(n, logl, None, fused=(mode == "rows fused"))
            assert probe["rc"] in (None, -1)                  # PTMI_EINVAL between begin and end (None: the function had no pick in this run)
            snaps[mode] = _snapshot(g)
        monkeypatch.delenv("PTMI_SPLIT_ROWS", raising=False)
        it = engines[0][1].iter
        a, b, c = (snaps[m] for m, _ in engines)
        assert a.keys() == b.keys() == c.keys() and "cjstat" in a
        for k in a:
            assert_same(b[k], c[k], "two launches vs shape kernels at iteration %d: %s" % (it, k))
            assert_same(a[k], b[k], "one launch vs two at iteration %d: %s" % (it, k))
    g = engines[0][1]
    js, cj = g.get("jstat").astype(np.int64), g.get("cjstat").astype(np.int64)
    assert (js[..., 0].sum(-1) + cj[..., 0].sum(-1) == g.iter).all()
    assert cj[..., 0].sum(axis=(0, 1)).min() > 0 and (cj[..., 1] <= cj[..., 0]).all() and cj[..., 1].sum() > 0
    assert 0 < g.get("nacc").sum() < W * nt * g.iter


LB, STRIDE = 1024, 32                                         # chain slots per listing block, partial sums per function (csrc/ptmi_cj.hip)


def _box_uniforms(orc, seed, it, sid, d):
    """The d uniforms of the library's box draw for stream ``sid`` at iteration ``it`` (test_box_draw_holds_the_oracles_uniforms)."""
    u = np.empty(d)
    for i in range(d):
        wd = orc.philox([it & 0xFFFFFFFF, it >> 32, sid, SLOT_CJ + (i >> 1)], [seed & 0xFFFFFFFF, seed >> 32])
        word = ((wd[3] << 32) | wd[2]) if (i & 1) else ((wd[1] << 32) | wd[0])
        u[i] = (word >> 11) * 2.0 ** -53
    return u


@pytest.mark.parametrize("d,pick_mode", [(6, "chain"), (5, "chain"), (6, "walker")])
def test_listing_beyond_one_stride_of_blocks(mods, d, pick_mode):
    """7 x 10 007 = 70 049 chains: 69 listing blocks, 417 slots in the last.  cj_gather_kernel sums the block counts of a function in
    32 strided partial sums (``for (b = part; b < nblk; b += 32)``: ptot, and ppre for the blocks before its own): from 33 blocks on the
    loop takes a second step, here a second and a third, and the blocks 32 .. 68 have counts of earlier strides in their ppre.  A wrong
    start sends rows to the wrong chains, and nothing the device compares with itself notices.

    So every jump stage of the run is held to NumPy, from what the proposal launch left: the picks in qaux[.][1], temp_of and the
    proposal buffer give, per function, the ascending slot list; each callback must have been handed exactly those rows and
    beta[temp_of], in that order (hence offs); after ptmi_cj_end the proposal buffer holds what the callbacks returned at the listed
    chains and its old bits everywhere else, qaux[.][0] the qxy.  The box draw (cj_box_kernel reads list[k0 + k]) is held to the
    oracle's Philox for rows at both ends of its span and seeded ones between.  Three functions of weights 3, 2, 1 beside SCAM and DE;
    16-byte and 8-byte pieces; pick_mode "walker": runs of 7 slots share a function.  Swaps (3), covariance epochs (4) and the DE
    activation (8) lie inside, so temp_of is not the identity."""
    from ptmcmcsampler_amd.engine import box_draw_jump
    orc, _lib, PTEngine = mods
    nt, W, seed = 7, 10007, 31
    n = W * nt
    nblk = -(-n // LB)
    assert nblk == 69 and nblk > 2 * STRIDE and n - (nblk - 1) * LB == 417
    rs = np.random.RandomState(d + nt)
    lo, hi = -0.4 - 0.1 * rs.rand(d), 0.4 + 0.1 * rs.rand(d)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.05
    log = []

    def stretchJump(X, it, beta):
        return X * 0.5 + (0.05 * beta)[:, None], -0.1 * beta

    def shiftJump(X, it, beta):
        X += 0.01 * float((it % 5) - 2)                       # in place: the same rows come back
        return X, None

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    g = PTEngine(d, nt, W, cov0, weights=(3, 0, 2), cov_update=4, burn=8, tskip=3, seed=seed, split=True, cov_mode="pooled", pick_mode=pick_mode,
                 jumps=[(stretchJump, 3), (box_draw_jump(lo, hi), 2), (shiftJump, 1)])
    nb = C.c_size_t(0)
    _lib.check(g.lib.ptmi_cj_work_bytes(g.h, C.byref(nb)))
    al16 = lambda v: (v + 15) & ~15                                   # noqa: E731
    assert nb.value == al16(4 * n) + 4 * nblk * _lib.CJ_MAXFUN + al16(8 * (_lib.CJ_MAXFUN + 1))   # the library's own block count
    nf, fop, beta_of = len(g._jumps), np.asarray(g._fun_of_pick), 1.0 / g.temps_mh
    assert nf == 3 and fop.tolist() == [0, 0, 0, 1, 1, 2]

    def recorded(f, func):
        def call(X, it, beta):
            given = (X.clone(), beta.clone())
            Q, qxy = func(X, it, beta)
            log.append((f, it, given[0], given[1], Q.clone(), None if qxy is None else qxy.clone()))
            return Q, qxy
        return call

    g._jumps[:] = [recorded(f, func) for f, func in enumerate(g._jumps)]
    stage, seen = g.jump_stage, dict(stages=0, rows=np.zeros(nf, np.int64), moved=0)

    def checked_stage(it):
        g.sync()
        before = g.proposals().cpu().numpy().reshape(n, d).copy()
        qa = g.t["qaux"].cpu().numpy().reshape(n, 4).copy()
        temp_of = g.get("temp_of").reshape(n).astype(np.int64)
        del log[:]
        total = stage(it)
        g.sync()
        after = g.proposals().cpu().numpy().reshape(n, d)
        qa2 = g.t["qaux"].cpu().numpy().reshape(n, 4)
        what = "%s d=%d iteration %d" % (pick_mode, d, it)
        pick = qa[:, 1].astype(np.int64) - _lib.J_NTYPES
        fun = np.where((pick >= 0) & (pick < len(fop)), fop[np.clip(pick, 0, len(fop) - 1)], -1)
        if pick_mode == "walker":
            assert (fun.reshape(W, nt) == fun.reshape(W, nt)[:, :1]).all(), what
        want_after, want_qxy = before.copy(), qa[:, 0].copy()
        assert [e[0] for e in log] == [f for f in range(nf) if (fun == f).any()] and all(e[1] == it for e in log), what
        for f, _, X, beta, Q, qxy in log:
            slots = np.flatnonzero(fun == f)                          # ascending: the order of the list
            assert_same(X.cpu().numpy(), before[slots], "%s: the rows function %d was handed" % (what, f))
            assert_same(beta.cpu().numpy(), beta_of[temp_of[slots]], "%s: the beta function %d was handed" % (what, f))
            want_after[slots] = Q.cpu().numpy()
            want_qxy[slots] = 0.0 if qxy is None else qxy.cpu().numpy()
            seen["rows"][f] += len(slots)
            if f == 0:
                assert_same(Q.cpu().numpy(), before[slots] * 0.5 + (0.05 * beta_of[temp_of[slots]])[:, None], what + ": stretchJump")
            if f == 1:                                                # the library's draw: both ends of the span and seeded rows between
                q = Q.cpu().numpy()
                assert (q >= lo).all() and (q <= hi).all(), what
                ks = np.unique(np.concatenate([[0, 1, len(slots) - 2, len(slots) - 1], np.random.RandomState(it).randint(0, len(slots), 12)]))
                for k in ks:
                    sid = (slots[k] // nt) * nt + int(temp_of[slots[k]])
                    assert_same(q[k], lo + (hi - lo) * _box_uniforms(orc, seed, it, int(sid), d), "%s: the box draw of list entry %d" % (what, k))
        assert total == (fun >= 0).sum() == sum(len(e[2]) for e in log), what
        assert list(g._cj_offs) == [int((fun >= 0)[fun < f].sum()) for f in range(nf + 1)], what + ": offs"   # the chains of the functions before f
        assert_same(after, want_after, what + ": the proposal buffer behind ptmi_cj_end")
        assert_same(qa2[:, 0], want_qxy, what + ": qxy")
        assert_same(qa2[:, 1:], qa[:, 1:], what + ": the rest of qaux")
        seen["stages"] += 1
        seen["moved"] += int((temp_of != np.tile(np.arange(nt), W)).sum())
        return total

    g.jump_stage = checked_stage
    g.init_state_callback(p0, logl, None)
    for m, fused in ((4, True), (3, False), (4, True)):
        g.run_callback(m, logl, None, fused=fused)
    g.sync()
    assert g.iter == 11 and seen["stages"] == 11 and seen["moved"] > 0 and g.get("nswap").sum() > 0
    # every function had rows in every stage, in about the proportion of its weight (3 : 2 : 1 of 9 before DE joins, of 11 after)
    assert (seen["rows"] > 11 * n // 22).all() and seen["rows"][0] > seen["rows"][1] > seen["rows"][2]
    cj = g.get("cjstat").astype(np.int64)
    assert (g.get("jstat").astype(np.int64)[..., 0].sum(-1) + cj[..., 0].sum(-1) == g.iter).all()
    assert cj[..., 0].sum() == seen["rows"].sum() and cj[..., 1].sum() > 0


def test_accept_is_refused_inside_the_stage_and_empty_spans_are_not_called(mods):
    """One chain: every iteration has one pick, so at most one of the two functions has a row -- the other is not called -- and a
    ptmi_accept issued between ptmi_cj_begin and ptmi_cj_end comes back PTMI_EINVAL."""
    import torch
    orc, _lib, PTEngine = mods
    d, calls, rcs = 4, [0, 0], []
    g = None

    def f1(X, it, beta):
        assert X.shape == (1, d)
        calls[0] += 1
        rcs.append(g.lib.ptmi_accept(g.h, it, g.t["lnL"].data_ptr(), g.t["lp"].data_ptr()))
        return X * 0.9, None

    def f2(X, it, beta):
        assert X.shape == (1, d)
        calls[1] += 1
        return X * 1.1, 0

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    g = PTEngine(d, 1, 1, np.eye(d) * 0.1, weights=(3, 0, 2), cov_update=20, burn=40, tskip=7, seed=5, split=True, jumps=[(f1, 2), (f2, 1)])
    g.init_state_callback(np.full(d, 0.2), logl, None)
    g.run_callback(120, logl, None)
    cj, js = g.get("cjstat").astype(np.int64), g.get("jstat").astype(np.int64)
    assert calls[0] == cj[0, 0, :2, 0].sum() and calls[1] == cj[0, 0, 2, 0]
    assert 0 < calls[0] < 120 and 0 < calls[1] < 120
    assert js[..., 0].sum() + cj[..., 0].sum() == 120
    assert rcs and all(rc == -1 for rc in rcs)                # PTMI_EINVAL
    # a checkpoint carries the counters; one without them restores zeros
    st = g.checkpoint()
    assert np.array_equal(st["t_cjstat"].view(np.uint64), g.get("cjstat"))
    del st["t_cjstat"]
    g.restore(st)
    assert not g.get("cjstat").any()


# ------------------------------------------------------------------------------------------------------------ 3. the box draw
@pytest.mark.parametrize("d", (4, 5))
def test_box_draw_holds_the_oracles_uniforms(mods, d):
    import torch
    orc, _lib, PTEngine = mods
    from ptmcmcsampler_amd.engine import box_draw_jump
    nt, W, seed, it = 3, 50, 0x123456789, 1
    rs = np.random.RandomState(d)
    lo, hi = -1.0 - rs.rand(d), 2.0 + rs.rand(d)
    jump = box_draw_jump(lo, hi)
    assert jump.__name__ == "boxDrawJump"
    g = PTEngine(d, nt, W, np.eye(d) * 0.01, weights=(3, 0, 2), seed=seed, split=True, jumps=[(jump, 2)])
    g.init_state_callback(rs.randn(W, nt, d) * 0.1, lambda X: -0.5 * (X * X).sum(-1), None)
    _lib.check(g.lib.ptmi_propose(g.h, it))
    before = g.proposals().cpu().numpy().copy()
    qa = g.t["qaux"].cpu().numpy()
    n = g.jump_stage(it)
    after = g.proposals().cpu().numpy()
    custom = qa[..., 1] >= _lib.J_NTYPES
    assert n == custom.sum() and 0 < n < W * nt
    temp_of = g.get("temp_of")
    for w in range(W):
        for s in range(nt):
            if not custom[w, s]:
                assert_same(after[w, s], before[w, s], "an untouched row")
                continue
            sid = w * nt + int(temp_of[w, s])
            u = np.empty(d)
            for i in range(d):
                wd = orc.philox([it & 0xFFFFFFFF, it >> 32, sid, SLOT_CJ + (i >> 1)], [seed & 0xFFFFFFFF, seed >> 32])
                word = ((wd[3] << 32) | wd[2]) if (i & 1) else ((wd[1] << 32) | wd[0])
                u[i] = (word >> 11) * 2.0 ** -53
            assert_same(after[w, s], lo + (hi - lo) * u, "the box draw of chain (%d, %d)" % (w, s))
    assert_same(g.t["qaux"].cpu().numpy()[..., 0], np.zeros((W, nt)), "qxy")
    ll = -0.5 * (g.proposals() ** 2).sum(-1).contiguous()
    lp = torch.zeros_like(ll)
    _lib.check(g.lib.ptmi_accept(g.h, it, ll.data_ptr(), lp.data_ptr()))
    g.sync()


# ------------------------------------------------------------------------------------------- 4. the reference's workload
@pytest.mark.parametrize("surface", ("batched", "rows_logl"))
def test_reference_cycle_with_a_uniform_jump_samples_the_target(tmp_path, surface):
    """BASELINE config 1's cycle (the reference's tests/test_simple.py:94-97: SCAM/AM/DE 20/20/20 + UniformJump 5) on the device: a 4-d
    dense Gaussian well inside a box prior, 64 walkers x 4 temperatures.  Mean and covariance of the cold chains against the truth with
    the error model of test_engine_modes_sample_the_same_posterior (40 iterations per independent sample); the jump's share of the
    proposals of all cold chains within 5 binomial standard errors of 5/45 before the DE jump joins (iterations 1 .. burn) and 5/65
    after; and some of its proposals accepted."""
    import torch
    from ptmcmcsampler_amd import PTSampler
    d, W, N, burn = 4, 64, 20000, 2000
    rs = np.random.RandomState(12)
    A = rs.randn(d, d)
    Cov = A @ A.T / d + 0.3 * np.eye(d)
    mu = rs.randn(d)
    P = np.linalg.inv(Cov)
    sd = np.sqrt(np.diag(Cov))
    lo, hi = mu - 6.0 * sd, mu + 6.0 * sd                    # the box cuts 6 sigma off: nothing a run of this length sees
    common = dict(outDir=str(tmp_path), verbose=False, seed=21, ntemps=4, nwalkers=W, keep_walkers=W)
    if surface == "batched":
        mu_t, P_t = torch.as_tensor(mu, device="cuda"), torch.as_tensor(P, device="cuda")
        lo_t, hi_t = torch.as_tensor(lo, device="cuda"), torch.as_tensor(hi, device="cuda")

        def logl(X):
            R = X - mu_t
            return -0.5 * (torch.mm(R, P_t) * R).sum(-1)

        def logp(X):
            return torch.where(((X >= lo_t) & (X <= hi_t)).all(-1), 0.0, -float("inf")).to(torch.float64)

        s = PTSampler(d, logl, logp, np.eye(d) * 0.01, batched=True, **common)
    else:
        s = PTSampler(d, ("dense", mu, P), ("box", lo, hi), np.eye(d) * 0.01, rows_logl=True, **common)
    s.addProposalToCycle(s.boxDrawJump(lo, hi), 5, batched=True)
    s.sample(mu + 0.1, N, burn=burn, thin=10, covUpdate=1000, isave=1000, Tskip=100, SCAMweight=20, AMweight=20, DEweight=20)
    x = s._chains[:, 300:, :].reshape(-1, d)
    se = np.sqrt(np.diag(Cov) / (x.shape[0] / 40.0))
    print("mean error / se", np.abs(x.mean(0) - mu) / se, "cov error", np.max(np.abs(np.cov(x.T) - Cov)) / np.max(np.abs(Cov)))
    assert np.all(np.abs(x.mean(0) - mu) < 5 * se)
    assert np.max(np.abs(np.cov(x.T) - Cov)) / np.max(np.abs(Cov)) < 0.12
    assert np.all(x >= lo) and np.all(x <= hi)
    eng = s.engine
    cj, js = eng.get("cjstat").astype(np.int64), eng.get("jstat").astype(np.int64)
    assert cj.shape == (W, 4, 5, 2) and (js[..., 0].sum(-1) + cj[..., 0].sum(-1) == N).all()
    # the cold chains of all walkers: W independent draws per iteration
    prop, acc = cj[:, 0, :, 0].sum(), cj[:, 0, :, 1].sum()
    p1, p2, n1, n2 = 5.0 / 45.0, 5.0 / 65.0, W * burn, W * (N - burn)
    expect, sigma = n1 * p1 + n2 * p2, np.sqrt(n1 * p1 * (1 - p1) + n2 * p2 * (1 - p2))
    print("boxDrawJump: proposed %d (expected %.0f +- %.0f), accepted %d" % (prop, expect, sigma, acc))
    assert abs(prop - expect) < 5 * sigma
    assert acc > 0
    # walker 0's cold chain is what jumpDict and the jump files report
    assert s.jumpDict["boxDrawJump"] == [int(cj[0, 0, :, 0].sum()), int(cj[0, 0, :, 1].sum())]
    p1n, p2n = burn * p1, (N - burn) * p2
    assert abs(s.jumpDict["boxDrawJump"][0] - (p1n + p2n)) < 5 * np.sqrt(p1n * (1 - p1) + p2n * (1 - p2))
    assert sum(v[0] for v in s.jumpDict.values()) == N
    assert "boxDrawJump %4.2g" % (5.0 / 65.0) in open(tmp_path / "jumps.txt").read()
    assert len(open(tmp_path / "boxDrawJump_jump.txt").read().split()) >= N // 1000
