"""Log-evidence from the ladder on the device (csrc/ptmi_ev.hip; ``PTEngine.with_stages(evidence=True)``, ``PTSampler.log_evidence``): the
accumulators equal the NumPy restatement of the rule (tests/test_evidence.py ``ev_rule``) bit for bit -- crafted cells that reach every
branch, a grid tail, the fused, row and callback paths with the sampling rule of ``PTEngine.swap``, the hot rank, checkpoints -- the stage
only reads (the chains are the same bits), the C ABI refuses what it must, the sampler delivers the estimates, and a run on a Gaussian in
a box measures its known ln Z.

Run with ``python -m pytest tests -m gpu``.  Nothing here reads the reference."""
import ctypes as C

import numpy as np
import pytest

from test_evidence import LNZ_BOX, ev_rule
from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

CHAINS = ("X", "lnL", "lp", "slot_of", "temp_of", "nacc", "nswap")


def _planes(g):
    g.sync()
    return g.t["ev_acc"].cpu().numpy(), g.t["ev_cnt"].cpu().numpy().view(np.uint64)


def _by_rank(g):
    """lnL [W][T] by local rank as it stands on the device."""
    g.sync()
    return np.take_along_axis(g.get("lnL"), g.get("slot_of").astype(np.int64), 1)


def _perms(rs, W, T):
    """A non-identity permutation per walker and its inverse, int32 [W][T]."""
    so = np.stack([rs.permutation(T) for _ in range(W)])
    for w in range(W):
        if (so[w] == np.arange(T)).all():
            so[w] = np.roll(so[w], 1)
    to = np.argsort(so, axis=1)
    return so.astype(np.int32), to.astype(np.int32)


def _own_stage(g, _lib, dbeta, pad=64):
    """Caller-owned buffers attached through the C ABI, with ``pad`` words behind each that no call may touch."""
    import torch
    n = g.W * g.nt
    acc = torch.zeros(5 * n + pad, dtype=torch.float64, device=g.device)
    cnt = torch.zeros(2 * n + pad, dtype=torch.int64, device=g.device)
    dbeta = np.ascontiguousarray(dbeta, dtype=np.float64)
    _lib.check(g.lib.ptmi_ev_attach(g.h, C.c_void_p(acc.data_ptr()), C.c_void_p(cnt.data_ptr()), dbeta.ctypes.data_as(_lib._dp)))

    def read():
        g.sync()
        a, c = acc.cpu().numpy(), cnt.cpu().numpy().view(np.uint64)
        assert not a[5 * n:].any() and not c[2 * n:].any(), "a call wrote behind its planes"
        return a[:5 * n].reshape(5, g.W, g.nt), c[:2 * n].reshape(2, g.W, g.nt)

    return read


def test_crafted_cells_reach_every_branch(mods):
    orc, _lib, PTEngine = mods
    W, T, d = 3, 5, 2
    g = PTEngine(d, T, W, np.eye(d), tskip=10)
    dbeta = np.array([0.0, 1.0, 0.5, 1e-300, 3.0])                    # rank 0 has no colder neighbour; a tiny gap for huge |lnL|
    read = _own_stage(g, _lib, dbeta)
    rs = np.random.RandomState(7)
    so, to = _perms(rs, W, T)
    g.put("slot_of", so)
    g.put("temp_of", to)
    nan, inf = np.nan, np.inf
    rows = [[nan, -inf, inf, inf, -inf],                               # skipped before any sample
            [1.0, -2.0, 5.0, 1e300, 0.5],                              # first samples
            [0.5, -800.0, 4.0, -1e300, 0.25],                          # a falls (rank 1: a - m = -798 < -745.13, the exponential is 0)
            [2.0, 900.0, 6.0, 9.9e299, 300.0],                         # a rises (ranks 1 and 4: m - a below -745.13, es = es * 0 + 1)
            [2.0, 900.0, 6.0, 9.9e299, 300.0],                         # equal values: es += 1
            [inf, nan, -inf, 2.0, nan],                                # skipped between samples
            [-3.0, 900.0 - 745.0, 6.5, -3.0e299, 299.0],               # rank 1: exp(-745), the smallest subnormal
            [7.0, 900.0 - 745.2, -40.0, 1e300, 301.0]]                 # rank 1: just below the underflow threshold
    seq = np.empty((len(rows), W, T))
    for k, row in enumerate(rows):
        for w in range(W):
            v = np.array(row)
            if w and k not in (3, 4):
                v = np.where(np.abs(v) < 1e6, v + 0.125 * w * (1 + k), v)      # walkers differ (the huge values and the equal rows stay)
            seq[k, w] = v
        by_slot = np.empty((W, T))
        np.put_along_axis(by_slot, so.astype(np.int64), seq[k], 1)    # lnL[w][slot_of[w][r]] = the value meant for rank r
        g.put("lnL", by_slot)
        assert_same(_by_rank(g), seq[k], "crafted lnL by rank")
        _lib.check(g.lib.ptmi_ev_update(g.h))
    acc, cnt = read()
    want_acc, want_cnt = ev_rule(seq, dbeta)
    assert_same(cnt, want_cnt, "counts")
    assert_same(acc, want_acc, "planes")
    assert ((cnt[0] + cnt[1]) == len(rows)).all()
    # the crafted values did what they are there for
    assert cnt[1, 0].tolist() == [2, 2, 2, 1, 2] and cnt[0, 0].tolist() == [6, 6, 6, 7, 6]
    assert acc[3, 0, 0] == 0.0 and acc[4, 0, 0] == 6.0                # dbeta[0] = 0: m = 0, es counts the samples
    assert acc[3, 0, 1] == 900.0 and acc[4, 0, 1] == 2.0              # 1 -> (+ 0) -> es * 0 + 1 -> 2 -> (+ 5e-324, + 0: both round away)
    assert acc[2, 0, 3] == np.inf and np.isfinite(acc[4, 0, 3])       # (2e300)^2 overflows s2 as the rule says; the stones do not
    assert acc[3, 0, 4] == 903.0                                      # 3 * 301


def test_grid_tail(mods):
    orc, _lib, PTEngine = mods
    W, T, d = 70, 3, 2                                                  # 210 cells: no multiple of 64 or 256
    g = PTEngine(d, T, W, np.eye(d), tskip=10)
    dbeta = np.array([0.0, 0.25, 0.125])
    read = _own_stage(g, _lib, dbeta)
    rs = np.random.RandomState(8)
    so, to = _perms(rs, W, T)
    g.put("slot_of", so)
    g.put("temp_of", to)
    lnl = rs.randn(W, T) * 10
    lnl[rs.rand(W, T) < 0.1] = -np.inf
    g.put("lnL", lnl)
    _lib.check(g.lib.ptmi_ev_update(g.h))
    seq = np.take_along_axis(lnl, so.astype(np.int64), 1)[None]
    acc, cnt = read()
    want_acc, want_cnt = ev_rule(seq, dbeta)
    assert_same(cnt, want_cnt, "counts")
    assert_same(acc, want_acc, "planes")
    assert cnt[1].sum() > 0 and (cnt.sum(0) == 1).all()


KW = dict(cov_update=20, burn=20, tskip=7, seed=17)                    # the default mix (SCAM / AM / DE at 20 each); DE joins after burn
STAGE = dict(evidence=True, evidence_from=14, evidence_every=2)
W_, T_, D_ = 70, 4, 5


def _selected(it, tskip=7, ev_from=14, every=2):
    return it > ev_from and (it // tskip) % every == 0


def _drive(g, advance, epochs=10, state=None, first=1):
    """``epochs`` swap epochs of 7 iterations; lnL by rank is copied after each, the rule gets the epochs ``PTEngine.swap`` selects.
    Returns the expected (acc, cnt)."""
    seq = []
    for e in range(first, first + epochs):
        advance(7)
        assert g.iter == 7 * e
        if _selected(7 * e):
            seq.append(_by_rank(g))
    if not seq:
        return state
    return ev_rule(np.stack(seq), g.ev_dbeta, state)


def _p0(seed=1):
    return np.random.RandomState(seed).randn(W_, T_, D_) * 0.5


def _dense(d=D_):
    A = np.random.RandomState(3).randn(d, d)
    return ("dense", np.linspace(-0.2, 0.2, d), A @ A.T / d + np.eye(d))


@pytest.fixture(scope="module")
def fused_iso(mods):
    """The fused run with the stage: (engine, its planes) -- computed once, left unchanged."""
    orc, _lib, PTEngine = mods
    g = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, **STAGE, **KW)
    g.init_state(_p0())
    want = _drive(g, g.run)
    return g, want


def test_fused_path_sampling_rule_and_chains_unchanged(mods, fused_iso):
    orc, _lib, PTEngine = mods
    g, (want_acc, want_cnt) = fused_iso
    acc, cnt = _planes(g)
    assert g.ev_epochs == 4 and (cnt[0] == 4).all() and not cnt[1].any()      # iterations 28, 42, 56, 70
    assert_same(cnt, want_cnt, "counts")
    assert_same(acc, want_acc, "planes")
    assert g.swap_proposed == 10 and g.get("nswap").sum() > 0
    assert (g.get("slot_of") != np.arange(T_)).any()                          # the ladder did move: rank and slot differ
    mo = g.evidence_moments()
    assert sorted(mo) == ["betas", "es", "m", "n", "s1", "s2", "shift", "skipped"]
    assert_same(mo["n"], cnt[0], "n")
    assert_same(mo["es"], acc[4], "es")
    assert_same(mo["betas"], 1.0 / g.temps_mh)
    ev = g.evidence()
    assert np.isfinite(ev["lnZ_ss"]) and ev["lnZ_ss_per_walker"].shape == (W_,) and ev["beta_min"] == 1.0 / g.temps_mh[-1]
    # a second engine without the stage: the same chains, bit for bit, and nothing of the stage in it
    b = PTEngine(D_, T_, W_, np.eye(D_) * 0.3, **KW)
    b.init_state(_p0())
    for _ in range(10):
        b.run(7)
    b.sync()
    for name in CHAINS:
        assert_same(g.get(name), b.get(name), name)
    assert "ev_acc" not in b.t and "ev_epochs" not in b.checkpoint() and not b.evidence_on
    with pytest.raises(ValueError, match="evidence=True"):
        b.evidence_moments()


def test_row_path_equals_the_fused_run(mods):
    orc, _lib, PTEngine = mods
    f = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, logl=_dense(), **STAGE, **KW)
    r = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, logl=_dense(), rows_logl=True, **STAGE, **KW)
    want = {}
    for name, g in (("fused", f), ("rows", r)):
        g.init_state(_p0())
        want[name] = _drive(g, g.run)
    for name in CHAINS:
        assert_same(r.get(name), f.get(name), "row path: " + name)            # the chains first
    (fa, fc), (ra, rc) = _planes(f), _planes(r)
    assert_same(rc, fc, "counts")                                             # ... then the accumulators, wherever a state is kept
    assert_same(ra, fa, "planes")
    assert_same(fa, want["fused"][0], "fused dense against the rule")
    assert_same(ra, want["rows"][0], "rows against the rule")
    assert r.ev_epochs == 4 and f.ev_epochs == 4


def test_callback_path(mods, fused_iso):
    orc, _lib, PTEngine = mods
    f, _ = fused_iso
    # the library's own likelihood as a callback: the fused run's chains, and so its accumulators
    c = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, split=True, **STAGE, **KW)
    logl = c.builtin_logl()
    c.init_state_callback(_p0(), logl, None)
    want = _drive(c, lambda n: c.run_callback(n, logl, None))
    for name in CHAINS:
        assert_same(c.get(name), f.get(name), "callback path: " + name)       # the chains first
    (fa, fc), (ca, cc) = _planes(f), _planes(c)
    assert_same(cc, fc, "counts")
    assert_same(ca, fa, "planes")
    assert_same(ca, want[0], "callback path against the rule")

    # a torch expression (its sum rounds in torch's order, not in the step kernels': chains of its own, held to the rule)
    def expr(X):
        return -0.5 * (X * X).sum(-1)

    t = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, split=True, **STAGE, **KW)
    t.init_state_callback(_p0(), expr, None)
    want = _drive(t, lambda n: t.run_callback(n, expr, None))
    ta, tc = _planes(t)
    assert_same(tc, want[1], "torch expression: counts")
    assert_same(ta, want[0], "torch expression: planes")
    assert t.ev_epochs == 4 and (tc[0] == 4).all()
    # ... and every segment as one graph launch (cycles without AM entries are captured): the same chains, the same accumulators
    kw = dict(KW, weights=(20, 0, 20))
    runs = []
    for graph in (False, True):
        e = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, split=True, **STAGE, **kw)
        e.init_state_callback(_p0(), expr, None)
        want = _drive(e, lambda n: e.run_callback(n, expr, None, graph=graph))
        assert_same(_planes(e)[0], want[0], "graph=%r against the rule" % graph)
        runs.append(e)
    assert getattr(runs[1], "_graphs", None), "no segment was captured"
    for name in CHAINS:
        assert_same(runs[1].get(name), runs[0].get(name), "graph: " + name)
    assert_same(_planes(runs[1])[0], _planes(runs[0])[0], "graph: planes")
    assert_same(_planes(runs[1])[1], _planes(runs[0])[1], "graph: counts")


def test_hot_chain_reaches_the_prior(mods):
    orc, _lib, PTEngine = mods
    W, T, d = 5, 4, 3
    g = PTEngine.with_stages(d, T, W, np.eye(d) * 0.3, hot_chain=True, evidence=True, evidence_from=0, **KW)
    assert g.temps_mh[-1] == 1e80
    beta = 1.0 / g.temps_mh
    assert beta[-1] == 1.0 / 1e80 and g.ev_dbeta[-1] == beta[-2] - beta[-1] and g.ev_dbeta[-1] == beta[-2]
    assert g.ev_dbeta[0] == 0.0 and np.array_equal(g.ev_dbeta[1:], beta[:-1] - beta[1:])
    g.init_state(np.random.RandomState(2).randn(W, T, d))
    g.run(7)
    acc, cnt = _planes(g)
    want_acc, want_cnt = ev_rule(_by_rank(g)[None], g.ev_dbeta)
    assert g.ev_epochs == 1
    assert_same(cnt, want_cnt, "counts")
    assert_same(acc, want_acc, "planes")
    assert_same(acc[3][:, -1], beta[-2] * _by_rank(g)[:, -1], "the last stone spans the whole gap to beta = 0")
    mo = g.evidence_moments()
    assert mo["betas"][-1] == 1e-80 and g.evidence()["beta_min"] == 1e-80


def test_checkpoint_resumes_the_accumulators(mods):
    orc, _lib, PTEngine = mods
    W, T, d = 6, 3, 4
    stage = dict(evidence=True, evidence_from=0)
    make = lambda **kw: PTEngine.with_stages(d, T, W, np.eye(d) * 0.3, **kw, **KW)      # noqa: E731
    p0 = np.random.RandomState(4).randn(W, T, d) * 0.5
    a = make(**stage)
    a.init_state(p0)
    a.run(56)
    b = make(**stage)
    b.init_state(p0)
    b.run(28)
    st = b.checkpoint()
    assert st["ev_epochs"] == 4 and st["t_ev_acc"].shape == (5, W, T) and st["t_ev_cnt"].shape == (2, W, T)
    c = make(**stage)
    c.restore(st)
    assert c.ev_epochs == 4
    c.run(28)
    assert a.ev_epochs == 8 and c.ev_epochs == 8
    for name in CHAINS:
        assert_same(c.get(name), a.get(name), "resumed " + name)
    assert_same(_planes(c)[1], _planes(a)[1], "resumed counts")
    assert_same(_planes(c)[0], _planes(a)[0], "resumed planes")
    assert (_planes(a)[1][0] == 8).all()
    # a checkpoint written without the stage is refused before anything is touched
    plain = make()
    plain.init_state(p0)
    plain.run(28)
    before = _planes(c)
    with pytest.raises(ValueError, match="evidence"):
        c.restore(plain.checkpoint())
    assert c.iter == 56 and c.ev_epochs == 8
    assert_same(_planes(c)[0], before[0], "a refused restore touches nothing")


def test_abi_refusals(mods):
    import torch
    orc, _lib, PTEngine = mods
    W, T, d = 4, 3, 2
    g = PTEngine(d, T, W, np.eye(d), tskip=10)
    L = g.lib
    err = lambda: L.ptmi_last_error().decode()      # noqa: E731
    ptr = lambda a: a.ctypes.data_as(_lib._dp)      # noqa: E731
    assert L.ptmi_ev_update(g.h) == -1 and "ptmi_ev_attach" in err()           # PTMI_EINVAL: update before attach
    acc = torch.zeros(5 * W * T + 1, dtype=torch.float64, device=g.device)
    cnt = torch.zeros(2 * W * T + 1, dtype=torch.int64, device=g.device)
    pa, pc = acc.data_ptr(), cnt.data_ptr()
    ok = np.array([0.0, 0.5, 0.25])
    assert L.ptmi_ev_attach(g.h, None, C.c_void_p(pc), ptr(ok)) == -1 and "acc" in err()
    assert L.ptmi_ev_attach(g.h, C.c_void_p(pa + 4), C.c_void_p(pc), ptr(ok)) == -1 and "acc" in err() and "aligned" in err()
    assert L.ptmi_ev_attach(g.h, C.c_void_p(pa), None, ptr(ok)) == -1 and "cnt" in err()
    assert L.ptmi_ev_attach(g.h, C.c_void_p(pa), C.c_void_p(pc + 1), ptr(ok)) == -1 and "cnt" in err() and "aligned" in err()
    assert L.ptmi_ev_attach(g.h, C.c_void_p(pa), C.c_void_p(pc), None) == -1 and "dbeta" in err()
    for bad, at in ((-1e-9, 1), (np.nan, 2), (np.inf, 0), (-np.inf, 2)):
        db = ok.copy()
        db[at] = bad
        assert L.ptmi_ev_attach(g.h, C.c_void_p(pa), C.c_void_p(pc), ptr(db)) == -1 and "dbeta[%d]" % at in err(), (bad, at)
    assert L.ptmi_ev_update(g.h) == -1 and "ptmi_ev_attach" in err()           # none of them attached anything
    _lib.check(L.ptmi_ev_attach(g.h, C.c_void_p(pa), C.c_void_p(pc), ptr(ok)))
    assert L.ptmi_ev_attach(g.h, C.c_void_p(pa), C.c_void_p(pc), ptr(ok)) == -1 and "already" in err()
    torch.cuda.synchronize()
    assert not acc.any().item() and not cnt.any().item()               # a refused call launched nothing
    _lib.check(L.ptmi_ev_update(g.h))
    torch.cuda.synchronize()
    assert cnt[:W * T].tolist() == [1] * (W * T) and int(cnt.sum().item()) == W * T      # lnL = 0 everywhere: one sample each
    assert acc[4 * W * T:5 * W * T].tolist() == [1.0] * (W * T) and acc[-1].item() == 0.0


def _sampler(out, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 4
    kw.setdefault("ntemps", 4)
    s = PTSampler(d, ("iso",), ("box", -5.0 * np.ones(d), 5.0 * np.ones(d)), np.eye(d) * 0.5, outDir=str(out), verbose=False, seed=21,
                  nwalkers=8, **kw)
    s.log_evidence = True
    return s


def test_sampler_delivers_the_estimates_and_resumes(tmp_path):
    from ptmcmcsampler_amd import PTSampler, evidence
    run = dict(burn=100, thin=1, covUpdate=50, isave=50, Tskip=10)
    p0 = np.zeros(4)
    a = _sampler(tmp_path / "a", checkpoint=True)
    a.sample(p0, 300, **run)
    moments = ["betas", "es", "m", "n", "s1", "s2", "shift", "skipped"]
    assert sorted(a.evidence) == sorted(list(evidence.KEYS) + moments)
    assert (a.evidence["n"] == 20).all() and a.evidence["n"].shape == (8, 4) and not a.evidence["skipped"].any()      # swaps at 110 .. 300
    assert a.engine.ev_epochs == 20 and a.engine.evidence_from == 100 and a.engine.evidence_every == 1
    assert np.isfinite([a.evidence[k] for k in ("lnZ_ti", "lnZ_ti_corrected", "lnZ_ss", "lnZ_ss_sem")]).all()
    assert a.evidence["beta_min"] == 1.0 / a.engine.temps_mh[-1] and a.evidence["lnZ_ss_per_walker"].shape == (8,)
    again = evidence.estimates(*(a.evidence[k] for k in ("betas", "n", "shift", "s1", "s2", "m", "es")))
    f = np.load(tmp_path / "a" / "evidence.npz")
    assert sorted(f.files) == sorted(a.evidence)
    for k in f.files:
        assert_same(f[k], a.evidence[k], k)
        if k in again:
            assert_same(again[k], a.evidence[k], "recomputed " + k)
    # stopped at 150 and resumed from its checkpoint: the sums of the uninterrupted run
    b1 = _sampler(tmp_path / "b", checkpoint=True)
    b1.sample(p0, 150, **run)
    assert (b1.evidence["n"] == 5).all()
    b2 = _sampler(tmp_path / "b", checkpoint=True, resume=True)
    b2.sample(p0, 300, **run)
    assert np.array_equal(a._chains, b2._chains)
    for k in f.files:
        assert_same(b2.evidence[k], a.evidence[k], "resumed " + k)
    # every second swap
    e = _sampler(tmp_path / "e")
    e.log_evidence = {"every": 2}
    e.sample(p0, 300, **run)
    assert (e.evidence["n"] == 10).all() and e.engine.evidence_every == 2
    # one temperature: no ladder, no evidence
    one = _sampler(tmp_path / "one", ntemps=1)
    with pytest.raises(ValueError, match="one temperature"):
        one.sample(p0, 100, **run)
    # set after the engine was built
    late = PTSampler(4, ("iso",), ("flat",), np.eye(4) * 0.5, outDir=str(tmp_path / "late"), verbose=False, seed=21, ntemps=2)
    late.sample(p0, 100, **run)
    assert late.evidence is None and not (tmp_path / "late" / "evidence.npz").exists() and not late.engine.evidence_on
    late.log_evidence = True
    with pytest.raises(ValueError, match="before the first sample"):
        late.writeOutput(100)


def test_the_run_measures_ln_z(mods):
    """Iso Gaussian in the box [-5, 5]^4, ladder 2^k (k = 0 .. 10) and the hot rank: exact ln Z = -5.53459, the trapezoid's bias on this
    ladder is -0.204 and the corrected trapezoid's +0.011 (tests/test_evidence.py computes both from the exact moments).  64 walkers
    x 600 samples per chain; with exact independent sampling at these sizes the standard error is 0.008 for all three estimators,
    the cap of 0.05 leaves a factor of six for the chains' autocorrelation.  Measured on an MI355X with this seed: lnZ_ss -5.53369 +- 0.00881,
    lnZ_ti -5.73452 +- 0.00947, lnZ_ti_corrected -5.52039 +- 0.00897."""
    orc, _lib, PTEngine = mods
    d, T, W = 4, 12, 64
    g = PTEngine.with_stages(d, T, W, np.eye(d), ladder=2.0 ** np.arange(T), hot_chain=True, logp=("box", -5.0 * np.ones(d), 5.0 * np.ones(d)),
                             tskip=10, burn=2000, cov_update=1000, seed=2025, evidence=True)
    assert g.evidence_from == 2000 and g.temps_mh[-1] == 1e80 and g.temps_mh[-2] == 1024.0
    g.init_state(np.random.RandomState(0).uniform(-1, 1, (W, T, d)))
    g.run(8000)
    ev = g.evidence()
    mo = g.evidence_moments()
    assert (mo["n"] == 600).all() and not mo["skipped"].any() and g.ev_epochs == 600
    print("lnZ_ss %.5f +- %.5f   lnZ_ti %.5f +- %.5f   lnZ_ti_corrected %.5f +- %.5f   (exact %.5f)" % (
        ev["lnZ_ss"], ev["lnZ_ss_sem"], ev["lnZ_ti"], ev["lnZ_ti_sem"], ev["lnZ_ti_corrected"], ev["lnZ_ti_corrected_sem"], LNZ_BOX))
    assert abs(ev["lnZ_ss"] - LNZ_BOX) < 5 * ev["lnZ_ss_sem"]
    assert abs(ev["lnZ_ti"] - LNZ_BOX - (-0.204)) < 5 * ev["lnZ_ti_sem"]
    assert abs(ev["lnZ_ti_corrected"] - LNZ_BOX) < 5 * ev["lnZ_ti_corrected_sem"] + 0.011
    assert ev["lnZ_ss_sem"] < 0.05
