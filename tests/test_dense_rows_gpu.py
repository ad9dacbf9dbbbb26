"""The built-in dense Gaussian and the built-in priors as ROW kernels (csrc/ptmi_dense_rows.hip: ptmi_rows_logl for PTMI_LOGL_DENSE,
ptmi_rows_logl_grad, ptmi_rows_logp) and the split path driven by them (PTEngine(rows_logl=True), PTSampler's own choice beyond 104-d).

Everything bit for bit: the rows against the oracle's k-ascending fma chains (orc_logl / orc_logl_grad), the engine with
rows_logl=True against the fused kernels AND against OracleEngine.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

DIMS = (1, 2, 3, 15, 16, 17, 40, 100, 104, 105, 112, 113, 200, 416, 417, 512, 513, 1000, 1025)
STATE = ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM", "DE", "cov", "Ut", "S")


def _dense(d, seed, sym=True):
    rs = np.random.RandomState(seed)
    A = rs.randn(d, d)
    P = np.linalg.inv(A @ A.T / d + np.eye(d))
    if not sym:
        P = P + 0.05 * rs.randn(d, d) / np.sqrt(d)       # the value takes the symmetrized half, the gradient Pt as given
    return rs.randn(d) * 0.3, P


def _oracle_rows(orc, o, q):
    L = orc.lib()
    g = np.zeros_like(q)
    v = np.array([L.orc_logl(C.byref(o.cfg), q[i].ctypes.data_as(orc._dp)) for i in range(len(q))])
    vg = np.array([L.orc_logl_grad(C.byref(o.cfg), q[i].ctypes.data_as(orc._dp), g[i].ctypes.data_as(orc._dp)) for i in range(len(q))])
    return v, vg, g


def _special_rows(q, rs):
    """inf, NaN, -0.0 and 1e300 (overflow to inf inside the chain) in some rows; row 0 stays ordinary when there is more than one."""
    n, d = q.shape
    q[n // 2] = -0.0
    for j, val in enumerate((np.inf, np.nan, 1e300, -np.inf, -1e300)):
        r = n - 1 - j
        if r < (1 if n > 1 else 0):
            break
        q[r, rs.randint(d)] = val
    if n > 8:
        q[1, 0] = np.inf                                   # first and last element: before / behind every table row
        q[2, d - 1] = np.nan
        q[3, :] = 1e300
    return q


@pytest.mark.parametrize("d", DIMS)
def test_rows_equal_the_oracle_bit_for_bit(mods, d):
    """ptmi_rows_logl and ptmi_rows_logl_grad against orc_logl / orc_logl_grad row by row: handles made without and with gradient
    jumps (4 / 16 / 64 lanes per chain: another order of the row's dot product), a non-symmetric P, n = 1, 17 and 151 (neither a
    multiple of the 16-row tile nor of 64), ordinary rows and rows with inf, NaN, -0.0 and 1e300.  Both launch layouts (one and two
    row tiles per wave, picked by the number of rows): the rows repeated to a batch of 32919 give the same bits row for row."""
    import torch
    orc, _lib, PTEngine = mods
    cov0 = np.eye(d) * 0.01
    for grad in (False, True):
        if grad and d > 512:
            continue                                       # ptmi_create: gradient jumps are built for ndim <= 512
        for sym in (True, False):
            mu, P = _dense(d, 3 * d + sym, sym)
            kw = dict(logl=("dense", mu, P), weights=(20, 0, 0), tskip=0, grad_weights=(0, 20) if grad else (0, 0))
            g = PTEngine(d, 1, 1, cov0, **kw)
            o = orc.OracleEngine(d, 1, 1, cov0, **kw)
            assert o.lanes == _lib.lanes_for(d, grad=grad)
            fv, fg = g.builtin_logl(), g.builtin_logl_grad()
            for n in (1, 17, 151):
                rs = np.random.RandomState(d + n)
                for special in (False, True):
                    q = mu + rs.randn(n, d)
                    if special:
                        q = _special_rows(q, rs)
                    X = torch.from_numpy(q).to(g.device)
                    v = fv(X).cpu().numpy()
                    vg, gg = fg(X)
                    ov, ovg, og = _oracle_rows(orc, o, q)
                    what = "d=%d grad=%d sym=%d n=%d special=%d " % (d, grad, sym, n, special)
                    assert_same(v, ov, what + "value")
                    assert_same(vg.cpu().numpy(), ovg, what + "value beside the gradient")
                    assert_same(gg.cpu().numpy(), og, what + "gradient")
                    if special and n > 8:
                        assert np.isnan(ov).any() and np.isfinite(ov).any()
                        big = X.repeat(-(-32919 // n), 1)[:32919].contiguous()    # 32768 + 151 rows: two row tiles per wave, a ragged last block
                        idx = np.arange(32919) % n
                        assert_same(fv(big).cpu().numpy(), ov[idx], what + "value, large batch")
                        bv, bg = fg(big)
                        assert_same(bv.cpu().numpy(), ovg[idx], what + "value beside the gradient, large batch")
                        assert_same(bg.cpu().numpy(), og[idx], what + "gradient, large batch")


def test_rows_logl_grad_iso_and_the_families_not_served(mods):
    import torch
    orc, _lib, PTEngine = mods
    d = 37
    g = PTEngine(d, 1, 1, np.eye(d))
    X = torch.randn((70, d), dtype=torch.float64, device=g.device)
    v, gr = g.builtin_logl_grad()(X)
    assert_same(v.cpu().numpy(), g.builtin_logl()(X).cpu().numpy(), "iso value")
    assert_same(gr.cpu().numpy(), (-X).cpu().numpy(), "iso gradient")
    c = PTEngine(6, 1, 1, np.eye(6), logl=("curved",))
    with pytest.raises(_lib.PtmiError):
        c.builtin_logl()(X[:4, :6].contiguous())
    with pytest.raises(_lib.PtmiError):
        c.builtin_logl_grad()(X[:4, :6].contiguous())
    with pytest.raises(ValueError, match="rows_logl"):
        PTEngine(6, 1, 1, np.eye(6), logl=("curved",), rows_logl=True)
    with pytest.raises(ValueError, match="w_host"):
        PTEngine(6, 1, 1, np.eye(6), w_host=2, rows_logl=True)
    with pytest.raises(ValueError, match="ntemps_global"):
        PTEngine(6, 2, 1, np.eye(6), ntemps_global=4, rows_logl=True)


@pytest.mark.parametrize("d", (1, 16, 113, 1000))
def test_rows_logp(mods, d):
    """ptmi_rows_logp against eval_logp's rule: -inf unless lo <= x <= hi in every element; a NaN element gives -inf; values exactly
    on lo / hi are inside; the flat prior is 0 everywhere; the gradient is zeros."""
    import torch
    orc, _lib, PTEngine = mods
    rs = np.random.RandomState(d)
    lo, hi = -1.0 - rs.rand(d), 1.0 + rs.rand(d)
    n = 151
    q = rs.uniform(-1.0, 1.0, (n, d))
    q[1, d - 1] = hi[d - 1] + 1e-9
    q[2, 0] = lo[0] - 1e-9
    q[3, rs.randint(d)] = np.nan
    q[4] = lo
    q[5] = hi
    q[6, d // 2] = np.inf
    q[7, d // 2] = -np.inf
    q[150, 0] = np.nextafter(hi[0], np.inf)
    want = np.array([0.0 if all((lo[i] <= x[i]) and (hi[i] >= x[i]) for i in range(d)) else -np.inf for x in q])
    assert np.isneginf(want[[1, 2, 3, 6, 7, 150]]).all() and (want[[0, 4, 5]] == 0).all()
    g = PTEngine(d, 1, 1, np.eye(d), logp=("box", lo, hi))
    X = torch.from_numpy(q).to(g.device)
    assert_same(g.builtin_logp()(X).cpu().numpy(), want, "box")
    lp, gp = g.builtin_logp_grad()(X)
    assert_same(lp.cpu().numpy(), want, "box beside the gradient")
    assert gp.shape == (n, d) and not gp.any()
    f = PTEngine(d, 1, 1, np.eye(d))
    assert_same(f.builtin_logp()(X).cpu().numpy(), np.zeros(n), "flat")


def _engines(mods, d, nt, W, case, box=False, **kw):
    orc, _lib, PTEngine = mods
    rs = np.random.RandomState(case)
    mu, P = _dense(d, case)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.02
    p0 = mu + rs.randn(W, nt, d) * 0.3
    kw = dict(kw, logl=("dense", mu, P))
    if box:
        p0 = mu + rs.uniform(-0.6, 0.6, (W, nt, d))
        kw["logp"] = ("box", mu - 0.62, mu + 0.62)         # the starts fill the box: proposals of elements near its faces leave it
    r = PTEngine(d, nt, W, cov0, rows_logl=True, **kw)
    f = PTEngine(d, nt, W, cov0, **kw)
    o = orc.OracleEngine(d, nt, W, cov0, **kw)
    for e in (r, f, o):
        e.init_state(p0)
    return r, f, o


def _same_state(r, f, o, what, names=STATE):
    r.sync()
    f.sync()
    for name in names:
        if r.t.get(name) is None:
            continue
        if name == "AM" and getattr(r, "am_rle", False):       # am_mode "rle": the ring keeps the rows of the current covariance period
            lo, hi = r.am_period()
            rows = np.arange(lo, hi + 1) % r.cov_update
            assert_same(r.get("AM")[:, rows], f.get("AM")[:, rows], "%s rows vs fused: AM (current period)" % what)
            assert_same(r.get("AM")[:, rows], o.AM[:, rows], "%s rows vs oracle: AM (current period)" % what)
            continue
        assert_same(r.get(name), f.get(name), "%s rows vs fused: %s" % (what, name))
        if name in ("cov", "Ut", "S", "DE"):
            continue                                       # (the oracle's DE rows are in parameter order; the fused engine's are compared above)
        else:
            assert_same(r.get(name), getattr(o, name), "%s rows vs oracle: %s" % (what, name))


@pytest.mark.parametrize("d,nt,W,kw", [
    (105, 4, 6, {}),
    (113, 3, 5, dict(box=True)),
    # (pooled: am_mode "rows" on all three -- the split path stores every rank-0 row and the pooled statistics sum in the rows' order;
    # the fused path's default "rle" sums the same statistics by run lengths, another order: tests/test_split_rows_gpu.py does the same)
    (200, 4, 6, dict(cov_mode="pooled", am_mode="rows")),
    (200, 4, 6, dict(cov_mode="per_walker")),
    (1000, 3, 5, dict(cov_mode="pooled", am_mode="rows")),
])
def test_split_path_with_the_row_kernels_is_the_fused_path_and_the_oracle(mods, d, nt, W, kw):
    """PTEngine(rows_logl=True).run against the same engine on the fused kernels and against OracleEngine.run: default SCAM / AM / DE
    mix, covariance epochs at 50 and 100, the DE activation at 100, swaps every 10 iterations -- every buffer."""
    r, f, o = _engines(mods, d, nt, W, 7 + d, weights=(20, 20, 20), cov_update=50, burn=100, tskip=10, seed=d, **kw)
    assert r.rows_logl and not f.rows_logl and r.t["Q"] is not None
    _same_state(r, f, o, "init d=%d" % d)
    for n in (60, 90):
        for e in (r, f, o):
            e.run(n)
        _same_state(r, f, o, "d=%d it=%d" % (d, r.iter))
    assert r.swap_proposed == o.swap_proposed and o.nswap.sum() > 0
    js = o.jstat.astype(np.int64)
    assert js[..., 2, 0].sum() > 0 and js[..., 1, 1].sum() > 0            # DE was proposed behind the burn, AM proposals were accepted
    if kw.get("box"):
        assert (js[..., 0].sum(-1) > js[..., 1].sum(-1)).all()


@pytest.mark.parametrize("mode", ("two launches", "graph"))
def test_run_callback_variants_with_the_row_kernels(mods, mode):
    """The built-in callbacks through run_callback(fused=False) (propose / accept as two launches) and run_callback(graph=True)
    (a segment as one captured graph: the row kernels launch on the handle's stream without synchronising): the fused path's bits."""
    d, nt, W = 130, 3, 5
    r, f, o = _engines(mods, d, nt, W, 11, box=True, weights=(20, 0, 20), cov_update=40, burn=80, tskip=8, seed=3)
    logl, logp = r.builtin_logl(), r.builtin_logp()
    for n in (50, 75):
        if mode == "graph":
            r.run_callback(n, logl, logp, graph=True)
        else:
            r.run_callback(n, logl, logp, fused=False)
        f.run(n)
        o.run(n)
        _same_state(r, f, o, "%s it=%d" % (mode, r.iter))
    if mode == "graph":
        assert len(r._graphs) > 0


@pytest.mark.parametrize("d,gw", [(40, (0, 20)), (130, (0, 20)), (40, (20, 10)), (130, (20, 10))])
def test_gradient_jumps_on_the_row_kernels(mods, d, gw):
    """HMC in the cycle, and NUTS + HMC in the cycle (split_nuts): rows_logl=True serves the trajectories' values and gradients from
    ptmi_rows_logl_grad through the batched gradient stage -- against OracleEngine bit for bit, the gj state included."""
    orc, _lib, PTEngine = mods
    nt, W = 2, 3
    rs = np.random.RandomState(d)
    mu, P = _dense(d, d + 1)
    cov0 = np.linalg.inv(P) * 0.5
    p0 = mu + rs.randn(W, nt, d) * 0.3
    kw = dict(logl=("dense", mu, P), weights=(5, 5, 5), grad_weights=gw, hmc=(0.1, 2, 8), nuts_maxdepth=5, cov_update=20, burn=40, tskip=7, seed=17)
    r = PTEngine(d, nt, W, cov0, rows_logl=True, **kw)
    o = orc.OracleEngine(d, nt, W, cov0, **kw)
    assert r.split_nuts == (gw[0] > 0)
    r.init_state(p0)
    o.init_state(p0)
    for n in (30, 35):
        r.run(n)
        o.run(n)
        r.sync()
        for name in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM", "gj"):
            assert_same(r.get(name), getattr(o, name), "d=%d gw=%r it=%d %s" % (d, gw, r.iter, name))
    js = o.jstat.astype(np.int64)
    assert js[..., 4, 1].sum() > 0                                          # HMC proposals were accepted
    if gw[0]:
        assert js[..., 3, 0].sum() > 0                                      # NUTS was picked


def test_sampler_selects_the_row_path_by_itself(mods, tmp_path):
    """PTSampler(200, ("dense", mu, P), ("box", lo, hi), ...) with no option runs the row path; its chain files equal those of the same
    run with rows_logl=False character for character, and it resumes from its checkpoint bit-identically."""
    from ptmcmcsampler_amd import PTSampler
    d = 200
    mu, P = _dense(d, 5)
    lo, hi = mu - 3.0, mu + 3.0
    cov = np.linalg.inv(P) * 0.1
    p0 = mu + 0.1 * np.random.RandomState(1).randn(d)

    def run(out, niter, **kw):
        s = PTSampler(d, ("dense", mu, P), ("box", lo, hi), cov.copy(), ntemps=3, nwalkers=4, outDir=str(out), verbose=False, seed=12, **kw)
        s.sample(p0, niter, isave=100, thin=5, covUpdate=100, burn=200, Tskip=10)
        return s

    a = run(tmp_path / "rows", 400, checkpoint=True)
    assert a.rows_logl and a.engine.rows_logl
    b = run(tmp_path / "fused", 400, rows_logl=False)
    assert not b.rows_logl and not b.engine.rows_logl
    names = sorted(n for n in os.listdir(str(tmp_path / "fused")) if n.endswith(".txt"))
    assert any(n.startswith("chain_1") for n in names)
    for n in names:
        ta, tb = open(str(tmp_path / "rows" / n)).read(), open(str(tmp_path / "fused" / n)).read()
        assert len(tb) > 0 and ta == tb, n
    # stop at 200, resume to 400: the same files as the uninterrupted run
    c = run(tmp_path / "resumed", 200, checkpoint=True)
    assert c.rows_logl
    c2 = run(tmp_path / "resumed", 400, resume=True)
    assert c2.rows_logl and c2.engine.rows_logl
    for n in names:
        if n.startswith("chain_"):                        # (the jump files of a resumed run start at the resume)
            assert open(str(tmp_path / "resumed" / n)).read() == open(str(tmp_path / "rows" / n)).read(), n
    for name in ("X", "lnL", "lp", "nacc", "jstat", "AM"):
        assert_same(c2.engine.get(name), a.engine.get(name), "resumed " + name)


def test_full_size_200d_on_the_row_kernels(mods):
    """200-d dense Gaussian with a known covariance, 64 x 1024 chains, rows_logl=True, default SCAM / AM / DE mix (DE joins at 2001): the
    full launch geometry -- 512 blocks of 128 rows per iteration, the table shared through L2.  At the end ptmi_rows_logl of the state
    equals the stored lnL bit for bit for every chain, 64 seeded rows equal orc_logl, and the 1024 cold states have the target's
    covariance: every entry within 5.5 standard errors, the means within 5 (test_full_size_dense_target_covariance's criterion).
    5000 iterations is the smallest of 5000, 10000, ... at which the criterion held with the largest |z| below 4.5: measured 4.163
    (means: 2.966); at 10000 .. 40000 it stayed between 3.80 and 4.32."""
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 200, 64, 1024
    A = np.random.default_rng(0).standard_normal((d, d))
    Ctrue = A @ A.T / d + np.eye(d)
    kw = dict(weights=(20, 20, 20), cov_update=1000, burn=2000, tskip=100, seed=5, cov_mode="pooled", logl=("dense", np.zeros(d), np.linalg.inv(Ctrue)))
    g = PTEngine(d, nt, W, np.eye(d) * 0.01, rows_logl=True, **kw)
    g.init_state(np.zeros(d))
    g.run(5000)
    g.sync()
    js = g.get("jstat").astype(np.int64)
    assert js[..., 2, 0].sum() > 0 and js[..., 1, 1].sum() > 0 and g.get("nswap").sum() > 0
    lp = g.get("lp")
    assert np.isfinite(lp).all()
    again = g.builtin_logl()(g.t["X"].view(-1, d)).cpu().numpy().reshape(W, nt)
    assert_same(again, g.get("lnL"), "ptmi_rows_logl of the state vs the stored lnL")
    o = orc.OracleEngine(d, 1, 1, np.eye(d) * 0.01, **kw)
    X = g.get("X").reshape(-1, d)
    pick = np.random.RandomState(6).choice(len(X), 64, replace=False)
    L = orc.lib()
    want = np.array([L.orc_logl(C.byref(o.cfg), np.ascontiguousarray(X[i]).ctypes.data_as(orc._dp)) for i in pick])
    assert_same(again.reshape(-1)[pick], want, "64 rows of the state vs orc_logl")
    Xc = g.by_temp("X")[:, 0]
    Chat = Xc.T @ Xc / W
    se = np.sqrt((np.outer(np.diag(Ctrue), np.diag(Ctrue)) + Ctrue ** 2) / W)
    z, zm = np.abs((Chat - Ctrue) / se).max(), np.abs(Xc.mean(0) / np.sqrt(np.diag(Ctrue) / W)).max()
    print("full size 200-d: max |z| of the covariance entries %.3f, of the means %.3f" % (z, zm))
    assert z < 5.5, z
    assert zm < 5.0, zm
