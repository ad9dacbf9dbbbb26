"""Posterior histograms of every cold chain from the AM ring (csrc/ptmi_hist.hip; ``PTEngine.with_stages(hist=(lo, hi, nbins))``,
``PTSampler.posterior_hist``): the device counts equal a NumPy restatement of the rule (tests/test_hist.py ``hist_rule``) applied to
the ring as it was copied before each covariance epoch -- exact integer equality, every row format, both ring modes, clipped runs,
column tiles, the callback path, two rings, the sampler and its checkpoint -- and the stage only reads: the chains are the same bits.

Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _compare, assert_same, mods  # noqa: F401  (mods is a fixture)
from test_hist import hist_rule

pytestmark = pytest.mark.gpu


def _cov0(d, seed=0):
    A = np.random.RandomState(seed).randn(d, d)
    return (A @ A.T / d + 0.5 * np.eye(d)) * 0.01


def _ring(g):
    """The ring in use as it is on the device: rows in parameter order [W][cov_update][d], the flag bits [W][cov_update] or None."""
    g.sync()
    am = g.am_params(g.t["AM"].cpu().numpy())
    fl = g.t["AMflag"].cpu().numpy().view(np.uint64) & np.uint64(3) if g.t["AMflag"] is not None else None
    return am, fl


def _expand(am, fl, base, k_lo, k_hi):
    """Iterations base + k_lo .. base + k_hi of every walker [W][n][d]: a row without NEW / KEY repeats the last stored row before it."""
    cu = am.shape[1]
    out, cur = [], None
    for k in range(1, k_hi + 1):
        r = (base + k) % cu
        if fl is None or cur is None:
            assert fl is None or (fl[:, r] != 0).all(), "ring row 1 of a period is a KEY row"
            cur = am[:, r].copy()
        else:
            cur = np.where((fl[:, r] != 0)[:, None], am[:, r], cur)
        if k >= k_lo:
            out.append(cur.copy())
    return np.stack(out, axis=1)


def _counts(g):
    g.sync()
    return g.t["hist"].cpu().numpy().view(np.uint64)


def _drive(g, advance, periods, bins):
    """``periods`` whole covariance periods from iteration 0, the ring copied at each one's end (the first iteration of the next
    period counts it: update_cov), then one more iteration; returns the NumPy counts of iterations 1 .. periods * cov_update."""
    cu = g.cov_update
    want = np.zeros((g.d, bins[2] + 2), dtype=np.uint64)
    for p in range(periods):
        advance(cu)
        assert g.hist_iter == p * cu
        am, fl = _ring(g)
        want += hist_rule(_expand(am, fl, p * cu, 1, cu), *bins)
    advance(1)
    assert g.hist_iter == periods * cu
    return want


def test_crafted_ring_edge_values(mods):
    orc, _lib, PTEngine = mods
    d, W, cu, nbins = 5, 3, 8, 7
    lo = np.array([0.0, -1.3, 0.1, -2.0, 1e-3])
    hi = np.array([1.0, 2.9, 0.7, 5.0, 1.7e-3])
    g = PTEngine.with_stages(d, 1, W, np.eye(d), cov_update=cu, tskip=0, hist=(lo, hi, nbins), hist_from=0)
    assert g.t["AMflag"] is None                                     # per-walker covariances: every row is stored
    rs = np.random.RandomState(3)
    vals = np.empty((W * cu, d))
    for j in range(d):
        edges = [lo[j] + k * (hi[j] - lo[j]) / nbins for k in range(1, nbins)]
        v = [lo[j], hi[j], np.nextafter(hi[j], -np.inf), np.nextafter(lo[j], -np.inf)] + edges + [np.nextafter(e, -np.inf) for e in edges]
        v += [-0.0, np.inf, -np.inf, np.nan]
        v += list(rs.uniform(lo[j] - 0.1 * (hi[j] - lo[j]), hi[j] + 0.1 * (hi[j] - lo[j]), W * cu - len(v)))
        vals[:, j] = rs.permutation(np.array(v))
    ring = vals.reshape(W, cu, d)
    g.put("AM", ring)
    _lib.check(g.lib.ptmi_hist_update(g.h, 1, cu))
    got = _counts(g)
    assert_same(got, hist_rule(ring, lo, hi, nbins), "crafted ring")
    assert (got.sum(1) == W * cu).all()
    assert got[0, 0] >= 2 and got[0, nbins] == 3 and (got[:, nbins + 1] >= 2).all()      # lo and -0.0 in bin 0; -inf, NaN, below lo; hi and +inf
    # a range inside the period: ring rows 3 .. 5 once more
    _lib.check(g.lib.ptmi_hist_update(g.h, 3, 5))
    assert_same(_counts(g), got + hist_rule(ring[:, 3:6], lo, hi, nbins), "rows 3..5 again")


def test_permuted_row_format_rle_three_periods(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 100, 5, 20
    bins = (-0.4, np.linspace(0.3, 0.5, d), 33)
    g = PTEngine.with_stages(d, 2, W, _cov0(d), weights=(20, 20, 20), cov_update=cu, burn=40, tskip=7, seed=5, cov_mode="pooled",
                             am_mode="rle", hist=bins, hist_from=0)
    assert g.am_pos is not None and g.am_rle
    g.init_state(np.random.RandomState(1).randn(W, 2, d) * 0.1)
    want = _drive(g, g.run, 3, bins)
    assert_same(_counts(g), want, "three periods")
    h = g.hist_counts()                                              # ... and iteration 61
    am, fl = _ring(g)
    want += hist_rule(_expand(am, fl, 3 * cu, 1, 1), *bins)
    assert_same(np.concatenate([h["counts"], h["under"][:, None], h["over"][:, None]], 1), want, "hist_counts")
    assert h["first_iter"] == 1 and h["last_iter"] == 61 and h["nwalkers"] == W and h["edges"].shape == (d, 34)
    assert (want.sum(1) == W * 61).all()
    assert np.array_equal(h["edges"][:, 0], np.full(d, -0.4)) and np.array_equal(h["edges"][:, -1], bins[1])


def test_clipped_runs_and_a_start_inside_a_period(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 37, 4, 30
    rs = np.random.RandomState(4)
    box = ("box", -0.25 - rs.rand(d) * 0.1, 0.2 + rs.rand(d) * 0.1)
    p0 = rs.uniform(-0.05, 0.05, (W, 2, d))
    bins = (-0.3, 0.3, 16)
    kw = dict(weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=10, seed=31, cov_mode="pooled", am_mode="rle", logp=box)
    g = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, hist=bins, hist_from=0, **kw)
    g.init_state(p0)
    g.run(2 * cu)                                                    # iteration 31 counted the first period
    am, fl = _ring(g)
    assert (fl == 0).any(), "the tight prior must leave rows that were not stored"
    first = _counts(g).copy()
    # a mid-period iteration whose row is not stored for a walker and whose successor is not stored for a walker either: the run
    # under way there is cut by the first call and picked up by the second
    mids = [k for k in range(3, cu - 2) if ((fl[:, k] == 0) & (fl[:, k + 1] == 0)).any()]
    assert mids, "no run crosses a mid-period iteration: the test needs one"
    k = mids[len(mids) // 2]
    g.hist_sync(cu + k)
    assert g.hist_iter == cu + k
    assert_same(_counts(g), first + hist_rule(_expand(am, fl, cu, 1, k), *bins), "up to the middle")
    g.hist_sync(cu + k)                                              # again: nothing to count
    g.run(1)                                                         # the period's end counts the rest
    whole = first + hist_rule(_expand(am, fl, cu, 1, cu), *bins)
    assert_same(_counts(g), whole, "middle + rest = the whole period")
    assert (whole.sum(1) == W * 2 * cu).all()
    # the weights on the device are run lengths: the same counts from the stored rows alone, weighted
    rows = _expand(am, fl, cu, 1, cu)
    stored = np.stack([fl[:, (cu + kk) % cu] != 0 for kk in range(1, cu + 1)], 1)
    runs = np.zeros(stored.shape, dtype=np.int64)
    for w in range(W):
        idx = np.flatnonzero(stored[w])
        runs[w, idx] = np.diff(np.append(idx, cu))
    assert_same(hist_rule(rows, *bins, weight=runs), hist_rule(rows, *bins), "run-length weights")
    # a second engine that starts counting inside the second period: the same chains (the stage only reads)
    start = cu + 11
    e = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, hist=bins, hist_from=start, **kw)
    e.init_state(p0)
    e.run(2 * cu + 1)
    assert e.hist_iter == 2 * cu
    assert_same(_counts(e), hist_rule(_expand(am, fl, cu, 12, cu), *bins), "hist_from inside a period")
    assert e.hist_counts(2 * cu)["first_iter"] == start + 1
    with pytest.raises(ValueError, match="no longer in the ring"):
        f = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, hist=bins, hist_from=0, **kw)
        f.iter = cu + 1                                              # stepped from outside, past an epoch that never went through update_cov
        f.hist_sync(cu + 1)                                          # the first period was never counted
    with pytest.raises(ValueError, match="has reached iteration"):
        e.hist_sync(e.iter + 1)                                      # the ring's rows beyond the engine's iteration are the period before's
    assert e.hist_iter == 2 * cu


@pytest.mark.parametrize("d,W,mode,nbins", [(130, 3, "per_walker", 1024), (200, 3, "pooled", 1024), (1, 4, "per_walker", 2), (2048, 2, "pooled", 2),
                                            (1000, 2, "pooled", 64)])
def test_column_tiles(mods, d, W, mode, nbins):
    orc, _lib, PTEngine = mods
    cu = 12
    bins = (-0.35, 0.3, nbins)
    g = PTEngine.with_stages(d, 1, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=d, cov_mode=mode,
                             hist=bins, hist_from=2)
    assert _lib.lanes_for(d) == {130: 16, 200: 16, 1: 4, 2048: 64, 1000: 64}[d]      # every kernel shape writes the ring its way
    g.init_state(np.random.RandomState(d).randn(W, 1, d) * 0.2)
    g.run(cu)
    h = g.hist_counts()                                              # inside the period: no epoch
    am, fl = _ring(g)
    assert (fl is not None) == (mode == "pooled")
    want = hist_rule(_expand(am, fl, 0, 3, cu), *bins)
    assert_same(np.concatenate([h["counts"], h["under"][:, None], h["over"][:, None]], 1), want, "d=%d" % d)
    assert (want.sum(1) == W * (cu - 2)).all() and want[:, :nbins].sum() > 0


def test_callback_path_and_two_rings(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu = 24, 6, 16
    bins = (np.linspace(-0.5, -0.3, d), 0.4, 21)
    p0 = np.random.RandomState(2).randn(W, 2, d) * 0.1

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    g = PTEngine.with_stages(d, 2, W, _cov0(d), weights=(20, 20, 0), cov_update=cu, burn=1000, tskip=5, seed=8, cov_mode="pooled",
                             split=True, hist=bins, hist_from=0)
    g.init_state_callback(p0, logl, None)
    want = _drive(g, lambda n: g.run_callback(n, logl, None), 3, bins)
    assert_same(_counts(g), want, "run_callback")
    assert isinstance(g.t["hist"], torch.Tensor)
    a = PTEngine.with_stages(d, 2, W, _cov0(d), weights=(20, 20, 0), cov_update=cu, burn=1000, tskip=5, seed=8, cov_mode="pooled",
                             stats_async=True, eig_lag=1, hist=bins, hist_from=0)
    assert a.stats_async
    a.init_state(p0)
    want = _drive(a, a.run, 4, bins)
    assert_same(_counts(a), want, "two rings")


def test_the_stage_only_reads(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 100, 4, 20
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=40, tskip=10, seed=3, cov_mode="pooled")
    p0 = np.random.RandomState(5).randn(W, 3, d) * 0.1
    a = PTEngine.with_stages(d, 3, W, _cov0(d), hist=(-1.0, 1.0, 50), hist_from=0, **kw)
    b = PTEngine(d, 3, W, _cov0(d), **kw)
    for g in (a, b):
        g.init_state(p0)
        g.run(3 * cu + 1)
    assert _counts(a).sum() == d * W * 3 * cu
    for name in ("X", "lnL", "lp", "nacc", "jstat", "nswap", "mu", "M2", "cov", "Ut", "S", "DE", "AM"):
        assert_same(a.get(name), b.get(name), name)
    assert "hist" not in b.t and "hist_iter" not in b.checkpoint()


def test_against_the_oracle(mods):
    orc, _lib, PTEngine = mods
    d, nt, W, cu = 6, 3, 4, 25
    bins = (-1.5, 1.5, 30)
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=50, tskip=10, seed=12)
    cov0 = _cov0(d) * 20
    p0 = np.random.RandomState(7).randn(W, nt, d) * 0.3
    g = PTEngine.with_stages(d, nt, W, cov0, hist=bins, hist_from=0, **kw)
    o = orc.OracleEngine(d, nt, W, cov0, **kw)
    g.init_state(p0)
    o.init_state(p0)
    want = np.zeros((d, 32), dtype=np.uint64)
    for p in range(3):
        o.run(cu)
        want += hist_rule(_expand(np.array(o.AM), None, p * cu, 1, cu), *bins)      # the oracle's own ring: every row stored
    o.run(1)
    g.run(3 * cu + 1)
    _compare(g, o, "hist twin ")
    assert_same(_counts(g), want, "against the oracle's ring")
    assert (want.sum(1) == W * 3 * cu).all()


def test_a_hot_block_counts_nothing(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 8, 3, 10
    g = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=2, ntemps_global=4,
                             temp0=2, hist=(-1.0, 1.0, 12), hist_from=0)
    assert not g.owns_cold and g.t["AM"] is None
    g.init_state(np.zeros((W, 2, d)))
    g.run(2 * cu + 3)
    assert g.lib.ptmi_hist_update(g.h, 2 * cu + 1, 2 * cu + 3) == 0
    assert g.lib.ptmi_hist_update(g.h, 1, 2 * cu) == 0               # not even the range is looked at, as ptmi_update_cov
    h = g.hist_counts()
    assert not _counts(g).any() and h["counts"].shape == (d, 12) and not h["under"].any()


def test_refusals(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu = 5, 2, 8
    g = PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0)
    L = g.lib
    err = lambda: L.ptmi_last_error().decode()      # noqa: E731
    assert L.ptmi_hist_update(g.h, 1, 2) == -1 and "ptmi_hist_attach" in err()      # PTMI_EINVAL: update before attach
    buf = torch.zeros(d * (1025 + 2) + 1, dtype=torch.int64, device=g.device)      # counts [d][nbins + 2] of the attach that succeeds: its first d * 10 words
    lo, sc = np.zeros(d), np.ones(d)
    ptr = lambda a: a.ctypes.data_as(_lib._dp)      # noqa: E731
    for nbins in (1, 1025, 0, -4):
        assert L.ptmi_hist_attach(g.h, C.c_void_p(buf.data_ptr()), ptr(lo), ptr(sc), nbins) == -1 and "nbins" in err()
    assert L.ptmi_hist_attach(g.h, C.c_void_p(buf.data_ptr() + 4), ptr(lo), ptr(sc), 8) == -1 and "aligned" in err()
    assert L.ptmi_hist_attach(g.h, None, ptr(lo), ptr(sc), 8) == -1
    for bad in (0.0, -1.0, np.inf, np.nan):
        s2 = sc.copy()
        s2[3] = bad
        assert L.ptmi_hist_attach(g.h, C.c_void_p(buf.data_ptr()), ptr(lo), ptr(s2), 8) == -1 and "parameter 3" in err()
    assert L.ptmi_hist_update(g.h, 1, 2) == -1 and "ptmi_hist_attach" in err()      # none of them attached anything
    _lib.check(L.ptmi_hist_attach(g.h, C.c_void_p(buf.data_ptr()), ptr(lo), ptr(sc), 8))
    assert L.ptmi_hist_attach(g.h, C.c_void_p(buf.data_ptr()), ptr(lo), ptr(sc), 8) == -1 and "already" in err()
    for a, b in ((cu, cu + 1), (1, cu + 1), (cu - 2, 2 * cu), (0, 3), (-2, 1)):
        assert L.ptmi_hist_update(g.h, a, b) == -1 and "period" in err(), (a, b)
    torch.cuda.synchronize()
    assert not buf.any().item()                                      # a refused call launched nothing
    assert L.ptmi_hist_update(g.h, 5, 4) == 0                        # iter_hi < iter_lo: nothing to do
    assert L.ptmi_hist_update(g.h, cu + 1, 2 * cu) == 0 and L.ptmi_hist_update(g.h, cu, cu) == 0
    torch.cuda.synchronize()
    assert buf[:d * 10].view(d, 10)[:, 0].tolist() == [W * (cu + 1)] * d                # a ring of zeros with lo = 0: bin 0
    assert int(buf.sum().item()) == d * W * (cu + 1)


def _sampler(out, W, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 4
    s = PTSampler(d, ("iso",), ("box", -3.0 * np.ones(d), 3.0 * np.ones(d)), np.eye(d) * 0.5, outDir=str(out), verbose=False, seed=21, ntemps=2,
                  nwalkers=W, keep_walkers=W, **kw)
    s.posterior_hist = (np.array([-3.0, -2.0, -1.0, -0.5]), np.array([3.0, 2.0, 1.0, 0.5]), 24)
    return s


def test_sampler_counts_equal_the_harvested_chains_and_resume(tmp_path):
    W = 6
    run = dict(burn=100, thin=1, covUpdate=50, isave=50, Tskip=10)
    p0 = np.zeros(4)
    a = _sampler(tmp_path / "a", W, checkpoint=True)
    a.sample(p0, 300, **run)
    lo, hi, nbins = a.posterior_hist
    want = hist_rule(a._chains[:, 101:301], lo, hi, nbins)           # the harvested chains: another path out of the ring (_harvest)
    got = np.concatenate([a.hist["counts"], a.hist["under"][:, None], a.hist["over"][:, None]], 1)
    assert_same(got, want, "sampler.hist")
    assert a.hist["last_iter"] == 300 and a.hist["first_iter"] == 101 and a.hist["nwalkers"] == W
    assert (got.sum(1) == W * 200).all() and got[3, nbins:].sum() > 0        # the narrow range of parameter 3 leaves samples outside
    f = np.load(tmp_path / "a" / "hist.npz")
    assert sorted(f.files) == ["counts", "edges", "first_iter", "last_iter", "nwalkers", "over", "under"]
    for k in f.files:
        assert_same(f[k], a.hist[k], k)
    assert f["counts"].dtype == np.uint64 and int(f["last_iter"]) == 300
    # stopped at 150 and resumed from its checkpoint: the counts of the uninterrupted run
    b1 = _sampler(tmp_path / "b", W, checkpoint=True)
    b1.sample(p0, 150, **run)
    assert b1.hist["last_iter"] == 150 and (b1.hist["counts"].sum(1) + b1.hist["under"] + b1.hist["over"] == W * 50).all()
    b2 = _sampler(tmp_path / "b", W, checkpoint=True, resume=True)
    b2.sample(p0, 300, **run)
    assert np.array_equal(a._chains, b2._chains)
    for k in f.files:
        assert_same(b2.hist[k], a.hist[k], "resumed " + k)
    # a run without the attribute writes no file and has no histogram
    from ptmcmcsampler_amd import PTSampler
    c = PTSampler(4, ("iso",), ("flat",), np.eye(4) * 0.5, outDir=str(tmp_path / "c"), verbose=False, seed=21)
    c.sample(p0, 100, burn=50, thin=1, covUpdate=50, isave=50)
    assert c.hist is None and not (tmp_path / "c" / "hist.npz").exists() and c.engine.hist_spec is None

