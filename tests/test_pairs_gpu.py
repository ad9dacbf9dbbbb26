"""Joint posterior histograms of parameter pairs from the AM ring (csrc/ptmi_pairs.hip; ``PTEngine.with_stages(pairs=(pairs, lo, hi,
nbins))``, ``PTSampler.posterior_pairs``): the device counts equal the NumPy restatement of the rule (ptmcmcsampler_amd/pairs.py
``pairs_rule``) applied to the ring as it was copied before each covariance epoch -- exact integer equality, every row format, both
ring modes, clipped runs, pair tiles, slab edges, the callback path, two rings, the 1-D stage beside it, the sampler and its
checkpoint -- and the stage only reads: the chains are the same bits.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from ptmcmcsampler_amd.pairs import expand_pairs, pairs_rule
from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)
from test_hist_gpu import _cov0, _expand, _ring

pytestmark = pytest.mark.gpu


def _counts(g):
    g.sync()
    return g.t["pairs"].cpu().numpy().view(np.uint64)


def _flat(h):
    """``pairs_counts()`` back in the device's layout [npairs][nbins * nbins + 1]."""
    return np.concatenate([h["counts"].reshape(len(h["counts"]), -1), h["outside"][:, None]], 1)


def _drive(g, advance, periods, spec):
    """``periods`` whole covariance periods from iteration 0, the ring copied at each one's end (the first iteration of the next
    period counts it: update_cov), then one more iteration; returns the NumPy counts of iterations 1 .. periods * cov_update."""
    cu = g.cov_update
    want = 0
    for p in range(periods):
        advance(cu)
        assert g.pairs_iter == p * cu
        am, fl = _ring(g)
        want = want + pairs_rule(_expand(am, fl, p * cu, 1, cu), *spec)
    advance(1)
    assert g.pairs_iter == periods * cu
    return want


def test_crafted_ring_edge_values(mods):
    orc, _lib, PTEngine = mods
    d, W, cu, nbins = 3, 4, 100, 4
    lo, hi = np.array([0.0, -1.3, 0.1]), np.array([1.0, 2.9, 0.7])
    pairs = [[0, 1], [1, 2], [2, 0], [0, 2]]
    g = PTEngine.with_stages(d, 1, W, np.eye(d), cov_update=cu, tskip=0, pairs=(pairs, lo, hi, nbins), pairs_from=0)
    assert g.t["AMflag"] is None                                     # per-walker covariances: every row is stored
    rs = np.random.RandomState(3)
    sp = []
    for j in range(d):
        edges = [lo[j] + k * (hi[j] - lo[j]) / nbins for k in range(1, nbins)]
        sp.append(np.array([lo[j], hi[j], np.nextafter(hi[j], -np.inf), np.nextafter(lo[j], -np.inf)] + edges
                           + [np.nextafter(e, -np.inf) for e in edges] + [-0.0, np.inf, -np.inf, np.nan]))
    n = len(sp[0])                                                   # 14 special values an axis
    mid = 0.5 * (lo + hi)
    rows = [[sp[0][a], sp[1][b], sp[2][(a + b) % n]] for a in range(n) for b in range(n)]      # on two axes (and the third) at once
    for j in range(d):                                               # on one axis, the others inside
        for v in sp[j]:
            r = mid + 0.1 * (hi - lo) * rs.randn(d)
            r[j] = v
            rows.append(list(r))
    rows = np.array(rows)
    assert len(rows) <= W * cu
    fill = rs.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (W * cu - len(rows), d))
    ring = rs.permutation(np.concatenate([rows, fill])).reshape(W, cu, d)
    g.put("AM", ring)
    _lib.check(g.lib.ptmi_pairs_update(g.h, 1, cu))
    got = _counts(g)
    want = pairs_rule(ring, pairs, lo, hi, nbins)
    assert_same(got, want, "crafted ring")
    assert (got.sum(1) == W * cu).all() and (got[:, -1] >= n).all() and got[0, 0] >= 2      # (lo, lo) and (-0.0, lo) in cell 0
    t = lambda row: row[:-1].reshape(nbins, nbins)      # noqa: E731
    assert np.array_equal(t(got[2]), t(got[3]).T) and got[2, -1] == got[3, -1]      # (2, 0) is the transpose of (0, 2)
    # a range inside the period: ring rows 3 .. 5 once more
    _lib.check(g.lib.ptmi_pairs_update(g.h, 3, 5))
    assert_same(_counts(g), got + pairs_rule(ring[:, 3:6], pairs, lo, hi, nbins), "rows 3..5 again")


def test_permuted_row_format_rle_three_periods(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 100, 8, 20
    pairs = [[0, 99], [99, 0], [17, 50], [50, 73], [73, 0], [99, 17]]
    spec = (pairs, -0.4, np.linspace(0.3, 0.5, d), 33)
    g = PTEngine.with_stages(d, 2, W, _cov0(d), weights=(20, 20, 20), cov_update=cu, burn=40, tskip=7, seed=5, cov_mode="pooled",
                             am_mode="rle", pairs=spec, pairs_from=0)
    assert g.am_pos is not None and g.am_rle
    g.init_state(np.random.RandomState(1).randn(W, 2, d) * 0.1)
    want = _drive(g, g.run, 3, spec)
    assert_same(_counts(g), want, "three periods")
    h = g.pairs_counts()                                             # ... and iteration 61
    am, fl = _ring(g)
    want = want + pairs_rule(_expand(am, fl, 3 * cu, 1, 1), *spec)
    assert_same(_flat(h), want, "pairs_counts")
    assert h["first_iter"] == 1 and h["last_iter"] == 61 and h["nwalkers"] == W and h["edges"].shape == (d, 34)
    assert h["counts"].shape == (6, 33, 33) and h["counts"].dtype == np.uint64 and h["pairs"].tolist() == pairs
    assert (want.sum(1) == W * 61).all() and want[:, :-1].sum() > 0
    assert np.array_equal(h["counts"][0], h["counts"][1].T)


def test_clipped_runs_and_a_start_inside_a_period(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 37, 4, 30
    rs = np.random.RandomState(4)
    box = ("box", -0.25 - rs.rand(d) * 0.1, 0.2 + rs.rand(d) * 0.1)
    p0 = rs.uniform(-0.05, 0.05, (W, 2, d))
    spec = ({"params": [0, 36, 11, 5]}, -0.3, 0.3, 16)
    kw = dict(weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=10, seed=31, cov_mode="pooled", am_mode="rle", logp=box)
    g = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, pairs=spec, pairs_from=0, **kw)
    g.init_state(p0)
    g.run(2 * cu)                                                    # iteration 31 counted the first period
    am, fl = _ring(g)
    assert (fl == 0).any(), "the tight prior must leave rows that were not stored"
    first = _counts(g).copy()
    assert (first.sum(1) == W * cu).all()
    # a mid-period iteration whose row is not stored for a walker and whose successor is not stored for a walker either: the run
    # under way there is cut by the first call and picked up by the second
    mids = [k for k in range(3, cu - 2) if ((fl[:, k] == 0) & (fl[:, k + 1] == 0)).any()]
    assert mids, "no run crosses a mid-period iteration: the test needs one"
    k = mids[len(mids) // 2]
    g.pairs_sync(cu + k)
    assert g.pairs_iter == cu + k
    assert_same(_counts(g), first + pairs_rule(_expand(am, fl, cu, 1, k), *spec), "up to the middle")
    g.pairs_sync(cu + k)                                             # again: nothing to count
    g.run(1)                                                         # the period's end counts the rest
    whole = first + pairs_rule(_expand(am, fl, cu, 1, cu), *spec)
    assert_same(_counts(g), whole, "middle + rest = the whole period")
    assert (whole.sum(1) == W * 2 * cu).all()
    # a second engine that starts counting inside the second period: the same chains (the stage only reads)
    start = cu + 11
    e = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, pairs=spec, pairs_from=start, **kw)
    e.init_state(p0)
    e.run(2 * cu + 1)
    assert e.pairs_iter == 2 * cu
    assert_same(_counts(e), pairs_rule(_expand(am, fl, cu, 12, cu), *spec), "pairs_from inside a period")
    assert e.pairs_counts(2 * cu)["first_iter"] == start + 1
    with pytest.raises(ValueError, match="no longer in the ring"):
        f = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, pairs=spec, pairs_from=0, **kw)
        f.iter = cu + 1                                              # stepped from outside, past an epoch that never went through update_cov
        f.pairs_sync(cu + 1)                                         # the first period was never counted
    with pytest.raises(ValueError, match="has reached iteration"):
        e.pairs_sync(e.iter + 1)                                     # the ring's rows beyond the engine's iteration are the period before's
    assert e.pairs_iter == 2 * cu
    with pytest.raises(ValueError, match="no pair histogram"):
        PTEngine(d, 2, W, np.eye(d) * 0.01, **kw).pairs_sync(0)


# d, W, mode, pairs, nbins: a table that fills a tile almost alone and several tiles; many pairs per tile and more columns than a tile holds (all
# 4950 pairs of 100-d: a tile's columns are capped by its bin bytes); tiles that share columns; the 16- and 64-lane rows
TILES = [(100, 3, "pooled", [[3, 98], [98, 3], [41, 0]], 128),
         (100, 3, "pooled", {"params": list(range(100))}, 2),
         (37, 3, "per_walker", {"params": [36, 0, 7, 8, 9, 20, 21, 30, 1, 15]}, 32),
         (130, 3, "per_walker", {"params": [129, 0, 64, 65]}, 32),
         (420, 2, "pooled", {"params": [419, 0, 1, 255, 256, 300]}, 24)]


@pytest.mark.parametrize("d,W,mode,pairs,nbins", TILES, ids=["nbins128", "all4950", "shared-columns", "130d", "420d"])
def test_pair_tiles_and_row_shapes(mods, d, W, mode, pairs, nbins):
    orc, _lib, PTEngine = mods
    cu = 12
    spec = (pairs, -0.35, 0.3, nbins)
    g = PTEngine.with_stages(d, 1, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=d, cov_mode=mode,
                             pairs=spec, pairs_from=2)
    assert _lib.lanes_for(d) == {100: 4, 37: 4, 130: 16, 420: 64}[d]      # every kernel shape writes the ring its way
    g.init_state(np.random.RandomState(d).randn(W, 1, d) * 0.2)
    g.run(cu)
    h = g.pairs_counts()                                             # inside the period: no epoch
    am, fl = _ring(g)
    assert (fl is not None) == (mode == "pooled")
    want = pairs_rule(_expand(am, fl, 0, 3, cu), *spec)
    assert_same(_flat(h), want, "d=%d nbins=%d" % (d, nbins))
    assert len(want) == len(expand_pairs(d, pairs)) and (want.sum(1) == W * (cu - 2)).all() and want[:, :-1].sum() > 0


@pytest.mark.parametrize("W,cu,npairs", [(3, 341, 2), (4, 256, 2), (5, 205, 2), (80, 900, 8)], ids=["1023", "1024", "1025", "72000"])
def test_slab_edges_and_more_slabs_than_blocks(mods, W, cu, npairs):
    """Rings of one slab less a row, one slab, one slab and a row; and 71 slabs for the 64 blocks a tile gets where four tiles
    (two pairs each at nbins = 128) share the launch's 256."""
    orc, _lib, PTEngine = mods
    d, nbins = 4, 128
    pairs = [[0, 1], [2, 3], [1, 0], [3, 0], [1, 2], [2, 0], [3, 1], [0, 3]][:npairs]
    g = PTEngine.with_stages(d, 1, W, np.eye(d), cov_update=cu, tskip=0, pairs=(pairs, -1.0, 1.0, nbins), pairs_from=0)
    ring = np.random.RandomState(cu).uniform(-1.1, 1.1, (W, cu, d))
    g.put("AM", ring)
    _lib.check(g.lib.ptmi_pairs_update(g.h, 1, cu))
    got = _counts(g)
    assert_same(got, pairs_rule(ring, pairs, -1.0, 1.0, nbins), "%d rows" % (W * cu))
    assert (got.sum(1) == W * cu).all()
    _lib.check(g.lib.ptmi_pairs_update(g.h, cu, cu))                 # the period's last iteration sits in ring row 0
    assert_same(_counts(g), got + pairs_rule(ring[:, 0], pairs, -1.0, 1.0, nbins), "ring row 0 again")


def test_callback_path_and_two_rings(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu = 24, 6, 16
    spec = ({"params": [0, 23, 5, 12]}, np.linspace(-0.5, -0.3, d), 0.4, 21)
    p0 = np.random.RandomState(2).randn(W, 2, d) * 0.1

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    g = PTEngine.with_stages(d, 2, W, _cov0(d), weights=(20, 20, 0), cov_update=cu, burn=1000, tskip=5, seed=8, cov_mode="pooled",
                             split=True, pairs=spec, pairs_from=0)
    g.init_state_callback(p0, logl, None)
    want = _drive(g, lambda n: g.run_callback(n, logl, None), 3, spec)
    assert_same(_counts(g), want, "run_callback")
    assert isinstance(g.t["pairs"], torch.Tensor)
    a = PTEngine.with_stages(d, 2, W, _cov0(d), weights=(20, 20, 0), cov_update=cu, burn=1000, tskip=5, seed=8, cov_mode="pooled",
                             stats_async=True, eig_lag=1, pairs=spec, pairs_from=0)
    assert a.stats_async
    a.init_state(p0)
    want = _drive(a, a.run, 4, spec)
    assert_same(_counts(a), want, "two rings")


def test_the_stage_only_reads_and_agrees_with_the_marginals(mods):
    orc, _lib, PTEngine = mods
    d, W, cu, nbins = 100, 4, 20, 50
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=40, tskip=10, seed=3, cov_mode="pooled")
    p0 = np.random.RandomState(5).randn(W, 3, d) * 0.1
    par = [99, 0, 42, 57]
    # a box that contains every sample (a unit Gaussian's chains, the cycle's ten-fold jumps included, stay far inside 8 sigma): no
    # pair has a row outside, so a table's margins are the 1-D stage's rows
    a = PTEngine.with_stages(d, 3, W, _cov0(d), pairs=({"params": par}, -8.0, 8.0, nbins), pairs_from=0, hist=(-8.0, 8.0, nbins), hist_from=0, **kw)
    b = PTEngine(d, 3, W, _cov0(d), **kw)
    for g in (a, b):
        g.init_state(p0)
        g.run(3 * cu + 1)
    for name in ("X", "lnL", "lp", "nacc", "jstat", "nswap", "mu", "M2", "cov", "Ut", "S", "DE", "AM"):
        assert_same(a.get(name), b.get(name), name)
    assert "pairs" not in b.t and "pairs_iter" not in b.checkpoint() and b.pairs_spec is None
    h2, h1 = a.pairs_counts(3 * cu), a.hist_counts(3 * cu)
    assert not h2["outside"].any() and not h1["under"].any() and not h1["over"].any(), (h2["outside"], h1["under"][par], h1["over"][par])
    assert (h2["counts"].sum((1, 2)) == W * 3 * cu).all()
    for p, (i, j) in enumerate(h2["pairs"]):
        assert_same(h2["counts"][p].sum(1), h1["counts"][i], "pair (%d, %d) summed over j" % (i, j))
        assert_same(h2["counts"][p].sum(0), h1["counts"][j], "pair (%d, %d) summed over i" % (i, j))
    assert_same(h1["edges"], h2["edges"], "edges")
    assert (h2["counts"] > 0).sum() > 6                              # (the samples are spread over cells)


def test_a_hot_block_counts_nothing(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 8, 3, 10
    g = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=2, ntemps_global=4,
                             temp0=2, pairs=([[0, 7], [3, 4]], -1.0, 1.0, 12), pairs_from=0)
    assert not g.owns_cold and g.t["AM"] is None
    g.init_state(np.zeros((W, 2, d)))
    g.run(2 * cu + 3)
    assert g.lib.ptmi_pairs_update(g.h, 2 * cu + 1, 2 * cu + 3) == 0
    assert g.lib.ptmi_pairs_update(g.h, 1, 2 * cu) == 0              # not even the range is looked at, as ptmi_update_cov
    h = g.pairs_counts()
    assert not _counts(g).any() and h["counts"].shape == (2, 12, 12) and not h["outside"].any()


def test_refusals(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu = 5, 2, 8
    g = PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0)
    L = g.lib
    err = lambda: L.ptmi_last_error().decode()      # noqa: E731
    assert L.ptmi_pairs_update(g.h, 1, 2) == -1 and "ptmi_pairs_attach" in err()      # PTMI_EINVAL: update before attach
    buf = torch.zeros(2 * 65 + 1, dtype=torch.int64, device=g.device)      # counts [2][8 * 8 + 1] of the attach that succeeds
    lo, sc = np.zeros(d), np.ones(d)
    pr = np.array([[0, 1], [4, 2]], dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib._dp)      # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    cnt = C.c_void_p(buf.data_ptr())
    for nbins in (1, 129, 0, -4, 1024):
        assert L.ptmi_pairs_attach(g.h, cnt, ip(pr), 2, ptr(lo), ptr(sc), nbins) == -1 and "nbins" in err()
    for npairs in (0, -1, 8193):
        assert L.ptmi_pairs_attach(g.h, cnt, ip(pr), npairs, ptr(lo), ptr(sc), 8) == -1 and "npairs" in err()
    assert L.ptmi_pairs_attach(g.h, C.c_void_p(buf.data_ptr() + 4), ip(pr), 2, ptr(lo), ptr(sc), 8) == -1 and "aligned" in err()
    assert L.ptmi_pairs_attach(g.h, None, ip(pr), 2, ptr(lo), ptr(sc), 8) == -1
    assert L.ptmi_pairs_attach(g.h, cnt, None, 2, ptr(lo), ptr(sc), 8) == -1
    for bad in ([0, 0], [0, 5], [-1, 2], [5, 0], [3, 3]):
        p2 = pr.copy()
        p2[1] = bad
        assert L.ptmi_pairs_attach(g.h, cnt, ip(p2), 2, ptr(lo), ptr(sc), 8) == -1 and "pair 1" in err(), bad
    for bad in (0.0, -1.0, np.inf, np.nan):
        s2 = sc.copy()
        s2[3] = bad
        assert L.ptmi_pairs_attach(g.h, cnt, ip(pr), 2, ptr(lo), ptr(s2), 8) == -1 and "parameter 3" in err()
    for bad in (np.inf, -np.inf, np.nan):
        l2 = lo.copy()
        l2[1] = bad
        assert L.ptmi_pairs_attach(g.h, cnt, ip(pr), 2, ptr(l2), ptr(sc), 8) == -1 and "parameter 1" in err()
    assert L.ptmi_pairs_update(g.h, 1, 2) == -1 and "ptmi_pairs_attach" in err()      # none of them attached anything
    _lib.check(L.ptmi_pairs_attach(g.h, cnt, ip(pr), 2, ptr(lo), ptr(sc), 8))
    assert L.ptmi_pairs_attach(g.h, cnt, ip(pr), 2, ptr(lo), ptr(sc), 8) == -1 and "already" in err()
    for a, b in ((cu, cu + 1), (1, cu + 1), (cu - 2, 2 * cu), (0, 3), (-2, 1)):
        assert L.ptmi_pairs_update(g.h, a, b) == -1 and "period" in err(), (a, b)
    torch.cuda.synchronize()
    assert not buf.any().item()                                      # a refused call launched nothing
    assert L.ptmi_pairs_update(g.h, 5, 4) == 0                       # iter_hi < iter_lo: nothing to do
    assert L.ptmi_pairs_update(g.h, cu + 1, 2 * cu) == 0 and L.ptmi_pairs_update(g.h, cu, cu) == 0
    torch.cuda.synchronize()
    assert buf[:130].view(2, 65)[:, 0].tolist() == [W * (cu + 1)] * 2                   # a ring of zeros with lo = 0: cell (0, 0)
    assert int(buf.sum().item()) == 2 * W * (cu + 1)
    # the 1-D stage attaches beside it
    hb = torch.zeros(d * 10, dtype=torch.int64, device=g.device)
    _lib.check(L.ptmi_hist_attach(g.h, C.c_void_p(hb.data_ptr()), ptr(lo), ptr(sc), 8))
    assert L.ptmi_hist_update(g.h, 1, cu) == 0 and L.ptmi_pairs_update(g.h, 1, cu) == 0
    torch.cuda.synchronize()
    assert hb.view(d, 10)[:, 0].tolist() == [W * cu] * d and buf[:130].view(2, 65)[:, 0].tolist() == [W * (2 * cu + 1)] * 2


def test_checkpoint_and_restore_mid_run(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 100, 4, 20
    spec = ({"params": [0, 99, 50]}, -0.5, 0.5, 40)
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=40, tskip=10, seed=9, cov_mode="pooled")
    p0 = np.random.RandomState(6).randn(W, 2, d) * 0.1
    a = PTEngine.with_stages(d, 2, W, _cov0(d), pairs=spec, pairs_from=5, **kw)
    a.init_state(p0)
    a.run(3 * cu + 7)
    whole = a.pairs_counts()
    b = PTEngine.with_stages(d, 2, W, _cov0(d), pairs=spec, pairs_from=5, **kw)
    b.init_state(p0)
    b.run(cu + 9)
    b.pairs_sync(cu + 4)                                             # counted up to the middle of a period: the checkpoint says so
    st = b.checkpoint()
    assert st["pairs_iter"] == cu + 4 and st["t_pairs"].shape == (3, 1601)
    c = PTEngine.with_stages(d, 2, W, _cov0(d), pairs=spec, pairs_from=5, **kw)
    c.init_state(p0)
    c.restore(st)
    assert c.pairs_iter == cu + 4
    c.run(2 * cu - 2)
    got = c.pairs_counts()
    for k in whole:
        assert_same(got[k], whole[k], "restored " + k)
    assert (whole["counts"].sum((1, 2)) + whole["outside"] == W * (3 * cu + 2)).all()
    # a checkpoint without the stage, or with other bins, is refused before anything is touched
    plain = PTEngine(d, 2, W, _cov0(d), **kw)
    plain.init_state(p0)
    plain.run(3)
    x0 = c.get("X").copy()
    with pytest.raises(ValueError, match="no pair histograms"):
        c.restore(plain.checkpoint())
    other = dict(st, t_pairs=np.zeros((3, 1025), dtype=np.int64))
    with pytest.raises(ValueError, match="no pair histograms"):
        c.restore(other)
    assert_same(c.get("X"), x0, "X after the refusals")
    assert c.pairs_iter == 3 * cu + 7


def _sampler(out, W, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 4
    s = PTSampler(d, ("iso",), ("box", -3.0 * np.ones(d), 3.0 * np.ones(d)), np.eye(d) * 0.5, outDir=str(out), verbose=False, seed=21, ntemps=2,
                  nwalkers=W, keep_walkers=W, **kw)
    s.posterior_pairs = ({"params": [0, 3, 1]}, np.array([-3.0, -2.0, -1.0, -0.5]), np.array([3.0, 2.0, 1.0, 0.5]), 24)
    return s


def test_sampler_counts_equal_the_harvested_chains_and_resume(tmp_path):
    W = 6
    run = dict(burn=100, thin=1, covUpdate=50, isave=50, Tskip=10)
    p0 = np.zeros(4)
    a = _sampler(tmp_path / "a", W, checkpoint=True)
    a.sample(p0, 300, **run)
    pairs, lo, hi, nbins = a.posterior_pairs
    want = pairs_rule(a._chains[:, 101:301], [[0, 3], [0, 1], [3, 1]], lo, hi, nbins)      # the harvested chains: another path out of the ring (_harvest)
    assert_same(_flat(a.pairs2d), want, "sampler.pairs2d")
    assert a.pairs2d["pairs"].tolist() == [[0, 3], [0, 1], [3, 1]]
    assert a.pairs2d["last_iter"] == 300 and a.pairs2d["first_iter"] == 101 and a.pairs2d["nwalkers"] == W
    assert (want.sum(1) == W * 200).all() and want[0, -1] > 0        # the narrow range of parameter 3 leaves samples outside
    f = np.load(tmp_path / "a" / "pairs.npz")
    assert sorted(f.files) == ["counts", "edges", "first_iter", "last_iter", "nwalkers", "outside", "pairs"]
    for k in f.files:
        assert_same(f[k], a.pairs2d[k], k)
    assert f["counts"].dtype == np.uint64 and f["counts"].shape == (3, 24, 24) and int(f["last_iter"]) == 300
    # stopped at 150 and resumed from its checkpoint: the counts of the uninterrupted run
    b1 = _sampler(tmp_path / "b", W, checkpoint=True)
    b1.sample(p0, 150, **run)
    assert b1.pairs2d["last_iter"] == 150 and (b1.pairs2d["counts"].sum((1, 2)) + b1.pairs2d["outside"] == W * 50).all()
    b2 = _sampler(tmp_path / "b", W, checkpoint=True, resume=True)
    b2.sample(p0, 300, **run)
    assert np.array_equal(a._chains, b2._chains)
    for k in f.files:
        assert_same(b2.pairs2d[k], a.pairs2d[k], "resumed " + k)
    # a run without the attribute writes no file and has no pair histogram
    from ptmcmcsampler_amd import PTSampler
    c = PTSampler(4, ("iso",), ("flat",), np.eye(4) * 0.5, outDir=str(tmp_path / "c"), verbose=False, seed=21)
    c.sample(p0, 100, burn=50, thin=1, covUpdate=50, isave=50)
    assert c.pairs2d is None and not (tmp_path / "c" / "pairs.npz").exists() and c.engine.pairs_spec is None
