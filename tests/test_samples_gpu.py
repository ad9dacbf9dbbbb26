"""Thinned samples of every cold chain kept on the device (csrc/ptmi_samples.hip; ``PTEngine.with_stages(samples=...)``,
``PTSampler.posterior_samples``): every held snapshot equals, bit for bit, the row the cold chain held at that iteration -- NumPy on the
ring as it was copied before each covariance epoch (tests/test_hist_gpu.py ``_ring`` / ``_expand``), lnL and lp from AMaux at the
iteration's own ring row -- on a crafted ring with runs of rows that were not stored, in the permuted row format, at widths that fill
no wave and no block, with more pairs than one launch carries, across decimations, in both ring modes, with two rings and on the
callback path, through ``samples_sync``, a checkpoint, the C ABI's refusals and the sampler; and the stage only reads.

Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)
from test_hist_gpu import _cov0, _expand, _ring

pytestmark = pytest.mark.gpu


def _same_bits(a, b, what=""):
    """Equality of the words themselves: a NaN equals only the NaN with its payload, -0.0 is not 0.0."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), "%s: %d of %d words differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def _record(g, chain, base, k_hi):
    """Iterations base + 1 .. base + k_hi of every cold chain from the ring as it stands: chain[it] = (x [W][d], aux [W][2] or None)."""
    am, fl = _ring(g)
    rows = _expand(am, fl, base, 1, k_hi)
    aux = g.t["AMaux"].cpu().numpy() if g.t["AMaux"] is not None else None
    for k in range(1, k_hi + 1):
        chain[base + k] = (rows[:, k - 1].copy(), aux[:, (base + k) % g.cov_update].copy() if aux is not None else None)
    return fl


def _drive(g, advance, periods, extra=0):
    """``periods`` whole covariance periods from iteration 0 and ``extra`` iterations of the next one, the ring copied at each period's
    end (the next iteration's epoch takes it: update_cov); returns every cold chain by iteration."""
    cu, chain = g.cov_update, {}
    for p in range(periods):
        advance(cu)
        _record(g, chain, p * cu, cu)
    if extra:
        advance(extra)
        _record(g, chain, periods * cu, extra)
    return chain


def _held(first, every, stride, last):
    return list(range(first + stride, last + 1, stride)) if last > first else []


def _check(g, chain, what=""):
    """``g.samples()`` against the chains: the held iterations are the multiples of the stride, every row is the chain's."""
    s = g.samples()
    slots, every = g.samples_spec
    first = g.samples_from
    assert s["every"] == every and s["stride"] % every == 0 and s["first_iter"] == first + 1 and s["last_iter"] == g.iter and s["nwalkers"] == g.W
    assert s["iters"].tolist() == _held(first, every, int(s["stride"]), g.iter), what
    M = (g.iter - first) // every
    assert len(s["iters"]) == M if M <= slots else slots // 2 <= len(s["iters"]) <= slots
    assert s["x"].shape == (len(s["iters"]), g.W, g.d)
    for j, it in enumerate(s["iters"].tolist()):
        x, aux = chain[it]
        _same_bits(s["x"][j], x, "%s x at iteration %d" % (what, it))
        if aux is not None:
            _same_bits(s["lnlike"][j], aux[:, 0], "%s lnL at iteration %d" % (what, it))
            _same_bits(s["lnprob"][j], (1.0 / g.temps_mh[0]) * aux[:, 0] + aux[:, 1], "%s lnprob at iteration %d" % (what, it))
        else:
            assert "lnlike" not in s and "lnprob" not in s
    xd, auxd, itd = g.samples_device()
    assert xd.is_cuda and np.array_equal(itd, s["iters"])
    _same_bits(xd.cpu().numpy(), s["x"], what + " samples_device")
    return s


def _take(g, iters, slots):
    it, sl = np.ascontiguousarray(iters, dtype=np.int64), np.ascontiguousarray(slots, dtype=np.int32)
    return g.lib.ptmi_samples_take(g.h, it.ctypes.data_as(C.POINTER(C.c_int64)), sl.ctypes.data_as(C.POINTER(C.c_int32)), len(it))


# ---------------------------------------------------------------------- the kernel on rings made by hand
def _crafted_flags(cu):
    """Three flag rows of a period of 200 (1 = stored) with runs of rows that were not stored of length 1, 63, 64, 65 / 130 / 198 -- the
    last one hangs on ring row 1 -- and the iterations worth taking: inside each run (first, middle, last) and right behind it."""
    assert cu == 200
    lay = np.ones((3, cu + 1), dtype=np.int64)                       # by k = 1 .. cu (column 0 unused)
    runs = [[(3, 3), (5, 67), (69, 132), (134, 198)], [(3, 132)], [(2, 199)]]
    ks = {1, 2, cu, cu - 1}
    for row, rr in zip(lay, runs):
        for a, b in rr:
            assert b - a + 1 in (1, 63, 64, 65, 130, 198)
            row[a:b + 1] = 0
            ks |= {a, (a + b) // 2, b, b + 1, max(a - 1, 1)}
    return lay, sorted(ks)


def test_crafted_ring_runs_and_special_values(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu, nslots = 5, 3, 200, 64
    g = PTEngine.with_stages(d, 1, W, np.eye(d), cov_update=cu, tskip=0, cov_mode="pooled", keep_lnl=True, samples=nslots, samples_from=0)
    assert g.t["AMflag"] is not None and g.am_pos is None
    rs = np.random.RandomState(11)
    ring = rs.randn(W, cu, d)
    payload = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
    special = np.array([np.nan, np.inf, -np.inf, -0.0, payload])
    ring[:, 1] = special                                             # the row the long runs hang on
    ring[:, 0] = special[::-1]                                       # iteration cu
    ring[1, 2] = special
    aux = rs.randn(W, cu, 2)
    aux[:, 1] = [payload, -0.0]
    g.put("AM", ring)
    g.put("AMaux", aux)
    lay, ks = _crafted_flags(cu)
    assert len(ks) <= nslots
    for shift in range(3):                                           # every walker gets every layout once
        fl = np.stack([lay[(w + shift) % 3] for w in range(W)])      # [W][k]
        word = np.zeros((W, cu), dtype=np.int64)
        for k in range(1, cu + 1):
            word[:, k % cu] = np.where(fl[:, k] != 0, _lib.AMROW_NEW if k % 3 else _lib.AMROW_KEY, 0)
        word[:, 1] = _lib.AMROW_KEY
        g.t["AMflag"].copy_(torch.from_numpy(word))
        g.t["samples"].fill_(7.0)
        g.t["samples_aux"].fill_(7.0)
        slots = rs.permutation(nslots)[:len(ks)]
        assert _take(g, ks, slots) == 0, g.lib.ptmi_last_error()
        am, flags = _ring(g)
        truth = _expand(am, flags, 0, 1, cu)
        got, gaux = g.t["samples"].cpu().numpy(), g.t["samples_aux"].cpu().numpy()
        for k, s in zip(ks, slots):
            _same_bits(got[s], truth[:, k - 1], "shift %d, k = %d" % (shift, k))
            _same_bits(gaux[s], aux[:, k % cu], "shift %d, aux of k = %d" % (shift, k))      # the iteration's OWN row, stored or not
        rest = np.setdiff1d(np.arange(nslots), slots)
        assert (got[rest] == 7.0).all() and (gaux[rest] == 7.0).all()      # no other slot was written
    # k = 199 of the walker whose run 2 .. 199 hangs on ring row 1: the special row, through four steps of the walk back
    w = [w for w in range(W) if (w + 2) % 3 == 2][0]
    _same_bits(got[slots[ks.index(199)], w], special, "the long run")
    # the same ring without flags (per-walker covariances): every row is its own
    p = PTEngine.with_stages(d, 1, W, np.eye(d), cov_update=cu, tskip=0, keep_lnl=True, samples=nslots, samples_from=0)
    assert p.t["AMflag"] is None
    p.put("AM", ring)
    p.put("AMaux", aux)
    slots = rs.permutation(nslots)[:len(ks)]
    assert _take(p, ks, slots) == 0, p.lib.ptmi_last_error()
    p.sync()
    got, gaux = p.t["samples"].cpu().numpy(), p.t["samples_aux"].cpu().numpy()
    for k, s in zip(ks, slots):
        _same_bits(got[s], ring[:, k % cu], "no flags, k = %d" % k)
        _same_bits(gaux[s], aux[:, k % cu], "no flags, aux of k = %d" % k)


def test_permuted_row_format_rle_three_periods(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 100, 5, 20
    g = PTEngine.with_stages(d, 2, W, _cov0(d), weights=(20, 20, 20), cov_update=cu, burn=40, tskip=7, seed=5, cov_mode="pooled",
                             am_mode="rle", keep_lnl=True, samples=32, samples_from=0)
    assert g.am_pos is not None and g.am_rle
    g.init_state(np.random.RandomState(1).randn(W, 2, d) * 0.1)
    chain = _drive(g, g.run, 3, extra=1)
    assert g.samples_iter == 3 * cu
    s = _check(g, chain, "permuted")                                 # ... and iteration 61, inside the fourth period
    assert s["stride"] == 2 and len(s["iters"]) == 30 and g.samples_iter == 61


@pytest.mark.parametrize("d,W,mode", [(1, 1, "per_walker"), (37, 3, "pooled"), (64, 5, "per_walker"), (65, 3, "pooled"), (300, 5, "pooled")])
def test_widths(mods, d, W, mode):
    orc, _lib, PTEngine = mods
    cu = 12
    g = PTEngine.with_stages(d, 1, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=d, cov_mode=mode,
                             keep_lnl=(d != 37), samples={"slots": 6, "every": 1}, samples_from=2)
    g.init_state(np.random.RandomState(d).randn(W, 1, d) * 0.2)
    chain = _drive(g, g.run, 1, extra=5)
    assert (g.t["AMflag"] is not None) == (mode == "pooled") and (g.t["samples_aux"] is None) == (d == 37)
    s = _check(g, chain, "d=%d W=%d" % (d, W))
    assert s["stride"] == 4 and s["iters"].tolist() == [6, 10, 14]


def test_more_pairs_than_one_launch_carries(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 4, 3, 300
    box = ("box", -0.3 * np.ones(d), 0.3 * np.ones(d))
    g = PTEngine.with_stages(d, 1, W, np.eye(d) * 0.05, weights=(20, 0, 0), cov_update=cu, burn=10000, tskip=0, seed=4, cov_mode="pooled",
                             logp=box, keep_lnl=True, samples={"slots": 512, "every": 1}, samples_from=0)
    g.init_state(np.zeros((W, 1, d)))
    chain = _drive(g, g.run, 1, extra=1)                             # iteration 301's epoch takes 300 pairs in one call: two launches
    assert (_ring(g)[1] is not None)
    s = _check(g, chain, "512 slots")
    assert len(s["iters"]) == 301 and s["stride"] == 1


def test_decimation_across_periods_with_rows_that_were_not_stored(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 6, 4, 20
    rs = np.random.RandomState(4)
    box = ("box", -0.25 - rs.rand(d) * 0.1, 0.2 + rs.rand(d) * 0.1)
    g = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.05, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=10, seed=31, cov_mode="pooled",
                             am_mode="rle", logp=box, keep_lnl=True, samples={"slots": 4, "every": 3}, samples_from=0)
    g.init_state(rs.uniform(-0.05, 0.05, (W, 2, d)))
    chain, unstored = {}, 0
    for p in range(5):
        g.run(cu)
        unstored += int((_record(g, chain, p * cu, cu) == 0).sum())
    g.run(7)
    _record(g, chain, 5 * cu, 7)
    assert unstored > 0, "the tight prior must leave rows that were not stored"
    s = _check(g, chain, "five periods and a part")
    # 35 candidates through 4 slots: strides 3, 6, 12, 24; the multiples of 24 up to 107
    assert s["stride"] == 24 and s["iters"].tolist() == [24, 48, 72, 96] and g._splan.level == 3
    held = g.samples()["x"]
    moved = sum(int((held[j] != held[j - 1]).any()) for j in range(1, len(held)))
    assert moved == len(held) - 1                                    # the chains went somewhere: the snapshots are four different states


# ---------------------------------------------------------------------- every way of running the engine
def test_both_ring_modes_two_rings_and_the_callback_path(mods):
    orc, _lib, PTEngine = mods
    d, W, cu, n = 24, 6, 16, 3 * 16 + 5
    p0 = np.random.RandomState(2).randn(W, 2, d) * 0.1
    kw = dict(weights=(20, 20, 0), cov_update=cu, burn=1000, tskip=5, seed=8, cov_mode="pooled", keep_lnl=True)
    spec = dict(samples={"slots": 5, "every": 2}, samples_from=3)

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    def pair(**more):
        a, b = PTEngine.with_stages(d, 2, W, _cov0(d), **kw, **more, **spec), PTEngine(d, 2, W, _cov0(d), **kw, **more)
        chain = {}
        for g in (a, b):
            if more.get("split"):
                g.init_state_callback(p0, logl, None)
                adv = lambda m, g=g: g.run_callback(m, logl, None)      # noqa: E731
            else:
                g.init_state(p0)
                adv = g.run
            if g is a:
                chain = _drive(g, adv, 3, extra=5)
            else:
                adv(n)
        for name in ("X", "lnL", "lp", "nacc", "jstat", "nswap", "cov", "AM", "AMaux"):      # the stage only reads
            assert_same(a.get(name), b.get(name), "%r %s" % (more, name))
        assert "samples" not in b.t and "samples_iter" not in b.checkpoint() and b.samples_spec is None
        return _check(a, chain, repr(more))

    rle, rows = pair(am_mode="rle"), pair(am_mode="rows")
    lag, two, cb = pair(am_mode="rle", eig_lag=1), pair(am_mode="rle", stats_async=True, eig_lag=1), pair(split=True)
    for s in (rle, rows, lag, two, cb):
        assert s["iters"].tolist() == rle["iters"].tolist() == [19, 35, 51]
    for k in ("x", "lnlike", "lnprob"):
        _same_bits(two[k], lag[k], "two rings " + k)                 # a scheduling change only: the run with the same eig_lag on one ring


def test_samples_sync_inside_a_period_and_the_readers_refusals(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 8, 3, 20
    kw = dict(weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=3, cov_mode="pooled", keep_lnl=True,
              logp=("box", -0.3 * np.ones(d), 0.3 * np.ones(d)), samples={"slots": 6, "every": 1}, samples_from=0)
    p0 = np.zeros((W, 1, d))
    a, b = (PTEngine.with_stages(d, 1, W, np.eye(d) * 0.05, **kw) for _ in range(2))
    for g in (a, b):
        g.init_state(p0)
        g.run(2 * cu)                                                # iteration 21 took the first period
    a.samples_sync(cu + 9)
    assert a.samples_iter == cu + 9 and b.samples_iter == cu
    a.samples_sync(cu + 9)                                           # again: nothing to take
    a.samples_sync(2 * cu)
    for g in (a, b):
        g.run(1)
    assert a.samples_iter == b.samples_iter == 2 * cu
    assert np.array_equal(a._splan.slot_iter, b._splan.slot_iter) and a._splan.level == b._splan.level
    sa, sb = a.samples(), b.samples()
    assert sa["iters"].tolist() == sb["iters"].tolist() == [8, 16, 24, 32, 40]
    for k in ("x", "lnlike", "lnprob"):
        _same_bits(sa[k], sb[k], "middle + rest = the whole period: " + k)
    with pytest.raises(ValueError, match=r"samples_sync\(42\): the engine has reached iteration 41"):
        a.samples_sync(a.iter + 1)
    f = PTEngine.with_stages(d, 1, W, np.eye(d) * 0.05, **kw)
    f.iter = cu + 1                                                  # stepped from outside, past an epoch that never went through update_cov
    with pytest.raises(ValueError, match=r"samples_sync\(21\): iterations 1..20 are no longer in the ring"):
        f.samples_sync(cu + 1)
    assert f.samples_iter == 0 and (f._splan.slot_iter == -1).all()
    with pytest.raises(ValueError, match=r"no sample buffer: PTEngine.with_stages\(..., samples=slots\)"):
        PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0).samples()


def test_checkpoint_mid_period_after_a_decimation(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 10, 4, 20
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=40, tskip=10, seed=6, cov_mode="pooled", keep_lnl=True)
    spec = dict(samples={"slots": 4, "every": 1}, samples_from=0)
    p0 = np.random.RandomState(3).randn(W, 2, d) * 0.1
    a = PTEngine.with_stages(d, 2, W, _cov0(d), **kw, **spec)
    a.init_state(p0)
    a.run(cu + 10)
    a.samples_sync(cu + 6)                                           # the checkpoint falls inside a period, with part of it taken
    assert a._splan.level >= 1 and a.samples_iter == cu + 6
    st = a.checkpoint()
    assert st["samples_iter"] == cu + 6 and st["samples_level"] == a._splan.level and st["t_samples"].shape == (4, W, d)
    assert np.array_equal(st["samples_slot_iter"], a._splan.slot_iter) and st["t_samples_aux"].shape == (4, W, 2)
    b = PTEngine.with_stages(d, 2, W, _cov0(d), **kw, **spec)
    b.restore(st)
    for g in (a, b):
        g.run(2 * cu + 5)
    sa, sb = a.samples(), b.samples()
    assert a._splan.level == b._splan.level >= 3 and np.array_equal(a._splan.slot_iter, b._splan.slot_iter)
    _same_bits(a.t["samples"].cpu().numpy(), b.t["samples"].cpu().numpy(), "the restored run's slots")
    _same_bits(a.t["samples_aux"].cpu().numpy(), b.t["samples_aux"].cpu().numpy(), "the restored run's aux")
    for k in sa:
        assert_same(sa[k], sb[k], k)
    assert_same(a.get("X"), b.get("X"), "X")
    # a checkpoint without the stage, or with another number of slots, is refused before anything is touched
    c = PTEngine(d, 2, W, _cov0(d), **kw)
    c.init_state(p0)
    c.run(cu + 10)
    assert st["samples_every"] == 1 and st["samples_from"] == 0
    for bad, other in ((c.checkpoint(), None), (st, dict(samples=5, samples_from=0)), (st, dict(samples={"slots": 4, "every": 2}, samples_from=0)),
                       (st, dict(samples=4, samples_from=3))):      # ... or filled on another schedule
        e = PTEngine.with_stages(d, 2, W, _cov0(d), **kw, **(other or spec))
        e.init_state(p0)
        x0 = e.get("X")
        with pytest.raises(ValueError, match="the checkpoint carries no sample buffer of this shape"):
            e.restore(bad)
        assert e.iter == 0 and e.samples_iter == e.samples_from and (e._splan.slot_iter == -1).all()
        assert_same(e.get("X"), x0, "nothing was touched")


def test_a_hot_block_takes_nothing(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 8, 3, 10
    g = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=2, ntemps_global=4,
                             temp0=2, keep_lnl=True, samples=4, samples_from=0)
    assert not g.owns_cold and g.t["AM"] is None and g.t["samples_aux"] is None
    g.init_state(np.zeros((W, 2, d)))
    g.run(2 * cu + 3)
    assert _take(g, [1, 2 * cu], [0, 1]) == 0                        # not even the range is looked at, as ptmi_update_cov
    s = g.samples()
    assert s["x"].shape == (0, W, d) and len(s["iters"]) == 0 and "lnlike" not in s
    g.sync()
    assert not g.t["samples"].any().item()


def test_c_abi_refusals(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu, nslots = 5, 2, 8, 6
    g = PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0)         # no AMaux
    L = g.lib
    err = lambda: L.ptmi_last_error().decode()      # noqa: E731
    assert _take(g, [1], [0]) == -1 and "ptmi_samples_attach" in err()      # PTMI_EINVAL: take before attach
    buf = torch.ones(nslots * W * d + 1, dtype=torch.float64, device=g.device)
    aux = torch.ones(nslots * W * 2, dtype=torch.float64, device=g.device)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    for n in (0, -1, 65536):
        assert L.ptmi_samples_attach(g.h, p(buf), None, n) == -1 and "nslots" in err()
    assert L.ptmi_samples_attach(g.h, p(buf, 4), None, nslots) == -1 and "aligned" in err()
    assert L.ptmi_samples_attach(g.h, None, None, nslots) == -1 and "rows" in err()
    assert L.ptmi_samples_attach(g.h, p(buf), p(aux, 4), nslots) == -1 and "aux" in err() and "aligned" in err()
    assert L.ptmi_samples_attach(g.h, p(buf), p(aux), nslots) == -1 and "AMaux" in err()
    assert _take(g, [1], [0]) == -1 and "ptmi_samples_attach" in err()      # none of them attached anything
    _lib.check(L.ptmi_samples_attach(g.h, p(buf), None, nslots))
    assert L.ptmi_samples_attach(g.h, p(buf), None, nslots) == -1 and "already attached" in err()
    for iters in ([2, 2], [3, 2], [1, 4, 3]):
        assert _take(g, iters, list(range(len(iters)))) == -1 and "ascending" in err(), iters
    assert _take(g, [1, 2, 3], [0, 4, 0]) == -1 and "repeated" in err()
    for bad in (-1, nslots, 70000):
        assert _take(g, [1, 2], [0, bad]) == -1 and "out of range" in err(), bad
    for iters in ([cu, cu + 1], [1, cu + 1], [cu - 2, 2 * cu], [0, 3], [-2, 1], [0]):
        assert _take(g, iters, list(range(len(iters)))) == -1 and "period" in err(), iters
    assert L.ptmi_samples_take(g.h, None, None, -1) == -1 and "n >= 0" in err()
    assert L.ptmi_samples_take(g.h, None, None, 3) == -1 and "non-NULL" in err()
    torch.cuda.synchronize()
    assert (buf == 1.0).all().item()                                 # a refused call launched nothing
    assert L.ptmi_samples_take(g.h, None, None, 0) == 0 and _take(g, [], []) == 0      # n = 0: nothing to do
    ring = np.random.RandomState(0).randn(W, cu, d)
    g.put("AM", ring)
    assert _take(g, [cu + 1, 2 * cu], [5, 2]) == 0 and _take(g, [cu], [0]) == 0
    torch.cuda.synchronize()
    got = buf[:-1].view(nslots, W, d).cpu().numpy()
    _same_bits(got[5], ring[:, 1], "iteration cu + 1: ring row 1")
    _same_bits(got[2], ring[:, 0], "iteration 2 cu: ring row 0")
    _same_bits(got[0], ring[:, 0], "iteration cu: ring row 0")
    assert (got[[1, 3, 4]] == 1.0).all() and buf[-1].item() == 1.0


# ---------------------------------------------------------------------- the sampler
def _sampler(out, W, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 6
    s = PTSampler(d, ("iso",), ("box", -3.0 * np.ones(d), 3.0 * np.ones(d)), np.eye(d) * 0.5, outDir=str(out), verbose=False, seed=21, ntemps=2,
                  nwalkers=W, keep_walkers=W, **kw)
    s.posterior_samples = {"slots": 8, "every": 4}
    return s


def test_sampler_samples_equal_the_harvested_chains_and_resume(tmp_path):
    W, thin = 16, 2
    run = dict(burn=100, thin=thin, covUpdate=50, isave=50, Tskip=10)
    p0 = np.zeros(6)
    a = _sampler(tmp_path / "a", W, checkpoint=True)
    a.sample(p0, 400, **run)
    s = a.samples
    # 75 candidates through 8 slots: stride 4 << 4 = 64 from iteration 100
    assert s["every"] == 4 and s["stride"] == 64 and s["iters"].tolist() == [164, 228, 292, 356] and s["first_iter"] == 101 and s["last_iter"] == 400
    assert s["nwalkers"] == W and s["x"].shape == (4, W, 6) and s["lnlike"].shape == s["lnprob"].shape == (4, W)
    for j, it in enumerate(s["iters"].tolist()):                     # the harvested chains: another path out of the ring (_harvest)
        _same_bits(s["x"][j], a._chains[:, it // thin], "x at %d" % it)
        _same_bits(s["lnlike"][j], a._lnlikes[:, it // thin], "lnlike at %d" % it)
        _same_bits(s["lnprob"][j], a._lnprobs[:, it // thin], "lnprob at %d" % it)
    f = np.load(tmp_path / "a" / "samples.npz")
    assert sorted(f.files) == ["every", "first_iter", "iters", "last_iter", "lnlike", "lnprob", "nwalkers", "stride", "x"]
    for k in f.files:
        assert_same(f[k], s[k], k)
    from ptmcmcsampler_amd.samples import flat
    fx, flp, fll = flat(f)
    assert fx.shape == (4 * W, 6) and np.array_equal(fx[W + 3], a._chains[3, 228 // thin]) and flp[W + 3] == a._lnprobs[3, 228 // thin]
    # stopped at 200 and resumed from its checkpoint: the file of the uninterrupted run
    b1 = _sampler(tmp_path / "b", W, checkpoint=True)
    b1.sample(p0, 200, **run)
    assert b1.samples["last_iter"] == 200 and b1.samples["stride"] == 16 and b1.samples["iters"].tolist() == [116, 132, 148, 164, 180, 196]
    b2 = _sampler(tmp_path / "b", W, checkpoint=True, resume=True)
    b2.sample(p0, 400, **run)
    assert np.array_equal(a._chains, b2._chains)
    fb = np.load(tmp_path / "b" / "samples.npz")
    assert sorted(fb.files) == sorted(f.files)
    for k in f.files:
        assert_same(fb[k], f[k], "resumed " + k)
    # chain files alone cannot continue the buffer
    c1 = _sampler(tmp_path / "c", W, checkpoint=False)
    c1.sample(p0, 50, **run)
    c2 = _sampler(tmp_path / "c", W, checkpoint=False, resume=True)
    with pytest.raises(NotImplementedError, match="posterior_samples"):
        c2.sample(p0, 100, **run)
    # a run without the attribute writes no file and has no samples
    from ptmcmcsampler_amd import PTSampler
    e = PTSampler(6, ("iso",), ("flat",), np.eye(6) * 0.5, outDir=str(tmp_path / "e"), verbose=False, seed=21)
    e.sample(p0, 100, burn=50, thin=1, covUpdate=50, isave=50)
    assert e.samples is None and not (tmp_path / "e" / "samples.npz").exists() and e.engine.samples_spec is None
