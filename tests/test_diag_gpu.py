"""Convergence diagnostics of every cold chain from the AM ring (csrc/ptmi_diag.hip; ``PTEngine.with_stages(diag=True)``,
``PTSampler.chain_diagnostics``): the device's planes equal the NumPy restatement of the rule (tests/test_diag.py ``diag_rule``) applied
to the ring as it was copied before each covariance epoch -- BIT FOR BIT, every row format, both ring modes, clipped runs, lane and
wave edges, the callback path, two rings, the sampler, its checkpoint and its stop rule -- and the stage only reads: the chains are
the same bits.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from test_diag import diag_rule
from test_gpu_parity import _compare, assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

PLANES = ("c", "S1", "S2", "A", "Q", "H")


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


def _planes(g):
    from ptmcmcsampler_amd.diagnostics import planes
    g.sync()
    return planes(g.t["diag"].cpu().numpy(), g.diag_levels)


def _same_state(got, want, what):
    for k in PLANES:
        assert_same(got[k], want[k], "%s: plane %s" % (what, k))


def _drive(g, advance, periods, state=None, flags=None):
    """``periods`` whole covariance periods from iteration 0, the ring copied at each one's end (the first iteration of the next
    period folds it: update_cov), then one more iteration; returns the NumPy state of iterations 1 .. periods * cov_update (and
    appends each period's flags to ``flags``)."""
    cu = g.cov_update
    for p in range(periods):
        advance(cu)
        assert g.diag_iter == max(p * cu, g.diag_from)
        am, fl = _ring(g)
        if flags is not None:
            flags.append(fl)
        state = diag_rule(_expand(am, fl, p * cu, 1, cu), g.diag_batch, g.diag_levels, state)
    advance(1)
    assert g.diag_iter == periods * cu
    return state


def _crafted(PTEngine, L, b0, ring):
    W, cu, d = ring.shape
    g = PTEngine.with_stages(d, 1, W, np.eye(d), cov_update=cu, tskip=0, diag=True, diag_from=0, diag_batch=b0, diag_levels=L)
    assert g.t["AMflag"] is None                                     # per-walker covariances: every row is stored
    assert tuple(g.t["diag"].shape) == (2 * L + 3, W, d)
    g.put("AM", ring)
    return g


def test_crafted_ring(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 5, 3, 24
    ring = np.random.RandomState(3).randn(W, cu, d) * np.array([1.0, 1e-3, 50.0, 1.0, 7.0]) + np.array([0.0, 5.0, -300.0, 1e6, 0.1])
    rows = _expand(ring, None, 0, 1, cu)                             # iteration k sits in ring row k % cu
    assert np.array_equal(rows[:, -1], ring[:, 0]) and np.array_equal(rows[:, 0], ring[:, 1])
    # one call over the period: carries through every level, the top level takes three batches
    g = _crafted(PTEngine, 4, 1, ring)
    _lib.check(g.lib.ptmi_diag_update(g.h, 1, cu, 0))
    want = diag_rule(rows, 1, 4)
    _same_state(_planes(g), want, "1..24")
    assert (want["Q"][3] > 0).all() and (want["A"] == 0).all()
    # the calls 1..5, 6..6, 7..24 on a fresh engine: the same bits
    f = _crafted(PTEngine, 4, 1, ring)
    for lo, hi in ((1, 5), (6, 6), (7, cu)):
        _lib.check(f.lib.ptmi_diag_update(f.h, lo, hi, lo - 1))
    _same_state(_planes(f), want, "1..5, 6..6, 7..24")
    assert_same(f.t["diag"].cpu().numpy(), g.t["diag"].cpu().numpy(), "split against whole")
    # fewer levels on the same ring; a batch length that leaves the period inside a batch (24 = 4 * 5 + 4)
    for L, b0 in ((1, 1), (2, 1), (4, 5), (3, 2)):
        e = _crafted(PTEngine, L, b0, ring)
        _lib.check(e.lib.ptmi_diag_update(e.h, 1, cu, 0))
        w = diag_rule(rows, b0, L)
        _same_state(_planes(e), w, "L = %d, b0 = %d" % (L, b0))
        if b0 == 5:
            assert (w["A"] != 0).all()
            # ... and the next period picks the batch up: ring rows again as iterations 25 .. 48
            _lib.check(e.lib.ptmi_diag_update(e.h, cu + 1, 2 * cu, cu))
            _same_state(_planes(e), diag_rule(rows, b0, L, w), "second period, b0 = 5")
    # +-inf / NaN stay in their own stream
    bad = ring.copy()
    bad[0, 3, 1], bad[1, 7, 2], bad[2, 0, 4], bad[2, 1, 0] = np.inf, np.nan, -np.inf, np.inf      # (ring row 1: the shift itself)
    h = _crafted(PTEngine, 4, 1, bad)
    _lib.check(h.lib.ptmi_diag_update(h.h, 1, cu, 0))
    got, w = _planes(h), diag_rule(_expand(bad, None, 0, 1, cu), 1, 4)
    _same_state(got, w, "non-finite entries")
    poisoned = np.zeros((W, d), dtype=bool)
    poisoned[0, 1] = poisoned[1, 2] = poisoned[2, 4] = poisoned[2, 0] = True
    assert (np.isfinite(got["S2"]) == ~poisoned).all()
    for k in PLANES:
        assert_same(got[k][..., ~poisoned], want[k][..., ~poisoned], "the other streams, plane " + k)


def test_permuted_row_format_rle_three_periods(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 100, 5, 20
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=40, tskip=7, seed=5, cov_mode="pooled", diag=True, diag_from=0, diag_batch=3,
              diag_levels=5)
    p0 = np.random.RandomState(1).randn(W, 2, d) * 0.1
    g = PTEngine.with_stages(d, 2, W, _cov0(d), am_mode="rle", **kw)
    assert g.am_pos is not None and g.am_rle
    g.init_state(p0)
    # every row stored (am_mode="rows"): the same rows give the same bits.  The two modes' RUNS are the same chains only up to the first
    # covariance epoch -- their pooled statistics round differently (tests/test_am_rle_gpu.py: "the runs then part at the level of the
    # last bits") -- so the first period is compared run against run, and all three with the rle run's rows in the rows engine's ring
    r = PTEngine.with_stages(d, 2, W, _cov0(d), am_mode="rows", **kw)
    assert not r.am_rle and r.t["AMflag"] is None and r.am_pos is not None
    r.init_state(p0)
    r.run(cu + 1)
    want = None
    for p in range(3):
        g.run(cu)
        assert g.diag_iter == p * cu
        am, fl = _ring(g)
        assert (fl == 0).any()
        rows = _expand(am, fl, p * cu, 1, cu)
        want = diag_rule(rows, 3, 5, want)
        if p == 0:
            _same_state(_planes(r), want, "am_mode='rows', its own first period")
        else:
            r.put("AM", np.roll(rows, 1, axis=1))                    # iteration p cu + k in ring row k % cu
            _lib.check(r.lib.ptmi_diag_update(r.h, p * cu + 1, (p + 1) * cu, p * cu))
    g.run(1)
    assert g.diag_iter == 3 * cu
    _same_state(_planes(g), want, "three periods")
    _same_state(_planes(r), want, "am_mode='rows' on the same rows")
    assert_same(r.t["diag"].cpu().numpy(), g.t["diag"].cpu().numpy(), "rows against rle")
    m = g.diag_moments()                                             # ... and iteration 61
    am, fl = _ring(g)
    assert (fl == 0).any()
    want = diag_rule(_expand(am, fl, 3 * cu, 1, 1), 3, 5, want)
    _same_state(m, want, "diag_moments")
    assert m["n"] == 61 and m["k"] == 20 and m["first_iter"] == 1 and m["last_iter"] == 61 and m["batch0"] == 3 and m["levels"] == 5
    assert m["nwalkers"] == W and m["Q"].shape == (5, W, d) and m["H"].shape == (4, W, d)
    e = g.diagnostics()
    assert e["rhat"].shape == (d,) and e["last_iter"] == 61 and int(e["n"]) == 61


@pytest.mark.parametrize("d,W", [(1, 70), (2, 70), (37, 4), (64, 3), (130, 3)])
def test_lane_and_wave_edges(mods, d, W):
    orc, _lib, PTEngine = mods
    cu = 12
    rs = np.random.RandomState(d)
    box = ("box", -0.25 - rs.rand(d) * 0.1, 0.2 + rs.rand(d) * 0.1)    # tight: rejections leave rows that are not stored
    g = PTEngine.with_stages(d, 1, W, np.eye(d) * 0.02, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=d, cov_mode="pooled",
                             am_mode="rle", logp=box, diag=True, diag_from=0, diag_batch=2, diag_levels=3)
    g.init_state(rs.uniform(-0.05, 0.05, (W, 1, d)))
    flags = []
    want = _drive(g, g.run, 2, flags=flags)
    fl = np.concatenate(flags, axis=1)                               # (a period's jumps follow the covariance of the one before: not every period has rejections)
    assert (fl == 0).any() and (fl != 0).any()
    assert (fl[0] != fl[1]).any()                                    # neighbouring walkers' flags differ: lane by lane where a wave holds both
    _same_state(_planes(g), want, "d = %d, W = %d" % (d, W))
    assert want["n"] == 2 * cu


def test_clipped_runs_and_a_start_inside_a_period(mods):
    orc, _lib, PTEngine = mods
    d, W, cu, b0, L = 37, 4, 30, 4, 3
    rs = np.random.RandomState(4)
    box = ("box", -0.25 - rs.rand(d) * 0.1, 0.2 + rs.rand(d) * 0.1)
    p0 = rs.uniform(-0.05, 0.05, (W, 2, d))
    kw = dict(weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=10, seed=31, cov_mode="pooled", am_mode="rle", logp=box, diag=True,
              diag_batch=b0, diag_levels=L)
    g = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, diag_from=0, **kw)
    g.init_state(p0)
    g.run(cu)
    am1, fl1 = _ring(g)
    g.run(cu)                                                        # iteration 31 folded the first period
    am, fl = _ring(g)
    assert (fl == 0).any(), "the tight prior must leave rows that were not stored"
    first = diag_rule(_expand(am1, fl1, 0, 1, cu), b0, L)
    _same_state(_planes(g), first, "the first period")
    # a mid-period iteration whose row is not stored for a walker and whose successor is not stored for a walker either: the run
    # under way there is cut by the first call and picked up by the second
    mids = [k for k in range(3, cu - 2) if ((fl[:, k] == 0) & (fl[:, k + 1] == 0)).any()]
    assert mids, "no run crosses a mid-period iteration: the test needs one"
    k = mids[len(mids) // 2]
    g.diag_sync(cu + k)
    assert g.diag_iter == cu + k
    _same_state(_planes(g), diag_rule(_expand(am, fl, cu, 1, k), b0, L, first), "up to the middle")
    g.diag_sync(cu + k)                                              # again: nothing to fold
    g.run(1)                                                         # the period's end folds the rest
    whole = diag_rule(_expand(am, fl, cu, 1, cu), b0, L, first)
    _same_state(_planes(g), whole, "middle + rest = the whole period")
    # a second engine that starts inside the second period, at an iteration whose row a walker did not store: the same chains (the
    # stage only reads), and the run under way at iter_lo is found by the walk back
    start = cu + k
    e = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, diag_from=start, **kw)
    e.init_state(p0)
    e.run(2 * cu + 1)
    assert e.diag_iter == 2 * cu
    _same_state(_planes(e), diag_rule(_expand(am, fl, cu, k + 1, cu), b0, L), "diag_from inside a period")
    m = e.diag_moments(2 * cu)
    assert m["first_iter"] == start + 1 and m["n"] == cu - k and m["last_iter"] == 2 * cu
    with pytest.raises(ValueError, match="no longer in the ring"):
        f = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, diag_from=0, **kw)
        f.iter = cu + 1                                              # stepped from outside, past an epoch that never went through update_cov
        f.diag_sync(cu + 1)                                          # the first period was never folded
    with pytest.raises(ValueError, match="has reached iteration"):
        e.diag_sync(e.iter + 1)                                      # the ring's rows beyond the engine's iteration are the period before's
    assert e.diag_iter == 2 * cu


def test_callback_path_and_two_rings(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 24, 6, 16
    p0 = np.random.RandomState(2).randn(W, 2, d) * 0.1

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    kw = dict(weights=(20, 20, 0), cov_update=cu, burn=1000, tskip=5, seed=8, cov_mode="pooled", diag=True, diag_from=0, diag_batch=2, diag_levels=4)
    g = PTEngine.with_stages(d, 2, W, _cov0(d), split=True, **kw)
    g.init_state_callback(p0, logl, None)
    want = _drive(g, lambda n: g.run_callback(n, logl, None), 3)
    _same_state(_planes(g), want, "run_callback")
    a = PTEngine.with_stages(d, 2, W, _cov0(d), stats_async=True, eig_lag=1, **kw)
    assert a.stats_async
    a.init_state(p0)
    want = _drive(a, a.run, 4)
    _same_state(_planes(a), want, "two rings")


class _As(object):
    """An engine's state with the attributes ``_compare`` reads from an oracle."""

    def __init__(self, g):
        g.sync()
        for name in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM"):
            setattr(self, name, g.get(name))


def test_the_stage_only_reads(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 100, 4, 20
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=40, tskip=10, seed=3, cov_mode="pooled")
    p0 = np.random.RandomState(5).randn(W, 3, d) * 0.1
    a = PTEngine.with_stages(d, 3, W, _cov0(d), diag=True, diag_from=0, **kw)
    b = PTEngine(d, 3, W, _cov0(d), **kw)
    for g in (a, b):
        g.init_state(p0)
        g.run(3 * cu + 1)
    assert a.diag_iter == 3 * cu and a.diag_levels == 16 and a.diag_batch == 1
    _compare(a, _As(b), "with and without the stage: ")
    for name in ("mu", "M2", "cov", "Ut", "S", "DE"):
        assert_same(a.get(name), b.get(name), name)
    assert "diag" not in b.t and "diag_iter" not in b.checkpoint() and not b.diag_on
    st = a.checkpoint()
    assert st["diag_iter"] == 3 * cu and st["t_diag"].shape == (35, W, d)
    with pytest.raises(ValueError, match="no diagnostics"):
        b.diag_sync(1)
    with pytest.raises(ValueError, match="carries no diagnostics"):
        a.restore(b.checkpoint())                                    # refused before anything is touched
    assert a.diag_iter == 3 * cu
    assert_same(a.get("X"), b.get("X"), "X after the refused restore")


def test_refusals(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu = 5, 2, 8
    g = PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0)
    L = g.lib
    err = lambda: L.ptmi_last_error().decode()      # noqa: E731
    assert L.ptmi_diag_update(g.h, 1, 2, 0) == -1 and "ptmi_diag_attach" in err()      # PTMI_EINVAL: update before attach
    buf = torch.zeros(35 * W * d + 1, dtype=torch.float64, device=g.device)
    for nl in (0, 17, -3):
        assert L.ptmi_diag_attach(g.h, C.c_void_p(buf.data_ptr()), nl, 1) == -1 and "nlevels" in err()
    for b0 in (0, -1):
        assert L.ptmi_diag_attach(g.h, C.c_void_p(buf.data_ptr()), 4, b0) == -1 and "batch0" in err()
    assert L.ptmi_diag_attach(g.h, C.c_void_p(buf.data_ptr() + 4), 4, 1) == -1 and "aligned" in err()
    assert L.ptmi_diag_attach(g.h, None, 4, 1) == -1
    assert L.ptmi_diag_update(g.h, 1, 2, 0) == -1 and "ptmi_diag_attach" in err()      # none of them attached anything
    _lib.check(L.ptmi_diag_attach(g.h, C.c_void_p(buf.data_ptr()), 16, 1))
    assert L.ptmi_diag_attach(g.h, C.c_void_p(buf.data_ptr()), 16, 1) == -1 and "already" in err()
    for a, b in ((cu, cu + 1), (1, cu + 1), (cu - 2, 2 * cu), (0, 3), (-2, 1)):
        assert L.ptmi_diag_update(g.h, a, b, 0) == -1 and "period" in err(), (a, b)
    assert L.ptmi_diag_update(g.h, 1, 2, -1) == -1 and "n_done" in err()
    torch.cuda.synchronize()
    assert not buf.any().item()                                      # a refused call launched nothing
    assert L.ptmi_diag_update(g.h, 5, 4, 0) == 0                     # iter_hi < iter_lo: nothing to do
    torch.cuda.synchronize()
    assert not buf.any().item()
    g.put("AM", np.ones((W, cu, d)) * 2.5)
    assert L.ptmi_diag_update(g.h, cu + 1, 2 * cu, 0) == 0
    torch.cuda.synchronize()
    acc = buf[:35 * W * d].view(35, W, d).cpu().numpy()
    assert (acc[0] == 2.5).all() and not acc[1:].any()               # a constant ring: the shift, and sums of zeros
    assert buf[-1].item() == 0.0                                     # nothing beyond the planes
    # a hot block of a sharded ladder: the engine refuses the stage, the library's update is a no-op there
    hot = PTEngine(d, 2, W, np.eye(d), cov_update=cu, tskip=0, ntemps_global=4, temp0=2)
    assert not hot.owns_cold and hot.t["AM"] is None
    buf2 = torch.zeros(5 * W * d, dtype=torch.float64, device=g.device)
    _lib.check(hot.lib.ptmi_diag_attach(hot.h, C.c_void_p(buf2.data_ptr()), 1, 1))
    assert hot.lib.ptmi_diag_update(hot.h, 1, 2, 0) == 0 and hot.lib.ptmi_diag_update(hot.h, 1, 2 * cu, 0) == 0
    torch.cuda.synchronize()
    assert not buf2.any().item()
    with pytest.raises(ValueError, match="no cold ring"):
        PTEngine.with_stages(d, 2, W, np.eye(d), cov_update=cu, tskip=0, ntemps_global=4, temp0=2, diag=True)


def _sampler(out, W, cd, ntemps=2, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 4
    s = PTSampler(d, ("iso",), ("box", -3.0 * np.ones(d), 3.0 * np.ones(d)), np.eye(d) * 0.5, outDir=str(out), verbose=False, seed=21, ntemps=ntemps,
                  nwalkers=W, keep_walkers=W, cov_mode="pooled", **kw)
    s.chain_diagnostics = cd
    return s


def test_sampler_sums_equal_the_harvested_chains_and_resume(tmp_path):
    from ptmcmcsampler_amd.diagnostics import estimates
    W, b0, L = 6, 2, 6
    cd = {"batch": b0, "levels": L}
    run = dict(burn=100, thin=1, covUpdate=50, isave=50, Tskip=10)
    p0 = np.zeros(4)
    a = _sampler(tmp_path / "a", W, cd, checkpoint=True)
    a.sample(p0, 300, **run)
    want = diag_rule(a._chains[:, 101:301], b0, L)                   # the harvested chains: another path out of the ring (_harvest)
    _same_state(a.diagnostics, want, "sampler.diagnostics")
    est = estimates(want)
    for k, v in est.items():
        assert_same(a.diagnostics[k], v, "estimate " + k)
    dg = a.diagnostics
    assert dg["last_iter"] == 300 and dg["first_iter"] == 101 and dg["n"] == 200 and dg["k"] == 100 and dg["nwalkers"] == W
    assert dg["rhat"].shape == (4,) and np.isfinite(dg["rhat"]).all() and int(dg["level"]) >= 0 and np.isfinite(dg["ess"]).all()
    f = np.load(tmp_path / "a" / "diagnostics.npz")
    assert set(f.files) == set(dg) and {"rhat", "ess", "tau", "tau_batch", "tau_walkers", "reliable", "S1", "Q", "H"} <= set(f.files)
    for k in f.files:
        assert_same(f[k], dg[k], k)
    assert not (tmp_path / "a" / "diagnostics.tmp.npz").exists()
    # stopped at 150 and resumed from its checkpoint: the sums of the uninterrupted run
    b1 = _sampler(tmp_path / "b", W, cd, checkpoint=True)
    b1.sample(p0, 150, **run)
    assert b1.diagnostics["last_iter"] == 150 and b1.diagnostics["n"] == 50
    b2 = _sampler(tmp_path / "b", W, cd, checkpoint=True, resume=True)
    b2.sample(p0, 300, **run)
    assert np.array_equal(a._chains, b2._chains)
    for k in f.files:
        assert_same(b2.diagnostics[k], dg[k], "resumed " + k)
    # a checkpoint of a run with other batches is another run's
    b3 = _sampler(tmp_path / "b", W, {"batch": 3, "levels": L}, checkpoint=True, resume=True)
    with pytest.raises(Exception, match="engine modes"):
        b3.sample(p0, 300, **run)
    # a run without the attribute writes no file and has no diagnostics; setting it late is refused
    c = _sampler(tmp_path / "c", W, False)
    c.sample(p0, 100, **run)
    assert c.diagnostics is None and not (tmp_path / "c" / "diagnostics.npz").exists() and not c.engine.diag_on
    c.chain_diagnostics = True
    with pytest.raises(ValueError, match="after the engine was built"):
        c.writeOutput(100)


def test_sampler_stop_rule(tmp_path, capsys):
    from ptmcmcsampler_amd import PTSampler
    d, W, Niter = 4, 64, 40000
    run = dict(burn=500, thin=10, covUpdate=500, isave=500)

    def make(name, cd):
        s = PTSampler(d, ("iso",), ("flat",), np.eye(d) * 0.5, outDir=str(tmp_path / name), verbose=True, seed=5, nwalkers=W, cov_mode="pooled")
        s.chain_diagnostics = cd
        return s

    s = make("stop", {"batch": 1, "levels": 16, "stop_ess": 3000, "stop_rhat": 1.05})
    s.sample(np.zeros(d), Niter, **run)
    dg = s.diagnostics
    last = int(dg["last_iter"])
    print("stopped at %d: level %d, tau %s, ess %s, rhat %s" % (last, int(dg["level"]), dg["tau"], dg["ess"], dg["rhat"]))
    assert last < Niter and last % 500 == 0 and s.Niter == last, "an iso Gaussian with ample iterations stops early"
    assert dg["reliable"].all() and dg["ess"].min() >= 3000 and dg["rhat"].max() <= 1.05
    assert last > 500 + 10 * float(dg["tau"].max())                  # not before a batch is ten autocorrelation times long
    out = capsys.readouterr().out
    assert "Run Complete with" in out and "effective samples and R-hat" in out      # one line, as the neff stop prints one
    rows = np.loadtxt(tmp_path / "stop" / "chain_1.txt", ndmin=2)
    assert rows.shape[0] == last // 10 + 1
    # one level of single samples can never be reliable (b = 1 < 10 tau): thresholds that any chain meets do not stop the run
    u = make("never", {"batch": 1, "levels": 1, "stop_ess": 1, "stop_rhat": 100.0})
    u.sample(np.zeros(d), 2000, **run)
    assert int(u.diagnostics["last_iter"]) == 2000 and not u.diagnostics["reliable"].any()
    assert u.diagnostics["ess"].min() >= 1 and u.diagnostics["rhat"].max() <= 100.0
    # without thresholds the stage only reports
    v = make("report", True)
    v.sample(np.zeros(d), 1500, **run)
    assert int(v.diagnostics["last_iter"]) == 1500
