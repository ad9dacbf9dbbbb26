"""The covariance epoch's kernels (csrc/ptmi_cov.hip), driven directly at their tile, chunk, slab and trip edges: pool_rle_kernel,
pool_syrk_kernel in its eight forms, pool_reduce_kernel, pool_finish_kernel, welford_rows_kernel, welford_kernel, welford_mean_kernel,
am_expand_kernel and de_update_kernel.  No chain is stepped: a synthetic ring is written into an engine of one temperature, the epoch
is called through the C ABI, and mu / M2 / cov are compared with the oracle BIT FOR BIT (orc.pool_update, orc.pool_update_rle,
orc.welford), epochs 1, 2 and 3 with a fresh ring each -- the first takes its shift from an AM row in the buffer's row format, the
later ones from mu.  The shapes are the tables of tests/test_cov_epoch_edges.py, which holds the oracle to the longdouble sample
covariance at every one of them and proves on the host that each sits on its edge.  ptmi_am_expand and ptmi_update_de are held to
plain NumPy.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

import test_cov_epoch_edges as E
from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


def _engine(mods, d, W, cu, **kw):
    """One temperature, no launches: the engine is its buffers and its handle."""
    kw.setdefault("weights", (1, 0, 0))
    kw.setdefault("burn", cu)
    g = mods[2](d, 1, W, np.eye(d), cov_update=cu, tskip=0, **kw)
    assert (g.am_epl != 0) == (d == 100)                    # 100 is the only shape whose AM rows are in lane order
    return g


def _epoch(mods, g, it):
    mods[1].check(g.lib.ptmi_update_cov(g.h, it))


def _put_flags(g, fl):
    import torch
    g.t["AMflag"].copy_(torch.from_numpy(fl.astype(np.int64)))          # after put("AM"), which resets the flags to KEY


def _same_stats(g, mu, M2, cov, tag):
    assert_same(g.get("mu"), np.reshape(mu, (-1, g.d)), "mu %s" % (tag,))
    assert_same(g.get("M2"), np.reshape(M2, (-1, g.d, g.d)), "M2 %s" % (tag,))
    assert_same(g.get("cov"), np.reshape(cov, (-1, g.d, g.d)), "cov %s" % (tag,))


@pytest.mark.parametrize("d,W,cu", E.POOLED_CASES)
def test_pooled_rows_at_column_row_and_slab_edges(mods, d, W, cu):
    """pool_syrk_kernel<DIAG, false, PAIR> -> pool_reduce_kernel -> pool_finish_kernel on plain rows: the ones column as the last
    column of the only tile, as a tile of its own and one past it (d = 111 / 112, 224 / 113, 225: one, two and three tile groups, the
    off-diagonal launch and the side stream), the clamps of the PAIR and non-PAIR loads (d = 2, 1), lane-order rows (d = 100), chunks of
    32 and 16 rows never full / full / one row over, short last slabs and the 32 / 8 / 1 batches of the slab reduction."""
    orc = mods[0]
    g = _engine(mods, d, W, cu, cov_mode="pooled", am_mode="rows")
    assert not g.am_rle
    for offset in E.OFFSETS:
        rs = np.random.RandomState(1000 * d + W + cu)
        mu, M2 = np.zeros(d), np.zeros((d, d))
        for ep in range(1, E.EPOCHS + 1):
            AM = E.make_ring(d, W, cu, offset, rs)
            g.put("AM", AM)
            _epoch(mods, g, ep * cu)
            cov = orc.pool_update(AM, mu, M2, ep * cu)
            _same_stats(g, mu, M2, cov, (d, W, cu, offset, ep))


def _rle_epochs(mods, g, d, W, cu, pattern, offset):
    orc = mods[0]
    rs = np.random.RandomState(1000 * d + W + cu + len(pattern))
    mu, M2 = np.zeros(d), np.zeros((d, d))
    for ep in range(1, E.EPOCHS + 1):
        AM, fl = E.make_ring(d, W, cu, offset, rs), E.make_flags(pattern, W, cu, rs)
        AM = E.with_nan(AM, fl)                                 # NaN in every unstored row, on the device as in the oracle's buffer
        g.put("AM", AM)
        _put_flags(g, fl)
        _epoch(mods, g, ep * cu)
        cov = orc.pool_update_rle(AM, fl, mu, M2, ep * cu)
        assert np.isfinite(cov).all() and np.isfinite(mu).all()
        _same_stats(g, mu, M2, cov, (d, W, cu, pattern, offset, ep))


@pytest.mark.parametrize("d,W,cu", E.RLE_CASES)
def test_pooled_rle_at_column_and_slab_edges(mods, d, W, cu):
    """pool_rle_kernel -> pool_syrk_kernel<DIAG, true, PAIR> -> reduce -> finish at the same column and slab edges, under every flag
    pattern: every row stored, only row 0 (a list of one entry, one run of cov_update rows), alternating, 57 % stored with NEW and KEY
    bits, the last row stored and not stored.  Unstored rows hold NaN: every result is finite and equals the oracle's."""
    g = _engine(mods, d, W, cu, cov_mode="pooled", am_mode="rle")
    assert g.am_rle
    for pattern in E.RLE_PATTERNS:
        for offset in E.OFFSETS:
            _rle_epochs(mods, g, d, W, cu, pattern, offset)


@pytest.mark.parametrize("d,W,cu,pattern", E.RLE_TRIPS + E.RLE_RUNS)
def test_pooled_rle_trips_and_run_lengths(mods, d, W, cu, pattern):
    """pool_rle_kernel's trips of 2048 flags (2047 / 2048 / 2049 rows in a slab) and of 2048 list entries (as many stored rows; 4100
    rows at 60 %: the weight loop's second trip), with one and two tile groups behind them; runs that end at the slab's end, and a
    first walker's last run that stops at the second walker's row 0."""
    g = _engine(mods, d, W, cu, cov_mode="pooled", am_mode="rle")
    for offset in E.OFFSETS:
        _rle_epochs(mods, g, d, W, cu, pattern, offset)


def test_side_form_takes_every_row_of_the_ring_it_is_given(mods):
    """ptmi_update_cov_on(h, it, NULL, AM2, NULL) on an RLE handle: the statistics of the second ring with every row taken
    (orc.pool_update), whatever the handle's own flags say -- they list one row per walker here, over NaN.  Two tile groups."""
    import torch
    orc, _lib, _ = mods
    d, W, cu = 112, 3, 17
    assert E.pool_groups(d) == 2
    g = _engine(mods, d, W, cu, cov_mode="pooled", am_mode="rle")
    assert g.am_rle and g.am_epl == 0                           # the second ring below is in parameter order
    rs = np.random.RandomState(7)
    for offset in E.OFFSETS:
        mu, M2 = np.zeros(d), np.zeros((d, d))
        for ep in range(1, E.EPOCHS + 1):
            fl = E.make_flags("first", W, cu, rs)
            g.put("AM", E.with_nan(E.make_ring(d, W, cu, offset, rs), fl))
            _put_flags(g, fl)
            AM2 = E.make_ring(d, W, cu, offset, rs)
            dev = torch.from_numpy(AM2).to(g.device)
            _lib.check(g.lib.ptmi_update_cov_on(g.h, ep * cu, None, C.c_void_p(dev.data_ptr()), None))
            g.sync()
            cov = orc.pool_update(AM2, mu, M2, ep * cu)
            _same_stats(g, mu, M2, cov, ("side", offset, ep))


@pytest.mark.parametrize("d,W,cu", E.WELFORD_CASES)
def test_per_walker_kernels_at_their_switches(mods, d, W, cu):
    """The reference's recurrence per walker (PTMCMCSampler.py:769-794; orc.welford): welford_rows_kernel up to d = 100 (two walkers
    per block: an odd W leaves a slot idle; batches of 8 rows), one tile of welford_kernel<false> up to d = 112 (mu written by the
    carriers, 8 rows fetched and 4 handed over), 2 x 2 and 3 x 3 tiles with welford_mean_kernel beyond."""
    orc = mods[0]
    g = _engine(mods, d, W, cu, cov_mode="per_walker")
    rs = np.random.RandomState(1000 * d + W + cu)
    mu, M2, cov = np.zeros((W, d)), np.zeros((W, d, d)), np.zeros((W, d, d))
    for ep in range(1, E.EPOCHS + 1):
        AM = E.make_ring(d, W, cu, 3.0, rs)
        g.put("AM", AM)
        _epoch(mods, g, ep * cu)
        for w in range(W):
            cov[w] = orc.welford(AM[w], mu[w], M2[w], ep * cu)
        _same_stats(g, mu, M2, cov, (d, W, cu, ep))
        for w in range(1, W):                                   # the walkers' rings differ, and so do their results
            assert not np.array_equal(AM[w], AM[0]) and not np.array_equal(M2[w], M2[0]) and not np.array_equal(mu[w], mu[0])


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("d", [1, 100, 128, 129, 300])
def test_am_expand_on_sub_ranges(mods, d):
    """ptmi_am_expand on a synthetic period (row 0 KEY, NaN in the unstored rows), sub-ranges of walkers and iterations: the rows of the
    range equal NumPy's copy-forward -- also where the range starts on an unstored row whose stored predecessor lies before it_lo --
    and every other element of the ring keeps its bits, NaN included.  128 threads stride over a row (d = 1, 128, 129, 300); d = 100
    holds its rows in lane order."""
    _lib = mods[1]
    W, cu = 4, 12
    g = _engine(mods, d, W, cu, cov_mode="pooled", am_mode="rle")
    rs = np.random.RandomState(d)
    for base in (0, 3 * cu):                                    # ring row = iteration % cov_update
        ring = E.make_ring(d, W, cu, 0.0, rs)
        fl = E.make_flags("random57", W, cu, rs)
        fl[1, 2], fl[1, 3:6] = E.NEW, 0                         # walker 1: rows 3, 4, 5 hang on row 2
        fl[2, 1:] = 0                                           # walker 2: everything hangs on row 0
        want = E.with_nan(ring, fl)
        full = E.expand(ring, fl)
        g.put("AM", want)
        _put_flags(g, fl)
        assert np.isnan(want[1, 4]).all() and not np.isnan(want[1, 2]).any()
        for w0, nw, lo, hi in ((1, 2, 4, 9), (0, 1, 7, 7), (3, 1, 0, cu - 1), (0, W, 1, cu - 1)):
            _lib.check(g.lib.ptmi_am_expand(g.h, w0, nw, base + lo, base + hi))
            want[w0:w0 + nw, lo:hi + 1] = full[w0:w0 + nw, lo:hi + 1]
            got = g.am_params(g.t["AM"].cpu().numpy())
            assert _bits_equal(got, want), (d, base, w0, nw, lo, hi)
            if (w0, lo) == (1, 4):
                assert np.isnan(got[1, 3]).all() and np.array_equal(got[1, 4], ring[1, 2])     # row 3 lies before the range
        assert _bits_equal(got[:, 1:], full[:, 1:])


@pytest.mark.parametrize("cov_mode", ["pooled", "per_walker"])
@pytest.mark.parametrize("burn,cu", [(10, 4), (6, 6), (5, 8)])
@pytest.mark.parametrize("d", [3, 100, 104, 105])
def test_de_ring_update(mods, d, burn, cu, cov_mode):
    """ptmi_update_de (PTMCMCSampler.py:806-817 as a ring) against NumPy: drop the oldest rows and append the AM buffer -- pooled: new
    row r from walker r mod W.  A write that wraps in the middle of an epoch (burn 10, cov_update 4), cov_update == burn, and
    cov_update > burn (only the tail is kept); the piece-cyclic row formats of the 4-lane shapes (d = 3, 100, 104: padding positions
    stay zero) and rows in element order (d = 105)."""
    W = 3
    g = _engine(mods, d, W, cu, burn=burn, weights=(1, 0, 1), cov_mode=cov_mode)
    Wc = W if cov_mode == "per_walker" else 1
    assert (g.de_epl != 0) == (d <= 104) and g.de_ld == (8 * ((g.de_epl + 1) // 2) if g.de_epl else d) and g.de_ld >= d
    pad = np.zeros(0, dtype=np.int64)
    if g.de_epl:
        lane, slot = np.arange(d) % 4, np.arange(d) // 4
        pad = np.setdiff1d(np.arange(g.de_ld), 8 * (slot // 2) + 2 * lane + slot % 2)
        assert len(pad) == g.de_ld - d == {3: 5, 100: 4, 104: 0}[d]
    rs = np.random.RandomState(d + burn)
    logical = np.zeros((Wc, burn, d))
    for ep in range(5):
        AM = E.make_ring(d, W, cu, 0.0, rs)
        g.put("AM", AM)
        g.update_de()
        for wc in range(Wc):
            new = AM[wc] if cov_mode == "per_walker" else np.stack([AM[r % W, r] for r in range(cu)])
            logical[wc] = new[cu - burn:] if cu >= burn else np.concatenate([logical[wc][cu:], new])
        got = g.get("DE")
        assert got.shape == logical.shape
        assert_same(np.roll(got, -g.de_head, axis=1), logical, "DE d=%d burn=%d cu=%d %s epoch %d" % (d, burn, cu, cov_mode, ep))
        assert (g.t["DE"].cpu().numpy()[..., pad] == 0.0).all()
    assert g.de_head == (5 * min(cu, burn)) % burn
