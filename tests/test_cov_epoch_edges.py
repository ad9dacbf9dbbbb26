"""The covariance epoch's definition at the shapes where its kernels change path (csrc/ptmi_cov.hip: pool_rle_kernel, pool_syrk_kernel,
pool_reduce_kernel, pool_finish_kernel, welford_rows_kernel, welford_kernel, welford_mean_kernel): macro tiles of 112 columns with
the ones column at position d, staged chunks of 32 and 16 rows, slabs (up to 512 of them, 32 beyond d = 111) reduced in batches of
32 / 8 / 1, trips of 2048 flags and of 2048 stored rows, the per-walker kernels' switches at d = 100 and d = 112.

This file holds the SHAPE TABLES (tests/test_cov_epoch_edges_gpu.py imports them and holds the kernels to the oracle bit for bit at
every one) and pins the oracle itself at them: orc.pool_update, orc.pool_update_rle and orc.welford against the sample covariance
of every row seen so far, summed in np.longdouble -- the method and the bounds of tests/test_pooled_definition.py.  A third test
proves with host arithmetic alone that every case sits on the edge it is built for, so that a later change of a constant cannot
silently turn an edge case into a generic one."""
import numpy as np
import pytest

from oracle import oracle as orc

PS_W = 112                          # columns of a macro tile (pool_syrk_kernel); column d of the staged matrix is the ones column
CHUNK_DIAG, CHUNK_OFF = 32, 16      # rows per staged chunk on / off the diagonal
RLE_TRIP = 2048                     # flags (and list entries) per trip of pool_rle_kernel: eight groups of 256
OFFSETS = (0.0, 1e6)                # mean of the pooled data: at the origin, and 1e6 sigma away
EPOCHS = 3                          # the first takes its shift from an AM row, the later ones from mu (Chan's formula)
EPOCHS_HOST = 2                     # ... of which this file runs two: both branches, at two thirds of the longdouble products
NEW, KEY = 1, 2                     # AM row flags (include/ptmi.h)

ROW_EDGES = (2, 15, 16, 17, 31, 32, 33, 65)
COLUMN_EDGES = (1, 2, 3, 15, 16, 17, 99, 100, 111, 112, 113, 223, 224, 225)
# (d, W, cov_update).  Column edges: W = 2 or 3, cov_update walks through the row edges.
POOLED_COLUMN = [(d, 2 + k % 2, ROW_EDGES[(3 * k) % len(ROW_EDGES)]) for k, d in enumerate(COLUMN_EDGES)]
# Row edges: one walker per slab, the diagonal form alone (d = 16) and both forms (d = 112)
POOLED_ROW = [(d, 2, cu) for d in (16, 112) for cu in ROW_EDGES]
# Slab edges: a short last slab, rows per slab odd against both chunk sizes, every batch size of the reduction
POOLED_SLAB = [(99, 513, 3), (99, 1025, 5), (112, 33, 5), (113, 70, 3)]
SLAB_FACTS = {  # (d, W): (walkers per slab, slabs, walkers of the last slab, (batches of 32, of 8, of 1))
    (99, 513): (2, 257, 1, (8, 0, 1)), (99, 1025): (3, 342, 2, (10, 2, 6)), (112, 33): (2, 17, 1, (0, 2, 1)), (113, 70): (3, 24, 1, (0, 3, 0))}
POOLED_CASES = POOLED_COLUMN + POOLED_ROW + POOLED_SLAB

# RLE: the same column and slab edges under every flag pattern ...
RLE_PATTERNS = ("all", "first", "alternating", "random57", "last_stored", "last_unstored")
RLE_CASES = POOLED_COLUMN + POOLED_SLAB
# ... the trips of pool_rle_kernel (one walker per slab: rows per slab = cov_update) ...
RLE_TRIPS = [(d, 2, cu, pat) for d in (3, 112) for cu, pat in ((2047, "all"), (2048, "all"), (2049, "all"), (2047, "random57"), (2048, "random57"),
                                                                (2049, "random57"), (4100, "random60"))]
# ... and run lengths: a run that ends at the slab's end, and a first walker's last run that stops at the second walker's row 0
RLE_RUNS = [(3, 513, 4, "first"), (2, 514, 7, "last_unstored"), (5, 3, 9, "last_unstored")]

WELFORD_ROWS_D, WELFORD_TILE1_D, WELFORD_TILES_D = (1, 2, 99, 100), (101, 111, 112), (113, 224, 225)
WELFORD_CU = (3, 4, 5, 7, 8, 9, 17)
# every d meets every cov_update and every W in {1, 2, 3}
WELFORD_CASES = [(d, 1 + (k + i) % 3, cu) for k, d in enumerate(WELFORD_ROWS_D + WELFORD_TILE1_D + WELFORD_TILES_D) for i, cu in enumerate(WELFORD_CU)]


def pool_groups(d):
    """Macro tiles per side (columns 0 .. d: the ones column included)."""
    return (d + 1 + PS_W - 1) // PS_W


def slab_facts(d, W, cu):
    slab = orc.pool_slab(W, d)
    nslab = -(-W // slab)
    return dict(slab=slab, nslab=nslab, last=W - (nslab - 1) * slab, rows=slab * cu, groups=pool_groups(d),
                batches=(nslab // 32, nslab % 32 // 8, nslab % 8))


def make_flags(pattern, W, cu, rs):
    """AM row flags [W][cu] of a pattern; row 0 of every walker is a KEY row (as the engine writes it and orc.pool_update_rle requires)."""
    fl = np.zeros((W, cu), dtype=np.uint64)
    if pattern == "all":
        fl[:] = NEW
    elif pattern == "alternating":
        fl[:, ::2] = NEW
    elif pattern in ("random57", "random60", "last_stored", "last_unstored"):
        stored = rs.rand(W, cu) < (0.60 if pattern == "random60" else 0.57)
        fl[:] = np.where(stored, rs.randint(1, 4, size=(W, cu)), 0).astype(np.uint64)       # NEW, KEY or both
        if pattern == "last_stored":
            fl[:, -1] = NEW
        if pattern == "last_unstored":
            fl[:, -1] = 0
    else:
        assert pattern == "first"
    fl[:, 0] |= np.uint64(KEY)
    return fl


def make_ring(d, W, cu, offset, rs):
    """Correlated rows around a (far) non-zero mean, different for every walker."""
    A = rs.randn(d, d)
    L = np.linalg.cholesky(A @ A.T / d + 0.3 * np.eye(d))
    return (rs.randn(W, cu, d) @ L.T) + rs.randn(d) * 0.1 + rs.randn(W, 1, d) * 0.05 + offset


def expand(AM, flags):
    """The ring with every unstored row copied forward from the stored row before it."""
    stored = (flags & np.uint64(3)) != 0
    src = np.maximum.accumulate(np.where(stored, np.arange(AM.shape[1])[None, :], 0), axis=1)
    return np.take_along_axis(AM, src[:, :, None], axis=1)


def with_nan(AM, flags):
    out = AM.copy()
    out[(flags & np.uint64(3)) == 0] = np.nan
    return out


class LongRef(object):
    """Sample covariance and mean of all rows handed over so far, summed in np.longdouble about a fixed shift."""

    def __init__(self, d, shift):
        self.shift = np.longdouble(shift)
        self.n, self.s, self.S = 0, np.zeros(d, np.longdouble), np.zeros((d, d), np.longdouble)

    def add(self, rows):
        x = np.ascontiguousarray((rows.reshape(-1, rows.shape[-1]).astype(np.longdouble) - self.shift).T)       # [d][n]
        self.n += x.shape[1]
        self.s += x.sum(1)
        for i0 in range(0, len(x), 28):         # the upper triangle by row blocks (the longdouble product is the cost of this file)
            self.S[i0:i0 + 28, i0:] += np.tensordot(x[i0:i0 + 28], x[i0:], axes=(1, 1))
        return self

    def cov(self):
        S = np.triu(self.S) + np.triu(self.S, 1).T
        return np.asarray((S - np.outer(self.s, self.s) / self.n) / (self.n - 1), dtype=np.float64)

    def mean(self):
        return np.asarray(self.shift + self.s / self.n, dtype=np.float64)


WORST = {}


def _hold_pooled(cov_o, mu, ref, tag):
    c, m = ref.cov(), ref.mean()
    assert np.isfinite(cov_o).all() and np.isfinite(mu).all(), tag
    dev = np.max(np.abs(cov_o - c)) / np.max(np.abs(c))
    WORST[tag[0]] = max(WORST.get(tag[0], 0.0), dev)
    assert dev <= 1e-9, tag
    assert np.max(np.abs(mu - m)) <= 1e-12 * np.max(np.abs(m)), tag
    assert np.array_equal(cov_o, cov_o.T), tag


@pytest.mark.parametrize("d,W,cu", POOLED_CASES)
def test_pooled_rows_are_the_sample_covariance_at_the_edges(d, W, cu):
    """orc.pool_update over two epochs at every shape of the GPU file, offsets 0 and 1e6, against the longdouble sample covariance:
    1e-9 max|ref| on cov, 1e-12 relative on mu (the bounds of test_pooled_definition.py).  Observed worst deviation over all
    cases: 2.5e-11 max|ref| at offset 1e6, 1.1e-14 max|ref| at offset 0."""
    for offset in OFFSETS:
        rs = np.random.RandomState(1000 * d + W + cu)
        mu, M2, ref = np.zeros(d), np.zeros((d, d)), LongRef(d, offset)
        for ep in range(1, EPOCHS_HOST + 1):
            AM = make_ring(d, W, cu, offset, rs)
            cov_o = orc.pool_update(AM, mu, M2, ep * cu)
            _hold_pooled(cov_o, mu, ref.add(AM), (offset, d, W, cu, ep))


def _rle_epochs(d, W, cu, pattern, offset):
    rs = np.random.RandomState(1000 * d + W + cu + len(pattern))
    mu, M2, ref = np.zeros(d), np.zeros((d, d)), LongRef(d, offset)
    for ep in range(1, EPOCHS_HOST + 1):
        AM, fl = make_ring(d, W, cu, offset, rs), make_flags(pattern, W, cu, rs)
        # NaN in every unstored row: a stored-row statistic never reads them
        cov_o = orc.pool_update_rle(with_nan(AM, fl), fl, mu, M2, ep * cu)
        _hold_pooled(cov_o, mu, ref.add(expand(AM, fl)), (offset, d, W, cu, pattern, ep))


@pytest.mark.parametrize("d,W,cu", RLE_CASES)
def test_pooled_rle_is_the_sample_covariance_of_the_expanded_ring(d, W, cu):
    """orc.pool_update_rle, every flag pattern, NaN in the unstored rows, against the longdouble sample covariance of the EXPANDED ring
    (every unstored row copied forward): same bounds, every result finite.  Observed worst deviation: 6.3e-11 max|ref| at offset 1e6,
    2.1e-14 max|ref| at offset 0."""
    for pattern in RLE_PATTERNS:
        for offset in OFFSETS:
            _rle_epochs(d, W, cu, pattern, offset)


@pytest.mark.parametrize("d,W,cu,pattern", RLE_TRIPS + RLE_RUNS)
def test_pooled_rle_trips_and_run_lengths(d, W, cu, pattern):
    """The same at the trip edges of the listing (2047 / 2048 / 2049 rows, more than 2048 stored rows in a slab) and the run-length
    edges.  Observed worst deviation: 7.8e-12 max|ref| at offset 1e6, 2.0e-14 max|ref| at offset 0."""
    for offset in OFFSETS:
        _rle_epochs(d, W, cu, pattern, offset)


@pytest.mark.parametrize("d,W,cu", WELFORD_CASES)
def test_per_walker_welford_is_numpy_cov_at_the_edges(d, W, cu):
    """orc.welford per walker (the reference's recurrence, PTMCMCSampler.py:769-794), data offset 3.0, against the longdouble sample
    covariance of the walker's rows: 1e-7 max|ref| (the bound of test_pooled_definition.py).  Observed worst deviation: 5.5e-16 max|ref|."""
    rs = np.random.RandomState(1000 * d + W + cu)
    mu, M2 = np.zeros((W, d)), np.zeros((W, d, d))
    refs = [LongRef(d, 3.0) for _ in range(W)]
    for ep in range(1, EPOCHS_HOST + 1):
        AM = make_ring(d, W, cu, 3.0, rs)
        for w in range(W):
            c = orc.welford(AM[w], mu[w], M2[w], ep * cu)
            r = refs[w].add(AM[w]).cov()
            dev = np.max(np.abs(c - r)) / np.max(np.abs(r))
            WORST["welford"] = max(WORST.get("welford", 0.0), dev)
            assert dev <= 1e-7, (d, W, cu, ep, w)
            assert np.max(np.abs(mu[w] - refs[w].mean())) <= 1e-12 * np.max(np.abs(refs[w].mean()))


def test_every_case_sits_on_the_edge_it_is_built_for():
    """Host arithmetic only: the engine's slab rule (orc.pool_slab), the macro tile width, the chunk sizes, the 2048-entry trips and the
    32 / 8 / 1 reduction put every case where the tables above say."""
    # --- columns: the ones column is the last column of the only tile (111), a tile of its own (112, 224), one past that (113, 225)
    assert [pool_groups(d) for d in (1, 111, 112, 113, 223, 224, 225)] == [1, 1, 2, 2, 2, 3, 3]
    assert 111 % PS_W == PS_W - 1 and 112 % PS_W == 0 and 224 % PS_W == 0 and 223 % PS_W == PS_W - 1
    cols = {d: (W, cu) for d, W, cu in POOLED_COLUMN}
    assert set(cols) == set(COLUMN_EDGES) and {pool_groups(d) for d in cols} == {1, 2, 3}
    assert {d % 2 for d in cols} == {0, 1}                                     # PAIR and non-PAIR loads
    assert 1 in cols and 2 in cols                                             # the clamps d - 1 and d - 2 + e with nothing to spare
    assert pool_groups(224) * (pool_groups(224) - 1) // 2 == 3                 # three off-diagonal pairs
    assert all(W in (2, 3) and cu in ROW_EDGES and slab_facts(d, W, cu)["slab"] == 1 for d, (W, cu) in cols.items())
    assert {cu for W, cu in cols.values()} == set(ROW_EDGES)
    # --- rows: one walker per slab, so a slab's row count is cov_update
    for d, W, cu in POOLED_ROW:
        f = slab_facts(d, W, cu)
        assert f["slab"] == 1 and f["rows"] == cu and f["groups"] == (1 if d == 16 else 2)
    for chunk in (CHUNK_DIAG, CHUNK_OFF):
        rows = sorted({cu for d, W, cu in POOLED_ROW if d == 112})
        assert rows == sorted({cu for d, W, cu in POOLED_ROW if d == 16}) == sorted(ROW_EDGES)
        assert any(cu < chunk for cu in rows)                                  # a chunk that is never full
        assert chunk - 1 in rows and chunk in rows and chunk + 1 in rows       # one short, exactly one chunk, one row into the next
        assert 2 * chunk + 1 in rows or 4 * chunk + 1 in rows                  # one row into the next double-buffer turn
    # --- slabs
    assert {(d, W) for d, W, cu in POOLED_SLAB} == set(SLAB_FACTS)
    for d, W, cu in POOLED_SLAB:
        f = slab_facts(d, W, cu)
        slab, nslab, last, batches = SLAB_FACTS[(d, W)]
        assert (f["slab"], f["nslab"], f["last"], f["batches"]) == (slab, nslab, last, batches), (d, W)
        assert last < slab                                                     # a short last slab
        assert batches[0] * 32 + batches[1] * 8 + batches[2] == nslab
        assert all(n % CHUNK_DIAG and n % CHUNK_OFF for n in (f["rows"], last * cu))          # no slab is a multiple of a chunk
        assert nslab <= (512 if d + 1 <= PS_W else 32)
    assert {b > 0 for b in SLAB_FACTS[(99, 1025)][3]} == {True}                # all three batch sizes in one reduction
    # --- the listing's trips: flags per trip, stored rows per trip
    trips = lambda n: -(-n // RLE_TRIP)        # noqa: E731
    for d, W, cu, pattern in RLE_TRIPS:
        f = slab_facts(d, W, cu)
        assert f["slab"] == 1 and f["rows"] == cu
        rs = np.random.RandomState(1000 * d + W + cu + len(pattern))
        for ep in range(EPOCHS):
            make_ring(d, W, cu, 0.0, rs)
            fl = make_flags(pattern, W, cu, rs)
            stored = ((fl & np.uint64(3)) != 0).sum(1)                         # per slab: one walker each
            assert (stored >= 1).all()
            if pattern == "all":
                assert (stored == cu).all() and trips(cu) == {2047: 1, 2048: 1, 2049: 2}[cu]
            elif cu == 4100:
                assert trips(cu) == 3 and (stored > RLE_TRIP).all() and (stored < 2 * RLE_TRIP).all()     # the weight loop's second trip
            else:
                assert (stored < RLE_TRIP).all() and trips(cu) == {2047: 1, 2048: 1, 2049: 2}[cu]
    assert {cu for d, W, cu, p in RLE_TRIPS} == {2047, 2048, 2049, 4100} and {d for d, W, cu, p in RLE_TRIPS} == {3, 112}
    # --- run lengths
    rs = np.random.RandomState(0)
    d, W, cu, pattern = RLE_RUNS[0]
    fl = make_flags(pattern, W, cu, rs)
    assert slab_facts(d, W, cu)["slab"] == 2 and slab_facts(d, W, cu)["last"] == 1
    assert ((fl & np.uint64(3)) != 0).sum() == W                               # lists of one entry per walker: a run of cov_update rows
    assert not fl[0, -1] & np.uint64(3) and fl[1, 0] & np.uint64(KEY)          # walker 0's run must stop at walker 1's row 0
    for d, W, cu, pattern in RLE_RUNS[1:]:
        fl = make_flags(pattern, W, cu, rs)
        assert not (fl[:, -1] & np.uint64(3)).any() and (fl[:, 0] & np.uint64(KEY)).all()        # every walker's last run ends at the slab's / its ring's end
    assert slab_facts(*RLE_RUNS[1][:3])["slab"] == 2 and slab_facts(*RLE_RUNS[2][:3])["slab"] == 1
    # --- the flag patterns say what their names say
    for pattern in RLE_PATTERNS:
        fl = make_flags(pattern, 3, 9, rs)
        st = (fl & np.uint64(3)) != 0
        assert st[:, 0].all()
        assert {"all": st.all(), "first": st.sum() == 3, "alternating": st[:, ::2].all() and not st[:, 1::2].any(),
                "random57": 0 < st.sum() < st.size, "last_stored": st[:, -1].all(), "last_unstored": not st[:, -1].any()}[pattern]
    big = make_flags("random57", 64, 64, rs)
    assert {int(v) for v in np.unique(big)} == {0, NEW, KEY, NEW | KEY}        # both bits in use
    # --- per walker: welford_rows_kernel up to 100, one tile of welford_kernel up to 112, 2 x 2 and 3 x 3 tiles beyond
    tiles = lambda d: -(-d // PS_W)            # noqa: E731
    assert max(WELFORD_ROWS_D) == 100 and min(WELFORD_TILE1_D) == 101 and max(WELFORD_TILE1_D) == 112 and min(WELFORD_TILES_D) == 113
    assert [tiles(d) for d in WELFORD_TILE1_D] == [1, 1, 1] and [tiles(d) for d in WELFORD_TILES_D] == [2, 2, 3]
    for d in WELFORD_ROWS_D + WELFORD_TILE1_D + WELFORD_TILES_D:
        mine = [(W, cu) for dd, W, cu in WELFORD_CASES if dd == d]
        assert {W for W, cu in mine} == {1, 2, 3} and {cu for W, cu in mine} == set(WELFORD_CU)
    assert {cu % 8 for cu in WELFORD_CU} >= {0, 1, 7} and {cu % 4 for cu in WELFORD_CU} == {0, 1, 3}    # batches of 8 rows; 8 fetched, 4 handed over
