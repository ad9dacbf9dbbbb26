"""eig_mode="ql" beyond 128 parameters: ptmi_eig_ql's wide kernels (csrc/ptmi_eig_wide.hip -- the matrix in a global scratch, the
apply step tiled over rows, the finish across the tiles, the scratch in batches) against the oracle's orc_eig_ql bit for bit: alone,
in batches, with chain and rows together, inside whole runs (pooled, per-walker, eig_lag), with parameter groups, at the bounds and through the
sampler facade."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle as orc
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    _lib.load()
    assert _lib.device_count() >= 1, "no MI355X visible"
    return orc, _lib, PTEngine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    if a.dtype.kind == "f":
        bad = _bits(a) != _bits(b)
        bad &= ~(np.isnan(a) & np.isnan(b))
        assert not bad.any(), "%s: %d of %d differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])
    else:
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), what


def _spd(d, rs, floor=0.1):
    A = rs.randn(d, d)
    c = A @ A.T / d + floor * np.eye(d)
    return (c + c.T) / 2


def _six(d):
    """Three scaled random SPD matrices, the sample covariance of 3000 isotropic rows, 0.01 I, zeros."""
    rs = np.random.RandomState(200 + d)
    X = rs.randn(3000, d)
    return np.stack([_spd(d, rs) * 10.0 ** rs.uniform(-4, 2) for _ in range(3)] + [np.cov(X.T).reshape(d, d), np.eye(d) * 0.01, np.zeros((d, d))])


def _many(d, W):
    """W matrices of the same four kinds in turn."""
    rs = np.random.RandomState(300 + d)
    out = []
    for w in range(W):
        kind = w % 4 if w < W - 2 else 2 + w - (W - 2)
        if kind == 0:
            out.append(_spd(d, rs) * 10.0 ** rs.uniform(-4, 2))
        elif kind == 1:
            out.append(np.cov(rs.randn(3 * d, d).T).reshape(d, d))
        elif kind == 2:
            out.append(np.eye(d) * 0.01)
        else:
            out.append(np.zeros((d, d)))
    return np.stack(out)


_oracle = {}


def _oracle_of(orc, key, covs):
    """orc_eig_ql of every matrix, computed once per set."""
    if key not in _oracle:
        res = [orc.eig_ql(c) for c in covs]
        assert all(r[2] >= 0 for r in res)                          # every one converged
        _oracle[key] = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]))
    return _oracle[key]


def _device(mods, covs):
    orc, _lib, PTEngine = mods
    W, d = covs.shape[:2]
    g = PTEngine(d, 1, W, np.eye(d), weights=(1, 0, 0), cov_update=4, burn=4, tskip=0, eig_mode="ql")
    g.put("cov", covs)
    _lib.check(g.lib.ptmi_eig_ql(g.h))
    g.sync()
    return g.get("Ut")[:, 0].copy(), g.get("S")[:, 0].copy()


@pytest.mark.parametrize("d", [129, 130, 192, 257, 513])
def test_wide_ql_is_bit_identical_to_the_oracle(mods, d):
    """129: one row past two waves, odd; 130: even; 192: three waves of rows; 257 / 513: a row past the 256- / 512-thread blocks."""
    covs = _six(d)
    oUt, oS = _oracle_of(mods[0], ("six", d), covs)
    Ut, S = _device(mods, covs)
    for w in range(len(covs)):
        assert_same(Ut[w], oUt[w], "Ut d=%d w=%d" % (d, w))
        assert_same(S[w], oS[w], "S d=%d w=%d" % (d, w))


def test_many_matrices_in_batches(mods):
    """70 matrices of 129 x 129 (past the 64-matrix switch of the dispatch below 128), one batch: all equal the oracle."""
    d, W = 129, 70
    covs = _many(d, W)
    oUt, oS = _oracle_of(mods[0], ("many", d, W), covs)
    Ut, S = _device(mods, covs)
    assert_same(Ut, oUt, "Ut")
    assert_same(S, oS, "S")


def test_two_batches_under_the_budget(mods):
    """The scratch is 14 782 616 bytes per 513 x 513 matrix (z, the record of 3 n^2 rotations, de, ev, the headers) and the budget
    4096 MB: 290 matrices a batch.  296 matrices -- the six kinds in turn, so the oracle's six factorizations cover them all -- are a
    full batch and a partial one of 6; a matrix's bits do not depend on the batch or the place it has in it."""
    d, W = 513, 296
    per = 8 * (d * d + 2 * d + 2 * 3 * d * d + d) + 4 * (2 * 8 * d + 2)
    assert (4096 << 20) // per == 290 < W
    six = _six(d)
    oUt, oS = _oracle_of(mods[0], ("six", d), six)
    idx = np.arange(W) % 6
    Ut, S = _device(mods, six[idx])
    for k in range(6):
        sel = idx == k
        assert_same(Ut[sel], np.broadcast_to(oUt[k], Ut[sel].shape), "Ut, kind %d" % k)
        assert_same(S[sel], np.broadcast_to(oS[k], S[sel].shape), "S, kind %d" % k)


def test_chain_and_rows_together(mods, monkeypatch):
    """PTMI_QL_SPLIT = 0 beyond 128: the record gets no room, every matrix that rotates at all is flagged by the chain kernel and
    redone with the chain and the rows together (what a matrix whose rotations overflow the 3 n^2 record takes); the same bits as the
    oracle and as the recorded form (the scratch's flag word is not exposed)."""
    d = 129
    covs = _six(d)[[0, 3, 4]]
    oUt, oS = _oracle_of(mods[0], ("redo", d), covs)
    monkeypatch.setenv("PTMI_QL_SPLIT", "1")
    Ut0, S0 = _device(mods, covs)
    monkeypatch.setenv("PTMI_QL_SPLIT", "0")
    Ut1, S1 = _device(mods, covs)
    assert_same(Ut1, oUt, "Ut, together")
    assert_same(S1, oS, "S, together")
    assert_same(Ut0, Ut1, "Ut, recorded against together")
    assert_same(S0, S1, "S, recorded against together")


@pytest.mark.parametrize("cov_mode,d,nt,W,lag", [("per_walker", 130, 2, 3, 0), ("pooled", 129, 2, 8, 0), ("per_walker", 130, 2, 3, 1)])
def test_sampling_with_the_wide_eigensolver_matches_oracle(mods, cov_mode, d, nt, W, lag):
    """A whole run adapted through the wide kernels (lag = 1: ptmi_eig_ql_from on the side stream): every array equals the oracle's."""
    orc, _lib, PTEngine = mods
    kw = dict(weights=(20, 20, 20), cov_update=40, burn=80, tskip=10, seed=5, cov_mode=cov_mode, eig_mode="ql", eig_lag=lag)
    rs = np.random.RandomState(3)
    cov0, p0 = _spd(d, rs) * 0.01, rs.randn(W, nt, d) * 0.3
    g, o = PTEngine(d, nt, W, cov0, **kw), orc.OracleEngine(d, nt, W, cov0, **kw)
    assert g.eig_lag == lag and o.eig_lag == lag
    for e in (g, o):
        e.init_state(p0)
        e.run(170)
    g.sync()
    for name in ("X", "lnL", "slot_of", "nacc", "jstat", "nswap", "cov", "Ut", "S") + (("AM",) if cov_mode == "per_walker" else ()):
        assert_same(g.get(name), getattr(o, name), name)
    assert g.eig_epochs == 4 and o.jstat[..., 1, 1].sum() > 0


@pytest.mark.parametrize("cov_mode,W", [("pooled", 4), ("per_walker", 2)])
@pytest.mark.parametrize("d,groups", [(200, [list(range(0, 129)), list(range(129, 199)), [199]]), (150, [list(range(75)), list(range(75, 150))])])
def test_parameter_groups_beyond_128_parameters(mods, d, groups, cov_mode, W):
    """One wide group, one LDS-sized group and a singleton at 200-d; two groups of 75 at 150-d (refused before only because
    ndim > 128): two covariance epochs against OracleEngine(groups=..., eig_mode="ql")."""
    orc, _lib, PTEngine = mods
    kw = dict(groups=groups, weights=(20, 20, 20), cov_update=40, burn=80, tskip=10, seed=17, cov_mode=cov_mode, eig_mode="ql")
    rs = np.random.RandomState(d + 1)
    cov0, p0 = _spd(d, rs) * 0.01, rs.randn(W, 2, d) * 0.3
    g, o = PTEngine(d, 2, W, cov0, **kw), orc.OracleEngine(d, 2, W, cov0, **kw)
    for e in (g, o):
        e.init_state(p0)
        e.run(90)
    g.sync()
    assert g.eig_epochs == 2
    for name in ("X", "lnL", "slot_of", "nacc", "jstat", "nswap", "cov", "Ut", "S"):
        assert_same(g.get(name), getattr(o, name), name)


def test_the_largest_order_decomposes_its_matrix(mods):
    """1024 x 1024, one pooled matrix (the oracle takes several seconds there: held to the decomposition)."""
    orc, _lib, PTEngine = mods
    d = 1024
    g = PTEngine(d, 2, 2, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=100, burn=1000, tskip=10, seed=1, cov_mode="pooled",
                 use_de_buffer=False, eig_mode="ql")
    g.init_state(np.zeros(d))
    rs = np.random.RandomState(7)
    cov = _spd(d, rs) * 3.0e-3
    g.put("cov", cov[None])
    _lib.check(g.lib.ptmi_eig_ql(g.h))
    g.sync()
    Ut, S = g.get("Ut")[0, 0], g.get("S")[0, 0]
    assert np.abs((Ut.T * S) @ Ut - cov).max() <= 1e-12 * np.abs(cov).max()
    assert np.abs(Ut @ Ut.T - np.eye(d)).max() <= 1e-12
    assert (np.diff(S) <= 0).all() and (S >= 0).all()


def test_beyond_1024_is_refused(mods):
    orc, _lib, PTEngine = mods
    d = 1025
    g = PTEngine(d, 2, 2, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=100, burn=1000, tskip=10, seed=1, cov_mode="pooled",
                 use_de_buffer=False, eig_mode="ql")
    with pytest.raises(_lib.PtmiError, match="1024"):
        _lib.check(g.lib.ptmi_eig_ql(g.h))


@pytest.mark.parametrize("split", ["0", "1"])
def test_the_dispatch_at_128_is_intact(mods, split, monkeypatch):
    monkeypatch.setenv("PTMI_QL_SPLIT", split)
    d = 128
    covs = _six(d)
    oUt, oS = _oracle_of(mods[0], ("six", d), covs)
    Ut, S = _device(mods, covs)
    assert_same(Ut, oUt, "Ut")
    assert_same(S, oS, "S")


def test_sampler_facade_at_130_parameters(mods, tmp_path):
    orc, _lib, PTEngine = mods
    from ptmcmcsampler_amd.sampler import PTSampler
    d = 130
    s = PTSampler(d, ("iso",), ("flat",), np.eye(d) * 0.01, nwalkers=2, ntemps=2, eig_mode="ql", outDir=str(tmp_path), verbose=False, seed=3)
    s.sample(np.zeros(d), 200, covUpdate=100, burn=1000, thin=10, isave=100, Tskip=10)
    g = s.engine
    g.sync()
    assert g.eig_mode == "ql" and g.eig_epochs >= 1
    cov, Ut, S = g.get("cov"), g.get("Ut")[:, 0], g.get("S")[:, 0]
    for w in range(cov.shape[0]):
        oUt, oS, iters = orc.eig_ql(cov[w])
        assert iters >= 0
        assert_same(Ut[w], oUt, "Ut w=%d" % w)
        assert_same(S[w], oS, "S w=%d" % w)
