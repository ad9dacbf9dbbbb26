"""The likelihood callback only inside the prior's support on the device callback path (csrc/ptmi_sup.hip, ``PTEngine.with_stages(...,
logl_in_support=True)``; the reference: ``lp = logp(y)``, ``logl(y)`` only when ``lp != -inf``, PTMCMCSampler.py:605-612, and the first
evaluation at :479-487).

  1. the kernels through the C ABI against NumPy, exact: the count, the compacted rows, the scattered values, every call twice;
  2. engines with the stage on and off, one launch per iteration and two: every buffer equal after every segment, the stage-on engine
     equal to the oracle, no row outside the box ever reaches the likelihood, and a quarter or so of the rows is skipped;
  3. a likelihood that raises -- or returns NaN -- outside the box runs with the stage and not without it;
  4. the stage beside custom, auxiliary and gradient jumps; graph mode falls back with the same bits;
  5. the sampler facade: ``s.logl_in_support = True`` changes no chain file.

Callbacks whose bits for a row do not depend on the number of rows (the library's own row kernels; element-wise torch with the sum
spelled out column by column), so that "the same chains" means the same bits.  Run on the GPU box: ``python -m pytest tests -m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_parity import _compare, assert_same, mods  # noqa: F401  (mods is a fixture)
from test_split_rows_gpu import NAMES, _same, _snapshot

pytestmark = pytest.mark.gpu

NINF = -np.inf


# ------------------------------------------------------------------------------------------------------ 1. the kernels, exact
@pytest.fixture(scope="module")
def handles(mods):
    """A small split handle per ndim (the stage reads ndim and the stream from it and nothing else)."""
    orc, _lib, PTEngine = mods
    made = {}

    def get(d):
        if d not in made:
            made[d] = PTEngine(d, 2, 3, np.eye(d) * 0.01, weights=(20, 0, 0), split=True)
        return made[d]

    return get


def _patterns(n_in, rs):
    half = np.where(rs.rand(n_in) < 0.5, rs.randn(n_in), NINF)
    out = [("all finite", rs.randn(n_in)), ("all -inf", np.full(n_in, NINF)), ("a seeded half", half)]
    first = np.full(n_in, NINF)
    first[0] = 0.25
    last = np.full(n_in, NINF)
    last[-1] = -3.0
    out += [("only the first row", first), ("only the last row", last)]
    if n_in > 2048:
        hole = half.copy()
        hole[1024:2048] = NINF                                        # a whole listing block without a row, mixed neighbours
        assert np.isfinite(hole[:1024]).any() and np.isfinite(hole[2048:]).any()
        out.append(("a middle block of 1024 rows -inf", hole))
    odd = half.copy()
    odd[rs.rand(n_in) < 0.2] = np.nan                                 # listed: the reference tests lp == -inf and nothing else
    odd[rs.rand(n_in) < 0.2] = np.inf
    odd[0 if n_in < 3 else 2] = np.nan
    odd[-1] = np.inf
    out.append(("NaN and +inf entries", odd))
    return out


class _Stage(object):
    """ptmi_sup_* on one handle and one work area."""

    def __init__(self, _lib, g, n_in):
        import torch
        self.torch, self._lib, self.g, self.n_in = torch, _lib, g, n_in
        nb = C.c_size_t(0)
        _lib.check(g.lib.ptmi_sup_work_bytes(g.h, n_in, C.byref(nb)))
        assert nb.value >= 8 * n_in + 8 and nb.value % 16 == 0
        self.work = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device=g.device)

    def begin(self, lp):
        n = C.c_int64(-7)
        self._lib.check(self.g.lib.ptmi_sup_begin(self.g.h, self.work.data_ptr(), lp.data_ptr(), self.n_in, C.byref(n)))
        return n.value

    def pos(self):
        self.g.sync()
        return self.work[:4 * self.n_in].view(self.torch.int32).cpu().numpy().copy()

    FILL32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]           # what the work area holds where the stage wrote nothing

    def tables(self):
        """pos [n_in] and list [n_in] (entries beyond the count: never written)."""
        self.g.sync()
        n, off = self.n_in, (4 * self.n_in + 15) & ~15
        w = self.work.cpu().numpy()
        return w[:4 * n].view(np.int32).copy(), w[off:off + 4 * n].view(np.int32).copy()

    def rows(self, rows_in, rows):
        self._lib.check(self.g.lib.ptmi_sup_rows(self.g.h, self.work.data_ptr(), rows_in.data_ptr(), rows.data_ptr()))

    def end(self, vals, out):
        self._lib.check(self.g.lib.ptmi_sup_end(self.g.h, self.work.data_ptr(), vals.data_ptr() if vals is not None else None, out.data_ptr()))


def _check_listing(_lib, g, d, n_in, rs, patterns):
    """ptmi_sup_begin / _rows / _end on every pattern of ``patterns(n_in, rs)`` (drawn behind the rows) against
    np.flatnonzero(lp != -inf) and its inverse, exact, every call twice."""
    import torch
    SENT, PAD = -77.25, 8
    rows_np = rs.randn(n_in, d)
    rows_in = torch.from_numpy(rows_np).to(g.device)
    for what, lp_np in patterns(n_in, rs):
        what = "%s, n_in=%d, d=%d" % (what, n_in, d)
        mask = ~np.isneginf(lp_np)
        rank = np.cumsum(mask) - 1
        n_want = int(mask.sum())
        want_list = np.flatnonzero(mask)
        vals_np = rs.randn(max(n_want, 1))
        lp, vals = torch.from_numpy(lp_np).to(g.device), torch.from_numpy(vals_np).to(g.device)
        want_out = np.where(mask, vals_np[np.maximum(rank, 0)], NINF)
        got = []
        for rep in range(2):                                          # a second call gives the same bytes
            st = _Stage(_lib, g, n_in)
            n = st.begin(lp)
            assert n == n_want, what
            pos, lst = st.tables()
            assert np.array_equal(pos, np.where(mask, rank, -1)), what + ": pos"
            assert np.array_equal(lst[:n], want_list), what + ": list"
            assert (lst[n:] == _Stage.FILL32).all(), what + ": list beyond n is not touched"
            rows = torch.full((n_in + PAD, d), SENT, dtype=torch.float64, device=g.device)
            if 0 < n:                                                 # (n == n_in too: the caller may skip the copy, the kernel may not get it wrong)
                st.rows(rows_in, rows)
            out = torch.full((n_in + PAD,), SENT, dtype=torch.float64, device=g.device)
            st.end(vals if n else None, out)
            g.sync()
            r, o = rows.cpu().numpy(), out.cpu().numpy()
            assert_same(r[:n], rows_np[mask], what + ": rows")
            assert (r[n:] == SENT).all(), what + ": rows beyond n are not touched"
            assert_same(o[:n_in], want_out, what + ": out")
            assert (o[n_in:] == SENT).all(), what + ": out beyond n_in is not touched"
            got.append((r.tobytes(), o.tobytes(), st.pos().tobytes()))
        assert got[0] == got[1], what
        # vals == NULL: -inf everywhere, whatever was listed
        st = _Stage(_lib, g, n_in)
        assert st.begin(lp) == n_want
        out = torch.full((n_in + PAD,), SENT, dtype=torch.float64, device=g.device)
        st.end(None, out)
        g.sync()
        o = out.cpu().numpy()
        assert np.isneginf(o[:n_in]).all() and (o[n_in:] == SENT).all(), what


@pytest.mark.parametrize("n_in", [1, 63, 64, 65, 1024, 1025, 2100, 3073])
@pytest.mark.parametrize("d", [1, 5, 6])
def test_listing_rows_and_values_against_numpy(mods, handles, d, n_in):
    """Waves and blocks that are full, one short and one over; one, two, three and four listing blocks; odd and even ndim.  (At most
    four blocks: sup_scan_kernel's cross-wave sums and its carry stay zero here -- test_listing_beyond_one_wave_of_blocks.)"""
    orc, _lib, PTEngine = mods
    rs = np.random.RandomState(1000 * d + n_in)
    _check_listing(_lib, handles(d), d, n_in, rs, _patterns)


LB = 1024                                                             # rows per block of the listing kernels (csrc/ptmi_sup.hip)


def _block_patterns(n_in, rs):
    """Patterns chosen from the BLOCK index: with the same count in every block a wrong start offset of a block can cancel; here the
    counts differ from block to block, and whole blocks, wave-ends of the scan included, are empty."""
    b = np.arange(n_in) // LB
    nblk = int(b[-1]) + 1
    half = np.where(rs.rand(n_in) < 0.5, rs.randn(n_in), NINF)
    one = np.full(n_in, NINF)
    one[np.minimum((np.arange(nblk) + 1) * LB, n_in) - 1] = rs.randn(nblk)
    tail = np.where(b == nblk - 1, half, NINF)
    tail[-1] = 0.5
    dense = np.where(rs.rand(n_in) < (b % 7) / 6.0, rs.randn(n_in), NINF)
    assert np.isneginf(dense[:min(LB, n_in)]).all() and (nblk < 7 or np.isfinite(dense[6 * LB:min(7 * LB, n_in)]).all())
    return [("one row per block, the block's last", one),
            ("rows in the last block only", tail),
            ("every block but block 0", np.where(b == 0, NINF, half)),
            ("every block but those = 63 (mod 64)", np.where(b % 64 == 63, NINF, half)),
            ("a density per block, (b % 7) / 6", dense)]


BIG = [
    # n_in, blocks, chunks of 1024 block counts
    (65536, 64, 1),                                                   # the last size one wave of sup_scan_kernel serves: wtot[1..] = 0
    (65537, 65, 1),                                                   # one block in wave 1: wtot[0] is added for the first time
    (66561, 66, 1),                                                   # ... a second block behind it, ragged
    (1048576, 1024, 1),                                               # exactly one chunk: every wtot[k], no carry yet
    (1048577, 1025, 2),                                               # the carry with a single block behind it
    (2098177, 2050, 3),                                               # three chunks, a ragged last block
]


@pytest.mark.parametrize("n_in,nblk,nchunk", BIG)
@pytest.mark.parametrize("d", [1, 2])
def test_listing_beyond_one_wave_of_blocks(mods, handles, d, n_in, nblk, nchunk):
    """sup_scan_kernel (ONE block of 1024 threads over the block counts) beyond the sizes an engine of a few thousand chains gives it:
    from 65 blocks on its cross-wave sums wtot[k], k >= 1, are non-zero -- a block's start is carry + wtot[0 .. wv) + the wave's own
    scan --, from 1025 blocks on the running ``carry`` from one chunk of 1024 block counts to the next.  Sizes on both sides of each
    threshold, 8-byte and 16-byte pieces (d = 1, 2), the patterns of the small test and five more that depend on the block index.  The
    block count is checked against the library's own (the work area holds two int32 per block), so another LB fails here first."""
    orc, _lib, PTEngine = mods
    g = handles(d)
    assert nblk == -(-n_in // LB) and nchunk == -(-nblk // LB)
    assert (nblk > 64) == (n_in > 65536) and (nchunk > 1) == (n_in > 1048576)
    al16 = lambda v: (v + 15) & ~15                                   # noqa: E731
    nb = C.c_size_t(0)
    _lib.check(g.lib.ptmi_sup_work_bytes(g.h, n_in, C.byref(nb)))
    assert nb.value == 2 * al16(4 * n_in) + 2 * al16(4 * nblk) + 16   # pos, list, bcnt, boff, n
    rs = np.random.RandomState(7 * n_in + d)
    _check_listing(_lib, g, d, n_in, rs, lambda n, r: _patterns(n, r) + _block_patterns(n, r))


def test_the_stage_refuses_calls_out_of_sequence(mods, handles):
    import torch
    orc, _lib, PTEngine = mods
    g = handles(6)
    L, h = g.lib, g.h
    n_in = 100
    st, other = _Stage(_lib, g, n_in), _Stage(_lib, g, n_in)
    lp = torch.zeros(n_in, dtype=torch.float64, device=g.device)
    lp[::3] = NINF
    rows_in = torch.zeros((n_in, 6), dtype=torch.float64, device=g.device)
    rows, out = torch.zeros_like(rows_in), torch.zeros_like(lp)
    n = C.c_int64(0)
    nb = C.c_size_t(0)
    for bad in (0, -5):
        with pytest.raises(_lib.PtmiError, match="n_in"):
            _lib.check(L.ptmi_sup_work_bytes(h, bad, C.byref(nb)))
        with pytest.raises(_lib.PtmiError, match="n_in"):
            _lib.check(L.ptmi_sup_begin(h, st.work.data_ptr(), lp.data_ptr(), bad, C.byref(n)))
    with pytest.raises(_lib.PtmiError, match="ptmi_sup_begin first"):
        st.rows(rows_in, rows)
    with pytest.raises(_lib.PtmiError, match="ptmi_sup_begin first"):
        st.end(None, out)
    with pytest.raises(_lib.PtmiError, match="16-byte aligned"):
        _lib.check(L.ptmi_sup_begin(h, st.work.data_ptr() + 8, lp.data_ptr(), n_in, C.byref(n)))
    with pytest.raises(_lib.PtmiError, match="NULL"):
        _lib.check(L.ptmi_sup_begin(h, st.work.data_ptr(), None, n_in, C.byref(n)))
    assert st.begin(lp) == n_in - 34
    with pytest.raises(_lib.PtmiError, match="not the work area"):
        other.rows(rows_in, rows)
    with pytest.raises(_lib.PtmiError, match="not the work area"):
        other.end(None, out)
    with pytest.raises(_lib.PtmiError, match="16-byte aligned"):     # even ndim: 16-byte pieces
        _lib.check(L.ptmi_sup_rows(h, st.work.data_ptr(), rows_in.data_ptr() + 8, rows.data_ptr()))
    with pytest.raises(_lib.PtmiError, match="8-byte aligned"):
        _lib.check(L.ptmi_sup_end(h, st.work.data_ptr(), None, out.data_ptr() + 4))
    with pytest.raises(_lib.PtmiError, match="16-byte aligned"):     # a refused ptmi_sup_begin changes nothing either
        _lib.check(L.ptmi_sup_begin(h, other.work.data_ptr() + 8, lp.data_ptr(), n_in, C.byref(n)))
    st.rows(rows_in, rows)                                            # the refused calls left the stage open
    st.end(None, out)
    with pytest.raises(_lib.PtmiError, match="ptmi_sup_begin first"):    # ... and ptmi_sup_end closed it
        st.end(None, out)
    # odd ndim copies 8-byte pieces: rows at any 8-byte boundary
    g5 = handles(5)
    s5 = _Stage(_lib, g5, 4)
    big = torch.arange(6 * 5 + 1, dtype=torch.float64, device=g5.device)
    lp5 = torch.tensor([0.0, NINF, NINF, 1.0], dtype=torch.float64, device=g5.device)
    assert s5.begin(lp5) == 2
    dst = torch.zeros((4, 5), dtype=torch.float64, device=g5.device)
    _lib.check(g5.lib.ptmi_sup_rows(g5.h, s5.work.data_ptr(), big.data_ptr() + 8, dst.data_ptr()))
    g5.sync()
    assert dst[:2].cpu().numpy().tolist() == [[1, 2, 3, 4, 5], [16, 17, 18, 19, 20]]
    # not in device-iteration (graph) mode: the count is read on the host
    _lib.check(L.ptmi_device_iter(h, 1))
    try:
        with pytest.raises(_lib.PtmiError, match="ptmi_device_iter"):
            _lib.check(L.ptmi_sup_begin(h, st.work.data_ptr(), lp.data_ptr(), n_in, C.byref(n)))
    finally:
        _lib.check(L.ptmi_device_iter(h, 0))


# ------------------------------------------------------------------------------------ 2. engines with the stage on and off, the oracle
class _Watch(object):
    """The library's own prior and likelihood row kernels as callbacks that keep count on the device: rows the prior let through, rows
    the likelihood was handed, and how many of those lay outside the box."""

    def __init__(self, g, lo, hi):
        import torch
        self.torch = torch
        self.logp0, self.logl0 = g.builtin_logp(), g.builtin_logl()
        self.lo, self.hi = torch.as_tensor(lo, device=g.device), torch.as_tensor(hi, device=g.device)
        z = lambda: torch.zeros((), dtype=torch.int64, device=g.device)   # noqa: E731
        self.inside, self.given, self.outside = z(), z(), z()

    def logp(self, X):
        lp = self.logp0(X)
        self.inside += (lp != NINF).sum()
        return lp

    def logl(self, X):
        self.given += X.shape[0]
        self.outside += ((X < self.lo) | (X > self.hi)).any(-1).sum()
        return self.logl0(X)


def _box_case(d, nt, W, half):
    rs = np.random.RandomState(d + nt)
    hw = half + (0.1 if half > 0.3 else 0.05) * rs.rand(d)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.05
    return -hw, hw, cov0, p0


@pytest.mark.parametrize("d,nt,W,half", [(6, 4, 300, 0.4),           # 1200 slots: two listing blocks, the second partial
                                         (5, 3, 700, 0.4),           # 2100: three blocks, odd ndim
                                         (100, 4, 37, 0.12)])        # 148 slots; a box tight enough at 100-d
def test_stage_on_equals_stage_off_and_the_oracle(mods, d, nt, W, half):
    """evaluated / offered in [0.40, 0.95]: on the CPU oracle with these inputs the acceptance over the 105 iterations is 0.47-0.64,
    0.52-0.64, 0.60-0.71 with the box and 0.80-0.82, 0.80-0.81, 0.93 with a flat prior, i.e. at most 0.44 / 0.42 / 0.36 and about a
    quarter of the proposals have lp = -inf; a run that never skipped anything does not pass."""
    orc, _lib, PTEngine = mods
    lo, hi, cov0, p0 = _box_case(d, nt, W, half)
    kw = dict(weights=(20, 20, 20), cov_update=20, burn=40, tskip=7, seed=31, logp=("box", lo, hi))
    o = orc.OracleEngine(d, nt, W, cov0, **kw)
    o.init_state(p0)
    runs = []
    for fused in (True, False):
        pair = []
        for on in (True, False):
            g = PTEngine.with_stages(d, nt, W, cov0, split=True, logl_in_support=on, **kw)
            w = _Watch(g, lo, hi)
            cb = (w.logl, w.logp)
            g.init_state_callback(p0, *cb)
            pair.append((g, w, cb))
        runs.append((fused, pair))
    for n in (25, 3, 1, 46, 30):                                      # covariance epochs, DE activation and swaps inside
        o.run(n)
        for fused, pair in runs:
            snaps = []
            for g, w, cb in pair:
                g.run_callback(n, cb[0], cb[1], fused=fused)
                snaps.append(_snapshot(g))
            what = "fused=%s at iteration %d" % (fused, pair[0][0].iter)
            _same(snaps[0], snaps[1], "stage on vs off, " + what)
            _compare(pair[0][0], o, "stage on vs the oracle, %s: " % what)
    offered = W * nt * 106                                            # the first evaluation and 105 iterations
    for fused, ((g, w, _), (g_off, w_off, _)) in runs:
        inside, given, outside = int(w.inside), int(w.given), int(w.outside)
        what = "d=%d fused=%s: offered %d, inside the support %d, handed to logl %d (%.3f), of those outside %d; stage off: handed %d, outside %d" % (
            d, fused, offered, inside, given, given / offered, outside, int(w_off.given), int(w_off.outside))
        assert outside == 0, what
        assert g.support_counts == (offered, inside) and given == inside, what
        assert 0.40 <= given / offered <= 0.95, what
        assert g_off.support_counts == (0, 0) and int(w_off.given) == offered and int(w_off.outside) == offered - int(w_off.inside) > 0, what
    assert o.nswap.sum() > 0 and o.jstat[..., 2, 0].sum() > 0 and o.jstat[..., 1, 1].sum() > 0


# ----------------------------------------------------------------------------- 3. a likelihood that cannot stand a row outside
def _colsum(T, d):
    """The row sums of T [n, d] spelled out column by column: the same bits for a row whatever n is."""
    s = T[:, 0]
    for j in range(1, d):
        s = s + T[:, j]
    return s


def _columns(X, d):
    return _colsum(X * X, d)


@pytest.mark.parametrize("how", ["raises", "nan"])
def test_a_likelihood_defined_only_inside_the_support(mods, how):
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 3, 50
    lo, hi, cov0, p0 = _box_case(d, nt, W, 0.4)
    p0[::7, 0, 0] = hi[0] + 0.3                                       # some chains start outside the box
    p0[3, 2, 4] = lo[4] - 1.0
    started_out = ((p0 < lo) | (p0 > hi)).any(-1)
    assert 0 < started_out.sum() < W * nt
    lo_t, hi_t = torch.as_tensor(lo, device="cuda"), torch.as_tensor(hi, device="cuda")
    nans = torch.zeros((), dtype=torch.int64, device="cuda")

    def logp(X):
        return torch.where(((X >= lo_t) & (X <= hi_t)).all(-1), 0.0, NINF).to(torch.float64)

    def logl(X):
        # a Gaussian times a density on the box, sum of log(hi - x) + log(x - lo): NaN outside the box
        v = -0.5 * _columns(X, d) + 1e-3 * _colsum(torch.log(hi_t - X) + torch.log(X - lo_t), d)
        bad = torch.isnan(v)
        if how == "raises":
            if bool(bad.any()):
                raise FloatingPointError("logl was handed %d rows outside the prior's support" % int(bad.sum()))
        else:
            nans.add_(bad.sum())
        return v

    kw = dict(weights=(20, 20, 20), cov_update=20, burn=40, tskip=7, seed=31, split=True)
    g = PTEngine.with_stages(d, nt, W, cov0, logl_in_support=True, **kw)
    g.init_state_callback(p0, logl, logp)
    assert np.isneginf(g.get("lnL")[started_out]).all() and np.isfinite(g.get("lnL")[~started_out]).all()
    assert g.support_counts == (W * nt, W * nt - int(started_out.sum()))
    for n, fused in ((25, True), (25, False), (50, True)):
        g.run_callback(n, logl, logp, fused=fused)
    g.sync()
    assert g.iter == 100 and int(nans) == 0
    lnL, X = g.get("lnL"), g.get("X")
    inside = ((X >= lo) & (X <= hi)).all(-1)
    # (a chain inside never leaves; one that started outside stays at -inf until a proposal of its own lands inside)
    assert np.isfinite(lnL[inside]).all() and np.isneginf(lnL[~inside]).all() and inside.sum() >= (~started_out).sum()
    assert g.support_counts[0] == 101 * W * nt and 0 < g.support_counts[1] < g.support_counts[0]
    assert 0 < g.get("nacc").sum() < 100 * W * nt
    # the same configuration with the stage off, from a start inside the box: the first segment meets a row outside
    off = PTEngine.with_stages(d, nt, W, cov0, logl_in_support=False, **kw)
    off.init_state_callback(np.clip(p0, lo * 0.9, hi * 0.9), logl, logp)
    if how == "raises":
        with pytest.raises(FloatingPointError, match="outside the prior's support"):
            off.run_callback(25, logl, logp)
    else:
        off.run_callback(25, logl, logp)
        off.sync()
        assert int(nans) > 0 and off.support_counts == (0, 0)


def test_logl_must_return_n_values(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 2, 5
    g = PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, split=True, logl_in_support=True)
    p0 = np.zeros((W, nt, d))
    p0[1, 1, 2] = 9.0
    p0[4, 0, 0] = -9.0

    def logp(X):
        return torch.where((X.abs() <= 1.0).all(-1), 0.0, NINF).to(torch.float64)

    with pytest.raises(ValueError, match="n = 8"):
        g.init_state_callback(p0, lambda X: torch.zeros(W * nt, dtype=torch.float64, device=X.device), logp)
    # ... on the zero-copy route too (every row inside the support)
    with pytest.raises(ValueError, match="n = 10"):
        g.init_state_callback(np.zeros(d), lambda X: torch.zeros(3, dtype=torch.float64, device=X.device), logp)
    seen = []
    g.init_state_callback(p0, lambda X: seen.append(X.shape[0]) or -0.5 * _columns(X, d), logp)
    assert seen == [8]
    # nothing inside the support: logl is not called at all; everything inside: it is handed the tensor itself
    g.init_state_callback(np.full((W, nt, d), 5.0), lambda X: 1 / 0, logp)
    assert np.isneginf(g.get("lnL")).all() and np.isneginf(g.get("lp")).all()
    ptrs = []
    g.init_state_callback(np.zeros(d), lambda X: ptrs.append(X.data_ptr()) or -0.5 * _columns(X, d), logp)
    assert ptrs == [g.t["X"].data_ptr()] and g.support_counts == (50, 8 + 10 + 8 + 0 + 10)
    # a flat prior: the stage launches nothing
    g.init_state_callback(p0, lambda X: -0.5 * _columns(X, d), None)
    assert g.support_counts == (50, 36) and getattr(g, "_sup_rows", None) is not None


# ------------------------------------------------------------------------------------------------------------- 4. composition
def test_the_stage_beside_custom_auxiliary_and_gradient_jumps(mods):
    from ptmcmcsampler_amd.engine import box_draw_jump
    orc, _lib, PTEngine = mods
    d, nt, W = 20, 3, 40
    rs = np.random.RandomState(5)
    lo, hi = -0.5 - 0.1 * rs.rand(d), 0.5 + 0.1 * rs.rand(d)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.05

    def make(on):
        def kick(X, it, beta):
            return X + 10.0, None                                     # always outside the box

        def nudge(X, Q, it, beta):
            Q += 0.001 * float((it % 3) - 1)
            return Q, None

        g = PTEngine.with_stages(d, nt, W, cov0, rows_logl=True, logp=("box", lo, hi), jumps=[(box_draw_jump(lo, hi), 2), (kick, 2)], aux=[nudge],
                                 grad_weights=(0, 5), jumps_with_grad=True, logl_in_support=on, hmc=(0.1, 2, 20),
                                 weights=(3, 2, 2), cov_update=20, burn=40, tskip=7, seed=23, am_mode="rows")
        g.init_state(p0)
        return g

    a, b = make(True), make(False)
    for n in (25, 3, 1, 46, 30):
        for g in (a, b):
            g.run(n)
            g.sync()
        for name in NAMES + ("cjstat", "gj"):
            if a.t.get(name) is not None:
                assert_same(a.get(name), b.get(name), "stage on vs off at iteration %d: %s" % (a.iter, name))
    cj = a.get("cjstat").astype(np.int64)                             # [W][nt][pick][proposed, accepted]
    assert cj[..., 2:, 0].sum() > 0 and cj[..., 2:, 1].sum() == 0     # kick: proposed, never accepted
    assert cj[..., :2, 1].sum() > 0                                   # the box draw lands inside
    assert a.get("jstat").astype(np.int64)[..., 4, 1].sum() > 0       # HMC accepted
    offered, given = a.support_counts
    assert offered == 106 * W * nt and cj[..., 2:, 0].sum() <= offered - given < offered and b.support_counts == (0, 0)


def test_graph_mode_falls_back_with_the_same_bits(mods):
    orc, _lib, PTEngine = mods
    d, nt, W = 37, 5, 3
    lo, hi, cov0, p0 = _box_case(d, nt, W, 0.4)
    runs = []
    for graph, on in ((True, True), (False, True), (True, False)):
        g = PTEngine.with_stages(d, nt, W, cov0, split=True, logl_in_support=on, logp=("box", lo, hi), weights=(20, 0, 20), cov_update=20, burn=40,
                                 tskip=7, seed=31)
        logl, logp = g.builtin_logl(), g.builtin_logp()
        g.init_state_callback(p0, logl, logp)
        for n in (25, 3, 1, 46, 30):
            g.run_callback(n, logl, logp, graph=graph)
        runs.append(_snapshot(g))
        assert bool(getattr(g, "_graphs", None)) == (graph and not on)     # with the stage no segment is captured
        assert (g.support_counts[1] > 0) == on
        if on:
            assert g.callback_segment_graph(g.iter + 1, g.iter + 1, logl, logp) is False
    _same(runs[0], runs[1], "stage on: graph=True vs graph=False")
    _same(runs[0], runs[2], "stage on vs stage off in graph mode")


# --------------------------------------------------------------------------------------------------------------- 5. the facade
def _same_files(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".txt"))
    assert "chain_1.0.txt" in names and "jumps.txt" in names and names == sorted(f for f in os.listdir(b) if f.endswith(".txt"))
    for f in names:
        assert open(os.path.join(a, f)).read() == open(os.path.join(b, f)).read(), f
    assert np.array_equal(np.load(os.path.join(a, "cov.npy")), np.load(os.path.join(b, "cov.npy")))
    assert len(open(os.path.join(a, "chain_1.0.txt")).readlines()) > 50


@pytest.mark.parametrize("kind", ["batched", "rows_logl"])
def test_the_sampler_passes_the_stage_on(tmp_path, kind):
    import torch
    from ptmcmcsampler_amd import PTSampler
    kw = dict(burn=40, thin=1, covUpdate=20, isave=100, Tskip=7, SCAMweight=4, AMweight=4, DEweight=4)
    common = dict(verbose=False, seed=4, ntemps=3, nwalkers=4, keep_walkers=4)
    if kind == "batched":
        d = 5
        args = (lambda X: -0.5 * _columns(X, d), lambda X: torch.where(((X >= -0.6) & (X <= 0.6)).all(-1), 0.0, NINF).to(torch.float64))
        cov, p0 = np.eye(d) * 0.05, np.full(d, 0.1)
        common["batched"] = True
    else:
        d = 120
        rs = np.random.RandomState(d)
        B = rs.randn(d, d)
        P = np.linalg.inv(B @ B.T / d + 0.5 * np.eye(d))
        hw = 0.12 + 0.05 * rs.rand(d)
        args = (("dense", rs.randn(d) * 0.01, (P + P.T) / 2.0), ("box", -hw, hw))
        cov, p0 = np.eye(d) * 0.01, np.zeros(d)
        common["rows_logl"] = True
    out = []
    for on in (False, True):
        # (a copy: the sampler adapts its cov argument in place)
        s = PTSampler(d, args[0], args[1], cov.copy(), outDir=str(tmp_path / ("on" if on else "off")), **common)
        if on:
            s.logl_in_support = True
        s.sample(p0, 100, **kw)
        out.append(s)
    off, on = out
    for name in ("X", "lnL", "lp", "slot_of", "nacc", "jstat", "nswap", "Ut"):
        assert_same(off.engine.get(name), on.engine.get(name), name)
    _same_files(str(tmp_path / "off"), str(tmp_path / "on"))
    assert off.engine.support_counts == (0, 0) and off.engine.logl_in_support is False and on.engine.logl_in_support is True
    offered, given = on.engine.support_counts
    assert offered == 101 * 12 and 0 < given < offered              # rows were skipped, and not all of them
    assert 0 < on.engine.get("nacc").sum() < 100 * 12
