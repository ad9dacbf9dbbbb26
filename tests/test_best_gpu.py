"""The best-fit (MAP / ML) row of every cold chain, tracked on the device (csrc/ptmi_best.hip; ``PTEngine.with_stages(best=True)``,
``PTSampler.track_best``): the held rows, values and iterations equal, bit for bit, the rule restated in NumPy (tests/test_best.py
``np_update``) on the ring as it was copied before each covariance epoch (tests/test_hist_gpu.py ``_ring`` / ``_expand``) -- driven through
the C ABI on crafted rings with guard words around every buffer (the maximum at the period's ends, inside and at the end of runs of
rows that were not stored, ties, signed zeros, NaN, infinities, every cut of a period into calls, every width and walker count at
which the kernel takes another path), through the engine in both ring modes and on every path, with two rings, ``best_sync``, a
checkpoint, the five ring readers together, and through the sampler against its chain files; and the stage only reads.

Run where there is a GPU: ``python -m pytest tests -m gpu``.  Nothing here reads the reference's tree."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from test_best import PAYLOAD, np_update, same_bits, same_state, seeded_aux
from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)
from test_hist_gpu import _cov0, _expand, _ring

pytestmark = pytest.mark.gpu

GUARD = 8                                                            # words before and behind every buffer
FILL = 7.0                                                           # what rows and val hold before anything is written


# ---------------------------------------------------------------------- the C ABI on buffers of the test's own
class _Abi(object):
    """rows [2][W][d], val [2][W][3] and iters [2][W] between guard words, attached to the handle of ``g`` (an engine without the stage)."""

    def __init__(self, g, beta0, attach=True):
        import torch
        self.g, self.beta0, W, d = g, beta0, g.W, g.d
        mk = lambda n, dt, v: torch.full((GUARD + n + GUARD,), v, dtype=dt, device=g.device)      # noqa: E731
        self.buf = dict(rows=mk(2 * W * d, torch.float64, -3.25), val=mk(2 * W * 3, torch.float64, -3.25), iters=mk(2 * W, torch.int64, -77))
        self.shape = dict(rows=(2, W, d), val=(2, W, 3), iters=(2, W))
        self.guard = {k: v[0].item() for k, v in self.buf.items()}
        self.reset()
        if attach:
            rc = g.lib.ptmi_best_attach(g.h, self.ptr("rows"), self.ptr("val"), self.ptr("iters"), beta0)
            assert rc == 0, g.lib.ptmi_last_error()

    def view(self, name):
        n = int(np.prod(self.shape[name]))
        return self.buf[name][GUARD:GUARD + n].view(self.shape[name])

    def ptr(self, name, off=0):
        return C.c_void_p(self.view(name).data_ptr() + off)

    def reset(self):
        self.view("rows").fill_(FILL)
        self.view("val").fill_(FILL)
        self.view("iters").fill_(-1)

    def update(self, lo, hi):
        return self.g.lib.ptmi_best_update(self.g.h, lo, hi)

    def state(self):
        """The buffers as they are (the guards checked)."""
        self.g.sync()
        for k, b in self.buf.items():
            n = int(np.prod(self.shape[k]))
            assert (b[:GUARD] == self.guard[k]).all().item() and (b[GUARD + n:] == self.guard[k]).all().item(), "guard words of " + k
        return {k: self.view(k).cpu().numpy().copy() for k in self.buf}


def _fresh(W, d):
    return dict(rows=np.full((2, W, d), FILL), val=np.full((2, W, 3), FILL), iters=np.full((2, W), -1, dtype=np.int64))


def _ref(g, st, beta0, base, klo, khi):
    """The rule on iterations base + klo .. base + khi of the ring as it stands, into ``st``."""
    am, fl = _ring(g)
    cu = g.cov_update
    x = _expand(am, fl, base, 1, khi)[:, klo - 1:]
    aux = g.t["AMaux"].cpu().numpy()
    ks = np.arange(klo, khi + 1)
    return np_update(st, aux[:, (base + ks) % cu], base + ks, beta0, x)


def _set_flags(g, _lib, stored):
    """``stored`` [W][cu + 1] by k = 1 .. cu (column 0 unused; 1 = stored) -> the ring's flag words, NEW and KEY alternating; ring row 1 is KEY."""
    import torch
    W, cu = g.W, g.cov_update
    word = np.zeros((W, cu), dtype=np.int64)
    for k in range(1, cu + 1):
        word[:, k % cu] = np.where(stored[:, k] != 0, _lib.AMROW_NEW if k % 3 else _lib.AMROW_KEY, 0)
    word[:, 1] = _lib.AMROW_KEY
    g.t["AMflag"].copy_(torch.from_numpy(word).to(g.device))


CU, W5, D3 = 200, 5, 3
# runs of rows that were not stored, by walker (first, last): lengths 1, 63, 64, 65 / 130 / 130 hanging on ring row 1 / none / the first again
RUNS = [[(3, 3), (5, 67), (69, 132), (134, 198)], [(3, 132)], [(2, 131)], [], [(3, 3), (5, 67), (69, 132), (134, 198)]]


def _stored():
    lay = np.ones((W5, CU + 1), dtype=np.int64)
    for row, rr in zip(lay, RUNS):
        for a, b in rr:
            assert b - a + 1 in (1, 63, 64, 65, 130)
            row[a:b + 1] = 0
    return lay


def _low(rs):
    """lnL and lp nobody picks: all below -5."""
    return -5.0 - 5.0 * rs.rand(W5, CU, 2)


@pytest.mark.parametrize("flags", [True, False])
def test_crafted_ring_through_the_c_abi(mods, flags):
    orc, _lib, PTEngine = mods
    beta0 = 1.0 / 1.7
    g = PTEngine(D3, 1, W5, np.eye(D3), cov_update=CU, tskip=0, keep_lnl=True, **(dict(cov_mode="pooled") if flags else {}))
    assert (g.t["AMflag"] is not None) == flags and g.am_pos is None and g.t["AMaux"] is not None
    rs = np.random.RandomState(12)
    ring = rs.randn(W5, CU, D3)
    ring[:, 1] = [np.nan, -0.0, PAYLOAD]                             # the row the long run hangs on: the words arrive as they were
    ring[:, 0] = [np.inf, -np.inf, 0.0]
    g.put("AM", ring)
    if flags:
        _set_flags(g, _lib, _stored())
    abi = _Abi(g, beta0)
    row = lambda k: k % CU      # noqa: E731

    def run(aux, calls, what, st=None, reset=True):
        """``aux`` onto the device, the calls (lo, hi) one after the other, the buffers against the rule."""
        g.put("AMaux", aux)
        if reset:
            abi.reset()
        st = _fresh(W5, D3) if st is None else st
        for lo, hi in calls:
            assert abi.update(lo, hi) == 0, g.lib.ptmi_last_error()
            _ref(g, st, beta0, 0, lo, hi)
        got = abi.state()
        same_state(got, st, what)
        return got

    whole = [(1, CU)]
    # the position of the maximum: the period's first and last iteration (ring row 0), inside and at the end of every run, behind it
    spots = {1, CU}
    for rr in RUNS:
        for a, b in rr:
            spots |= {a, (a + b) // 2, b, b + 1}
    for k in sorted(spots):
        aux = _low(rs)
        aux[:, row(k)] = [5.0, 0.25]
        got = run(aux, whole, "maximum at k = %d" % k)
        assert (got["iters"] == k).all()
        if flags and k == 131:                                       # walker 2's run 2 .. 131: ring row 1 through three steps of the walk back
            same_bits(got["rows"][:, 2], np.stack([ring[2, 1]] * 2), "the long run")
    assert {1, 2, 3, 4, 36, 67, 68, 100, 131, 132, 133, 166, 198, 199, CU} <= spots
    # two equal maxima in one call: the earlier wins
    aux = _low(rs)
    aux[:, row(50)] = aux[:, row(120)] = [5.0, 0.25]
    assert (run(aux, whole, "two maxima")["iters"] == 50).all()
    # a later call whose maximum equals the held one: the held one stays
    aux = _low(rs)
    aux[:, row(40)] = aux[:, row(150)] = [5.0, 0.25]
    assert (run(aux, [(1, 100), (101, CU)], "an equal maximum later")["iters"] == 40).all()
    # 0.0 held against -0.0 coming, and the other way round
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        aux = _low(rs)
        aux[:, row(40)], aux[:, row(150)] = [first, first], [second, second]
        got = run(aux, [(1, 100), (101, CU)], "signed zeros %r" % first)
        assert (got["iters"] == 40).all() and (np.signbit(got["val"][1, :, 0]) == np.signbit(first)).all()
    # a NaN with a payload at the would-be maximum of one plane only: lp, so the MAP score is NaN and ML carries the payload
    aux = _low(rs)
    aux[:, row(70)] = [9.0, PAYLOAD]
    aux[:, row(90)] = [5.0, 0.25]
    got = run(aux, whole, "NaN in lp")
    assert (got["iters"][0] == 90).all() and (got["iters"][1] == 70).all()
    same_bits(got["val"][1, :, 2], np.full(W5, PAYLOAD), "the payload")
    # ... and lnL: ML passes over it too
    aux = _low(rs)
    aux[:, row(70)] = [PAYLOAD, 100.0]
    aux[:, row(90)] = [5.0, 0.25]
    assert (run(aux, whole, "NaN in lnL")["iters"] == 90).all()
    # +inf in lnL with -inf in lp: NaN for MAP, a winner for ML
    aux = _low(rs)
    aux[:, row(80)] = [np.inf, -np.inf]
    aux[:, row(90)] = [5.0, 0.25]
    got = run(aux, whole, "inf - inf")
    assert (got["iters"][0] == 90).all() and (got["iters"][1] == 80).all() and (got["val"][1, :, 0] == np.inf).all()
    # a first candidate of -inf wins against nothing and loses to the next finite one; alone, it stays
    aux = _low(rs)
    aux[:, row(1)] = [-np.inf, 0.0]
    assert (run(aux, [(1, 1)], "-inf alone")["iters"] == 1).all()
    assert (run(aux, [(1, 1), (2, 2)], "-inf, then a finite one")["iters"] == 2).all()
    # a walker whose every score is NaN: its iters stay -1, its rows and val untouched
    aux = _low(rs)
    aux[3] = np.nan
    aux[3, ::2, 0] = PAYLOAD
    got = run(aux, whole, "a walker of NaN")
    assert (got["iters"][:, 3] == -1).all() and (got["rows"][:, 3] == FILL).all() and (got["val"][:, 3] == FILL).all()
    assert (np.delete(got["iters"], 3, axis=1) >= 1).all()
    # lp crafted so that MAP and ML pick different iterations
    aux = _low(rs)
    aux[:, row(30)] = [8.0, -40.0]
    aux[:, row(160)] = [6.0, 1.0]
    got = run(aux, whole, "MAP and ML apart")
    assert (got["iters"][0] == 160).all() and (got["iters"][1] == 30).all()
    same_bits(got["val"][0, :, 0], np.full(W5, beta0 * 6.0 + 1.0))
    # seeded random lnL / lp under beta0 = 1 / 1.7, one iteration a call from nothing: a contracted multiply-add would show in the score
    aux = rs.randn(W5, CU, 2) * np.array([300.0, 3.0])
    g.put("AMaux", aux)
    differ = 0
    for k in range(1, 41):
        abi.reset()
        assert abi.update(k, k) == 0
        got = abi.state()
        want = beta0 * aux[:, row(k), 0] + aux[:, row(k), 1]
        same_bits(got["val"][0, :, 0], want, "score of k = %d" % k)
        same_bits(got["val"][0, :, 1:], aux[:, row(k)], "lnL, lp of k = %d" % k)
        assert (got["iters"] == k).all()
        fused = np.array([float(Fraction(beta0) * Fraction(float(a)) + Fraction(float(b))) for a, b in aux[:, row(k)]])      # one rounding
        differ += int((fused != want).sum())
    assert differ > 0, "no candidate at which a fused multiply-add rounds another way: the case shows nothing"
    # one period in one call, and in calls of 1, 63, 64, 65 and the rest: the same state (ties, NaN and infinities sprinkled in)
    aux = seeded_aux(rs, W5, CU)
    one = run(aux, whole, "one call")
    cut = run(aux, [(1, 1), (2, 64), (65, 128), (129, 193), (194, CU)], "five calls")
    same_state(cut, one, "however the period is cut")


@pytest.mark.parametrize("d,W,pooled", [(1, 1, False), (2, 3, True), (63, 4, False), (64, 5, True), (65, 3, False), (100, 5, True), (300, 4, True),
                                        (3, 261, True)])
def test_widths_and_walker_counts(mods, d, W, pooled):
    orc, _lib, PTEngine = mods
    cu, beta0 = 70, 0.5
    g = PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0, keep_lnl=True, **(dict(cov_mode="pooled") if pooled else {}))
    assert (g.am_pos is not None) == (d == 100) and (g.t["AMflag"] is not None) == pooled
    rs = np.random.RandomState(1000 + d + W)
    g.put("AM", rs.randn(W, cu, d))
    if pooled:
        stored = (rs.rand(W, cu + 1) < 0.3).astype(np.int64)
        stored[:, 1] = 1
        _set_flags(g, _lib, stored)
    g.put("AMaux", np.round(rs.randn(W, cu, 2) * 4.0) / 4.0)
    abi = _Abi(g, beta0)
    st = _fresh(W, d)
    for base, lo, hi in ((0, 1, 37), (0, 38, cu), (cu, 1, 3)):       # the third call: the next period reads the same ring again
        assert abi.update(base + lo, base + hi) == 0, g.lib.ptmi_last_error()
        _ref(g, st, beta0, base, lo, hi)
        same_state(abi.state(), st, "d = %d, W = %d, %d..%d" % (d, W, base + lo, base + hi))
    assert (st["iters"] >= 1).all()


def test_c_abi_refusals_and_a_hot_block(mods, monkeypatch):
    import torch
    orc, _lib, PTEngine = mods
    d, W, cu = 5, 2, 8
    bare = PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0)      # no AMaux
    L = bare.lib
    err = lambda: L.ptmi_last_error().decode()      # noqa: E731
    assert L.ptmi_best_update(bare.h, 1, 2) == -1 and "ptmi_best_attach" in err()      # PTMI_EINVAL: update before attach
    a = _Abi(bare, 1.0, attach=False)
    assert L.ptmi_best_attach(bare.h, a.ptr("rows"), a.ptr("val"), a.ptr("iters"), 1.0) == -1 and "AMaux" in err()
    assert L.ptmi_best_attach(None, a.ptr("rows"), a.ptr("val"), a.ptr("iters"), 1.0) == -1 and "NULL handle" in err()
    assert L.ptmi_best_update(None, 1, 2) == -1 and "NULL handle" in err()
    g = PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0, keep_lnl=True)
    a = _Abi(g, 1.0, attach=False)
    full = lambda **kw: [kw.get(n, a.ptr(n)) for n in ("rows", "val", "iters")]      # noqa: E731
    for name in ("rows", "val", "iters"):
        assert L.ptmi_best_attach(g.h, *full(**{name: None}), 1.0) == -1 and name in err() and "non-NULL" in err()
        assert L.ptmi_best_attach(g.h, *full(**{name: a.ptr(name, 4)}), 1.0) == -1 and name in err() and "aligned" in err()
    for bad in (0.0, -1.0, np.inf, -np.inf, np.nan):
        assert L.ptmi_best_attach(g.h, *full(), bad) == -1 and "beta0" in err(), bad
    assert L.ptmi_best_update(g.h, 1, 2) == -1 and "ptmi_best_attach" in err()      # none of them attached anything
    _lib.check(L.ptmi_best_attach(g.h, *full(), 1.0))
    assert L.ptmi_best_attach(g.h, *full(), 1.0) == -1 and "already attached" in err()
    for lo, hi in ((cu, cu + 1), (1, cu + 1), (cu - 2, 2 * cu), (0, 3), (-2, 1), (0, 0)):
        assert L.ptmi_best_update(g.h, lo, hi) == -1 and "period" in err() and "ptmi_best_update" in err(), (lo, hi)
    for lo, hi in ((5, 4), (1, 0), (cu + 1, cu)):
        assert L.ptmi_best_update(g.h, lo, hi) == 0                  # an empty range: nothing to do
    st = a.state()
    same_state(st, _fresh(W, d), "refused and empty calls launched nothing")
    # the calls that are taken: the period's last iteration sits in ring row 0, the next period's first in ring row 1
    ring, aux = np.random.RandomState(0).randn(W, cu, d), np.random.RandomState(1).randn(W, cu, 2)
    g.put("AM", ring)
    g.put("AMaux", aux)
    want = _fresh(W, d)
    for base, lo, hi in ((0, cu, cu), (cu, 1, 1), (cu, 2, cu)):
        assert L.ptmi_best_update(g.h, base + lo, base + hi) == 0, err()
        _ref(g, want, 1.0, base, lo, hi)
        same_state(a.state(), want, "%d..%d" % (base + lo, base + hi))
    # a hot block: PTMI_OK, not even the range is looked at, every buffer untouched.  (The engine gives a block without rank 0 no
    # AMaux; the handle gets one here so that the attach is taken)
    spare = torch.zeros(W * cu * 2, dtype=torch.float64, device=g.device)
    real = _lib.Buffers

    def with_aux(**kw):
        if kw.get("AMaux") is None:
            kw["AMaux"] = C.c_void_p(spare.data_ptr())
        return real(**kw)

    monkeypatch.setattr(_lib, "Buffers", with_aux)
    hot = PTEngine(d, 2, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=2, ntemps_global=4, temp0=2, keep_lnl=True)
    monkeypatch.undo()
    assert not hot.owns_cold and hot.t["AM"] is None
    b = _Abi(hot, 1.0)
    hot.init_state(np.zeros((W, 2, d)))
    hot.run(cu + 3)
    for lo, hi in ((1, cu), (cu + 1, cu + 3), (1, 3 * cu)):
        assert L.ptmi_best_update(hot.h, lo, hi) == 0
    same_state(b.state(), _fresh(W, d), "a hot block")


# ---------------------------------------------------------------------- every way of running the engine
def _drive(g, advance, periods, extra=0, st=None):
    """``periods`` whole covariance periods from where the engine stands and ``extra`` iterations of the next one; the rule applied to
    the ring copied at each period's end (the next iteration's epoch takes it: update_cov).  Returns the reference state and the
    number of rows that were not stored."""
    cu, beta0 = g.cov_update, 1.0 / g.temps_mh[0]
    st = _fresh(g.W, g.d) if st is None else st
    first, unstored = g.best_from, 0
    for n in [cu] * periods + ([extra] if extra else []):
        base = g.iter
        assert base % cu == 0
        advance(n)
        lo = max(1, first + 1 - base)
        if lo <= n:
            _ref(g, st, beta0, base, lo, n)
        fl = _ring(g)[1]
        if fl is not None:
            unstored += int((fl[:, np.arange(base + 1, base + n + 1) % cu] == 0).sum())
    return st, unstored


def _check(g, st, what=""):
    """``best_device()`` against the reference state and ``best()`` against the arg-max over it."""
    rows, val, iters = g.best_device()
    assert rows.is_cuda and rows.data_ptr() == g.t["best"].data_ptr() and iters.dtype.is_floating_point is False
    got = dict(rows=rows.cpu().numpy(), val=val.cpu().numpy(), iters=iters.cpu().numpy())
    held = st["iters"] >= 0
    want = {k: np.where(held.reshape(held.shape + (1,) * (v.ndim - 2)), v, 0) for k, v in st.items() if k != "iters"}
    want["iters"] = st["iters"]                                      # (the engine's buffers start as zeros, the reference's as FILL)
    same_state(got, want, what)
    b = g.best(per_walker=True)
    assert b["first_iter"] == g.best_from + 1 and b["last_iter"] == g.iter == g.best_iter and b["nwalkers"] == g.W
    for p, tag in ((0, "map"), (1, "ml")):
        sc = np.where(held[p], st["val"][p, :, 0], -np.inf)
        w = int(np.argmax(sc)) if held[p].any() else -1              # the first of the largest
        assert b["walker_" + tag] == w and b["iter_" + tag] == (st["iters"][p, w] if w >= 0 else -1), (what, tag)
        if w >= 0:
            same_bits(b["x_" + tag], st["rows"][p, w], what + " x_" + tag)
            same_bits(b["lnlike_" + tag], st["val"][p, w, 1])
            same_bits(b["lp_" + tag], st["val"][p, w, 2])
            same_bits(b["lnprob_" + tag], (1.0 / g.temps_mh[0]) * st["val"][p, w, 1] + st["val"][p, w, 2])
    same_bits(b["x"], got["rows"])
    same_bits(b["val"], got["val"])
    assert np.array_equal(b["iters"], got["iters"])
    return b


def test_both_ring_modes_every_path_and_two_rings(mods):
    orc, _lib, PTEngine = mods
    d, W, cu, n = 12, 6, 16, 5 * 16 + 3
    rs = np.random.RandomState(2)
    box = ("box", -0.25 - rs.rand(d) * 0.1, 0.2 + rs.rand(d) * 0.1)  # tight: long runs of rejected steps
    p0 = rs.uniform(-0.05, 0.05, (W, 2, d))
    kw = dict(weights=(20, 20, 0), cov_update=cu, burn=1000, tskip=5, seed=8, cov_mode="pooled", keep_lnl=True, logp=box)

    def pair(**more):
        spec = dict(best=True)
        a, b = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.05, **kw, **more, **spec), PTEngine(d, 2, W, np.eye(d) * 0.05, **kw, **more)
        for g in (a, b):
            if more.get("split"):
                logl = g.builtin_logl()
                g.init_state_callback(p0, logl, None)
                adv = lambda m, g=g, logl=logl: g.run_callback(m, logl, None)      # noqa: E731
            else:
                g.init_state(p0)
                adv = g.run
            if g is a:
                st, unstored = _drive(g, adv, 5, extra=3)
            else:
                adv(n)
        assert a.best_from == 0 and a.best_iter == 5 * cu          # from the first iteration on, not from burn
        for name in ("X", "lnL", "lp", "nacc", "jstat", "nswap", "cov", "mu", "M2", "AM", "AMaux"):      # the stage only reads
            assert_same(a.get(name), b.get(name), "%r %s" % (more, name))
        assert "best" not in b.t and "best_iter" not in b.checkpoint() and not b.best_on
        return _check(a, st, repr(more)), st, unstored

    (rle, st_rle, un_rle), (rows, st_rows, un_rows) = pair(am_mode="rle"), pair(am_mode="rows")
    assert un_rle > 0 and un_rows == 0, "the tight prior must leave rows that were not stored"
    for st, b in ((st_rle, rle), (st_rows, rows)):
        assert (st["iters"] >= 1).all() and b["iter_map"] >= 1 and b["walker_ml"] >= 0
    lag, two = pair(am_mode="rle", eig_lag=1)[1], pair(am_mode="rle", stats_async=True, eig_lag=1)[1]
    same_state(two, lag, "two rings: a scheduling change only")
    for more in (dict(rows_logl=True), dict(split=True)):           # the row and the callback path (the fused one: above)
        assert pair(am_mode="rle", **more)[0]["iter_ml"] >= 1


def test_best_sync_inside_a_period_and_the_readers_refusals(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 8, 3, 20
    kw = dict(weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=3, cov_mode="pooled", keep_lnl=True,
              logp=("box", -0.3 * np.ones(d), 0.3 * np.ones(d)), best=True)
    p0 = np.zeros((W, 1, d))
    a, b = (PTEngine.with_stages(d, 1, W, np.eye(d) * 0.05, **kw) for _ in range(2))
    for g in (a, b):
        g.init_state(p0)
        g.run(2 * cu)                                                # iteration 21 took the first period
    a.best_sync(cu + 9)
    assert a.best_iter == cu + 9 and b.best_iter == cu and a.best_from == b.best_from == 0
    mid = a.best(it=cu + 9)
    assert mid["last_iter"] == cu + 9 and 1 <= mid["iter_map"] <= cu + 9
    a.best_sync(cu + 9)                                              # again: nothing to take
    a.best_sync(2 * cu)
    for g in (a, b):
        g.run(1)
    assert a.best_iter == b.best_iter == 2 * cu
    sa, sb = a.best(per_walker=True), b.best(per_walker=True)
    assert sa["last_iter"] == sb["last_iter"] == 2 * cu + 1
    for k in sa:
        assert_same(sa[k], sb[k], "middle + rest = the whole period: " + k)
    with pytest.raises(ValueError, match=r"best_sync\(42\): the engine has reached iteration 41"):
        a.best_sync(a.iter + 1)
    f = PTEngine.with_stages(d, 1, W, np.eye(d) * 0.05, **kw)
    f.iter = cu + 1                                                  # stepped from outside, past an epoch that never went through update_cov
    with pytest.raises(ValueError, match=r"best_sync\(21\): iterations 1..20 are no longer in the ring"):
        f.best_sync(cu + 1)
    assert f.best_iter == 0 and (f.t["best_iters"] == -1).all().item()
    none = f.best(it=0)                                              # nothing held yet: -1 and NaN, never an error
    assert none["iter_map"] == none["iter_ml"] == none["walker_map"] == -1 and np.isnan(none["lnprob_map"]) and np.isnan(none["x_ml"]).all()
    with pytest.raises(ValueError, match=r"no best-fit tracker: PTEngine.with_stages\(..., best=True\)"):
        PTEngine(d, 1, W, np.eye(d), cov_update=cu, tskip=0).best()
    # an engine that owns no cold ring: idle
    hot = PTEngine.with_stages(d, 2, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=1000, tskip=0, seed=2, ntemps_global=4,
                               temp0=2, keep_lnl=True, best=True)
    hot.init_state(np.zeros((W, 2, d)))
    hot.run(cu + 3)
    out = hot.best()
    assert out["iter_map"] == -1 and out["walker_ml"] == -1 and (hot.t["best_iters"] == -1).all().item() and not hot.t["best"].any().item()


def test_checkpoint_inside_a_period_and_its_refusals(mods):
    orc, _lib, PTEngine = mods
    d, W, cu = 10, 4, 20
    kw = dict(weights=(20, 20, 20), cov_update=cu, burn=40, tskip=10, seed=6, cov_mode="pooled", keep_lnl=True)
    spec = dict(best=True, best_from=3)
    p0 = np.random.RandomState(3).randn(W, 2, d) * 0.1
    a, u = (PTEngine.with_stages(d, 2, W, _cov0(d), **kw, **spec) for _ in range(2))
    for g in (a, u):
        g.init_state(p0)
    a.run(cu + 10)
    a.best_sync(cu + 6)                                              # the checkpoint falls inside a period, with part of it taken
    st = a.checkpoint()
    assert st["best_iter"] == cu + 6 and st["best_from"] == 3 and st["t_best"].shape == (2, W, d) and st["t_best_val"].shape == (2, W, 3)
    assert st["t_best_iters"].shape == (2, W) and st["t_best_iters"].dtype == np.int64 and (st["t_best_iters"] > 3).all()
    b = PTEngine.with_stages(d, 2, W, _cov0(d), **kw, **spec)
    b.restore(st)
    assert b.best_iter == cu + 6 and b.iter == cu + 10
    for g in (a, b):
        g.run(2 * cu + 5)
    u.run(3 * cu + 15)                                               # the uninterrupted run
    sa, sb, su = a.best(per_walker=True), b.best(per_walker=True), u.best(per_walker=True)
    for k in sa:
        assert_same(sa[k], sb[k], "restored: " + k)
        assert_same(sa[k], su[k], "uninterrupted: " + k)
    assert_same(a.get("X"), b.get("X"), "X")
    # a checkpoint without the stage, or with another best_from, is refused before anything is touched
    c = PTEngine(d, 2, W, _cov0(d), **kw)
    c.init_state(p0)
    c.run(cu + 10)
    for bad, other in ((c.checkpoint(), spec), (st, dict(best=True)), (st, dict(best=True, best_from=4))):
        e = PTEngine.with_stages(d, 2, W, _cov0(d), **kw, **other)
        e.init_state(p0)
        x0 = e.get("X")
        with pytest.raises(ValueError, match="the checkpoint carries no best-fit rows of this shape"):
            e.restore(bad)
        assert e.iter == 0 and e.best_iter == e.best_from and (e.t["best_iters"] == -1).all().item()
        assert_same(e.get("X"), x0, "nothing was touched")


def test_five_readers_on_one_engine_equal_five_engines_with_one_each(mods):
    orc, _lib, PTEngine = mods
    D, W, CU = 5, 6, 16
    stages = {"hist": dict(hist=(-0.6, 0.6, 8), hist_from=0), "pairs": dict(pairs=({"params": [0, 2, 4]}, -0.6, 0.6, 8), pairs_from=CU),
              "diag": dict(diag=True, diag_from=5, diag_levels=4), "samples": dict(samples={"slots": 4, "every": 3}, samples_from=2),
              "best": dict(best=True, best_from=7)}
    kw = dict(weights=(20, 20, 20), cov_update=CU, burn=CU, tskip=5, seed=11, cov_mode="pooled", am_mode="rle", keep_lnl=True)
    p0 = np.random.RandomState(3).randn(W, 2, D) * 0.1
    results = {"hist": lambda g, it: g.hist_counts(it), "pairs": lambda g, it: g.pairs_counts(it), "diag": lambda g, it: g.diag_moments(it),
               "samples": lambda g, it: g.samples(it), "best": lambda g, it: g.best(it, per_walker=True)}

    def make(**st):
        g = PTEngine.with_stages(D, 2, W, _cov0(D), **st, **kw)
        g.init_state(p0)
        return g

    a = make(**{k: v for s in stages.values() for k, v in s.items()})
    assert [r.name for r in a._ring] == ["hist", "pairs", "diag", "samples", "best"]
    one = {name: make(**s) for name, s in stages.items()}
    end = 3 * CU + 5
    for g in [a] + list(one.values()):
        g.run(end)
    assert all(r.iter == 3 * CU for r in a._ring)
    for name, g in one.items():
        got, alone = results[name](a, end), results[name](g, end)
        assert sorted(got) == sorted(alone), name
        for k in alone:
            assert_same(got[k], alone[k], "%s beside the others: %s" % (name, k))
        assert_same(g.get("X"), a.get("X"), "X of the engine with " + name)      # the stages only read
    assert all(r.iter == end for r in a._ring)


# ---------------------------------------------------------------------- the sampler
def _sampler(out, W, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 6
    s = PTSampler(d, ("iso",), ("box", -3.0 * np.ones(d), 3.0 * np.ones(d)), np.eye(d) * 0.5, outDir=str(out), verbose=False, seed=21, ntemps=2,
                  nwalkers=W, keep_walkers=W, **kw)
    s.track_best = True
    return s


def test_sampler_best_equals_the_arg_max_over_the_chain_files_and_resume(tmp_path):
    W, N, d = 16, 400, 6
    run = dict(burn=100, thin=1, covUpdate=50, isave=50, Tskip=10)   # chain files are thinned: thin = 1 keeps every iteration
    p0 = np.zeros(d)
    a = _sampler(tmp_path / "a", W, checkpoint=True)
    a.sample(p0, N, **run)
    s = a.best
    assert s["first_iter"] == 1 and s["last_iter"] == N and s["nwalkers"] == W and a.engine.best_from == 0
    assert s["x"].shape == (2, W, d) and s["val"].shape == (2, W, 3) and s["iters"].shape == (2, W) and (s["iters"] >= 1).all()
    beta0 = 1.0 / a.engine.temps_mh[0]
    same_bits(s["val"][0, :, 0], beta0 * s["val"][0, :, 1] + s["val"][0, :, 2], "the MAP score is lnprob")
    same_bits(s["val"][1, :, 0], s["val"][1, :, 1], "the ML score is lnlike")
    for p, held in ((0, a._lnprobs), (1, a._lnlikes)):               # the harvested chains: another path out of the ring (_harvest)
        for w in range(W):
            it = 1 + int(np.argmax(held[w, 1:N + 1]))                # the first of the largest; iteration 0 (p0) is not a candidate
            assert s["iters"][p, w] == it, (p, w)
            same_bits(s["val"][p, w, 0], held[w, it], "score of walker %d" % w)
            same_bits(s["val"][p, w, 1], a._lnlikes[w, it], "lnlike of walker %d" % w)
            same_bits(s["x"][p, w], a._chains[w, it], "row of walker %d" % w)
    # ... and the chain files themselves: values at the precision the text keeps, rows through the iteration
    for w in range(W):
        f = np.loadtxt(a.fname if w == 0 else a.fname[:-4] + "_w%d.txt" % w)
        assert f.shape == (N + 1, d + 4)
        for p, col in ((0, -4), (1, -3)):
            assert "%f" % f[1:, col].max() == "%f" % s["val"][p, w, 0], (w, p)
            assert abs(f[s["iters"][p, w], col] - s["val"][p, w, 0]) <= 0.5000001e-6
            assert np.abs(f[s["iters"][p, w], :d] - s["x"][p, w]).max() <= 1e-15
    wm, wl = int(np.argmax(s["val"][0, :, 0])), int(np.argmax(s["val"][1, :, 0]))
    assert s["walker_map"] == wm and s["iter_map"] == s["iters"][0, wm] and s["walker_ml"] == wl and s["iter_ml"] == s["iters"][1, wl]
    same_bits(s["x_map"], s["x"][0, wm])
    same_bits(s["x_ml"], s["x"][1, wl])
    assert s["lnprob_map"] == a._lnprobs[:, 1:N + 1].max() and s["lnlike_ml"] == a._lnlikes[:, 1:N + 1].max()
    f = np.load(tmp_path / "a" / "best.npz")
    assert sorted(f.files) == sorted(["x_map", "lnprob_map", "lnlike_map", "lp_map", "iter_map", "walker_map", "x_ml", "lnlike_ml", "lp_ml",
                                      "lnprob_ml", "iter_ml", "walker_ml", "first_iter", "last_iter", "nwalkers", "x", "val", "iters"])
    for k in f.files:
        assert_same(f[k], s[k], k)
    # stopped at 200 and resumed from its checkpoint: the file of the uninterrupted run
    b1 = _sampler(tmp_path / "b", W, checkpoint=True)
    b1.sample(p0, 200, **run)
    assert b1.best["last_iter"] == 200 and (b1.best["iters"] <= 200).all() and os.path.exists(tmp_path / "b" / "best.npz")
    b2 = _sampler(tmp_path / "b", W, checkpoint=True, resume=True)
    b2.sample(p0, N, **run)
    assert np.array_equal(a._chains, b2._chains)
    fb = np.load(tmp_path / "b" / "best.npz")
    assert sorted(fb.files) == sorted(f.files)
    for k in f.files:
        assert_same(fb[k], f[k], "resumed " + k)
    # chain files alone cannot continue the comparison
    c1 = _sampler(tmp_path / "c", W, checkpoint=False)
    c1.sample(p0, 50, **run)
    c2 = _sampler(tmp_path / "c", W, checkpoint=False, resume=True)
    with pytest.raises(NotImplementedError, match="track_best.*checkpoint=True"):
        c2.sample(p0, 100, **run)
    # {"from": k} reaches the engine; a run without the attribute writes no file and has no best
    from ptmcmcsampler_amd import PTSampler
    e = _sampler(tmp_path / "e", 4)
    e.track_best = {"from": 30}
    e.sample(p0, 100, **run)
    assert e.engine.best_from == 30 and e.best["first_iter"] == 31 and (e.best["iters"] > 30).all()
    n = PTSampler(d, ("iso",), ("flat",), np.eye(d) * 0.5, outDir=str(tmp_path / "n"), verbose=False, seed=21)
    n.sample(p0, 100, burn=50, thin=1, covUpdate=50, isave=50)
    assert n.best is None and not (tmp_path / "n" / "best.npz").exists() and not n.engine.best_on
