"""The temperature ladder adapted on the device (csrc/ptmi_ladder.hip; ``PTEngine.with_stages(adapt_ladder=...)``, ``PTSampler.adapt_ladder``):
the planes, ``seen`` and the handle's tables equal the NumPy restatement of the rule (tests/test_ladder_adapt.py ``ladder_rule``) bit for
bit -- crafted counters at shapes that reach every edge of the reduction, consecutive updates, the hot rank, the evidence stage's gaps --
``ptmi_ladder_publish`` installs a ladder a run then tempers with, a driven run on real chains follows the rule update by update, freezes
after ``until`` and equalises the pairs' acceptance, every path of the engine gives the same chains and planes, checkpoints resume to the
bit, the C ABI refuses what it must, and the sampler writes what it holds.

Run with ``python -m pytest tests -m gpu``.  Nothing here reads the reference."""
import ctypes as C

import numpy as np
import pytest

from test_evidence import ev_rule
from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)
from test_ladder_adapt import LADDER0, ladder_rule, model_worst_gap_deviation, planes_of

pytestmark = pytest.mark.gpu

CHAINS = ("X", "lnL", "lp", "slot_of", "temp_of", "nacc", "nswap")


def _own_stage(g, _lib, ladder, seen0=None, pad=64):
    """Caller-owned buffers attached through the C ABI, with ``pad`` words behind each that no call may touch."""
    import torch
    n = g.ntg
    gaps, T, seen = planes_of(ladder)
    if seen0 is not None:
        seen = np.asarray(seen0, dtype=np.uint64)
    host = np.zeros(3 * n + pad)
    host[:n], host[2 * n:3 * n] = gaps, T
    lad = torch.from_numpy(host).to(g.device)
    sn = torch.from_numpy(np.concatenate([seen, np.zeros(pad, dtype=np.uint64)]).view(np.int64)).to(g.device)
    _lib.check(g.lib.ptmi_ladder_attach(g.h, C.c_void_p(lad.data_ptr()), C.c_void_p(sn.data_ptr())))

    def read():
        g.sync()
        a, s = lad.cpu().numpy(), sn.cpu().numpy().view(np.uint64)
        assert not a[3 * n:].any() and not s[n:].any(), "a call wrote behind its planes"
        return a[:3 * n].reshape(3, n), s[:n]

    return read, lad, sn


def _tables(g, _lib):
    lad, tm, be = np.empty(g.ntg), np.empty(g.nt), np.empty(g.nt)
    _lib.check(g.lib.ptmi_ladder_read(g.h, lad.ctypes.data_as(_lib._dp), tm.ctypes.data_as(_lib._dp), be.ctypes.data_as(_lib._dp)))
    return lad, tm, be


def _some_ladder(rs, n):
    return np.cumprod(np.concatenate([[1.0], 1.0 + rs.rand(n - 1) * 1.5]))


# W x n: one row of ranks short of a wave; no multiple of 64 in either extent; more than one slab and 231 of a block's 256 threads at
# work; one interior rank; none
@pytest.mark.parametrize("W,n,hot,ev", [(3, 5, False, False), (70, 7, True, False), (300, 33, False, True), (5, 3, True, True),
                                        (4, 2, False, False)])
def test_crafted_counters(mods, W, n, hot, ev):
    orc, _lib, PTEngine = mods
    from ptmcmcsampler_amd.evidence import dbeta_of
    rs = np.random.RandomState(100 * W + n)
    d = 2
    ladder = _some_ladder(rs, n)
    make = PTEngine.with_stages if ev else PTEngine
    g = make(d, n, W, np.eye(d), ladder=ladder, tskip=10, hot_chain=hot, **(dict(evidence=True, evidence_from=0) if ev else {}))
    # cumulative counts beyond 2^53 (odd: no double holds them) that earlier windows have consumed: as a restored run stands
    ns = rs.randint(0, 1000, size=(W, n)).astype(np.uint64)
    ns[0, :] += np.uint64(2 ** 53 + 1)
    ns[W - 1, :] += np.uint64(2 ** 60)
    g.put("nswap", ns.view(np.int64))
    seen0 = ns.sum(0, dtype=np.uint64)
    seen0[-1] = 0                                                        # (column n - 1 is no pair: nothing reads or writes its entry)
    assert (seen0[:-1] > 2 ** 53).all() and (seen0[:-1] % 2 == 1).any()
    read, _, _ = _own_stage(g, _lib, ladder, seen0)
    gaps, T, seen = planes_of(ladder)
    seen = seen0.copy()
    lad0, tm0, be0 = _tables(g, _lib)
    assert_same(lad0, ladder, "tables before any update")
    assert_same(be0, 1.0 / tm0)
    for call, (kappa, te, to) in enumerate(((8.0, 3, 2), (1.25, 1, 4), (0.3, 5, 7))):      # tries_even != tries_odd, three gains
        tries = np.where(np.arange(n) % 2, to, te)
        inc = (rs.rand(W, n) * (tries + 1)).astype(np.uint64)             # 0 .. tries accepted swaps of a walker and pair in the window
        inc[:, 0] = te                                                    # pair 0 accepted every try: A = 1
        if n > 2:
            inc[:, 1] = 0                                                 # pair 1 none: A = 0
        ns = ns + inc
        g.put("nswap", ns.view(np.int64))
        _lib.check(g.lib.ptmi_ladder_update(g.h, kappa, te, to))
        gaps, A, T, seen = ladder_rule(gaps, T, seen, ns.sum(0, dtype=np.uint64), W, kappa, te, to)
        planes, sn = read()
        assert A[0] == 1.0 and (n == 2 or A[1] == 0.0) and (A <= 1.0).all()
        assert_same(sn, seen, "seen after update %d" % call)
        assert_same(planes[1], A, "A after update %d" % call)
        assert_same(planes[0], gaps, "g after update %d" % call)
        assert_same(planes[2], T, "T after update %d" % call)
        lad, tm, be = _tables(g, _lib)
        assert_same(lad, T, "the swap's ladder")
        assert lad[0] == ladder[0] and lad[-1] == ladder[-1]
        want_tm = T.copy()
        if hot:
            want_tm[-1] = 1e80                                            # the hot chain's rank keeps its temperature, the ladder's end its value
        assert_same(tm, want_tm, "temps_mh")
        assert_same(be, 1.0 / tm, "beta == 1 / temps_mh")
        if n == 2:
            assert_same(lad, lad0, "two temperatures: the tables are untouched")
            assert_same(tm, tm0)
            assert_same(be, be0)
        else:
            assert (np.diff(lad) > 0).all() and not np.array_equal(lad, lad0)
        if ev:
            # the evidence stage's gaps are those of the new tables: one sample of a crafted lnL lands on m = dbeta * lnL
            import torch
            g.t["ev_acc"].zero_()
            g.t["ev_cnt"].zero_()
            lnl = rs.randn(W, n) * 10
            g.put("lnL", lnl)
            _lib.check(g.lib.ptmi_ev_update(g.h))
            torch.cuda.synchronize()
            want_acc, _ = ev_rule(lnl[None], dbeta_of(tm))               # (slot == rank: the tables are the identity here)
            assert_same(g.t["ev_acc"].cpu().numpy(), want_acc, "ev_dbeta == dbeta_of(temps_mh) on the device")


def test_publish_installs_a_ladder_and_a_run_tempers_with_it(mods):
    import torch
    orc, _lib, PTEngine = mods
    W, n, d = 70, 5, 5
    rs = np.random.RandomState(12)
    L0, L1 = _some_ladder(rs, n), _some_ladder(rs, n) * 1.5
    kw = dict(cov_update=20, burn=20, tskip=7, seed=23, hot_chain=True)
    p0 = rs.randn(W, n, d) * 0.5
    a = PTEngine(d, n, W, np.eye(d) * 0.3, ladder=L0, **kw)
    read, lad, _ = _own_stage(a, _lib, L0)
    g1, T1, _ = planes_of(L1)
    lad[:n].copy_(torch.from_numpy(g1))
    lad[2 * n:3 * n].copy_(torch.from_numpy(T1))
    _lib.check(a.lib.ptmi_ladder_publish(a.h))
    la, tm, be = _tables(a, _lib)
    assert_same(la, L1, "ladder")
    assert_same(tm[:-1], L1[:-1], "temps_mh")
    assert_same(be, 1.0 / tm, "beta")
    assert tm[-1] == 1e80 and la[-1] == L1[-1]
    assert_same(read()[0][2], T1, "publish only reads the planes")
    b = PTEngine(d, n, W, np.eye(d) * 0.3, ladder=L1, **kw)
    for e in (a, b):
        e.init_state(p0)
        e.run(63)
        e.sync()
    assert b.get("nswap").sum() > 0
    for name in CHAINS:
        assert_same(a.get(name), b.get(name), "published ladder: " + name)


# ------------------------------------------------------------------ engines with the stage, held to the rule on what they count
def _planes(g):
    g.sync()
    return g.t["lad"].cpu().numpy(), g.t["lad_seen"].cpu().numpy().view(np.uint64)


class _Follow(object):
    """The rule applied beside an engine: after every swap epoch ``epoch(g)`` reads nswap and, where ``PTEngine.swap`` updates, updates."""

    def __init__(self, g, sweep=True):
        self.g, self.sweep = g, sweep
        self.gaps, self.T, self.seen = planes_of(g.ladder0)
        self.calls, self.n, self.tries = 0, 0, [0, 0]
        self.hist = dict(iter=[], kappa=[], A=[], ladder=[])

    def epoch(self):
        g = self.g
        it = g.iter
        assert it % g.tskip == 0
        if it > g.adapt_until:
            return None
        if self.sweep:
            self.tries = [self.tries[0] + 1, self.tries[1] + 1]
        else:
            self.tries[(it // g.tskip) & 1] += 1
        self.n += 1
        if self.n < g.adapt_every:
            return None
        ns = g.get("nswap")
        kappa = g.adapt_kappa * g.adapt_t0 / (self.calls + g.adapt_t0)
        self.gaps, A, self.T, self.seen = ladder_rule(self.gaps, self.T, self.seen, ns.sum(0, dtype=np.uint64), g.W, kappa, *self.tries)
        for k, v in (("iter", it), ("kappa", kappa), ("A", A[:-1]), ("ladder", self.T.copy())):
            self.hist[k].append(v)
        self.calls, self.n, self.tries = self.calls + 1, 0, [0, 0]
        return A[:-1]

    def check(self, what):
        g = self.g
        planes, seen = _planes(g)
        assert_same(planes[0], self.gaps, what + ": g")
        assert_same(planes[2], self.T, what + ": T")
        assert_same(seen, self.seen, what + ": seen")
        h = g.ladder_history()
        assert sorted(h) == ["A", "iter", "kappa", "ladder"] and g.lad_calls == self.calls == len(h["iter"])
        assert_same(h["iter"], np.asarray(self.hist["iter"], dtype=np.int64), what + ": history iter")
        assert_same(h["kappa"], np.asarray(self.hist["kappa"], dtype=np.float64), what + ": history kappa")
        assert_same(h["A"], np.asarray(self.hist["A"]).reshape(-1, g.ntg - 1), what + ": history A")
        assert_same(h["ladder"], np.asarray(self.hist["ladder"]).reshape(-1, g.ntg), what + ": history ladder")
        # the host's mirrors show what the device holds
        assert_same(g.ladder, self.T, what + ": engine.ladder")
        want = self.T.copy()
        hot = g.temps_mh0[-1] == 1e80
        if hot:
            want[-1] = 1e80
        assert_same(g.temps_mh, want, what + ": engine.temps_mh")
        assert_same(g.ladder0, planes_of(g.ladder0)[1], what + ": ladder0 stays")


@pytest.fixture(scope="module")
def driven(mods):
    """d = 5, W = 256, the ladder [1, 1.1, 1.25, 8, 9.5, 64], iso likelihood, flat prior; 500 swap epochs of 10 iterations, the ladder
    adapting every 10 epochs up to iteration 4000 -- stepped epoch by epoch with nswap read after each; computed once, left unchanged."""
    orc, _lib, PTEngine = mods
    d, W, n = 5, 256, len(LADDER0)
    kw = dict(ladder=LADDER0, tskip=10, burn=4000, cov_update=1000, seed=5, cov_mode="pooled")
    g = PTEngine.with_stages(d, n, W, np.eye(d) * 0.5, adapt_ladder=dict(every=10), **kw)
    assert g.adapt_until == 4000 and g.adapt_every == 10 and g.adapt_kappa == 2.0 and g.adapt_t0 == 10.0
    p0 = np.random.RandomState(9).randn(W, n, d) * 0.5
    g.init_state(p0)
    fol = _Follow(g)
    out = dict(g=g, fol=fol, kw=kw, p0=p0, windows=[], nswap={}, tables={})
    last = np.zeros((W, n), dtype=np.uint64)
    for e in range(1, 501):
        g.run(10)
        ns = g.get("nswap")
        assert (ns >= last).all() and not ns[:, -1].any()                # counters only grow; column n - 1 is no pair
        last = ns
        A = fol.epoch()
        if A is not None:
            out["windows"].append(A)
        if e == 10:
            out["at100"] = {name: g.get(name) for name in CHAINS}
        if e in (400, 500):
            out["nswap"][e] = g.get("nswap")
            out["tables"][e] = _tables(g, _lib)
    return out


def test_driven_run_follows_the_rule_and_freezes(mods, driven):
    orc, _lib, PTEngine = mods
    g, fol = driven["g"], driven["fol"]
    fol.check("driven run")
    assert g.lad_calls == 40 and g.ladder_history()["iter"].tolist() == list(range(100, 4001, 100))
    # up to the first update the chains are those of an engine without the stage, and that engine carries nothing of it
    b = PTEngine(5, len(LADDER0), 256, np.eye(5) * 0.5, **driven["kw"])
    b.init_state(driven["p0"])
    b.run(100)
    b.sync()
    for name in CHAINS:
        assert_same(driven["at100"][name], b.get(name), "before the first update: " + name)
    assert "lad" not in b.t and "lad_seen" not in b.t and not b.adapt_on and not [k for k in b.checkpoint() if "lad" in k]
    assert_same(b.ladder, LADDER0)
    assert_same(b.ladder0, LADDER0)
    with pytest.raises(ValueError, match="adapt_ladder"):
        b.ladder_history()
    # after iteration 4000 the tables never change again
    for x, y in zip(driven["tables"][400], driven["tables"][500]):
        assert_same(x, y, "frozen after until")
    assert_same(driven["tables"][500][0], g.ladder_history()["ladder"][-1], "the last update's ladder is the one in force")


def test_driven_run_equalises_the_acceptance(driven):
    """Real chains against the independent-sample model (tests/test_ladder_adapt.py: worst final gap deviation 0.0258 over its six runs):
    the cap on the gaps is 5 x the model's worst -- the margin covers what the model lacks, autocorrelation between swap epochs ten
    iterations apart and equilibration after each change -- and the frozen ladder's acceptance spread over epochs 4010 - 5000 stays under
    0.15 against >= 0.7 in the first window.  Measured on an MI355X with this seed: see DESIGN.md section 3.18."""
    g = driven["g"]
    first = driven["windows"][0]
    gaps = np.diff(np.log(driven["tables"][500][0]))
    dev = np.abs(gaps - np.log(64.0) / 5).max()
    acc = (driven["nswap"][500].astype(np.int64) - driven["nswap"][400].astype(np.int64)).sum(0)[:-1] / (g.W * 100.0)
    cap = 5 * model_worst_gap_deviation()
    print("first window: acceptance %s, spread %.3f" % (np.round(first, 3).tolist(), first.max() - first.min()))
    print("final ladder %s" % np.round(driven["tables"][500][0], 4).tolist())
    print("final gaps %s, worst deviation from ln 64 / 5 = %.4f: %.4f (cap %.4f)" % (np.round(gaps, 4).tolist(), np.log(64.0) / 5, dev, cap))
    print("frozen acceptance over epochs 4010 - 5000 %s, spread %.4f (cap 0.15)" % (np.round(acc, 4).tolist(), acc.max() - acc.min()))
    assert first.max() - first.min() >= 0.7
    assert dev < cap
    assert acc.max() - acc.min() < 0.15


KW = dict(cov_update=20, burn=20, tskip=7, seed=17)                    # the default mix (SCAM / AM / DE at 20 each); DE joins after burn
ADAPT = dict(adapt_ladder=dict(every=2, kappa=4.0, t0=3.0, until=63))
W_, T_, D_ = 70, 4, 5


def _p0(seed=1):
    return np.random.RandomState(seed).randn(W_, T_, D_) * 0.5


def _drive(g, advance, epochs=10, sweep=True, fol=None):
    fol = fol or _Follow(g, sweep)
    for _ in range(epochs):
        advance(g.tskip)
        fol.epoch()
    return fol


def test_every_path_gives_the_same_chains_and_planes(mods):
    orc, _lib, PTEngine = mods
    make = lambda **kw: PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, **ADAPT, **dict(KW, **kw))      # noqa: E731
    f = make()
    f.init_state(_p0())
    _drive(f, f.run).check("fused")
    assert f.lad_calls == 4 and f.ladder_history()["iter"].tolist() == [14, 28, 42, 56]      # the window of 63 is half open at until
    assert not np.array_equal(f.ladder, f.ladder0) and f.get("nswap").sum() > 0
    r = make(rows_logl=True)
    r.init_state(_p0())
    _drive(r, r.run).check("rows")
    c = make(split=True)
    logl = c.builtin_logl()
    c.init_state_callback(_p0(), logl, None)
    _drive(c, lambda n: c.run_callback(n, logl, None)).check("callback")
    for name, e in (("rows", r), ("callback", c)):
        for ch in CHAINS:
            assert_same(e.get(ch), f.get(ch), "%s path: %s" % (name, ch))
        assert_same(_planes(e)[0], _planes(f)[0], name + " path: planes")
        assert_same(_planes(e)[1], _planes(f)[1], name + " path: seen")
    # every segment as one graph launch (cycles without AM entries are captured): the tables change under the captured launches
    runs = []
    for graph in (False, True):
        e = make(split=True, weights=(20, 0, 20))
        lg = e.builtin_logl()
        e.init_state_callback(_p0(), lg, None)
        _drive(e, lambda n: e.run_callback(n, lg, None, graph=graph)).check("graph=%r" % graph)
        runs.append(e)
    assert getattr(runs[1], "_graphs", None), "no segment was captured"
    for ch in CHAINS:
        assert_same(runs[1].get(ch), runs[0].get(ch), "graph: " + ch)
    assert_same(_planes(runs[1])[0], _planes(runs[0])[0], "graph: planes")


def test_oddeven_takes_its_tries_from_the_parities(mods):
    orc, _lib, PTEngine = mods
    g = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, swap_mode="oddeven", hot_chain=True,
                             adapt_ladder=dict(every=4, kappa=4.0, until=70), **KW)
    g.init_state(_p0())
    fol = _drive(g, g.run, sweep=False)
    fol.check("oddeven")
    assert g.lad_calls == 2 and g.temps_mh[-1] == 1e80 and g.ladder[-1] == g.ladder0[-1]
    A = g.ladder_history()["A"]
    assert (A <= 1.0).all() and (A > 0).any()                           # two tries per pair and window: a sweep's count of 4 would halve A


def test_evidence_after_an_adapted_burn_in_uses_the_final_gaps(mods):
    orc, _lib, PTEngine = mods
    from ptmcmcsampler_amd.evidence import dbeta_of
    g = PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, adapt_ladder=dict(every=2, kappa=4.0, until=42), evidence=True, evidence_from=42,
                             hot_chain=True, **KW)
    g.init_state(_p0())
    fol = _Follow(g)
    seq = []
    for e in range(1, 11):
        g.run(7)
        fol.epoch()
        if g.iter > 42:
            g.sync()
            seq.append(np.take_along_axis(g.get("lnL"), g.get("slot_of").astype(np.int64), 1))
    fol.check("with the evidence stage")
    assert g.lad_calls == 3 and g.ev_epochs == 4
    assert_same(g.ev_dbeta, dbeta_of(g.temps_mh), "ev_dbeta == dbeta_of(temps_mh)")
    assert not np.array_equal(g.ev_dbeta, dbeta_of(g.temps_mh0))
    want_acc, want_cnt = ev_rule(np.stack(seq), g.ev_dbeta)
    assert_same(g.t["ev_acc"].cpu().numpy(), want_acc, "the device sampled with the adapted gaps")
    assert_same(g.evidence_moments()["betas"], 1.0 / g.temps_mh, "betas")


def test_checkpoint_in_the_middle_of_a_window(mods):
    orc, _lib, PTEngine = mods
    stage = dict(adapt_ladder=dict(every=4, kappa=4.0, until=70))
    make = lambda **kw: PTEngine.with_stages(D_, T_, W_, np.eye(D_) * 0.3, **kw, **KW)      # noqa: E731
    a = make(**stage)
    a.init_state(_p0())
    a.run(70)
    b = make(**stage)
    b.init_state(_p0())
    b.run(42)                                                           # six epochs: one update, two epochs of the next window
    st = b.checkpoint()
    assert st["lad_calls"] == 1 and st["lad_epochs"] == 2 and st["lad_tries"].tolist() == [2, 2]
    assert st["t_lad"].shape == (3, T_) and st["t_lad_seen"].shape == (T_,) and st["lad_hist_planes"].shape == (1, 3, T_)
    c = make(**stage)
    c.restore(st)
    assert_same(c.ladder, b.ladder, "restore publishes the checkpoint's ladder")
    assert_same(c.temps_mh, b.temps_mh)
    c.run(28)
    assert a.lad_calls == 2 and c.lad_calls == 2
    for name in CHAINS:
        assert_same(c.get(name), a.get(name), "resumed " + name)
    assert_same(_planes(c)[0], _planes(a)[0], "resumed planes")
    assert_same(_planes(c)[1], _planes(a)[1], "resumed seen")
    ha, hc = a.ladder_history(), c.ladder_history()
    for k in ha:
        assert_same(hc[k], ha[k], "resumed history " + k)
    assert_same(c.ladder, a.ladder)
    assert_same(c.temps_mh, a.temps_mh)
    # a checkpoint written without the stage is refused before anything is touched
    plain = make()
    plain.init_state(_p0())
    plain.run(28)
    before = _planes(c)
    with pytest.raises(ValueError, match="adapt_ladder"):
        c.restore(plain.checkpoint())
    assert c.iter == 70 and c.lad_calls == 2
    assert_same(_planes(c)[0], before[0], "a refused restore touches nothing")


def test_abi_refusals(mods):
    import torch
    orc, _lib, PTEngine = mods
    W, T, d = 4, 3, 2
    g = PTEngine(d, T, W, np.eye(d), tskip=10)
    L = g.lib
    err = lambda: L.ptmi_last_error().decode()      # noqa: E731
    dp = lambda a: a.ctypes.data_as(_lib._dp)       # noqa: E731
    out = [np.empty(T) for _ in range(3)]
    assert L.ptmi_ladder_update(g.h, 1.0, 1, 1) == -1 and "ptmi_ladder_attach" in err()
    assert L.ptmi_ladder_publish(g.h) == -1 and "ptmi_ladder_attach" in err()
    assert L.ptmi_ladder_read(g.h, dp(out[0]), dp(out[1]), dp(out[2])) == -1 and "ptmi_ladder_attach" in err()
    gaps, Tl, _ = planes_of(g.ladder)
    host = np.concatenate([gaps, np.zeros(T), Tl, [0.0]])
    lad = torch.from_numpy(host).to(g.device)
    seen = torch.zeros(T + 1, dtype=torch.int64, device=g.device)
    pl, ps = lad.data_ptr(), seen.data_ptr()
    assert L.ptmi_ladder_attach(g.h, None, C.c_void_p(ps)) == -1 and "lad" in err()
    assert L.ptmi_ladder_attach(g.h, C.c_void_p(pl + 4), C.c_void_p(ps)) == -1 and "lad" in err() and "aligned" in err()
    assert L.ptmi_ladder_attach(g.h, C.c_void_p(pl), None) == -1 and "seen" in err()
    assert L.ptmi_ladder_attach(g.h, C.c_void_p(pl), C.c_void_p(ps + 2)) == -1 and "seen" in err() and "aligned" in err()
    assert L.ptmi_ladder_update(g.h, 1.0, 1, 1) == -1 and "ptmi_ladder_attach" in err()      # none of them attached anything
    one = PTEngine(d, 1, W, np.eye(d), tskip=10)
    assert L.ptmi_ladder_attach(one.h, C.c_void_p(pl), C.c_void_p(ps)) == -1 and "ntemps_global" in err()
    part = PTEngine(d, T, W, np.eye(d), tskip=10, ntemps_global=2 * T, temp0=0)
    assert L.ptmi_ladder_attach(part.h, C.c_void_p(pl), C.c_void_p(ps)) == -3 and "sharded" in err()      # PTMI_EUNSUPPORTED
    _lib.check(L.ptmi_ladder_attach(g.h, C.c_void_p(pl), C.c_void_p(ps)))
    assert L.ptmi_ladder_attach(g.h, C.c_void_p(pl), C.c_void_p(ps)) == -1 and "already" in err()
    g.put("nswap", np.full((W, T), 3, dtype=np.int64))
    for kappa in (np.nan, np.inf, -np.inf, -1e-9, 8.0000001):
        assert L.ptmi_ladder_update(g.h, kappa, 1, 1) == -1 and "kappa" in err(), kappa
    for te in (0, -5):
        assert L.ptmi_ladder_update(g.h, 1.0, te, 1) == -1 and "tries_even" in err()
    for to in (0, -1):
        assert L.ptmi_ladder_update(g.h, 1.0, 1, to) == -1 and "tries_odd" in err()
    assert L.ptmi_ladder_read(g.h, None, dp(out[1]), dp(out[2])) == -1 and "non-NULL" in err()
    torch.cuda.synchronize()
    assert_same(lad.cpu().numpy(), host, "a refused call launched nothing")
    assert not seen.any().item()
    # two temperatures: one pair, tries_odd is not asked for
    two = PTEngine(d, 2, W, np.eye(d), tskip=10)
    read, _, _ = _own_stage(two, _lib, two.ladder)
    _lib.check(L.ptmi_ladder_update(two.h, 8.0, 1, 0))
    assert read()[1].tolist() == [0, 0]
    # ... and a good call goes through
    _lib.check(L.ptmi_ladder_update(g.h, 8.0, 4, 3))
    torch.cuda.synchronize()
    assert seen.cpu().numpy().tolist() == [3 * W, 3 * W, 0, 0] and lad.cpu().numpy()[T:2 * T].tolist() == [0.75, 1.0, 0.0]


# ------------------------------------------------------------------ the sampler
def _sampler(out, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 4
    kw.setdefault("ntemps", 4)
    s = PTSampler(d, ("iso",), ("box", -5.0 * np.ones(d), 5.0 * np.ones(d)), np.eye(d) * 0.5, outDir=str(out), verbose=False, seed=21,
                  nwalkers=8, **kw)
    s.adapt_ladder = {"every": 2}
    s.log_evidence = True
    return s


def test_sampler_writes_the_ladder_and_resumes(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    run = dict(burn=100, thin=1, covUpdate=50, isave=50, Tskip=10, Tmax=30.0, writeHotChains=True)
    p0 = np.zeros(4)
    a = _sampler(tmp_path / "a", checkpoint=True)
    a.sample(p0, 300, **run)
    la = a.ladder_adapted
    assert sorted(la) == ["A", "history", "iter", "kappa", "ladder", "ladder0", "until"]
    assert la["until"] == 100 and la["iter"].tolist() == list(range(20, 101, 20)) and la["history"].shape == (5, 4) and la["A"].shape == (5, 3)
    assert_same(la["ladder"], la["history"][-1])
    assert_same(la["ladder0"], np.asarray(a.ladder, dtype=np.float64))
    assert la["ladder"][0] == 1.0 and la["ladder"][-1] == la["ladder0"][-1] and not np.array_equal(la["ladder"], la["ladder0"])
    assert_same(a.engine.ladder, la["ladder"])
    assert_same(a.engine.ladder0, la["ladder0"])
    f = np.load(tmp_path / "a" / "ladder.npz")
    assert sorted(f.files) == sorted(la)
    for k in f.files:
        assert_same(f[k], la[k], k)
    # chain files keep the names of the initial ladder's temperatures
    for t in la["ladder0"][1:]:
        assert (tmp_path / "a" / "chain_{0}.txt".format(t)).exists()
    # the evidence after an adapted burn-in reports the betas of the final ladder
    assert_same(a.evidence["betas"], 1.0 / a.engine.temps_mh, "betas == 1 / temps_mh of the final ladder")
    assert_same(a.engine.temps_mh, la["ladder"]) and (a.evidence["n"] == 20).all()
    # stopped at 50 -- inside burn-in, one update and half a window in -- and resumed from its checkpoint
    b1 = _sampler(tmp_path / "b", checkpoint=True)
    b1.sample(p0, 50, **run)
    assert b1.ladder_adapted["iter"].tolist() == [20, 40] and b1.engine.lad_epochs == 1
    b2 = _sampler(tmp_path / "b", checkpoint=True, resume=True)
    b2.sample(p0, 300, **run)
    assert np.array_equal(a._chains, b2._chains)
    for k in la:
        assert_same(b2.ladder_adapted[k], la[k], "resumed " + k)
    for k in a.evidence:
        assert_same(b2.evidence[k], a.evidence[k], "resumed evidence " + k)
    # the ladder must be frozen before the evidence stage's first sample
    late = _sampler(tmp_path / "late")
    late.adapt_ladder = {"until": 150}
    with pytest.raises(ValueError, match="evidence_from"):
        late.sample(p0, 300, **run)
    # set after the engine was built
    off = PTSampler(4, ("iso",), ("flat",), np.eye(4) * 0.5, outDir=str(tmp_path / "off"), verbose=False, seed=21, ntemps=2)
    off.sample(p0, 100, **run)
    assert off.ladder_adapted is None and not (tmp_path / "off" / "ladder.npz").exists() and not off.engine.adapt_on
    off.adapt_ladder = True
    with pytest.raises(ValueError, match="before the first sample"):
        off.writeOutput(100)
