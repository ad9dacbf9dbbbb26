"""The temperature ladder adapted from every walker's swaps (csrc/ptmi_ladder.hip, include/ptmi.h ptmi_ladder_attach / _update / _publish /
_read; ``PTEngine.with_stages(adapt_ladder=...)``, ``PTSampler.adapt_ladder``) -- what can be checked without a GPU: the rule restated in
NumPy one operation at a time (``ladder_rule``, which tests/test_ladder_adapt_gpu.py holds the device to, bit for bit) against plain
expressions; its behaviour in a model that samples lnL independently at every rank of an iso Gaussian (``model_run``: not real chains --
the GPU test drives those -- but the same swap test, the same counters, the same windows); the C ABI; the refusals that fall before a
library is loaded; and that the stage is opt-in."""
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_ladder_attach", "ptmi_ladder_update", "ptmi_ladder_publish", "ptmi_ladder_read")
LADDER0 = np.array([1.0, 1.1, 1.25, 8.0, 9.5, 64.0])                     # two pairs nearly closed, two wide open: the driven runs' start


def planes_of(ladder):
    """(g, T, seen) as the caller of ptmi_ladder_attach fills them: log gaps (entry n - 1 unused), the ladder, zeros."""
    T = np.array(ladder, dtype=np.float64)
    g = np.zeros(len(T))
    g[:-1] = np.log(T[1:]) - np.log(T[:-1])
    return g, T, np.zeros(len(T), dtype=np.uint64)


def ladder_rule(g, T, seen, acc, W, kappa, tries_even, tries_odd):
    """The contract of ptmi_ladder_update, restated: planes ``g [n]``, ``T [n]``, ``seen [n]`` (uint64) and the column sums ``acc [n]`` of
    nswap (uint64) -> ``(g', A, T', seen')``.  Every operation is one IEEE double operation in the order of include/ptmi.h; the
    exponential is the oracle's (the one the device's is held to bit for bit).  Entry n - 1 of g, A and seen is not a pair: it stays
    (A: zero)."""
    from oracle import oracle as orc
    exp = orc.lib().orc_exp
    g, T = np.array(g, dtype=np.float64), np.array(T, dtype=np.float64)
    seen, acc = np.array(seen, dtype=np.uint64), np.asarray(acc, dtype=np.uint64)
    n = len(T)
    n1 = n - 1
    A = np.zeros(n)
    kappa = np.float64(kappa)
    for k in range(n1):
        tries = tries_odd if k & 1 else tries_even
        diff = (int(acc[k]) - int(seen[k])) & (2 ** 64 - 1)             # the difference in integers
        A[k] = np.float64(float(diff)) / (np.float64(float(W)) * np.float64(float(tries)))
        seen[k] = acc[k]
    if n > 2:
        h = np.zeros(n1)
        for k in range(n1):
            h[k] = g[k] * np.float64(exp(float(kappa * A[k])))
        s = np.float64(0.0)
        for k in range(n1):
            s = s + h[k]
        G = np.float64(0.0)
        for k in range(n1):
            G = G + g[k]
        for k in range(n1):
            g[k] = G * (h[k] / s)
        c = np.float64(0.0)
        for k in range(1, n1):
            c = c + g[k - 1]
            T[k] = T[0] * np.float64(exp(float(c)))
    return g, A, T, seen


# ------------------------------------------------------------------ the independent-sample model
def model_run(mode, seed, ladder=LADDER0, d=5, W=64, every=10, updates=40, kappa0=2.0, t0=10.0):
    """lnL = -|x|^2 / 2 with x ~ N(0, T_r) drawn afresh at every rank and swap epoch (no chains: no autocorrelation, no equilibration), the
    reference's swap test on it -- the sweep hottest pair first with the states travelling, or the disjoint pairs of the epoch's parity
    -- credited to nswap [W][n] as the device credits it, and ``ladder_rule`` behind every ``every`` epochs with kappa0 t0 / (call + t0).
    Returns (A of every window [updates][n - 1], gaps after every update [updates][n - 1])."""
    rs = np.random.RandomState(seed)
    g, T, seen = planes_of(ladder)
    n = len(T)
    nswap = np.zeros((W, n), dtype=np.uint64)
    epoch = 0
    As, gaps = [], []
    for call in range(updates):
        tries = [0, 0]
        for _ in range(every):
            epoch += 1
            lnl = -0.5 * T[None, :] * rs.chisquare(d, size=(W, n))
            logu = np.log(rs.rand(W, n - 1))
            if mode == "sweep":
                pairs = range(n - 2, -1, -1)
                tries[0] += 1
                tries[1] += 1
            else:
                pairs = [k for k in range(n - 1) if k % 2 == epoch % 2]
                tries[epoch % 2] += 1
            for k in pairs:
                acc = logu[:, k] < (1.0 / T[k] - 1.0 / T[k + 1]) * (lnl[:, k + 1] - lnl[:, k])
                lo, hi = lnl[:, k].copy(), lnl[:, k + 1].copy()
                lnl[:, k], lnl[:, k + 1] = np.where(acc, hi, lo), np.where(acc, lo, hi)
                nswap[:, k] += acc.astype(np.uint64)
        g, A, T, seen = ladder_rule(g, T, seen, nswap.sum(0, dtype=np.uint64), W, kappa0 * t0 / (call + t0), tries[0], tries[1])
        As.append(A[:-1].copy())
        gaps.append(g[:-1].copy())
    return np.array(As), np.array(gaps)


@functools.lru_cache(maxsize=None)
def model_results():
    """(mode, seed) -> (spread of the first window's acceptances, spread of the last window's, worst |gap - ln 64 / 5| at the end)."""
    out = {}
    for mode in ("sweep", "oddeven"):
        for seed in (1, 2, 3):
            A, gaps = model_run(mode, seed)
            out[mode, seed] = (A[0].max() - A[0].min(), A[-1].max() - A[-1].min(), np.abs(gaps[-1] - np.log(64.0) / 5).max())
    return out


def model_worst_gap_deviation():
    """The worst final |gap - ln 64 / 5| over the model's six runs: what the GPU test scales its convergence cap from."""
    return max(v[2] for v in model_results().values())


# ------------------------------------------------------------------ the rule against plain expressions
def test_the_rule_preserves_the_sum_of_the_gaps_and_the_ends():
    rs = np.random.RandomState(3)
    for n in (3, 4, 7, 33, 64):
        ladder = np.cumprod(np.concatenate([[0.7], 1.0 + rs.rand(n - 1) * 2.0]))
        g, T, seen = planes_of(ladder)
        W, te, to = 50, 7, 5
        acc = np.zeros(n, dtype=np.uint64)
        for call in range(3):
            acc[:-1] += (rs.rand(n - 1) * W * np.where(np.arange(n - 1) % 2, to, te)).astype(np.uint64)
            g2, A, T2, seen2 = ladder_rule(g, T, seen, acc, W, 8.0 / (1 + call), te, to)
            assert abs(g2[:-1].sum() - g[:-1].sum()) <= 1e-14 * g[:-1].sum()
            assert T2[0] == ladder[0] and T2[-1] == ladder[-1]             # both ends are never rewritten
            assert np.allclose(np.log(T2[1:]) - np.log(T2[:-1]), g2[:-1], rtol=0, atol=1e-12)      # (ln T reaches 20: its own rounding is 4e-15 an entry)
            assert np.array_equal(seen2[:-1], acc[:-1]) and (0 <= A).all() and (A <= 1).all()
            plain = g[:-1] * np.exp(8.0 / (1 + call) * A[:-1])
            assert np.allclose(g2[:-1], g[:-1].sum() * plain / plain.sum(), rtol=1e-13)
            g, T, seen = g2, T2, seen2


def test_equal_acceptance_and_zero_gain_leave_the_gaps():
    rs = np.random.RandomState(4)
    n, W = 9, 32
    ladder = np.cumprod(np.concatenate([[1.0], 1.0 + rs.rand(n - 1)]))
    g, T, seen = planes_of(ladder)
    acc = np.zeros(n, dtype=np.uint64)
    acc[:-1] = 3 * W                                                       # A = 0.75 on every pair: only differences of A matter
    g2, A, T2, _ = ladder_rule(g, T, seen, acc, W, 8.0, 4, 4)
    assert (A[:-1] == 0.75).all()
    assert np.allclose(g2[:-1], g[:-1], rtol=1e-15, atol=0) and np.allclose(T2, T, rtol=1e-14)
    acc[:-1] = (rs.rand(n - 1) * 4 * W).astype(np.uint64)                  # any acceptance at kappa = 0
    g3, A3, T3, _ = ladder_rule(g, T, seen, acc, W, 0.0, 4, 4)
    assert A3[:-1].max() > A3[:-1].min()
    assert np.allclose(g3[:-1], g[:-1], rtol=1e-15, atol=0)


def test_gaps_stay_positive_and_the_ladder_increasing_at_the_extremes():
    n, W = 6, 10
    for bits in range(2 ** (n - 1)):                                       # every pattern of A in {0, 1}, at the largest gain
        g, T, seen = planes_of(LADDER0)
        acc = np.array([W * 5 * ((bits >> k) & 1) for k in range(n - 1)] + [0], dtype=np.uint64)
        for _ in range(3):
            g, A, T, seen = ladder_rule(g, T, seen, acc, W, 8.0, 5, 5)
            acc = acc + np.array([W * 5 * ((bits >> k) & 1) for k in range(n - 1)] + [0], dtype=np.uint64)
            assert set(A[:-1].tolist()) <= {0.0, 1.0}
            assert (g[:-1] > 0).all() and (np.diff(T) > 0).all() and T[0] == 1.0 and T[-1] == 64.0


def test_the_difference_is_taken_in_integers_and_two_temperatures_write_no_table():
    W = 4
    g, T, seen = planes_of([1.0, 2.0, 5.0])
    seen[:2] = [2 ** 53 + 1, 2 ** 60 + 3]                                  # neither is a double: a floating-point difference would be off
    acc = np.array([2 ** 53 + 1 + 8, 2 ** 60 + 3 + 2, 0], dtype=np.uint64)
    g2, A, T2, seen2 = ladder_rule(g, T, seen, acc, W, 1.0, 2, 1)
    assert A[0] == 1.0 and A[1] == 0.5 and seen2[0] == acc[0] and g2[0] > g[0]
    g, T, seen = planes_of([1.0, 3.0])
    g2, A, T2, seen2 = ladder_rule(g, T, seen, np.array([6, 9], dtype=np.uint64), W, 2.0, 3, 0)
    assert A.tolist() == [0.5, 0.0] and seen2.tolist() == [6, 0]           # (column n - 1 is no pair)
    assert np.array_equal(g2, g) and np.array_equal(T2, T)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("mode", ["sweep", "oddeven"])
def test_the_model_equalises_the_acceptance(mode):
    """Measured over seeds 1 - 3 and both modes: first-window spread 0.84 - 0.88, last-window spread 0.02 - 0.12, final gaps within 0.026
    of ln 64 / 5.  The caps: a first-window spread of at least 0.7 (the start is far from equal acceptance), final gaps within 0.06 of
    equal (twice the worst this model showed when the rule was designed, 0.029)."""
    for seed in (1, 2, 3):
        first, last, dev = model_results()[mode, seed]
        print("%s seed %d: first-window spread %.3f, last-window spread %.3f, worst gap deviation %.4f" % (mode, seed, first, last, dev))
        assert first >= 0.7
        assert dev <= 0.06
    assert 0.0 < model_worst_gap_deviation() <= 0.06


def test_a_geometric_ladder_stays_where_it_is():
    d, n = 100, 64
    ladder = (1.0 + np.sqrt(2.0 / d)) ** np.arange(n)
    _, gaps = model_run("sweep", 5, ladder=ladder, d=d, updates=20)
    g0 = np.log(1.0 + np.sqrt(2.0 / d))
    print("worst |gap - gap0| over 20 updates: %.4f of %.4f" % (np.abs(gaps - g0).max(), g0))
    assert np.abs(gaps - g0).max() <= 0.5 * g0                            # equal acceptance is this ladder's own property (Gaussian target): no gap gains or loses half of itself to the windows' noise


# ------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from ptmcmcsampler_amd import _lib
    if not os.path.exists(_lib.SO):
        ge.build()
    return _lib


def test_header_binding_and_library_carry_the_entry_points(lib):
    import ctypes as C
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_ladder_\w+)\(([^;]*)\);", hdr)}
    assert decl == {"ptmi_ladder_attach": "ptmi_handle h, double *lad , uint64_t *seen",
                    "ptmi_ladder_update": "ptmi_handle h, double kappa, int64_t tries_even, int64_t tries_odd",
                    "ptmi_ladder_publish": "ptmi_handle h",
                    "ptmi_ladder_read": "ptmi_handle h, double *ladder , double *temps_mh , double *beta"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS and s in exported, s
    assert not [s for s in exported if "ladder_free" in s or "ev_dbeta" in s]      # the units' own links stay inside the library
    H, dp = C.c_void_p, C.POINTER(C.c_double)
    assert L.ptmi_ladder_attach.argtypes == [H, C.c_void_p, C.c_void_p]
    assert L.ptmi_ladder_update.argtypes == [H, C.c_double, C.c_int64, C.c_int64]
    assert L.ptmi_ladder_publish.argtypes == [H]
    assert L.ptmi_ladder_read.argtypes == [H, dp, dp, dp]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_ladder.hip" for src in _build.deps())
    assert re.search(r'"ptmi_ladder\.hip"\), os\.path\.join\(OBJ, "ladder\.o"\)', inspect.getsource(_build.build))


# ------------------------------------------------------------------ opt-in, refusals
def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTSampler.adapt_ladder is False and PTSampler.ladder_adapted is None
    assert PTEngine.adapt_on is False and PTEngine._adapt is None
    sig = inspect.signature(PTEngine.with_stages).parameters
    assert sig["adapt_ladder"].default is None and sig["adapt_ladder"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "adapt_ladder" not in inspect.signature(PTEngine.__init__).parameters
    for name in ("adapt_ladder", "ladder_adapted"):
        assert name not in inspect.signature(PTSampler.__init__).parameters
        assert name not in inspect.signature(PTSampler.sample).parameters
    with pytest.raises(TypeError, match="adapt_ladder"):                # the plain constructors keep their parameters
        PTEngine(6, 2, 1, np.eye(6), adapt_ladder=True)
    with pytest.raises(TypeError, match="adapt_ladder"):
        _sampler(tmp_path, "kw", adapt_ladder=True)
    s = _sampler(tmp_path, "kw2")
    assert s._adapt_kw() == {}
    s.adapt_ladder = True
    assert s._adapt_kw() == dict(adapt_ladder=True)
    s.adapt_ladder = {"every": 4, "until": 50}
    assert s._adapt_kw() == dict(adapt_ladder={"every": 4, "until": 50})
    for bad in ({"each": 2}, 3, "yes"):
        s.adapt_ladder = bad
        with pytest.raises(ValueError, match="adapt_ladder"):
            s._adapt_kw()


def test_refusals_fall_before_any_library_is_loaded(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    from ptmcmcsampler_amd.sharded import ShardedPTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    d = 4
    make = lambda nt=3, **kw: PTEngine.with_stages(d, nt, 2, np.eye(d), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="one temperature"):
        make(nt=1, adapt_ladder=True)
    with pytest.raises(ValueError, match="oddeven"):
        make(adapt_ladder=dict(every=5), swap_mode="oddeven")
    with pytest.raises(ValueError, match="evidence_from"):
        make(adapt_ladder=dict(until=200), evidence=True, evidence_from=100, burn=300)
    with pytest.raises(ValueError, match="evidence_from"):
        make(adapt_ladder=True, evidence=True, evidence_from=100, burn=300)           # until defaults to burn
    for every in (0, -3, 2.5):
        with pytest.raises(ValueError, match="every"):
            make(adapt_ladder=dict(every=every))
    for kappa in (-0.1, 8.5, np.nan, np.inf, "2"):
        with pytest.raises(ValueError, match="kappa"):
            make(adapt_ladder=dict(kappa=kappa))
    for t0 in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="t0"):
            make(adapt_ladder=dict(t0=t0))
    for until in (-1, 2.5):
        with pytest.raises(ValueError, match="until"):
            make(adapt_ladder=dict(until=until))
    with pytest.raises(ValueError, match="tskip"):
        make(adapt_ladder=True, tskip=0)
    with pytest.raises(ValueError, match="keys among"):
        make(adapt_ladder=dict(each=3))
    with pytest.raises(ValueError, match="keys among"):
        make(adapt_ladder=7)
    for kw in (dict(ntemps_global=6), dict(ntemps_global=6, temp0=3)):
        with pytest.raises(ValueError, match="sharded ladder"):
            make(adapt_ladder=True, **kw)
    with pytest.raises(ValueError, match="sharded ladder"):
        ShardedPTEngine(d, 4, 2, np.eye(d), local_factory=PTEngine.with_stages, adapt_ladder=True)
    # good requests: the constructor gets as far as loading the library
    for kw in (dict(adapt_ladder=True), dict(adapt_ladder=dict(every=4, kappa=8.0, t0=1.0, until=0), swap_mode="oddeven"),
               dict(adapt_ladder=dict(until=100), evidence=True, evidence_from=100), dict(nt=2, adapt_ladder=dict(every=1)),
               dict(adapt_ladder=False), dict()):
        with pytest.raises(AssertionError, match="library was loaded"):
            make(**kw)


def test_a_replayed_resume_names_the_checkpoint(tmp_path):
    s = _sampler(tmp_path, "replay", resume=True, checkpoint=False)
    os.makedirs(s.outDir, exist_ok=True)
    np.savetxt(os.path.join(s.outDir, "chain_1.txt"), np.zeros((1, 3 + 4)))      # a chain file and no device checkpoint
    s.adapt_ladder = True
    with pytest.raises(NotImplementedError, match="checkpoint=True"):
        s.sample(np.zeros(3), 10, isave=10, thin=1)
