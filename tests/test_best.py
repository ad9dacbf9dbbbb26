"""The best-fit (MAP / ML) row of every cold chain, tracked on the device (csrc/ptmi_best.hip, include/ptmi.h ptmi_best_attach /
ptmi_best_update; ``PTEngine.with_stages(best=True)``, ``PTSampler.track_best``) -- what can be checked without a GPU: the C ABI
carries the two entry points to the letter, the stage is opt-in, its refusals fall before a library is loaded, the reader's calls, the
rule restated in NumPy (``np_update``: what the GPU tests hold the kernel to) against a plain Python loop with ties, NaN, infinities
and signed zeros and over random cuts of one run into calls, the walker pick of ``best()``, and the sampler's refusals.
The runs themselves: tests/test_best_gpu.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_best_attach", "ptmi_best_update")


# ---------------------------------------------------------------------- the rule, restated
def new_state(W, d=0):
    """Nothing held: rows [2][W][d], val [2][W][3] (score, lnL, lp), iters [2][W] = -1."""
    return dict(rows=np.zeros((2, W, d)), val=np.zeros((2, W, 3)), iters=np.full((2, W), -1, dtype=np.int64))


def np_update(state, aux, its, beta0, x=None):
    """One call of the rule in NumPy, in place: ``aux`` [W][n][2] = (lnL, lp) of the iterations ``its`` [n] (ascending), ``x`` [W][n][d]
    their rows (or None).  Plane 0 scores ``beta0 * lnL + lp`` (the product rounded, then the sum), plane 1 ``lnL``; per walker the
    call's candidate is the EARLIEST iteration with the largest non-NaN score, and it replaces the held best iff nothing is held or
    its score is ``>`` the held one."""
    aux, its = np.asarray(aux, dtype=np.float64), np.asarray(its, dtype=np.int64)
    if its.size == 0:
        return state
    with np.errstate(invalid="ignore"):
        scores = (beta0 * aux[..., 0] + aux[..., 1], aux[..., 0])
    ar = np.arange(aux.shape[0])
    for p, sc in enumerate(scores):
        valid = ~np.isnan(sc)
        m = np.where(valid, sc, -np.inf).max(axis=1)
        j = np.argmax(valid & (sc == m[:, None]), axis=1)             # the first of the maxima (0.0 == -0.0: a tie)
        with np.errstate(invalid="ignore"):
            better = valid.any(axis=1) & ((state["iters"][p] < 0) | (m > state["val"][p, :, 0]))
        w = ar[better]
        state["val"][p, w, 0] = sc[w, j[w]]
        state["val"][p, w, 1:] = aux[w, j[w]]
        state["iters"][p, w] = its[j[w]]
        if x is not None:
            state["rows"][p, w] = x[w, j[w]]
    return state


def loop_update(state, aux, its, beta0):
    """The rule as the issue words it, one iteration and one walker at a time."""
    for w in range(len(aux)):
        for n, it in enumerate(its):
            lnl, lp = float(aux[w][n][0]), float(aux[w][n][1])
            prod = np.float64(beta0) * np.float64(lnl)
            with np.errstate(invalid="ignore"):
                score = (float(prod + np.float64(lp)), lnl)
            for p in range(2):
                s = score[p]
                if s != s:
                    continue
                if state["iters"][p, w] < 0 or s > state["val"][p, w, 0]:
                    state["val"][p, w] = (s, lnl, lp)
                    state["iters"][p, w] = it
    return state


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), "%s: %d of %d words differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[0])


def same_state(a, b, what=""):
    assert np.array_equal(a["iters"], b["iters"]), (what, a["iters"], b["iters"])
    same_bits(a["val"], b["val"], what + " val")
    same_bits(a["rows"], b["rows"], what + " rows")


PAYLOAD = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]


def seeded_aux(rs, W, n):
    """lnL / lp with ties, NaN (one with a payload), infinities and signed zeros sprinkled in; values on a coarse grid so maxima repeat."""
    aux = np.round(rs.randn(W, n, 2) * 2.0) / 2.0
    for v in (np.nan, PAYLOAD, np.inf, -np.inf, 0.0, -0.0):
        hit = rs.rand(W, n, 2) < 0.04
        aux[hit] = v
    return aux


# ---------------------------------------------------------------------- the C ABI and the stage's surface
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from ptmcmcsampler_amd import _lib
    if not os.path.exists(_lib.SO):
        ge.build()
    return _lib


def test_header_binding_and_library_carry_the_entry_points(lib):
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_best_\w+)\(([^;]*)\);", hdr)}
    assert decl == {
        "ptmi_best_attach": "ptmi_handle h, double *rows /* dev [2][W][ndim], PARAMETER order, caller-owned */, "
                            "double *val /* dev [2][W][3]: score, lnL, lp */, int64_t *iters /* dev [2][W], -1 = nothing held */, double beta0",
        "ptmi_best_update": "ptmi_handle h, int64_t iter_lo, int64_t iter_hi"}
    assert "_writeToFile" in hdr[hdr.index("csrc/ptmi_best.hip"):hdr.index("int ptmi_best_attach")]      # it says what it replaces
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS, s
        assert s in exported, s
    H = C.c_void_p
    assert L.ptmi_best_attach.argtypes == [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
    assert L.ptmi_best_update.argtypes == [H, C.c_int64, C.c_int64]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_best.hip" for src in _build.deps())
    assert re.search(r'"ptmi_best\.hip"\), os\.path\.join\(OBJ, "best\.o"\), \[\]\)', inspect.getsource(_build.build))
    # ptmi_config and ptmi_buffers are what they were: the stage's state lives in the handle
    assert "best" not in lib.BUFFER_FIELDS and not any("best" in n for n, _ in lib.Config._fields_)
    unit = open(os.path.join(ROOT, "ptmcmcsampler_amd", "csrc", "ptmi_best.hip")).read()
    assert re.search(r'#define PTMI_RING_RANGE_ONLY[^\n]*\n#include "ptmi_ring_weight\.h"', unit) and "atomic" not in unit.lower().replace("no atomics", "")


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine, _RingReader
    assert PTSampler.track_best is None and PTSampler.best is None
    assert _sampler(tmp_path, "default").track_best is None
    sig = inspect.signature(PTEngine.with_stages).parameters
    assert sig["best"].default is False and sig["best_from"].default is None
    for name in ("best", "best_from"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert name not in inspect.signature(PTEngine.__init__).parameters
        assert name not in inspect.signature(PTSampler.__init__).parameters
        assert name not in inspect.signature(PTSampler.sample).parameters
    assert "track_best" not in inspect.signature(PTSampler.__init__).parameters
    assert "track_best" not in inspect.signature(PTSampler.sample).parameters
    with pytest.raises(TypeError, match="best"):                     # the plain constructors keep their parameters
        PTEngine(6, 1, 1, np.eye(6), best=True)
    with pytest.raises(TypeError, match="track_best"):
        _sampler(tmp_path, "kw", track_best=True)
    assert list(_RingReader.WORDS) == ["hist", "pairs", "diag", "samples", "best"] and len(_RingReader.WORDS["best"]) == 4
    for prop in ("best_from", "best_iter"):
        assert isinstance(getattr(PTEngine, prop), property) and getattr(PTEngine, prop).fset is None


def test_refusals_fall_before_any_library_is_loaded(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    d = 4
    make = lambda **kw: PTEngine.with_stages(d, 1, 1, np.eye(d), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="keep_lnl=True"):
        make(best=True)
    with pytest.raises(ValueError, match="keep_lnl=True"):
        make(best=True, keep_lnl=False, best_from=3)
    with pytest.raises(ValueError, match="best_from"):
        make(best=True, keep_lnl=True, best_from=-1)
    with pytest.raises(ValueError, match="best_from= goes with best=True"):
        make(best_from=5, keep_lnl=True)
    for kw in (dict(best=True, keep_lnl=True), dict(best=True, keep_lnl=True, best_from=0), dict(best=True, keep_lnl=True, best_from=70, samples=8)):
        with pytest.raises(AssertionError, match="library was loaded"):      # good specs: the constructor gets as far as loading the library
            make(**kw)


def test_the_reader_calls_nothing_up_to_best_from_then_the_open_range():
    from ptmcmcsampler_amd.engine import PTEngine
    calls = []
    e = PTEngine.__new__(PTEngine)                                   # an engine that never saw its constructor, with what best_sync reads
    e.iter, e.cov_update, e.owns_cold, e._ring = 0, 20, True, []
    e._ring_reader("samples", True, None, 7, lambda eng, lo, hi, n: calls.append(("samples", lo, hi)))
    e._ring_reader("best", True, None, 0, lambda eng, lo, hi, n: calls.append(("best", lo, hi, n)))
    assert [r.name for r in e._ring] == ["samples", "best"] and e.best_from == 0 and e.best_iter == 0 and e.samples_from == 7
    e.iter = 9
    e.best_sync(0)
    assert calls == []
    e.best_sync(4)
    e.best_sync(4)
    e.best_sync(9)
    assert calls == [("best", 1, 4, 0), ("best", 5, 9, 4)] and e.best_iter == 9
    with pytest.raises(ValueError, match=r"best_sync\(10\): the engine has reached iteration 9"):
        e.best_sync(10)
    e.iter = 45
    with pytest.raises(ValueError, match=r"best_sync\(45\): iterations 10..40 are no longer in the ring"):
        e.best_sync(45)
    assert e.best_iter == 9
    with pytest.raises(AttributeError):
        e.best_from = 3                                              # read-only
    # a later start: nothing up to best_from, then (iter + 1, it)
    calls.clear()
    f = PTEngine.__new__(PTEngine)
    f.iter, f.cov_update, f.owns_cold, f._ring = 19, 20, True, []
    f._ring_reader("best", True, 12, 0, lambda eng, lo, hi, n: calls.append((lo, hi, n)))
    for it in (5, 12):
        f.best_sync(it)
    assert calls == [] and f.best_iter == 12
    f.best_sync(13)
    f.best_sync(19)
    assert calls == [(13, 13, 0), (14, 19, 1)]
    g = PTEngine.__new__(PTEngine)
    g._ring = []
    with pytest.raises(ValueError, match=r"no best-fit tracker: PTEngine.with_stages\(..., best=True\)"):
        g.best_sync(1)


# ---------------------------------------------------------------------- the rule
def test_numpy_rule_equals_the_plain_loop_on_special_values():
    rs = np.random.RandomState(20)
    for trial, beta0 in enumerate((1.0, 1.0 / 1.7, 0.25, 1.0, 3.0)):
        W, n = 7, 90
        aux = seeded_aux(rs, W, n)
        its = np.arange(1, n + 1)
        a, b = new_state(W), new_state(W)
        np_update(a, aux, its, beta0)
        loop_update(b, aux, its, beta0)
        same_state(a, b, "trial %d" % trial)
        assert (a["iters"] >= 1).all()


def test_rule_edge_cases():
    nan, inf = np.nan, np.inf
    # ties: the earliest of the maxima; 0.0 and -0.0 tie; NaN never wins and never poisons; -inf wins only against nothing
    aux = np.array([[[1.0, 0.0], [2.0, 0.0], [2.0, 0.0], [nan, 0.0], [1.5, 0.0]],            # tie of 2.0: iteration 2
                    [[-inf, 0.0], [-inf, 0.0], [nan, nan], [nan, 0.0], [nan, 1.0]],          # a first candidate of -inf: iteration 1 stays
                    [[-0.0, 0.0], [0.0, 0.0], [-0.0, -0.0], [0.0, -0.0], [-1.0, 0.0]],       # signed zeros tie: iteration 1, lnL = -0.0
                    [[nan, 0.0], [nan, nan], [PAYLOAD, 0.0], [0.0, nan], [nan, 0.0]],        # MAP: every score NaN; ML: iteration 4, lp NaN
                    [[inf, -inf], [1.0, 1.0], [0.5, 9.0], [inf, 0.0], [2.0, 0.0]],           # inf - inf: NaN for MAP, a winner for ML
                    [[-inf, 0.0], [-5.0, 0.0], [-inf, 0.0], [-5.0, 0.0], [-6.0, 0.0]]])      # -inf held, then beaten
    its = np.arange(11, 16)
    a, b = new_state(6), new_state(6)
    np_update(a, aux, its, 1.0)
    loop_update(b, aux, its, 1.0)
    same_state(a, b)
    assert a["iters"][0].tolist() == [12, 11, 11, -1, 14, 12] and a["iters"][1].tolist() == [12, 11, 11, 14, 11, 12]
    assert np.signbit(a["val"][1, 2, 0]) and np.signbit(a["val"][1, 2, 1])      # the held -0.0 stayed
    assert (a["val"][0, 3] == 0.0).all()                             # nothing held: untouched
    assert np.isnan(a["val"][1, 3, 2]) and a["val"][1, 3, 0] == 0.0
    assert a["val"][0, 4].tolist() == [inf, inf, 0.0] and a["val"][1, 4].tolist() == [inf, inf, -inf]
    # a later call whose maximum equals the held one: the held one stays; NaN against a held value: stays
    later = np.array([[[2.0, 0.0], [nan, 0.0]], [[-inf, 0.0], [-inf, 0.0]], [[0.0, 0.0], [-0.0, 0.0]], [[nan, 0.0], [nan, nan]],
                      [[inf, 0.0], [inf, 1.0]], [[-5.0, 0.0], [-4.5, 0.0]]])
    before = {k: v.copy() for k, v in a.items()}
    np_update(a, later, np.array([16, 17]), 1.0)
    loop_update(b, later, np.array([16, 17]), 1.0)
    same_state(a, b, "second call")
    assert a["iters"][0].tolist() == [12, 11, 11, -1, 14, 17] and a["iters"][1].tolist() == [12, 11, 11, 14, 11, 17]
    same_bits(a["val"][:, :5], before["val"][:, :5], "held")
    # MAP and ML pick different iterations where lp says so
    c = new_state(1)
    np_update(c, np.array([[[3.0, -10.0], [1.0, 0.0], [2.0, -0.5]]]), np.array([1, 2, 3]), 1.0)
    assert c["iters"][:, 0].tolist() == [3, 1] and c["val"][0, 0].tolist() == [1.5, 2.0, -0.5] and c["val"][1, 0].tolist() == [3.0, 3.0, -10.0]
    # an empty call changes nothing
    same_state(np_update(new_state(2), np.zeros((2, 0, 2)), np.zeros(0, dtype=np.int64), 1.0), new_state(2))


def test_random_cuts_of_one_run_give_the_same_state():
    rs = np.random.RandomState(23)
    for trial in range(60):
        W, n, d = int(rs.randint(1, 6)), int(rs.randint(1, 150)), 2
        beta0 = float(rs.choice([1.0, 1.0 / 1.7, 0.5]))
        aux = seeded_aux(rs, W, n)
        x = rs.randn(W, n, d)
        its = np.arange(1, n + 1)
        whole = np_update(new_state(W, d), aux, its, beta0, x)
        ref = loop_update(new_state(W, d), aux, its, beta0)
        ref["rows"] = whole["rows"]
        same_state(whole, ref, "trial %d" % trial)
        held = whole["iters"] >= 0
        for p in range(2):
            for w in np.flatnonzero(held[p]):
                same_bits(whole["rows"][p, w], x[w, whole["iters"][p, w] - 1])
        for _ in range(4):
            cuts = sorted(set(rs.randint(0, n + 1, rs.randint(0, 8)).tolist()) | {0, n})
            parts = new_state(W, d)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                np_update(parts, aux[:, lo:hi], its[lo:hi], beta0, x[:, lo:hi])
            same_state(parts, whole, "trial %d, cuts %s" % (trial, cuts))


# ---------------------------------------------------------------------- the walker pick of best()
def test_walker_pick():
    from ptmcmcsampler_amd.engine import best_pick
    it = np.array([5, 6, 7, 8], dtype=np.int64)
    assert best_pick(np.array([1.0, 3.0, 3.0, 2.0]), it) == 1        # ties across walkers: the lowest index
    assert best_pick(np.array([0.0, -0.0, 0.0, -1.0]), it) == 0 and best_pick(np.array([-0.0, 0.0, 0.0, -1.0]), it) == 0
    assert best_pick(np.array([9.0, 1.0, 2.0, 2.0]), np.array([-1, 3, -1, 4])) == 3      # walkers holding nothing are passed over
    assert best_pick(np.array([9.0, 2.0, 9.0, 2.0]), np.array([-1, 3, -1, 4])) == 1
    assert best_pick(np.array([-np.inf, -np.inf]), np.array([-1, 2])) == 1 and best_pick(np.array([-np.inf, -np.inf]), np.array([1, 2])) == 0
    assert best_pick(np.array([np.inf, 1.0, np.inf]), np.array([-1, 0, 9])) == 2
    assert best_pick(np.array([7.0, 7.0]), np.array([-1, -1])) == -1 and best_pick(np.zeros(0), np.zeros(0, dtype=np.int64)) == -1      # nothing held at all


def test_best_on_crafted_buffers_reads_one_row_per_plane_and_never_raises():
    from ptmcmcsampler_amd.engine import PTEngine

    class T(object):                                                 # a device tensor's surface as best() uses it
        reads = []

        def __init__(self, a, name):
            self.a, self.name, self.shape = np.asarray(a), name, np.shape(a)

        def __getitem__(self, idx):
            return T(self.a[idx], "%s%r" % (self.name, idx))

        def cpu(self):
            T.reads.append(self.name)
            return self

        def numpy(self):
            return self.a

    W, d = 4, 3
    e = PTEngine.__new__(PTEngine)
    e.iter, e.cov_update, e.owns_cold, e._ring, e.W = 30, 40, True, [], W
    e._temps_mh = np.array([2.0])
    e._ring_reader("best", True, 4, 0, lambda eng, lo, hi, n: None)
    rows = np.arange(2 * W * d, dtype=np.float64).reshape(2, W, d)
    val = np.zeros((2, W, 3))
    iters = np.full((2, W), -1, dtype=np.int64)
    e.t = dict(best=T(rows, "rows"), best_val=T(val, "val"), best_iters=T(iters, "iters"))
    out = e.best()
    assert T.reads == ["val", "iters"]                               # nothing held: no row is read
    assert out["iter_map"] == out["iter_ml"] == out["walker_map"] == out["walker_ml"] == -1
    for k in ("lnprob_map", "lnlike_map", "lp_map", "lnprob_ml", "lnlike_ml", "lp_ml"):
        assert np.isnan(out[k]), k
    assert out["x_map"].shape == out["x_ml"].shape == (d,) and np.isnan(out["x_map"]).all() and np.isnan(out["x_ml"]).all()
    assert out["first_iter"] == 5 and out["last_iter"] == 30 and out["nwalkers"] == W and "x" not in out
    val[0, :, 0], val[0, :, 1], val[0, :, 2] = [9.0, 2.5, 2.5, 1.0], [4.0, 3.0, 3.0, 1.0], [7.0, 1.0, 1.0, 0.5]
    val[1, :, 0], val[1, :, 1], val[1, :, 2] = [1.0, 3.0, 8.0, 8.0], [1.0, 3.0, 8.0, 8.0], [0.5, 1.0, -1.0, -2.0]
    iters[0], iters[1] = [-1, 12, 9, 30], [20, 21, 22, 6]
    T.reads = []
    out = e.best(per_walker=True)
    assert T.reads[:4] == ["val", "iters", "rows(0, 1)", "rows(1, 2)"]      # ONE row per plane, then per_walker's whole buffer
    assert out["walker_map"] == 1 and out["iter_map"] == 12 and out["lnprob_map"] == 2.5 and out["lnlike_map"] == 3.0 and out["lp_map"] == 1.0
    assert out["walker_ml"] == 2 and out["iter_ml"] == 22 and out["lnlike_ml"] == 8.0 and out["lp_ml"] == -1.0
    assert out["lnprob_ml"] == (1.0 / 2.0) * 8.0 + -1.0
    assert np.array_equal(out["x_map"], rows[0, 1]) and np.array_equal(out["x_ml"], rows[1, 2])
    assert np.array_equal(out["x"], rows) and np.array_equal(out["val"], val) and np.array_equal(out["iters"], iters)
    assert sorted(out) == sorted(["x_map", "lnprob_map", "lnlike_map", "lp_map", "iter_map", "walker_map", "x_ml", "lnlike_ml", "lp_ml",
                                  "lnprob_ml", "iter_ml", "walker_ml", "first_iter", "last_iter", "nwalkers", "x", "val", "iters"])


# ---------------------------------------------------------------------- the sampler
def test_track_best_keywords_and_refusals(tmp_path):
    s = _sampler(tmp_path, "kw2")
    assert s._best_kw() == {}
    s.track_best = False
    assert s._best_kw() == {}
    s.track_best = True
    assert s._best_kw() == dict(best=True)
    s.track_best = {"from": 40}
    assert s._best_kw() == dict(best=True, best_from=40)
    s.track_best = {}
    assert s._best_kw() == dict(best=True)
    for bad in ({"first": 3}, 5, "yes", (1,)):
        s.track_best = bad
        with pytest.raises(ValueError, match="track_best is True or"):
            s._best_kw()


def test_a_replayed_resume_names_the_checkpoint(tmp_path):
    s = _sampler(tmp_path, "replay", resume=True, checkpoint=False)
    os.makedirs(s.outDir, exist_ok=True)
    np.savetxt(os.path.join(s.outDir, "chain_1.txt"), np.zeros((1, 3 + 4)))      # a chain file and no device checkpoint
    s.track_best = True
    with pytest.raises(NotImplementedError, match="track_best.*checkpoint=True"):
        s.sample(np.zeros(3), 10, isave=10, thin=1)


def test_set_after_the_engine_is_built_is_refused(tmp_path):
    class Built:                                                     # an engine that was built without any stage
        pairs_spec = hist_spec = samples_spec = None
        adapt_on = evidence_on = diag_on = best_on = False

    s = _sampler(tmp_path, "late")
    s.engine = Built()
    s.track_best = {"from": 10}
    with pytest.raises(ValueError, match="track_best was set after the engine was built"):
        s.writeOutput(0)
