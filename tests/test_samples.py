"""Thinned posterior samples of every cold chain, kept on the device (csrc/ptmi_samples.hip, include/ptmi.h ptmi_samples_attach /
ptmi_samples_take; ``PTEngine.with_stages(samples=64)``, ``PTSampler.posterior_samples``, ptmcmcsampler_amd/samples.py) -- what can be
checked without a GPU: the C ABI carries the two entry points to the letter, the stage is opt-in, the spec and its refusals before a
library is loaded, the snapshot schedule's invariants over a seeded random sweep, the flat view, and the sampler's refusals.
The runs themselves: tests/test_samples_gpu.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ptmcmcsampler_amd.samples import SlotPlan, flat, samples_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_samples_attach", "ptmi_samples_take")


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
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_samples_\w+)\(([^;]*)\);", hdr)}
    assert decl == {
        "ptmi_samples_attach": "ptmi_handle h, double *rows /* dev [nslots][W][ndim], PARAMETER order, caller-owned */, "
                               "double *aux /* dev [nslots][W][2] (lnL, lp) or NULL */, int32_t nslots",
        "ptmi_samples_take": "ptmi_handle h, const int64_t *iters /* host [n], strictly ascending */, "
                             "const int32_t *slots /* host [n], distinct, 0 <= slot < nslots */, int32_t n"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS, s
        assert s in exported, s
    H = C.c_void_p
    assert L.ptmi_samples_attach.argtypes == [H, C.c_void_p, C.c_void_p, C.c_int32]
    assert L.ptmi_samples_take.argtypes == [H, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_samples.hip" for src in _build.deps())
    assert re.search(r'"ptmi_samples\.hip"\), os\.path\.join\(OBJ, "samples\.o"\), \[\]\)', inspect.getsource(_build.build))
    # ptmi_config and ptmi_buffers are what they were: the stage's state lives in the handle
    assert "samples" not in lib.BUFFER_FIELDS and not any("samples" in n for n, _ in lib.Config._fields_)


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTSampler.posterior_samples is None and PTSampler.samples is None
    assert _sampler(tmp_path, "default").posterior_samples is None
    sig = inspect.signature(PTEngine.with_stages).parameters
    for name in ("samples", "samples_from"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert name not in inspect.signature(PTEngine.__init__).parameters
        assert name not in inspect.signature(PTSampler.__init__).parameters
        assert name not in inspect.signature(PTSampler.sample).parameters
    assert "posterior_samples" not in inspect.signature(PTSampler.__init__).parameters
    assert "posterior_samples" not in inspect.signature(PTSampler.sample).parameters
    with pytest.raises(TypeError, match="samples"):                  # the plain constructors keep their parameters
        PTEngine(6, 1, 1, np.eye(6), samples=8)
    with pytest.raises(TypeError, match="posterior_samples"):
        _sampler(tmp_path, "kw", posterior_samples=8)


def test_spec_parsing_and_every_refusal():
    assert samples_spec(64) == (64, 1) and samples_spec(np.int32(7)) == (7, 1)
    assert samples_spec({"slots": 64, "every": 10}) == (64, 10) and samples_spec(dict(slots=1)) == (1, 1)
    assert samples_spec(65535) == (65535, 1)
    assert all(type(v) is int for v in samples_spec({"slots": np.int64(3), "every": np.int64(2)}))
    for bad in (0, -1, 65536, 2.0, "8", None, True, (4, 2), {"slots": 0}, {"slots": 65536}, {"slots": 4.5}, {"slots": None}, {"every": 3}):
        with pytest.raises(ValueError, match="slots"):
            samples_spec(bad)
    for bad in (0, -2, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="every"):
            samples_spec({"slots": 4, "every": bad})
    with pytest.raises(ValueError, match="'thin'"):
        samples_spec({"slots": 4, "thin": 2})


def test_refusals_fall_before_any_library_is_loaded(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    d = 4
    make = lambda **kw: PTEngine.with_stages(d, 1, 1, np.eye(d), **kw)      # noqa: E731
    for bad in (0, 65536, 2.5, {"slots": 0}):
        with pytest.raises(ValueError, match="slots"):
            make(samples=bad)
    with pytest.raises(ValueError, match="every"):
        make(samples={"slots": 4, "every": 0})
    with pytest.raises(ValueError, match="samples_from"):
        make(samples=8, samples_from=-1)
    with pytest.raises(ValueError, match="samples_from"):
        make(samples_from=5)                                         # goes with samples=
    for kw in (dict(samples=1), dict(samples={"slots": 64, "every": 10}, samples_from=0), dict(samples=8, hist=(0.0, 1.0, 8), diag=True)):
        with pytest.raises(AssertionError, match="library was loaded"):      # good specs: the constructor gets as far as loading the library
            make(**kw)


def _held_want(first, every, level, last):
    M = max(0, (last - first) // every)
    return [first + every * (1 << level) * j for j in range(1, (M >> level) + 1)]


def _check(plan, first, last):
    it, slots = plan.held()
    assert it.tolist() == _held_want(first, plan.every, plan.level, last)      # evenly spaced over the whole run so far
    assert len(set(slots.tolist())) == len(slots) <= plan.nslots
    assert (plan.slot_iter[slots] == it).all() and (np.delete(plan.slot_iter, slots) == -1).all()
    M = max(0, (last - first) // plan.every)
    assert len(it) == min(M, plan.nslots) if M <= plan.nslots else plan.nslots // 2 <= len(it) <= plan.nslots
    assert plan.stride == plan.every << plan.level


def test_slot_plan_invariants_over_a_random_sweep():
    rs = np.random.RandomState(19)
    deep = 0
    for trial in range(400):
        nslots, every, cu = int(rs.randint(1, 10)), int(rs.randint(1, 6)), int(rs.randint(2, 41))
        first, length = int(rs.randint(0, 3 * cu)), int(rs.randint(1, 12 * cu))
        # the engine's cuts: every covariance period ends a call, and random syncs fall inside the periods
        ends = sorted(set(range(cu, length, cu)) | set(rs.randint(1, length + 1, rs.randint(0, 6)).tolist()) | {length})
        a, b = SlotPlan(nslots, every), SlotPlan(nslots, every)
        content = {}                                                 # slot -> iteration, as the device buffer would hold it
        lo = 1
        for hi in ends:
            pairs = a.take(first, lo, hi)
            assert pairs == sorted(pairs) and len({s for _, s in pairs}) == len(pairs) == len({i for i, _ in pairs})      # one iteration per slot and call
            base = ((hi - 1) // cu) * cu
            for i, s in pairs:
                assert lo <= i <= hi and i > first and (i - first) % every == 0 and 0 <= s < nslots
                assert base < i <= base + cu                         # one period per call: what ptmi_samples_take asks for
                content[s] = i
            _check(a, first, hi)
            it, slots = a.held()
            assert [content[s] for s in slots.tolist()] == it.tolist()      # what was gathered is what is held
            lo = hi + 1
        # ... and period by period alone, without the syncs: the same state
        lo = 1
        for hi in sorted(set(range(cu, length, cu)) | {length}):
            b.take(first, lo, hi)
            lo = hi + 1
        assert a.level == b.level and np.array_equal(a.slot_iter, b.slot_iter)
        deep = max(deep, a.level)
    assert deep >= 5                                                 # the sweep reaches several decimations


def test_slot_plan_edge_cases():
    one = SlotPlan(1, 1)                                             # one slot: the last power of two
    for hi in range(1, 40):
        pairs = one.take(0, hi, hi)
        assert one.held()[0].tolist() == [1 << (hi.bit_length() - 1)]
        assert pairs == ([(hi, 0)] if hi & (hi - 1) == 0 else [])
    far = SlotPlan(3, 50)                                            # every beyond the covariance period: most calls take nothing
    got = [far.take(7, lo, lo + 19) for lo in range(1, 400, 20)]
    assert [p for p in got if p] == [[(57, 0)], [(107, 1)], [(157, 2)], [(207, 0)], [(307, 2)]]      # 207 found no room: 57 and 157 went
    assert far.level == 1 and far.held()[0].tolist() == [107, 207, 307]
    assert far.take(7, 401, 420) == [(407, 1)] and far.level == 2 and far.held()[0].tolist() == [207, 407]
    whole = SlotPlan(3, 50)
    assert whole.take(7, 1, 420) == [(207, 0), (407, 1)]             # the final assignment of one call: the others came and went
    assert whole.level == 2 and np.array_equal(whole.slot_iter, far.slot_iter)
    assert SlotPlan(4, 3).take(10, 1, 10) == [] and SlotPlan(4, 3).take(10, 11, 12) == []      # nothing at or before first


def test_a_failed_take_leaves_the_plan_where_the_reader_is(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    class Lib(object):
        rc, calls = 0, []

        def ptmi_samples_take(self, h, iters, slots, n):
            self.calls.append(([iters[i] for i in range(n)], [slots[i] for i in range(n)]))
            return self.rc

    def check(rc):
        if rc != 0:
            raise _lib.PtmiError("libptmi error %d" % rc)

    monkeypatch.setattr(_lib, "check", check)
    e = PTEngine.__new__(PTEngine)                                   # an engine that never saw its constructor, with what samples_sync reads
    e.iter, e.cov_update, e.owns_cold, e.h, e.lib = 9, 20, True, None, Lib()
    e._splan, e._ring = SlotPlan(3, 1), []
    e._ring_reader("samples", True, 0, None, PTEngine._samples_take)
    e.samples_sync(3)
    assert e.lib.calls == [([1, 2, 3], [0, 1, 2])] and e.samples_iter == 3
    level, slot_iter = e._splan.level, e._splan.slot_iter.copy()
    e.lib.rc = -1
    with pytest.raises(_lib.PtmiError):
        e.samples_sync(9)                                            # 4 and 8 find the buffer full: the plan moves two levels, then the call fails
    assert e.lib.calls[-1] == ([4, 8], [0, 1])
    assert e.samples_iter == 3 and e._splan.level == level and np.array_equal(e._splan.slot_iter, slot_iter)
    e.lib.rc = 0
    e.samples_sync(9)                                                # the same call again, and it is taken
    assert e.lib.calls[-1] == ([4, 8], [0, 1]) and e.samples_iter == 9 and e._splan.held()[0].tolist() == [4, 8] and e._splan.level == 2


def test_slot_plan_with_many_slots_places_without_scanning():
    plan = SlotPlan(65535, 1)                                        # the largest buffer, a candidate an iteration: a placement is a heap pop
    lo = 1
    for hi in range(1000, 140001, 1000):
        pairs = plan.take(0, lo, hi)
        assert len(pairs) == len({s for _, s in pairs})
        lo = hi + 1
    _check(plan, 0, 140000)
    assert plan.level == 2 and plan.held()[1].size == 35000


def test_flat():
    rs = np.random.RandomState(1)
    x, ll, lp = rs.randn(3, 4, 5), rs.randn(3, 4), rs.randn(3, 4)
    fx, flp, fll = flat(dict(x=x, lnlike=ll, lnprob=lp, iters=np.arange(3)))
    assert fx.shape == (12, 5) and flp.shape == fll.shape == (12,)
    assert np.array_equal(fx[5], x[1, 1]) and fll[5] == ll[1, 1] and flp[5] == lp[1, 1]
    fx, flp, fll = flat(dict(x=x[:0]))
    assert fx.shape == (0, 5) and flp is None and fll is None


def test_a_replayed_resume_names_the_checkpoint(tmp_path):
    s = _sampler(tmp_path, "replay", resume=True, checkpoint=False)
    os.makedirs(s.outDir, exist_ok=True)
    np.savetxt(os.path.join(s.outDir, "chain_1.txt"), np.zeros((1, 3 + 4)))      # a chain file and no device checkpoint
    s.posterior_samples = 16
    with pytest.raises(NotImplementedError, match="posterior_samples.*checkpoint=True"):
        s.sample(np.zeros(3), 10, isave=10, thin=1)


def test_set_after_the_engine_is_built_is_refused(tmp_path):
    class Built:                                                     # an engine that was built without any stage
        pairs_spec = hist_spec = samples_spec = None
        adapt_on = evidence_on = diag_on = False

    s = _sampler(tmp_path, "late")
    s.engine = Built()
    s.posterior_samples = {"slots": 8, "every": 2}
    with pytest.raises(ValueError, match="posterior_samples was set after the engine was built"):
        s.writeOutput(0)
