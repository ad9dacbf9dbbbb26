"""The stages that read the cold chains' AM ring a second time -- the histograms (``hist``), the pair histograms (``pairs``), the
diagnostics sums (``diag``) -- share one bookkeeping: which iterations a stage has taken, which call comes next, which calls are refused
(``engine._RingReader``).  Checked without a GPU and without the library: the refusals of ``PTEngine.<stage>_sync`` to the
letter, on an engine that never saw its constructor, and the reader itself with an update callable that only records its calls.  The
runs: tests/test_ring_stages_gpu.py."""
import types

import pytest

from ptmcmcsampler_amd import engine
from ptmcmcsampler_amd.engine import PTEngine

STAGES = ("hist", "pairs", "diag")
CU, FIRST = 8, 3

# the engine's messages as they stood before the stages shared their code, for hist_sync(it); the other stages say their own name
REACHED = "hist_sync(7): the engine has reached iteration 5; the ring's rows beyond it are the period before's"
LOST = ("hist_sync(20): iterations 4..16 are no longer in the ring (it holds the period after 16); every period must end through "
        "update_cov")


class FakeLib(object):
    """``ptmi_<stage>_update`` that only records its arguments behind the handle."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda h, *a: self.calls.append((name,) + a) or 0


def engine_stub(stage, at):
    """A PTEngine that never saw its constructor, with what ``<stage>_sync`` reads: the engine at iteration ``at``, every stage on from
    iteration FIRST and with nothing taken yet."""
    e = PTEngine.__new__(PTEngine)
    e.iter, e.cov_update, e.owns_cold, e.h, e.lib = at, CU, True, None, FakeLib()
    e.hist_spec = e.pairs_spec = ()
    e.diag_on = True
    if hasattr(PTEngine, "_ring_reader"):
        e._ring = []
        calls = {"hist": lambda g, lo, hi, n: g.lib.ptmi_hist_update(g.h, lo, hi), "pairs": lambda g, lo, hi, n: g.lib.ptmi_pairs_update(g.h, lo, hi),
                 "diag": lambda g, lo, hi, n: g.lib.ptmi_diag_update(g.h, lo, hi, n)}
        for s in STAGES:
            e._ring_reader(s, True, FIRST, None, calls[s])
    else:                                                             # an engine that keeps a stage's iterations in attributes of its own
        for s in STAGES:
            setattr(e, s + "_from", FIRST)
            setattr(e, s + "_iter", FIRST)
    return e


@pytest.mark.parametrize("stage", STAGES)
def test_the_engine_refuses_in_the_words_it_always_used(stage):
    e = engine_stub(stage, 5)
    sync = getattr(e, stage + "_sync")
    with pytest.raises(ValueError) as err:
        sync(7)                                                       # beyond the engine's iteration
    assert str(err.value) == REACHED.replace("hist", stage)
    assert e.lib.calls == [] and getattr(e, stage + "_iter") == FIRST
    sync(5)
    extra = (0,) if stage == "diag" else ()                           # n_done: nothing folded before
    assert e.lib.calls == [("ptmi_%s_update" % stage, FIRST + 1, 5) + extra] and getattr(e, stage + "_iter") == 5
    e = engine_stub(stage, 20)
    with pytest.raises(ValueError) as err:
        getattr(e, stage + "_sync")(20)                               # the period 9..16 was never taken
    assert str(err.value) == LOST.replace("hist", stage)
    assert e.lib.calls == [] and getattr(e, stage + "_iter") == FIRST


def test_a_stage_that_is_off_says_how_to_ask_for_it():
    e = engine_stub("hist", 5)
    e.hist_spec = e.pairs_spec = None
    e.diag_on = False
    e._ring = []
    for stage, msg in (("hist", "no histogram: PTEngine.with_stages(..., hist=(lo, hi, nbins))"),
                       ("pairs", "no pair histogram: PTEngine.with_stages(..., pairs=(pairs, lo, hi, nbins))"),
                       ("diag", "no diagnostics: PTEngine.with_stages(..., diag=True)")):
        with pytest.raises(ValueError) as err:
            getattr(e, stage + "_sync")(1)
        assert str(err.value) == msg


# ---------------------------------------------------------------------- the reader itself
def reader(stage, at):
    """A reader of ``stage``, an engine of three attributes that its calls get, and the list its update callable records (lo, hi, n_done) in."""
    calls = []
    eng = types.SimpleNamespace(iter=at, cov_update=CU, owns_cold=True)
    return engine._RingReader(stage, FIRST, lambda g, lo, hi, n: calls.append((lo, hi, n)) if g is eng else None), eng, calls


@pytest.mark.parametrize("stage", STAGES)
def test_the_reader_issues_every_iteration_once_and_in_one_period(stage):
    r, eng, calls = reader(stage, 7)
    assert (r.name, r.first, r.iter) == (stage, FIRST, FIRST)
    for it in (0, 1, FIRST):                                          # nothing up to `first`
        r.sync(eng, it)
    assert calls == [] and r.iter == FIRST
    r.sync(eng, 6)                                                    # inside the first period: (first + 1, it)
    assert calls == [(FIRST + 1, 6, 0)] and r.iter == 6
    r.sync(eng, 6)                                                    # taken already
    r.sync(eng, 4)
    assert len(calls) == 1 and r.iter == 6
    r.sync(eng, 7)                                                    # the second call: (iter + 1, it), n_done = iter - first
    assert calls[1:] == [(7, 7, 6 - FIRST)] and r.iter == 7
    with pytest.raises(ValueError) as err:
        r.sync(eng, 8)                                                # beyond the engine's iteration
    assert str(err.value) == "%s_sync(8): the engine has reached iteration 7; the ring's rows beyond it are the period before's" % stage
    assert len(calls) == 2 and r.iter == 7
    r.advance(eng, 8)                                                 # update_cov's call is not held against the engine's iteration
    assert calls[2:] == [(8, 8, 7 - FIRST)] and r.iter == 8
    eng.iter = 12
    r.sync(eng, 12)                                                   # the next period from its first iteration: base = 8 = iter
    assert calls[3:] == [(9, 12, 8 - FIRST)] and r.iter == 12
    eng.iter = 30
    for call in (r.sync, r.advance):
        with pytest.raises(ValueError) as err:
            call(eng, 30)                                             # 13..24 were never taken: a whole period was skipped
        assert str(err.value) == ("%s_sync(30): iterations 13..24 are no longer in the ring (it holds the period after 24); every period "
                                  "must end through update_cov" % stage)
        assert len(calls) == 4 and r.iter == 12
    r.sync(eng, 16)                                                   # a call is held against the reader's own period only
    assert calls[4:] == [(13, 16, 12 - FIRST)] and r.iter == 16


def test_the_literal_messages_come_out_of_the_reader():
    r, eng, calls = reader("hist", 5)
    with pytest.raises(ValueError) as err:
        r.sync(eng, 7)
    assert str(err.value) == REACHED
    eng.iter = 20
    with pytest.raises(ValueError) as err:
        r.sync(eng, 20)
    assert str(err.value) == LOST and calls == [] and r.iter == FIRST


def test_an_engine_without_a_cold_ring_skips_nothing():
    # temp0 != 0: update_cov returns at once and the C call does nothing, so no period can be missed (diag is refused on such an engine)
    r, eng, calls = reader("pairs", 40)
    eng.owns_cold = False
    r.sync(eng, 40)
    assert calls == [(FIRST + 1, 40, 0)] and r.iter == 40
