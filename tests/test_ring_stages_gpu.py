"""The three stages that read the cold chains' AM ring a second time on ONE engine -- histograms, pair histograms, diagnostics sums
(``engine._RingReader``) -- against three engines that carry one stage each: the stages start in different covariance
periods, stand at different iterations inside one when the checkpoint is taken, and give the same counts and the same bits as alone,
before and behind a restore; the chains are the same bits on every engine; a checkpoint without a stage is refused by an engine with
it before anything is touched.  Both ring modes.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)
from test_hist_gpu import _cov0

pytestmark = pytest.mark.gpu

D, W, CU = 5, 6, 16
STAGES = {"hist": dict(hist=(-0.6, 0.6, 8), hist_from=0),
          "pairs": dict(pairs=({"params": [0, 2, 4]}, -0.6, 0.6, 8), pairs_from=CU),
          "diag": dict(diag=True, diag_from=5, diag_levels=4)}
REFUSED = {"hist": "the checkpoint carries no histogram: it was written by a run without hist=",
           "pairs": "the checkpoint carries no pair histograms of this shape: it was written by a run without pairs= (or with other pairs or bins)",
           "diag": "the checkpoint carries no diagnostics sums of this shape: it was written by a run without diag=True (or with other diag_levels)"}


def _results(g, it):
    return {"hist": g.hist_counts(it) if g.hist_spec is not None else None, "pairs": g.pairs_counts(it) if g.pairs_spec is not None else None,
            "diag": g.diag_moments(it) if g.diag_on else None}


def _assert_stage(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert_same(got[k], want[k], "%s: %s" % (what, k))           # the counts to the last one, the sums bit for bit


@pytest.mark.parametrize("am_mode", ["rows", "rle"])
def test_three_readers_on_one_engine_equal_three_engines_with_one_each(mods, am_mode):
    orc, _lib, PTEngine = mods
    kw = dict(weights=(20, 20, 20), cov_update=CU, burn=CU, tskip=5, seed=11, cov_mode="pooled", am_mode=am_mode)
    p0 = np.random.RandomState(3).randn(W, 2, D) * 0.1
    every = {k: v for s in STAGES.values() for k, v in s.items()}

    def make(**stages):
        g = PTEngine.with_stages(D, 2, W, _cov0(D), **stages, **kw)
        g.init_state(p0)
        return g

    a = make(**every)
    one = {name: make(**s) for name, s in STAGES.items()}
    end = 4 * CU
    for g in [a] + list(one.values()):
        g.run(3 * CU + 5)
    assert (a.hist_iter, a.pairs_iter, a.diag_iter) == (3 * CU,) * 3 and (a.hist_from, a.pairs_from, a.diag_from) == (0, CU, 5)
    # the three readers at three iterations of one period
    a.hist_sync(3 * CU + 2)
    a.diag_sync(3 * CU + 4)
    mid = a.pairs_counts()
    assert (a.hist_iter, a.pairs_iter, a.diag_iter) == (3 * CU + 2, 3 * CU + 5, 3 * CU + 4)
    assert (mid["counts"].sum((1, 2)) + mid["outside"] == W * (2 * CU + 5)).all()
    st = a.checkpoint()
    assert (st["hist_iter"], st["pairs_iter"], st["diag_iter"]) == (3 * CU + 2, 3 * CU + 5, 3 * CU + 4)
    b = make(**every)
    b.restore(st)
    assert (b.hist_iter, b.pairs_iter, b.diag_iter) == (3 * CU + 2, 3 * CU + 5, 3 * CU + 4) and b.iter == a.iter == 3 * CU + 5
    for g in [a, b] + list(one.values()):
        g.run(CU - 5)
    ra, rb = _results(a, end), _results(b, end)
    assert (ra["hist"]["counts"].sum(1) + ra["hist"]["under"] + ra["hist"]["over"] == W * end).all()
    assert int(ra["diag"]["n"]) == end - 5 and ra["hist"]["counts"].any() and ra["pairs"]["counts"].any()
    for name, g in one.items():
        alone = _results(g, end)[name]
        _assert_stage(ra[name], alone, "%s beside the others" % name)
        _assert_stage(rb[name], alone, "%s behind the restore" % name)
        _assert_stage(rb[name], ra[name], "%s restored against the original" % name)
    for name, g in [("restored", b)] + list(one.items()):
        assert_same(g.get("X"), a.get("X"), "X of the engine: " + name)      # the stages only read
    # a checkpoint without a stage: refused by an engine with it, in its own words, before anything is touched
    for name, g in one.items():
        other = one[{"hist": "pairs", "pairs": "diag", "diag": "hist"}[name]]
        x0, it0 = g.get("X").copy(), getattr(g, name + "_iter")
        with pytest.raises(ValueError) as err:
            g.restore(other.checkpoint())
        assert str(err.value) == REFUSED[name]
        assert_same(g.get("X"), x0, "X behind the refusal of " + name)
        assert getattr(g, name + "_iter") == it0 == end
