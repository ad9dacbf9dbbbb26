"""Every shape, likelihood family and dispatch route of the fused step kernels, HIP vs oracle, bit for bit.

The cases and what ``ptmi_last_mh_variant`` must report for each are tests/test_step_variants.py's (one table for both files; its
ledger keeps the table complete).  Every case runs the same recipe -- an initial covariance wide enough for proposals to be refused,
three launches of 41, 3 and 26 iterations over three covariance epochs, DE activation and ten swap iterations -- and asserts on the
oracle's run what keeps it from passing vacuously (acceptance shares, refusals by the prior, diverged per-walker tables, accepted AM
and proposed DE jumps, accepted swaps).
Run on an MI355X: ``python -m pytest tests -m gpu``."""
import numpy as np
import pytest

from test_gpu_parity import _compare, _pair, assert_same, mods  # noqa: F401  (mods is a fixture)
from test_step_variants import CASES, LAUNCHES, box_in_lds, case_id, case_setup, expected_flags, oracle_conditions

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_step_variant(mods, case, monkeypatch):
    orc, _lib, _ = mods
    d, nt, W, kw, env = case_setup(case)
    for name in ("PTMI_ULDS_PERS", "PTMI_NO_PC"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    g, o = _pair(mods, d, nt, W, **dict(kw))
    what = case_id(case) + " "
    for n in LAUNCHES:
        g.run(n)
        o.run(n)
        _compare(g, o, what + "it=%d " % g.iter)
        flags, G, E = g.last_variant()
        assert (G, E) == case.shape, what
    assert_same(g.get("cov"), o.cov, what + "cov")
    assert_same(g.get("Ut"), o.Ut, what + "Ut")
    assert_same(g.get("S"), o.S, what + "S")
    # the instantiation that ran the last launch (DE is on): the route the case is in the table for
    must, must_not = expected_flags(case)
    box = _lib.VAR_LDS_BOX if box_in_lds(case) else 0
    assert flags & (must | must_not | _lib.VAR_LDS_BOX) == must | box, "%sflags 0x%x: wants 0x%x set, 0x%x clear" % (what, flags, must | box, must_not)
    shares = oracle_conditions(case, o, kw)
    print(what, "flags 0x%x" % flags, " ".join("%s %.2f" % kv for kv in sorted(shares.items())))
    if case.prior == "box":
        # the same case under the flat prior ends somewhere else: the prior did refuse proposals
        fkw = {k: v for k, v in kw.items() if k not in ("cov0", "p0", "logp")}
        f = orc.OracleEngine(d, nt, W, kw["cov0"], **fkw)
        f.init_state(kw["p0"])
        f.run(sum(LAUNCHES))
        assert not np.array_equal(f.X, o.X), what
