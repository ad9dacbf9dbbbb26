"""Every shape, likelihood family, layout, table form and prior of the fused gradient-jump kernels, HIP vs oracle, bit for bit.

The cases and what ``ptmi_last_gj_launch`` must report for each are tests/test_gj_variants.py's (one table for both files; its
ledger keeps the table complete).  Every case runs ``PTEngine`` and ``OracleEngine`` from the same start in uneven pieces -- 260
iterations over five covariance epochs, DE activation and 26 swap iterations; from 256-d on 90 iterations over four epochs, DE
activation and nine swaps, 2 x 2 chains --, and after each piece asserts that the launch was the layout the case is in the table
for (all layouts give the same bits: nothing else tells them apart), with the LDS levels, LDS bytes and chain slots worked out
there, then compares every buffer; at the end it asserts on the oracle's run what keeps the case from passing idle.

The oracle's run of the slowest case, 64x8-d512-dense-CHAIN-full-flat-both, takes 3.0 s on one CPU core (the other 512-d cases
1 to 2 s, the rest well below 1 s); the box cases run it a second time under the flat prior.  On an MI355X the slowest case takes
5 s with both engines, the 166 cases together one minute.
Run on an MI355X: ``python -m pytest tests -m gpu``."""
import pytest

from test_gj_variants import CASES, HOOKS, box_did_bind, case_id, case_setup, expected_launch, oracle_conditions
from test_gpu_parity import _compare, assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

FLAG_NAMES = ("DIAG", "GRP", "BOX_LDS", "ORDERED", "AM_AHEAD")


def _spell(_lib, layout):
    names = {getattr(_lib, "GJL_" + n): n for n in ("WAVE", "PAIR", "W16", "CHAIN")}
    return "|".join([names.get(layout & _lib.GJL_LAYOUT_MASK, "?")] + [n for n in FLAG_NAMES if layout & getattr(_lib, "GJL_" + n)])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gj_variant(mods, case, monkeypatch):
    orc, _lib, PTEngine = mods
    d, nt, W, cov0, p0, kw, env, pieces = case_setup(case)
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    g, o = PTEngine(d, nt, W, cov0, **kw), orc.OracleEngine(d, nt, W, cov0, **kw)
    assert o.lanes == case.shape[0] == _lib.lanes_for(d, grad=True)
    assert g.last_gj_launch() == (0, 0, 0, 0)
    g.init_state(p0)
    o.init_state(p0)
    what = case_id(case) + " "
    want = expected_launch(case)
    for n in pieces:
        g.run(n)
        o.run(n)
        at = what + "it=%d " % g.iter
        # first the kernel that ran (a wrong one that computes the right bits shows nowhere else), then what it computed
        flags, G, E = g.last_variant()
        assert flags & _lib.VAR_GRADJUMP and (G, E) == case.shape, at
        got = g.last_gj_launch()
        assert got == want, "%slaunched %s with %d levels, %d bytes of LDS, %d chain slots; the table says %s, %d, %d, %d" % (
            (at, _spell(_lib, got[0])) + got[1:] + (_spell(_lib, want[0]),) + want[1:])
        _compare(g, o, at)
        assert_same(g.get("gj"), o.gj, at + "gj")
        assert_same(g.get("Ut"), o.Ut, at + "Ut")
        assert_same(g.get("S"), o.S, at + "S")
    oracle_conditions(case, o, kw, sum(pieces))
    if case.prior == "box":
        box_did_bind(case, o, orc)
