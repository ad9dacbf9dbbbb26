"""The four-lane SCAM draw pass with one iteration per lane (ScamBatch::QUAD, ptmi_mh.inc.h): lane j of a chain draws both
Philox slots of iteration it + j, so a pass serves four steps and a launch whose length is no multiple of four ends in a short
pass.  HIP against the CPU oracle bit for bit (PTMCMCSampler.py:605-622, 843-873) at the boundaries that pass creates: every
launch length mod 4, one run cut into launches of odd lengths against the same run in one piece, persistent blocks and a table
copy per block, a table per walker, the exact shape (ndim 100) and its neighbours, chain counts that are no multiple of 16.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import numpy as np
import pytest

from test_gpu_parity import _compare, _pair, assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

# no epoch and no swap inside the launches below: every g.run(n) is ONE launch of n steps
_KW = dict(weights=(20, 0, 0), cov_update=1000, burn=1000, tskip=0)


def _scam_pair(mods, d, nt, W, cov_mode="pooled", seed=11):
    return _pair(mods, d, nt, W, seed=seed, rs=d, cov_mode=cov_mode, cov0=np.eye(d) * 0.02, **_KW)


@pytest.mark.parametrize("pers", [512, 0])
@pytest.mark.parametrize("d", [100, 81, 99, 101, 104])
def test_every_launch_length_mod_four(mods, d, pers, monkeypatch):
    """Launches of 1, 2, 3, 4, 5, 7 and 101 steps in a row: every residue of the launch length and of its first iteration mod
    4; 4 x 37 = 148 chains (9.25 units of 16).  Compared after every launch."""
    orc, _lib, _ = mods
    monkeypatch.setenv("PTMI_ULDS_PERS", str(pers))
    g, o = _scam_pair(mods, d, 4, 37, seed=d + pers)
    for n in (1, 2, 3, 4, 5, 7, 101):
        g.run(n)
        o.run(n)
        flags, G, E = g.last_variant()
        assert not flags & _lib.VAR_STAGED and not flags & _lib.VAR_FULL and G == 4
        assert bool(flags & _lib.VAR_PERSISTENT) == (pers != 0)
        _compare(g, o, "scam d=%d pers=%d after %d steps " % (d, pers, g.iter))
    assert o.nacc.sum() > 0


@pytest.mark.parametrize("d", [100, 101])
def test_odd_launches_against_one_piece(mods, d):
    """One run of 123 iterations in one launch, and cut into launches of 3, 5, 7, 9, 11, 1 and 87 steps: the same bits, both
    equal to the oracle's.  70 walkers x 3 ranks = 210 chains."""
    g1, o = _scam_pair(mods, d, 3, 70, seed=7)
    g2, _ = _scam_pair(mods, d, 3, 70, seed=7)
    g1.run(123)
    for n in (3, 5, 7, 9, 11, 1, 87):
        g2.run(n)
    o.run(123)
    _compare(g1, o, "one piece d=%d " % d)
    _compare(g2, o, "pieces d=%d " % d)
    for name in ("X", "lnL", "lp", "nacc", "jstat"):
        assert_same(g1.get(name), g2.get(name), "one piece vs pieces: " + name)


@pytest.mark.parametrize("d", [100, 99])
def test_table_per_walker(mods, d):
    """cov_mode "per_walker": a table per walker, the kernel with a table copy per block of 64 chains (no persistent blocks);
    5 walkers x 7 ranks = 35 chains, launches of every length mod 4."""
    orc, _lib, _ = mods
    g, o = _scam_pair(mods, d, 7, 5, cov_mode="per_walker", seed=3)
    for n in (5, 2, 7, 4, 1, 3, 66):
        g.run(n)
        o.run(n)
        flags, G, E = g.last_variant()
        assert not flags & _lib.VAR_PERSISTENT and G == 4
        _compare(g, o, "per-walker table d=%d after %d steps " % (d, g.iter))
    assert_same(g.get("Ut"), o.Ut, "Ut")
