"""The software-pipelined direction row of the persistent exact-shape SCAM kernel (mh_steps_kernel, PIPE, ptmi_mh.inc.h): a full pass
of four steps runs as straight-line code, the table row of step s + 1 is requested behind the products of step s, and a short last
pass (launch length no multiple of four) keeps the rolled loop.  HIP against the CPU oracle bit for bit (PTMCMCSampler.py:605-622,
843-873, 327-328) at the seams of that structure: launches with no full pass, with full passes only and with both; passes that start
at every iteration residue mod 4; a covariance epoch between two launches (the table in LDS changes); flat and box prior; chain
counts that are no multiple of 16 and far fewer units than persistent waves; ndim 99 and 101 beside 100 (both run the general
shape (4, 26), whose kernels this change leaves alone).

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import numpy as np
import pytest

from test_gpu_parity import _compare, _pair, assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


def _kw(d, prior, W, nt, seed, **over):
    kw = dict(weights=(20, 0, 0), cov_update=1000, burn=1000, tskip=0, seed=seed, rs=d, cov_mode="pooled", cov0=np.eye(d) * 0.02)
    if prior == "box":
        kw.update(logp=("box", -0.4 * np.ones(d), 0.5 * np.ones(d)), p0=np.random.RandomState(seed).uniform(-0.1, 0.1, (W, nt, d)))
    kw.update(over)
    return kw


def _compare_all(g, o, what, _lib):
    """X, lnL, lp, nacc, jump statistics, the AM ring (_compare) and the ring's flags."""
    flags, G, E = g.last_variant()
    assert flags & _lib.VAR_PERSISTENT and flags & _lib.VAR_LDS_UT and not flags & _lib.VAR_FULL and G == 4
    _compare(g, o, what)
    if getattr(g, "am_rle", False):
        lo, hi = g.am_period()
        rows = np.arange(lo, hi + 1) % g.cov_update
        assert_same(g.get("AMflag")[:, rows] & 3, o.AMflag[:, rows] & 3, what + "AM flags")


@pytest.mark.parametrize("prior", ["flat", "box"])
@pytest.mark.parametrize("d", [100, 99, 101])
def test_launch_lengths_around_a_pass(mods, d, prior):
    """Launches of 1, 2, 3 (the rolled loop alone), 4, 8, 100 (full passes alone), 5 and 7 steps (both) in a row, compared after every
    launch; 4 x 37 = 148 chains: 9.25 units of 16, so most of the 2048 persistent waves have no unit and one unit is ragged."""
    orc, _lib, _ = mods
    g, o = _pair(mods, d, 4, 37, **_kw(d, prior, 37, 4, seed=3 * d))
    for n in (1, 2, 3, 4, 5, 7, 8, 100):
        g.run(n)
        o.run(n)
        _compare_all(g, o, "d=%d %s after %d steps: " % (d, prior, g.iter), _lib)
    assert tuple(g.last_variant()[1:]) == ((4, 25) if d == 100 else (4, 26))
    assert 0 < o.nacc.sum() < o.nacc.size * g.iter


@pytest.mark.parametrize("prior", ["flat", "box"])
@pytest.mark.parametrize("d", [100, 99])
def test_unequal_launches_against_one_piece(mods, d, prior):
    """One run of 69 iterations in one launch, and cut into launches of 4, 1, 4, 1, 4, 1, 4, 3, 8, 2, 5, 7, 12, 1 and 12 steps: full
    passes start at iterations 0, 5, 10, 15 (every residue mod 4) and later at 22, 32, 37, 44, 57: the same bits, each equal to its
    oracle's.  70 walkers x 3 ranks = 210 chains."""
    orc, _lib, _ = mods
    pieces = (4, 1, 4, 1, 4, 1, 4, 3, 8, 2, 5, 7, 12, 1, 12)
    total = sum(pieces)
    g1, o1 = _pair(mods, d, 3, 70, **_kw(d, prior, 70, 3, seed=7))
    g2, o2 = _pair(mods, d, 3, 70, **_kw(d, prior, 70, 3, seed=7))
    g1.run(total)
    o1.run(total)
    for n in pieces:
        g2.run(n)
        o2.run(n)                                   # (the ring's KEY flags follow the launches: an oracle per cut)
    _compare_all(g1, o1, "one piece d=%d %s: " % (d, prior), _lib)
    _compare_all(g2, o2, "pieces d=%d %s: " % (d, prior), _lib)
    for name in ("X", "lnL", "lp", "nacc", "jstat"):
        assert_same(g1.get(name), g2.get(name), "one piece vs pieces: " + name)


@pytest.mark.parametrize("prior", ["flat", "box"])
@pytest.mark.parametrize("d,nt,W,tskip", [(100, 16, 5, 6), (100, 32, 3, 0), (100, 5, 9, 0), (100, 5, 9, 7), (99, 4, 37, 0), (101, 4, 37, 10)])
def test_covariance_epoch_and_swaps_between_launches(mods, d, nt, W, tskip, prior):
    """Covariance epochs every 24 iterations (the pooled statistics of the AM ring, a new table in LDS for the launches behind them)
    inside runs of 24, 8, 100, 3, 17 and 40 iterations: without swaps the launches between two epochs are 24 steps long (six full
    passes) or what a run's end leaves of them; with swaps every 6 or 7 iterations a full pass and a short one.  Ranks in whole
    units per walker (16, 32): the cold-first walk, the cold chain changing its unit with the swaps; the others: ragged units.
    Chains, ring, flags, covariance and table after every run."""
    orc, _lib, _ = mods
    g, o = _pair(mods, d, nt, W, **_kw(d, prior, W, nt, seed=11 * d + nt, cov_update=24, tskip=tskip))
    for n in (24, 8, 100, 3, 17, 40):
        g.run(n)
        o.run(n)
        what = "epochs d=%d nt=%d %s it=%d: " % (d, nt, prior, g.iter)
        _compare_all(g, o, what, _lib)
        assert_same(g.get("cov"), o.cov, what + "cov")
        assert_same(g.get("Ut"), o.Ut, what + "Ut")
    assert g.eig_epochs >= 7 and (tskip == 0 or o.nswap.sum() > 0)
