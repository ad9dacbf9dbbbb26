"""The persistent SCAM kernel's two claim counters on the GPU (mh_steps_kernel with PERS, ptmi_mh.inc.h; the rule is restated in
tests/test_unit_claims.py): a block hands out its cold and its hot claims from a counter each, a wave prefers one list and falls back to
the other.  Which wave serves a unit changes no result, so every case is held to the CPU oracle bit for bit (PTMCMCSampler.py:499-503,
605-697, 820-876): X, lnL, lp, nacc, nswap, the AM rows and flags of the current covariance period, cov.  Pooled covariance,
am_mode "rle", swaps every 10 iterations that move the cold chain between a walker's units, three covariance epochs in 60 iterations;
with two blocks (the test hook PTMI_ULDS_PERS = 2, so that a block has more units than waves) and with the default grid.

The shapes are the smallest that reach every branch of the claim: an empty hot list, a cold prefix that ends inside a row of eight,
fewer claims than preferring waves on either list, a block without units, ncold = 0.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import pytest

from test_unit_walk_gpu import _run, mods  # noqa: F401  (mods is a fixture)

gpu = pytest.mark.gpu
_BLOCKS = [2, 1]                                                             # PTMI_ULDS_PERS: two blocks; 1 = the default grid


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
@pytest.mark.parametrize("nt,W", [(16, 25), (32, 25), (32, 3), (64, 1)])
def test_cold_and_hot_lists_of_every_length(mods, monkeypatch, nt, W, blocks):
    """ndim 100, flat prior.  (16, 25): every unit is cold, the hot list is empty from the start.  (32, 25): at two blocks, block 0 has
    16 cold claims and block 1 has 9 -- the prefix ends inside a row of eight.  (32, 3): block 0 has 3 cold and 3 hot claims, fewer than
    preferring waves on either side, and block 1 has no unit at all.  (64, 1): one cold unit and three hot ones."""
    _run(mods, monkeypatch, blocks, 100, nt, W)


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
@pytest.mark.parametrize("d,nt,box", [(100, 48, True), (99, 32, False)])
def test_the_other_persistent_instantiations(mods, monkeypatch, d, nt, box, blocks):
    """The box prior at the exact shape with an odd count of hot units per walker, and ndim 99 in the shape (4, 26)."""
    _run(mods, monkeypatch, blocks, d, nt, 25, box=box)


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
@pytest.mark.parametrize("how", ["ranks", "hot_block"])
def test_no_cold_list(mods, monkeypatch, how, blocks):
    """ncold = 0: 24 ranks do not fill whole units; a hot block of a sharded ladder has no AM buffer (and cannot swap on its own)."""
    if how == "ranks":
        _run(mods, monkeypatch, blocks, 100, 24, 25)
    else:
        g, o = _run(mods, monkeypatch, blocks, 100, 32, 25, tskip=0, ntemps_global=64, temp0=32, am_mode="auto")
        assert not g.owns_cold


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
def test_the_rolled_tail_pass_at_every_claimed_unit(mods, monkeypatch, blocks):
    """Launches of 7 steps (swaps every 7, covariance epochs every 21 iterations): a full pass and a rolled pass of three steps."""
    _run(mods, monkeypatch, blocks, 100, 32, 25, n=63, tskip=7, cov_update=21)
