"""The persistent SCAM kernel's walk over units of 16 chains (mh_steps_kernel with PERS, ptmi_mh.inc.h): the waves of a block claim
the block's units one after the other from a counter in LDS.  A wave only walks when the block has more units than waves, which at
test sizes needs fewer blocks than CUs: the test hook PTMI_ULDS_PERS = n > 1 caps the launch at n blocks of eight waves.  Every
GPU case runs with two blocks (16 waves) and with the default grid and is held to the CPU oracle bit for bit
(PTMCMCSampler.py:499-503, 605-697, 820-876); a host-only test restates the claim-to-position-to-unit mapping and checks that every
unit is claimed exactly once, cold units first and dealt evenly.

Run the GPU cases on the GPU box: ``python -m pytest tests -m gpu``."""
import numpy as np
import pytest

from test_gpu_parity import _compare, _pair, assert_same, mods  # noqa: F401  (mods is a fixture)

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the mapping, restated
def positions(nt, W, nblocks, wpb=8):
    """The positions of the walk that each block of the launch hands out, in the order of its claim counter: claim c of block b is
    position wpb b + c % wpb + (c // wpb) stride with stride = wpb nblocks, and the first claim whose position lies past the last unit
    ends the block's walk (mh_steps_kernel, "the chains").  A wave starts with the claim of its own number and takes the block's
    next claim whenever it has finished a unit."""
    nunits = (W * nt + 15) // 16
    stride = wpb * nblocks
    res = []
    for b in range(nblocks):
        c = np.arange((nunits // stride + 2) * wpb)
        upos = wpb * b + c % wpb + (c // wpb) * stride
        assert (np.diff(upos) > 0).all(), "ascending in c: nothing behind the first claim past the end"
        res.append(upos[upos < nunits])
    return res


def unit_of(upos, nt, W, slot_of, cold_first=True):
    """Position -> unit.  Cold-first order: position p < W is walker p's cold unit (the unit of ``slot_of[p][0]``), the walkers'
    other units follow walker by walker; else the plain order."""
    if not cold_first:
        return upos
    upw = nt // 16
    upw1 = max(upw - 1, 1)
    r = upos - W
    is_cold = upos < W
    wq = np.where(is_cold, upos, r // upw1)
    cq = slot_of[wq, 0] >> 4
    return wq * upw + np.where(is_cold, cq, (cq + 1 + r % upw1) % upw)


@pytest.mark.parametrize("nwaves", [16, 2048])
@pytest.mark.parametrize("W", [1, 2, 25, 4096])
@pytest.mark.parametrize("nt", [16, 32, 48, 64])
def test_the_walk_visits_every_unit_once_and_deals_the_cold_units_evenly(nt, W, nwaves):
    """Every unit is claimed exactly once; a block hands out its cold units before its hot ones; and the cold units are dealt evenly:
    the claims c, c + 8, ... that a wave would take at an even pace hold cold counts that differ by at most one over the whole
    launch."""
    rs = np.random.RandomState(nt + W + nwaves)
    slot_of = np.argsort(rs.rand(W, nt), axis=1).astype(np.int32)           # slot of every rank: a random permutation per walker
    nunits = W * nt // 16
    pos = positions(nt, W, nwaves // 8)
    units = [unit_of(p, nt, W, slot_of) for p in pos]
    assert np.array_equal(np.sort(np.concatenate(units)), np.arange(nunits)), "a permutation of the units"
    is_cold = np.zeros(nunits, dtype=bool)
    is_cold[np.arange(W) * (nt // 16) + (slot_of[:, 0] >> 4)] = True
    per_block = np.array([is_cold[u].sum() for u in units])
    per_slot = np.array([is_cold[u[j::8]].sum() for u in units for j in range(8)])
    assert per_block.sum() == W and per_slot.sum() == W
    assert per_slot.max() - per_slot.min() <= 1
    assert per_block.max() - per_block.min() <= 8                          # (eight such rows per block)
    for u, n in zip(units, per_block):
        assert is_cold[u[:n]].all() and not is_cold[u[n:]].any(), "a block's cold units come first"
    # the plain order (no AM buffer, a hot block of a sharded ladder, ranks that do not fill whole units)
    plain = np.concatenate([unit_of(p, nt, W, slot_of, cold_first=False) for p in pos])
    assert np.array_equal(np.sort(plain), np.arange(nunits))


# ---------------------------------------------------------------------------------------------- on the GPU
# pooled covariance, am_mode rle (the default of a pooled covariance), swaps every 10 iterations that move the cold chain between a
# walker's units, three covariance epochs inside the 60 iterations
_KW = dict(weights=(20, 0, 0), cov_mode="pooled", am_mode="rle", tskip=10, cov_update=20, burn=1000)
_BLOCKS = [2, 1]                                                             # PTMI_ULDS_PERS: two blocks; 1 = the default grid


def _run(mods, monkeypatch, blocks, d, nt, W, n=60, box=False, **over):
    orc, _lib, _ = mods
    monkeypatch.setenv("PTMI_ULDS_PERS", str(blocks))
    kw = dict(_KW, seed=1000 * d + 10 * nt + W, cov0=np.eye(d) * 0.02)
    kw.update(over)
    if box:
        kw.update(logp=("box", -0.4 * np.ones(d), 0.5 * np.ones(d)), p0=np.random.RandomState(d + nt).uniform(-0.1, 0.1, (W, nt, d)))
    g, o = _pair(mods, d, nt, W, rs=d + nt + W, **kw)
    g.run(n)
    o.run(n)
    flags, G, E = g.last_variant()
    assert flags & _lib.VAR_PERSISTENT and flags & _lib.VAR_LDS_UT and G == 4
    assert E == (25 if d == 100 else 26)
    what = "walk d=%d nt=%d W=%d blocks=%d " % (d, nt, W, blocks)
    _compare(g, o, what)
    if g.owns_cold:
        if getattr(g, "am_rle", False):
            lo, hi = g.am_period()                                           # as _compare's AM rows: the current covariance period
            rows = np.arange(lo, hi + 1) % g.cov_update
            assert_same(g.get("AMflag")[:, rows], o.AMflag[:, rows], what + "AMflag (current period)")
        assert_same(g.get("cov"), o.cov, what + "cov")
    return g, o


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
@pytest.mark.parametrize("nt", [16, 32, 48])
def test_exact_shape_flat_prior(mods, monkeypatch, nt, blocks):
    """ndim 100, flat prior: the software-pipelined kernel.  25 walkers of one, two and three units: at two blocks of eight waves a
    block hands out 12-13, 25 and 37-38 units, the last claims of a row of eight past the end for some waves and not for others; no
    hot units at all with 16 ranks, an odd count of them per walker with 48."""
    g, o = _run(mods, monkeypatch, blocks, 100, nt, 25)
    assert o.nacc.sum() > 0 and o.nswap[:, 0].sum() > 0      # steps were accepted, and the cold chain did change places


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
@pytest.mark.parametrize("d,box", [(100, True), (99, False), (101, False)])
def test_box_prior_and_the_inexact_shapes(mods, monkeypatch, d, box, blocks):
    """The persistent kernel's other instantiations: the box prior at the exact shape, and ndim 99 / 101 in the shape (4, 26)
    with its bounds checks."""
    _run(mods, monkeypatch, blocks, d, 32, 25, box=box)


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
def test_launch_lengths_that_are_no_multiple_of_four(mods, monkeypatch, blocks):
    """Swaps every 7 and covariance epochs every 21 iterations: launches of 7 steps, so the rolled tail pass of three steps runs
    at every unit of the walk."""
    _run(mods, monkeypatch, blocks, 100, 32, 25, n=63, tskip=7, cov_update=21)


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
def test_a_single_unit(mods, monkeypatch, blocks):
    """One walker of 16 ranks: one wave has one unit, every other wave none, and that wave's next claim is past the end."""
    _run(mods, monkeypatch, blocks, 100, 16, 1)


@gpu
@pytest.mark.parametrize("blocks", _BLOCKS)
@pytest.mark.parametrize("how", ["ranks", "hot_block"])
def test_the_plain_order_without_cold_first(mods, monkeypatch, how, blocks):
    """The cold-first order is off when a walker's ranks do not fill whole units (24 ranks) and in a block of a sharded ladder that
    does not hold rank 0 (temp0 = 32: no AM buffer; such a block cannot swap on its own, so tskip is 0): the waves then walk the
    units in their plain order."""
    if how == "ranks":
        _run(mods, monkeypatch, blocks, 100, 24, 25)
    else:
        g, o = _run(mods, monkeypatch, blocks, 100, 32, 25, tskip=0, ntemps_global=64, temp0=32, am_mode="auto")
        assert not g.owns_cold
