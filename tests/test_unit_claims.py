"""The persistent SCAM kernel's two claim counters (mh_steps_kernel with PERS, ptmi_mh.inc.h, "the chains"), restated on the host.

A block owns the positions p(c) = 8 block + c % 8 + (c // 8) stride of the cold-first order, c = 0, 1, ...  p ascends in c, so the
block's cold claims (p < W: walker p's cold unit) are the prefix c < ncold and its hot claims are ncold <= c < ntot.  One counter in LDS
runs over the cold claims and one over the hot claims.  Of the two waves of a SIMD (waves j and j + 4 of the block) one prefers the cold
list and one the hot list; a wave takes from the other list only when its own is exhausted and leaves when both are.  The waves take their
first claims from the counters as well.  Without the cold-first order ncold = 0 and the claims come out as 0, 1, 2, ...

(The docstring of ``positions()`` in tests/test_unit_walk_gpu.py still says that a wave starts with the claim of its own number: that
sentence is stale since the first claims come from the counters; the mapping claim -> position -> unit it restates is unchanged and is
what this file checks the cold prefix against.)

Host only: no GPU, no library.  The GPU cases are in tests/test_unit_claims_gpu.py."""
import numpy as np
import pytest

from test_unit_walk_gpu import positions, unit_of

WPB = 8                                      # waves per block


def prefers_cold(wave):
    """The kernel's assignment: of a SIMD's two waves the older one (0-3 of the block) takes the cold list first."""
    return wave < WPB // 2


def counts(nt, W, nblocks, b, cold_first=True):
    """(ncold, ntot) of block b as the kernel forms them: the claims whose position lies below a limit are whole rows of eight, then
    what the last row holds of it."""
    nunits = (W * nt + 15) // 16
    stride = WPB * nblocks

    def below(lim):
        m = lim - WPB * b
        if m <= 0:
            return 0
        q = (m - 1) // stride
        return q * WPB + min(m - q * stride, WPB)

    return (below(min(W, nunits)) if cold_first else 0), below(nunits)


def serve(ncold, ntot, rs):
    """One block's launch: its eight waves claim in a random order (a wave that claims has finished its unit), each by the kernel's
    rule.  Returns the log of (wave, claim, cold claims left, hot claims left at that moment) in time order, the ending claims
    (claim == ntot) included."""
    ctr = [0, 0]                             # the two counters in LDS: cold claims handed out, hot claims handed out
    log = []
    active = list(range(WPB))
    while active:
        w = active[rs.randint(len(active))]
        left = (max(ncold - ctr[0], 0), max(ntot - ncold - ctr[1], 0))
        if prefers_cold(w):
            c = ctr[0]
            ctr[0] += 1
            if c >= ncold:
                c = ncold + ctr[1]
                ctr[1] += 1
        else:
            c = ncold + ctr[1]
            ctr[1] += 1
            if c >= ntot:
                c = ctr[0]
                ctr[0] += 1
                if c >= ncold:
                    c = ntot
        c = min(c, ntot)                     # (the first position past the end ends the walk, whichever claim named it)
        log.append((w, c, left[0], left[1]))
        if c >= ntot:
            active.remove(w)
    return log


def position(c, b, nblocks):
    return WPB * b + c % WPB + (c // WPB) * WPB * nblocks


@pytest.mark.parametrize("nblocks", [2, 256])
@pytest.mark.parametrize("W", [1, 2, 3, 25, 4096])
@pytest.mark.parametrize("nt", [16, 32, 48, 64])
def test_two_counters_hand_out_every_position_once_and_keep_the_preference(nt, W, nblocks):
    rs = np.random.RandomState(1000 * nt + 7 * W + nblocks)
    nunits = W * nt // 16
    slot_of = np.argsort(rs.rand(W, nt), axis=1).astype(np.int32)
    is_cold = np.zeros(nunits, dtype=bool)
    is_cold[np.arange(W) * (nt // 16) + (slot_of[:, 0] >> 4)] = True
    ref = positions(nt, W, nblocks)
    handed = []
    for b in range(nblocks):
        ncold, ntot = counts(nt, W, nblocks, b)
        # the prefix agrees with the restated walk: as many claims as the block has positions, the cold ones first and only they
        assert ntot == len(ref[b]) and ncold == int((ref[b] < W).sum())
        assert np.array_equal(ref[b], [position(c, b, nblocks) for c in range(ntot)])
        assert position(ntot, b, nblocks) >= nunits, "the ending claim names a position past the end"
        units = unit_of(ref[b], nt, W, slot_of)
        assert is_cold[units[:ncold]].all() and not is_cold[units[ncold:]].any()
        log = serve(ncold, ntot, rs)
        got = [c for _, c, _, _ in log if c < ntot]
        assert sorted(got) == list(range(ntot)), "every claim of the block exactly once"
        assert sum(c >= ntot for _, c, _, _ in log) == WPB, "every wave leaves once, and only when both lists are exhausted"
        for w, c, cold_left, hot_left in log:
            if c >= ntot:
                assert cold_left == 0 and hot_left == 0
            elif (c < ncold) != prefers_cold(w):
                assert (cold_left if prefers_cold(w) else hot_left) == 0, "a claim of the other list while the wave's own had one"
        handed += [position(c, b, nblocks) for c in got]
    assert sorted(handed) == list(range(nunits)), "every position of the launch exactly once"


@pytest.mark.parametrize("nblocks", [2, 256])
@pytest.mark.parametrize("W", [1, 2, 3, 25, 4096])
@pytest.mark.parametrize("nt", [16, 32, 48, 64])
def test_without_the_cold_first_order_the_claims_come_out_in_order(nt, W, nblocks):
    """ncold = 0 (no AM buffer, a hot block of a sharded ladder, ranks that do not fill whole units): whichever wave claims, the block's
    claims are served 0, 1, 2, ... as with one counter."""
    rs = np.random.RandomState(nt + W + nblocks)
    ref = positions(nt, W, nblocks)
    for b in range(nblocks):
        ncold, ntot = counts(nt, W, nblocks, b, cold_first=False)
        assert ncold == 0 and ntot == len(ref[b])
        log = serve(ncold, ntot, rs)
        assert [c for _, c, _, _ in log if c < ntot] == list(range(ntot))
