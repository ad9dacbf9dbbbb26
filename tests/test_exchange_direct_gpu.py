"""The sharded form of the swap, piece by piece on one GPU and one thread: R engines, each a block of ``nt`` ranks of one ladder
(``ntemps_global = R nt, temp0 = r nt``), call ptmi_swap_gather_lnl, ptmi_swap_sweep_blocks, ptmi_exchange_pack, ptmi_exchange_multihop,
ptmi_exchange_apply and ptmi_swap_write_am in turn; the transport between them is done by hand (``recv_r[q] = send_q[r]``).  No
ThreadComm, no MH step: every epoch's map, tables, counters and multi-hop flag are compared with the whole-ladder oracle and with the
NumPy restatement of tests/test_swap_routes.py -- the flag EXACTLY, at every epoch -- on the fused kernel, the two-kernel form and, at
3 x 803 ranks, the direct stores with the standalone scan (exchange_multihop_kernel).

Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)
from test_swap_routes import (SWL_DIRECT, SWL_FUSED, SWL_LDS, generic_lnl, geometric_ladder, model_lds, model_route, multihop,
                              place_decisions, ptswap)

pytestmark = pytest.mark.gpu
POISON = -7.25e300
D = 4


class Blocks(object):
    """R block engines and the whole-ladder oracle, from the same initial state."""

    def __init__(self, mods, R, nt, W, swap_mode="sweep", carry="all"):
        import torch
        orc, _lib, PTEngine = mods
        self.orc, self._lib, self.torch = orc, _lib, torch
        self.R, self.nt, self.W, self.ntg, self.carry = R, nt, W, R * nt, carry
        self.ladder = geometric_ladder(self.ntg)
        kw = dict(ladder=self.ladder, weights=(20, 20, 0), cov_update=16, burn=1000, tskip=1, seed=11 * R + nt + W, cov_mode="pooled",
                  swap_mode=swap_mode)
        cov0 = np.eye(D) * 0.01
        p0 = np.random.RandomState(R * nt + W).randn(W, self.ntg, D) * 0.3
        self.o = orc.OracleEngine(D, self.ntg, W, cov0, **kw)
        self.o.init_state(p0)
        self.aux = np.zeros((W, 16, 2))
        self.aux[:, 0, 0], self.aux[:, 0, 1] = self.o.by_temp(self.o.lnL)[:, 0], self.o.by_temp(self.o.lp)[:, 0]
        self.eng = []
        for r in range(R):
            e = PTEngine(D, nt, W, cov0, ntemps_global=self.ntg, temp0=r * nt, keep_lnl=True, **kw)
            e.init_state(p0[:, r * nt:(r + 1) * nt])
            assert e.last_swap_launch() == (0, 0, 0, 0)
            self.eng.append(e)
        dev = self.eng[0].device
        self.parts = torch.zeros((R, W, nt), dtype=torch.float64, device=dev)
        self.maps = [torch.zeros((W, self.ntg), dtype=torch.int32, device=dev) for _ in range(R)]
        self.send = [torch.zeros((R, W, D + 2), dtype=torch.float64, device=dev) for _ in range(R)]
        self.recv = [torch.zeros((R, W, D + 2), dtype=torch.float64, device=dev) for _ in range(R)]
        self.flags_seen, self.launch = set(), None

    def _by_slot(self, slot_of, by_pos):
        out = np.empty(by_pos.shape)
        np.put_along_axis(out, slot_of.astype(np.int64), by_pos, 1)
        return out

    def epoch(self, it, lnl_pos, u=None, pack_map=None, what=""):
        """One swap epoch with the likelihoods ``lnl_pos[W][ntg]`` (by position) and, if given, the pair uniforms ``u[W][ntg - 1]``
        instead of the Philox ones.  Returns (the oracle's map, the flag, written segments per block [R][R][W])."""
        torch, o, R, nt, W = self.torch, self.o, self.R, self.nt, self.W
        rp = ud = None
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            rp = self.orc.make_replay(np.ones(u.size, np.uint8), np.ascontiguousarray(u[:, ::-1]).ravel(), np.zeros(u.size, np.int64))
            ud = torch.from_numpy(u).to(self.eng[0].device)
        o.lnL[...] = self._by_slot(o.slot_of, lnl_pos)
        before = o.nswap.copy()
        m = o.swap(it, replay0=C.byref(rp[0]) if rp else None)
        accepted = (o.nswap - before).astype(np.int64)
        self.aux[:, it % 16, 0], self.aux[:, it % 16, 1] = o.by_temp(o.lnL)[:, 0], o.by_temp(o.lp)[:, 0]
        want_flag = multihop(m, nt)
        for r, e in enumerate(self.eng):
            e.put("lnL", self._by_slot(e.get("slot_of"), lnl_pos[:, r * nt:(r + 1) * nt]))
            e.gather_lnl(self.parts[r])
        flags, written = [], []
        for r, e in enumerate(self.eng):
            self._lib.check(e.lib.ptmi_test_replay(e.h, C.c_void_p(ud.data_ptr()) if ud is not None else None, None))
            try:
                e.sweep_blocks(it, self.parts, self.maps[r])
            finally:
                self._lib.check(e.lib.ptmi_test_replay(e.h, None, None))
            self.launch = e.last_swap_launch()
            self.send[r].fill_(POISON)
            e.exchange_pack(self.maps[r] if pack_map is None else pack_map, self.send[r])
            flags.append(e.exchange_multihop())
        if pack_map is not None:
            return m, flags, None
        for r, e in enumerate(self.eng):
            e.sync()
            assert np.array_equal(self.maps[r].cpu().numpy(), m), "%s: the map of block %d is not the oracle's" % (what, r)
            written.append((self.send[r] != POISON).any(dim=2).cpu().numpy())           # [q][w]
        written = np.stack(written)                                                     # [r][q][w]
        assert flags == [want_flag] * R, "%s epoch %d: multi-hop flags %r, the map says %r" % (what, it, flags, want_flag)
        self.flags_seen.add(want_flag)
        # a walker sends at most two rows from a block, never to the block itself, and only whole segments that are filled
        assert written.sum(axis=1).max() <= 2 and not written[np.arange(R), np.arange(R)].any(), what
        # every accepted edge pair sends the state it displaces one block up, and the carried state down: one row for every edge it
        # crosses unless it crosses several (which is what the flag says)
        edges = accepted[:, nt - 1:self.ntg - 1:nt].sum()
        if want_flag:
            assert edges < written.sum() < 2 * edges, (what, it, written.sum(), edges)
        else:
            assert written.sum() == 2 * edges, (what, it, written.sum(), edges)
            far = np.abs(np.arange(R)[:, None] - np.arange(R)[None, :]) > 1
            assert not written[far].any(), "%s: a row sent beyond a neighbouring block with the flag at 0" % what
        for r, e in enumerate(self.eng):
            if self.carry == "neighbours" and not want_flag:                            # only the two edge segments travel
                self.recv[r].fill_(POISON)
                for q in (r - 1, r + 1):
                    if 0 <= q < R:
                        self.recv[r][q].copy_(self.send[q][r])
            else:
                for q in range(R):
                    self.recv[r][q].copy_(self.send[q][r])
            e.exchange_apply(self.recv[r])
            e.write_am(it)
            e.iter = it
        self.compare(what + " epoch %d" % it)
        return m, want_flag, written

    def compare(self, what):
        o, nt = self.o, self.nt
        for r, e in enumerate(self.eng):
            e.sync()
            sl = slice(r * nt, (r + 1) * nt)
            assert e.exchange_violations() == 0, what
            so, to = e.get("slot_of").astype(np.int64), e.get("temp_of").astype(np.int64)
            assert np.array_equal(np.sort(so, axis=1), np.tile(np.arange(nt), (self.W, 1))), what + ": slot_of is no permutation"
            assert np.array_equal(np.take_along_axis(to, so, 1), np.tile(np.arange(nt), (self.W, 1))), what + ": temp_of is not its inverse"
            for name in ("X", "lnL", "lp"):
                assert_same(e.by_temp(name), o.by_temp(getattr(o, name))[:, sl], "%s block %d by_temp %s" % (what, r, name))
            ns = e.get("nswap")
            assert_same(ns[:, sl], o.nswap[:, sl], "%s block %d nswap" % (what, r))
            assert ns.sum() == ns[:, sl].sum(), what + ": credits outside the block's own columns"
        e0 = self.eng[0]
        assert_same(e0.get("AM"), o.AM, what + " AM")
        assert_same(e0.get("AMflag"), o.AMflag, what + " AMflag")
        assert_same(e0.get("AMaux"), self.aux, what + " AMaux")


def _expected_launch(fused, ntg):
    kernel, wpb = model_route(ntg, fused)
    return kernel, wpb, model_lds(kernel, wpb, ntg), int(kernel != SWL_DIRECT)


SHAPES = [(2, 3), (4, 3), (8, 3), (2, 70), (4, 70), (3, 803)]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("W", [5, 70])
@pytest.mark.parametrize("R,nt", SHAPES)
def test_exchange_pieces_against_the_whole_ladder_oracle(mods, R, nt, W, fused, monkeypatch):
    """Three epochs of generic likelihoods (about half of the pairs accept), run twice: with every segment transported, and with the
    two edge segments only (the rest poisoned) whenever the flag is 0 -- what a multi-GPU run does.  Both equal the oracle.  (3, 803):
    the direct stores and the standalone scan (kernel 3, ``hop_in_sweep == 0``), the plan kernel in 13 passes of 64 lanes, the last
    partial; three blocks let a state go from block 2 to block 0."""
    monkeypatch.setenv("PTMI_SWAP_FUSED", str(fused))
    want = _expected_launch(fused, R * nt)
    assert want[0] == ((SWL_FUSED if fused else SWL_LDS) if R * nt < 2409 else SWL_DIRECT) and want[3] == (want[0] != SWL_DIRECT)
    moved = 0
    for carry in ("all", "neighbours"):
        b = Blocks(mods, R, nt, W, carry=carry)
        rs = np.random.RandomState(R + nt + W)
        for it in (1, 2, 3):
            m, flag, written = b.epoch(it, generic_lnl(rs, b.ladder, W), what="R=%d nt=%d W=%d fused=%d %s" % (R, nt, W, fused, carry))
            if it == 1:
                print("R=%d nt=%d W=%d fused=%d %s: ptmi_last_swap_launch -> %r, flag %r" % (R, nt, W, fused, carry, b.launch, flag))
            assert b.launch == want, b.launch
            moved += written.sum()
    assert moved > 0, "no row ever crossed an edge: the test would prove nothing"


def _patterns(R, nt):
    """Accept patterns [*][ntg - 1], one carried state each: (what, pattern)."""
    ntg = R * nt
    top = ntg - 1                                                       # the top position of the hottest block

    def run(start, length):
        a = np.zeros(ntg - 1, dtype=bool)
        assert 0 <= start - length
        a[start - length:start] = True                                  # pairs start - 1 .. start - length: the state at `start` comes down `length` ranks
        return a

    out = [("no accept", np.zeros(ntg - 1, dtype=bool))]
    for start in (top, top - 1):
        for length in (nt - 1, nt, nt + 1, 2 * nt - 2, 2 * nt - 1, 2 * nt):
            out.append(("run of %d from %d" % (length, start), run(start, length)))
    out.append(("run to position 0 from the next block", run(2 * nt - 1, 2 * nt - 1)))
    out.append(("run to position 0 from the top", run(top, top)))
    alt = np.zeros(ntg - 1, dtype=bool)
    alt[2 * nt - 1 - 4:2 * nt - 1 + 5:2] = True                         # every second pair around the edge pair 2 nt - 1, which accepts
    alt[2 * nt - 1] = True
    out.append(("alternating across an edge", alt[:ntg - 1]))
    return out


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("R,nt", [(4, 3), (4, 70), (3, 803)])
def test_placed_decisions_pin_the_multihop_flag(mods, R, nt, fused, monkeypatch):
    """Decisions placed by hand (place_decisions + replayed uniforms): a run of accepts of nt - 1, nt, nt + 1, 2 nt - 2, 2 nt - 1 and
    2 nt pairs from a block's top position and from one below it carries a state across exactly one edge, to the neighbouring block's
    last position and one beyond it; runs that end at position 0; alternating decisions across an edge.  One pattern per epoch in one
    of eight walkers (the others accept nothing), so the epoch's flag is that pattern's; then all of them packed eight to an epoch.
    Flag and state must match for each; both flag values occur.  (3, 803) puts the same boundary to the standalone scan."""
    monkeypatch.setenv("PTMI_SWAP_FUSED", str(fused))
    W = 8
    b = Blocks(mods, R, nt, W, carry="neighbours")
    pats = _patterns(R, nt)
    it = 0
    singles = {}
    for i, (name, a) in enumerate(pats):
        acc = np.zeros((W, b.ntg - 1), dtype=bool)
        acc[i % W] = a
        L, u = place_decisions(acc, b.ladder)
        it += 1
        m, flag, _ = b.epoch(it, L, u=u, what="R=%d nt=%d fused=%d %s" % (R, nt, fused, name))
        assert np.array_equal(m, ptswap(b.ladder, L, u)[0]) and flag == multihop(m, nt)
        singles[name] = flag
    top = b.ntg - 1
    assert not singles["run of %d from %d" % (2 * nt - 1, top)] and singles["run of %d from %d" % (2 * nt, top)]
    assert not singles["run of %d from %d" % (2 * nt - 2, top - 1)] and singles["run of %d from %d" % (2 * nt - 1, top - 1)]
    assert singles["run to position 0 from the top"] and not singles["run to position 0 from the next block"]
    assert b.flags_seen == {False, True}
    for g0 in range(0, len(pats), W):
        acc = np.zeros((W, b.ntg - 1), dtype=bool)
        for j, (_, a) in enumerate(pats[g0:g0 + W]):
            acc[j] = a
        L, u = place_decisions(acc, b.ladder)
        it += 1
        b.epoch(it, L, u=u, what="R=%d nt=%d fused=%d packed %d" % (R, nt, fused, g0))
    print("placed R=%d nt=%d fused=%d: ptmi_last_swap_launch -> %r, flags %r" % (R, nt, fused, b.launch, singles))
    assert b.launch == _expected_launch(fused, b.ntg)


@pytest.mark.parametrize("R,nt", [(4, 3), (2, 70)])
def test_oddeven_blocks_cross_an_edge_only_with_the_edge_pair(mods, R, nt):
    """Odd/even mode on a sharded ladder (the masked sweep): for both parities the flag is 0, and rows cross an edge only in the
    epochs whose parity tries that edge's pair."""
    b = Blocks(mods, R, nt, 70, swap_mode="oddeven", carry="neighbours")
    rs = np.random.RandomState(nt)
    crossed = {0: 0, 1: 0}
    for it in (1, 2, 3, 4):
        parity = b.orc.swap_parity(it, 1)
        m, flag, written = b.epoch(it, generic_lnl(rs, b.ladder, 70), what="oddeven R=%d nt=%d" % (R, nt))
        assert flag is False
        for r in range(R - 1):                                            # the edge above block r: pair (r + 1) nt - 1
            n_edge = written[r, r + 1].sum() + written[r + 1, r].sum()
            if ((r + 1) * nt - 1) & 1 != parity:
                assert n_edge == 0, (it, r)
            crossed[parity] += n_edge
    tried = {((r + 1) * nt - 1) & 1 for r in range(R - 1)}
    assert all(crossed[p] > 0 for p in tried) and all(crossed[p] == 0 for p in (0, 1) if p not in tried)


def test_plan_detector_counts_a_map_that_is_not_the_sweeps(mods):
    """exchange_plan_kernel's violation counter: after a valid sweep on (4, 3) that moved rows across an edge, ptmi_exchange_pack is
    handed the identity -- a valid permutation, every entry inside [0, ntg), but not the map whose inverse the sweep stored: the
    blocks the sweep's inverse says a row leaves find no arrival to match it and must count.  The engines are thrown away."""
    import torch
    R, nt, W = 4, 3, 5
    b = Blocks(mods, R, nt, W)
    rs = np.random.RandomState(1)
    m, _, written = b.epoch(1, generic_lnl(rs, b.ladder, W), what="detector, valid epoch")
    assert written.sum() > 0 and all(e.exchange_violations() == 0 for e in b.eng)
    ident = torch.arange(b.ntg, dtype=torch.int32, device=b.eng[0].device).repeat(W, 1).contiguous()
    m2, _, _ = b.epoch(2, generic_lnl(rs, b.ladder, W), pack_map=ident, what="detector")
    leaves = [bool((m2[:, r * nt:(r + 1) * nt] // nt != r).any()) for r in range(R)]       # an arrival by the true map: as many rows leave
    assert any(leaves)
    for r, e in enumerate(b.eng):
        e.sync()
        assert (e.exchange_violations() > 0) == leaves[r], (r, leaves)
    del b
