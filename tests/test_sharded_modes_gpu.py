"""The sharded ladder's mode matrix (tests/sharded_modes.py) on the device: one thread per temperature block on the one GPU
(thread_comm.ThreadComm), the HIP kernels behind every block, against the whole ladder on ``OracleEngine``, bit for bit -- chains by
temperature, counters, ``Ut`` / ``S`` on every block, the DE ring rolled by its head, and on the block that holds rank 0 the AM ring,
the running statistics and the covariance.

What it reaches that no sharded run did: a device factorization (``ptmi_eig_jacobi``, ``ptmi_eig_ql`` narrow and wide,
``ptmi_eig_sytrd``, the ROCm library's solver) queued on the owner's stream with the broadcast of its table right behind it
(``eig_lag = 0``), per-walker tables beyond 104-d (the owner makes its AM increments ahead of the launch from the ring it holds,
the other blocks hold none), parameter groups (one factorization per group, ``ngroups`` tables per walker broadcast) and groups with
gradient jumps.  "sytrd" and "hipsolver" are not restated by the oracle: a single ``PTEngine`` of the same configuration is held to
the oracle through the tables it made (test_device_tables_gpu.lockstep, its own 1e-12 on every table), the blocks to that engine and
to the oracle stepped with those tables, bit for bit.

Every case also states, on the oracle's run alone, that its blocks depend on what the owner broadcast
(sharded_modes.depends_on_the_broadcast).  ``pytest -s`` prints a line per case: the routes taken and those counts.

Run on the GPU box: ``python -m pytest tests -m gpu``."""
import json
import types

import numpy as np
import pytest

import sharded_modes as sm
from test_gpu_parity import _compare, assert_same, mods  # noqa: F401  (mods is a fixture)
from test_sharded_gpu import _check_blocks, _run_emulated_ladder
from thread_comm import ThreadComm

pytestmark = pytest.mark.gpu


class _Recorded(ThreadComm):
    """A ThreadComm that keeps the order of the transports a rank used: "n" the two neighbour links, "a" the all-to-all."""

    def __init__(self, world, rank):
        ThreadComm.__init__(self, world, rank)
        self.log = []

    def neighbour_exchange(self, send, recv):
        self.log.append("n")
        ThreadComm.neighbour_exchange(self, send, recv)

    def all_to_all(self, out, inp, out_splits=None, in_splits=None):
        self.log.append("a")
        ThreadComm.all_to_all(self, out, inp, out_splits, in_splits)


class _LosesS(_Recorded):
    """... whose broadcast of ``S`` (the one that follows the four-dimensional ``Ut``, ShardedPTEngine._bcast_table) never reaches
    the ranks beside the root: they take part in the collective and copy nothing."""

    def __init__(self, world, rank):
        _Recorded.__init__(self, world, rank)
        self.after_ut, self.lost = False, 0

    def broadcast(self, t):
        is_s, self.after_ut = self.after_ut and t.dim() == 3, t.dim() == 4
        if is_s and self.rank != 0:
            self._sync()
            self._sync()
            self.lost += 1
            return
        ThreadComm.broadcast(self, t)


def _single_engine_in_lockstep(mods, case, cov0, p0, kw):
    """A solver the oracle does not restate: one PTEngine with the whole ladder, held to the oracle through the tables it made."""
    from test_device_tables_gpu import TableTap, lockstep
    orc, _lib, PTEngine = mods
    g = PTEngine(case.d, sm.NTG, case.W, cov0, **kw)
    o = orc.OracleEngine(case.d, sm.NTG, case.W, cov0, **sm.oracle_kw(case, kw))
    g.init_state(p0)
    o.init_state(p0)
    marks = types.SimpleNamespace(Ut0=o.Ut.copy(), S0=o.S.copy())
    tap = TableTap(g)
    first = sm.first_table_in_force(case)
    used = lockstep(g, o, tap, first, "single engine, %s, to the first epoch" % case.name)
    marks.jstat_first = o.jstat.copy()
    used += lockstep(g, o, tap, case.n - first, "single engine, %s" % case.name)
    assert used >= 3 and g.eig_epochs >= 3
    g.mh_steps = type(g).mh_steps.__get__(g)
    _compare(g, o, "single engine vs oracle (%s): " % case.name)
    for name in ("cov", "Ut", "S"):
        assert_same(g.get(name), getattr(o, name), "single engine vs oracle (%s): %s" % (case.name, name))
    return g, o, marks


@pytest.mark.parametrize("name", list(sm.CASES))
def test_sharded_mode_equals_the_whole_ladder(mods, name):
    orc, _lib, PTEngine = mods
    case = sm.CASES[name]
    cov0, p0, kw = sm.inputs(case)
    d, ntb, nranks, n = case.d, case.ntb, case.nranks, case.n
    nswaps = n // kw["tskip"]
    single = None
    if case.hold == "oracle":
        ref, marks = sm.reference(case, orc)
    else:
        single, ref, marks = _single_engine_in_lockstep(mods, case, cov0, p0, kw)
    _, engines = _run_emulated_ladder(nranks, ntb, d, case.W, n, cov0, p0, kw, ref=ref, comm=_Recorded)
    # chains by temperature, counters, Ut / S on every block, AM and M2 on the owner's, every edge crossed, one transport count
    _check_blocks(ref, engines, ntb, nswaps, gj=sm.has_gj(case))
    routes = []
    for r, e in enumerate(engines):
        L, sl = e.local, slice(r * ntb, (r + 1) * ntb)
        what = "%s, block %d: " % (name, r)
        assert_same(np.roll(L.get("DE"), -L.de_head, axis=1), ref.DE, what + "DE ring")
        assert L.de_head == e.de_head and L.de_on
        if r == 0:
            assert_same(L.get("cov"), ref.cov, what + "cov")
            if L.am_rle:                                 # the ring keeps the current period's rows (test_gpu_parity._compare)
                lo, hi = L.am_period()
                rows = np.arange(lo, hi + 1) % L.cov_update
                assert_same(L.get("AM")[:, rows], ref.AM[:, rows], what + "AM (current period)")
        if single is not None:                           # the single engine of the same configuration, directly
            for nm in ("X", "lnL", "lp"):
                assert_same(L.by_temp(nm), single.by_temp(nm)[:, sl], what + nm + " vs the single engine")
            for nm in ("Ut", "S"):
                assert_same(L.get(nm), single.get(nm), what + nm + " vs the single engine")
            assert_same(L.get("jstat"), single.get("jstat")[:, sl], what + "jstat vs the single engine")
        # the route the case names really ran
        assert e.eig_lag == kw["eig_lag"] and L.eig_mode == kw["eig_mode"] and L.per_walker == (kw["cov_mode"] == "per_walker")
        assert L.ngr == len(kw.get("groups", [0])) and tuple(L.get("Ut").shape) == (case.W if L.per_walker else 1, L.ngr, d, d)
        assert (L.eig_epochs >= 3) if r == 0 else (L.eig_epochs == 0), what + "eig_epochs = %d" % L.eig_epochs
        assert (L.t["AM"] is not None) == (r == 0) and L.am_rle == (r == 0 and not L.per_walker)
        flags, G, E = L.last_variant()
        assert G == _lib.lanes_for(d, grad=sm.has_gj(case)), what + "lanes"
        if d > 104:
            assert G == 16 and flags & _lib.VAR_FULL, what + "not the 16-lane full-cycle kernel (AM increments ahead of the launch)"
        if sm.has_gj(case):
            assert flags & _lib.VAR_GRADJUMP, what + "no gradient-jump kernel"
        elif L.ngr > 1:
            assert flags & _lib.VAR_GROUPS, what + "no group kernel"
        # every rank took the same transport decision at every epoch
        log = "".join(e.comm.log)
        assert log == "".join(engines[0].comm.log), what + "transports %s against block 0's %s" % (log, "".join(engines[0].comm.log))
        assert log.count("n") == nswaps and e.neighbour_swaps == nswaps - log.count("a") and "aa" not in log and not log.startswith("a")
        routes.append(dict(variant=[hex(flags), G, E], eig_epochs=L.eig_epochs, neighbour_swaps=e.neighbour_swaps))
    if nranks == 2:
        assert engines[0].neighbour_swaps == nswaps          # two blocks have no one but each other
    counts = sm.depends_on_the_broadcast(case, ref, marks)
    print("\nsharded mode %s: %s" % (name, json.dumps(dict(blocks=routes, oracle=counts))))


@pytest.mark.parametrize("name", ["ql-per_walker-d130-lag0-wide", "groups-100+30-ql-pooled-d130-wide"])
def test_a_lost_broadcast_of_S_shows_on_the_device_blocks(mods, name):
    """The CPU leg's sensitivity test with the kernels behind the blocks, at the two widest cases: ``S`` never arrives beside the
    root, so the other blocks' step kernels scale the new eigenvectors with the initial eigenvalues -- their chains and their ``S``
    must then differ from the whole ladder's (they would not if a block took its scales from anywhere but the broadcast table)."""
    orc, _lib, PTEngine = mods
    case = sm.CASES[name]
    cov0, p0, kw = sm.inputs(case)
    ref, marks = sm.reference(case, orc)
    _, engines = _run_emulated_ladder(case.nranks, case.ntb, case.d, case.W, case.n, cov0, p0, kw, ref=ref, comm=_LosesS)
    own = engines[0].local
    assert engines[0].comm.lost == 0 and not np.array_equal(own.get("S"), marks.S0)
    for r, e in enumerate(engines[1:], 1):
        L, sl = e.local, slice(r * case.ntb, (r + 1) * case.ntb)
        assert e.comm.lost == 4 and L.exchange_violations() == 0             # one broadcast per covariance epoch
        # the eigenvectors arrived, the eigenvalues are still the initial ones (states that crossed the edges took the difference
        # to the owner's block too: its tables are compared with what it broadcast, not with the whole ladder's)
        assert np.array_equal(L.get("Ut"), own.get("Ut")) and np.array_equal(L.get("S"), marks.S0), r
        assert not np.array_equal(L.by_temp("X"), ref.by_temp(ref.X)[:, sl]), "block %d steps as if S had arrived" % r


def test_what_a_block_refuses_it_refuses_on_every_block(mods):
    """The engine's own refusals (tests/test_sharded_modes.py reads their messages without a GPU) with the real device behind them:
    the owner's block and another raise alike, so that no block is left waiting in a collective."""
    from ptmcmcsampler_amd.sharded import ShardedPTEngine
    import re
    d = 6
    for kw, words, own in sm.REFUSALS:
        kw = dict(kw)
        ntg = kw.pop("ntemps_global", 6)
        for rank in (0, 1):
            with pytest.raises(ValueError, match=re.escape(words)):
                ShardedPTEngine(d, ntg, 3, np.eye(d) * 0.05, comm=types.SimpleNamespace(rank=rank, world=2), **kw)
