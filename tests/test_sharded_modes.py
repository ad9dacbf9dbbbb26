"""The sharded ladder's mode matrix (tests/sharded_modes.py) with real processes over gloo, world sizes 2 and 3, the oracle standing in
for the per-GPU engine (tests/oracle_local.py): ``ShardedPTEngine``'s epoch ordering -- statistics, factorization, the broadcast of
``Ut`` / ``S`` and of the new DE rows, the late table -- for parameter groups, the restated device solvers ("jacobi", "ql") and
per-walker tables, against the whole ladder on ``OracleEngine``, bit for bit.  No GPU.

One group of processes per world size runs every case (a module fixture: the processes start once), each test reads its case's
verdict.  What a rank asserts is what tests/test_sharded_gloo.py's ``_worker`` asserts, and the jump objects' state where gradient
jumps are in the cycle.

The sensitivity test runs three cases again with a communicator that loses the broadcast of ``S`` on every rank but the root: the
comparison must then FAIL on a block that does not hold rank 0 -- else the case's inputs would be too tame to notice a stale table."""
import datetime
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sharded_modes as sm
from test_sharded_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (2, 3)


class _LosesS(object):
    """A communicator whose broadcast of the engine's ``S`` never reaches the ranks beside the root (they take part in the
    collective, the result goes to a scratch tensor); everything else is the wrapped communicator's."""

    def __init__(self, inner):
        self.inner, self.rank, self.world = inner, inner.rank, inner.world
        self.target, self.lost = None, 0

    def broadcast(self, t):
        if self.rank != 0 and self.target is not None and t.data_ptr() == self.target.data_ptr():
            self.inner.broadcast(t.clone())
            self.lost += 1
            return
        self.inner.broadcast(t)

    def all_gather(self, out, inp):
        self.inner.all_gather(out, inp)

    def all_to_all(self, out, inp, out_splits=None, in_splits=None):
        self.inner.all_to_all(out, inp, out_splits, in_splits)


def _compare_block(case, e, ref, rank):
    """A rank's block against the whole ladder: test_sharded_gloo._worker's assertions, one by one."""
    nt, t0 = e.nt, e.temp0
    o = e.local.o
    sl = slice(t0, t0 + nt)
    assert np.array_equal(o.by_temp(o.X), ref.by_temp(ref.X)[:, sl]), "states by temperature"
    assert np.array_equal(o.by_temp(o.lnL), ref.by_temp(ref.lnL)[:, sl]), "lnL"
    assert np.array_equal(o.by_temp(o.lp), ref.by_temp(ref.lp)[:, sl]), "lp"
    assert np.array_equal(o.nacc, ref.nacc[:, sl]) and np.array_equal(o.jstat, ref.jstat[:, sl]), "nacc, jstat"
    assert np.array_equal(o.nswap[:, sl], ref.nswap[:, sl]), "nswap"
    assert np.array_equal(o.Ut, ref.Ut) and np.array_equal(o.S, ref.S), "Ut, S"
    assert np.array_equal(np.roll(e.local.ring, -e.local.head, axis=1), ref.DE), "DE ring"
    if sm.has_gj(case):
        assert np.array_equal(o.gj, ref.gj[:, sl]), "gj"                          # a rank's jump-object state
    if rank == 0:
        assert np.array_equal(o.AM, ref.AM) and np.array_equal(o.M2, ref.M2) and np.array_equal(o.cov, ref.cov), "AM, M2, cov"
    assert e.swap_proposed == ref.swap_proposed == case.n // case.kw["tskip"], "swap epochs"


def _run_case(case, rank, world, orc, ref, lose_s):
    from oracle_local import OracleLocal
    from ptmcmcsampler_amd.sharded import DistComm, ShardedPTEngine
    cov0, p0, kw = sm.inputs(case)
    comm = DistComm(dist.group.WORLD)
    if lose_s:
        comm = _LosesS(comm)
    e = ShardedPTEngine(case.d, sm.NTG, case.W, cov0, comm=comm, local_factory=OracleLocal, **kw)
    if lose_s:
        comm.target = e.local.t["S"]
    assert e.eig_lag == kw["eig_lag"] and e.local.o.ngr == len(kw.get("groups", [0])) and e.local.o.eig_mode == kw["eig_mode"]
    e.init_state(p0)
    e.run(case.n)
    moved = torch.tensor([e.rows_moved])
    dist.all_reduce(moved)
    out = dict(rows_moved=int(moved), lost=comm.lost if lose_s else 0, verdict="ok")
    try:
        _compare_block(case, e, ref, rank)
    except AssertionError as ex:
        out["verdict"] = "differs: %s" % (str(ex).splitlines()[0] if str(ex) else "?")
    return out


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    try:
        from oracle import oracle as orc
        res = {}
        for name in sm.ORACLE_CASES:
            case = sm.CASES[name]
            ref, _ = sm.reference(case, orc)
            res[name] = _run_case(case, rank, world, orc, ref, False)
            if name in sm.SENSITIVITY_CASES:
                res[name + " without S"] = _run_case(case, rank, world, orc, ref, True)
        with open(os.path.join(out_dir, "rank_%d.json" % rank), "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module", params=WORLDS, ids=["world%d" % w for w in WORLDS])
def verdicts(request, tmp_path_factory):
    """{case: [every rank's result]} of one group of ``world`` processes over gloo."""
    world = request.param
    out_dir = str(tmp_path_factory.mktemp("sharded_modes_w%d" % world))
    mp.spawn(_worker, args=(world, _free_port(), out_dir), nprocs=world, join=True)
    per_rank = [json.load(open(os.path.join(out_dir, "rank_%d.json" % r))) for r in range(world)]
    return world, {name: [pr[name] for pr in per_rank] for name in per_rank[0]}


@pytest.mark.parametrize("name", sm.ORACLE_CASES)
def test_sharded_case_equals_the_whole_ladder(verdicts, name):
    world, res = verdicts
    assert [r["verdict"] for r in res[name]] == ["ok"] * world, res[name]
    assert res[name][0]["rows_moved"] > 0, "no row ever crossed a block edge: the test would prove nothing"


@pytest.mark.parametrize("name", sm.SENSITIVITY_CASES)
def test_a_lost_broadcast_of_S_shows_on_a_block_without_rank_0(verdicts, name):
    """The same run with ``S`` never arriving beside the root: every other block steps with the initial eigenvalues under the new
    eigenvectors, and the comparison that passed above fails there."""
    world, res = verdicts
    assert [r["verdict"] for r in res[name]] == ["ok"] * world
    lost = res[name + " without S"]
    assert lost[0]["lost"] == 0 and all(r["lost"] >= 3 for r in lost[1:]), lost        # one broadcast per covariance epoch was lost
    assert all(r["verdict"].startswith("differs") for r in lost[1:]), lost


@pytest.mark.parametrize("name", list(sm.CASES))
def test_the_oracle_run_of_every_case_depends_on_the_broadcast(name):
    """The conditions under which a case can notice a stale or partial table, on the oracle's run alone (for "sytrd" / "hipsolver" the
    oracle's own factorization stands in: the GPU leg states them again on the run stepped with the device's tables)."""
    from oracle import oracle as orc
    case = sm.CASES[name]
    ref, marks = sm.reference(case, orc)
    sm.depends_on_the_broadcast(case, ref, marks)


def test_the_table_holds_the_cases_the_matrix_names():
    by = {(c.d, c.kw["cov_mode"], c.kw["eig_mode"], c.kw["eig_lag"], tuple(len(g) for g in c.kw.get("groups", ())), sm.has_gj(c)) for c in sm.CASES.values()}
    for want in ((12, "pooled", "jacobi", 0, (), False), (33, "per_walker", "jacobi", 0, (), False), (60, "per_walker", "ql", 0, (), False),
                 (130, "pooled", "ql", 0, (), False), (130, "per_walker", "ql", 0, (), False), (130, "pooled", "ql", 2, (), False),
                 (130, "per_walker", "lapack", 0, (), False), (130, "pooled", "sytrd", 0, (), False), (130, "pooled", "hipsolver", 0, (), False),
                 (6, "per_walker", "lapack", 0, (3, 3), False), (40, "pooled", "ql", 0, (25, 14, 1), False), (130, "pooled", "ql", 0, (100, 30), False),
                 (6, "pooled", "lapack", 0, (3, 3), True)):
        assert want in by, want
    for c in sm.CASES.values():
        assert c.nranks * c.ntb == sm.NTG and c.nranks in (2, 3) and 3 <= c.W <= 6 and c.kw["weights"] == (20, 20, 20)
        assert (c.hold == "lockstep") == (c.kw["eig_mode"] in ("sytrd", "hipsolver"))
    assert set(sm.SENSITIVITY_CASES) <= set(sm.ORACLE_CASES)


class _Ranks(object):
    """The two numbers ShardedPTEngine reads off a communicator before it builds anything."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world


def test_what_a_sharded_ladder_refuses(monkeypatch):
    """The combinations refused by design, by their messages: ShardedPTEngine's own before a block's engine exists (no library is
    loaded), PTEngine's on every block alike (from the configuration alone: no block raises by itself and leaves the others waiting
    in a collective)."""
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    from ptmcmcsampler_amd.sharded import ShardedPTEngine
    import re
    d = 6
    loads = []
    real_load = _lib.load

    def counted():
        loads.append(1)
        return real_load()

    monkeypatch.setattr(_lib, "load", counted)
    # PTEngine asks for a device right behind loading the library and refuses a configuration before it touches one: the two probes
    # are answered for it, so that its refusals can be read on a machine without a GPU too (the library itself is loaded first, with
    # the probes' true answers; ``loads`` counts the calls from here on)
    real_load()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(_lib, "device_count", lambda: 1)
    for kw, words, own in sm.REFUSALS:
        kw = dict(kw)
        ntg = kw.pop("ntemps_global", 6)
        for rank in (0, 1):                                                   # the owner's block and another: the same refusal
            before = len(loads)
            made = []

            def factory(*a, **k):
                made.append(1)
                return PTEngine(*a, **k)

            with pytest.raises(ValueError, match=re.escape(words)):
                ShardedPTEngine(d, ntg, 3, np.eye(d) * 0.05, comm=_Ranks(rank, 2), local_factory=factory, **kw)
            assert bool(made) == (not own), (kw, rank)
            if own:
                assert len(loads) == before, "the library was loaded before the refusal: %r" % (kw,)
