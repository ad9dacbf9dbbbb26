"""The sharded ladder's mode matrix: one case for every combination of covariance mode, eigensolver, ``eig_lag`` and parameter groups
that ``ShardedPTEngine`` (ptmcmcsampler_amd/sharded.py) forwards to its blocks and that no sharded run reached before, shared by

  * tests/test_sharded_modes.py      -- real processes over gloo with the oracle standing in for the per-GPU engine (no GPU), and
  * tests/test_sharded_modes_gpu.py  -- one thread per block on the one GPU, the HIP kernels behind every block,

both against the WHOLE ladder on ``OracleEngine``, bit for bit.  Every ladder has six ranks: two blocks of three or three blocks of
two, so that the same oracle run serves world sizes 2 and 3.  Covariance epochs every 20 iterations, DE epochs every 40, swaps every 5,
85 iterations: four covariance epochs (the owner broadcasts ``Ut`` / ``S`` four times), two DE epochs with DE coming on at iteration
41, 17 swap epochs.

A case proves something only if the blocks that do NOT hold rank 0 step with what the owner broadcast: ``depends_on_the_broadcast``
states that as conditions on the ORACLE's run alone (swaps accepted across every block edge, tables that moved away from the initial
ones, AM jumps accepted and DE proposed on the other blocks after the first epoch).  The seeds and scales in the table were chosen on the
CPU so that the oracle meets them; tests/test_sharded_modes.py checks that for every case, the sensitivity test there drops the
broadcast of ``S`` and sees the comparison fail.

Nothing here needs a GPU to import."""
import collections
import types

import numpy as np

# name, ndim, blocks and ranks per block of the GPU leg, walkers, iterations, engine keywords, how the single reference is held
# ("oracle": OracleEngine restates the configuration; "lockstep": the oracle does not restate the solver -- a single PTEngine is held to
# the oracle through the tables it made, test_device_tables_gpu.lockstep, and the blocks to both), the engine's seed, the seed and
# scale of the start, the scale of the initial covariance
Case = collections.namedtuple("Case", "name d nranks ntb W n kw hold seed p0_seed p0_scale cov0_scale")

NTG = 6
N = 85
COMMON = dict(weights=(20, 20, 20), cov_update=20, burn=40, tskip=5)


def _c(name, d, nranks, W, cov_mode, eig_mode, eig_lag=0, hold="oracle", seed=5, p0_seed=3, p0_scale=0.4, cov0_scale=0.05, **extra):
    assert NTG % nranks == 0
    kw = dict(COMMON, cov_mode=cov_mode, eig_mode=eig_mode, eig_lag=eig_lag, **extra)
    return Case(name, d, nranks, NTG // nranks, W, N, kw, hold, seed, p0_seed, p0_scale, cov0_scale)


_BOX6 = ("box", np.full(6, -10.0), np.full(6, 10.0))

CASES = collections.OrderedDict((c.name, c) for c in (
    # on-stream Jacobi (ptmi_eig_jacobi), the broadcast right behind it
    _c("jacobi-pooled-d12-lag0", 12, 3, 5, "pooled", "jacobi"),
    # [W] tables broadcast; odd ndim
    _c("jacobi-per_walker-d33-lag0", 33, 2, 4, "per_walker", "jacobi"),
    # the <= 128 QL kernel (ptmi_eig_ql) at lag 0, a table per walker
    _c("ql-per_walker-d60-lag0", 60, 3, 4, "per_walker", "ql"),
    # the first ndim of the wide solver (ptmi_eig_wide.hip), 16 lanes per chain, AM increments ahead of the launch
    _c("ql-pooled-d130-lag0-wide", 130, 2, 4, "pooled", "ql", p0_scale=0.2, cov0_scale=0.01),
    # the wide solver per walker; one AM list per walker; the owner holds the AM ring, the other blocks do not
    _c("ql-per_walker-d130-lag0-wide", 130, 3, 3, "per_walker", "ql", p0_scale=0.2, cov0_scale=0.01),
    # the wide solver on the owner's side stream, the table broadcast two launches late
    _c("ql-pooled-d130-lag2-wide-late", 130, 2, 4, "pooled", "ql", eig_lag=2, p0_scale=0.2, cov0_scale=0.01),
    # per-walker AM lists beyond 104-d with the host's factorization
    _c("lapack-per_walker-d130-lag0", 130, 2, 3, "per_walker", "lapack", p0_scale=0.2, cov0_scale=0.01),
    # ptmi_eig_sytrd on the engine's stream, the broadcast right behind it
    _c("sytrd-pooled-d130-lag0-on-stream", 130, 3, 4, "pooled", "sytrd", hold="lockstep", p0_scale=0.2, cov0_scale=0.01),
    # the ROCm library's solver on the engine's stream
    _c("hipsolver-pooled-d130-lag0-on-stream", 130, 2, 4, "pooled", "hipsolver", hold="lockstep", p0_scale=0.2, cov0_scale=0.01),
    # group tables from the host, per walker
    _c("groups-3+3-lapack-per_walker-d6", 6, 3, 5, "per_walker", "lapack", groups=[[0, 1, 2], [3, 4, 5]]),
    # one QL call per group; three unequal groups, one of a single parameter
    _c("groups-25+14+1-ql-pooled-d40", 40, 2, 5, "pooled", "ql", groups=[list(range(25)), list(range(25, 39)), [39]]),
    # groups with AM increments ahead of the launch beyond 104-d, the wide solver on the group of 100
    _c("groups-100+30-ql-pooled-d130-wide", 130, 3, 4, "pooled", "ql", groups=[list(range(100)), list(range(100, 130))],
       p0_scale=0.2, cov0_scale=0.01),
    # parameter groups with gradient jumps (tests/test_gj_groups_gpu.py's interleaved groups): curved likelihood, box prior, NUTS and
    # HMC in the cycle; the jump objects' state belongs to the ranks and stays put while states cross the block edges
    _c("groups-gradjump-curved-box-lapack-pooled-d6", 6, 2, 4, "pooled", "lapack", groups=[[0, 2, 4], [1, 3, 5]], logl=("curved",),
       logp=_BOX6, grad_weights=(10, 10), hmc=(0.08, 2, 50), seed=7, p0_seed=5, p0_scale=0.3, cov0_scale=1.0),
))

ORACLE_CASES = [c.name for c in CASES.values() if c.hold == "oracle"]          # what the CPU leg's stand-in can run
SENSITIVITY_CASES = ("jacobi-pooled-d12-lag0", "ql-per_walker-d60-lag0", "groups-25+14+1-ql-pooled-d40")     # pooled, per walker, groups


def has_gj(case):
    return sum(case.kw.get("grad_weights", (0, 0))) > 0


def inputs(case):
    """(cov0, p0 [W][6][d], engine keywords): the same for every engine of the case, sharded or not, device or oracle."""
    d, W = case.d, case.W
    rs = np.random.RandomState(case.p0_seed)
    cov0 = np.eye(d) * case.cov0_scale
    p0 = rs.randn(W, NTG, d) * case.p0_scale
    if has_gj(case):                                     # the curved family: around its ridge, wider with the rank, inside the box
        p0 = np.array([-0.1, -0.5] * (d // 2)) + p0 * np.linspace(0.5, 3.0, NTG)[None, :, None]
        p0 = np.clip(p0, -9.5, 9.5)
    return cov0, p0, dict(case.kw, seed=case.seed)


def oracle_kw(case, kw):
    """The keywords of the oracle that stands beside the case: "sytrd" and "hipsolver" are not restated -- the oracle's own factorization
    (LAPACK's) serves where only its chains' statistics matter, lockstep replaces it with the device's tables on the GPU."""
    return dict(kw, eig_mode="lapack") if case.hold == "lockstep" else kw


def first_table_in_force(case):
    """The iteration behind which every block steps with the first adapted table: the first covariance epoch, eig_lag launches later."""
    kw = case.kw
    return kw["cov_update"] + kw["eig_lag"] * kw["tskip"]


def reference(case, orc):
    """The whole ladder on the oracle: (engine after ``case.n`` iterations, marks for ``depends_on_the_broadcast``)."""
    cov0, p0, kw = inputs(case)
    o = orc.OracleEngine(case.d, NTG, case.W, cov0, **oracle_kw(case, kw))
    o.init_state(p0)
    marks = types.SimpleNamespace(Ut0=o.Ut.copy(), S0=o.S.copy())
    first = first_table_in_force(case)
    o.run(first)
    marks.jstat_first = o.jstat.copy()
    o.run(case.n - first)
    return o, marks


def counts(case, ref, marks):
    """The oracle-side figures that make the case meaningful, for both ways the six ranks are cut into blocks."""
    js = ref.jstat.astype(np.int64)
    am = js[..., 1, 1] - marks.jstat_first.astype(np.int64)[..., 1, 1]           # AM jumps accepted with an adapted table in force
    out = dict(swaps_by_pair=ref.nswap.sum(0).astype(np.int64)[:NTG - 1].tolist(), am_accepts_by_rank=am.sum(0).tolist(),
               de_proposed_by_rank=js[..., 2, 0].sum(0).tolist(), de_accepted_by_rank=js[..., 2, 1].sum(0).tolist())
    if has_gj(case):
        out["nuts_hmc_proposed"] = js[..., 3:5, 0].sum(axis=(0, 1)).tolist()
    return out


def depends_on_the_broadcast(case, ref, marks):
    """Conditions on the ORACLE's run alone without which the case would pass with a broadcast that never arrived."""
    kw, what = case.kw, case.name
    assert ref.iter == case.n and case.n // kw["tskip"] >= 6 and (case.n - 1) // kw["cov_update"] >= 3 and case.n > kw["burn"] + kw["cov_update"]
    c = counts(case, ref, marks)
    for ntb in (2, 3):
        edges = [c["swaps_by_pair"][k] for k in range(ntb - 1, NTG - 1, ntb)]
        assert min(edges) > 0, "%s: a block edge (blocks of %d) no swap ever crossed: %r" % (what, ntb, edges)
        for b in range(1, NTG // ntb):                   # every block but the owner's
            sl = slice(b * ntb, (b + 1) * ntb)
            assert sum(c["am_accepts_by_rank"][sl]) > 0, "%s: no AM jump accepted on block %d of %d ranks after the first table" % (what, b, ntb)
            assert sum(c["de_proposed_by_rank"][sl]) > 0, "%s: DE never proposed on block %d of %d ranks" % (what, b, ntb)
    assert not np.array_equal(ref.Ut, marks.Ut0) and not np.array_equal(ref.S, marks.S0), "%s: the tables never moved" % what
    for w in range(ref.S.shape[0]):
        for gi, g in enumerate(ref.groups):
            assert not np.array_equal(ref.S[w, gi, :len(g)], marks.S0[w, gi, :len(g)]), "%s: S of walker %d, group %d never moved" % (what, w, gi)
    if has_gj(case):
        assert min(c["nuts_hmc_proposed"]) > 0, what
    return c


# ------------------------------------------------------------------------------------------------------------------- refusals
# what a sharded ladder refuses by design: (keywords beside cov_mode / eig_mode defaults, words of the message, raised by ShardedPTEngine
# itself -- before a block's engine is made, hence before a library is loaded)
REFUSALS = (
    (dict(adapt_ladder=True), "adapt_ladder serves a whole ladder on one GPU", True),
    (dict(ntemps_global=7), "ntemps_global=7 is not a multiple of the 2 ranks", True),
    (dict(eig_mode="ql", eig_lag=2, cov_mode="per_walker"), "eig_lag with eig_mode='ql' and per-walker covariances is a one-GPU mode", True),
    (dict(eig_mode="ql", eig_lag=1), "eig_lag with eig_mode='ql' and per-walker covariances is a one-GPU mode", True),     # per_walker is the default
    (dict(eig_mode="jacobi", cov_mode="pooled", groups=[[0, 1, 2], [3, 4, 5]]), "eig_mode='jacobi' factorizes the full covariance: no parameter groups", False),
    (dict(eig_mode="sytrd", cov_mode="pooled", groups=[[0, 1, 2], [3, 4, 5]]), "eig_mode='sytrd' factorizes the full covariance: no parameter groups", False),
    (dict(eig_mode="jacobi", cov_mode="pooled", eig_lag=2), "eig_lag > 0 is implemented for eig_mode 'lapack', 'hipsolver', 'sytrd' and 'ql'", False),
    (dict(eig_mode="sytrd", cov_mode="per_walker"), "eig_mode='sytrd' factorizes one pooled covariance", False),
)
