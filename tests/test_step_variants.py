"""The step-kernel matrix: one case for every (shape, likelihood family, dispatch route, prior) that ``launch_mh_k``
(csrc/ptmi_mh.inc.h) can launch, and the ledger that keeps the matrix complete (no GPU needed).

A CELL is a shape (G, E) of ``PTMI_SHAPE_LIST`` x a likelihood family (iso, dense, curved) x a route of the shape's lane class
x a prior; a CASE is a cell with the ndim it runs at.  tests/test_step_variants_gpu.py runs every case on the device against
the oracle; this file holds the table both share, the flags ``ptmi_last_mh_variant`` must report for each case (read off
``launch_mh_k``, with the LDS byte arithmetic restated beside them) and the tests that fail when a shape of the list has no
cases.  To add a shape: put its ndim into ``NDIM`` (even, and with the last slot of lanes 2 and 3 empty where the shape allows
it); the table grows by itself, ``test_every_cell_has_exactly_one_case`` then passes again, and the GPU file runs the new cells.

Families: family 3 (interval) and the gradient-jump kernels have a matrix and a ledger of their own, tests/test_gj_variants.py with
tests/test_gj_variants_gpu.py (every shape of PTMI_GJ_SHAPE_LIST x family x layout x tables x prior, the layout asserted through
ptmi_last_gj_launch); tests/test_gradjump_gpu.py and tests/test_gj_groups_gpu.py hold the single cases that grew before it."""
import collections
import os
import re

import numpy as np

from ptmcmcsampler_amd import _lib as L
from test_gpu_bench_kernels import _dense          # the dense Gaussian of bench.py --logl dense (a NumPy helper: nothing there needs a GPU to import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = collections.namedtuple("Case", "shape ndim family prior route")

FAMILIES = ("iso", "dense", "curved")
# the ndim a shape's cases run at: even (the curved family pairs parameters), the last slot of lanes 2 and 3 empty
NDIM = {(4, 2): 6, (4, 5): 18, (4, 8): 30, (4, 14): 54, (4, 20): 78, (4, 25): 100, (4, 26): 102,
        (16, 7): 106, (16, 13): 114, (16, 26): 210, (64, 8): 418, (64, 16): 514, (64, 32): 1026}
# (4, 26) where a route's LDS test fails at 102-d (see route_fits): the smallest even ndim of the shape with that slot pattern
NDIM_SMALL = {(4, 26): 82}
EXACT = ((4, 25),)                                  # ptmi_shape_exact: these serve ndim == G * E only

# ------------------------------------------------------------------------------------------------------------- the routes
# name -> (weights, cov_mode, (nt, W), (nt, W) of the dense family or None, extras, environment)
ROUTES4 = collections.OrderedDict([
    ("R1", ((20, 0, 0), "pooled", (3, 6), None, {}, {})),
    ("R2", ((20, 0, 0), "pooled", (3, 6), None, {}, {"PTMI_ULDS_PERS": "0"})),
    ("R3", ((20, 0, 0), "per_walker", (3, 6), None, {}, {})),
    ("R4", ((20, 0, 0), "per_walker", (64, 2), (128, 2), {}, {})),          # a block per walker: 256 / 4 chains, dense 512 / 4
    ("R5", ((20, 20, 20), "pooled", (3, 6), None, {}, {})),
    ("R6", ((20, 20, 20), "pooled", (3, 6), None, {}, {"PTMI_NO_PC": "1"})),
    ("R7", ((1, 30, 0), "pooled", (3, 6), None, {}, {"PTMI_NO_PC": "1"})),
    ("R8", ((20, 20, 20), "per_walker", (64, 2), None, {}, {})),
    ("R9", ((20, 20, 20), "per_walker", (3, 6), None, {}, {})),
    ("R10", ((20, 0, 20), "pooled", (3, 6), None, {}, {})),
    ("R11", ((20, 20, 20), "pooled", (3, 6), None, {"pick_mode": "walker"}, {})),
    ("R12", ((20, 20, 20), "pooled", (3, 6), None, {"groups": True}, {})),
])
ROUTESW = collections.OrderedDict([
    ("W1", ((20, 0, 0), "pooled", (2, 3), None, {}, {})),
    ("W2", ((20, 0, 0), "per_walker", (2, 3), None, {}, {})),
    ("W3", ((20, 20, 20), "pooled", (2, 3), None, {}, {})),
    ("W4", ((20, 20, 20), "per_walker", (2, 3), None, {}, {})),
    ("W5", ((20, 20, 20), "pooled", (2, 3), None, {"groups": True}, {})),
    ("W6", ((20, 20, 20), "pooled", (2, 3), None, {"pick_mode": "walker"}, {})),
])
# routes in which the prior is a template argument of the kernel or box_off is placed behind other tables: these get a box cell too
BOX_ROUTES = ("R1", "R3", "R4", "R5", "R6", "R8", "R9", "W1", "W2", "W3")
# (route, family) pairs that are no cell: R2 is R1 without the persistent kernel, which the dense family never takes
NOT_A_CELL = (("R2", "dense"),)
# Cells whose route cannot be reached at ANY ndim of the shape because the route's tables exceed the 160 KB of a CU's LDS:
# (shape, family, route, prior) -> "bytes needed at the shape's smallest ndim against 163840".  Nothing else belongs here.
# Empty: the two LDS tests that fail at a shape's preferred ndim ((4, 26) at 102-d: two copies of the 102 x 103 table are 168096
# bytes in R2 / R4, the dense 512-thread kernel's tables 168352 bytes in R1 / R4) pass at 82-d (108896 and 109184 bytes).
UNREACHABLE = {}


def shape_list():
    """PTMI_SHAPE_LIST of csrc/ptmi_common.h, in its order."""
    txt = open(os.path.join(ROOT, "ptmcmcsampler_amd", "csrc", "ptmi_common.h")).read()
    line = re.search(r"#define PTMI_SHAPE_LIST\(X\)(.*)", txt).group(1)
    return [(int(g), int(e)) for g, e in re.findall(r"X\((\d+),\s*(\d+)\)", line)]


def lanes_for(d):
    """ptmi_lanes_for (csrc/ptmi_abi.hip)."""
    return 4 if d <= 104 else (16 if d <= 416 else 64)


def pick_shape(d, shapes):
    """pick_shape (csrc/ptmi_abi.hip) without gradient jumps: the first shape of the lane count that holds ndim."""
    return next((g, e) for g, e in shapes if g == lanes_for(d) and g * e >= d and ((g, e) not in EXACT or g * e == d))


def routes_of(shape):
    return ROUTES4 if shape[0] == 4 else ROUTESW


def cells(shapes):
    """Every cell of the matrix for the given shapes, UNREACHABLE ones included."""
    out = []
    for shape in shapes:
        for route in routes_of(shape):
            for family in FAMILIES:
                if (route, family) in NOT_A_CELL:
                    continue
                out.append((shape, family, route, "flat"))
                if route in BOX_ROUTES:
                    out.append((shape, family, route, "box"))
    return out


# ------------------------------------------------------------------------------------------- launch_mh_k's byte arithmetic
LDS = 160 * 1024
DRAWT = 8 * 128                                     # the draw tables (ptmi_tables.h)


def even(doubles):
    return (doubles + 1) & ~1


def mfma_ld(E):
    return 16 * ((4 * E + 15) // 16)


def box_bytes(G, E):
    return 8 * 2 * G * E                            # box_table_doubles: a lower and an upper bound per register slot


def staged_table(d, E):
    return 8 * 4 * ((d + 3) // 4) * mfma_ld(E)      # a zero-padded d x d table of the staged kernels


def dense_scam_bytes(d, E):
    """mh_dense_scam_kernel's tables: the two halves of the precision matrix, the eigenvectors, the mean, sqrt(S)."""
    half = ((d + 1) // 2) * d
    podd = half + ((16 - half % 32) + 32) % 32      # dense_podd
    return 8 * (podd + (d // 2) * d + d * d + 4 * E + d)


def ulds_table(d):
    return 8 * (d * d + d)                          # the SCAM-only table kernel's copy: eigenvectors and sqrt(S), unpadded


def staged_full_lds(d, E, dense, dense_pc):
    """(bytes in front of the AM ring, lds_u) of the staged FULL kernels: [likelihood table] [eigenvectors] sqrt(S)."""
    tab = staged_table(d, E)
    lds = tab if dense else 0
    lds_u = not dense_pc and lds + tab + 8 * d <= LDS
    if lds_u:
        lds += tab
    return lds + 8 * d, lds_u


def amq_bytes(E):
    return 8 * 4 * 16 * (4 * E + 2) + 4 * 4 * 128   # the ring of the block's four waves and their event lists


def route_fits(shape, d, family, route):
    """Do the LDS tests hold on which the route's kernel is launched at all?  (The prior's table never decides the route except in
    R4, where it takes sqrt(S)'s place when both do not fit twice: see box_in_lds.)"""
    G, E = shape
    dense = family == "dense"
    if G != 4 or route in ("R9", "R12"):
        return True                                 # kernels without tables in LDS
    if route in ("R1", "R4") and dense:
        return dense_scam_bytes(d, E) <= LDS        # 100-d: 161664; 102-d: 168352; 82-d: 109184
    if route == "R1":
        return 8 * even(d * d + d) + box_bytes(G, E) + DRAWT + 16 <= LDS      # one copy per CU: 102-d with bounds 86752
    if route in ("R2", "R4"):
        return 2 * ulds_table(d) <= LDS             # a copy per block, two blocks per CU: 100-d 161600; 102-d 168096; 82-d 108896
    if route == "R3":
        return not dense or staged_table(d, E) <= LDS
    # the staged FULL kernels: everything up to the AM ring must fit; the producer / consumer form needs its lists behind it too
    no_pc = route in ("R6", "R7")
    with_am = route != "R10"
    dense_pc = dense and E >= 14 and with_am and not no_pc
    lds, lds_u = staged_full_lds(d, E, dense, dense_pc)
    lds = 8 * even(lds // 8) + amq_bytes(E)
    if lds > LDS:
        return False
    if route in ("R5", "R8", "R11") and (lds_u != dense):                     # tables_ok: mh_pc_kernel
        lists = 8 * 4 * 128 + 4 * 8 + (8 * 4 * E if dense else 0)
        return lds + box_bytes(G, E) + DRAWT + lists <= LDS                   # (4, 26) at 102-d, iso, bounds: 157136
    return True


def box_in_lds(case):
    """PTMI_VAR_LDS_BOX of a case: does launch_mh_k place the bounds table (2 G E doubles) in LDS?"""
    if case.prior != "box":
        return False
    (G, E), d, dense = case.shape, case.ndim, case.family == "dense"
    bb = box_bytes(G, E)
    if G != 4 or case.route == "R9" or (case.route == "R3" and not dense):
        return True                                 # the generic and padded-table kernels: box_off = 0, the only table (at most 32 KB)
    if case.route in ("R1", "R4") and dense:        # behind the 512-thread kernel's tables: 100-d 161664 + 1600 = 163264
        return 8 * even(dense_scam_bytes(d, E) // 8) + bb <= LDS
    if case.route == "R1":
        return True                                 # the persistent kernel always places it (route_fits counts it)
    if case.route == "R4":
        # behind sqrt(S) when two such copies fit a CU, else in sqrt(S)'s place: 100-d 2 x 82400 = 164800 does not fit, 2 x (80000 + 1600) = 163200 does
        return 2 * (8 * even(d * d + d) + bb) <= LDS or 2 * (8 * even(d * d) + bb) <= LDS
    if case.route == "R3":
        return 8 * even(staged_table(d, E) // 8) + bb <= LDS
    no_pc = case.route == "R6"
    dense_pc = dense and E >= 14 and not no_pc
    lds, _ = staged_full_lds(d, E, dense, dense_pc)
    return 8 * even(lds // 8) + amq_bytes(E) + bb <= LDS                      # behind the ring: (4, 26) at 102-d, iso 151984


# --------------------------------------------------------------------------------------------------------- expected flags
def expected_flags(case):
    """(must, must_not) of ``last_variant()[0]`` after the case's last launch (DE is on by then), from launch_mh_k.  PTMI_VAR_LDS_BOX
    is box_in_lds's."""
    G, E = case.shape
    dense, r = case.family == "dense", case.route
    ST, FU, UT, GR, UN, AQ = L.VAR_STAGED, L.VAR_FULL, L.VAR_LDS_UT, L.VAR_GROUPS, L.VAR_UNIFORM, L.VAR_AMQ
    DT, DS, PE, PC, UP = L.VAR_LDS_DRAWT, L.VAR_DENSE_SCAM, L.VAR_PERSISTENT, L.VAR_PC, L.VAR_UTPAD
    # dense with AM in the cycle: the producer / consumer kernel from 14 slots per lane on (dense_pc); below, both tables fit the LDS
    # and the one-wave kernel runs whatever the covariance mode or the pick mode -- mh_pc_kernel wants the eigenvectors in global memory
    small_dense = dense and E < 14
    if r == "R1":
        return (ST | DS | UT, FU | PE) if dense else (PE | UT | DT, ST | FU)
    if r == "R2":
        return UT, PE | ST | FU
    if r == "R3":
        return (ST, DS | FU | PE) if dense else (0, ST | UT | PE | FU)
    if r == "R4":
        return (ST | DS | UT, FU | PE) if dense else (UT, PE | ST | FU)
    if r == "R5":
        if small_dense:
            return ST | FU | UT | AQ, PC | PE
        return (ST | FU | PC | PE, UT | AQ) if dense else (ST | FU | UT | PC | PE | DT, AQ)
    if r == "R6":
        return ST | FU | AQ, PC | PE
    if r == "R7":
        return ST | FU, AQ | PC | PE
    if r == "R8":
        return (ST | FU | UT | AQ, PC | PE) if small_dense else (FU | PC, PE)
    if r == "R9":
        return FU, ST | UT | GR | UN | AQ | DT | DS | PE | PC
    if r == "R10":
        return ST | FU, PC | AQ | PE
    if r == "R11":
        return (ST | FU | UT | UN, PC | AQ | PE) if small_dense else (FU | PC | UN, AQ)
    if r == "R12":
        return FU | GR, ST | PC | AQ | PE
    if r == "W1":
        return UP, FU | ST
    if r == "W2":
        return 0, UP | FU | ST
    if r in ("W3", "W4"):
        return FU, UP | GR | UN | ST
    if r == "W5":
        return FU | GR, UP | ST
    if r == "W6":
        return FU | UN, UP | GR | ST
    raise KeyError(r)


# ---------------------------------------------------------------------------------------------------------------- the table
def _ndim(shape, family, route):
    d = NDIM[shape]
    if shape in NDIM_SMALL and not route_fits(shape, d, family, route):
        d = NDIM_SMALL[shape]
    return d


def case_table(shapes=None):
    shapes = shape_list() if shapes is None else shapes
    return [Case(shape, _ndim(shape, family, route), family, prior, route)
            for shape, family, route, prior in cells([s for s in shapes if s in NDIM]) if (shape, family, route, prior) not in UNREACHABLE]


CASES = case_table()


def case_id(c):
    return "%dx%d-d%d-%s-%s-%s" % (c.shape[0], c.shape[1], c.ndim, c.family, c.route, c.prior)


# Cells that miss a condition of oracle_conditions with the recipe's covariance: cov0 is scaled by this factor, the smallest power of
# four with which the oracle's run meets them all (the conditions themselves stay).  R4 / R8, flat prior: a block per walker needs 64
# (dense: 128) ranks, and on the default ladder most of them are so hot that they accept every proposal -- 95.1 to 97.8 % of the SCAM
# proposals accepted with factor 1 (with the box prior the walls refuse them).  cov0 acts up to the first covariance epoch only, hence
# the large factors where the ladder is steepest (tstep = 1 + sqrt(2 / ndim)) and longest.  W2 / W4, curved, flat: none of the 30
# (20 at 1026-d) swap proposals was accepted with factor 1; 1026-d dense W4: 121 of 127 SCAM proposals accepted.
COV0_SCALE = {((4, 2), "iso", "R4", "flat"): 16, ((4, 2), "dense", "R4", "flat"): 65536, ((4, 2), "dense", "R8", "flat"): 4,
              ((4, 5), "iso", "R4", "flat"): 4, ((4, 5), "dense", "R4", "flat"): 1024, ((4, 5), "iso", "R8", "flat"): 4,
              ((4, 5), "dense", "R8", "flat"): 4, ((4, 8), "iso", "R4", "flat"): 4, ((4, 8), "dense", "R4", "flat"): 256,
              ((4, 8), "dense", "R8", "flat"): 4, ((4, 14), "dense", "R4", "flat"): 64, ((4, 20), "dense", "R4", "flat"): 16,
              ((4, 25), "dense", "R4", "flat"): 16, ((4, 26), "dense", "R4", "flat"): 16,
              ((16, 13), "curved", "W2", "flat"): 4, ((64, 32), "dense", "W4", "flat"): 4, ((64, 32), "curved", "W4", "flat"): 4}


def case_setup(case):
    """(d, nt, W, keywords of the engine and of the oracle, environment of the launch) of a case: the recipe every case shares."""
    d = case.ndim
    weights, cov_mode, ntw, ntw_dense, extra, env = routes_of(case.shape)[case.route]
    nt, W = ntw_dense if (case.family == "dense" and ntw_dense) else ntw
    if case.shape[0] > 4 and cov_mode == "per_walker" and d >= 514:
        W = 2                                       # the oracle factorizes every walker's covariance at every epoch
    A = np.random.RandomState(d).randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.4 * COV0_SCALE.get((case.shape, case.family, case.route, case.prior), 1.0)
    kw = dict(cov0=cov0, weights=weights, cov_mode=cov_mode, cov_update=20, burn=40, tskip=7, seed=d)
    if "pick_mode" in extra:
        kw["pick_mode"] = extra["pick_mode"]
    if "groups" in extra:
        kw["groups"] = [list(range(d)), list(range(1, d, 2))]
    if case.family == "dense":
        kw["logl"] = _dense(d)
    elif case.family == "curved":
        kw["logl"] = ("curved",)
    rs = np.random.RandomState(d + 1000)
    if case.prior == "box":                         # the bounds of test_box_prior_from_lds_table: walls close enough to be hit
        kw["logp"] = ("box", -0.25 - rs.rand(d) * 0.1, 0.2 + rs.rand(d) * 0.1)
        kw["p0"] = rs.uniform(-0.05, 0.05, (W, nt, d))
    else:
        kw["p0"] = rs.randn(W, nt, d) * 0.3
    return d, nt, W, kw, env


LAUNCHES = (41, 3, 26)      # three covariance epochs, DE activation (burn = 40), ten swap iterations, odd lengths and a launch of 3


def oracle_conditions(case, o, kw):
    """What keeps a case from passing vacuously, on the oracle's finished run.  Returns the acceptance shares by jump type."""
    weights = kw["weights"]
    js = o.jstat.astype(np.int64)
    shares = {}
    for j, name in enumerate(("SCAM", "AM", "DE")):
        if weights[j] > 0:
            prop, acc = js[..., j, 0].sum(), js[..., j, 1].sum()
            assert prop > 0, "%s was never proposed" % name
            shares[name] = acc / prop
            assert 0.05 <= shares[name] <= 0.95, "%s: %d of %d proposals accepted" % (name, acc, prop)
    if weights[1] > 0:
        assert js[..., 1, 1].sum() > 0, "no AM proposal was accepted"
    if weights[2] > 0:
        assert js[..., 2, 0].sum() > 0, "DE was never proposed"
    assert o.nswap.sum() > 0, "no swap was accepted"
    if kw["cov_mode"] == "per_walker":
        assert not np.array_equal(o.Ut[0], o.Ut[1]), "the walkers' tables did not diverge"
    if case.prior == "box":
        assert not np.isinf(o.lp).any(), "a chain ended outside the prior"
    return shares


# --------------------------------------------------------------------------------------------------------------- the ledger
def test_every_cell_has_exactly_one_case():
    """Every shape of PTMI_SHAPE_LIST x family x route of its lane class (flat), x the box routes, minus UNREACHABLE: one case each.
    A shape added to the list fails here until NDIM names its ndim."""
    shapes = shape_list()
    assert len(shapes) == len(set(shapes)) >= 13
    assert [s for s in shapes if s not in NDIM] == [], "shapes of PTMI_SHAPE_LIST without cases: give them an ndim in NDIM"
    assert sorted(NDIM) == sorted(shapes), "NDIM names a shape the library does not build"
    want = collections.Counter(c for c in cells(shapes) if c not in UNREACHABLE)
    got = collections.Counter((c.shape, c.family, c.route, c.prior) for c in CASES)
    assert got == want and max(got.values()) == 1
    assert set(UNREACHABLE) <= set(cells(shapes))
    # the count, spelled out: 4-lane shapes have 12 routes, R2 without the dense family, 7 of them with a box cell; the others 6 and 3
    n4, nw = sum(g == 4 for g, _ in shapes), sum(g > 4 for g, _ in shapes)
    assert len(CASES) + len(UNREACHABLE) == n4 * ((12 * 3 - 1) + 7 * 3) + nw * (6 * 3 + 3 * 3)
    assert len(set(case_id(c) for c in CASES)) == len(CASES)


def test_every_case_runs_in_its_shape():
    shapes = shape_list()
    for c in CASES:
        assert pick_shape(c.ndim, shapes) == c.shape, case_id(c)
        assert c.family != "curved" or c.ndim % 2 == 0, case_id(c)
        assert c.ndim in (NDIM[c.shape], NDIM_SMALL.get(c.shape)), case_id(c)
    # the preferred ndim leaves the last slot of lanes 2 and 3 empty (ndim = G E - 2 at four lanes), the exact shape aside
    for (g, e), d in NDIM.items():
        assert d % 2 == 0 and (d == g * e - 2 or (g, e) in EXACT or g > 4), (g, e)
    # (the wide shapes run just above the shape below them: the first even ndim that the shape serves and its neighbour does not)
    for (g, e), d in NDIM.items():
        assert g == 4 or pick_shape(d - 2, shapes) != (g, e), (g, e)


def test_every_case_fits_the_lds_its_route_needs():
    """The LDS tests of launch_mh_k that decide the route hold at the case's ndim, and fail where NDIM_SMALL was taken."""
    for c in CASES:
        assert route_fits(c.shape, c.ndim, c.family, c.route), case_id(c)
        if c.ndim != NDIM[c.shape]:
            assert not route_fits(c.shape, NDIM[c.shape], c.family, c.route), case_id(c)
    small = sorted(set((c.family, c.route) for c in CASES if c.ndim != NDIM[c.shape]))
    assert small == [("curved", "R2"), ("curved", "R4"), ("dense", "R1"), ("dense", "R4"), ("iso", "R2"), ("iso", "R4")]
    # the edges the table sits on: 100-d fits the table-per-block kernel by 192 bytes with the draw tables, the dense kernel by 576 with bounds
    assert LDS - 2 * (ulds_table(100) + DRAWT) == 192
    assert LDS - (dense_scam_bytes(100, 25) + box_bytes(4, 25)) == 576
    assert dense_scam_bytes(102, 26) == 168352 and 2 * ulds_table(102) == 168096
    # every box cell has its bounds in LDS; in R4 at 100-d only in sqrt(S)'s place
    assert all(box_in_lds(c) for c in CASES if c.prior == "box")
    assert 2 * (8 * even(100 * 101) + box_bytes(4, 25)) > LDS >= 2 * (8 * 100 * 100 + box_bytes(4, 25))


def test_expected_flags_are_consistent():
    for c in CASES:
        must, must_not = expected_flags(c)
        assert must & must_not == 0, case_id(c)
        assert (must | must_not) & L.VAR_LDS_BOX == 0, case_id(c)
        if c.ndim > 210:
            continue                                # (the recipe's matrices at 418-d and beyond: the GPU file builds them)
        d, nt, W, kw, env = case_setup(c)
        assert kw["p0"].shape == (W, nt, d) and kw["cov0"].shape == (d, d)
        if c.route in ("R4", "R8"):                 # a walker's ranks fill whole blocks of 256 threads (the dense SCAM kernel: 512)
            assert kw["cov_mode"] == "per_walker" and nt % ((512 if c.family == "dense" and c.route == "R4" else 256) // 4) == 0
    assert all(k in set((c.shape, c.family, c.route, c.prior) for c in CASES) for k in COV0_SCALE)

