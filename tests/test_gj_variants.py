"""The gradient-jump matrix: one case for every (shape, likelihood family, layout, tables, prior) that the ``PTMI_OP_MH_GJ`` branch of
csrc/ptmi_shape.hip can launch, and the ledger that keeps the matrix complete (no GPU needed).

A CELL is a shape (G, E) of ``PTMI_GJ_SHAPE_LIST`` x a likelihood family (iso, dense, curved, interval) x a layout of
``mh_steps_gj_kernel<G, E, L, PAIR, W16, GRP>`` x the whitening tables (full / diagonal) x a prior (flat / box); it has exactly one
case.  The further axes ride on the cells instead of multiplying them: the ndim (each family of a layout sits on the shape's upper
or lower edge, see ``_ndim``), the cycle (NUTS + HMC; one HMC-only and one NUTS-only cell per layout, see ``_cycle``) -- and EXTRA
cases repeat a cell with one thing changed: the tree stack cut to one level of LDS (``PTMI_GJ_LDS_LEVELS=1``), chains with a wave of
their own (``PTMI_GJ_SOLO``), exactly one wave of chains in the pair layout.  tests/test_gj_variants_gpu.py runs every case on the
device against the oracle; this file holds the table both share, what ``ptmi_last_gj_launch`` must report for each case (the
selection of csrc/ptmi_shape.hip and its LDS arithmetic, restated) and the tests that fail when a shape of the list has no cases.
All layouts give the same bits by design: only the report tells a case which kernel it ran.

The 16-lane shape (16, 7) is two shape classes here, ndim <= 64 and beyond: the whole-wave layout serves the first alone."""
import collections
import os
import re

import numpy as np
import pytest

from ptmcmcsampler_amd import _lib as L
from test_step_variants import ROOT

GCase = collections.namedtuple("GCase", "shape cls ndim family layout tables prior cycle extra")

FAMILIES = ("iso", "dense", "curved", "interval")
GJ_BLOCK = 64                                       # csrc/ptmi_gj.inc.h: one wave per block
GJ_REG_MAX = 512                                    # PTMI_GJ_REG_MAX
# a shape class: (shape, the ndim range it serves); (16, 7) splits at the a.d <= 64 rule of the whole-wave layout
CLASSES = collections.OrderedDict([("4x2", ((4, 2), 2, 8)), ("4x5", ((4, 5), 9, 20)), ("4x8", ((4, 8), 21, 32)),
                                   ("16x7lo", ((16, 7), 33, 64)), ("16x7hi", ((16, 7), 65, 112)), ("64x8", ((64, 8), 113, 512))])
# layout name -> (PTMI_GJL_* layout, GRP instantiation, hook that forces it or None)
LAYOUTS = collections.OrderedDict([
    ("WAVE", (L.GJL_WAVE, False, None)), ("WAVE-NOPAIR", (L.GJL_WAVE, False, "PTMI_GJ_NOPAIR")), ("PAIR", (L.GJL_PAIR, False, None)),
    ("WAVE-GRP", (L.GJL_WAVE, True, None)), ("W16", (L.GJL_W16, False, None)), ("CHAIN-NOWIDE16", (L.GJL_CHAIN, False, "PTMI_GJ_NOWIDE16")),
    ("CHAIN", (L.GJL_CHAIN, False, None)), ("CHAIN-GRP", (L.GJL_CHAIN, True, None))])
# (layout, tables, families) of each shape class: what csrc/ptmi_shape.hip can reach there.  WAVE with diagonal tables is the dense
# family's own choice (the pair layout has no dense products) and the other families' through PTMI_GJ_NOPAIR; ptmi_create refuses
# the interval family with parameter groups.
NO_DENSE, NO_INTERVAL = ("iso", "curved", "interval"), ("iso", "dense", "curved")
LANES4 = (("WAVE", "full", FAMILIES), ("WAVE", "diag", ("dense",)), ("WAVE-NOPAIR", "diag", NO_DENSE), ("PAIR", "diag", NO_DENSE),
          ("WAVE-GRP", "full", NO_INTERVAL))
REACH = {"4x2": LANES4, "4x5": LANES4, "4x8": LANES4,
         "16x7lo": (("W16", "full", FAMILIES), ("W16", "diag", FAMILIES), ("CHAIN-NOWIDE16", "full", FAMILIES)),
         "16x7hi": (("CHAIN", "full", FAMILIES), ("CHAIN", "diag", FAMILIES), ("CHAIN-GRP", "full", NO_INTERVAL)),
         "64x8": (("CHAIN", "full", FAMILIES), ("CHAIN", "diag", FAMILIES), ("CHAIN-GRP", "full", NO_INTERVAL))}
# Layouts whose cells run under one prior, with the reason (as NOT_A_CELL of test_step_variants.py: nothing else is left out).
ONE_PRIOR = {"WAVE-NOPAIR": ("flat", "a test hook forces it: the same instantiation as WAVE with diagonal tables, whose box_off the dense cells place"),
             "CHAIN-NOWIDE16": ("flat", "a test hook forces it: the same instantiation as CHAIN beyond 64-d, whose box_off those cells place"),
             "WAVE-GRP": ("box", "box_off sits where WAVE puts it; the bounds test of the GRP instantiation is the code that differs"),
             "CHAIN-GRP": ("box", "box_off sits where CHAIN puts it; the bounds test of the GRP instantiation is the code that differs")}


def gj_shape_list():
    """PTMI_GJ_SHAPE_LIST of csrc/ptmi_common.h, in its order."""
    txt = open(os.path.join(ROOT, "ptmcmcsampler_amd", "csrc", "ptmi_common.h")).read()
    line = re.search(r"#define PTMI_GJ_SHAPE_LIST\(X\)(.*)", txt).group(1)
    return [(int(g), int(e)) for g, e in re.findall(r"X\((\d+),\s*(\d+)\)", line)]


def lanes_for_grad(d):
    """ptmi_lanes_for_grad (csrc/ptmi_abi.hip) up to the fused kernels' limit."""
    return 4 if d <= 32 else (16 if d <= 112 else 64)


def pick_shape(d, shapes):
    """pick_shape (csrc/ptmi_abi.hip) with gradient jumps: the first shape of the lane count with at most 8 slots that holds ndim."""
    return next(((g, e) for g, e in shapes if g == lanes_for_grad(d) and g * e >= d and e <= 8), None)


def cells():
    """Every cell: (class, family, layout, tables, prior)."""
    out = []
    for cls, reach in REACH.items():
        for layout, tables, fams in reach:
            for family in fams:
                for prior in ("flat", "box"):
                    if layout in ONE_PRIOR and prior != ONE_PRIOR[layout][0]:
                        continue
                    out.append((cls, family, layout, tables, prior))
    return out


def _ndim(cls, family, prior):
    """The ndim of a cell: the shape's upper edge (8, 20, 32, 64, 112, 512) or its lower one (2, 10, 22, 34, 66, 114 for the curved
    family, which pairs parameters; 2, 9, 21, 33, 65, 113 for the others).  iso and interval sit low under the flat prior and high
    under the box, dense and curved the other way round: a layout with both priors has both edges in every family, one with a
    single prior both edges in two families each."""
    _, lo, hi = CLASSES[cls]
    low = (family in ("iso", "interval")) == (prior == "flat")
    if not low:
        return hi
    return lo + 1 if (family == "curved" and lo % 2) else lo


def _cycle(family, layout, prior):
    """The cycle of a cell.  Per (class, layout): the iso cell under the layout's last prior runs HMC alone (the launch order is off:
    PTMI_GJL_ORDERED clear), one cell NUTS alone with no AM entry (interval under the flat prior; where the layout has no such cell,
    dense under its first prior) -- so the 16- and 64-lane layouts run once without the AM increments ahead of the launch --, all
    others NUTS + HMC beside SCAM, AM and DE."""
    priors = (ONE_PRIOR[layout][0],) if layout in ONE_PRIOR else ("flat", "box")
    if family == "iso" and prior == priors[-1]:
        return "hmc"
    if layout in ("WAVE-GRP", "CHAIN-GRP"):
        return "nuts" if (family == "dense" and prior == priors[0]) else "both"
    if family == "interval" and prior == priors[0]:
        return "nuts"
    return "both"


def _case(cls, family, layout, tables, prior, extra=""):
    cyc = _cycle(family, layout, prior)
    if layout == "WAVE" and tables == "diag":       # (the dense family's own cells: no iso or interval cell beside them)
        cyc = {"flat": "nuts", "box": "hmc"}[prior]
    return GCase(CLASSES[cls][0], cls, _ndim(cls, family, prior), family, layout, tables, prior, cyc, extra)


def _extras(cases):
    """The cases beyond the cells: a cell's recipe with one thing changed."""
    by = {(c.cls, c.layout, c.tables, c.family, c.prior): c for c in cases}
    out = []
    for cls, reach in REACH.items():
        G = CLASSES[cls][0][0]
        for layout, tables, fams in reach:
            prior = ONE_PRIOR[layout][0] if layout in ONE_PRIOR else "box"
            if layout == "WAVE" and tables == "diag":
                continue                            # (one instantiation with WAVE-NOPAIR, which carries the extras)
            base = by[(cls, layout, tables, "curved", prior)]
            assert base.cycle == "both"
            # the tree stack with one level in LDS, every height above 0 in global scratch
            out.append(base._replace(extra="lds1"))
            # the launch order with chains that have a wave to themselves, where a wave holds more than one chain
            if G < 64:
                out.append(base._replace(extra="solo"))
        if G == 4:                                  # the pair layout with exactly one full wave of chains
            out.append(by[(cls, "PAIR", "diag", "iso", "flat")]._replace(extra="wave16", cycle="both"))
    return out


def case_table():
    cs = [_case(*cell) for cell in cells()]
    return cs + _extras(cs)


CASES = case_table()


def case_id(c):
    return "%s-d%d-%s-%s-%s-%s-%s%s" % (c.cls, c.ndim, c.family, c.layout, c.tables, c.prior, c.cycle, "-" + c.extra if c.extra else "")


# ------------------------------------------------------------------------------------------------------------- the recipe
def short_run(c):
    return c.ndim >= 256


def run_plan(c):
    """(engine keywords of the run, the pieces it goes in).  The default is the run of tests/test_gradjump_gpu.py: 260 iterations over
    five covariance epochs, DE activation and 26 swap iterations; from 256-d on four covariance epochs, DE activation and nine swaps."""
    if short_run(c):
        return dict(cov_update=20, burn=40, tskip=10), (33, 7, 50)
    return dict(cov_update=50, burn=100, tskip=10), (60, 7, 63, 130)


def chains(c):
    """(nt, W): never a whole number of waves where a wave holds several chains (dead chain groups repeat a chain and write nothing),
    more than one wave at four lanes; the 64-lane shape has one chain per wave."""
    if c.extra == "wave16":
        return 4, 4
    if short_run(c):
        return 2, 2
    return {4: (3, 6), 16: (3, 3), 64: (2, 3)}[c.shape[0]]


def solo_of(c):
    """PTMI_GJ_SOLO of a case: the library's default is a 32nd of the chains, none here."""
    nt, W = chains(c)
    return {4: 5, 16: 2}[c.shape[0]] if c.extra == "solo" else (nt * W) // 32


# step size, shortest and longest trajectory of HMC: long enough to be refused at the cold end, short enough for the oracle
HMC = {"iso": (0.35, 2, 12), "dense": (0.35, 2, 12), "curved": (0.08, 2, 30), "interval": (0.4, 2, 24)}
HMC_WIDE = {"iso": (0.1, 2, 8), "dense": (0.22, 2, 8), "curved": (0.08, 2, 12), "interval": (0.3, 2, 10)}      # ndim >= 256 (iso at 0.22: none of 165 accepted)


def case_setup(c):
    """(d, nt, W, cov0, p0, keywords of the engine and of the oracle, environment of the launch)."""
    d, (nt, W) = c.ndim, chains(c)
    grp = LAYOUTS[c.layout][1]
    rs = np.random.RandomState(7 * d + len(c.family))
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + np.eye(d)) * (1.0 if c.family == "curved" else 0.3)
    if c.tables == "diag":
        cov0 = np.diag(np.diag(cov0))
    kw, pieces = run_plan(c)
    kw.update(seed=1000 + d, hmc=(HMC_WIDE if short_run(c) else HMC)[c.family],
              weights=(10, 0, 10) if c.cycle == "nuts" else (10, 10, 10),
              grad_weights={"both": (10, 10), "hmc": (0, 20), "nuts": (20, 0)}[c.cycle])
    if c.family == "dense":
        B = rs.randn(d, d)
        kw["logl"] = ("dense", rs.randn(d) * 0.1, np.linalg.inv(B @ B.T / d + 0.5 * np.eye(d)))
    elif c.family == "interval":                    # uneven intervals around (0, 10), the reference's own NUTS workload
        kw["logl"] = ("interval", 0.0 - rs.uniform(0, 0.5, d), 10.0 + rs.uniform(0, 2.0, d))
    else:
        kw["logl"] = (c.family,)
    if c.family == "curved":
        centre, spread = np.array([-0.1, -0.5] * (d // 2)), 0.05
        lo, hi = np.array([-0.5, -1.4] * (d // 2)), np.array([0.45, -0.1] * (d // 2))
    elif c.family == "interval":                    # the unconstrained parameter: x = a + (b - a) / (1 + exp(-p)) near 1 at p = -2.3
        centre, spread = np.full(d, -2.3), 0.3
        lo, hi = np.full(d, -3.6), np.full(d, -1.2)
    else:
        centre, spread = np.zeros(d), 0.3
        lo, hi = np.full(d, -1.6), np.full(d, 1.5)
    if short_run(c) and c.family != "curved":
        # From 256-d on HMC, which moves every parameter at once, would never land inside the walls above once the chains have spread
        # (512 parameters, each outside with a few per cent); and in 90 iterations from this start they have not spread.  The
        # interval family gets walls at the per-mille quantiles of its parameter; iso walls stand just inside the start's largest
        # elements (0.3 x 3.5 sigma of 2048 draws; the start is clipped into them): some HMC proposals cross them, some do not.
        lo, hi = (np.full(d, -9.0), np.full(d, -0.7)) if c.family == "interval" else (np.full(d, -0.9), np.full(d, 0.9))
    p0 = centre + rs.randn(W, nt, d) * spread
    if c.prior == "box":                            # walls close enough to refuse proposals, uneven, the start inside them
        lo, hi = lo - rs.rand(d) * 0.1, hi + rs.rand(d) * 0.1
        kw["logp"] = ("box", lo, hi)
        p0 = np.clip(p0, lo + 0.05, hi - 0.05)
    if grp:                                         # overlapping groups of uneven size, no parameter left out
        kw["groups"] = [list(range(0, d, 2)), list(range(1, d)), list(range(d))] if d > 2 else [[0], [1, 0]]
    env = {}
    hook = LAYOUTS[c.layout][2]
    if hook:
        env[hook] = "1"
    if c.extra == "lds1":
        env["PTMI_GJ_LDS_LEVELS"] = "1"
    env["PTMI_GJ_SOLO"] = str(solo_of(c))
    return d, nt, W, cov0, p0, kw, env, pieces


HOOKS = ("PTMI_GJ_NOPAIR", "PTMI_GJ_NOWIDE16", "PTMI_GJ_LDS_LEVELS", "PTMI_GJ_SOLO", "PTMI_AM_BUDGET_MB")


# ------------------------------------------------------------------------- the selection of csrc/ptmi_shape.hip, restated
def gjw_table_doubles(E):
    return 3 * (4 * E) * (4 * E)                    # the three whitening tables, rows padded to 4 E


def gjw_level_doubles(E):
    return 4 * 4 * E + 4                            # a stack entry of the whole-wave layouts: four vectors in element order, four scalars


def gj_level_doubles(E):
    return (4 * E + 4) * 64                         # ... of the per-chain layout: every lane keeps its slots and its copy of the scalars


def box_table_doubles(G, E):
    return 2 * G * E


def expected_launch(c, nuts_maxdepth=24):
    """(layout | flags, lds_levels, lds_bytes, nslots) that ptmi_last_gj_launch reports after the case's last launch: the
    PTMI_OP_MH_GJ branch of csrc/ptmi_shape.hip, launch_gj and the pieces loop of csrc/ptmi_abi.hip."""
    (G, E), d = c.shape, c.ndim
    nt, W = chains(c)
    _, grp, hook = LAYOUTS[c.layout]
    diag, dense = c.tables == "diag", c.family == "dense"
    box = box_table_doubles(G, E) if c.prior == "box" else 0
    lv = 1 if c.extra == "lds1" else 1 << 30
    wave_levels = min(nuts_maxdepth + 1, 11, lv)    # heights 0 .. 10 in LDS, the rest in global scratch
    if G == 4:
        pair = diag and not dense and not grp and hook != "PTMI_GJ_NOPAIR"
        layout = L.GJL_PAIR if pair else L.GJL_WAVE
        levels = wave_levels
        off = 3 * 4 * E if diag else gjw_table_doubles(E)
        off += (2 if pair else 1) * levels * gjw_level_doubles(E) + (72 + 2 * GJ_BLOCK if pair else 64)
    elif G == 16 and d <= 64 and not grp and hook != "PTMI_GJ_NOWIDE16":
        layout, levels = L.GJL_W16, wave_levels
        off = (3 * 64 if diag else 0) + levels * gjw_level_doubles(16) + 64
    else:
        layout = L.GJL_CHAIN
        budget = 40 * 1024 // 8                     # a quarter of the CU's LDS for each of its four waves
        levels = min((budget - box) // gj_level_doubles(E) if box < budget else 0, nuts_maxdepth + 1, lv)
        off = levels * gj_level_doubles(E)
    off = (off + 1) & ~1
    off += box
    cpw = 64 // G
    ordered = c.cycle != "hmc"                      # the launch order serves the cycles with NUTS
    nch, solo = nt * W, min(solo_of(c) if cpw > 1 else 0, nt * W)
    nslots = solo * cpw + -(-(nch - solo) // cpw) * cpw if ordered else nch
    am_ahead = c.cycle != "nuts" and (grp or G > 4)     # w_am > 0 and (parameter groups or a 16- / 64-lane shape): ptmi_am_prepare's pieces
    flags = ((L.GJL_DIAG if diag else 0) | (L.GJL_GRP if grp else 0) | (L.GJL_BOX_LDS if box else 0) |
             (L.GJL_ORDERED if ordered else 0) | (L.GJL_AM_AHEAD if am_ahead else 0))
    return layout | flags, levels, 8 * off, nslots


# ------------------------------------------------------------------------------------------------------------ not idle
def oracle_conditions(c, o, kw, niter):
    """What keeps a case from passing vacuously, on the oracle's finished run."""
    js = o.jstat.astype(np.int64)
    w, gw = kw["weights"], kw["grad_weights"]
    assert (js[..., 0].sum(-1) == niter).all(), "a chain did not propose once per iteration"
    for j, (name, wt) in enumerate(zip(("SCAM", "AM", "DE", "NUTS", "HMC"), tuple(w) + tuple(gw))):
        assert (js[..., j, 0].sum() > 0) == (wt > 0), "%s: weight %d, %d proposals" % (name, wt, js[..., j, 0].sum())
    if gw[0]:
        assert js[..., 3, 0].sum() == js[..., 3, 1].sum(), "NUTS proposals are always accepted (nutsjump.py:838)"
    if gw[1]:
        assert 0 < js[..., 4, 1].sum() < js[..., 4, 0].sum(), "HMC: %d of %d accepted" % (js[..., 4, 1].sum(), js[..., 4, 0].sum())
    for j, name in ((1, "AM"), (2, "DE")):
        assert not w[j] or js[..., j, 1].sum() > 0, "no %s proposal was accepted" % name
    assert o.nswap.sum() > 0, "no swap was accepted"
    assert all(np.isfinite(getattr(o, k)).all() for k in ("X", "lnL", "gj")), "a chain left the finite numbers"


def box_did_bind(c, o, orc):
    """A box case's oracle run under the flat prior ends somewhere else: the walls refused proposals."""
    d, nt, W, cov0, p0, kw, _, pieces = case_setup(c)
    f = orc.OracleEngine(d, nt, W, cov0, **{k: v for k, v in kw.items() if k != "logp"})
    f.init_state(p0)
    f.run(sum(pieces))
    assert not np.array_equal(f.X, o.X), "the box prior never refused a proposal"


def run_oracle(c, orc):
    d, nt, W, cov0, p0, kw, _, pieces = case_setup(c)
    o = orc.OracleEngine(d, nt, W, cov0, **kw)
    assert o.lanes == c.shape[0]
    o.init_state(p0)
    o.run(sum(pieces))
    return o, kw, sum(pieces)


# --------------------------------------------------------------------------------------------------------------- the ledger
def test_every_cell_has_exactly_one_case():
    """Every class of PTMI_GJ_SHAPE_LIST x layout it can reach x tables x family x prior has one case without an extra tag; the extras
    name a cell that exists.  A shape added to the list fails here until CLASSES and REACH name it."""
    shapes = gj_shape_list()
    assert len(shapes) == len(set(shapes)) >= 5
    assert sorted(set(s for s, _, _ in CLASSES.values())) == sorted(shapes), "CLASSES and PTMI_GJ_SHAPE_LIST name different shapes"
    assert sorted(REACH) == sorted(CLASSES)
    key = lambda c: (c.cls, c.family, c.layout, c.tables, c.prior)  # noqa: E731
    got = collections.Counter(key(c) for c in CASES if not c.extra)
    assert got == collections.Counter(cells()) and max(got.values()) == 1
    assert all(key(c) in got for c in CASES if c.extra)
    # the count, spelled out.  Four lanes: WAVE 4 x 2, its dense diagonal cells 2, NOPAIR 3, PAIR 3 x 2, GRP 3.  (16, 7) to 64-d: W16
    # 2 x 4 x 2, NOWIDE16 4.  (16, 7) beyond and (64, 8): CHAIN 2 x 4 x 2, GRP 3.
    assert len(cells()) == 3 * (8 + 2 + 3 + 6 + 3) + (16 + 4) + 2 * (16 + 3) == 124
    # extras: per (class, layout, tables) a one-level stack, and chains with a wave of their own below 64 lanes; the pair layout's full wave
    assert collections.Counter(c.extra for c in CASES) == {"": 124, "lds1": 3 * 4 + 3 + 3 + 3, "solo": 3 * 4 + 3 + 3, "wave16": 3}
    assert len(CASES) == 166 and len(set(case_id(c) for c in CASES)) == len(CASES)
    for layout, (prior, reason) in ONE_PRIOR.items():
        assert prior in ("flat", "box") and reason and layout in LAYOUTS


def test_every_case_runs_in_its_shape_and_on_an_edge():
    shapes = gj_shape_list()
    for c in CASES:
        shape, lo, hi = CLASSES[c.cls]
        assert pick_shape(c.ndim, shapes) == shape == c.shape and lo <= c.ndim <= hi, case_id(c)
        assert c.family != "curved" or c.ndim % 2 == 0, case_id(c)
        assert c.ndim in (hi, lo, lo + 1) and c.ndim <= GJ_REG_MAX, case_id(c)
    # the classes tile 2 .. PTMI_GJ_REG_MAX, and a class ends where its shape (or the whole-wave rule a.d <= 64) does
    edges = [CLASSES[k][1:] for k in CLASSES]
    assert edges[0][0] == 2 and edges[-1][1] == GJ_REG_MAX and all(b[0] == a[1] + 1 for a, b in zip(edges, edges[1:]))
    for cls, ((g, e), lo, hi) in CLASSES.items():
        assert hi == min(g * e, GJ_REG_MAX) or (cls, hi) == ("16x7lo", 64), cls
        assert pick_shape(hi + 1, shapes) != (g, e) or cls == "16x7lo", cls
    # per class: both edges in at least two families, the curved family on both; per (class, layout, tables): the upper edge
    for cls, (_, lo, hi) in CLASSES.items():
        mine = [c for c in CASES if c.cls == cls and not c.extra]
        for edge in ((hi,), (lo, lo + 1)):
            fams = set(c.family for c in mine if c.ndim in edge)
            assert len(fams) >= 2 and "curved" in fams, (cls, edge)
        assert cls == "4x2" or any(c.ndim == lo and lo % 2 for c in mine), cls          # the odd first ndim of the shape
        for layout, tables, _ in REACH[cls]:
            assert any(c.ndim == hi for c in mine if (c.layout, c.tables) == (layout, tables)), (cls, layout, tables)
            assert any(c.ndim < hi for c in mine if (c.layout, c.tables) == (layout, tables)) or (layout, tables) == ("WAVE", "diag"), (cls, layout)


def test_every_layout_has_every_cycle_and_its_extras():
    for cls in CLASSES:
        G = CLASSES[cls][0][0]
        for layout in set(r[0] for r in REACH[cls]):
            mine = [c for c in CASES if c.cls == cls and c.layout == layout]
            plain = [c for c in mine if not c.extra]
            assert set(c.cycle for c in plain) == {"both", "hmc", "nuts"}, (cls, layout)
            # box cells on every layout (WAVE with diagonal tables: through the dense family)
            assert any(c.prior == "box" for c in plain) or layout in ONE_PRIOR, (cls, layout)
            assert any(c.extra == "lds1" for c in mine), (cls, layout)
            assert any(c.extra == "solo" for c in mine) == (G < 64), (cls, layout)
            for c in mine:
                nt, W = chains(c)
                cpw = 64 // G
                if c.extra == "wave16":
                    assert nt * W == 16 and layout == "PAIR"
                elif cpw > 1:
                    assert (nt * W) % cpw != 0 and (G != 4 or nt * W > cpw), case_id(c)
                if c.extra == "solo":
                    assert 1 <= solo_of(c) < nt * W and c.cycle != "hmc", case_id(c)
                else:
                    assert solo_of(c) == 0, case_id(c)
        assert G != 4 or sum(c.extra == "wave16" for c in CASES if c.cls == cls) == 1


def test_expected_launch_reports():
    """The restated selection names the layout every case is in the table for, and the arithmetic gives the sizes worked out by
    hand below.  No cell needs more than 64 KB of dynamic LDS: the hipFuncSetAttribute branches of the PTMI_OP_MH_GJ code are
    never taken by this table (the largest block is the 4-lane full-table layout at E = 8 under the box prior, 37 216 bytes)."""
    biggest = (0, None)
    for c in CASES:
        flags, levels, nbytes, nslots = expected_launch(c)
        want, grp, _ = LAYOUTS[c.layout]
        assert flags & L.GJL_LAYOUT_MASK == want and bool(flags & L.GJL_GRP) == grp, case_id(c)
        assert bool(flags & L.GJL_DIAG) == (c.tables == "diag") and bool(flags & L.GJL_BOX_LDS) == (c.prior == "box"), case_id(c)
        assert bool(flags & L.GJL_ORDERED) == (c.cycle != "hmc"), case_id(c)
        nt, W = chains(c)
        assert nslots >= nt * W and (nslots == nt * W or flags & L.GJL_ORDERED), case_id(c)
        assert levels >= 1 and (levels == 1) == (c.extra == "lds1" or (c.shape == (64, 8) and c.prior == "box")), case_id(c)
        biggest = max(biggest, (nbytes, case_id(c)))
    assert biggest[0] == 8 * (3 * 32 * 32 + 11 * 132 + 64 + 64) == 37216 < 64 * 1024, biggest
    assert "4x8" in biggest[1] and "WAVE-full-box" in biggest[1]
    by = {case_id(c): c for c in CASES}
    # by hand: 18 chains in the pair layout at E = 5, three diagonals of 20, 2 x 11 levels of 84, the exchange area and the states
    assert expected_launch(by["4x5-d9-iso-PAIR-diag-flat-both"]) == (L.GJL_PAIR | L.GJL_DIAG | L.GJL_ORDERED, 11, 8 * (60 + 22 * 84 + 200), 32)
    # the whole-wave layout of 16 lanes: diagonals of 64, 11 levels of 260, the exchange area, 2 x 112 bounds; 9 chains in 4-chain waves
    assert expected_launch(by["16x7lo-d64-iso-W16-diag-box-hmc"]) == (L.GJL_W16 | L.GJL_DIAG | L.GJL_BOX_LDS | L.GJL_AM_AHEAD, 11, 8 * (192 + 2860 + 64 + 224), 9)
    # per chain at 64 lanes: 5120 doubles hold two levels of 2304, with the 1024 bounds one
    assert expected_launch(by["64x8-d512-dense-CHAIN-full-flat-both"]) == (L.GJL_CHAIN | L.GJL_ORDERED | L.GJL_AM_AHEAD, 2, 8 * 4608, 4)
    assert expected_launch(by["64x8-d512-iso-CHAIN-diag-box-hmc"]) == (L.GJL_CHAIN | L.GJL_DIAG | L.GJL_BOX_LDS | L.GJL_AM_AHEAD, 1, 8 * (2304 + 1024), 4)
    # two chains with a wave of their own beside 7 others in 4-chain waves: 2 x 4 + 8 slots
    assert expected_launch(by["16x7hi-d66-curved-CHAIN-full-box-both-solo"])[3] == 16
    assert expected_launch(by["4x2-d2-curved-WAVE-GRP-full-box-both-lds1"])[1:3] == (1, 8 * (3 * 64 + 36 + 64 + 16))


def test_every_case_sets_up():
    for c in CASES:
        if c.ndim > 112 and not (c.family == "iso" and c.tables == "full"):
            continue                                # (the recipe's matrices beyond: the GPU file builds them)
        d, nt, W, cov0, p0, kw, env, pieces = case_setup(c)
        assert p0.shape == (W, nt, d) and cov0.shape == (d, d) and set(env) <= set(HOOKS)
        assert (np.count_nonzero(cov0 - np.diag(np.diag(cov0))) == 0) == (c.tables == "diag")
        if c.prior == "box":
            assert (p0 > kw["logp"][1]).all() and (p0 < kw["logp"][2]).all()
        assert ("groups" in kw) == LAYOUTS[c.layout][1] and c.family == kw["logl"][0]
        assert sum(pieces) == (90 if d >= 256 else 260)


# ------------------------------------------------------------------------------------- the oracle's side of the matrix
def _one_per_layout():
    """One case per (class, layout, tables): a box cell with the full cycle where the layout has one."""
    seen, out = set(), []
    for want in (("box", "both"), ("flat", "both")):
        for c in CASES:
            k = (c.cls, c.layout, c.tables)
            if not c.extra and k not in seen and (c.prior, c.cycle) == want and c.ndim < 256:
                seen.add(k)
                out.append(c)
    return out


@pytest.mark.parametrize("case", _one_per_layout(), ids=case_id)
def test_oracle_run_is_not_idle(case):
    """The oracle's run of one case per layout meets what the GPU file asserts for every case: nothing there passes idle."""
    from oracle import oracle as orc
    o, kw, niter = run_oracle(case, orc)
    oracle_conditions(case, o, kw, niter)
    if case.prior == "box":
        box_did_bind(case, o, orc)
