#!/usr/bin/env python
"""Where a wave of the persistent SCAM kernel spends its life: table staging, unit headers, steps, unit exits.

    tools/unit_stamps.py --build                  # compiles ab/libptmi_stamps.so (-DPTMI_UNIT_STAMPS), needs hipcc only
    tools/unit_stamps.py [--out FILE]             # runs the plain bench shape on that library and prints the report

The diagnostic library is a private copy of the shipped one whose persistent step kernel reads the clock (s_memtime) at launch
entry, behind the table staging's barrier and four times per unit of 16 chains -- unit entry; behind the header, when x, lnL, lp
have arrived and the chain's constants are computed; behind the last step; behind the exit stores -- into a buffer of its own
(csrc/ptmi_common.h PTMI_STAMP_WAVE).  The stamps are fenced, so the build's run time is not the shipped kernel's: read the SHARES.
Reported, in clock ticks, over all waves of the last launch: the medians of header, steps and exit for cold and for hot units, the
staging, the share of header + exit + staging in a wave's life, the skew between the two waves of a SIMD (waves j and j + 4 of a
block) at every unit entry and at their ends, the blocks' lives, the units (cold, hot) each half of a block served, and the steps of a
unit by wave class and by what the SIMD's partner wave was in meanwhile: a cold unit, a hot unit, or gone."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "ab", "libptmi_stamps.so")
UNITS, WAVES = 16, 8 * 1024           # csrc/ptmi_common.h PTMI_STAMP_UNITS, PTMI_STAMP_WAVES
WORDS = 2 + 5 * UNITS


def build():
    from ptmcmcsampler_amd import _build
    _build.OBJ = os.path.join(ROOT, "ab", "stamps_obj")
    _build.OUT = LIB
    _build.FLAGS = _build.FLAGS + ["-DPTMI_UNIT_STAMPS"]
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    print(_build.build(force=True, verbose=True))


def report(st, W, cold_first, out):
    import numpy as np
    st = st.reshape(WAVES, WORDS).astype(np.int64)
    nw = int((st[:, 0] != 0).sum())
    st = st[:nw]
    t_in, t_staged = st[:, 0], st[:, 1]
    u = st[:, 2:].reshape(nw, UNITS, 5)
    # the buffer is not cleared between launches, and a wave serves another number of units in every launch: a wave's units of the last
    # launch are the leading ones that follow each other directly (entry within GAP ticks behind the staging or the exit before it; a
    # stamp left by an earlier launch is older, or from another XCD's clock)
    GAP = 50000
    prev = np.concatenate([t_staged[:, None], u[:, :-1, 3]], axis=1)
    n_units = np.cumprod((u[:, :, 0] >= prev) & (u[:, :, 0] - prev < GAP), axis=1).sum(1)
    on = np.arange(UNITS)[None, :] < n_units[:, None]
    header, steps, exit_ = u[:, :, 1] - u[:, :, 0], u[:, :, 2] - u[:, :, 1], u[:, :, 3] - u[:, :, 2]
    cold = on & (u[:, :, 4] < W) & cold_first
    hot = on & ~cold
    end = u[np.arange(nw), np.maximum(n_units, 1) - 1, 3]
    life = end - t_in
    staging = t_staged - t_in
    between = np.where(on[:, 1:], u[:, 1:, 0] - u[:, :-1, 3], 0)             # exit stamp -> next entry stamp: the cost of a stamp pair

    def med(v, m=None):
        v = v[m] if m is not None else v
        return "n=0" if v.size == 0 else "median %8d   p10 %8d   p90 %8d   (n=%d)" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90), v.size)

    p = lambda s="": print(s, file=out)       # noqa: E731
    p("waves %d, units per wave %d..%d, cold-first %s; clock ticks of s_memtime" % (nw, n_units.min(), n_units.max(), bool(cold_first)))
    p("wave life (launch entry -> last exit)   %s" % med(life))
    p("table staging (entry -> behind barrier) %s" % med(staging))
    for name, m in (("cold", cold), ("hot", hot)):
        p("%-4s units: header  %s" % (name, med(header, m)))
        p("%-4s units: steps   %s" % (name, med(steps, m)))
        p("%-4s units: exit    %s" % (name, med(exit_, m)))
    p("exit stamp -> next entry stamp          %s" % med(between[on[:, 1:]]))
    hdr_w, exit_w = np.where(on, header, 0).sum(1), np.where(on, exit_, 0).sum(1)
    for name, v in (("staging", staging), ("headers", hdr_w), ("exits", exit_w), ("staging + headers + exits", staging + hdr_w + exit_w)):
        p("share of a wave's life: %-26s median %.3f %%   p90 %.3f %%" % (name, 100 * np.median(v / life), 100 * np.percentile(v / life, 90)))
    # the two waves of a SIMD: waves j and j + 4 of a block of eight
    blk = (nw // 8) * 8
    e = u[:blk, :, 0].reshape(-1, 2, 4, UNITS)
    o = on[:blk].reshape(-1, 2, 4, UNITS)
    for i in range(int(n_units.max())):
        both = o[:, 0, :, i] & o[:, 1, :, i]
        if both.any():
            p("skew of a SIMD's two waves at the entry of unit %2d: |dt| %s" % (i, med(np.abs(e[:, 0, :, i] - e[:, 1, :, i])[both])))
    en = end[:blk].reshape(-1, 2, 4)
    p("skew of a SIMD's two waves at their ends:            |dt| %s" % med(np.abs(en[:, 0] - en[:, 1]).reshape(-1)))
    p("a block's last wave ends behind its first by              %s" % med(end[:blk].reshape(-1, 8).max(1) - end[:blk].reshape(-1, 8).min(1)))
    # (the clocks of different XCDs are not aligned: blocks are compared by their lengths, not by their stamps)
    bl = end[:blk].reshape(-1, 8).max(1) - t_in[:blk].reshape(-1, 8).min(1)
    p("a block's life (first entry -> last end)                  %s   max %d" % (med(bl), bl.max()))
    p("units served per wave: waves 0-3 %s" % med(n_units[:blk].reshape(-1, 2, 4)[:, 0].reshape(-1)))
    p("units served per wave: waves 4-7 %s" % med(n_units[:blk].reshape(-1, 2, 4)[:, 1].reshape(-1)))
    # cold and hot units by wave class, and the steps of a unit by what the SIMD's partner wave did meanwhile: the state (in a cold
    # unit, in a hot unit, gone: behind its last exit) that covers most of the unit's steps
    cls = ("waves 0-3", "waves 4-7")
    cu, hu = cold[:blk].reshape(-1, 2, 4, UNITS), hot[:blk].reshape(-1, 2, 4, UNITS)
    for h in (0, 1):
        p("cold units served per wave: %s %s" % (cls[h], med(cu[:, h].sum(-1).reshape(-1))))
        p("hot  units served per wave: %s %s" % (cls[h], med(hu[:, h].sum(-1).reshape(-1))))
    t0, t1 = u[:blk, :, 1].reshape(-1, 2, 4, UNITS), u[:blk, :, 2].reshape(-1, 2, 4, UNITS)          # a unit's steps
    p0, p3 = u[:blk, :, 0].reshape(-1, 2, 4, UNITS), u[:blk, :, 3].reshape(-1, 2, 4, UNITS)          # a unit from entry to exit
    pend = end[:blk].reshape(-1, 2, 4)
    st_ = steps[:blk].reshape(-1, 2, 4, UNITS)
    for h in (0, 1):
        q = 1 - h                                                          # the partner's half of the block
        ov = np.zeros((3,) + t0[:, h].shape, dtype=np.int64)               # overlap with the partner cold / hot / gone
        for k in range(UNITS):
            lap = np.maximum(np.minimum(t1[:, h], p3[:, q, :, k, None]) - np.maximum(t0[:, h], p0[:, q, :, k, None]), 0)
            ov[0] += np.where(cu[:, q, :, k, None], lap, 0)
            ov[1] += np.where(hu[:, q, :, k, None], lap, 0)
        ov[2] = np.maximum(t1[:, h] - np.maximum(t0[:, h], pend[:, q, :, None]), 0)
        state = ov.argmax(0)
        for kind, mine in (("cold", cu[:, h]), ("hot", hu[:, h])):
            for si, sname in enumerate(("cold", "hot", "gone")):
                p("%s, %-4s unit, partner %-4s: steps  %s" % (cls[h], kind, sname, med(st_[:, h], mine & (state == si))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--build", action="store_true", help="compile the diagnostic library and stop")
    ap.add_argument("--out", default=None, help="write the report here as well")
    ap.add_argument("--ndim", type=int, default=100)
    ap.add_argument("--ntemps", type=int, default=64)
    ap.add_argument("--nwalkers", type=int, default=4096)
    ap.add_argument("--prior", default="flat", choices=["flat", "box"])
    ap.add_argument("--iters", type=int, default=3000, help="iterations before the stamped launch is read (launches of 100, swaps, covariance epochs)")
    a = ap.parse_args()
    if a.build:
        return build()
    if not os.path.exists(LIB):
        raise SystemExit("%s is missing: tools/unit_stamps.py --build" % LIB)
    os.environ["PTMI_LIB"] = LIB                                  # before the package loads its library
    import numpy as np
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    L = _lib.load()
    L.ptmi_unit_stamps.argtypes = [C.c_void_p, C.c_size_t]
    d, nt, W = a.ndim, a.ntemps, a.nwalkers
    kw = dict(weights=(20, 0, 0), cov_update=1000, burn=10000, tskip=100, seed=1234, cov_mode="pooled", eig_lag=1)     # bench.py's plain line
    if a.prior == "box":
        kw.update(logp=("box", np.full(d, -10.0), np.full(d, 10.0)))
    eng = PTEngine(d, nt, W, np.eye(d) * 0.01, **kw)
    eng.init_state(np.zeros(d))
    eng.run(a.iters)
    eng.sync()
    flags, G, E = eng.last_variant()
    assert flags & _lib.VAR_PERSISTENT, "the launch did not take the persistent kernel"
    st = np.zeros(WAVES * WORDS, dtype=np.uint64)
    _lib.check(L.ptmi_unit_stamps(st.ctypes.data, st.nbytes))
    cold_first = eng.owns_cold and nt % 16 == 0
    outs = [sys.stdout] + ([open(a.out, "w")] if a.out else [])
    for o in outs:
        print("tools/unit_stamps.py: ndim %d, %d ranks x %d walkers, %s prior, shape (%d, %d), the last launch (100 iterations) of a run of %d" % (
            d, nt, W, a.prior, G, E, a.iters), file=o)
        report(st, W, cold_first, o)


if __name__ == "__main__":
    main()
