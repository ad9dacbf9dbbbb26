#!/usr/bin/env python
"""What the pair histograms (PTEngine.with_stages(pairs=...), csrc/ptmi_pairs.hip) cost per covariance epoch, beside the statistics
pass that reads the same ring in the same epoch and beside the 1-D histograms, and what they add to a run's wall time.

    python tools/pairs_timing.py [--shapes c2 c4 pw] [--epochs 6] [--nbins 32] [--params 10] [--wall] [--reps 5] [--out FILE]

Shapes: the cold rings of the benchmarked configurations, one temperature each (the stages and the statistics see the cold rank only)
  c2   4096 walkers x 1000 rows x 100-d, pooled covariance, am_mode "rle" (the headline configuration's ring; permuted rows)
  c4    512 walkers x 1000 rows x 1000-d, pooled (rle), device factorization
  pw   4096 walkers x 1000 rows x 100-d, per-walker covariances (every row stored), device QL
The pairs: all pairs of --params parameters spread over the row (10 -> 45 pairs) at --nbins bins an axis.
Each shape is ONE ``rocprofv3 --kernel-trace --stats`` run of a child process of its own: a warm-up epoch, then --epochs covariance epochs
of a real SCAM run, each of which launches the 1-D stage's kernels (hist_weight + hist_rows, for context), the pair stage's (hist_weight
+ pairs_rows) and then the statistics' (pool_rle + pool_syrk + pool_reduce + pool_finish, or welford_rows) on the same ring.  Reported:
median (min - max) over the epochs of the kernel times summed per epoch.  The yardstick: the pair stage's median should not exceed
the statistics' median.
--wall: ``engine.run`` per 1000 iterations at the headline configuration (64 x 4096 x 100-d, SCAM, pooled, rle, eig_lag 1) with the pair
stage on and off, the two alternating in processes of their own, median (min - max) of 2 x --reps repeats each, each ending in a device
synchronise; no profiler."""
import argparse
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CU = 1000
SHAPES = {
    "c2": dict(d=100, W=4096, kw=dict(cov_mode="pooled", am_mode="rle")),
    "c4": dict(d=1000, W=512, kw=dict(cov_mode="pooled", am_mode="rle", eig_mode="sytrd")),
    "pw": dict(d=100, W=4096, kw=dict(cov_mode="per_walker", eig_mode="ql")),
}
WEIGHT, HIST, PAIRS = "hist_weight_kernel", "hist_rows_kernel", "pairs_rows_kernel"
STATS = ("pool_rle_kernel", "pool_syrk_kernel", "pool_reduce_kernel", "pool_finish_kernel", "welford_rows_kernel")


def params_of(d, k):
    """k parameters spread over the row, both ends included."""
    return [int(v) for v in np.unique(np.linspace(0, d - 1, k).round().astype(int))]


def make(d, nt, W, nbins, k, pairs_on, hist_on, **kw):
    from ptmcmcsampler_amd.engine import PTEngine
    kw = dict(dict(weights=(20, 0, 0), cov_update=CU, burn=10000, tskip=100, seed=1234), **kw)
    # a Gaussian of unit width: the bins cover what the chains visit
    if pairs_on:
        kw.update(pairs=({"params": params_of(d, k)}, -4.0, 4.0, nbins), pairs_from=0)
    if hist_on:
        kw.update(hist=(-4.0, 4.0, 64), hist_from=0)
    if pairs_on or hist_on:
        return PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, **kw)
    return PTEngine(d, nt, W, np.eye(d) * 0.01, **kw)


def child_shape(name, epochs, nbins, k):
    s = SHAPES[name]
    g = make(s["d"], 1, s["W"], nbins, k, True, True, **s["kw"])
    g.init_state(np.zeros(s["d"]))
    g.run((epochs + 1) * CU + 1)                                     # every epoch: the stages, then the statistics, on the period's ring
    g.sync()
    h = g.pairs_counts()
    total = h["counts"].sum((1, 2)) + h["outside"]
    assert (total == s["W"] * g.pairs_iter).all(), (total, g.pairs_iter)
    fl = g.t["AMflag"]
    print(json.dumps(dict(shape=name, rle=bool(g.am_rle), stored=float((fl & 3).ne(0).double().mean().item()) if fl is not None else 1.0,
                          npairs=int(len(total)), inside=float(h["counts"].sum()) / float(total.sum()),
                          cells=float((h["counts"] > 0).mean()))), flush=True)


def child_wall(on, reps, nbins, k):
    import torch
    g = make(100, 64, 4096, nbins, k, on, False, cov_mode="pooled", am_mode="rle", eig_lag=1)
    g.init_state(np.zeros(100))
    g.run(CU + 1)
    g.sync()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.run(CU)
        g.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(on=on, ms=ms)), flush=True)


def run_child(args, prefix=()):
    # a limit of its own that reaches the profiled process too (the profiler's wrapper alone would leave it with the GPU open)
    cmd = ["timeout", "-k", "10", "300"] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("child %s failed (%d)" % (args, p.returncode))            # nothing more is started on the GPU behind it
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def epochs_of(db):
    """Per epoch (the first hist_weight_kernel launch behind a statistics kernel opens it): ns of the 1-D stage's kernels, of the pair
    stage's and of the statistics' kernels.  A weight launch belongs to the stage whose rows kernel follows it."""
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    out, weight, closed = [], 0, True
    for name, t0, t1 in rows:
        if WEIGHT in name:
            if closed:
                out.append(dict(hist=0, pairs=0, stats=0, names={}))
                closed = False
            weight = t1 - t0
            continue
        if not out:
            continue
        e = out[-1]
        for key, k in (("hist", HIST), ("pairs", PAIRS)):
            if k in name:
                e[key] += t1 - t0 + weight
                e["names"][k] = e["names"].get(k, 0) + (t1 - t0)
                e["names"][WEIGHT + " (" + key + ")"] = weight
                weight = 0
        for k in STATS:
            if k in name:
                e["stats"] += t1 - t0
                e["names"][k] = e["names"].get(k, 0) + (t1 - t0)
                closed = True
    return out


def fmt(ns):
    us = np.asarray(ns, dtype=np.float64) / 1e3
    return "%9.1f (%.1f - %.1f) us" % (np.median(us), us.min(), us.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--shapes", nargs="*", default=["c2", "c4", "pw"])
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--nbins", type=int, default=32)
    ap.add_argument("--params", type=int, default=10)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "wall":
            return child_wall(a.child[1] == "on", int(a.child[2]), int(a.child[3]), int(a.child[4]))
        return child_shape(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                                     # line by line: a leg that fails later loses nothing
            open(a.out, "w").write("\n".join(lines) + "\n")

    if a.epochs < 5:
        raise SystemExit("--epochs: at least five")
    say("pair histograms (all pairs of %d parameters, %d bins an axis) beside the statistics pass and the 1-D histograms (64 bins) of the same "
        "epochs: kernel time per covariance epoch, median (min - max) of %d epochs behind a warm-up epoch, one rocprofv3 --kernel-trace "
        "--stats run per shape" % (a.params, a.nbins, a.epochs))
    for name in a.shapes:
        s = SHAPES[name]
        out = tempfile.mkdtemp()
        r = run_child([name, a.epochs, a.nbins, a.params], prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", name, "--"])
        dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_results.db")]
        try:
            ep = epochs_of(dbs[0])[1:]                                # (the first epoch is the warm-up)
        except (IndexError, sqlite3.Error) as e:                      # the trace database alone: missing, or another layout
            say("%s: not measured (%s: %s)" % (name, type(e).__name__, e))
            continue
        ep = [e for e in ep if e["stats"] > 0]                        # (the launch of pairs_counts at the end has no statistics beside it)
        pairs, hist, stats = [e["pairs"] for e in ep], [e["hist"] for e in ep], [e["stats"] for e in ep]
        gb = s["W"] * CU * s["d"] * 8 * r["stored"] / 1e9
        say("%s: %d walkers x %d rows x %d-d, %s, %.0f %% of the rows stored (%.2f GB), %d pairs, %.1f %% of the samples inside the bins "
            "in %.1f %% of the cells, %d epochs" % (name, s["W"], CU, s["d"], "pooled rle" if r["rle"] else "per-walker rows", 100 * r["stored"],
                                                  gb, r["npairs"], 100 * r["inside"], 100 * r["cells"], len(ep)))
        say("  pair histograms  %s" % fmt(pairs))
        say("  statistics       %s" % fmt(stats))
        say("  1-D histograms   %s" % fmt(hist))
        for k in sorted({k for e in ep for k in e["names"]}):
            say("    %-30s %s" % (k, fmt([e["names"][k] for e in ep if k in e["names"]])))
        say("  yardstick (pair histograms <= statistics, medians): %s" % ("met" if np.median(pairs) <= np.median(stats) else "MISSED"))
    if a.wall:
        on, off = [], []
        for _ in range(2):                                            # stage off and on alternating
            off += run_child(["wall", "off", a.reps, a.nbins, a.params])["ms"]
            on += run_child(["wall", "on", a.reps, a.nbins, a.params])["ms"]
        f = lambda ms: "%8.1f (%.1f - %.1f) ms" % (np.median(ms), min(ms), max(ms))      # noqa: E731
        say("engine.run per 1000 iterations, 64 x 4096 x 100-d, SCAM, pooled rle, eig_lag 1, %d repeats each:" % len(on))
        say("  stage off   %s" % f(off))
        say("  stage on    %s   (%+.2f ms per 1000 iterations)" % (f(on), float(np.median(on)) - float(np.median(off))))


if __name__ == "__main__":
    main()
