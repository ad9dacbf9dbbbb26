#!/usr/bin/env python
"""What the best-fit tracker (PTEngine.with_stages(best=True), csrc/ptmi_best.hip) costs per covariance epoch, beside the statistics pass
that reads the same ring in the same epoch, what rate it reads its bytes at, and what it adds to a run's wall time.

    python tools/best_timing.py [--shapes c2 c4 pw] [--epochs 6] [--wall] [--reps 5] [--out FILE]

Shapes: the cold rings of the benchmarked configurations, one temperature each (the stage and the statistics see the cold rank only)
  c2   4096 walkers x 1000 rows x 100-d, pooled covariance, am_mode "rle" (the headline configuration's ring; permuted rows)
  c4    512 walkers x 1000 rows x 1000-d, pooled (rle), device factorization
  pw   4096 walkers x 1000 rows x 100-d, per-walker covariances (every row stored), device QL
Each shape is ONE ``rocprofv3 --kernel-trace --stats`` run of a child process of its own: a warm-up epoch, then --epochs covariance epochs
of a real SCAM run started far from the mode (so that walkers go on improving and the kernel's copy path runs), each of which launches the stage's kernel (best_rows) and then the statistics' (pool_rle + pool_syrk + pool_reduce +
pool_finish, or welford_rows) on the same ring.  Reported: median (min - max) over the epochs of the kernel times summed per epoch, and
the stage's bytes read per second, 16 W cov_update / t (lnL and lp of every iteration; the rows it copies where a walker improves are
at most 2 W (ndim + 4) 8 bytes more).  The yardstick: the stage's median should not exceed the statistics' median.
--wall: ``engine.run`` per 1000 iterations at the headline configuration (64 x 4096 x 100-d, SCAM, pooled, rle, eig_lag 1) with the stage
on and off, the two alternating in processes of their own, median (min - max) of 2 x --reps repeats each, each ending in a device
synchronise; no profiler.  Every GPU step is a child process under a ``timeout`` of its own; a child that fails ends the tool."""
import argparse
import json
import os
import shutil
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
BEST = "best_rows_kernel"
STATS = ("pool_rle_kernel", "pool_syrk_kernel", "pool_reduce_kernel", "pool_finish_kernel", "welford_rows_kernel")


def make(d, nt, W, on, **kw):
    from ptmcmcsampler_amd.engine import PTEngine
    kw = dict(dict(weights=(20, 0, 0), cov_update=CU, burn=10000, tskip=100, seed=1234, keep_lnl=True), **kw)
    if on:
        return PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, best=True, **kw)
    return PTEngine(d, nt, W, np.eye(d) * 0.01, **kw)


def child_shape(name, epochs):
    s = SHAPES[name]
    g = make(s["d"], 1, s["W"], True, **s["kw"])
    g.init_state(np.full(s["d"], 3.0))                               # far from the mode: the chains climb, so walkers improve in every epoch and copy rows
    g.run((epochs + 1) * CU + 1)                                     # every epoch: the stage, then the statistics, on the period's ring
    g.sync()
    out = g.best(per_walker=True)
    assert (out["iters"] >= 1).all() and np.isfinite(out["x"]).all() and np.isfinite(out["val"]).all()
    fl = g.t["AMflag"]
    print(json.dumps(dict(shape=name, rle=bool(g.am_rle), stored=float((fl & 3).ne(0).double().mean().item()) if fl is not None else 1.0,
                          iter_map=int(out["iter_map"]), lnprob_map=float(out["lnprob_map"]),
                          last_period=float((out["iters"] > epochs * CU).mean()))), flush=True)


def child_wall(on, reps):
    import torch
    g = make(100, 64, 4096, on, cov_mode="pooled", am_mode="rle", eig_lag=1)
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


def run_child(args, prefix=(), limit=300):
    # a limit of its own that reaches the profiled process too (the profiler's wrapper alone would leave it with the GPU open)
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("child %s failed (%d)" % (args, p.returncode))            # nothing more is started on the GPU behind it
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def epochs_of(db):
    """Per epoch (a best_rows launch opens it): ns of the stage's kernel, ns of the statistics' kernels behind it."""
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    out = []
    for name, t0, t1 in rows:
        if BEST in name:
            out.append(dict(best=t1 - t0, stats=0, names={}))
            continue
        if not out:
            continue
        e = out[-1]
        for k in STATS:
            if k in name:
                e["stats"] += t1 - t0
                e["names"][k] = e["names"].get(k, 0) + (t1 - t0)
    return out


def fmt(ns):
    us = np.asarray(ns, dtype=np.float64) / 1e3
    return "%9.1f (%.1f - %.1f) us" % (np.median(us), us.min(), us.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--shapes", nargs="*", default=["c2", "c4", "pw"])
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "wall":
            return child_wall(a.child[1] == "on", int(a.child[2]))
        return child_shape(a.child[0], int(a.child[1]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                                     # line by line: a leg that fails later loses nothing
            open(a.out, "w").write("\n".join(lines) + "\n")

    if a.epochs < 5:
        raise SystemExit("--epochs: at least five")
    if a.shapes:
        say("best-fit tracker beside the statistics pass of the same epochs: kernel time per covariance epoch, median (min - max) of %d epochs "
            "behind a warm-up epoch, one rocprofv3 --kernel-trace --stats run per shape" % a.epochs)
    for name in a.shapes:
        s = SHAPES[name]
        out = tempfile.mkdtemp()
        r = run_child([name, a.epochs], prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", name, "--"])
        dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_results.db")]
        try:
            ep = epochs_of(dbs[0])
        except (IndexError, sqlite3.Error) as e:                      # the trace database alone: missing, or another layout
            say("%s: not measured (%s: %s)" % (name, type(e).__name__, e))
            continue
        finally:
            shutil.rmtree(out, ignore_errors=True)
        ep = [e for e in ep[1:] if e["stats"] > 0]                    # (the first epoch is the warm-up; the last call has no statistics beside it)
        if len(ep) < a.epochs - 1:
            say("%s: not measured (%d epochs with statistics in the trace)" % (name, len(ep)))
            continue
        best, stats = [e["best"] for e in ep], [e["stats"] for e in ep]
        rate = [16.0 * s["W"] * CU / (e["best"] * 1e-9) / 1e12 for e in ep]
        say("%s: %d walkers x %d rows x %d-d, %s, %.0f %% of the rows stored, %d epochs; %.0f %% of the held rows (MAP and ML) were found in the "
            "last period" % (name, s["W"], CU, s["d"], "pooled rle" if r["rle"] else "per-walker rows", 100 * r["stored"], len(ep),
                        100 * r["last_period"]))
        say("  best-fit tracker %s" % fmt(best))
        say("  statistics       %s" % fmt(stats))
        for k in sorted({k for e in ep for k in e["names"]}):
            say("    %-30s %s" % (k, fmt([e["names"][k] for e in ep if k in e["names"]])))
        say("  bytes read       %9.2f (%.2f - %.2f) TB/s   (16 W cov_update bytes over the stage's kernel time)" % (np.median(rate), min(rate), max(rate)))
        say("  yardstick (best-fit tracker <= statistics, medians): %s" % ("met" if np.median(best) <= np.median(stats) else "MISSED"))
    if a.wall:
        on, off = [], []
        for _ in range(2):                                            # stage off and on alternating
            off += run_child(["wall", "off", a.reps])["ms"]
            on += run_child(["wall", "on", a.reps])["ms"]
        f = lambda ms: "%8.1f (%.1f - %.1f) ms" % (np.median(ms), min(ms), max(ms))      # noqa: E731
        diff = float(np.median(on)) - float(np.median(off))
        inside = abs(diff) <= max(max(off) - min(off), max(on) - min(on))      # within either leg's own spread
        say("engine.run per 1000 iterations, 64 x 4096 x 100-d, SCAM, pooled rle, eig_lag 1, %d repeats each:" % len(on))
        say("  stage off   %s" % f(off))
        say("  stage on    %s   (%+.2f ms per 1000 iterations: %s the spread of a leg)" % (f(on), diff, "inside" if inside else "outside"))


if __name__ == "__main__":
    main()
