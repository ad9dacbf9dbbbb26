#!/usr/bin/env python
"""What the sample buffer (PTEngine.with_stages(samples=...), csrc/ptmi_samples.hip) costs per covariance epoch, beside the statistics
pass that reads the same ring in the same epoch, what rate it moves its bytes at, and what it adds to a run's wall time.

    python tools/samples_timing.py [--shapes c2 c4 pw] [--epochs 6] [--slots 1024] [--every 10] [--wall] [--harvest] [--reps 5] [--out FILE]

Shapes: the cold rings of the benchmarked configurations, one temperature each (the stage and the statistics see the cold rank only)
  c2   4096 walkers x 1000 rows x 100-d, pooled covariance, am_mode "rle" (the headline configuration's ring; permuted rows)
  c4    512 walkers x 1000 rows x 1000-d, pooled (rle), device factorization
  pw   4096 walkers x 1000 rows x 100-d, per-walker covariances (every row stored), device QL
The buffer: --slots snapshots, a candidate every --every iterations (1024 and 10: every epoch takes 100 snapshots, none is let go
within the measured epochs).
Each shape is ONE ``rocprofv3 --kernel-trace --stats`` run of a child process of its own: a warm-up epoch, then --epochs covariance epochs
of a real SCAM run, each of which launches the stage's kernel (samples_gather) and then the statistics' (pool_rle + pool_syrk +
pool_reduce + pool_finish, or welford_rows) on the same ring.  Reported: median (min - max) over the epochs of the kernel times summed
per epoch, and the stage's bytes per second, 2 n W (d + 2) 8 / t (every word read once and written once).  The yardstick: the stage's
median should not exceed the statistics' median.
--wall: ``engine.run`` per 1000 iterations at the headline configuration (64 x 4096 x 100-d, SCAM, pooled, rle, eig_lag 1) with the stage
on and off, the two alternating in processes of their own, median (min - max) of 2 x --reps repeats each, each ending in a device
synchronise; no profiler.
--harvest: for context, the route the stage replaces -- the same configuration through ``PTSampler`` with ``keep_walkers = nwalkers`` and
``thin = every`` (every thinned row of every walker to the host and into a text file per walker), seconds per 1000 iterations."""
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
GATHER = "samples_gather_kernel"
STATS = ("pool_rle_kernel", "pool_syrk_kernel", "pool_reduce_kernel", "pool_finish_kernel", "welford_rows_kernel")


def make(d, nt, W, slots, every, on, **kw):
    from ptmcmcsampler_amd.engine import PTEngine
    kw = dict(dict(weights=(20, 0, 0), cov_update=CU, burn=10000, tskip=100, seed=1234, keep_lnl=True), **kw)
    if on:
        return PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, samples=dict(slots=slots, every=every), samples_from=0, **kw)
    return PTEngine(d, nt, W, np.eye(d) * 0.01, **kw)


def child_shape(name, epochs, slots, every):
    s = SHAPES[name]
    g = make(s["d"], 1, s["W"], slots, every, True, **s["kw"])
    taken, take = [], g._splan.take
    g._splan.take = lambda first, lo, hi: (lambda p: (taken.append(len(p)), p)[1])(take(first, lo, hi))      # pairs per call
    g.init_state(np.zeros(s["d"]))
    g.run((epochs + 1) * CU + 1)                                     # every epoch: the stage, then the statistics, on the period's ring
    g.sync()
    out = g.samples()
    assert len(out["iters"]) >= min(slots // 2, (g.iter // every)) and np.isfinite(out["x"]).all()
    fl = g.t["AMflag"]
    print(json.dumps(dict(shape=name, rle=bool(g.am_rle), stored=float((fl & 3).ne(0).double().mean().item()) if fl is not None else 1.0,
                          taken=taken, held=int(len(out["iters"])), stride=int(out["stride"]))), flush=True)


def child_wall(on, reps, slots, every):
    import torch
    g = make(100, 64, 4096, slots, every, on, cov_mode="pooled", am_mode="rle", eig_lag=1)
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


def child_harvest(niter, every):
    from ptmcmcsampler_amd import PTSampler
    d, W = 100, 4096
    out = tempfile.mkdtemp()
    s = PTSampler(d, ("iso",), ("flat",), np.eye(d) * 0.01, outDir=out, verbose=False, seed=1234, ntemps=64, nwalkers=W, keep_walkers=W,
                  cov_mode="pooled", checkpoint=False)
    t0 = time.perf_counter()
    s.sample(np.zeros(d), niter, burn=10000, thin=every, covUpdate=CU, isave=CU, Tskip=100, SCAMweight=20, AMweight=0, DEweight=0)
    s.engine.sync()
    sec = time.perf_counter() - t0
    names = [f for f in os.listdir(out) if f.startswith("chain_")]
    nbytes = sum(os.path.getsize(os.path.join(out, f)) for f in names)
    shutil.rmtree(out, ignore_errors=True)
    print(json.dumps(dict(sec=sec, niter=niter, files=len(names), bytes=nbytes)), flush=True)


def run_child(args, prefix=(), limit=300):
    # a limit of its own that reaches the profiled process too (the profiler's wrapper alone would leave it with the GPU open)
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("child %s failed (%d)" % (args, p.returncode))            # nothing more is started on the GPU behind it
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def epochs_of(db):
    """Per epoch (the first samples_gather launch behind a statistics kernel opens it): ns and launches of the stage's kernel, ns of the
    statistics' kernels."""
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    out, closed = [], True
    for name, t0, t1 in rows:
        if GATHER in name:
            if closed:
                out.append(dict(samples=0, launches=0, stats=0, names={}))
                closed = False
            out[-1]["samples"] += t1 - t0
            out[-1]["launches"] += 1
            continue
        if not out:
            continue
        e = out[-1]
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
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--harvest", action="store_true")
    ap.add_argument("--harvest-iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "wall":
            return child_wall(a.child[1] == "on", int(a.child[2]), int(a.child[3]), int(a.child[4]))
        if a.child[0] == "harvest":
            return child_harvest(int(a.child[1]), int(a.child[2]))
        return child_shape(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                                     # line by line: a leg that fails later loses nothing
            open(a.out, "w").write("\n".join(lines) + "\n")

    if a.epochs < 5:
        raise SystemExit("--epochs: at least five")
    say("sample buffer (%d slots, a candidate every %d iterations) beside the statistics pass of the same epochs: kernel time per covariance "
        "epoch, median (min - max) of %d epochs behind a warm-up epoch, one rocprofv3 --kernel-trace --stats run per shape"
        % (a.slots, a.every, a.epochs))
    for name in a.shapes:
        s = SHAPES[name]
        out = tempfile.mkdtemp()
        r = run_child([name, a.epochs, a.slots, a.every], prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", name, "--"])
        dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_results.db")]
        try:
            ep = epochs_of(dbs[0])
        except (IndexError, sqlite3.Error) as e:                      # the trace database alone: missing, or another layout
            say("%s: not measured (%s: %s)" % (name, type(e).__name__, e))
            continue
        finally:
            shutil.rmtree(out, ignore_errors=True)
        taken = [n for n in r["taken"] if n > 0]                      # pairs of every call that launched, in the epochs' order
        if len(taken) != len(ep):
            say("%s: not measured (%d calls that took snapshots, %d epochs in the trace)" % (name, len(taken), len(ep)))
            continue
        for e, n in zip(ep, taken):
            e["n"] = n
        ep = [e for e in ep[1:] if e["stats"] > 0]                    # (the first epoch is the warm-up; the last call has no statistics beside it)
        smp, stats = [e["samples"] for e in ep], [e["stats"] for e in ep]
        rate = [2.0 * e["n"] * s["W"] * (s["d"] + 2) * 8 / (e["samples"] * 1e-9) / 1e12 for e in ep]
        say("%s: %d walkers x %d rows x %d-d, %s, %.0f %% of the rows stored, %s snapshots an epoch in %s launches, %d held at stride %d, %d epochs"
            % (name, s["W"], CU, s["d"], "pooled rle" if r["rle"] else "per-walker rows", 100 * r["stored"],
               "/".join(str(v) for v in sorted({e["n"] for e in ep})), "/".join(str(v) for v in sorted({e["launches"] for e in ep})),
               r["held"], r["stride"], len(ep)))
        say("  sample buffer    %s" % fmt(smp))
        say("  statistics       %s" % fmt(stats))
        for k in sorted({k for e in ep for k in e["names"]}):
            say("    %-30s %s" % (k, fmt([e["names"][k] for e in ep if k in e["names"]])))
        say("  bytes moved      %9.2f (%.2f - %.2f) TB/s   (2 n W (d + 2) 8 bytes over the stage's kernel time)" % (np.median(rate), min(rate), max(rate)))
        say("  yardstick (sample buffer <= statistics, medians): %s" % ("met" if np.median(smp) <= np.median(stats) else "MISSED"))
    if a.wall:
        on, off = [], []
        for _ in range(2):                                            # stage off and on alternating
            off += run_child(["wall", "off", a.reps, a.slots, a.every])["ms"]
            on += run_child(["wall", "on", a.reps, a.slots, a.every])["ms"]
        f = lambda ms: "%8.1f (%.1f - %.1f) ms" % (np.median(ms), min(ms), max(ms))      # noqa: E731
        say("engine.run per 1000 iterations, 64 x 4096 x 100-d, SCAM, pooled rle, eig_lag 1, %d repeats each:" % len(on))
        say("  stage off   %s" % f(off))
        say("  stage on    %s   (%+.2f ms per 1000 iterations)" % (f(on), float(np.median(on)) - float(np.median(off))))
    if a.harvest:
        r = run_child(["harvest", a.harvest_iters, a.every], limit=900)
        say("for context, the route the stage replaces: PTSampler, 64 x 4096 x 100-d, keep_walkers = 4096, thin = %d: %.1f s per %d iterations "
            "(%d chain files, %.0f MB of text)" % (a.every, r["sec"], r["niter"], r["files"], r["bytes"] / 1e6))


if __name__ == "__main__":
    main()
