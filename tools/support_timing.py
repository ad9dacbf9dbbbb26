#!/usr/bin/env python
"""What the support stage (PTEngine.with_stages(logl_in_support=True), csrc/ptmi_sup.hip) costs and gains on the callback path: ms per 100
iterations, median (min - max) of --reps repeats after a warm-up, each ending in a device synchronise.

    python tools/support_timing.py [--parent-lib PATH] [--legs off price gain yardstick] [--reps 5] [--profile] [--out FILE]

Legs:
  off        64 temperatures x 4096 walkers x 100-d, ``builtin_logl`` / ``builtin_logp`` with a box nobody leaves, stage OFF -- with
             --parent-lib also on that build of the library (PTMI_LIB), the two builds alternating: the off path gains one Python branch;
  price      the same run with the stage ON and every row inside the support: the listing (count, scan, rank) and the read-back per
             iteration, nothing saved;
  gain       dense 1000-d, 64 x 256, ``rows_logl=True`` with boxes of three widths, so that three different shares of the proposals fall
             outside: stage on against off, with the share the stage reports; and the break-even share (the price leg's cost per
             iteration / time of the likelihood; "not measured" without the off and price legs);
  yardstick  the stage's kernels against their restatement in torch in one process on the same masks, one synchronisation each:
             ``idx = nonzero(lp != -inf)``, ``rows_in[idx]``, ``out.fill_(-inf); out[idx] = vals``.
Every engine measurement is a child process of its own (PTMI_LIB is read at import).  --profile: the price leg once more under
``rocprofv3 --kernel-trace --stats`` in a run of its own, its kernels summed by name."""
import argparse
import ctypes as C
import json
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, ITERS = 120, 100
# half-widths of the gain leg's boxes.  With the jump covariance 0.01 I a cold SCAM step moves one coordinate by about
# 2.4 / sqrt(2) * 0.1 = 0.17 (hot ranks further): from a start uniform in the box, roughly a step, three steps and nine steps wide --
# three different out-of-support shares, which the stage itself reports
GAIN_BOXES = (0.2, 0.5, 1.5)


def engine(leg, on, box=None):
    from ptmcmcsampler_amd.engine import PTEngine
    rs = np.random.RandomState(3)
    if leg in ("off", "price"):
        d, nt, W = 100, 64, 4096
        kw = dict(logp=("box", -1e3 * np.ones(d), 1e3 * np.ones(d)), split=True, weights=(20, 0, 20), cov_update=1000, burn=100, tskip=100,
                  seed=5, cov_mode="pooled", am_mode="rows")
        p0 = rs.randn(W, nt, d) * 0.3
    else:
        d, nt, W = 1000, 64, 256
        A = rs.randn(d, d)
        P = np.linalg.inv(A @ A.T / d + 0.3 * np.eye(d))
        kw = dict(logl=("dense", np.zeros(d), (P + P.T) / 2), logp=("box", -box * np.ones(d), box * np.ones(d)), rows_logl=True,
                  weights=(20, 0, 20), cov_update=1000, burn=100, tskip=100, seed=5, cov_mode="pooled", am_mode="rows")
        p0 = (2 * rs.rand(W, nt, d) - 1) * box
    if on is None:                                                    # the parent build: no keyword at all
        return PTEngine(d, nt, W, np.eye(d) * 0.01, **kw), p0
    return PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, logl_in_support=on, **kw), p0


def child(leg, on, reps, box=None):
    import torch
    from ptmcmcsampler_amd import _lib
    g, p0 = engine(leg, on, box)
    if g.rows_logl:
        logl, logp = g._rows_callbacks()[:2]
    else:
        logl, logp = g.builtin_logl(), g.builtin_logp()
    g.init_state_callback(p0, logl, logp)
    g.run_callback(WARMUP, logl, logp)
    g.sync()
    _lib.check(g.lib.ptmi_set_device_iter(g.h, 0))               # a marker launch: the timed region starts behind it
    c0 = getattr(g, "support_counts", (0, 0))
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.run_callback(ITERS, logl, logp)
        g.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    c1 = getattr(g, "support_counts", (0, 0))
    # the likelihood alone over all rows, for the break-even share
    X = g.t["X"].view(-1, g.d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        logl(X)
    torch.cuda.synchronize()
    logl_ms = (time.perf_counter() - t0) * 1e3 / 20
    print(json.dumps(dict(leg=leg, on=on, lib=os.path.basename(os.path.dirname(_lib.SO)) + "/" + os.path.basename(_lib.SO), ms=ms,
                          offered=c1[0] - c0[0], given=c1[1] - c0[1], logl_ms=logl_ms,
                          accept=float(g.get("nacc").sum()) / (g.W * g.nt * g.iter))), flush=True)


def yardstick(reps):
    """The stage's three calls against the torch form on the same masks, in this process; each side synchronises once per pass (the
    read-back of n / nonzero's own)."""
    import torch
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    out = []
    for d, n_in in ((100, 262144), (1000, 16384)):
        g = PTEngine(d, 2, 2, np.eye(d) * 0.01, weights=(20, 0, 0), split=True)
        L, h = g.lib, g.h
        nb = C.c_size_t(0)
        _lib.check(L.ptmi_sup_work_bytes(h, n_in, C.byref(nb)))
        work = torch.empty(nb.value, dtype=torch.uint8, device=g.device)
        rows_in = torch.randn((n_in, d), dtype=torch.float64, device=g.device)
        rows = torch.empty_like(rows_in)
        res = torch.empty(n_in, dtype=torch.float64, device=g.device)
        for share in (0.0, 0.25, 0.5):
            lp = torch.where(torch.rand(n_in, device=g.device) < share, -float("inf"), 0.0).to(torch.float64)
            vals = torch.randn(n_in, dtype=torch.float64, device=g.device)
            n = C.c_int64(0)

            def hand():
                _lib.check(L.ptmi_sup_begin(h, work.data_ptr(), lp.data_ptr(), n_in, C.byref(n)))
                if 0 < n.value < n_in:
                    _lib.check(L.ptmi_sup_rows(h, work.data_ptr(), rows_in.data_ptr(), rows.data_ptr()))
                    _lib.check(L.ptmi_sup_end(h, work.data_ptr(), vals.data_ptr(), res.data_ptr()))

            def form():
                idx = torch.nonzero(lp != -float("inf")).view(-1)    # (its own synchronisation: the size of idx)
                if 0 < idx.numel() < n_in:
                    r = rows_in[idx]
                    res.fill_(-float("inf"))
                    res[idx] = vals[:idx.numel()]
                    return r

            t = {}
            for name, f in (("hand", hand), ("torch", form)) * 2:    # alternating
                for _ in range(3):
                    f()
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    t.setdefault(name, []).append((time.perf_counter() - t0) * 1e6)
            out.append(dict(d=d, n_in=n_in, share=share, hand=t["hand"], torch=t["torch"]))
    print(json.dumps(dict(leg="yardstick", rows=out)), flush=True)


def run_child(args, lib=None, prefix=()):
    env = dict(os.environ)
    if lib:
        env["PTMI_LIB"] = lib
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=420)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("child %s failed (%d)" % (args, p.returncode))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def fmt(ms):
    return "%8.2f (%.2f - %.2f) ms per %d iterations, %d repeats" % (np.median(ms), min(ms), max(ms), ITERS, len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--legs", nargs="+", default=["off", "price", "gain", "yardstick"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libptmi.so of the parent commit's build, for the off leg")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "yardstick":
            return yardstick(int(a.child[1]))
        return child(a.child[0], {"on": True, "off": False, "parent": None}[a.child[1]], int(a.child[2]),
                     float(a.child[3]) if len(a.child) > 3 else None)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                                     # line by line: a leg that fails later loses nothing
            open(a.out, "w").write("\n".join(lines) + "\n")

    off_med = price_us = None
    if "off" in a.legs:
        say("off: 64 x 4096 x 100-d, builtin_logl + builtin_logp (a box nobody leaves), SCAM/DE 20/20, stage off")
        new, par = [], []
        for _ in range(2):                                            # the two builds alternating
            if a.parent_lib:
                par += run_child(["off", "parent", a.reps], lib=a.parent_lib)["ms"]
            new += run_child(["off", "off", a.reps])["ms"]
        if par:
            say("  parent build   %s" % fmt(par))
        say("  this build     %s" % fmt(new))
        off_med = float(np.median(new))
    if "price" in a.legs:
        r = run_child(["price", "on", 2 * a.reps])
        say("price: the same run, stage on, every row inside the support (%d of %d rows handed to logl)" % (r["given"], r["offered"]))
        if off_med is not None:
            price_us = (float(np.median(r["ms"])) - off_med) * 1e3 / ITERS
        say("  stage on       %s%s" % (fmt(r["ms"]), "; stage %+.1f us per iteration" % price_us if price_us is not None else ""))
        if a.profile:
            import tempfile
            out = tempfile.mkdtemp()
            # (a child that fails ends the tool, here as everywhere: nothing more is started on the GPU behind a fault or a hang)
            r = run_child(["price", "on", a.reps], prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "price", "--"])
            try:
                dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_results.db")]
                c = sqlite3.connect(dbs[0])
                t0 = c.execute("select max(start) from kernels where name like '%set_iter_kernel%'").fetchone()[0]
                rows = c.execute("select name, count(*), sum(end-start) from kernels where start >= ? group by name order by 3 desc", (t0,)).fetchall()
                total = sum(r_[2] for r_ in rows)
                say("  kernel trace of the price leg, %d x %d timed iterations (wall %s):" % (a.reps, ITERS, fmt(r["ms"])))
                for name, n, ns in rows[:12]:
                    say("    %9.3f ms %5.1f %% %7d calls %8.2f us each  %s" % (ns / 1e6, 100.0 * ns / total, n, ns / 1e3 / n, name[:80]))
            except (IndexError, TypeError, sqlite3.Error) as e:       # the trace database alone: missing, or another layout
                say("  kernel trace of the price leg: not measured (%s: %s)" % (type(e).__name__, e))
    if "gain" in a.legs:
        logl_ms = None
        for box in GAIN_BOXES:
            say("gain: dense 1000-d, 64 x 256, rows_logl=True, box half-width %.2f, SCAM/DE 20/20" % box)
            on, off = [], []
            for _ in range(2):                                        # stage off and on alternating
                r0 = run_child(["gain", "off", a.reps, box])
                r1 = run_child(["gain", "on", a.reps, box])
                off += r0["ms"]
                on += r1["ms"]
            share = 1.0 - r1["given"] / max(1, r1["offered"])
            logl_ms = r0["logl_ms"]
            say("  stage off      %s" % fmt(off))
            say("  stage on       %s; out-of-support share %.3f, acceptance %.3f" % (fmt(on), share, r1["accept"]))
            say("  saved %+.2f ms per %d iterations at share %.3f; the likelihood over all %d rows: %.3f ms per call" % (
                float(np.median(off)) - float(np.median(on)), ITERS, share, 64 * 256, logl_ms))
        # break-even: the share of rows outside at which what the likelihood no longer does pays the stage's fixed price
        if price_us is None:
            say("  break-even share: not measured (it needs the off and price legs)")
        else:
            say("  break-even share = price of the stage / time of the likelihood = %.1f us / %.1f us = %.3f (the price leg's per-iteration "
                "cost at 64 x 4096 x 100-d, where only the listing runs; the row copy of a partly supported batch comes on top)" % (
                    price_us, logl_ms * 1e3, price_us / (logl_ms * 1e3)))
    if "yardstick" in a.legs:
        r = run_child(["yardstick", a.reps * 4])
        say("yardstick: ptmi_sup_begin / rows / end against torch (nonzero, index, fill + index_put), us per pass, median (min - max)")
        for row in r["rows"]:
            h, t = np.array(row["hand"]), np.array(row["torch"])
            bound = np.median(t) * (1 + (t.max() - t.min()) / np.median(t))
            say("  %4d-d x %6d rows, %.2f outside: hand %7.1f (%.1f - %.1f)   torch %7.1f (%.1f - %.1f)   bound %.1f: %s" % (
                row["d"], row["n_in"], row["share"], np.median(h), h.min(), h.max(), np.median(t), t.min(), t.max(), bound,
                "inside" if np.median(h) <= bound else "OUTSIDE"))


if __name__ == "__main__":
    main()
