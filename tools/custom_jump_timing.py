#!/usr/bin/env python
"""What the custom-jump stage (PTEngine.jump_stage, csrc/ptmi_cj.hip) costs on the callback path: ms per 100 iterations, median (min - max)
of --reps repeats after a warm-up, each ending in a device synchronise, with the built-in likelihood as the only callback.

    python tools/custom_jump_timing.py [--parent-lib PATH] [--sizes iso100 dense20] [--reps 5] [--profile] [--out FILE]

Sizes: iso100 = 64 temperatures x 4096 walkers x 100-d with ``builtin_logl`` (ptmi_rows_logl, one pass over the proposals); dense20 =
64 x 1024 x 20-d with the dense family's row kernel.  Legs:
  (i)   the default cycle SCAM/AM/DE 20/20/20 without custom entries -- with --parent-lib also on that build of the library (PTMI_LIB),
        the two builds alternating: whether the accept path's extra branch costs anything;
  (ii)  the default cycle + boxDrawJump 5 (the reference's test cycle, tests/test_simple.py:94-97);
  (iii) the default cycle + a torch-expression jump of weight 5 (lo + (hi - lo) * rand_like(X)).
(ii) - (i) is the price of the stage: from bytes about 5/65 of three extra row passes plus one read-back and three small launches per
iteration.  Every measurement is a child process of its own (PTMI_LIB is read at import).  --profile: leg (ii) once more under
``rocprofv3 --kernel-trace --stats`` in a run of its own, its kernels summed by name."""
import argparse
import json
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"iso100": (100, 64, 4096, "iso"), "dense20": (20, 64, 1024, "dense")}
WARMUP, ITERS = 120, 100


def child(size, leg, reps):
    import torch
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine, box_draw_jump
    d, nt, W, fam = SIZES[size]
    rs = np.random.RandomState(3)
    if fam == "dense":
        A = rs.randn(d, d)
        logl_spec = ("dense", np.zeros(d), np.linalg.inv(A @ A.T / d + 0.3 * np.eye(d)))
    else:
        logl_spec = ("iso",)
    lo, hi = -4.0 * np.ones(d), 4.0 * np.ones(d)
    kw = {}
    if leg == "ii":
        kw = dict(jumps=[(box_draw_jump(lo, hi), 5)])
    elif leg == "iii":
        lo_t, w_t = torch.as_tensor(lo, device="cuda"), torch.as_tensor(hi - lo, device="cuda")

        def torchJump(X, it, beta):
            return lo_t + w_t * torch.rand_like(X), None
        kw = dict(jumps=[(torchJump, 5)])
    # burn = 100: the DE jump is in the cycle from iteration 101 on; no covariance epoch inside the timed iterations
    g = PTEngine(d, nt, W, np.eye(d) * 0.1, logl=logl_spec, weights=(20, 20, 20), cov_update=1000, burn=100, tskip=100, seed=5, split=True,
                 cov_mode="pooled", am_mode="rows", **kw)
    logl = g.builtin_logl()
    g.init_state_callback(rs.randn(W, nt, d) * 0.3, logl, None)
    g.run_callback(WARMUP, logl, None)
    g.sync()
    _lib.check(g.lib.ptmi_set_device_iter(g.h, 0))               # a marker launch: the timed region starts behind it
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.run_callback(ITERS, logl, None)
        g.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    out = dict(size=size, leg=leg, lib=os.path.basename(os.path.dirname(_lib.SO)) + "/" + os.path.basename(_lib.SO), ms=ms)
    if kw:
        cj = g.get("cjstat").astype(np.int64)
        out.update(custom_share=float(cj[..., 0].sum()) / (W * nt * g.iter), custom_accept=float(cj[..., 1].sum()) / max(1, cj[..., 0].sum()))
    print(json.dumps(out), flush=True)


def run_child(size, leg, reps, lib=None, prefix=()):
    env = dict(os.environ)
    if lib:
        env["PTMI_LIB"] = lib
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", size, leg, "--reps", str(reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("child %s %s failed (%d)" % (size, leg, p.returncode))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def fmt(ms):
    return "%8.2f (%.2f - %.2f) ms per %d iterations, %d repeats" % (np.median(ms), min(ms), max(ms), ITERS, len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("SIZE", "LEG"))
    ap.add_argument("--sizes", nargs="+", default=list(SIZES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libptmi.so of the parent commit's build, for leg (i)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.reps)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for size in args.sizes:
        d, nt, W, fam = SIZES[size]
        say("%s: %d temperatures x %d walkers x %d-d, %s likelihood as a row kernel" % (size, nt, W, d, fam))
        new, par = [], []
        for _ in range(2):                                        # the two builds alternating
            if args.parent_lib:
                par += run_child(size, "i", args.reps, lib=args.parent_lib)["ms"]
            new += run_child(size, "i", args.reps)["ms"]
        if par:
            say("  (i)   default cycle, parent build   %s" % fmt(par))
        say("  (i)   default cycle, this build     %s" % fmt(new))
        base = float(np.median(new))
        for leg, what in (("ii", "+ boxDrawJump 5            "), ("iii", "+ torch-expression jump 5  ")):
            r = run_child(size, leg, 2 * args.reps)
            say("  %-5s %s   %s; stage %+.2f ms; custom share %.4f (5/65 = %.4f), accepted %.4f" % (
                "(%s)" % leg, what, fmt(r["ms"]), float(np.median(r["ms"])) - base, r["custom_share"], 5.0 / 65.0, r["custom_accept"]))
        rows_mb = W * nt * d * 8 / 1e6
        say("  from bytes: 5/65 of three passes over %.0f MB of rows = %.1f MB per iteration" % (rows_mb, 3 * rows_mb * 5 / 65))
        if args.profile:
            import tempfile
            out = tempfile.mkdtemp()
            r = run_child(size, "ii", args.reps, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", size, "--"])
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_results.db")]
            c = sqlite3.connect(dbs[0])
            t0 = c.execute("select max(start) from kernels where name like '%set_iter_kernel%'").fetchone()[0]
            rows = c.execute("select name, count(*), sum(end-start) from kernels where start >= ? group by name order by 3 desc", (t0,)).fetchall()
            total = sum(r_[2] for r_ in rows)
            say("  kernel trace of leg (ii), %d x %d timed iterations (wall %s):" % (args.reps, ITERS, fmt(r["ms"])))
            for name, n, ns in rows[:12]:
                say("    %9.3f ms %5.1f %% %7d calls  %s" % (ns / 1e6, 100.0 * ns / total, n, name[:90]))
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
