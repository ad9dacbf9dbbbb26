#!/usr/bin/env python
"""What the auxiliary-jump stage (PTEngine.aux_stage, csrc/ptmi_aux.hip) and the mixed cycle cost on the callback path (developer tool, one
GPU).  Device events around --iters iterations of a warmed-up engine, --reps repeats per leg, the legs of one process alternating.

    python tools/aux_timing.py [--parent-lib PATH] [--what aux mixed] [--iters 200] [--reps 3] [--profile] [--out FILE]

aux:   64 temperatures x 4096 walkers x 100-d, SCAM cycle, the likelihood a device kernel behind the C ABI (``builtin_logl`` =
       ptmi_rows_logl, what ``bench.py --callback --callback-kind hip`` uses).  Legs: (i) no auxiliary jump -- with --parent-lib also
       on that build of the library (PTMI_LIB; a process of its own, the builds alternating): that path gains one phase check on the
       host; (ii) one identity auxiliary jump (``return Q, None``): the stage is then the state gather alone, 8 d bytes in and 8 d
       out per chain; (iii) a plain ``copy_`` of a [chains, d] f64 tensor, the same bytes without the indirection, per call.
       --profile: the whole child once more -- legs (i), (ii) and the copy_ calls alternating -- under ``rocprofv3 --kernel-trace
       --stats`` in a run of its own, its kernels summed by name: the gather's and the copy's time per call come from there.
mixed: 64 x 1024 x 40-d, the interval Gaussian of tools/nuts40_timing.py as batched torch callbacks with gradients; SCAM / AM / DE /
       HMC 10/10/10/10 (HMC <= 10 steps) with and without a box-draw entry of weight 5: the custom stage beside the gradient stage."""
import argparse
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 120


def timed(torch, run, iters, reps_of):
    """ms of ``run(iters)`` between two device events, appended to reps_of."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    run(iters)
    e1.record()
    torch.cuda.synchronize()
    reps_of.append(e0.elapsed_time(e1))


def child_aux(iters, reps, legs):
    import torch
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    d, nt, W = 100, 64, 4096
    engines = {}
    for leg in legs:
        def identity(X, Q, it, beta):
            return Q, None
        g = PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=10000, burn=100000, tskip=100, seed=5, split=True,
                                 cov_mode="pooled", am_mode="rows", **(dict(aux=[identity]) if leg == "ii" else {}))
        logl = g.builtin_logl()
        g.init_state_callback(np.zeros(d), logl, None)
        g.run_callback(WARMUP, logl, None)
        g.sync()
        engines[leg] = (g, logl)
    _lib.check(g.lib.ptmi_set_device_iter(g.h, 0))               # a marker launch: the timed region starts behind it
    ms = {leg: [] for leg in legs}
    for _ in range(reps):                                         # the legs alternate
        for leg, (g, logl) in engines.items():
            timed(torch, lambda n: g.run_callback(n, logl, None), iters, ms[leg])
    out = dict(lib=os.path.basename(os.path.dirname(_lib.SO)) + "/" + os.path.basename(_lib.SO), ms=ms)
    if "ii" in legs:
        a, b = torch.randn((W * nt, d), dtype=torch.float64, device="cuda"), torch.empty((W * nt, d), dtype=torch.float64, device="cuda")
        cp = []
        for _ in range(reps):
            timed(torch, lambda n: [b.copy_(a) for _ in range(n)], iters, cp)
        out["copy_ms"] = cp
    print(json.dumps(out), flush=True)


def child_mixed(iters, reps):
    import torch
    from ptmcmcsampler_amd.engine import PTEngine, box_draw_jump
    d, nt, W, a, b = 40, 64, 1024, 0.0, 10.0
    c, lw = 0.5 * np.log(2 * np.pi), float(np.log(b - a))

    def logl(X):
        x = a + (b - a) * torch.sigmoid(X)
        return (-0.5 * x * x - c).sum(-1) + (lw + torch.nn.functional.logsigmoid(X) + torch.nn.functional.logsigmoid(-X)).sum(-1)

    def logl_grad(X):                                             # analytic: d/dp of the above, x' = (x - a) (b - x) / (b - a)
        s = torch.sigmoid(X)
        x = a + (b - a) * s
        return logl(X), -x * (b - a) * s * (1 - s) + (1 - 2 * s)

    engines = {}
    for leg in ("without", "with box 5"):
        kw = dict(jumps=[(box_draw_jump(np.full(d, -6.0), np.full(d, 3.0)), 5)], jumps_with_grad=True) if leg != "without" else {}
        g = PTEngine.with_stages(d, nt, W, np.eye(d) / 0.25, weights=(10, 10, 10), grad_weights=(0, 10), hmc=(0.4, 2, 10), cov_update=1000, burn=100,
                                 tskip=100, seed=1, split=True, cov_mode="pooled", am_mode="rows", **kw)
        g.init_state_callback(np.full(d, -2.3), logl, None)
        g.run_callback(WARMUP, logl, None, logl_grad=logl_grad)
        g.sync()
        engines[leg] = g
    ms = {leg: [] for leg in engines}
    for _ in range(reps):
        for leg, g in engines.items():
            timed(torch, lambda n: g.run_callback(n, logl, None, logl_grad=logl_grad), iters, ms[leg])
    out = dict(ms=ms)
    g = engines["with box 5"]
    cj, js = g.get("cjstat").astype(np.int64), g.get("jstat").astype(np.int64)
    out.update(custom_share=float(cj[..., 0].sum()) / (W * nt * g.iter), hmc_share=float(js[..., 4, 0].sum()) / (W * nt * g.iter))
    print(json.dumps(out), flush=True)


def run_child(what, iters, reps, lib=None, prefix=()):
    env = dict(os.environ)
    if lib:
        env["PTMI_LIB"] = lib
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", what, "--iters", str(iters), "--reps", str(reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=900)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("child %s failed (%d)" % (what, p.returncode))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--what", nargs="+", default=["aux", "mixed"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libptmi.so of the parent commit's build, for leg (i)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        if args.child == "mixed":
            return child_mixed(args.iters, args.reps)
        return child_aux(args.iters, args.reps, ("i",) if args.child == "aux_i" else ("i", "ii"))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(ms):
        return "%8.2f (%.2f - %.2f) ms per %d iterations, %d repeats" % (np.median(ms), min(ms), max(ms), args.iters, len(ms))

    if "aux" in args.what:
        say("aux: 64 temperatures x 4096 walkers x 100-d, SCAM cycle, ptmi_rows_logl as the callback")
        par, new, aux, cp = [], [], [], []
        for _ in range(2):                                        # the two builds alternating
            if args.parent_lib:
                par += run_child("aux_i", args.iters, args.reps, lib=args.parent_lib)["ms"]["i"]
            r = run_child("aux", args.iters, args.reps)
            new += r["ms"]["i"]
            aux += r["ms"]["ii"]
            cp += r["copy_ms"]
        if par:
            say("  (i)   no auxiliary jump, parent build   %s" % fmt(par))
        say("  (i)   no auxiliary jump, this build     %s" % fmt(new))
        say("  (ii)  one identity auxiliary jump       %s; stage %+.3f ms per iteration" % (fmt(aux), (np.median(aux) - np.median(new)) / args.iters))
        nbytes = 2 * 64 * 4096 * 100 * 8
        say("  (iii) copy_ of [262144, 100] f64        %s; %.3f ms per call = %.2f TB/s for %.0f MB read + written" % (
            fmt(cp), np.median(cp) / args.iters, nbytes / (np.median(cp) / args.iters * 1e-3) / 1e12, nbytes / 1e6))
        if args.profile:
            import tempfile
            out = tempfile.mkdtemp()
            r = run_child("aux", args.iters, args.reps, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "aux", "--"])
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_results.db")]
            c = sqlite3.connect(dbs[0])
            t0 = c.execute("select max(start) from kernels where name like '%set_iter_kernel%'").fetchone()[0]
            rows = c.execute("select name, count(*), sum(end-start) from kernels where start >= ? group by name order by 3 desc", (t0,)).fetchall()
            total = sum(r_[2] for r_ in rows)
            say("  kernel trace of legs (i), (ii), (iii) alternating, %d x %d timed iterations each:" % (args.reps, args.iters))
            for name, n, ns in rows[:12]:
                say("    %9.3f ms %5.1f %% %7d calls %9.4f ms per call  %s" % (ns / 1e6, 100.0 * ns / total, n, ns / 1e6 / n, name[:90]))
    if "mixed" in args.what:
        say("mixed: 64 x 1024 x 40-d interval Gaussian as torch callbacks, SCAM / AM / DE / HMC 10/10/10/10 (HMC <= 10 steps)")
        r = run_child("mixed", args.iters, args.reps)
        for leg, ms in r["ms"].items():
            say("  %-12s %s" % (leg, fmt(ms)))
        say("  custom share %.4f (5/45 = %.4f), HMC share %.4f (10/45 = %.4f)" % (r["custom_share"], 5 / 45.0, r["hmc_share"], 10 / 45.0))
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
