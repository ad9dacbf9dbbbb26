#!/usr/bin/env python
"""What the evidence stage (PTEngine.with_stages(evidence=True), csrc/ptmi_ev.hip) costs per step, and that a handle which never attaches
it runs what it ran before (developer tool, one GPU).

    python tools/ev_timing.py [--configs headline callback] [--rounds 7] [--steps N] [--parent-lib FILE] [--out FILE]

Configurations, one step = 100 iterations and the swap behind them (tskip = 100), the stage sampling behind EVERY swap:
  headline   64 x 4096 x 100-d, SCAM cycle in the fused kernels, pooled covariance, am_mode "rle", eig_lag 1 (bench.py's flagship)
  callback   64 x 4096 x 100-d on the callback path: builtin_logl + builtin_logp (a box nobody leaves), SCAM/DE 20/20, pooled
Legs: the parent commit's library (--parent-lib, through PTMI_LIB: a process of its own, the library is chosen at import), this library with
the stage off, this library with the stage on.  Every timing is a process of its own with one engine, and a round runs the three legs
one after the other, so they alternate through the whole session.  A timing is --steps steps (default: 400 on the headline configuration,
40 on the callback path -- a third of a second and more) behind a warm-up of 1100 iterations, ending in a device synchronise; reported per
step: median (min - max) of --rounds rounds.  Stage off must lie inside the parent's own min - max spread; the stage's cost is stage on
against stage off.  The stage-on leg also times ptmi_ev_update alone, 200 launches back to back between two events (the planes stay in
the Infinity Cache between such launches: a lower bound of what a launch costs inside a run)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, STEP = 1100, 100
D, NT, W = 100, 64, 4096


def engine(config, on):
    from ptmcmcsampler_amd.engine import PTEngine
    if config == "headline":
        kw = dict(weights=(20, 0, 0), cov_update=1000, burn=10000, tskip=STEP, seed=1234, cov_mode="pooled", am_mode="rle", eig_lag=1)
    else:
        kw = dict(logp=("box", -1e3 * np.ones(D), 1e3 * np.ones(D)), split=True, weights=(20, 0, 20), cov_update=1000, burn=100, tskip=STEP,
                  seed=5, cov_mode="pooled", am_mode="rows")
    if on is None:                                                    # the parent build: no keyword at all
        return PTEngine(D, NT, W, np.eye(D) * 0.01, **kw)
    return PTEngine.with_stages(D, NT, W, np.eye(D) * 0.01, evidence=on, evidence_from=0 if on else None, **kw)


def child(config, leg, steps):
    import torch
    from ptmcmcsampler_amd import _lib
    g = engine(config, {"parent": None, "off": False, "on": True}[leg])
    if config == "headline":
        g.init_state(np.zeros(D))
        adv = g.run
    else:
        logl, logp = g.builtin_logl(), g.builtin_logp()
        g.init_state_callback(np.random.RandomState(3).randn(W, NT, D) * 0.3, logl, logp)
        adv = lambda n: g.run_callback(n, logl, logp)      # noqa: E731
    adv(WARMUP)
    g.sync()
    out = dict(config=config, leg=leg, lib=os.path.basename(os.path.dirname(_lib.SO)) + "/" + os.path.basename(_lib.SO))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        adv(STEP)
    g.sync()
    out["ms"] = (time.perf_counter() - t0) * 1e3 / steps
    if leg == "on":
        assert g.ev_epochs == (WARMUP + steps * STEP) // STEP, g.ev_epochs
        n = g.evidence_moments()["n"]
        assert (n == g.ev_epochs).all()
        g.timer_start()
        for _ in range(200):
            _lib.check(g.lib.ptmi_ev_update(g.h))
        out["update_us"] = g.timer_stop_ms() * 1e3 / 200
    print(json.dumps(out), flush=True)


def run_child(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["PTMI_LIB"] = lib
    # a limit of its own: a child that hangs ends the tool, nothing more is started on the GPU behind it
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("child %s failed (%d)" % (args, p.returncode))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def fmt(ms):
    return "%8.3f (%.3f - %.3f) ms per step" % (np.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--configs", nargs="+", default=["headline", "callback"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--parent-lib", default=None, help="libptmi.so of the parent commit's build")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                                     # line by line: a leg that fails later loses nothing
            open(a.out, "w").write("\n".join(lines) + "\n")

    say("evidence stage: wall time per step (100 iterations + swap), %d chains x %d-d, median (min - max) of %d rounds, the legs "
        "alternating, a process each" % (NT * W, D, a.rounds))
    for config in a.configs:
        steps = a.steps or (400 if config == "headline" else 40)
        t = {"parent": [], "off": [], "on": []}
        upd = []
        for k in range(a.rounds):
            print("%s: round %d of %d" % (config, k + 1, a.rounds), file=sys.stderr, flush=True)
            if a.parent_lib:
                t["parent"].append(run_child([config, "parent", steps], lib=a.parent_lib)["ms"])
            t["off"].append(run_child([config, "off", steps])["ms"])
            r = run_child([config, "on", steps])
            t["on"].append(r["ms"])
            upd.append(r["update_us"])
        say("%s, %d steps per timing:" % (config, steps))
        if t["parent"]:
            say("  parent library      %s" % fmt(t["parent"]))
        say("  stage off           %s" % fmt(t["off"]))
        say("  stage on            %s" % fmt(t["on"]))
        off, on = float(np.median(t["off"])), float(np.median(t["on"]))
        say("  stage on - off      %+.1f us per step (%+.2f %%)" % ((on - off) * 1e3, 100 * (on - off) / off))
        if t["parent"]:
            inside = min(t["parent"]) <= off <= max(t["parent"])
            say("  stage off (median) inside the parent's min - max: %s" % ("yes" if inside else "NO"))
        # per cell and call: slot_of 4 B, lnL 8 B, five planes and one count read and written 96 B
        say("  ptmi_ev_update alone, 200 launches back to back: %.1f (%.1f - %.1f) us each = %.2f TB/s of the %d B a cell moves" % (
            np.median(upd), min(upd), max(upd), 108.0 * NT * W / np.median(upd) / 1e6, 108))


if __name__ == "__main__":
    main()
