#!/usr/bin/env python
"""HMC and NUTS through batched gradient callbacks (PTEngine.gradient_stage, csrc/ptmi_gjcb.hip) at full size: updates/s, leapfrogs/s,
callback rounds per iteration (mean, max), rows per round (mean, and the share of rounds that list fewer than 1 % of the chains), and --
with --profile -- the library's kernels' share of the wall time against the callback's.

    python tools/gj_callback_timing.py [--ntemps 64 --nwalkers 1024 --ndim 40 --iters 50 --warmup 10] [--profile] [--only CALLBACK CYCLE]
    python tools/gj_callback_timing.py --ndim 1000 --nwalkers 256 --epoch 1000 --only iso hmc     (beyond 512-d: HMC, the iso callback)

Two callbacks, each with five cycles -- SCAM + HMC, HMC only, NUTS only, SCAM + NUTS, and sample()'s default mix SCAM = AM = DE = NUTS =
HMC = 20 (NUTS on the split path: PTEngine(split_nuts=True)).  The NUTS cycles are timed in steady state: after --nuts-warmup
iterations (default 30), when every chain has made its first NUTS call (its step-size search) -- the share that has is reported:
  * interval: the reference's own gradient workload (tests/test_nuts.py: a unit Gaussian behind intervalTransform on (0, 10)) as a
    torch expression, its gradient by autograd;
  * iso: the built-in isotropic Gaussian (ptmi_rows_logl, one pass over the rows) with -X as its gradient -- the stage's own cost
    with the cheapest callback there is.
--profile runs each case again in a fresh child under ``rocprofv3 --kernel-trace --stats`` and sums the kernels of the timed region
(from the marker launch on) by owner: the library's (split_rows / gj_* / rows_iso / am_*) and everything else (the callback's)."""
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
LIB_KERNELS = ("split_rows_kernel", "gj_begin_kernel", "gj_step_kernel", "gj_count_kernel", "gj_fill_kernel", "rows_iso_kernel", "am_",
               "set_iter_kernel", "gjw_")                      # gjw_: the stage beyond 512-d (csrc/ptmi_gjcb_wide.hip)


def interval_callbacks(d, a=0.0, b=10.0):
    import torch
    c = 0.5 * np.log(2 * np.pi)
    lw = float(np.log(b - a))

    def logl(X):
        x = a + (b - a) * torch.sigmoid(X)
        return (-0.5 * x * x - c).sum(-1) + (lw + torch.nn.functional.logsigmoid(X) + torch.nn.functional.logsigmoid(-X)).sum(-1)

    def logl_grad(X):
        Xg = X.detach().requires_grad_(True)
        with torch.enable_grad():
            ll = logl(Xg)
            g, = torch.autograd.grad(ll.sum(), Xg)
        return ll.detach(), g

    return logl, logl_grad


def run_case(args, which, cycle):
    import torch
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    d, nt, W = args.ndim, args.ntemps, args.nwalkers
    weights, grad_weights = CYCLES[cycle]
    nuts = grad_weights[0] > 0
    warmup = args.nuts_warmup if nuts else args.warmup
    # the default mix: its covariance epoch, DE's start and the end of NUTS's step-size adaptation all fall inside the warm-up
    burn = warmup if weights[1] + weights[2] > 0 else args.epoch     # (the AM ring is nwalkers x epoch x ndim doubles)
    logl_name = ("iso",) if which == "iso" else ("interval", 0.0, 10.0)
    cov0 = np.eye(d) * (0.5 if which == "interval" else 1.0)
    if args.full_cov:                                            # full whitening tables (the identity's are diagonal: d multiplications)
        A = np.random.RandomState(1).randn(d, d)
        cov0 = A @ A.T / d + 0.5 * np.eye(d)
    g = PTEngine(d, nt, W, cov0, logl=logl_name, weights=weights, grad_weights=grad_weights,
                 hmc=(args.eps, 2, args.hmc_steps), cov_update=burn, burn=burn, tskip=0, seed=5, split=True, split_nuts=nuts,
                 cov_mode="pooled", am_mode="rows")
    if which == "iso":
        bl = g.builtin_logl()
        logl = bl

        def logl_grad(X):
            return bl(X), -X
        p0 = np.random.RandomState(0).randn(W, nt, d)
    else:
        logl, logl_grad = interval_callbacks(d)
        x = np.clip(np.abs(np.random.RandomState(0).randn(W, nt, d)), 1e-6, 9.999)
        p0 = np.log(x / 10.0) - np.log1p(-x / 10.0)
    rows = [[]]                                                  # rows of every round, per iteration (the likelihood callback ends one)

    def counted_logl(X):
        rows.append([])
        return logl(X)

    def counted(X):
        rows[-1].append(X.shape[0])
        return logl_grad(X)

    g.init_state_callback(p0, logl, None)
    g.run_callback(warmup, logl, None, logl_grad=counted)
    g.sync()
    gj0 = g.get("gj")
    js0 = g.get("jstat").astype(np.int64)
    rows[:] = [[]]
    _lib.check(g.lib.ptmi_set_device_iter(g.h, 0))               # a marker launch: the timed region starts behind it
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.run_callback(args.iters, counted_logl, None, logl_grad=counted)
    g.sync()
    wall = time.perf_counter() - t0
    gj = g.get("gj")
    nleap = gj[..., _lib.GJ_NLEAP].sum() - gj0[..., _lib.GJ_NLEAP].sum()
    js = g.get("jstat").astype(np.int64) - js0
    # rows[k]: the rounds of iteration k + 1's stage (each likelihood call opens the next iteration's list; the last one stays empty)
    nrounds = np.array([len(r) for r in rows[:args.iters]], dtype=np.int64)
    allrows = np.array([n for r in rows for n in r], dtype=np.int64)
    r = dict(callback=which, cycle=cycle, ndim=d, ntemps=nt, nwalkers=W, iters=args.iters, wall_s=wall,
             updates_per_s=W * nt * args.iters / wall, leapfrogs_per_s=float(nleap) / wall,
             rounds_per_iter=float(allrows.size) / args.iters, us_per_round=1e6 * wall / max(1, allrows.size), rounds_per_iter_max=int(nrounds.max()) if nrounds.size else 0,
             rows_per_round=float(allrows.mean()) if allrows.size else 0.0,
             rounds_under_1pct=float((allrows < 0.01 * W * nt).mean()) if allrows.size else 0.0,
             hmc_share=float(js[..., 4, 0].sum() / js[..., 0].sum()), hmc_accept=float(js[..., 4, 1].sum() / max(1, js[..., 4, 0].sum())))
    if nuts:
        r.update(nuts_share=float(js[..., 3, 0].sum() / js[..., 0].sum()), nuts_accept=float(js[..., 3, 1].sum() / max(1, js[..., 3, 0].sum())),
                 past_first_call=float((gj0[..., _lib.GJ_HAVE_EPS] == 1.0).mean()),
                 leapfrogs_per_nuts_call=float((gj[..., _lib.GJ_NLEAP].sum() - gj0[..., _lib.GJ_NLEAP].sum()) /
                                               max(1.0, gj[..., _lib.GJ_NITER].sum() + gj[..., _lib.GJ_HITER].sum()
                                                   - gj0[..., _lib.GJ_NITER].sum() - gj0[..., _lib.GJ_HITER].sum())))
    return r


# cycle -> (SCAM, AM, DE weights), (NUTS, HMC weights)
CYCLES = {"scam_hmc": ((20, 0, 0), (0, 20)), "hmc": ((0, 0, 0), (0, 20)), "nuts": ((0, 0, 0), (20, 0)), "scam_nuts": ((20, 0, 0), (20, 0)),
          "default_mix": ((20, 20, 20), (20, 20))}


def kernel_share(db, wall_s):
    c = sqlite3.connect(db)
    t0 = c.execute("select max(start) from kernels where name like '%set_iter_kernel%'").fetchone()[0]
    rows = c.execute("select name, sum(end-start) from kernels where start >= ? group by name", (t0,)).fetchall()
    lib = sum(r[1] for r in rows if any(k in r[0] for k in LIB_KERNELS)) / 1e9
    other = sum(r[1] for r in rows if not any(k in r[0] for k in LIB_KERNELS)) / 1e9
    top = sorted(rows, key=lambda r: -r[1])[:6]
    return dict(library_kernels_s=lib, callback_kernels_s=other, library_share_of_wall=lib / wall_s, callback_share_of_wall=other / wall_s,
                top=[(r[0][:80], r[1] / 1e9) for r in top])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndim", type=int, default=40)
    ap.add_argument("--ntemps", type=int, default=64)
    ap.add_argument("--nwalkers", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nuts-warmup", type=int, default=30)
    ap.add_argument("--eps", type=float, default=0.4)
    ap.add_argument("--hmc-steps", type=int, default=50)
    ap.add_argument("--epoch", type=int, default=100000, help="covariance epoch and burn of the cycles without AM / DE: beyond the run; "
                    "a smaller one keeps the AM ring of a large ndim in memory")
    ap.add_argument("--full-cov", action="store_true", help="a full initial covariance instead of the identity: full whitening tables")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--only", nargs=2, metavar=("CALLBACK", "CYCLE"))
    ap.add_argument("--out", default=None, help="profile databases go under this directory (default: a temporary one)")
    args = ap.parse_args()
    cases = [tuple(args.only)] if args.only else [(w, c) for w in ("interval", "iso") for c in CYCLES]
    for which, cycle in cases:
        r = run_case(args, which, cycle)
        if args.profile:
            import tempfile
            out = args.out or tempfile.mkdtemp()
            name = "%s_%s" % (which, cycle)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(out, name), "-o", name, "--", sys.executable,
                   os.path.abspath(__file__), "--only", which, cycle] + [
                "--%s=%s" % (k.replace("_", "-"), getattr(args, k)) for k in ("ndim", "ntemps", "nwalkers", "iters", "warmup", "nuts_warmup", "eps",
                                                                              "hmc_steps", "epoch")] + (["--full-cov"] if args.full_cov else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
            if p.returncode != 0:
                print(p.stdout[-3000:])
                raise SystemExit("rocprofv3 run failed (%d)" % p.returncode)
            prof = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(out, name)) for f in fs if f.endswith("_results.db")]
            r["profiled_wall_s"] = prof["wall_s"]
            r.update(kernel_share(dbs[0], prof["wall_s"]))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
