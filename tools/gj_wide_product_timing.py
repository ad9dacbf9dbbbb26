#!/usr/bin/env python
"""The whitening-product kernel of the gradient stage beyond 512-d (gjw_product_kernel, csrc/ptmi_gjcb_wide.hip) beside its yardstick,
the matrix-core dense gradient ptmi_rows_logl_grad (dense_rows_kernel<.., GRAD>), on the same (n, d) in the same process:

    python tools/gj_wide_product_timing.py --ndim 1000 --ntemps 64 --nwalkers 256 [--iters 3] [--profile]

An HMC-only cycle on the built-in dense Gaussian served by the row kernels (rows_logl=True), started at the mode with a small step:
every call takes one leapfrog (the reference's energy guard ends it, nutsjump.py:284-286), so every round lists every chain and is one
yardstick launch and two product launches (gradient, backward) over n = ntemps x nwalkers rows; ptmi_gj_begin adds two (forward,
backward); the yardstick's kernel also serves the accept step's value-only launches (its minimum).  --profile
runs the case in a fresh child under ``rocprofv3 --kernel-trace --stats`` and prints count / min / median / max per kernel."""
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


def run_case(args):
    import torch
    from ptmcmcsampler_amd.engine import PTEngine
    d, nt, W = args.ndim, args.ntemps, args.nwalkers
    rs = np.random.RandomState(0)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    B = rs.randn(d, d)
    P = np.linalg.inv(B @ B.T / d + 0.5 * np.eye(d))
    g = PTEngine(d, nt, W, cov0, logl=("dense", np.zeros(d), (P + P.T) / 2.0), weights=(0, 0, 0), grad_weights=(0, 20),
                 hmc=(1e-3, 2, 3), cov_update=1000, burn=1000, tskip=0, seed=5, rows_logl=True, cov_mode="pooled")
    g.init_state(rs.randn(W, nt, d) * 1e-3)
    logl, logp, logl_grad, logp_grad = g._rows_callbacks()
    rows = []

    def counted(X):
        rows.append(X.shape[0])
        return logl_grad(X)

    g.run_callback(1, logl, logp, logl_grad=counted, logp_grad=logp_grad)
    g.sync()
    del rows[:]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.run_callback(args.iters, logl, logp, logl_grad=counted, logp_grad=logp_grad)
    g.sync()
    wall = time.perf_counter() - t0
    return dict(ndim=d, n=nt * W, iters=args.iters, rounds=len(rows), rows_min=min(rows), rows_max=max(rows), wall_s=wall,
                us_per_round=1e6 * wall / len(rows), flop_per_product=2.0 * nt * W * d * d)


def kernel_stats(db, flop):
    c = sqlite3.connect(db)
    out = {}
    for key in ("gjw_product_kernel", "dense_rows_kernel", "gjw_step_kernel", "gjw_rows_kernel", "gj_fill_kernel", "gj_count_kernel", "gjw_mark_kernel"):
        t = np.array([r[0] for r in c.execute("select end-start from kernels where name like ?", ("%" + key + "%",)).fetchall()], dtype=np.float64)
        if t.size:
            out[key] = dict(launches=int(t.size), min_us=t.min() / 1e3, median_us=float(np.median(t)) / 1e3, max_us=t.max() / 1e3,
                            tflops_at_median=flop / float(np.median(t)) / 1e3 if "product" in key or "dense" in key else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndim", type=int, default=1000)
    ap.add_argument("--ntemps", type=int, default=64)
    ap.add_argument("--nwalkers", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None, help="profile databases go under this directory (default: a temporary one)")
    args = ap.parse_args()
    if not args.profile:
        print(json.dumps(run_case(args)), flush=True)
        return
    import tempfile
    out = args.out or tempfile.mkdtemp()
    name = "gjw_%d_%d" % (args.ndim, args.ntemps * args.nwalkers)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(out, name), "-o", name, "--", sys.executable, os.path.abspath(__file__)] + [
        "--%s=%s" % (k, getattr(args, k)) for k in ("ndim", "ntemps", "nwalkers", "iters")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    if p.returncode != 0:
        print(p.stdout[-3000:])
        raise SystemExit("rocprofv3 run failed (%d)" % p.returncode)
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(out, name)) for f in fs if f.endswith("_results.db")]
    r["kernels"] = kernel_stats(dbs[0], r["flop_per_product"])
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
