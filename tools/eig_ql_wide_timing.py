"""One covariance epoch's factorization beyond 128 parameters, three ways on the same cov buffer of one engine (developer tool, GPU):
eig_mode "ql" (ptmi_eig_ql's wide kernels), "hipsolver" (the ROCm library through torch.linalg.eigh) and "lapack" (the default: one
host SVD per walker through _eigworker, the copies both ways included -- what a run pays).

A short per-walker run on the iso target adapts realistic covariances first.  The three ways alternate, seven repeats each; device
ways by the engine's timer, "lapack" by wall time around the call plus sync().  Prints median (min - max) per shape.

    python tools/eig_ql_wide_timing.py [--shapes 4096x129,1024x200,256x512] [--repeats 7] [--ql-only] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptmcmcsampler_amd import _lib
from ptmcmcsampler_amd.engine import PTEngine


def fmt(v):
    return "%9.2f (%9.2f - %9.2f)" % (np.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x129,1024x200,256x512")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ql-only", action="store_true", help="time the device QL solver alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["%-12s %-10s %s" % ("W x d", "eig_mode", "ms per covariance epoch: median (min - max), %d repeats" % a.repeats)]
    for shape in a.shapes.split(","):
        W, d = (int(v) for v in shape.split("x"))
        cu = 2 * d                                                   # rows per covariance period: a full-rank sample covariance
        g = PTEngine(d, 1, W, np.eye(d) * 0.01, weights=(20, 0, 0), cov_update=cu, burn=100000, tskip=0, seed=1, cov_mode="per_walker",
                     eig_mode="ql", use_de_buffer=False)
        g.init_state(np.zeros(d))
        g.run(cu + 1)                                                # one covariance epoch: cov is adapted, and factorized once by "ql"
        g.sync()
        assert g.eig_epochs == 1
        ut_ql = g.get("Ut").copy()

        def ql():
            g.timer_start()
            _lib.check(g.lib.ptmi_eig_ql(g.h))
            return g.timer_stop_ms()

        def hipsolver():
            g.timer_start()
            g._eig_hipsolver()
            return g.timer_stop_ms()

        def lapack():
            g.sync()
            t = time.perf_counter()
            g._eig_host_all(g.get("cov"))
            g.sync()
            return (time.perf_counter() - t) * 1e3

        ways = [("ql", ql)] if a.ql_only else [("ql", ql), ("hipsolver", hipsolver), ("lapack", lapack)]
        ql()                                                         # warm-up: the scratch exists
        ms = {name: [] for name, _ in ways}
        for _ in range(a.repeats):
            for name, f in ways:
                ms[name].append(f())
        ql()
        g.sync()
        assert np.array_equal(g.get("Ut").view(np.uint64), ut_ql.view(np.uint64))     # the same table as the run's own epoch
        for name, _ in ways:
            lines.append("%-12s %-10s %s" % ("%d x %d" % (W, d), name, fmt(ms[name])))
        if not a.ql_only:
            med = np.median(ms["ql"])
            lines.append("%-12s ql median / lapack min = %.3f, ql median / hipsolver median = %.3f" % (
                "%d x %d" % (W, d), med / min(ms["lapack"]), med / np.median(ms["hipsolver"])))
        print("\n".join(lines[-(len(ways) + 1):]), flush=True)
        del g
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
