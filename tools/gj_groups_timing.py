"""Step time of the fused gradient-jump kernel with and without parameter groups (developer tool, one GPU).

The workload of ``bench.py --logl curved --ndim 20 --ntemps 16 --mix nuts``: the curved likelihood at 20-d in the box [-10, 10], 16
temperatures x 4096 walkers, SCAM / DE / NUTS 10/10/10, one pooled covariance that starts from the identity.  Two legs: ``groups=None``
(the pair layout) and two groups of 10 parameters (the whole-wave layout, one chain at a time: mh_steps_gj_kernel<..., GRP = true>).
Per leg: ms per 100 iterations as median (min - max) of the repeats, after a warm-up.

usage: gj_groups_timing.py [--repeats N] [--iters K] [--warmup W] [--leg one|two|both]
PTMI_LIB=<another libptmi.so> times that build of the library instead (the one-group leg of a parent build, for instance)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptmcmcsampler_amd.engine import PTEngine  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=100, help="iterations per repeat [100]")
ap.add_argument("--warmup", type=int, default=300)
ap.add_argument("--leg", default="both", choices=["one", "two", "both"])
a = ap.parse_args()

d, nt, W = 20, 16, 4096
legs = [("one group", None), ("two groups of 10", [np.arange(10), np.arange(10, 20)])]
legs = [leg for leg, key in zip(legs, ("one", "two")) if a.leg in (key, "both")]
for name, groups in legs:
    e = PTEngine(d, nt, W, np.eye(d), logl=("curved",), logp=("box", np.full(d, -10.0), np.full(d, 10.0)), weights=(10, 0, 10),
                 grad_weights=(10, 0), cov_update=1000, burn=10000, tskip=100, seed=1234, cov_mode="pooled", groups=groups)
    e.init_state(np.array([-0.1, -0.5] * (d // 2)))
    e.run(a.warmup)
    e.sync()
    ms = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        e.run(a.iters)
        e.sync()
        ms.append((time.perf_counter() - t) * 1e3 * 100.0 / a.iters)
    js = e.get("jstat").sum(axis=(0, 1))
    print("%-18s %8.3f ms per 100 iterations, median of %d (%.3f - %.3f)  %.3g updates/s  proposed %s  variant %s" % (
        name, float(np.median(ms)), len(ms), min(ms), max(ms), nt * W * 100 / (float(np.median(ms)) * 1e-3), js[:, 0].tolist(), e.last_variant()), flush=True)
    del e
