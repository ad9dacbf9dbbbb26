#!/usr/bin/env python
"""What one update of the adapted ladder (PTEngine.with_stages(adapt_ladder=...), csrc/ptmi_ladder.hip) costs beside the swap it follows
(developer tool, one GPU).

    python tools/ladder_timing.py [--rounds 5] [--launches 200] [--out FILE]

64 temperatures x 4096 walkers x 100-d, SCAM cycle in the fused kernels, pooled covariance (bench.py's flagship), tskip = 100.  Behind a
warm-up of 1100 iterations (eleven swaps: the counters are not all zero) a round times, each between two events on the engine's stream,
--launches calls back to back of
  ptmi_ladder_update   the column sums of nswap [4096][64] (2 MB, read once) and the finishing block; kappa = 0, so the ladder stays
  ptmi_swap            the swap of the same handle, at consecutive swap iterations
and reports microseconds per call, median (min - max) of --rounds rounds.  Back to back the counters stay in the Infinity Cache: a lower
bound of what a call costs inside a run, for both."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, STEP = 1100, 100
D, NT, W = 100, 64, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine
    g = PTEngine.with_stages(D, NT, W, np.eye(D) * 0.01, weights=(20, 0, 0), cov_update=1000, burn=10000, tskip=STEP, seed=1234,
                             cov_mode="pooled", am_mode="rle", eig_lag=1, adapt_ladder=dict(every=10, until=0))      # (until = 0: run() itself never updates)
    g.init_state(np.zeros(D))
    g.run(WARMUP)
    g.sync()
    upd, swp = [], []
    it = WARMUP
    for _ in range(a.rounds):
        g.timer_start()
        for _ in range(a.launches):
            _lib.check(g.lib.ptmi_ladder_update(g.h, 0.0, 10, 10))
        upd.append(g.timer_stop_ms() * 1e3 / a.launches)
        g.timer_start()
        for _ in range(a.launches):
            it += STEP
            _lib.check(g.lib.ptmi_swap(g.h, it))
        swp.append(g.timer_stop_ms() * 1e3 / a.launches)
    g.sync()
    assert np.allclose(g.ladder, g.ladder0, rtol=1e-12)              # kappa = 0 moved nothing
    lines = ["ladder adaptation: %d temperatures x %d walkers, %d launches back to back, median (min - max) of %d rounds" % (
                 NT, W, a.launches, a.rounds),
             "  ptmi_ladder_update  %7.1f (%.1f - %.1f) us per call" % (np.median(upd), min(upd), max(upd)),
             "  ptmi_swap           %7.1f (%.1f - %.1f) us per call" % (np.median(swp), min(swp), max(swp)),
             "  update / swap       %7.3f" % (np.median(upd) / np.median(swp))]
    print("\n".join(lines), flush=True)
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
