"""Every launch route of the swap (csrc/ptmi_swap.hip launch_swap_fused / launch_swap_sweep / the odd/even branch of ptmi_swap), driven
directly: whole ladder on one engine, no MH step, at the ladder lengths where the kernel or the walkers per block change.  The cases,
their inputs, what ``ptmi_last_swap_launch`` must report for each and the NumPy restatement of PTswap are tests/test_swap_routes.py's
(checked there on the CPU); here every table, counter and AM row is compared with the oracle bit for bit, and the edge values -- -inf,
NaN, exact ties, u = 0 -- with the restatement on replayed uniforms.

Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)
from test_swap_routes import (ROUTE_CASES, SWL_DIRECT, SWL_FUSED, SWL_LDS, SWL_ODDEVEN, RouteCase, edge_case, expected_launch,
                              model_lds, ptswap)

pytestmark = pytest.mark.gpu


def _engine(PTEngine, c):
    g = PTEngine(c.D, c.n, c.W, c.cov0, keep_lnl=True, **c.kw)
    assert g.am_rle and g.t["AMaux"] is not None                       # the AM ring's flag and (lnL, lp) rows are there to compare
    assert g.last_swap_launch() == (0, 0, 0, 0)
    g.init_state(c.p0)
    return g


def _run_and_compare(g, c, want, what):
    """The case's three sweeps on the engine, every table after each against the oracle's snapshot."""
    for s, it in enumerate(c.ITS):
        g.put("lnL", c.lnl[s])
        g.swap(it)
        g.iter = it
        g.sync()
        if s == 0:
            print("%s: ptmi_last_swap_launch -> %r" % (what, g.last_swap_launch()))
        assert g.last_swap_launch() == want, (what, g.last_swap_launch())
        for name in ("slot_of", "temp_of", "nswap"):
            assert_same(g.get(name), c.snap[s][name], "%s sweep %d %s" % (what, s, name))
    o = c.o
    assert_same(g.get("AM"), o.AM, what + " AM")
    assert_same(g.get("AMflag"), o.AMflag, what + " AMflag")
    assert_same(g.get("AMaux"), c.aux, what + " AMaux")
    for name in ("X", "lnL", "lp"):
        assert_same(g.by_temp(name), o.by_temp(getattr(o, name)), what + " by_temp " + name)
    assert g.swap_proposed == len(c.ITS)


@pytest.mark.parametrize("fused,n,W", ROUTE_CASES)
def test_swap_route_against_the_oracle(mods, fused, n, W, monkeypatch):
    """PTswap (PTMCMCSampler.py:631-697) on the route the ladder's length selects: swap_fused_kernel with 32 / 16 / 8 walkers per
    block, swap_prepare_kernel + swap_sweep_kernel<true> with 64 / 32 / 16 / 8, and from 2409 ranks on swap_sweep_kernel<false> with
    its direct stores and am_write_kernel behind it (2409, 2410, 2417: the pair count modulo the batch of eight varies); 70 walkers
    leave a partial last block for every block size, 3 do not fill one.  The route is asserted as literals."""
    orc, _lib, PTEngine = mods
    monkeypatch.setenv("PTMI_SWAP_FUSED", str(fused))
    c = RouteCase(n, W).run_oracle()
    assert c.proves_something()
    want = expected_launch(fused, n)
    assert want[0] in (SWL_FUSED, SWL_LDS, SWL_DIRECT) and (want[0] == SWL_FUSED) <= bool(fused)
    _run_and_compare(_engine(PTEngine, c), c, want, "fused=%d n=%d W=%d" % (fused, n, W))


def test_oddeven_both_parities_on_the_longest_ladder(mods):
    """Odd/even mode with the whole ladder local (swap_oddeven_kernel, one thread per tried pair) at 2409 ranks x 70 walkers: swap
    iterations 1, 2, 3 try the odd, the even and the odd pairs."""
    orc, _lib, PTEngine = mods
    c = RouteCase(2409, 70, swap_mode="oddeven").run_oracle()
    assert c.proves_something()
    _run_and_compare(_engine(PTEngine, c), c, (SWL_ODDEVEN, 0, 0, 0), "oddeven")
    acc = c.snap[0]["nswap"]
    assert acc[:, 1::2].sum() > 0 and acc[:, 0::2].sum() == 0 and c.snap[1]["nswap"][:, 0::2].sum() > 0


@pytest.mark.parametrize("fused,n", [(1, 17), (0, 17), (1, 2409)])
def test_edge_values_on_replayed_uniforms(mods, fused, n, monkeypatch):
    """-inf at one position, at two adjacent ones and at the top (the initial carried state), a NaN, exact ties, u = 0 and runs of
    accepts across batch edges (test_swap_routes.edge_case), each on a position that two batches of eight pairs share: the fused
    kernel, the two-kernel form and the direct stores take the restatement's decisions."""
    import torch
    orc, _lib, PTEngine = mods
    monkeypatch.setenv("PTMI_SWAP_FUSED", str(fused))
    T, L, u, _ = edge_case(n)
    W = L.shape[0]
    m, inv, acc = ptswap(T, L, u)
    g = PTEngine(2, n, W, np.eye(2), ladder=T, weights=(20, 0, 0), tskip=1, cov_mode="pooled")
    g.init_state(np.zeros(2))
    g.put("lnL", L)                                                    # slot s holds rank s at the start
    ud = torch.from_numpy(np.ascontiguousarray(u)).to(g.device)
    _lib.check(g.lib.ptmi_test_replay(g.h, C.c_void_p(ud.data_ptr()), None))
    try:
        g.swap(1)
        g.sync()
    finally:
        _lib.check(g.lib.ptmi_test_replay(g.h, None, None))
    kernel, wpb = (SWL_DIRECT, 64) if n == 2409 else ((SWL_FUSED, 16) if fused else (SWL_LDS, 64))
    print("edge values fused=%d n=%d: ptmi_last_swap_launch -> %r" % (fused, n, g.last_swap_launch()))
    assert g.last_swap_launch() == (kernel, wpb, model_lds(kernel, wpb, n), 0)
    assert_same(g.get("slot_of"), m, "slot_of")
    assert_same(g.get("temp_of"), inv, "temp_of")
    assert_same(g.get("nswap")[:, :-1], acc, "nswap")
    assert g.get("nswap")[:, -1].sum() == 0
    assert_same(g.by_temp("lnL"), np.take_along_axis(L, m, 1), "lnL by rank")
