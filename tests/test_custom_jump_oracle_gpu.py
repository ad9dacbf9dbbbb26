"""The device's custom-jump stage (csrc/ptmi_cj.hip, the split accept kernels, PTEngine(jumps=...)) against an INDEPENDENT restatement:
OracleEngine(jumps=...), which tests/test_cycle_golden.py pins to the reference's own sample() with addProposalToCycle.  Bit for bit.

tests/test_custom_jump_gpu.py compares the device with itself (one launch / two / shape kernels; batched / per chain), so a mistake
all of them share passes there: the sign of qxy in the accept test (PTMCMCSampler.py:615), the pick space with the custom entries
first before and after DE joins, cjstat kept by rank across swaps, the rank-0 AM row of an iteration whose pick was custom, the beta
a jump sees after a swap.  Here every one of those changes a compared array.

The likelihood is the library's (rows_logl=True), the jumps are single IEEE operations per element, so torch and NumPy agree to the bit.
Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads /root/reference."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


def _jump_pairs(lo, hi, seen):
    """[(device jump, oracle jump, weight)]: the same arithmetic in torch and in NumPy.  stretch: qxy depends on beta; shift: on the
    iteration, in place, qxy None; the library's box draw; out: steps by +-0.05, which takes some rows outside the box prior (lp = -inf:
    proposed, never accepted).  ``seen`` counts the oracle's rows per jump and the rows ``out`` put outside."""
    from ptmcmcsampler_amd.engine import box_draw_jump

    def stretch_t(X, it, beta):
        return X * 0.5 + (0.05 * beta)[:, None], -0.1 * beta

    def stretch_n(X, it, beta):
        seen["stretch"] += len(X)
        return X * 0.5 + (0.05 * beta)[:, None], -0.1 * beta

    def shift_t(X, it, beta):
        X += 0.01 * float((it % 5) - 2)
        return X, None

    def shift_n(X, it, beta):
        seen["shift"] += len(X)
        return X + 0.01 * float((it % 5) - 2), None

    def out_t(X, it, beta):
        return X + 0.05 * float(1 - 2 * (it & 1)), 0

    def out_n(X, it, beta):
        q = X + 0.05 * float(1 - 2 * (it & 1))
        seen["out"] += len(X)
        seen["outside"] += int((~((q >= lo) & (q <= hi)).all(-1)).sum())
        return q, 0

    return [(stretch_t, stretch_n, 2), (shift_t, shift_n, 1), (box_draw_jump(lo, hi), ("box", lo, hi), 1), (out_t, out_n, 1)]


def _compare(g, o, what):
    g.sync()
    assert not g.t["sloc"].any()
    for name in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "cjstat", "nswap", "AM", "cov", "Ut", "S"):
        assert_same(g.get(name), getattr(o, name), "%s: %s" % (what, name))
    assert_same(np.roll(g.get("DE"), -g.de_head, axis=1), o.DE, "%s: DE" % what)


def _oracle_logl(torch, orc, o):
    """The oracle's likelihood bits of every row, as a batched callback (tests/test_split_rows_gpu.py)."""
    def logl(X):
        q = X.cpu().numpy()
        v = np.array([orc.lib().orc_logl(C.byref(o.cfg), q[i].ctypes.data_as(orc._dp)) for i in range(len(q))])
        return torch.from_numpy(v).to(X.device)

    return logl


def _oracle_side(orc, d, nt, W, weights, like, extra):
    """The case's target, start and oracle; ``seen``: the oracle's rows per jump."""
    rs = np.random.RandomState(100 * d + nt)
    lo, hi = -0.4 - 0.1 * rs.rand(d), 0.4 + 0.1 * rs.rand(d)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.05
    logl = ("iso",)
    if like == "dense":
        B = rs.randn(d, d)
        P = np.linalg.inv(B @ B.T / d + 0.5 * np.eye(d))
        logl = ("dense", rs.randn(d) * 0.05, (P + P.T) / 2.0)
    seen = dict(stretch=0, shift=0, out=0, outside=0)
    pairs = _jump_pairs(lo, hi, seen)
    kw = dict(weights=weights, cov_update=20, burn=40, tskip=7, seed=31, logl=logl, logp=("box", lo, hi), am_mode="rows")
    kw.update(extra)
    o = orc.OracleEngine(d, nt, W, cov0, jumps=[(fn, w) for _, fn, w in pairs], **kw)
    o.init_state(p0)
    return o, kw, p0, cov0, lo, hi, seen


def _reached(o, seen, W, nt, niter=105):
    """The run went where the case is for."""
    js, cj = o.jstat.astype(np.int64), o.cjstat.astype(np.int64)
    assert cj.shape == (W, nt, 5, 2) and (js[..., 0].sum(-1) + cj[..., 0].sum(-1) == niter).all()
    assert seen["stretch"] == cj[..., :2, 0].sum() and seen["shift"] == cj[..., 2, 0].sum() and seen["out"] == cj[..., 4, 0].sum()
    assert cj[..., 4, 1].sum() <= seen["out"] - seen["outside"]       # a proposal outside the box is never accepted
    if W * nt > 1:
        assert cj[..., 0].sum(axis=(0, 1)).min() > 0 and cj[..., 1].sum(axis=(0, 1)).min() > 0   # every pick index proposed and accepted
        assert 0 < seen["outside"] < seen["out"]
        assert js[..., 2, 0].sum() > 0                                 # DE joined behind the custom entries
    if nt > 1:
        assert o.nswap.sum() > 0
    assert o.cfg.de_on == 1 and o.iter == niter


CASES = [
    # d, nt, W, weights, likelihood, extra
    (20, 4, 37, (3, 2, 2), "dense", {}),                              # 148 chains: 2.3 tiles; AM increments' scratch from ptmi_cj_attach
    (21, 3, 5, (3, 0, 2), "iso", {}),                                 # odd ndim: 8-byte pieces
    (6, 2, 700, (3, 2, 2), "iso", dict(cov_mode="pooled")),           # 1400 chains: two blocks of the listing
    (20, 4, 6, (3, 2, 2), "dense", dict(pick_mode="walker")),         # one pick per walker
    (5, 2, 3, (3, 2, 2), "iso", dict(groups=[[0, 1, 2, 3, 4], [3, 1], [2]])),   # parameter groups beside custom picks: no group drawn for those
    (4, 1, 1, (3, 2, 2), "dense", {}),                                # one chain: empty spans, no ladder
    # 70 049 chains: 69 listing blocks, 417 slots in the last -- cj_gather_kernel's strided sums over the blocks (32 partial sums per
    # function) take a second and a third step (tests/test_custom_jump_gpu.py test_listing_beyond_one_stride_of_blocks).  12 iterations
    # with the epochs drawn in: swaps at 3, 6, 9, 12, covariance epochs at 4, 8, 12, DE joins at 8.  The case is bound by the host: measured on
    # one core, the oracle's start 1.8 s and its 12 iterations 0.6 s, and the oracle's likelihood handed back row by row to the callback
    # engine 0.45 - 0.5 s per pass, 13 passes: 8 - 9 s in all on such a host, 1.9 s (pytest --durations) on the faster host of an MI355X.
    (6, 7, 10007, (3, 2, 2), "iso", dict(cov_mode="pooled", cov_update=4, burn=8, tskip=3, segments=(5, 1, 6), blocks=69)),
]
LB, STRIDE = 1024, 32                                                 # chain slots per listing block, partial sums per function (csrc/ptmi_cj.hip)


@pytest.mark.parametrize("d,nt,W,weights,like,extra", CASES)
def test_custom_jump_stage_equals_the_oracle(mods, d, nt, W, weights, like, extra, monkeypatch):
    """Four device engines -- row kernels with one launch per iteration, with two, the shape kernels, and the callback path with the
    oracle's likelihood handed back -- against ONE oracle run, after uneven pieces across covariance epochs (20), DE activation (40)
    and swaps (7); the 70 049-chain case sets its own, shorter ones (``extra``: epochs at 4, 8 and 3, pieces of 5, 1 and 6)."""
    import torch
    orc, _lib, PTEngine = mods
    extra = dict(extra)
    segments = extra.pop("segments", (25, 3, 1, 46, 30))
    blocks = extra.pop("blocks", None)                                # a case that is there for its number of listing blocks says so
    if blocks is not None:
        assert blocks == -(-W * nt // LB) > 2 * STRIDE
    o, kw, p0, cov0, lo, hi, seen = _oracle_side(orc, d, nt, W, weights, like, extra)
    lo_t, hi_t = torch.as_tensor(lo, device="cuda"), torch.as_tensor(hi, device="cuda")

    def logp_cb(X):
        return torch.where(((X >= lo_t) & (X <= hi_t)).all(-1), 0.0, -float("inf")).to(torch.float64)

    engines = []
    for mode in ("rows fused", "rows two launches", "shape kernels", "callback"):
        jumps = [(ft, w) for ft, _, w in _jump_pairs(lo, hi, dict(seen))]
        if mode == "callback":
            g = PTEngine(d, nt, W, cov0, split=True, jumps=jumps, **kw)
            cbs = (_oracle_logl(torch, orc, o), logp_cb)
            g.init_state_callback(p0, *cbs)
        else:
            g = PTEngine(d, nt, W, cov0, rows_logl=True, jumps=jumps, **kw)
            g.init_state(p0)
            cbs = g._rows_callbacks()[:2]
        engines.append((mode, g, cbs))
        _compare(g, o, "%s at the start" % mode)
    if weights[1] > 0:
        v = C.c_int32(0)
        _lib.check(engines[0][1].lib.ptmi_split_am_piece(engines[0][1].h, C.byref(v)))
        assert v.value > 0                                            # the row kernels serve the handle
    for n in segments:
        o.run(n)
        for mode, g, cbs in engines:
            if mode == "shape kernels":
                monkeypatch.setenv("PTMI_SPLIT_ROWS", "0")
            else:
                monkeypatch.delenv("PTMI_SPLIT_ROWS", raising=False)
            g.run_callback(n, *cbs, fused=(mode != "rows two launches"))
            monkeypatch.delenv("PTMI_SPLIT_ROWS", raising=False)
            _compare(g, o, "%s at iteration %d" % (mode, g.iter))
    _reached(o, seen, W, nt, sum(segments))
    if blocks is not None:
        assert not np.array_equal(o.slot_of, np.tile(np.arange(nt, dtype=o.slot_of.dtype), (W, 1)))   # the ladders have moved


@pytest.mark.parametrize("name", ["traj_custom_d4", "traj_custom_groups_d5"])
def test_reference_custom_cycles_in_counter_mode(mods, golden, name):
    """The two configurations whose replay pins the oracle to the reference (tests/test_cycle_golden.py), now on the library's own
    draws: three walkers of the same cycle on the device against the oracle."""
    import torch
    from ptmcmcsampler_amd.engine import box_draw_jump
    orc, _lib, PTEngine = mods
    g_ = golden(name)
    d, nt, W = int(g_["ndim"]), int(g_["nranks"]), 3
    logl = ("dense", g_["dense_mu"], g_["dense_icov"]) if "dense_mu" in g_ else ("iso",)
    logp = ("box", g_["box_lo"], g_["box_hi"]) if "box_lo" in g_ else ("flat",)
    groups = [a.tolist() for a in np.split(g_["groups_flat"], np.cumsum(g_["groups_size"])[:-1])] if "groups_flat" in g_ else None

    def shrink_t(X, it, beta):
        return X * 0.5 + (0.25 * beta + 0.01 * float((it % 7) - 3))[:, None], -0.1 * beta

    def shrink_n(X, it, beta):
        return X * 0.5 + (0.25 * beta + 0.01 * float((it % 7) - 3))[:, None], -0.1 * beta

    jt, jn = [], []
    for nm, w in zip(g_["custom_names"], g_["custom_weights"]):
        if str(nm) == "UniformJump":
            jt.append((box_draw_jump(g_["box_lo"], g_["box_hi"]), int(w)))
            jn.append((("box", g_["box_lo"], g_["box_hi"]), int(w)))
        else:
            jt.append((shrink_t, int(w)))
            jn.append((shrink_n, int(w)))
    kw = dict(ladder=g_["ladder"], weights=(int(g_["kw_SCAMweight"]), int(g_["kw_AMweight"]), int(g_["kw_DEweight"])),
              cov_update=int(g_["kw_covUpdate"]), burn=int(g_["kw_burn"]), tskip=int(g_["kw_Tskip"]), seed=int(g_["seed"]), logl=logl, logp=logp,
              groups=groups, am_mode="rows")
    p0 = np.broadcast_to(g_["p0"], (W, nt, d)).copy()
    o = orc.OracleEngine(d, nt, W, g_["cov0"], jumps=jn, **kw)
    o.init_state(p0)
    g = PTEngine(d, nt, W, g_["cov0"], rows_logl=True, jumps=jt, **kw)
    g.init_state(p0)
    for n in (151, 249):
        o.run(n)
        g.run(n)
        _compare(g, o, "%s at iteration %d" % (name, g.iter))
    cj = o.cjstat.astype(np.int64)
    assert cj[..., 0].sum(axis=(0, 1)).min() > 0 and cj[..., 1].sum(axis=(0, 1)).min() > 0 and o.nswap[:, :nt - 1].min() > 0
    assert not np.array_equal(o.X[0], o.X[1])                         # the walkers are replicas with their own streams
