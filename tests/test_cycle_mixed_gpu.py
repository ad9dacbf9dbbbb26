"""The MIXED proposal cycle on the device callback path -- custom jumps (csrc/ptmi_cj.hip) beside HMC / NUTS (csrc/ptmi_gjcb.hip) beside SCAM /
AM / DE, PTEngine.with_stages(jumps=..., grad_weights=..., jumps_with_grad=True) -- against the oracle's C step (oracle/ptmcmc_oracle.c mh_one), whose
pick space [custom, SCAM, AM, DE, NUTS, HMC] tests/test_cycle_golden.py pins to the reference's sample().  Bit for bit.

OracleEngine's constructor refuses the mix (as the device did); the C step underneath defines it, so the oracle is built with zero
gradient weights and the weights and whitening tables are set on its configuration before init_state.

The likelihood is the library's (rows_logl=True), the jumps are single IEEE operations per element, so torch and NumPy agree to the bit.
Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu

GRAD = (2, 2)                                                         # (NUTS, HMC) cycle entries
CUSTOM = 5                                                            # custom cycle entries: stretch 2, shift 1, box 1, out 1
GJ_KW = dict(hmc=(0.1, 2, 20), nuts_maxdepth=6)                      # short trajectories, trees of at most 64 leaves: the runs stay quick


def _jump_pairs(lo, hi, seen):
    """[(device jump, oracle jump, weight)] of tests/test_custom_jump_oracle_gpu.py: the same arithmetic in torch and in NumPy.  stretch:
    qxy depends on beta; shift: on the iteration, in place, qxy None; the library's box draw; out: steps by +-0.05, which takes some
    rows outside the box prior.  ``seen`` counts the oracle's rows per jump and the rows ``out`` put outside."""
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
    for name in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "cjstat", "gj", "nswap", "AM", "cov", "Ut", "S"):
        assert_same(g.get(name), getattr(o, name), "%s: %s" % (what, name))
    assert_same(np.roll(g.get("DE"), -g.de_head, axis=1), o.DE, "%s: DE" % what)


def _oracle_callbacks(torch, orc, o, lo, hi):
    """The oracle's likelihood and gradient bits of every row as batched callbacks (tests/test_gj_callback_gpu.py), the box prior in torch."""
    L = orc.lib()
    lo_t, hi_t = torch.as_tensor(lo, device="cuda"), torch.as_tensor(hi, device="cuda")

    def logl(X):
        q = np.ascontiguousarray(X.cpu().numpy())
        v = np.array([L.orc_logl(C.byref(o.cfg), q[i].ctypes.data_as(orc._dp)) for i in range(len(q))])
        return torch.from_numpy(v).to(X.device)

    def logl_grad(X):
        q = np.ascontiguousarray(X.cpu().numpy())
        g = np.zeros_like(q)
        v = np.array([L.orc_logl_grad(C.byref(o.cfg), q[i].ctypes.data_as(orc._dp), g[i].ctypes.data_as(orc._dp)) for i in range(len(q))])
        return torch.from_numpy(v).to(X.device), torch.from_numpy(g).to(X.device)

    def logp(X):
        return torch.where(((X >= lo_t) & (X <= hi_t)).all(-1), 0.0, -float("inf")).to(torch.float64)

    def logp_grad(X):
        return logp(X), torch.zeros_like(X)

    return logl, logp, logl_grad, logp_grad


def _oracle_side(orc, d, nt, W, like, extra):
    """The case's target, start and oracle with the mixed cycle; ``seen``: the oracle's rows per jump."""
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
    kw = dict(weights=(3, 2, 2), cov_update=20, burn=40, tskip=7, seed=31, logl=logl, logp=("box", lo, hi), am_mode="rows", **GJ_KW, **extra)
    o = orc.OracleEngine(d, nt, W, cov0, jumps=[(fn, w) for _, fn, w in pairs], lanes=orc.lanes_for(d, grad=True), **kw)
    # the gradient entries behind the others: what the constructor would have set had it taken grad_weights beside jumps
    o.grad_weights = GRAD
    o.gj_tab = orc.gj_tables(cov0)
    o.cfg.w_nuts, o.cfg.w_hmc = GRAD
    o.cfg.gj_tab = orc._p(o.gj_tab)
    o.init_state(p0)
    return o, kw, p0, cov0, lo, hi, seen


def _reached(o, seen, W, nt):
    """The run went where the case is for: every pick kind of both families and of the built-in jumps."""
    js, cj = o.jstat.astype(np.int64), o.cjstat.astype(np.int64)
    assert cj.shape == (W, nt, CUSTOM, 2) and (js[..., 0].sum(-1) + cj[..., 0].sum(-1) == 105).all()
    assert seen["stretch"] == cj[..., :2, 0].sum() and seen["shift"] == cj[..., 2, 0].sum() and seen["out"] == cj[..., 4, 0].sum()
    assert cj[..., 4, 1].sum() <= seen["out"] - seen["outside"]       # a proposal outside the box is never accepted
    if W * nt > 1:
        assert cj[..., 0].sum(axis=(0, 1)).min() > 0 and cj[..., 1].sum(axis=(0, 1)).min() > 0   # every custom pick index proposed and accepted
        assert js[..., 0].sum(axis=(0, 1)).min() > 0 and js[..., 1].sum(axis=(0, 1)).min() > 0   # SCAM, AM, DE, NUTS, HMC proposed and accepted
        assert 0 < seen["outside"] < seen["out"]
    else:
        assert js[..., 3:, 0].sum() > 0 and cj[..., 0].sum() > 0      # one chain: both families had picks
    if nt > 1:
        assert o.nswap.sum() > 0
    assert o.cfg.de_on == 1 and o.iter == 105
    assert o.gj[..., 4].sum() > 0 and o.gj[..., 5].sum() > 0          # NUTS and HMC calls counted in the jump state


CASES = [
    # d, nt, W, likelihood, extra, a callback engine on the oracle's bits too
    (6, 3, 5, "iso", {}, True),                                       # the basic mix
    (20, 4, 37, "dense", {}, False),                                  # 148 chains: more than two 64-row tiles; AM scratch from ptmi_cj_attach on a gradient-shape handle
    (21, 2, 3, "iso", {}, False),                                     # odd ndim: 8-byte pieces
    (40, 2, 3, "iso", dict(groups=[list(range(0, 25)), list(range(20, 40))]), False),   # 16 gradient lanes; groups beside both families
    (6, 2, 700, "iso", dict(cov_mode="pooled"), False),               # 1400 chains: two blocks of both listings
    (4, 1, 1, "dense", {}, True),                                     # one chain: empty spans, empty rounds, no ladder
]


@pytest.mark.parametrize("d,nt,W,like,extra,callback", CASES)
def test_mixed_cycle_equals_the_oracle(mods, d, nt, W, like, extra, callback):
    """Row kernels with one launch per iteration and with two (and, for the first and the last case, the callback path with the oracle's
    likelihood and gradients handed back) against ONE oracle run, after uneven pieces across covariance epochs (20), DE activation (40)
    and swaps (7).  On the commit before the mix every engine here is refused at construction."""
    import torch
    orc, _lib, PTEngine = mods
    o, kw, p0, cov0, lo, hi, seen = _oracle_side(orc, d, nt, W, like, extra)
    assert o.lanes == _lib.lanes_for(d, grad=True)
    engines = []
    for mode in ("rows fused", "rows two launches") + (("callback",) if callback else ()):
        jumps = [(ft, w) for ft, _, w in _jump_pairs(lo, hi, dict(seen))]
        if mode == "callback":
            g = PTEngine.with_stages(d, nt, W, cov0, split=True, split_nuts=True, jumps=jumps, grad_weights=GRAD, jumps_with_grad=True, **kw)
            cbs = _oracle_callbacks(torch, orc, o, lo, hi)
            g.init_state_callback(p0, *cbs[:2])
        else:
            g = PTEngine.with_stages(d, nt, W, cov0, rows_logl=True, jumps=jumps, grad_weights=GRAD, jumps_with_grad=True, **kw)
            g.init_state(p0)
            cbs = g._rows_callbacks()
        engines.append((mode, g, cbs))
        _compare(g, o, "%s at the start" % mode)
    v = C.c_int32(0)
    _lib.check(engines[0][1].lib.ptmi_split_am_piece(engines[0][1].h, C.byref(v)))
    assert v.value > 0                                                # the row kernels serve the handle: the AM scratch came from ptmi_cj_attach
    for n in (25, 3, 1, 46, 30):
        o.run(n)
        for mode, g, cbs in engines:
            g.run_callback(n, cbs[0], cbs[1], fused=(mode != "rows two launches"), logl_grad=cbs[2], logp_grad=cbs[3])
            _compare(g, o, "%s at iteration %d" % (mode, g.iter))
    _reached(o, seen, W, nt)


def test_the_order_of_the_two_stages_does_not_matter(mods):
    """Five iterations driven by hand through the C ABI: one engine runs the gradient stage first (PTEngine.split_step's order), the
    other the custom stage first.  The stages serve disjoint chains, so proposals, qaux and everything behind the accept test agree."""
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 3, 50
    rs = np.random.RandomState(9)
    lo, hi = -0.5 * np.ones(d), 0.5 * np.ones(d)
    p0 = rs.randn(W, nt, d) * 0.05
    kw = dict(weights=(3, 2, 2), cov_update=20, burn=40, tskip=7, seed=5, logp=("box", lo, hi), am_mode="rows", **GJ_KW)
    engines = []
    for _ in range(2):
        jumps = [(ft, w) for ft, _, w in _jump_pairs(lo, hi, dict(stretch=0, shift=0, out=0, outside=0))]
        g = PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, rows_logl=True, jumps=jumps, grad_weights=GRAD, jumps_with_grad=True, **kw)
        g.init_state(p0)
        engines.append(g)
    both = 0
    for it in range(1, 6):
        snaps = []
        for k, g in enumerate(engines):
            logl, logp, logl_grad, logp_grad = g._rows_callbacks()
            _lib.check(g.lib.ptmi_propose(g.h, it))
            jt = g.t["qaux"][..., 1].cpu().numpy()
            if k == 0:
                both += int(((jt == _lib.J_NUTS) | (jt == _lib.J_HMC)).any() and (jt >= _lib.J_NTYPES).any())
                g.gradient_stage(it, logl_grad, logp_grad)
                # between the stages the accept test is still refused: the custom stage is pending
                assert g.lib.ptmi_accept(g.h, it, g.t["lnL"].data_ptr(), g.t["lp"].data_ptr()) == -1
                g.jump_stage(it)
            else:
                g.jump_stage(it)
                assert g.lib.ptmi_accept(g.h, it, g.t["lnL"].data_ptr(), g.t["lp"].data_ptr()) == -1
                g.gradient_stage(it, logl_grad, logp_grad)
            snaps.append((g.proposals().cpu().numpy().copy(), g.t["qaux"].cpu().numpy().copy()))
            ll, lp = g.eval_callback(g.proposals(), logl, logp)
            _lib.check(g.lib.ptmi_accept(g.h, it, ll.data_ptr(), lp.data_ptr()))
        assert_same(snaps[0][0], snaps[1][0], "proposals of iteration %d" % it)
        assert_same(snaps[0][1], snaps[1][1], "qaux of iteration %d" % it)
        for name in ("X", "lnL", "lp", "nacc", "jstat", "cjstat", "gj", "AM"):
            assert_same(engines[0].get(name), engines[1].get(name), "%s after iteration %d" % (name, it))
    assert both > 0                                                   # an iteration had picks of both families
