"""Auxiliary jumps as batched device callbacks on the split path (csrc/ptmi_aux.hip; include/ptmi.h ptmi_aux_*; PTEngine.with_stages(aux=...),
PTEngine.aux_stage, PTSampler.batched_aux with addAuxilaryJump(..., batched=True)): the reference's loop over its auxiliary jumps,
q, qxy_aux = aux(x, q, iter, beta); qxy += qxy_aux (PTMCMCSampler.py:1062-1065), for every chain of the batch at once.

  1. a sampler with two auxiliary jumps as batched torch callbacks equals, character for character, the sampler that calls the same
     arithmetic per chain in NumPy on the host;
  2. on a cycle of custom entries only, jump + auxiliary jumps is itself one custom jump: the device equals the oracle with the folded
     function, bit for bit;
  3. the state gather: the X an auxiliary function is given is the chains' state wherever it lives (X, Q or Q2);
  4. the contract of the three entry points.

Run on the GPU box: ``python -m pytest tests -m gpu``.  Nothing here reads the reference tree."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------- 1. the sampler
def test_batched_aux_equals_the_per_chain_aux(tmp_path):
    """Two samplers, one seed, a custom jump beside SCAM / AM / DE and two auxiliary jumps that do not commute, swaps, covariance and DE
    epochs inside: (a) calls logl / logp / the jump / the auxiliary jumps per chain in NumPy on the host, (b) is batched=True,
    batched_aux set, with the same arithmetic in torch -- element-wise IEEE operations only, the sum spelled out column by column."""
    import torch
    from ptmcmcsampler_amd import PTSampler
    d = 5
    kw = dict(burn=40, thin=1, covUpdate=20, isave=100, Tskip=7, SCAMweight=4, AMweight=4, DEweight=4)

    def logl_np(x):
        return -0.5 * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4])

    def logp_np(x):
        return 0.0 if np.all((x >= -3.0) & (x <= 3.0)) else -np.inf

    def logl_t(X):
        return -0.5 * (X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1] + X[:, 2] * X[:, 2] + X[:, 3] * X[:, 3] + X[:, 4] * X[:, 4])

    def logp_t(X):
        return torch.where(((X >= -3.0) & (X <= 3.0)).all(-1), 0.0, -float("inf")).to(torch.float64)

    def make_np():
        def shrinkJump(x, it, beta):
            return x * 0.5 + (0.25 * beta + 0.01 * float((it % 7) - 3)), -0.1 * beta

        def halfway(x, q, it, beta):
            return x + 0.5 * (q - x), -0.05 * beta

        def nudge(x, q, it, beta):
            return q + 0.01 * float((it % 3) - 1), 0.0             # (per chain the reference's qxy += qxy_aux needs a number)

        return shrinkJump, halfway, nudge

    calls = []

    def make_t():
        def shrinkJump(X, it, beta):
            return X * 0.5 + (0.25 * beta + 0.01 * float((it % 7) - 3))[:, None], -0.1 * beta

        def halfway(X, Q, it, beta):
            assert X.is_cuda and X.shape == Q.shape == (12, d) and beta.shape == (12,) and X.data_ptr() != Q.data_ptr()
            calls.append(it)
            return X + 0.5 * (Q - X), -0.05 * beta                 # a tensor of its own: ptmi_aux_end copies it into the proposal buffer

        def nudge(X, Q, it, beta):
            Q += 0.01 * float((it % 3) - 1)                        # in place on what the function before returned
            return Q, None

        return shrinkJump, halfway, nudge

    common = dict(verbose=False, seed=4, ntemps=3, nwalkers=4, keep_walkers=4)
    a = PTSampler(d, logl_np, logp_np, np.eye(d) * 0.5, outDir=str(tmp_path / "a"), **common)
    jump, aux1, aux2 = make_np()
    a.addProposalToCycle(jump, 2)
    a.addAuxilaryJump(aux1)
    a.addAuxilaryJump(aux2)
    a.sample(np.full(d, 0.1), 300, **kw)
    b = PTSampler(d, logl_t, logp_t, np.eye(d) * 0.5, outDir=str(tmp_path / "b"), batched=True, **common)
    b.batched_aux = True
    jump, aux1, aux2 = make_t()
    b.addProposalToCycle(jump, 2, batched=True)
    b.addAuxilaryJump(aux1, batched=True)
    b.addAuxilaryJump(aux2, batched=True)
    b.sample(np.full(d, 0.1), 300, **kw)
    assert calls == list(range(1, 301))                               # once per iteration, for every chain
    for name in ("X", "lnL", "lp", "slot_of", "nacc", "jstat", "nswap", "Ut"):
        assert_same(a.engine.get(name), b.engine.get(name), name)
    assert np.array_equal(a._chains, b._chains) and np.array_equal(a._lnlikes, b._lnlikes) and np.array_equal(a._lnprobs, b._lnprobs)
    files = ["chain_1.0.txt"] + ["chain_1.0_w%d.txt" % k for k in range(1, 4)] + ["jumps.txt"]
    files += sorted(f for f in __import__("os").listdir(tmp_path / "a") if f.endswith("_jump.txt"))
    assert "shrinkJump_jump.txt" in files and "DEJump_jump.txt" in files
    for f in files:
        assert open(tmp_path / "a" / f).read() == open(tmp_path / "b" / f).read(), f
    assert np.array_equal(np.load(tmp_path / "a" / "cov.npy"), np.load(tmp_path / "b" / "cov.npy"))
    assert a.jumpDict == b.jumpDict and b.jumpDict["shrinkJump"][0] > 0
    nacc = b.engine.get("nacc").astype(np.int64)
    assert (nacc > 0).all() and (nacc < 300).all()


@pytest.mark.parametrize("nuts", (0, 10))
def test_sampler_runs_custom_jumps_beside_batched_gradients(tmp_path, nuts):
    """PTSampler(batched=True, logl_grad=, logp_grad=) with a batched custom jump: the reference's cycle of a custom entry, HMC (and,
    with batched_nuts=True, NUTS), SCAM, AM and DE, which this sampler refused before.  Shares in jumps.txt sum to 1; every jump of the
    cycle -- HMCJump, NUTSJUMP, the custom one -- writes its file."""
    import torch
    from ptmcmcsampler_amd import PTSampler
    d = 4

    def logl(X):
        return -0.5 * (X * X).sum(-1)

    def logp(X):
        return torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)

    def logl_grad(X):
        return logl(X), -X

    def logp_grad(X):
        return logp(X), torch.zeros_like(X)

    def pullJump(X, it, beta):
        return X * 0.5, None

    s = PTSampler(d, logl, logp, np.eye(d) * 0.5, logl_grad=logl_grad, logp_grad=logp_grad, outDir=str(tmp_path), verbose=False, seed=2,
                  ntemps=2, nwalkers=8, batched=True, batched_nuts=nuts > 0, nuts_maxdepth=4)
    s.addProposalToCycle(pullJump, 5, batched=True)
    s.sample(np.full(d, 0.1), 200, burn=50, thin=1, covUpdate=50, isave=100, Tskip=10, SCAMweight=10, AMweight=10, DEweight=10,
             NUTSweight=nuts, HMCweight=10, HMCstepsize=0.2, HMCsteps=10)
    shares = dict((ln.split()[0], float(ln.split()[1])) for ln in open(tmp_path / "jumps.txt"))
    assert set(shares) == {"HMCJump", "pullJump", "covarianceJumpProposalSCAM", "covarianceJumpProposalAM", "DEJump"} | ({"NUTSJUMP"} if nuts else set())
    # the file holds every share with two significant digits ("%4.2g"): each is between 0.09 and 0.23 here, so rounded by at most 0.005
    assert abs(sum(shares.values()) - 1.0) <= 0.005 * len(shares) + 1e-12
    if nuts:
        assert s.jumpDict["NUTSJUMP"][0] > 0 and s.engine.get("gj")[..., 4].sum() > 0
    for name in shares:
        assert len(open(tmp_path / (name + "_jump.txt")).read().split()) >= 2, name
    assert s.jumpDict["HMCJump"][0] > 0 and s.jumpDict["pullJump"][0] > 0
    assert sum(v[0] for v in s.jumpDict.values()) == 200
    js, cj = s.engine.get("jstat").astype(np.int64), s.engine.get("cjstat").astype(np.int64)
    assert (js[..., 0].sum(-1) + cj[..., 0].sum(-1) == 200).all()


# ------------------------------------------------------------------------------------------- 2. the oracle, all-custom cycle
def _walk_and_aux(np_side, second_qxy=False):
    """walk (the cycle's only entry), aux1, aux2 in torch or in NumPy, and for NumPy the folded jump aux2(x, aux1(x, walk(x))) with the
    qxy summed in the order the reference adds them.  ``second_qxy``: aux2 returns a qxy too (three terms: the order of the additions
    shows in the last bit)."""
    col = (lambda v: v[:, None])

    def walk(X, it, beta):
        return X * 0.9 + col(0.05 * beta + 0.02 * float((it % 5) - 2)), -0.1 * beta

    def aux1(X, Q, it, beta):
        return X + 0.5 * (Q - X), -0.05 * beta

    def aux2(X, Q, it, beta):
        return Q + 0.01 * float((it % 3) - 1), (0.07 * beta if second_qxy else None)

    def folded(X, it, beta):
        q, qxy = walk(X, it, beta)
        q, a1 = aux1(X, q, it, beta)
        q, a2 = aux2(X, q, it, beta)
        return q, (qxy + a1) + a2 if second_qxy else qxy + a1       # qxy += qxy_aux, one function after the other (PTMCMCSampler.py:1065)

    return (walk, aux1, aux2, folded) if np_side else (walk, aux1, aux2)


@pytest.mark.parametrize("d,nt,W,second_qxy", [(5, 3, 4, False), (21, 2, 70, False),   # (odd ndim, 140 chains: 8-byte pieces, more than two tiles)
                                               (5, 3, 4, True)])
def test_jump_and_aux_equal_the_oracles_folded_jump(mods, d, nt, W, second_qxy):
    """weights = (0, 0, 0): every pick is the custom entry, so jump + auxiliary jumps IS one custom jump, which the oracle runs."""
    orc, _lib, PTEngine = mods
    rs = np.random.RandomState(10 * d + nt)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.3
    kw = dict(weights=(0, 0, 0), cov_update=20, burn=40, tskip=7, seed=17, am_mode="rows")
    o = orc.OracleEngine(d, nt, W, cov0, jumps=[(_walk_and_aux(True, second_qxy)[3], 2)], **kw)
    o.init_state(p0)
    engines = []
    for mode in ("rows fused", "rows two launches"):
        walk, aux1, aux2 = _walk_and_aux(False, second_qxy)
        g = PTEngine.with_stages(d, nt, W, cov0, rows_logl=True, jumps=[(walk, 2)], aux=[aux1, aux2], **kw)
        g.init_state(p0)
        engines.append((mode, g))
    for n in (25, 3, 1, 46, 30):
        o.run(n)
        for mode, g in engines:
            g.run_callback(n, *g._rows_callbacks()[:2], fused=(mode == "rows fused"))
            g.sync()
            assert not g.t["sloc"].any()
            for name in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "cjstat", "nswap", "AM", "cov", "Ut", "S"):
                assert_same(g.get(name), getattr(o, name), "%s at iteration %d: %s" % (mode, g.iter, name))
    cj, nacc = o.cjstat.astype(np.int64), o.nacc.astype(np.int64)
    assert (cj[..., 0].sum(-1) == 105).all() and not o.jstat.any()    # every pick was custom
    assert cj[..., 0].sum(axis=(0, 1)).min() > 0 and cj[..., 1].sum(axis=(0, 1)).min() > 0
    assert 0 < nacc.sum() < 105 * W * nt and o.nswap.sum() > 0 and o.iter == 105


# ------------------------------------------------------------------------------------------------------ 3. the state gather
def _gather_case(PTEngine, d, nt, W, like, extra, stages, aux):
    rs = np.random.RandomState(7 * d + nt)
    A = rs.randn(d, d)
    cov0 = (A @ A.T / d + 0.5 * np.eye(d)) * 0.01
    p0 = rs.randn(W, nt, d) * 0.05
    logl = ("iso",)
    if like == "dense":
        B = rs.randn(d, d)
        P = np.linalg.inv(B @ B.T / d + 0.5 * np.eye(d))
        logl = ("dense", rs.randn(d) * 0.05, (P + P.T) / 2.0)
    kw = dict(weights=(3, 2, 2), cov_update=20, burn=40, tskip=7, seed=23, logl=logl, am_mode="rows", **extra)
    if stages:                                                        # custom and gradient jumps in the cycle: all three stages run

        def stretch(X, it, beta):
            return X * 0.5 + (0.05 * beta)[:, None], -0.1 * beta

        kw.update(jumps=[(stretch, 2)], grad_weights=(2, 2), jumps_with_grad=True, hmc=(0.1, 2, 20), nuts_maxdepth=6)
    g = PTEngine.with_stages(d, nt, W, cov0, rows_logl=True, aux=aux, **kw)
    g.init_state(p0)
    return g


@pytest.mark.parametrize("d,nt,W,like,extra,stages", [
    (20, 4, 37, "dense", {}, True),                                   # gradient and custom jumps in the cycle too: all three stages
    (21, 3, 5, "iso", {}, False),                                     # odd ndim: 8-byte pieces
    (6, 2, 700, "iso", dict(cov_mode="pooled"), False),               # 1400 chains: 22 blocks
])
def test_the_gathered_rows_are_the_states_wherever_they_live(mods, d, nt, W, like, extra, stages):
    """An auxiliary function that changes nothing and records the X it is given, in the same configuration with two launches per
    iteration (the states are in X, sloc is zero) and with one (the states sit in X, Q and Q2): the same rows at every iteration; and
    every array of the engine equals a run without the stage."""
    import torch
    orc, _lib, PTEngine = mods
    n = W * nt
    runs = {}
    for mode in ("two launches", "fused"):
        seen, slocs, holder = [], [], {}

        def record(X, Q, it, beta, seen=seen, slocs=slocs, holder=holder, mode=mode):
            g = holder["g"]
            assert X.shape == (n, d) and Q.data_ptr() == g.proposals().data_ptr() and beta.shape == (n,)
            assert torch.equal(beta, torch.as_tensor(1.0 / g.temps_mh, device=X.device)[g.t["temp_of"].view(-1).long()])
            if mode == "two launches":
                assert not g.t["sloc"].any() and torch.equal(X, g.t["X"].view(n, d))
            else:
                slocs.append(tuple(sorted(g.t["sloc"].unique().tolist())))
            seen.append(X.clone())
            return Q, None

        g = _gather_case(PTEngine, d, nt, W, like, extra, stages, [record])
        holder["g"] = g
        runs[mode] = (g, seen, slocs)
    plain = _gather_case(PTEngine, d, nt, W, like, extra, stages, None)
    for k in (25, 3, 1, 46, 30):
        for mode, (g, _, _) in runs.items():
            cb = g._rows_callbacks()
            g.run_callback(k, cb[0], cb[1], fused=(mode == "fused"), logl_grad=cb[2], logp_grad=cb[3])
        cb = plain._rows_callbacks()
        plain.run_callback(k, cb[0], cb[1], logl_grad=cb[2], logp_grad=cb[3])
        for mode, (g, _, _) in runs.items():
            g.sync()
            assert not g.t["sloc"].any()
            for name in ("X", "lnL", "lp", "temp_of", "slot_of", "nacc", "jstat", "nswap", "AM", "cov", "Ut", "S", "DE") + (("cjstat", "gj") if stages else ()):
                assert_same(g.get(name), plain.get(name), "%s against the run without aux at iteration %d: %s" % (mode, g.iter, name))
    (_, a, _), (_, b, slocs) = runs["two launches"], runs["fused"]
    assert len(a) == len(b) == 105
    for it, (xa, xb) in enumerate(zip(a, b), start=1):
        assert torch.equal(xa.view(torch.int64), xb.view(torch.int64)), "the gathered states of iteration %d" % it
    # in the middle of the segments states sat in X, in Q and in Q2: a call sees X and the buffer that does NOT hold the current proposals
    # (a state in the buffer the next proposals go to was moved to X by that launch), the two buffers in turn from call to call
    assert set(slocs) >= {(0, 1), (0, 2)} and all(set(v) <= {0, 1} or set(v) <= {0, 2} for v in slocs)
    assert any(x == (0, 1) and y == (0, 2) for x, y in zip(slocs, slocs[1:]))
    assert 0 < plain.get("nacc").sum() < 105 * n


# -------------------------------------------------------------------------------------------------------------- 4. contract
def _iso_engine(PTEngine, d, nt, W, aux, **kw):
    g = PTEngine.with_stages(d, nt, W, np.eye(d) * 0.01, weights=(3, 0, 2), cov_update=20, burn=40, tskip=7, seed=3, rows_logl=True, aux=aux,
                             **kw)
    g.init_state(np.random.RandomState(1).randn(W, nt, d) * 0.05)
    return g


def test_accept_waits_for_the_stage_and_the_stage_for_the_jumps(mods):
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 2, 8
    n = W * nt

    def keep(X, Q, it, beta):
        return Q, None

    def stretch(X, it, beta):
        return X * 0.5, None

    x = torch.empty((n, d), dtype=torch.float64, device="cuda")
    beta = torch.empty(n, dtype=torch.float64, device="cuda")
    # with custom jumps, then with gradient jumps, in the cycle: the auxiliary stage opens only behind theirs
    for kw in (dict(jumps=[(stretch, 4)]), dict(grad_weights=(0, 4), hmc=(0.1, 2, 5))):
        g = _iso_engine(PTEngine, d, nt, W, [keep], **kw)
        logl, logp, logl_grad, logp_grad = g._rows_callbacks()
        lib, h = g.lib, g.h
        accept = lambda: lib.ptmi_accept(h, 1, g.t["lnL"].data_ptr(), g.t["lp"].data_ptr())   # noqa: E731
        assert lib.ptmi_aux_begin(h, 1, x.data_ptr(), beta.data_ptr()) == -1          # nothing proposed yet
        _lib.check(lib.ptmi_propose(h, 1))
        assert lib.ptmi_aux_begin(h, 1, x.data_ptr(), beta.data_ptr()) == -1          # the jump's own stage has not ended
        assert b"stage of these proposals has not ended" in lib.ptmi_last_error()
        g.gradient_stage(1, logl_grad, logp_grad)
        g.jump_stage(1)
        assert accept() == -1                                                            # pending
        assert lib.ptmi_aux_end(h, None, None) == -1                                     # not open
        assert lib.ptmi_aux_begin(h, 2, x.data_ptr(), beta.data_ptr()) == -1          # another iteration's
        _lib.check(lib.ptmi_aux_begin(h, 1, x.data_ptr(), beta.data_ptr()))
        assert accept() == -1                                                            # open
        assert lib.ptmi_aux_begin(h, 1, x.data_ptr(), beta.data_ptr()) == -1          # twice
        assert lib.ptmi_aux_end(h, x.data_ptr() + 8, None) == -1                        # a misaligned qrows: refused, the stage stays open ...
        assert accept() == -1
        _lib.check(lib.ptmi_aux_end(h, None, None))                                      # ... and a correct call ends it
        assert lib.ptmi_aux_end(h, None, None) == -1
        ll, lp = g.eval_callback(g.proposals(), logl, logp)
        _lib.check(lib.ptmi_accept(h, 1, ll.data_ptr(), lp.data_ptr()))
        g.sync()
    # not in ptmi_device_iter mode, not attached twice, not without the stage
    _lib.check(lib.ptmi_device_iter(h, 1))
    assert lib.ptmi_aux_begin(h, 1, x.data_ptr(), beta.data_ptr()) == -3              # PTMI_EUNSUPPORTED
    _lib.check(lib.ptmi_device_iter(h, 0))
    assert lib.ptmi_aux_attach(h) == -1
    bare = _iso_engine(PTEngine, d, nt, W, None)
    _lib.check(bare.lib.ptmi_propose(bare.h, 1))
    assert bare.lib.ptmi_aux_begin(bare.h, 1, x.data_ptr(), beta.data_ptr()) == -1
    only = _iso_engine(PTEngine, d, nt, W, [keep])
    assert not only.callback_segment_graph(1, 5, *only._rows_callbacks()[:2])           # the stage is not captured


def test_a_wrong_shape_raises_and_names_the_function(mods):
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 2, 8

    def badRows(X, Q, it, beta):
        return Q[:-1], None

    def badQxy(X, Q, it, beta):
        return Q, beta[:-1]

    def notATuple(X, Q, it, beta):
        return Q

    for f in (badRows, badQxy, notATuple):
        g = _iso_engine(PTEngine, d, nt, W, [f])
        cb = g._rows_callbacks()
        with pytest.raises(ValueError, match=f.__name__):
            g.run_callback(3, cb[0], cb[1])
        # the stage did not stay open behind the function that raised
        assert g.lib.ptmi_aux_end(g.h, None, None) == -1
        g.init_state(np.zeros(d))
        g.sync()


def test_qxy_is_added_and_reaches_the_accept_test(mods):
    """qxy = -inf for every chain above the cold rank: those ranks never accept in 50 iterations, rank 0 goes on accepting."""
    import torch
    orc, _lib, PTEngine = mods
    d, nt, W = 6, 3, 16

    def wall(X, Q, it, beta):
        return Q, torch.where(beta < 1.0, -float("inf"), 0.0).to(torch.float64)

    g = _iso_engine(PTEngine, d, nt, W, [wall])
    cb = g._rows_callbacks()
    g.run_callback(50, cb[0], cb[1])
    nacc = g.get("nacc").astype(np.int64)                             # by rank
    assert (nacc[:, 1:] == 0).all() and (nacc[:, 0] > 0).all()
    free = _iso_engine(PTEngine, d, nt, W, None)
    cb = free._rows_callbacks()
    free.run_callback(50, cb[0], cb[1])
    assert (free.get("nacc").astype(np.int64)[:, 1:] > 0).all()
