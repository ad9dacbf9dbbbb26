"""The COMPOSED proposal cycle of the CPU oracle against the reference's own sample() (tests/golden/traj_grad_*.npz, traj_custom_*.npz,
made by tests/golden/make_golden.py gen_cycle with recorded draws): gradient jumps (NUTS / HMC, PTMCMCSampler.py:225-258) beside
SCAM / AM / DE -- alone, tempered, with parameter groups -- and custom jumps added with addProposalToCycle (PTMCMCSampler.py:988-1014,
the cycle of the reference's tests/test_simple.py:94-97).

What only a run of sample() pins: the jump objects belong to the RANK and stay behind when a swap moves the state; beta = 1 / T reaches
the trees; no group is drawn on a gradient or custom pick; NUTS adapts while the SAMPLER's iteration is <= burn but averages over its
own call count (nutsjump.py:174 against :809); the whitening stays that of the initial covariance while the tables adapt; a custom
jump's qxy enters the accept test with a plus sign; the custom entries come first in the pick space, before and after DE joins.

The recorded pick indexes count in the reference's cycle order [custom, HMC, NUTS, SCAM, AM, then DE]: run(..., cycle_order="reference").

Chain tolerance of a gradient fixture: make_golden.py runs the reference twice on the same draws, the second time with the gradient
callbacks in np.longdouble; the largest relative chain deviation of the two is the fixture's rounding floor (``floor_chain``).  The
oracle may differ from the reference by more than one rounding per operation (its own exp / log, sums in lane order, fma chains): ten
floors, and no less than the 1e-11 of the trajectories without gradient jumps.  The same bound, relative to max(1, |value|), holds lnlike,
lnprob and every rank's NUTS step size after its last call.  Decisions, counters and the consumption of the draws are exact.

  fixture                   floor_chain  allowed   oracle's largest deviation (chain, lnlike, lnprob, step size)
  traj_grad_single_d6       1.4e-12      1.4e-11   2.4e-12
  traj_grad_pt3_d5          3.2e-13      1.0e-11   3.7e-13
  traj_grad_groups_d6       1.1e-11      1.1e-10   2.5e-11
  traj_grad_groups_pt2_d6   2.4e-11      2.4e-10   2.5e-12
  traj_custom_d4            -            1.0e-11   6.9e-14
  traj_custom_groups_d5     -            1.0e-11   2.7e-14
(``pytest -s`` prints them per rank.)"""
import numpy as np
import pytest

from oracle import oracle as orc

NAMES = ["covarianceJumpProposalSCAM", "covarianceJumpProposalAM", "DEJump", "NUTSJUMP", "HMCJump"]
GRAD = ["traj_grad_single_d6", "traj_grad_pt3_d5", "traj_grad_groups_d6", "traj_grad_groups_pt2_d6"]
CUSTOM = ["traj_custom_d4", "traj_custom_groups_d5"]


def shrink_jump(X, it, beta):
    """make_golden.py's shrinkJump for a batch of rows: the same IEEE operation per element and step."""
    return X * 0.5 + (0.25 * beta + 0.01 * float((it % 7) - 3))[:, None], -0.1 * beta


def custom_jumps(g):
    """The fixture's custom cycle entries as OracleEngine(jumps=...): UniformJump is the oracle's box draw."""
    made = {"UniformJump": lambda: ("box", g["box_lo"], g["box_hi"]), "shrinkJump": lambda: shrink_jump}
    return [(made[str(n)](), int(w)) for n, w in zip(g["custom_names"], g["custom_weights"])] if "custom_names" in g else None


def engine_from(g, **kw):
    d, n = int(g["ndim"]), int(g["nranks"])
    logl = ("dense", g["dense_mu"], g["dense_icov"]) if "dense_mu" in g else ("iso",)
    logp = ("box", g["box_lo"], g["box_hi"]) if "box_lo" in g else ("flat",)
    groups = np.split(g["groups_flat"], np.cumsum(g["groups_size"])[:-1]) if "groups_flat" in g else None
    gw = (int(g["kw_NUTSweight"]), int(g["kw_HMCweight"])) if "kw_NUTSweight" in g else (0, 0)
    hmc = (float(g["kw_HMCstepsize"]), 2, int(g["kw_HMCsteps"])) if sum(gw) else (0.1, 2, 300)     # PTMCMCSampler.py:235-243
    e = orc.OracleEngine(d, n, 1, g["cov0"], ladder=g["ladder"], logl=logl, logp=logp, groups=groups,
                         weights=(int(g["kw_SCAMweight"]), int(g["kw_AMweight"]), int(g["kw_DEweight"])), grad_weights=gw, hmc=hmc,
                         cov_update=int(g["kw_covUpdate"]), burn=int(g["kw_burn"]), tskip=int(g["kw_Tskip"]), hot_chain=bool(g["hot"]),
                         jumps=custom_jumps(g), **kw)
    e.init_state(g["p0"])
    return e


def replay_and_check(g, e, name):
    n, niter, thin = int(g["nranks"]), int(g["kw_Niter"]), int(g["kw_thin"])
    tol = max(1e-11, 10.0 * float(g["floor_chain"])) if "floor_chain" in g else 1e-11
    assert np.array_equal(e.temps_mh, g["temps"])
    replay = [(g["dk_%d" % r], g["dv_%d" % r], g["db_%d" % r]) for r in range(n)]
    epochs, orig = [], e._svd

    def spy(w):
        orig(w)
        epochs.append((e.mu[0].copy(), e.M2[0].copy(), e.cov[0].copy(), e.S[0, 0, :e.gsize[0]].copy()))

    e._svd = spy
    rec = e.run(niter, replay=replay, record=True, cycle_order="reference")
    assert e.replay_left == [0] * n                      # every recorded draw consumed, in kind and bound
    worst = 0.0
    for r in range(n):
        # decisions are exact
        assert int(e.nacc[0, r]) == int(g["nacc_%d" % r])
        names = [str(s) for s in g["jnames_%d" % r]]
        stats = dict(zip(names, g["jstats_%d" % r].tolist()))
        for j, nm in enumerate(NAMES):
            assert e.jstat[0, r, j].astype(int).tolist() == stats.pop(nm, [0, 0]), (r, nm)
        pick = 0
        for func, w in (custom_jumps(g) or ()):          # the weight copies of a function are consecutive pick indexes
            nm = "UniformJump" if isinstance(func, tuple) else "shrinkJump"
            assert e.cjstat[0, r, pick:pick + w].sum(0).astype(int).tolist() == stats.pop(nm), (r, nm)
            assert (e.cjstat[0, r, pick:pick + w, 0] > 0).all()
            pick += w
        assert not stats and pick == e.w_host            # every entry of the reference's jumpDict was compared
        assert int(e.nswap[0, r]) == int(g["nswap_%d" % r])
        assert e.swap_proposed == int(g["swapprop_%d" % r])
        ref_chain, ref_lnl, ref_lnp = g["chain_%d" % r], g["lnlike_%d" % r], g["lnprob_%d" % r]
        got = rec["X"][::thin, 0, r]
        assert got.shape == ref_chain.shape
        devs = [np.max(np.abs(got - ref_chain) / np.maximum(1.0, np.abs(ref_chain))),
                np.max(np.abs(rec["lnL"][::thin, 0, r] - ref_lnl) / np.maximum(1.0, np.abs(ref_lnl))),
                np.max(np.abs(rec["lnprob"][::thin, 0, r] - ref_lnp) / np.maximum(1.0, np.abs(ref_lnp)))]
        if "nuts_eps_%d" % r in g:                       # the rank's NUTS object: its call count, and its step size after the last call
            assert int(e.gj[0, r, orc.GJ_NITER]) == int(g["nuts_calls_%d" % r]) == int(e.jstat[0, r, orc.J_NUTS, 0])
            devs.append(abs(e.gj[0, r, orc.GJ_EPS] - float(g["nuts_eps_%d" % r])) / float(g["nuts_eps_%d" % r]))
        print("%s rank %d: chain %.2e lnlike %.2e lnprob %.2e%s (allowed %.2e)" % (
            name, r, devs[0], devs[1], devs[2], " step size %.2e" % devs[3] if len(devs) > 3 else "", tol))
        worst = max([worst] + devs)
    assert worst <= tol, (worst, tol)
    assert len(epochs) == int(g["nepochs"])
    for i, (mu, M2, cov, S) in enumerate(epochs):
        assert np.allclose(mu, g["ep_mu_%d" % i], rtol=1e-10, atol=1e-12)
        assert np.allclose(M2, g["ep_M2_%d" % i], rtol=1e-9, atol=1e-12)
        assert np.allclose(cov, g["ep_cov_%d" % i], rtol=1e-9, atol=1e-12)
        assert np.allclose(S, g["ep_S_%d" % i], rtol=1e-8, atol=1e-14)


@pytest.mark.parametrize("name", GRAD + CUSTOM)
def test_composed_cycle_matches_reference(golden, name):
    """sample() end to end with gradient or custom jumps in the cycle, replayed from each rank's recorded draws."""
    g = golden(name)
    if name in GRAD:
        assert float(g["floor_chain"]) <= 1e-9 and int(g["kw_burn"]) < int(g["kw_Niter"]) and int(g["kw_MALAweight"]) == 0
    replay_and_check(g, engine_from(g), name)


@pytest.mark.parametrize("name", GRAD)
def test_fixture_separates_the_jumps_call_count_from_the_samplers_iteration(golden, name):
    """NUTS's dual averaging runs on the jump's own call count (nutsjump.py:174, 806-812) and stops adapting by the SAMPLER's
    iteration (:809).  With the two made one -- the call count set to the sampler's iteration before every step, which is all a
    fixture of a lone jump called with it = 1, 2, 3 ... can see -- the replay of this fixture must fail."""
    g = golden(name)
    e = engine_from(g)
    steps = e._mh_steps

    def conflated(it, n, rp_arr):
        if n != 1:                                       # (record=True: one iteration per call)
            raise RuntimeError("the replay is expected to step one iteration at a time")
        e.gj[..., orc.GJ_NITER] = it - 1                 # nuts_call counts this call on top
        return steps(it, n, rp_arr)

    e._mh_steps = conflated
    with pytest.raises(AssertionError):
        replay_and_check(g, e, name + " [call count = iteration]")


def test_custom_picks_come_first_and_cjstat_is_by_rank(golden):
    """Counter mode, no reference: every iteration of every chain lands in exactly one of jstat / cjstat, cjstat has one column per
    pick index, accepted <= proposed and nacc is their sum; the custom entries' share of the picks is w_host / L with DE in L from
    iteration burn + 2 on; the box draw is its own function of (seed, iteration, stream)."""
    d, nt, W, n = 4, 3, 5, 120
    rs = np.random.RandomState(3)
    p0 = rs.randn(W, nt, d) * 0.2
    lo, hi = -np.ones(d) * 2.0, np.ones(d) * 2.0
    kw = dict(weights=(3, 2, 2), cov_update=20, burn=40, tskip=7, seed=31, logp=("box", lo, hi))
    e = orc.OracleEngine(d, nt, W, np.eye(d) * 0.05, jumps=[(shrink_jump, 2), (("box", lo, hi), 1)], **kw)
    e.init_state(p0)
    e.run(n)
    js, cj = e.jstat.astype(np.int64), e.cjstat.astype(np.int64)
    assert cj.shape == (W, nt, 3, 2) and (js[..., 0].sum(-1) + cj[..., 0].sum(-1) == n).all()
    assert (cj[..., 1] <= cj[..., 0]).all() and cj[..., 0].sum(axis=(0, 1)).min() > 0 and cj[..., 1].sum(axis=(0, 1)).min() > 0
    assert (e.nacc.astype(np.int64) == js[..., 1].sum(-1) + cj[..., 1].sum(-1)).all()
    # the share of the custom picks: 3 of 8 before DE joins (iterations 1 .. burn + 1), 3 of 10 after
    share, want = cj[..., 0].sum() / (W * nt * n), (41 * 3 / 8.0 + (n - 41) * 3 / 10.0) / n
    assert abs(share - want) < 5 * np.sqrt(want * (1 - want) / (W * nt * n))
    # the box draw restated: chain (w, rank t) at iteration it holds lo + (hi - lo) u of its own stream
    q = orc.cj_box_draw(31, 7, 2 * nt + 1, lo, hi)
    assert ((q >= lo) & (q < hi)).all() and not np.array_equal(q, orc.cj_box_draw(31, 7, 2 * nt + 2, lo, hi))
