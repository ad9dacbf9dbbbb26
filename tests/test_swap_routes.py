"""The swap's reference, inputs and expected launch routes, checked on the CPU (no GPU, no /root/reference).

tests/test_swap_routes_gpu.py and tests/test_exchange_direct_gpu.py drive the swap and exchange entry points directly, at the ladder
lengths where ``launch_swap_fused`` / ``launch_swap_sweep`` (csrc/ptmi_swap.hip) change the kernel or the walkers per block.  What they
compare with and what they feed in is made -- and checked -- here:

* ``ptswap``: PTswap (PTMCMCSampler.py:666-686) restated in NumPy in the log form the project defines (oracle/ptmcmc_oracle.c
  orc_swap_sweep): hottest pair first, the four-term sum in the reference's order, accept iff ``log u <= sum`` with the oracle's own
  logarithm, all walkers at once, optionally one parity only.  Pinned against ``orc.swap_sweep`` and ``orc.swap_oddeven``.
* ``place_decisions``: likelihoods and uniforms that make the sweep take a REQUESTED accept / reject pattern.
* ``multihop``: does a map move a state beyond a neighbouring block?
* ``RouteCase``: the inputs of a route case (ladder, three sets of likelihoods) and its oracle run; the condition that a case proves
  something -- between 0.2 and 0.8 of the tried pairs accept, some walker's rank-0 state moves -- is asserted here for every case.
* ``FUSED_ROUTES`` / ``TWO_KERNEL_ROUTES``: what ``ptmi_last_swap_launch`` must report, as literals: a changed LDS budget in a launcher
  shows up as a failed route assertion, not as a silently moved edge.  ``model_route`` restates the launchers' rule; the tables must
  agree with it and sit on its edges."""
import numpy as np
import pytest

from oracle import oracle as orc

SLOT_SWAP = 0x10000
U_REJECT = 1.0 - 2.0 ** -53            # the largest uniform of [0, 1): log u = -2^-53, the pair accepts only with a sum >= that
SWL_FUSED, SWL_LDS, SWL_DIRECT, SWL_ODDEVEN = 1, 2, 3, 4
BATCH = 8                              # pairs the sweep kernels fetch at once (PTMI_SWEEP_BATCH)


# ------------------------------------------------------------------------------------------------ the restatement
def log_n(u):
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(u)
    orc.lib().orc_log_n(u.size, orc._p(u), orc._p(out))
    return out


def ptswap(ladder, L, u, parity=None):
    """PTswap for every walker: ``L[W][n]`` likelihoods by position, ``u[W][n - 1]`` the uniform of pair k = (k, k + 1).
    Returns (map[W][n]: the position whose state moves to j, its inverse, acc[W][n - 1]: pair k accepted)."""
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    W, n = L.shape
    T = np.asarray(ladder, dtype=np.float64)
    lu = log_n(np.asarray(u, dtype=np.float64).reshape(W, n - 1))
    m = np.tile(np.arange(n), (W, 1))
    acc = np.zeros((W, n - 1), dtype=bool)
    rows = np.arange(W)
    with np.errstate(invalid="ignore"):
        for k in range(n - 2, -1, -1):
            if parity is not None and (k & 1) != parity:
                continue
            a, b = m[:, k].copy(), m[:, k + 1].copy()
            La, Lb = L[rows, a], L[rows, b]
            la = -La / T[k]
            la = la + -Lb / T[k + 1]
            la = la + Lb / T[k]
            la = la + La / T[k + 1]
            ok = lu[:, k] <= la
            m[:, k], m[:, k + 1] = np.where(ok, b, a), np.where(ok, a, b)
            acc[:, k] = ok
    inv = np.empty_like(m)
    np.put_along_axis(inv, m, np.tile(np.arange(n), (W, 1)), 1)
    return m, inv, acc


def multihop(m, nt):
    """Does some state of the map move beyond a neighbouring block of ``nt`` ranks?"""
    m = np.atleast_2d(m)
    return bool((np.abs(m // nt - np.arange(m.shape[1]) // nt) > 1).any())


def geometric_ladder(n, step=1.02):
    """An explicit ladder for thousands of ranks (the default step 1 + sqrt(2 / d) overflows there)."""
    return step ** np.arange(n, dtype=np.float64)


def place_decisions(accept, ladder):
    """Likelihoods ``[W][n]`` by position and uniforms ``[W][n - 1]`` with which the sweep takes exactly the decisions
    ``accept[W][n - 1]``.  The likelihoods fall steeply with the temperature, L[k] = -10 (k + 1) T[k]: whatever hotter state is
    carried to pair k lies below position k's own, the sum is negative by more than 0.1 and the pair rejects at the largest uniform;
    it accepts at u = 0 (log 0 = -inf <= any sum that is no NaN)."""
    accept = np.atleast_2d(np.asarray(accept, dtype=bool))
    W, n = accept.shape[0], accept.shape[1] + 1
    T = np.asarray(ladder, dtype=np.float64)
    assert len(T) == n
    L = np.tile(-10.0 * np.arange(1, n + 1) * T, (W, 1))
    u = np.where(accept, 0.0, U_REJECT)
    got = ptswap(T, L, u)[2]
    assert np.array_equal(got, accept), "the restatement does not take the requested decisions"
    return L, u


def pair_uniform(seed, it, walker, n, k):
    """The Philox uniform of pair k (rank 0's stream of the walker, PT:679)."""
    w = orc.philox([it & 0xFFFFFFFF, it >> 32, walker * n, SLOT_SWAP + k], [seed & 0xFFFFFFFF, seed >> 32])
    return (((w[1] << 32) | w[0]) >> 11) * 2.0 ** -53


def oracle_sweep(ladder, L, u):
    """orc.swap_sweep on explicit uniforms ``u[W][n - 1]`` (indexed by pair): the replay is read walker after walker, hottest pair first."""
    u = np.atleast_2d(u)
    m, acc = orc.swap_sweep(ladder, L, uniforms=np.ascontiguousarray(u[:, ::-1]).ravel())
    return m, acc[:, :-1].astype(bool)


# ------------------------------------------------------------------------------------------------ edge values
def edge_case(n, seed=0):
    """Five walkers of non-finite and tied values (L[5][n], u[5][n - 1]) on the geometric ladder, each placed on a position that
    belongs to the last pair of one batch of eight and the first of the next:
    0: -inf at one position, u = 0 everywhere: every other pair accepts, runs of accepts across every batch edge;
    1: -inf at two adjacent positions and at the top position (the initial carried state), generic values elsewhere;
    2: a NaN, generic values elsewhere;
    3: all likelihoods 0: every sum is exactly 0 and accepts even at the largest uniform;
    4: all likelihoods -3: the four terms cancel up to their roundings, the sums are 0 or a few 1e-16 either way against log u = -2^-53."""
    T = geometric_ladder(n)
    rs = np.random.RandomState(1000 + n + seed)
    L = generic_lnl(rs, T, 5)
    u = rs.random_sample((5, n - 1))
    nb = (n - 1 + BATCH - 1) // BATCH
    edge = lambda b: n - 2 - BATCH * b - (BATCH - 1) if b < nb - 1 else (n - 1) // 2    # noqa: E731  (position in pairs of batches b and b + 1)
    p0, p1, p2 = edge(nb // 2), edge(nb // 3), edge((2 * nb) // 3)
    L[0, p0], u[0] = -np.inf, 0.0
    L[1, p1], L[1, p1 - 1], L[1, n - 1] = -np.inf, -np.inf, -np.inf
    L[2, p2] = np.nan
    L[3], u[3] = 0.0, U_REJECT
    L[4], u[4] = -3.0, U_REJECT
    u[1, ::5], u[2, ::7] = 0.0, 0.0
    return T, L, u, (p0, p1, p2)


# ------------------------------------------------------------------------------------------------ route cases
def generic_lnl(rs, T, W):
    """Likelihoods by position with which about half of a long ladder's pairs accept: L[k] = -T[k] (3000 + 75 z).  On the ladder of
    step 1.02 the spread makes the sum of neighbouring states +-1.5 z, the mean costs a carried state 1.2 more per rank it has come
    down: runs of accepts end.  The scale is the ladder's own, so the share is the same for every length."""
    return -T * (3000.0 + 75.0 * rs.standard_normal((W, len(T))))


def model_lds(kernel, wpb, n):
    if kernel == SWL_LDS:
        return 4 * (2 * wpb * (n + 1) + n)
    if kernel == SWL_FUSED:
        return ((4 * (2 * wpb * (n + 1) + n) + 15) & ~15) + 48 * (3 * BATCH + 1) * wpb
    return 0


def model_route(n, fused):
    """(kernel, walkers per block) by the launchers' rule: the widest block of 64 / 32 / 16 / 8 walkers (the fused kernel: at most 16
    up to 128 ranks, 32 beyond) whose tables fit 160 KB of LDS; none fits: the fused kernel hands over to the two-kernel form, that
    one to its direct stores."""
    if fused:
        for wpb in ((16, 8) if n <= 128 else (32, 16, 8)):
            if model_lds(SWL_FUSED, wpb, n) <= 160 * 1024:
                return SWL_FUSED, wpb
    for wpb in (64, 32, 16, 8):
        if model_lds(SWL_LDS, wpb, n) <= 160 * 1024:
            return SWL_LDS, wpb
    return SWL_DIRECT, 64


# n -> (kernel, walkers per block) that ptmi_last_swap_launch must report: LITERALS (see the module docstring)
FUSED_ROUTES = {128: (SWL_FUSED, 16), 129: (SWL_FUSED, 32), 481: (SWL_FUSED, 32), 482: (SWL_FUSED, 16), 1094: (SWL_FUSED, 16),
                1095: (SWL_FUSED, 8), 2267: (SWL_FUSED, 8), 2268: (SWL_LDS, 8), 2408: (SWL_LDS, 8), 2409: (SWL_DIRECT, 64)}
TWO_KERNEL_ROUTES = {316: (SWL_LDS, 64), 317: (SWL_LDS, 32), 629: (SWL_LDS, 32), 630: (SWL_LDS, 16), 1240: (SWL_LDS, 16),
                     1241: (SWL_LDS, 8), 2408: (SWL_LDS, 8), 2409: (SWL_DIRECT, 64), 2410: (SWL_DIRECT, 64), 2417: (SWL_DIRECT, 64)}
ROUTE_W = (70, 3)                      # a partial last block for every walkers-per-block value; fewer walkers than any block
ROUTE_CASES = [(1, n, W) for n in FUSED_ROUTES for W in ROUTE_W] + [(0, n, W) for n in TWO_KERNEL_ROUTES for W in ROUTE_W]


def expected_launch(fused, n, hop=0):
    kernel, wpb = (FUSED_ROUTES if fused else TWO_KERNEL_ROUTES)[n]
    return kernel, wpb, model_lds(kernel, wpb, n), hop if kernel != SWL_DIRECT else 0


class RouteCase(object):
    """Whole ladder of ``n`` ranks, ``W`` walkers, d = 3, no MH step: three sweeps at the swap iterations 1, 2, 3 with new
    likelihoods before each (the second and third start from non-identity slot tables), on an OracleEngine.  ``lnl[s]`` is the
    by-slot array to put before sweep s; ``snap[s]`` the oracle's tables after it."""
    D, CU, ITS = 3, 16, (1, 2, 3)

    def __init__(self, n, W, swap_mode="sweep"):
        self.n, self.W, self.swap_mode = n, W, swap_mode
        self.ladder = geometric_ladder(n)
        self.kw = dict(ladder=self.ladder, weights=(20, 20, 0), cov_update=self.CU, burn=1000, tskip=1, seed=7 * n + W,
                       cov_mode="pooled", swap_mode=swap_mode)
        self.cov0 = np.eye(self.D) * 0.01
        self.p0 = np.random.RandomState(n + W).randn(W, n, self.D) * 0.3

    def run_oracle(self):
        rs = np.random.RandomState(3 * self.n + self.W)
        o = orc.OracleEngine(self.D, self.n, self.W, self.cov0, **self.kw)
        o.init_state(self.p0)
        self.aux = np.zeros((self.W, self.CU, 2))                     # the (lnL, lp) beside every AM row (the engine's keep_lnl)
        self.aux[:, 0, 0], self.aux[:, 0, 1] = o.by_temp(o.lnL)[:, 0], o.by_temp(o.lp)[:, 0]
        self.lnl, self.snap, self.tried, self.moved0 = [], [], 0, False
        for it in self.ITS:
            by_slot = np.empty((self.W, self.n))
            np.put_along_axis(by_slot, o.slot_of.astype(np.int64), generic_lnl(rs, self.ladder, self.W), 1)
            self.lnl.append(by_slot)
            o.lnL[...] = by_slot
            m = o.swap(it)
            self.moved0 = self.moved0 or bool((m[:, 0] != 0).any())
            parity = orc.swap_parity(it, 1) if self.swap_mode == "oddeven" else None
            self.tried += self.W * (self.n - 1 if parity is None else (self.n - parity) // 2)
            self.aux[:, it % self.CU, 0], self.aux[:, it % self.CU, 1] = o.by_temp(o.lnL)[:, 0], o.by_temp(o.lp)[:, 0]
            self.snap.append(dict(slot_of=o.slot_of.copy(), temp_of=o.temp_of.copy(), nswap=o.nswap.copy(), m=m.copy()))
        self.o = o
        self.share = float(o.nswap.sum()) / self.tried
        return self

    def proves_something(self):
        return 0.2 <= self.share <= 0.8 and self.moved0


# ------------------------------------------------------------------------------------------------ the checks
@pytest.mark.parametrize("n", [2, 9, 17, 2409])
def test_restatement_equals_the_oracle_sweep(n):
    rs = np.random.RandomState(n)
    W = 6
    T = geometric_ladder(n)
    L, u = generic_lnl(rs, T, W), rs.random_sample((W, n - 1))
    u[0, ::3] = 0.0
    L[1] = np.sort(L[1])                                              # the hottest state is the best: it is carried all the way down
    m, inv, acc = ptswap(T, L, u)
    mo, acco = oracle_sweep(T, L, u)
    assert np.array_equal(m, mo) and np.array_equal(acc, acco)
    assert np.array_equal(np.take_along_axis(inv, m, 1), np.tile(np.arange(n), (W, 1)))
    assert acc[1].all() and (m[1, 0] == n - 1) and 0 < acc.sum() < acc.size or n == 2
    # the project's default ladder where it does not overflow
    if n <= 17:
        T2 = orc.temperature_ladder(n, 10)
        L2 = rs.standard_normal((W, n)) * 3.0
        assert np.array_equal(ptswap(T2, L2, u)[0], oracle_sweep(T2, L2, u)[0])


@pytest.mark.parametrize("n", [2, 9, 17, 2409])
def test_restatement_with_a_parity_mask_equals_the_oracle_oddeven(n):
    rs = np.random.RandomState(50 + n)
    W, seed, it, walker0 = 2, 0x1234567890, 700, 3
    T = geometric_ladder(n)
    L = generic_lnl(rs, T, W)
    u = np.array([[pair_uniform(seed, it, walker0 + w, n, k) for k in range(n - 1)] for w in range(W)])
    for parity in (0, 1):
        mo, acco = orc.swap_oddeven(T, L, parity, it=it, seed=seed, walker0=walker0)
        m, inv, acc = ptswap(T, L, u, parity=parity)
        assert np.array_equal(m, mo) and np.array_equal(acc, acco[:, :-1].astype(bool))
        assert not acc[:, 1 - parity::2].any()
    # ... and unmasked, with the same uniforms, the sweep in counter mode
    mo, acco = orc.swap_sweep(T, L, it=it, seed=seed, walker0=walker0)
    m, inv, acc = ptswap(T, L, u)
    assert np.array_equal(m, mo) and np.array_equal(acc, acco[:, :-1].astype(bool))


@pytest.mark.parametrize("n", [2, 9, 17, 2409])
def test_placed_decisions_are_taken_by_restatement_and_oracle(n):
    rs = np.random.RandomState(n)
    T = geometric_ladder(n)
    want = rs.random_sample((4, n - 1)) < 0.5
    want[0], want[1] = False, True
    L, u = place_decisions(want, T)
    m, inv, acc = ptswap(T, L, u)
    mo, acco = oracle_sweep(T, L, u)
    assert np.array_equal(acc, want) and np.array_equal(acco, want) and np.array_equal(m, mo)
    assert np.array_equal(m[0], np.arange(n)) and m[1, 0] == n - 1 and np.array_equal(m[1, 1:], np.arange(n - 1))


def test_multihop_is_a_state_crossing_a_whole_block():
    n, nt = 12, 3
    T = geometric_ladder(n)

    def flag(top, run):
        """a run of accepts that carries position ``top``'s state down by ``run`` ranks"""
        a = np.zeros((1, n - 1), dtype=bool)
        a[0, top - run:top] = True
        L, u = place_decisions(a, T)
        m = ptswap(T, L, u)[0]
        assert m[0, top - run] == top
        return multihop(m, nt)

    # from a block's top position (8): 2 nt - 1 = 5 ranks down is the neighbouring block's bottom position, one more leaves that block
    assert [flag(8, r) for r in (2, 3, 4, 5)] == [False] * 4 and [flag(8, r) for r in (6, 7, 8)] == [True] * 3
    # from a block's bottom position (6): nt ranks down is the neighbouring block's bottom, one more crosses it
    assert [flag(6, r) for r in (1, 3, 4)] == [False, False, True]
    assert not multihop(np.arange(n), nt) and multihop(np.array([[6, 1, 2, 3, 4, 5, 0, 7, 8, 9, 10, 11]]), nt)


@pytest.mark.parametrize("n", [17, 2409])
def test_edge_values_restatement_equals_oracle(n):
    T, L, u, (p0, p1, p2) = edge_case(n)
    m, inv, acc = ptswap(T, L, u)
    mo, acco = oracle_sweep(T, L, u)
    assert np.array_equal(m, mo) and np.array_equal(acc, acco)
    # a -inf or NaN likelihood makes every sum it enters a NaN: its pairs reject even at u = 0, and it stays where it is
    assert m[0, p0] == p0 and not acc[0, p0] and not acc[0, p0 - 1] and acc[0].sum() == n - 3
    assert m[1, p1] == p1 and m[1, p1 - 1] == p1 - 1 and m[1, n - 1] == n - 1 and not acc[1, [p1, p1 - 1, p1 - 2, n - 2]].any()
    assert m[2, p2] == p2 and not acc[2, [p2, p2 - 1]].any() and acc[1].any() and acc[2].any()
    assert acc[3].all()                                               # exact ties accept at the largest uniform
    nb = (n - 1 + BATCH - 1) // BATCH
    assert nb - 1 >= (2 if n > 17 else 1)                             # the runs of accepts of walkers 0 and 3 span that many batch edges


def test_route_tables_sit_on_the_edges_of_the_launchers_rule():
    for fused, table in ((1, FUSED_ROUTES), (0, TWO_KERNEL_ROUTES)):
        for n, route in table.items():
            assert model_route(n, fused) == route, (fused, n)
        ns = sorted(table)
        edges = [n for n in range(129 if fused else 2, 2420) if model_route(n, fused) != model_route(n - 1, fused)]
        assert edges == [n for n in ns if n <= 2409 and (n - 1 in ns or (fused and n == 129))], (fused, edges)    # (2410, 2417: more direct stores)
    assert {(n - 1) % BATCH for n in (2409, 2410, 2417)} == {0, 1}
    assert expected_launch(1, 2267) == (SWL_FUSED, 8, 163824, 0) and expected_launch(0, 2408) == (SWL_LDS, 8, 163808, 0)
    assert expected_launch(0, 2409, hop=1) == (SWL_DIRECT, 64, 0, 0)


@pytest.mark.parametrize("n,W", sorted({(n, W) for _, n, W in ROUTE_CASES}))
def test_route_case_inputs_prove_something(n, W):
    c = RouteCase(n, W).run_oracle()
    assert c.moved0 and 0.2 <= c.share <= 0.8, (n, W, c.share, c.moved0)
    assert all((s["slot_of"] != np.arange(n)).any() for s in c.snap)         # sweeps two and three start from non-identity tables


def test_oddeven_route_case_inputs_prove_something():
    c = RouteCase(2409, 70, swap_mode="oddeven").run_oracle()
    assert c.moved0 and 0.2 <= c.share <= 0.8, (c.share, c.moved0)
    assert [orc.swap_parity(it, 1) for it in c.ITS] == [1, 0, 1]
