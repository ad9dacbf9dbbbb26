"""Batched parallel-tempering engine: host-side driver of libptmi.so.

One ``PTEngine`` owns the chains of ``nwalkers`` independent replicas x ``ntemps``
temperature ranks on one MI355X and advances them with the fused HIP kernels.  The
host part below is the epoch logic of the reference's ``PTMCMCOneStep``
(PTMCMCSampler/PTMCMCSampler.py:545-585: covariance epoch, DE epoch, DE activation)
and the iteration loop of ``sample()`` (:495-528), restated for a batch; everything
per-chain runs on the device.  Device memory is held in torch tensors (plumbing only:
allocation, host<->device copies, and RCCL in ``sharded.py``).
"""
import ctypes as C

import os

import numpy as np

from . import _lib
from ._build import _usable_cores
from .callback_path import CallbackPath, _BoxDrawJump, _torch, box_draw_jump  # noqa: F401  (box_draw_jump is imported from here)
from .ladder import temperature_ladder


_BLAS_CTL = None


def _blas_threads(n):
    """Context that caps the BLAS thread pools at ``n``.  The controller is built once: discovering the loaded BLAS
    libraries is what costs (0.2 ms per call, a third of a 100 x 100 factorization)."""
    global _BLAS_CTL
    try:
        if _BLAS_CTL is None:
            from threadpoolctl import ThreadpoolController
            _BLAS_CTL = ThreadpoolController()
        return _BLAS_CTL.limit(limits=n)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def _blas_single_thread():
    return _blas_threads(1)


def factorize(cov, per_walker):
    """Eigen-directions U (columns) and variances S of a jump covariance.

    Per-walker mode is the reference's call, ``np.linalg.svd`` (PTMCMCSampler.py:145, 803), on one BLAS thread (LAPACK's
    last bits depend on the thread count; a 100 x 100 factorization gains nothing from more).  Pooled mode is not a
    replica of a reference run and uses the symmetric solver: ``np.linalg.eigh``, eigenvalues by decreasing size and
    in absolute value (what the SVD of a symmetric matrix returns up to signs), 2.5x cheaper at 1000 x 1000 where the
    factorization dominates the covariance epoch; beyond 256 parameters it runs on 8 BLAS threads."""
    if per_walker:
        with _blas_threads(1):
            U, S, _ = np.linalg.svd(cov)
        return U, S
    with _blas_threads(1 if len(cov) <= 256 else 8):
        w, V = np.linalg.eigh(cov)
    return np.ascontiguousarray(V[:, ::-1]), np.abs(w[::-1])



def hist_spec(ndim, hist):
    """``hist=(lo, hi, nbins)`` of ``PTEngine.with_stages`` -> (lo [ndim], hi [ndim], nbins), checked: scalars or [ndim], lo < hi and
    finite, 2 <= nbins <= 1024 (``ptmi_hist_attach``)."""
    try:
        lo, hi, nbins = hist
    except (TypeError, ValueError):
        raise ValueError("hist=(lo, hi, nbins)") from None
    if int(nbins) != nbins or not 2 <= int(nbins) <= 1024:
        raise ValueError("hist: 2 <= nbins <= 1024 (got %r)" % (nbins,))
    out = []
    for name, v in (("lo", lo), ("hi", hi)):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(ndim, float(v))
        if v.shape != (ndim,):
            raise ValueError("hist: %s is a scalar or has ndim = %d entries (got shape %r)" % (name, ndim, v.shape))
        out.append(np.ascontiguousarray(v))
    lo, hi = out
    bad = ~(np.isfinite(lo) & np.isfinite(hi) & (lo < hi))
    scale = int(nbins) / np.where(bad, 1.0, hi - lo)
    bad |= ~np.isfinite(scale)
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise ValueError("hist: lo < hi, both finite (parameter %d: lo = %r, hi = %r)" % (j, lo[j], hi[j]))
    return lo, hi, int(nbins)


def hist_edges(lo, hi, nbins):
    """The bin edges lo + k (hi - lo) / nbins, [d][nbins + 1]; the last one is hi itself."""
    k = np.arange(nbins + 1, dtype=np.float64)
    e = lo[:, None] + k[None, :] * ((hi - lo) / nbins)[:, None]
    e[:, nbins] = hi
    return e


def best_pick(score, iters):
    """The walker ``PTEngine.best`` reports for one plane: the device's rule (include/ptmi.h ``ptmi_best_attach``) over ascending walker
    index -- a walker that holds something (``iters >= 0``) replaces the pick iff nothing is picked yet or its score is ``>`` the
    pick's, so the lowest index wins a tie; -1 where no walker holds anything."""
    pick = -1
    for w in range(len(iters)):
        if iters[w] >= 0 and (pick < 0 or score[w] > score[pick]):
            pick = w
    return pick


class _RingReader(object):
    """A stage that reads the cold chains' AM ring a second time: iterations ``first + 1`` on, ``iter`` the last one taken.
    ``update(eng, lo, hi, n_done)`` issues the stage's C call for iterations ``lo .. hi`` of the period the ring holds, ``n_done`` taken
    before.  The engine comes in with every call: a reader that held it would keep it from being freed where its last name goes."""
    # name: what the messages call it, how with_stages asks for it, what it does to an iteration, what restore() says without its state
    WORDS = {"hist": ("histogram", "hist=(lo, hi, nbins)", "counted",
                      "the checkpoint carries no histogram: it was written by a run without hist="),
             "pairs": ("pair histogram", "pairs=(pairs, lo, hi, nbins)", "counted",
                       "the checkpoint carries no pair histograms of this shape: it was written by a run without pairs= (or with other pairs or bins)"),
             "diag": ("diagnostics", "diag=True", "folded",
                      "the checkpoint carries no diagnostics sums of this shape: it was written by a run without diag=True (or with other diag_levels)"),
             "samples": ("sample buffer", "samples=slots", "taken",
                         "the checkpoint carries no sample buffer of this shape: it was written by a run without samples= (or with other slots, every or samples_from)"),
             "best": ("best-fit tracker", "best=True", "compared",
                      "the checkpoint carries no best-fit rows of this shape: it was written by a run without best=True (or with another best_from)")}

    def __init__(self, name, first, update):
        self.name, self.first, self.iter, self.update = name, first, first, update

    def sync(self, eng, it):
        """The engine's ``<name>_sync(it)``."""
        if int(it) > eng.iter:
            raise ValueError("%s_sync(%d): the engine has reached iteration %d; the ring's rows beyond it are the period before's"
                             % (self.name, int(it), eng.iter))
        self.advance(eng, it)

    def advance(self, eng, it):
        """Take iterations ``(iter, it]``; ``it`` is not held against the engine's iteration (``update_cov`` ends a period this way)."""
        it = int(it)
        if it <= self.iter:
            return
        base = ((it - 1) // eng.cov_update) * eng.cov_update
        if self.iter < base and eng.owns_cold:
            raise ValueError("%s_sync(%d): iterations %d..%d are no longer in the ring (it holds the period after %d); every period "
                             "must end through update_cov" % (self.name, it, self.iter + 1, base, base))
        self.update(eng, self.iter + 1, it, self.iter - self.first)
        self.iter = it


def _ring_attr(name, field):
    """``PTEngine.<name>_from`` / ``<name>_iter``: the reader's ``first`` / ``iter`` (an engine without the stage has no such attribute)."""
    return property(lambda self: getattr(self._reader(name), field))


def interval_par(a, b, d):
    """Parameters of the ("interval", a, b) family (include/ptmi.h PTMI_LOGL_INTERVAL): a, w = b - a, log w."""
    a = np.broadcast_to(np.asarray(a, np.float64), (d,))
    b = np.broadcast_to(np.asarray(b, np.float64), (d,))
    if not np.all(b > a):
        raise ValueError("interval logl needs a < b")
    w = b - a
    return np.ascontiguousarray(np.concatenate([a, w, np.log(w)]))


class PTEngine(CallbackPath):
    """Chains of ``nwalkers`` x ``ntemps`` on one GPU.

    Parameters mirror the reference's sampler: ``cov0`` is the initial jump covariance
    (``PTSampler.__init__`` ``cov``), ``weights`` = (SCAMweight, AMweight, DEweight),
    ``cov_update`` = covUpdate, ``burn`` = burn (also the DE-buffer length), ``tskip`` =
    Tskip.  ``cov_mode``: ``"per_walker"`` makes every walker a faithful replica of a
    reference run (own covariance, eigenvectors and DE history); ``"pooled"`` adapts one
    covariance from all walkers' rank-0 samples.  ``logl`` / ``logp`` select the built-in
    device likelihood / prior: ("iso",), ("dense", mu, P) with P a (symmetric) precision matrix, ("curved",),
    ("interval", a, b) = the unit Gaussian on the box (a, b) in the coordinates of the reference's ``intervalTransform`` (its own NUTS
    workload, tests/test_nuts.py:13-140; ndim <= 512); ("flat",), ("box", lo, hi).  ``swap_mode``: ``"sweep"`` is the reference's hot -> cold PTswap; ``"oddeven"`` tries
    the disjoint pairs (k, k+1), k = swap epoch (mod 2), all at once (see include/ptmi.h).  ``pick_mode``: ``"chain"`` =
    every chain draws its own entry of the proposal cycle (the reference's ``_jump``); ``"walker"`` = one draw per walker
    and iteration fixes the proposal type of all its temperature ranks (wave-uniform on the device, include/ptmi.h).
    ``nuts_maxdepth``: NUTS stops doubling at this tree height.  The reference doubles ``while s == 1`` with no cap
    (nutsjump.py:716-802); the default 24 (2^24 leapfrogs in one call, the ABI's limit) is out of reach of any run, i.e. the
    reference's behaviour.  A lower value is an engine option (bounded cost per call).  Memory: the tree scratch holds
    7 + 4 (maxdepth + 1) vectors of ndim doubles and 4 (maxdepth + 1) scalars per chain (107 vectors at 24, 51 at 10):
    86 KB per chain at ndim = 100, i.e. 22 GB for 262 144 chains -- lower it for very large batches.
    ``split_nuts=True`` (with ``split=True``): NUTS on the callback path too -- ``grad_weights=(w_nuts, w_hmc)`` with ``w_nuts > 0``,
    the trees built round by round from the batched gradient callbacks (``gradient_stage``).  Opt-in: an iteration then takes as
    many host-synchronised callback rounds as its deepest tree has leaves (a chain's first NUTS call up to ~200 more for the
    step-size search), and the stage's work area grows with ``nuts_maxdepth`` (include/ptmi.h ``ptmi_gj_work_bytes``).
    ``grad_weights`` beyond 512 parameters, up to 2048: HMC alone on the callback path -- ``split=True`` or ``rows_logl=True`` with
    ``grad_weights=(0, w_hmc)``; the stage's whitening products then run on the matrix cores (csrc/ptmi_gjcb_wide.hip).  NUTS
    (``grad_weights[0] > 0``, ``split_nuts=True``), the fused kernels' gradient jumps and the interval family stop at 512: ValueError.
    ``eig_mode``: who factorizes the adapted covariance at a covariance epoch (PTMCMCSampler.py:797-803): ``"lapack"`` = the
    host, exactly as the reference (``np.linalg.svd`` per walker); ``"jacobi"`` = ``ptmi_eig_jacobi`` on the device, one
    block per walker, no host round trip (ndim <= 101, one parameter group; same subspaces, its own sign rule); ``"ql"`` =
    ``ptmi_eig_ql``, Householder tridiagonalization + implicit QL on the device (ndim <= 1024, parameter groups included; up to 128 x 128 the
    matrix lives in LDS -- a quarter of the Jacobi kernel's time on nearly degenerate spectra, two matrices per CU -- beyond that in a
    global scratch, factorized in batches: the choice for thousands of per-walker covariances, the oracle's bits at every size);
    ``"hipsolver"`` = the ROCm library's symmetric eigensolver on the engine's stream (``torch.linalg.eigh`` on the device
    tensor: no host round trip either; with parameter groups one call per group's block) -- the choice for large ndim, where the host's LAPACK call is the
    epoch (1000 x 1000: 22 ms against 83 ms on 8 host threads; at ndim = 100 the host's 0.6 ms wins).  Like LAPACK's, its
    last bits are the library's: such a run is not bit-reproducible against the oracle, only its decomposition is checked.
    ``"sytrd"`` = ``ptmi_eig_sytrd`` for ONE large pooled covariance (ndim <= 1024), all of it the library's own kernels: Householder
    tridiagonalization in one kernel with the matrix in the LDS of 64 blocks (a quarter of the CUs), the tridiagonal matrix's
    eigenvectors by divide and conquer (csrc/ptmi_dc.inc.h), back-transformed through the reflectors -- 12.6 ms at 1000 x 1000 where the
    ROCm library's own reduction is 7000 launches of one-block kernels, two thirds of its 35 ms.  No oracle restates its last bits; the
    tests check every table it makes against the covariance and step the oracle's chains with it.
    ``eig_lag`` (L >= 0 launches; pooled covariance): the eigenvectors of a covariance epoch take effect L launches late --
    ``run`` queues the L launches that follow the epoch (and their swaps) with the table in force, the factorization runs
    MEANWHILE, and the launch after them uses the result (a new epoch finishes a pending one first).  The reference applies the
    table at once (PTMCMCSampler.py:560); the pooled covariance is an engine mode anyway, and with L = 1 the adaptation sees its
    table a tenth of a period late.  ``eig_mode="lapack"``: the host factorizes while the GPU samples (L = 1 hides it at
    ndim = 100); ``eig_mode="hipsolver"``: the library's kernels run on a side stream BESIDE the launches (22 ms at ndim = 1000
    beside 2.6 ms launches: L = 9).  Same statistics, same factorization, no GPU idle time at the epoch (oracle:
    ``OracleEngine(eig_lag=L)``).  ``eig_mode="ql"`` (pooled or per-walker covariances, one GPU): ``ptmi_eig_ql_from`` on the side
    stream; built and bit-exact, but no faster at 4096 walkers -- the step launches slow down by what the factorization takes.
    ``am_mode``: how the rank-0 chain's samples (updateChains' buffer, PTMCMCSampler.py:327-328) are kept between covariance
    epochs.  ``"rows"``: every step stores its row.  ``"rle"`` (pooled covariance): a rejected proposal leaves the chain where it
    was, so a step stores its row only when it was accepted (or is a KEY row: first step of a launch, ring rows 0 and 1, the
    swap's row) plus a flag word, and the pooled statistics take every stored row once, weighted by its run length (include/ptmi.h
    ``AMflag``; oracle: ``orc_pool_update_rle`` -- the same sample covariance, summed in another order).  Readers that want
    every row (``get("AM")``, the DE history, chain files) get the repeats copied forward first (``am_expand``).
    ``"auto"`` = ``"rle"`` where it applies.
    ``rows_logl=True`` (``logl`` ("iso",) or ("dense", mu, P)): ``init_state`` / ``run`` / ``mh_steps`` take the split path -- propose, the
    built-in likelihood and prior as ROW kernels over the launch's proposals (``ptmi_rows_logl``, ``ptmi_rows_logp``; for the dense
    family one matrix-core product per iteration, csrc/ptmi_dense_rows.hip), accept -- instead of the fused step kernels, which beyond
    104 parameters stream the d x d table per chain-step from L2.  The same chains bit for bit (the row kernels restate the oracle's
    sums); HMC / NUTS in the cycle are served by ``ptmi_rows_logl_grad`` through the batched gradient stage (NUTS: ndim <= 512; HMC: ndim <= 2048).  Whatever
    ``run_callback`` supports; not with ``w_host`` or a sharded ladder (``ntemps_global`` / ``temp0``).  ``am_mode="auto"`` is ``"rows"``
    here (the split path stores every rank-0 row), so with a POOLED covariance the bits are those of the fused path with
    ``am_mode="rows"``; its default ``"rle"`` sums the same pooled statistics in another order.
    ``jumps=[(func, weight), ...]`` (with ``w_host`` = the sum of the weights, or 0 for that; ``split=True`` or ``rows_logl=True``): the
    cycle's custom entries (the reference's ``addProposalToCycle``, PTMCMCSampler.py:988-1014, 1058-1059) as BATCHED device callbacks --
    ``func(X[n, d], iter, beta[n]) -> (Q[n, d], qxy[n] | 0 | None)`` on torch tensors of this GPU, once per iteration for all chains
    whose pick is that function (``jump_stage``; include/ptmi.h ``ptmi_cj_*``).  ``box_draw_jump(lo, hi)`` is the reference's
    ``UniformJump`` as a library kernel.  ``get("cjstat")`` [W][nt][w_host][2]: proposed / accepted per pick index by rank.  Not in
    graph mode.  Beside gradient jumps (``grad_weights``) with ``with_stages(..., jumps_with_grad=True)``: the reference's cycle of custom entries, HMC,
    NUTS, SCAM, AM and DE, picked in the order [custom, SCAM, AM, DE, NUTS, HMC]; every proposal launch is then followed by both
    stages, which serve disjoint chains (opt-in, like ``split_nuts``: without the keyword the combination is refused).
    ``aux=[func, ...]`` (``split=True`` or ``rows_logl=True``): the reference's auxiliary jumps (``addAuxilaryJump``,
    PTMCMCSampler.py:1017-1028, run on every jump's result at :1062-1065) as BATCHED device callbacks -- ``func(X[n, d], Q[n, d], iter,
    beta[n]) -> (Q'[n, d], qxy[n] | 0 | None)`` on torch tensors of this GPU, ``n = W * nt``: every chain, in slot order.  ``X`` holds
    the chains' states (gathered once per iteration, ``ptmi_aux_begin``: between the launches of a segment a state lives in X or in a
    proposal buffer), ``Q`` is the proposal buffer itself (edit it in place, or return a tensor of your own); the functions run in the
    order given, each on the ``Q`` of the one before, their ``qxy`` added to the jump's in that order (``aux_stage``).  Not in graph mode.
    ``jumps_with_grad`` and ``aux`` are keywords of the alternative constructor ``PTEngine.with_stages(..., jumps_with_grad=True,
    aux=[f])``, which takes everything the plain constructor takes: the plain constructor's parameters stay what they were.
    ``with_stages(..., logl_in_support=True)`` (``split=True`` or ``rows_logl=True``): the likelihood callback is called only on rows
    inside the prior's support, as the reference does it (``lp = logp(y)``; ``logl(y)`` only when ``lp != -inf``, PTMCMCSampler.py:605-612,
    479-487) -- ``eval_callback`` lists the rows whose prior is not -inf (include/ptmi.h ``ptmi_sup_*``: one host read-back per iteration),
    hands ``logl`` the compacted rows ``[n, d]`` and scatters its ``n`` values back.  For likelihoods that are undefined outside the support
    (a Cholesky factorization, a logarithm of a parameter) and for expensive ones under a tight prior; the chains are the same bit for
    bit for a row-wise callback.  The gradient callbacks are not filtered (the reference's are not either, nutsjump.py:71-76).  With a flat
    prior (``logp=None``) the stage launches nothing.  Not in graph mode.  ``support_counts``: (rows offered, rows handed to ``logl``).
    ``with_stages(..., hist=(lo, hi, nbins), hist_from=None)``: the marginal posterior histograms of EVERY walker's cold chain, accumulated
    on the device from the AM ring (include/ptmi.h ``ptmi_hist_*``: ``t = (x - lo) * (nbins / (hi - lo))``, below 0 and NaN -> ``under``, at
    or above ``nbins`` -> ``over``, else bin ``int(t)``).  ``lo`` / ``hi``: scalars or ``[ndim]``; iterations ``hist_from + 1`` on are counted
    (default ``hist_from = burn``).  ``update_cov`` counts the period that ends before it touches anything else, so every way of running
    the engine is served; ``hist_sync(it)`` counts up to an iteration inside a period, ``hist_counts(it=None)`` returns the result.  The
    ring is only read: the chains are the same bits with and without.  ``t["hist"]`` and ``hist_iter`` are part of ``checkpoint()``.
    ``with_stages(..., pairs=(pairs, lo, hi, nbins), pairs_from=None)``: the joint posterior histograms of parameter PAIRS of every
    walker's cold chain -- the off-diagonal panels of a corner plot -- from the same ring with the same rule per axis (include/ptmi.h
    ``ptmi_pairs_*``, pairs.py ``pairs_rule``: both coordinates inside -> cell ``[int(ti)][int(tj)]``, else the pair's ``outside``).
    ``pairs``: an integer ``[npairs][2]`` array ((j, i) is the transpose of (i, j)) or ``{"params": [indices]}`` = every pair ``(a, b)``
    with ``a`` before ``b`` in the list; ``2 <= nbins <= 128``, ``npairs <= 8192``; ``pairs_from``, ``pairs_sync(it)``, ``pairs_counts(it=None)``
    as the histogram's; both stages may run on one engine.  ``t["pairs"]`` and ``pairs_iter`` are part of ``checkpoint()``.
    ``with_stages(..., evidence=True, evidence_from=None, evidence_every=1)``: the ladder's summaries for the log-evidence ln Z (include/ptmi.h
    ``ptmi_ev_*``, evidence.py): per walker and rank the count, mean and variance of lnL (shifted sums) and the running log-sum-exp of
    ``dbeta_r * lnL``, ``dbeta_r = beta_{r-1} - beta_r`` from ``temps_mh`` (``hot_chain=True``: beta = 1e-80 at the last rank, the last
    stone reaches the prior).  ``swap(it)`` -- the one call every path swaps through -- takes a sample behind the swap when
    ``it > evidence_from`` (default ``burn``) and ``(it // tskip) % evidence_every == 0``: the POST-swap state of a swap iteration, the row
    the reference's chain files hold for it.  The sampling period is ``tskip * evidence_every`` iterations; with autocorrelation times
    in the hundreds of iterations (tau about 600 at 100-d) a sample every ``tskip`` iterations loses next to nothing
    against one per iteration.  ``evidence_moments()`` returns the accumulators, ``evidence()`` the estimates (thermodynamic integration,
    its second-order correction, stepping stones; per walker and with standard errors from the walkers' scatter).  lnL is only read:
    the chains are the same bits with and without.  ``t["ev_acc"]``, ``t["ev_cnt"]`` and ``ev_epochs`` are part of ``checkpoint()``.
    ``with_stages(..., diag=True, diag_from=None, diag_batch=1, diag_levels=16)``: convergence diagnostics from EVERY walker's cold chain
    (include/ptmi.h ``ptmi_diag_*``, diagnostics.py): per walker and parameter the shifted sums ``S1``, ``S2`` and, over a binary counter of
    batches of ``diag_batch << l`` iterations, ``l < diag_levels``, the sums of squared batch sums -- streamed on the device from the AM ring
    for iterations ``diag_from + 1`` on (default ``diag_from = burn``), bit-defined whatever the ring mode.  ``update_cov`` folds the period
    that ends before it touches anything else; ``diag_sync(it)`` folds up to an iteration inside a period, ``diag_moments(it=None)``
    returns the planes, ``diagnostics(it=None)`` the estimates: Gelman-Rubin ``rhat``, ``tau`` (batch means pooled over the walkers),
    ``tau_walkers``, ``ess``.  The ring is only read: the chains are the same bits with and without.  ``t["diag"]`` and ``diag_iter`` are
    part of ``checkpoint()``.  Refused on an engine that owns no cold ring (``temp0 != 0``).
    ``with_stages(..., samples=slots | dict(slots=, every=1), samples_from=None)``: thinned SAMPLES of every walker's cold chain, kept on
    the device (include/ptmi.h ``ptmi_samples_*``, samples.py): a buffer of ``slots`` snapshots ``[W][ndim]`` in parameter order, each row
    with its lnL and lp (``keep_lnl=True``), gathered from the AM ring whatever the ring mode.  The candidates are the iterations
    ``samples_from + every * m`` (default ``samples_from = burn``); when the buffer is full every other snapshot is let go and the stride
    doubles (``SlotPlan``), so the held snapshots are evenly spaced over the whole run so far, between ``slots // 2`` and ``slots`` of
    them, and the run's length need not be known.  ``update_cov`` takes the period that ends before it touches anything else;
    ``samples_sync(it)`` takes up to an iteration inside a period, ``samples(it=None)`` returns the held snapshots by iteration (host
    arrays), ``samples_device()`` the same as device tensors.  The ring is only read: the chains are the same bits with and without.
    ``t["samples"]``, ``t["samples_aux"]``, ``samples_iter`` and the plan's state are part of ``checkpoint()``, with ``every`` and
    ``samples_from``: ``restore()`` refuses a checkpoint whose buffer was filled on another schedule.  Idle on an engine that
    owns no cold ring.
    ``with_stages(..., best=True, best_from=None)``: the BEST-FIT row of every walker's cold chain over ALL iterations, tracked on the
    device (include/ptmi.h ``ptmi_best_*``): per walker the row with the largest ``lnprob = (1 / temps_mh[0]) * lnlike + lp`` (MAP) and
    the row with the largest ``lnlike`` (ML), each in parameter order with its score, lnL, lp and iteration (``keep_lnl=True``), compared
    from the AM ring whatever the ring mode.  ``best_from`` defaults to 0, not ``burn``: an optimum is an optimum whenever it was
    visited; iteration 0 (``p0``) is not in the ring and is not a candidate.  A candidate replaces the held row iff its score is not NaN
    and nothing is held or the score is ``>`` the held one, so the earliest iteration with the maximum wins however the run is cut
    into calls.  ``update_cov`` takes the period that ends before it touches anything else; ``best_sync(it)`` takes up to an iteration
    inside a period, ``best(it=None, per_walker=False)`` returns the best point of all walkers (host), ``best_device()`` the per-walker
    device tensors.  The ring is only read: the chains are the same bits with and without.  ``t["best"]``, ``t["best_val"]``,
    ``t["best_iters"]``, ``best_iter`` and ``best_from`` are part of ``checkpoint()``: ``restore()`` refuses a checkpoint without them or
    with another ``best_from``.  Idle on an engine that owns no cold ring.
    ``with_stages(..., adapt_ladder=True | dict(every=10, kappa=2.0, t0=10.0, until=None))``: the temperature ladder adapts during burn-in
    from EVERY walker's accepted swaps (include/ptmi.h ``ptmi_ladder_*``).  ``swap(it)`` counts the swap epochs of a window by the parity
    of the pairs they try (``swap_mode="oddeven"``: epoch ``it // tskip`` tries the pairs of its parity, so ``every`` is even; the sweep
    tries all); behind the ``every``-th, while ``it <= until`` (default ``burn``), the device turns the window's acceptance per pair into
    new log gaps with the gain ``kappa * t0 / (updates so far + t0)`` -- a pair that accepts more than the others gets a wider gap -- and
    rewrites its temperature tables in place: no host round trip, nothing re-evaluated, captured graphs stay valid.  Both ends of the
    ladder stay (``Tmax`` keeps its meaning, the evidence integral its range; a ``hot_chain`` rank keeps 1e80).  After ``until`` the
    ladder is frozen and the run is ordinary parallel tempering: adaptation belongs to burn-in, and with ``evidence=True``
    ``until <= evidence_from``.  ``ladder`` / ``temps_mh`` / ``ev_dbeta`` show what the device holds (read back on first use after an
    update), ``ladder0`` / ``temps_mh0`` stay the constructor's; ``ladder_history()`` returns every update.  ``t["lad"]``,
    ``t["lad_seen"]``, the open window's counts and the history are part of ``checkpoint()``.  One GPU, a whole ladder.
    ``stats_async`` (pooled covariance with ``eig_lag >= 1``): the statistics of a covariance period that is over need nothing the next
    launches touch once those write ANOTHER ring -- so the engine keeps two rings (``t["AM"]`` is always the one in use), switches at
    every covariance epoch, and runs the period's statistics (``ptmi_update_cov_on``) and the factorization behind them on a side
    stream BESIDE the launches that follow; the table still takes effect ``eig_lag`` launches after the epoch.  A scheduling change
    only: every result equals the run without it bit for bit (oracle: ``OracleEngine(eig_lag=L)``).  Needs burn to be a multiple of
    cov_update when a DE history is kept (a DE epoch then reads the finished period's ring before the switch).
    """

    # what PTEngine.with_stages sets on the instance before __init__ runs (the plain constructor leaves the class defaults)
    _hist = None
    _hist_from = None
    _pairs = None
    _pairs_from = None
    _samples = None
    _samples_from = None
    _best = False
    _best_from = None
    _ev = False
    _ev_from = None
    _ev_every = 1
    _diag = False
    _diag_from = None
    _diag_batch = None
    _diag_levels = None
    _adapt = None
    adapt_on = False
    _lad_stale = False

    # the host's mirrors of the device's temperature tables.  With adapt_ladder the device rewrites them (ptmi_ladder_update): the
    # mirrors are then read back on their first use after an update (ptmi_ladder_read: one wait for the stream), never per update
    def _lad_refresh(self):
        if self._lad_stale:
            self._lad_stale = False
            lad, tm, be = np.empty(self.ntg), np.empty(self.nt), np.empty(self.nt)
            dp = _lib._dp
            _lib.check(self.lib.ptmi_ladder_read(self.h, lad.ctypes.data_as(dp), tm.ctypes.data_as(dp), be.ctypes.data_as(dp)))
            self._ladder, self._temps_mh = lad, tm
            if self.evidence_on:
                db = self._ev_dbeta.copy()
                db[1:] = be[:-1] - be[1:]                             # as the publish step writes it; dbeta[0] stays
                self._ev_dbeta = db

    ladder = property(lambda self: (self._lad_refresh(), self._ladder)[1], lambda self, v: setattr(self, "_ladder", v))
    temps_mh = property(lambda self: (self._lad_refresh(), self._temps_mh)[1], lambda self, v: setattr(self, "_temps_mh", v))
    ev_dbeta = property(lambda self: (self._lad_refresh(), self._ev_dbeta)[1], lambda self, v: setattr(self, "_ev_dbeta", v))

    @classmethod
    def with_stages(cls, *args, jumps_with_grad=False, aux=None, logl_in_support=False, hist=None, hist_from=None,
                    evidence=False, evidence_from=None, evidence_every=1, diag=False, diag_from=None, diag_batch=None, diag_levels=None,
                    adapt_ladder=None, pairs=None, pairs_from=None, samples=None, samples_from=None, best=False, best_from=None, **kw):
        """``PTEngine(*args, **kw)`` with the stages of the composed ``_jump`` on the callback path (see the class docstring):
        ``jumps_with_grad=True`` lets ``jumps=`` stand beside ``grad_weights`` in one cycle, ``aux=[func, ...]`` are the auxiliary jumps,
        ``logl_in_support=True`` hands the likelihood callback only the rows whose prior is not -inf (``eval_callback``),
        ``hist=(lo, hi, nbins)`` with ``hist_from`` accumulates the marginal histograms of every cold chain (``hist_counts``),
        ``evidence=True`` with ``evidence_from`` / ``evidence_every`` (default 1) the ladder's lnL summaries for ln Z (``evidence``),
        ``diag=True`` with ``diag_from`` / ``diag_batch`` (default 1) / ``diag_levels`` (default 16) the streaming sums of every cold chain
        for R-hat and ESS (``diagnostics``), ``adapt_ladder=True`` or ``dict(every=10, kappa=2.0, t0=10.0, until=None)`` adapts the
        temperature ladder during burn-in from every walker's accepted swaps (``ladder_history``),
        ``pairs=(pairs, lo, hi, nbins)`` with ``pairs_from`` accumulates the joint histograms of parameter pairs of every cold chain
        (``pairs_counts``; ``pairs``: int ``[npairs][2]`` or ``{"params": [indices]}`` = every pair of the list),
        ``samples=slots`` or ``dict(slots=, every=1)`` with ``samples_from`` keeps evenly spaced snapshots of every cold chain on the device
        (``samples``, ``samples_device``), ``best=True`` with ``best_from`` (default 0, not ``burn``: an optimum is an optimum whenever
        it was visited) tracks the MAP and the ML row of every cold chain over all iterations (``best``, ``best_device``; iteration 0,
        the starting point, is not in the ring and is not a candidate).
        The plain constructor keeps the parameters it had (tests/test_gj_groups.py holds them to the letter) and its refusals."""
        self = cls.__new__(cls)
        self.jumps_with_grad = bool(jumps_with_grad)
        self._aux = list(aux) if aux is not None else []
        self.logl_in_support = bool(logl_in_support)
        self._hist, self._hist_from = hist, hist_from
        self._pairs, self._pairs_from = pairs, pairs_from
        self._samples, self._samples_from = samples, samples_from
        self._best, self._best_from = bool(best), best_from
        self._ev,self._ev_from, self._ev_every = bool(evidence), evidence_from, evidence_every
        self._diag, self._diag_from, self._diag_batch, self._diag_levels = bool(diag), diag_from, diag_batch, diag_levels
        self._adapt = adapt_ladder
        self.__init__(*args, **kw)
        return self

    def __init__(self, ndim, ntemps, nwalkers, cov0, ladder=None, logl=("iso",), logp=("flat",),
                 weights=(20, 20, 20), cov_update=1000, burn=10000, tskip=100, seed=0,
                 cov_mode="per_walker", hot_chain=False, Tmin=1, Tmax=None,
                 ntemps_global=None, temp0=0, walker0=0, device=0, split=False, use_de_buffer=None,
                 w_host=0, keep_lnl=False, groups=None, swap_mode="sweep",
                 grad_weights=(0, 0), hmc=(0.1, 2, 300), nuts_delta=0.6, nuts_maxdepth=24, pick_mode="chain",
                 eig_mode="lapack", am_mode="auto", eig_lag=0, stats_async=False, split_nuts=False, rows_logl=False, jumps=None):
        torch = _torch()
        # jumps=, aux=, logl_in_support: the callback path's stages (callback_path.py), refused first of all
        w_host = self._check_callback_stages(split, rows_logl, w_host, grad_weights, jumps)
        # posterior histograms of the cold chains (with_stages(hist=(lo, hi, nbins), hist_from=...); see the class docstring)
        self._ring = []                                               # the ring's second readers, in the order update_cov serves them
        self.hist_spec = None if self._hist is None else hist_spec(int(ndim), self._hist)
        self._ring_reader("hist", self.hist_spec is not None, self._hist_from, burn,
                          lambda eng, lo, hi, n: _lib.check(eng.lib.ptmi_hist_update(eng.h, lo, hi)))
        # joint histograms of parameter pairs of the cold chains (with_stages(pairs=(pairs, lo, hi, nbins), pairs_from=...); see the class docstring)
        self.pairs_spec = None
        if self._pairs is not None:
            from .pairs import pairs_spec
            self.pairs_spec = pairs_spec(int(ndim), self._pairs)
        self._ring_reader("pairs", self.pairs_spec is not None, self._pairs_from, burn,
                          lambda eng, lo, hi, n: _lib.check(eng.lib.ptmi_pairs_update(eng.h, lo, hi)))
        # convergence diagnostics of the cold chains (with_stages(diag=True, diag_from=..., diag_batch=..., diag_levels=...); see the class docstring)
        self.diag_on = bool(self._diag)
        if self.diag_on:
            from .diagnostics import MAX_LEVELS
            b0 = 1 if self._diag_batch is None else self._diag_batch
            L = MAX_LEVELS if self._diag_levels is None else self._diag_levels
            if not isinstance(b0, (int, np.integer)) or not 1 <= int(b0) < 2 ** 31:
                raise ValueError("diag_batch = %r: the level-0 batch length, an integer >= 1" % (b0,))
            if not isinstance(L, (int, np.integer)) or not 1 <= int(L) <= MAX_LEVELS:
                raise ValueError("diag_levels = %r: 1 <= diag_levels <= %d" % (L, MAX_LEVELS))
            if int(temp0) != 0:
                raise ValueError("diag=True reads the cold chains' ring: this engine (temp0 = %d) holds no rank 0 and owns no cold ring at "
                                 "all; the stage belongs on the block with temp0 = 0" % int(temp0))
            self.diag_batch, self.diag_levels = int(b0), int(L)
        elif self._diag_from is not None or self._diag_batch is not None or self._diag_levels is not None:
            raise ValueError("diag_from= / diag_batch= / diag_levels= go with diag=True")
        self._ring_reader("diag", self.diag_on, self._diag_from, burn,
                          lambda eng, lo, hi, n: _lib.check(eng.lib.ptmi_diag_update(eng.h, lo, hi, n)))
        # thinned snapshots of the cold chains, kept on the device (with_stages(samples=slots | dict(slots=, every=), samples_from=...); see the class docstring)
        self.samples_spec = self._splan = None
        if self._samples is not None:
            from .samples import SlotPlan, samples_spec
            self.samples_spec = samples_spec(self._samples)
            self._splan = SlotPlan(*self.samples_spec)
        self._ring_reader("samples", self.samples_spec is not None, self._samples_from, burn, PTEngine._samples_take)
        # the best-fit (MAP / ML) row of every cold chain over all iterations (with_stages(best=True, best_from=...); see the class docstring)
        self.best_on = bool(self._best)
        if self.best_on and not keep_lnl:
            raise ValueError("best=True compares the lnL and lp of every iteration: it needs keep_lnl=True (AMaux beside the ring's rows)")
        self._ring_reader("best", self.best_on, self._best_from, 0,       # from iteration 0 on, not burn: an optimum is one whenever it was visited
                          lambda eng, lo, hi, n: _lib.check(eng.lib.ptmi_best_update(eng.h, lo, hi)) if eng.owns_cold else None)
        # the ladder's summaries for the log-evidence (with_stages(evidence=True, evidence_from=..., evidence_every=...); see the class docstring)
        self.evidence_on = bool(self._ev)
        if self.evidence_on:
            if int(ntemps) < 2:
                raise ValueError("evidence=True needs a ladder: ntemps = %d is one temperature, there is nothing to integrate over" % int(ntemps))
            if int(tskip) <= 0:
                raise ValueError("evidence=True samples behind the swaps: tskip = %d proposes none" % int(tskip))
            if (ntemps_global is not None and int(ntemps_global) != int(ntemps)) or int(temp0) != 0:
                raise ValueError("evidence=True serves a whole ladder on one GPU: on a sharded ladder (ntemps_global / temp0) the engine would "
                                 "not know the gap to the neighbouring block (ptmi_ev_attach takes it as dbeta[0]; ShardedPTEngine has no such stage yet)")
            self.evidence_from = int(burn) if self._ev_from is None else int(self._ev_from)
            if self.evidence_from < 0:
                raise ValueError("evidence_from = %d: the first iteration sampled lies behind evidence_from >= 0" % self.evidence_from)
            every = self._ev_every
            if not isinstance(every, (int, np.integer)) or int(every) < 1:
                raise ValueError("evidence_every = %r: every k-th swap epoch is sampled, k >= 1" % (every,))
            self.evidence_every = int(every)
            self.ev_epochs = 0
        elif self._ev_from is not None or self._ev_every != 1:
            raise ValueError("evidence_from= and evidence_every= go with evidence=True")
        # the ladder adapted from every walker's swaps (with_stages(adapt_ladder=True | dict(...)); see the class docstring)
        self.adapt_on = self._adapt is not None and self._adapt is not False
        if self.adapt_on:
            ad = {} if self._adapt is True else self._adapt
            if not isinstance(ad, dict) or not set(ad) <= {"every", "kappa", "t0", "until"}:
                raise ValueError("adapt_ladder is True or a dict with keys among every, kappa, t0, until (got %r)" % (self._adapt,))
            every, kappa, t0, until = ad.get("every", 10), ad.get("kappa", 2.0), ad.get("t0", 10.0), ad.get("until")
            if int(ntemps) < 2:
                raise ValueError("adapt_ladder needs a ladder: ntemps = %d is one temperature, there is no gap to move" % int(ntemps))
            if (ntemps_global is not None and int(ntemps_global) != int(ntemps)) or int(temp0) != 0:
                raise ValueError("adapt_ladder serves a whole ladder on one GPU: on a sharded ladder (ntemps_global / temp0) the pairs' "
                                 "acceptance would need a reduction across blocks (ShardedPTEngine has no such stage)")
            if int(tskip) <= 0:
                raise ValueError("adapt_ladder reads the swaps' acceptance: tskip = %d proposes none" % int(tskip))
            if not isinstance(every, (int, np.integer)) or int(every) < 1:
                raise ValueError("adapt_ladder: every = %r swap epochs per window, an integer >= 1" % (every,))
            if swap_mode == "oddeven" and int(every) % 2:
                raise ValueError("adapt_ladder: every = %d with swap_mode='oddeven': a window needs as many even as odd swap epochs, "
                                 "an even number" % int(every))
            if not isinstance(kappa, (int, float, np.integer, np.floating)) or not np.isfinite(kappa) or not 0.0 <= float(kappa) <= 8.0:
                raise ValueError("adapt_ladder: kappa = %r, the gain of the first update, lies in [0, 8]" % (kappa,))
            if not isinstance(t0, (int, float, np.integer, np.floating)) or not np.isfinite(t0) or not float(t0) > 0.0:
                raise ValueError("adapt_ladder: t0 = %r, the updates after which the gain has halved, is finite and > 0" % (t0,))
            if until is None:
                until = int(burn)
            if not isinstance(until, (int, np.integer)) or int(until) < 0:
                raise ValueError("adapt_ladder: until = %r, the last iteration at which the ladder may move, an integer >= 0" % (until,))
            if self.evidence_on and int(until) > self.evidence_from:
                raise ValueError("adapt_ladder: until = %d lies behind evidence_from = %d: the evidence stage's sums are per temperature, "
                                 "the ladder must be frozen before the first sample" % (int(until), self.evidence_from))
            self.adapt_every, self.adapt_kappa, self.adapt_t0, self.adapt_until = int(every), float(kappa), float(t0), int(until)
            self.lad_calls, self.lad_epochs, self.lad_tries = 0, 0, [0, 0]
            self._lad_sweep = swap_mode != "oddeven"
            self._lad_hist = []                                       # per update: (iteration, kappa, the planes [3][n]: device, or host once asked for)
        # rows_logl: the built-in likelihood as a row kernel on the split path (see the class docstring); refused before anything is built
        self.rows_logl = bool(rows_logl)
        if self.rows_logl:
            if logl[0] not in ("iso", "dense"):
                raise ValueError("rows_logl=True serves logl=('iso',) and ('dense', mu, P) (ptmi_rows_logl), not %r" % (logl[0],))
            if int(w_host) > 0 and not self._jumps:
                raise ValueError("rows_logl=True cannot be combined with w_host > 0: host-served jumps need the caller's own callbacks")
            if (ntemps_global is not None and int(ntemps_global) != int(ntemps)) or int(temp0) != 0:
                raise ValueError("rows_logl=True cannot be combined with ntemps_global / temp0 (a sharded ladder): run_callback swaps the whole ladder on one GPU")
            split = True
            split_nuts = split_nuts or int(grad_weights[0]) > 0
            if am_mode == "auto":
                am_mode = "rows"                                      # the split path stores every rank-0 row: the statistics sum in the rows' order
        self.lib = _lib.load()
        if not torch.cuda.is_available() or _lib.device_count() < 1:
            raise _lib.PtmiError("no MI355X visible: the engine has no CPU fallback")
        self.d, self.nt, self.W = int(ndim), int(ntemps), int(nwalkers)
        self.ntg = self.nt if ntemps_global is None else int(ntemps_global)
        self.temp0, self.walker0 = int(temp0), int(walker0)
        self.ladder = np.ascontiguousarray(
            temperature_ladder(self.ntg, ndim, Tmin, Tmax) if ladder is None else ladder, dtype=np.float64)
        if len(self.ladder) != self.ntg:
            raise ValueError("ladder has %d entries for %d temperatures" % (len(self.ladder), self.ntg))
        self.temps_mh = self.ladder[self.temp0:self.temp0 + self.nt].copy()
        if hot_chain and self.temp0 + self.nt == self.ntg:
            self.temps_mh[-1] = 1e80                                  # PTMCMCSampler.py:281-282
        self.ladder0, self.temps_mh0 = self.ladder.copy(), self.temps_mh.copy()      # the constructor's ladder (adapt_ladder moves self.ladder)
        self.cov_update, self.burn, self.tskip, self.seed = int(cov_update), int(burn), int(tskip), int(seed)
        self.weights = tuple(int(w) for w in weights)
        self.per_walker = cov_mode == "per_walker"
        if cov_mode not in ("per_walker", "pooled"):
            raise ValueError("cov_mode must be 'per_walker' or 'pooled'")
        if pick_mode not in _lib.PICK_MODES:
            raise ValueError("pick_mode must be 'chain' or 'walker'")
        self.pick_mode = pick_mode
        if eig_mode not in ("lapack", "jacobi", "ql", "hipsolver", "sytrd"):
            raise ValueError("eig_mode must be 'lapack', 'jacobi', 'ql', 'hipsolver' or 'sytrd'")
        if eig_mode == "sytrd" and (cov_mode != "pooled" or not 3 <= int(ndim) <= 1024):
            raise ValueError("eig_mode='sytrd' factorizes one pooled covariance of 3 <= ndim <= 1024")
        self.eig_mode = eig_mode
        if int(eig_lag) < 0:
            raise ValueError("eig_lag must be >= 0 launches")
        # (where the late table is not implemented -- per-walker covariances unless eig_mode is "ql", parameter groups, the on-stream
        # device eigensolver "jacobi" -- the table is applied at once, as OracleEngine defines it too)
        if int(eig_lag) > 0 and eig_mode == "jacobi" and cov_mode == "pooled" and groups is None:
            raise ValueError("eig_lag > 0 is implemented for eig_mode 'lapack', 'hipsolver', 'sytrd' and 'ql' (got %r)" % (eig_mode,))
        lag_ok = groups is None and ((cov_mode == "pooled" and eig_mode in ("lapack", "hipsolver", "sytrd")) or eig_mode == "ql")
        self.eig_lag, self._eig_pending, self._eig_wait = (int(eig_lag) if lag_ok else 0), False, 0
        self.Wc = self.W if self.per_walker else 1
        # parameter groups (PTMCMCSampler.py:129-145): per-group eigenvectors, embedded in the full space
        self.groups = [np.arange(self.d)] if groups is None else [np.asarray(g, dtype=np.int64) for g in groups]
        self.ngr = len(self.groups)
        # "whole": one group that IS the full parameter vector in order (a permutation of it needs put_eig's embedding)
        self.whole = self.ngr == 1 and np.array_equal(self.groups[0], np.arange(self.d))
        if eig_mode in ("jacobi", "sytrd") and not self.whole:
            raise ValueError("eig_mode=%r factorizes the full covariance: no parameter groups (eig_mode='ql' and 'hipsolver' take them)" % eig_mode)
        if eig_mode == "ql" and not self.whole and any(len(np.unique(g)) != len(g) for g in self.groups):
            raise ValueError("eig_mode='ql' with parameter groups: a group may not repeat a parameter")
        self.gsize = np.ascontiguousarray([len(g) for g in self.groups], dtype=np.int32)
        self.gmask = np.zeros((self.ngr, self.d))
        for gi, g in enumerate(self.groups):
            if len(g) < 1 or g.min() < 0 or g.max() >= self.d:
                raise ValueError("group %d has indices outside [0, %d)" % (gi, self.d))
            self.gmask[gi, g] = 1.0
        # gradient jumps on the built-in likelihoods (PTMCMCSampler.py:225-258): (NUTSweight, HMCweight); the whitening
        # comes from the INITIAL covariance and is never adapted (nutsjump.py:45, 53-54)
        self.grad_weights = tuple(int(w) for w in grad_weights)
        if split_nuts and not split:
            raise ValueError("split_nuts=True is NUTS on the callback path: it needs split=True")
        if split and self.grad_weights[0] > 0 and not split_nuts:
            raise ValueError("the callback path (split=True) runs HMC with batched gradient callbacks, not NUTS: grad_weights=(0, w_hmc)")
        self.split_nuts = bool(split_nuts)
        has_gj = sum(self.grad_weights) > 0
        if int(ndim) > 512 and (has_gj or split_nuts):
            # beyond the fused gradient kernels (ndim <= 512): HMC alone, through the batched gradient stage of the callback path
            if int(ndim) > 2048:
                raise ValueError("gradient jumps (grad_weights) stop at ndim 2048 (got %d)" % int(ndim))
            if self.grad_weights[0] > 0 or split_nuts:
                raise ValueError("NUTS (grad_weights[0] > 0, split_nuts=True) is built for ndim <= 512 (got %d): beyond, up to 2048, "
                                 "the callback path runs HMC alone, grad_weights=(0, w_hmc)" % int(ndim))
            if not split:
                raise ValueError("gradient jumps in the fused kernels are built for ndim <= 512 (got %d): beyond, up to 2048, HMC runs "
                                 "on the callback path (split=True or rows_logl=True, grad_weights=(0, w_hmc))" % int(ndim))
            if logl[0] == "interval":
                raise ValueError("the interval likelihood is built for ndim <= 512 (got %d)" % int(ndim))
        self.gj_tab = np.zeros(0)
        if has_gj:
            import scipy.linalg as sl
            L = sl.cholesky(np.asarray(cov0, dtype=np.float64), lower=True)
            Li = sl.solve_triangular(L, np.eye(self.d), trans=0, lower=True)
            self.gj_tab = np.ascontiguousarray(np.stack([L, Li, L.T]))
        self.device = torch.device("cuda", device)
        self.dev_index = device
        d, nt, W, Wc = self.d, self.nt, self.W, self.Wc
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        z = lambda shape, dt=f64: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        has_de = self.weights[2] > 0 if use_de_buffer is None else use_de_buffer
        st, ep = C.c_int(0), C.c_int(0)                                # row format of the DE buffer (include/ptmi.h)
        gshape = has_gj or logl[0] == "interval"                       # the interval family lives in the gradient-jump shapes (include/ptmi.h)
        _lib.check(self.lib.ptmi_de_row_stride(d, int(gshape), C.byref(st), C.byref(ep)))
        self.de_ld, self.de_epl = st.value, ep.value
        _lib.check(self.lib.ptmi_am_row_format(d, int(gshape), C.byref(ep)))         # row format of the AM buffer (include/ptmi.h)
        self.am_epl = ep.value
        self.am_pos = self.am_inv = None
        if self.am_epl:
            e_, ln_ = np.arange(d) // 4, np.arange(d) % 4
            self.am_pos = np.where(e_ < 2 * (self.am_epl // 2), 8 * (e_ // 2) + 2 * ln_ + e_ % 2, 8 * (self.am_epl // 2) + ln_)   # where parameter i sits
            self.am_inv = np.argsort(self.am_pos)                                   # which parameter sits at position p
        self.owns_cold = self.temp0 == 0
        if am_mode not in ("auto", "rows", "rle"):
            raise ValueError("am_mode must be 'auto', 'rows' or 'rle'")
        rle_ok = not self.per_walker and self.owns_cold                  # = ptmi_am_flags_ok
        if am_mode == "rle" and not rle_ok:
            raise ValueError("am_mode='rle' serves the pooled covariance (cov_mode='pooled')")
        self.am_rle = rle_ok and am_mode != "rows"
        self.t = dict(
            X=z((W, nt, d)), lnL=z((W, nt)), lp=z((W, nt)),
            temp_of=torch.arange(nt, dtype=i32, device=self.device).repeat(W, 1).contiguous(),
            slot_of=torch.arange(nt, dtype=i32, device=self.device).repeat(W, 1).contiguous(),
            Ut=z((Wc, self.ngr, d, d)), S=z((Wc, self.ngr, d)),
            DE=z((Wc, self.burn, self.de_ld)) if has_de else None,
            AM=z((W, self.cov_update, d)) if self.owns_cold else None,
            nacc=z((W, nt), i64), jstat=z((W, nt, _lib.J_NTYPES, 2), i64), nswap=z((W, self.ntg), i64),
            mu=z((Wc, d)) if self.owns_cold else None, M2=z((Wc, d, d)) if self.owns_cold else None,   # pooled: ONE running (mu, M2)
            cov=z((Wc, d, d)),
            Q=z((W, nt, d)) if split else None, qaux=z((W, nt, 4)) if split else None,
            # the second proposal buffer and the chains' state locations (include/ptmi.h: accepted proposals stay where they are)
            Q2=z((W, nt, d)) if split else None, sloc=z((W, nt), i32) if split else None,
            AMaux=z((W, self.cov_update, 2)) if (keep_lnl and self.owns_cold) else None,
            gj=z((W, nt, _lib.GJ_NSTATE)) if has_gj else None,
            AMflag=z((W, self.cov_update), i64) if self.am_rle else None,     # AM row flags (include/ptmi.h): every row starts as KEY
        )
        if self.am_rle:
            self.t["AMflag"].fill_(_lib.AMROW_KEY)
        if has_gj:
            self.t["gj"][..., _lib.GJ_EPSBAR] = 1.0
        cov0 = np.asarray(cov0, dtype=np.float64)
        self.t["cov"].copy_(torch.from_numpy(np.broadcast_to(cov0, (Wc, d, d)).copy()))
        # likelihood / prior parameters
        self._par_l = np.zeros(0)
        self._par_p = np.zeros(0)
        if logl[0] == "dense":
            mu, P = np.asarray(logl[1], np.float64), np.asarray(logl[2], np.float64)
            self._par_l = np.concatenate([mu, np.ascontiguousarray(P.T).ravel()])
        if logl[0] == "interval":
            self._par_l = interval_par(logl[1], logl[2], d)
        if logp[0] == "box":
            self._par_p = np.concatenate([np.asarray(logp[1], np.float64), np.asarray(logp[2], np.float64)])
        self.stream = torch.cuda.current_stream(self.device)
        cfg = _lib.Config(
            ndim=d, ntemps=nt, nwalkers=W, ntemps_global=self.ntg, temp0=self.temp0, walker0=self.walker0,
            logl_kind=_lib.LOGL[logl[0]], logp_kind=_lib.LOGP[logp[0]], w_host=int(w_host), w_scam=self.weights[0], w_am=self.weights[1],
            w_de=self.weights[2] if has_de else 0, de_size=self.burn, cov_update=self.cov_update, tskip=self.tskip,
            cov_per_walker=int(self.per_walker), device=device, ngroups=self.ngr if self.ngr > 1 else 0,
            swap_mode=_lib.SWAP_MODES[swap_mode], pick_mode=_lib.PICK_MODES[pick_mode], seed=self.seed,
            w_nuts=self.grad_weights[0], w_hmc=self.grad_weights[1], gj_nburn=self.burn, hmc_eps=float(hmc[0]),
            hmc_min=int(hmc[1]), hmc_max=int(hmc[2]), nuts_maxdepth=int(nuts_maxdepth), nuts_delta=float(nuts_delta),
            gj_tab=self.gj_tab.ctypes.data_as(_lib._dp) if has_gj else None,
            group_size=self.gsize.ctypes.data_as(C.POINTER(C.c_int32)), group_mask=self.gmask.ctypes.data_as(_lib._dp),
            stream=C.c_void_p(self.stream.cuda_stream),
            ladder=self.ladder.ctypes.data_as(_lib._dp), temps_mh=self.temps_mh.ctypes.data_as(_lib._dp),
            logl_par=self._par_l.ctypes.data_as(_lib._dp) if len(self._par_l) else None, logl_par_len=len(self._par_l),
            logp_par=self._par_p.ctypes.data_as(_lib._dp) if len(self._par_p) else None, logp_par_len=len(self._par_p))
        buf = _lib.Buffers(**{k: (C.c_void_p(v.data_ptr()) if v is not None else None) for k, v in self.t.items()})
        self.h = C.c_void_p()
        _lib.check(self.lib.ptmi_create(C.byref(cfg), C.byref(buf), C.byref(self.h)))
        self._attach_callback_stages(w_host)
        if self.hist_spec is not None:
            # uint64 [d][nbins + 2] (bins, under, over) in parameter order; in self.t: checkpoints carry it by itself
            lo, hi, nbins = self.hist_spec
            self.t["hist"] = z((d, nbins + 2), i64)
            self._hist_scale = nbins / (hi - lo)
            _lib.check(self.lib.ptmi_hist_attach(self.h, C.c_void_p(self.t["hist"].data_ptr()), lo.ctypes.data_as(_lib._dp),
                                                 self._hist_scale.ctypes.data_as(_lib._dp), nbins))
        if self.pairs_spec is not None:
            # uint64 [npairs][nbins * nbins + 1] (the table row-major, then "outside"); in self.t: checkpoints carry it by itself
            pr, lo, hi, nbins = self.pairs_spec
            self.t["pairs"] = z((len(pr), nbins * nbins + 1), i64)
            self._pairs_scale = nbins / (hi - lo)
            _lib.check(self.lib.ptmi_pairs_attach(self.h, C.c_void_p(self.t["pairs"].data_ptr()), pr.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  len(pr), lo.ctypes.data_as(_lib._dp), self._pairs_scale.ctypes.data_as(_lib._dp), nbins))
        if self.evidence_on:
            # double [5][W][nt] (shift, s1, s2, m, es) and uint64 [2][W][nt] (taken, skipped), plane-major, by local rank; in self.t:
            # checkpoints carry them by themselves
            from .evidence import dbeta_of
            self.t["ev_acc"] = z((5, W, nt))
            self.t["ev_cnt"] = z((2, W, nt), i64)
            self.ev_dbeta = np.ascontiguousarray(dbeta_of(self.temps_mh))
            _lib.check(self.lib.ptmi_ev_attach(self.h, C.c_void_p(self.t["ev_acc"].data_ptr()), C.c_void_p(self.t["ev_cnt"].data_ptr()),
                                               self.ev_dbeta.ctypes.data_as(_lib._dp)))
        if self.adapt_on:
            # double [3][n] (log gaps, the last window's acceptance, the ladder) and uint64 [n] (accepted swaps already consumed); in
            # self.t: checkpoints carry them by themselves
            lad = np.zeros((3, self.ntg))
            lad[0, :-1] = np.log(self.ladder0[1:]) - np.log(self.ladder0[:-1])
            lad[2] = self.ladder0
            self.t["lad"] = torch.from_numpy(lad).to(self.device)
            self.t["lad_seen"] = z((self.ntg,), i64)
            _lib.check(self.lib.ptmi_ladder_attach(self.h, C.c_void_p(self.t["lad"].data_ptr()), C.c_void_p(self.t["lad_seen"].data_ptr())))
        if self.diag_on:
            # double [2 L + 3][W][d] (c, S1, S2, A, Q[0 .. L - 1], H[0 .. L - 2]), plane-major, in parameter order; in self.t: checkpoints
            # carry it by itself
            self.t["diag"] = z((2 * self.diag_levels + 3, W, d))
            _lib.check(self.lib.ptmi_diag_attach(self.h, C.c_void_p(self.t["diag"].data_ptr()), self.diag_levels, self.diag_batch))
        if self.samples_spec is not None:
            # double [slots][W][d] in parameter order and, with keep_lnl on the block that owns the cold ring, [slots][W][2] (lnL, lp);
            # in self.t: checkpoints carry them by themselves
            self.t["samples"] = z((self.samples_spec[0], W, d))
            self.t["samples_aux"] = z((self.samples_spec[0], W, 2)) if self.t["AMaux"] is not None else None
            _lib.check(self.lib.ptmi_samples_attach(self.h, C.c_void_p(self.t["samples"].data_ptr()),
                                                    C.c_void_p(self.t["samples_aux"].data_ptr()) if self.t["samples_aux"] is not None else None,
                                                    self.samples_spec[0]))
        if self.best_on:
            # double [2][W][d] (MAP, ML) in parameter order, double [2][W][3] (score, lnL, lp) and int64 [2][W] (the iteration, -1 =
            # nothing held); in self.t: checkpoints carry them by themselves.  A block that owns no cold ring attaches nothing and stays idle
            self.t["best"] = z((2, W, d))
            self.t["best_val"] = z((2, W, 3))
            self.t["best_iters"] = torch.full((2, W), -1, dtype=i64, device=self.device)
            if self.owns_cold:
                _lib.check(self.lib.ptmi_best_attach(self.h, C.c_void_p(self.t["best"].data_ptr()), C.c_void_p(self.t["best_val"].data_ptr()),
                                                     C.c_void_p(self.t["best_iters"].data_ptr()), 1.0 / float(self.temps_mh[0])))
        self.de_on = False
        self.de_head = 0
        self.iter = 0
        self.swap_proposed = 0
        self.eig_epochs = 0
        # a pending device factorization is finished BEHIND the statistics of the next covariance epoch (update_cov); the same on
        # every block of a sharded ladder (from the configuration alone: ShardedPTEngine orders its broadcasts by it)
        self.late_finish = self.eig_lag > 0 and eig_mode in ("hipsolver", "sytrd", "ql") and not stats_async
        self.stats_async = False
        if stats_async:
            # from the configuration alone, on EVERY block of a sharded ladder: a block without rank 0 has no statistics to run, but it
            # must refuse what the owner refuses -- else the owner raises alone and the others wait in their first collective for ever
            ok = (not self.per_walker and self.eig_lag >= 1 and self.whole and eig_mode in ("lapack", "hipsolver", "sytrd")
                  and (not has_de or self.burn % self.cov_update == 0))
            if not ok:
                raise ValueError("stats_async needs a pooled covariance, eig_lag >= 1, eig_mode 'lapack', 'hipsolver' or 'sytrd', one "
                                 "parameter group, and burn a multiple of cov_update when a DE history is kept")
        if stats_async and self.owns_cold:                            # (a block without rank 0 has no statistics to run)
            self.stats_async = True
            # the second ring (and its flags): what the statistics of the period before read while this period is written
            self._alt = dict(AM=torch.zeros_like(self.t["AM"]),
                             AMaux=torch.zeros_like(self.t["AMaux"]) if self.t["AMaux"] is not None else None,
                             AMflag=torch.full_like(self.t["AMflag"], _lib.AMROW_KEY) if self.t["AMflag"] is not None else None)
            # high priority: the statistics' blocks go ahead of the step kernel's next blocks wherever a CU has room for them
            self._st = torch.cuda.Stream(device=self.device, priority=int(os.environ.get("PTMI_STATS_PRIO", "-1")))     # (0 measured the same, round 5)
            self._ev_period, self._ev_stats = torch.cuda.Event(), torch.cuda.Event()
            self._stats_queued = False
        self._eig_host(0, cov0)                                       # every walker starts from the same covariance
        if Wc > 1:
            self.t["Ut"][1:] = self.t["Ut"][0]
            self.t["S"][1:] = self.t["S"][0]

    def __del__(self):
        try:
            if getattr(self, "_eig_pool", None) is not None:
                self._eig_pool.terminate()
                self._eig_pool = None
            if getattr(self, "h", None) is not None and self.h:
                self.lib.ptmi_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ data access
    def get(self, name):
        """Device array -> numpy (counters as uint64; DE rows in parameter order whatever their device format)."""
        if name == "AM":
            self.am_expand()
        if self.stats_async and name in ("cov", "mu", "M2"):
            self._st.synchronize()                                    # the statistics run beside the launches
        a = self.t[name].cpu().numpy()
        if self.stats_async and name in ("AM", "AMflag", "AMaux"):
            # ONE ring as a reader of the reference's buffer sees it: the rows of the current period come from the ring in use,
            # the older ones from the other ring
            lo, hi = self.am_period()
            cur = np.zeros(self.cov_update, dtype=bool)
            cur[np.arange(lo, hi + 1) % self.cov_update] = True
            b = self._alt[name].cpu().numpy()
            a = np.where(cur.reshape((1, -1) + (1,) * (a.ndim - 2)), a, b)
        if name == "DE" and self.de_epl:
            lane, slot = np.arange(self.d) % 4, np.arange(self.d) // 4
            pos = 8 * (slot // 2) + 2 * lane + slot % 2                # where parameter i sits in a row (ptmi_de_row_stride)
            return np.ascontiguousarray(a[..., pos])
        if name == "AM" and self.am_pos is not None:
            return np.ascontiguousarray(a[..., self.am_pos])              # parameter order whatever the device format
        return a.view(np.uint64) if name in ("nacc", "jstat", "nswap", "AMflag", "cjstat") else a

    def put(self, name, value):
        torch = _torch()
        if name == "AM":
            value = self.am_rows(np.asarray(value))                      # parameter order in, the buffer's row format on the device
            if self.am_rle:
                self.t["AMflag"].fill_(_lib.AMROW_KEY)                    # rows written from outside are KEY rows
        self.t[name].copy_(torch.from_numpy(np.ascontiguousarray(value)).to(self.t[name].dtype))

    def by_temp(self, name):
        """A per-slot array ([W][nt][...]) reordered by temperature rank."""
        a, so = self.get(name), self.get("slot_of").astype(np.int64)
        return np.take_along_axis(a, so.reshape(so.shape + (1,) * (a.ndim - 2)), 1)

    def sync(self):
        _lib.check(self.lib.ptmi_sync(self.h))
        if self.stats_async:
            self._st.synchronize()
        self._check_sytrd_info()

    def _check_sytrd_info(self):
        """eig_mode "sytrd": the divide-and-conquer solver's convergence word of the last factorization that has finished (it follows
        the result to pinned host memory on the factorization's stream: reading it never waits)."""
        if self.eig_mode == "sytrd":
            v = C.c_int32(0)
            _lib.check(self.lib.ptmi_eig_sytrd_info(self.h, C.byref(v)))
            if v.value != 0:
                raise _lib.PtmiError("ptmi_eig_sytrd: the tridiagonal eigensolver did not converge (info = %d); the eigenvectors of "
                                     "that covariance epoch are not valid" % v.value)

    # ------------------------------------------------------------------ set-up
    def _eig_host(self, w, cov):
        """U, S of the jump covariance by LAPACK (see factorize)."""
        for gi, g in enumerate(self.groups):                          # per group, :139-145 and :797-803
            U, S = factorize(cov if self.whole else cov[np.ix_(g, g)], self.per_walker)
            self.put_eig(U, S, w, gi)

    def _eig_host_pooled(self):
        """The pooled covariance's factorization on the host (factorize(), the same bits as _eig_host) with the GPU idle for as
        short as possible: the matrix comes down into pinned memory, the eigenvector rows and eigenvalues go up from pinned
        memory, one wait in all (the download's); the uploads are queued and the next launch behind them."""
        self._eig_begin()
        self._eig_end()

    def _eig_begin(self, stream=None):
        """First half of _eig_host_pooled: the covariance sets out for pinned host memory behind the statistics kernels (on `stream`:
        the engine's, or the side stream the statistics run on)."""
        torch = _torch()
        d = self.d
        stream = self.stream if stream is None else stream
        if getattr(self, "_pin", None) is None:
            self._pin = (torch.empty((d, d), dtype=torch.float64).pin_memory(), torch.empty((d, d), dtype=torch.float64).pin_memory(),
                         torch.empty(d, dtype=torch.float64).pin_memory(), torch.cuda.Event())
        cov_h, ut_h, s_h, ev = self._pin
        with torch.cuda.stream(stream):
            cov_h.copy_(self.t["cov"][0], non_blocking=True)
            ev.record(stream)
        self._eig_pending = True

    def _eig_end(self):
        """Second half: wait for the covariance (NOT for the stream: with eig_lag = 1 a launch is running meanwhile), factorize,
        queue the uploads; whatever is launched next reads the new table."""
        torch = _torch()
        cov_h, ut_h, s_h, ev = self._pin
        with torch.cuda.stream(self.stream):
            ev.synchronize()
            U, S = factorize(cov_h.numpy(), False)
            np.copyto(ut_h.numpy(), U.T)
            np.copyto(s_h.numpy(), S)
            self.t["Ut"][0, 0].copy_(ut_h, non_blocking=True)
            self.t["S"][0, 0].copy_(s_h, non_blocking=True)
        self._eig_pending = False
        self.eig_epochs += 1

    def _eig_begin_side(self):
        """eig_mode "hipsolver" with eig_lag > 0: the library's eigensolver on a SIDE stream, behind the statistics kernels and
        beside the launches that follow (its thousands of small kernels fill what the step kernel leaves free); the result waits in
        staging tensors until _eig_end_side."""
        torch = _torch()
        if getattr(self, "_side", None) is None:
            # stats_async: the factorization follows the statistics on THEIR stream (which waits for the period's last launch itself)
            self._side = self._st if self.stats_async else torch.cuda.Stream(device=self.device, priority=-1)      # its small kernels go ahead of the step kernel's next blocks (priority 0: 7.1e8 against 7.3e8 at config 4)
            self._side_go, self._side_done = torch.cuda.Event(), torch.cuda.Event()
            # the staging tensors start as the table in force: whatever goes wrong on the side, they never hold garbage
            self._ut_next, self._s_next = self.t["Ut"].clone(), self.t["S"].clone()
            self._cov_side = torch.empty_like(self.t["cov"])          # the covariance the factorization reads: the next epoch's statistics may overwrite t["cov"] meanwhile
        with torch.cuda.stream(self._st if self.stats_async else self.stream):
            self._cov_side.copy_(self.t["cov"])                       # behind the statistics, on their stream
        if not self.stats_async:
            self._side_go.record(self.stream)
            self._side.wait_event(self._side_go)
        self._side_err = None

        def work():
            # on a thread of its own: the library's driver waits on the host for its status word, which would keep this
            # thread from queueing the launches the factorization is meant to run beside.  The thread reports through
            # self._side_err (the library's last-error text is per thread: it is read HERE, not by the thread that joins)
            try:
                torch.cuda.set_device(self.device)
                with torch.cuda.stream(self._side):
                    if self.eig_mode == "sytrd":
                        _lib.check(self.lib.ptmi_eig_sytrd_from(self.h, C.c_void_p(self._side.cuda_stream), C.c_void_p(self._cov_side.data_ptr()),
                                                                C.c_void_p(self._ut_next.data_ptr()), C.c_void_p(self._s_next.data_ptr())))
                    elif self.eig_mode == "ql":               # every walker's matrix (or the pooled one): chains of rotations, little of the GPU each
                        _lib.check(self.lib.ptmi_eig_ql_from(self.h, C.c_void_p(self._side.cuda_stream), C.c_void_p(self._cov_side.data_ptr()),
                                                             C.c_void_p(self._ut_next.data_ptr()), C.c_void_p(self._s_next.data_ptr())))
                    else:
                        w, V = torch.linalg.eigh(self._cov_side)
                        w, order = w.abs().sort(dim=-1, descending=True, stable=True)
                        self._ut_next[:, 0].copy_(torch.gather(V, -1, order.unsqueeze(-2).expand_as(V)).transpose(-1, -2))
                        self._s_next[:, 0].copy_(w)
            except BaseException as e:              # noqa: B902 -- re-raised by the thread that joins (_eig_end_side)
                self._side_err = e
            finally:
                self._side_done.record(self._side)

        import threading
        self._side_thread = threading.Thread(target=work, daemon=True)
        self._side_thread.start()
        self._eig_pending = True

    def _eig_end_side(self):
        torch = _torch()
        self._side_thread.join()
        self._eig_pending = False
        if self._side_err is not None:                # the table in force stays; the run does not go on with a half-made one
            err, self._side_err = self._side_err, None
            raise _lib.PtmiError("the factorization on the side stream failed: %r" % (err,)) from err
        self.stream.wait_event(self._side_done)
        with torch.cuda.stream(self.stream):
            self.t["Ut"].copy_(self._ut_next)
            self.t["S"].copy_(self._s_next)
        self.eig_epochs += 1

    def _eig_finish(self):
        """The pending factorization of the last covariance epoch takes effect (eig_lag launches after it, or at the next epoch)."""
        if self._eig_pending:
            if self.eig_mode in ("hipsolver", "sytrd", "ql"):
                self._eig_end_side()
            else:
                self._eig_end()
        self._eig_wait = 0

    def _eig_hipsolver(self):
        """U, S of every covariance the engine holds by the ROCm library's symmetric eigensolver, on the stream (factorize()'s
        pooled rule: eigenvalues by decreasing size and in absolute value, eigenvectors as the rows of Ut)."""
        torch = _torch()
        with torch.cuda.stream(self.stream):
            if not self.whole:
                # parameter groups (PTMCMCSampler.py:139-145, 797-803: one factorization per group's block of the covariance), any ndim:
                # the block gathered on the device, the vectors embedded in the full space, one per row of the group's table
                cov = self.t["cov"]
                self.t["Ut"].zero_()
                self.t["S"].zero_()
                for gi, g in enumerate(self.groups):
                    idx = torch.as_tensor(g, device=self.device)
                    m = len(g)
                    w, V = torch.linalg.eigh(cov[:, idx][:, :, idx])                           # [Wc][m], [Wc][m][m]
                    w, order = w.abs().sort(dim=-1, descending=True, stable=True)
                    Vt = torch.gather(V, -1, order.unsqueeze(-2).expand_as(V)).transpose(-1, -2)    # rows = eigenvectors
                    rows = self.t["Ut"][:, gi, :m]                                             # [Wc][m][d] (a view)
                    rows[:, :, idx] = Vt
                    self.t["S"][:, gi, :m] = w
                return
            w, V = torch.linalg.eigh(self.t["cov"])                  # [Wc][d], [Wc][d][d] (columns)
            # by decreasing |eigenvalue| (a covariance's are >= 0 up to rounding: a slightly negative one must not jump the queue)
            w, order = w.abs().sort(dim=-1, descending=True, stable=True)
            self.t["Ut"][:, 0].copy_(torch.gather(V, -1, order.unsqueeze(-2).expand_as(V)).transpose(-1, -2))
            self.t["S"][:, 0].copy_(w)

    def _eig_host_all(self, cov):
        """Per-walker mode: the W independent factorizations, one upload for all.  From 64 walkers on they run on a
        pool of spawned host processes (numpy only; every LAPACK call single-threaded, so each walker's bits are those
        of a lone reference run); PTMI_EIG_WORKERS sets the pool size (0 = in this process)."""
        import os
        from . import _eigworker
        torch = _torch()
        groups = None if self.whole else self.groups
        nwork = int(os.environ.get("PTMI_EIG_WORKERS", min(64, _usable_cores())))
        if self.Wc < 64 or nwork <= 1:
            Ut, Sv = _eigworker.svd_chunk((cov, groups))
        else:
            if getattr(self, "_eig_pool", None) is None:
                import multiprocessing as mp
                self._eig_pool = mp.get_context("spawn").Pool(nwork)       # spawn: no fork of a process that holds HIP state
            bounds = np.linspace(0, self.Wc, min(self.Wc, 4 * nwork) + 1).astype(int)
            parts = self._eig_pool.map(_eigworker.svd_chunk, [(cov[a:b], groups) for a, b in zip(bounds[:-1], bounds[1:]) if b > a])
            Ut, Sv = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        self.t["Ut"].copy_(torch.from_numpy(Ut))
        self.t["S"].copy_(torch.from_numpy(Sv))

    def put_eig(self, U, S, w=0, gi=0):
        """Upload a group's eigenvectors (columns of U) embedded in the full space, one per row."""
        torch = _torch()
        g = self.groups[gi]
        Ut = np.zeros((self.d, self.d))
        Sv = np.zeros(self.d)
        Ut[np.ix_(np.arange(len(g)), g)] = np.asarray(U).T
        Sv[:len(g)] = S
        self.t["Ut"][w, gi].copy_(torch.from_numpy(Ut))
        self.t["S"][w, gi].copy_(torch.from_numpy(Sv))

    def init_state(self, p0, i0=0):
        """Point(s) the chains hold at iteration ``i0``: ``p0`` of shape [d] (broadcast) or [W][nt][d] (by slot)."""
        torch = _torch()
        p0 = np.asarray(p0, dtype=np.float64)
        full = np.array(p0 if p0.ndim == 3 else np.broadcast_to(p0, (self.W, self.nt, self.d)))
        self.t["X"].copy_(torch.from_numpy(full))
        if self.t.get("sloc") is not None:
            self.t["sloc"].zero_()                                    # every state is in X (a segment of the split path abandoned half way left it otherwise)
        if self.rows_logl:
            return self.init_state_callback(full, *self._rows_callbacks()[:2], i0=i0)
        _lib.check(self.lib.ptmi_eval_state(self.h))                 # :479-487
        self._store_initial(i0)
        self.iter = int(i0)

    def am_rows(self, rows):
        """Rows in parameter order (last axis) -> the AM buffer's row format (a torch tensor or a numpy array)."""
        if self.am_inv is None:
            return rows
        if isinstance(rows, np.ndarray):
            return rows[..., self.am_inv]
        return rows[..., _torch().from_numpy(self.am_inv).to(rows.device)]

    def am_params(self, rows):
        """Rows of the AM buffer (last axis in its row format) -> parameter order."""
        if self.am_pos is None:
            return rows
        if isinstance(rows, np.ndarray):
            return rows[..., self.am_pos]
        return rows[..., _torch().from_numpy(self.am_pos).to(rows.device)]

    def am_expand(self, w0=0, nw=None, it_lo=None, it_hi=None):
        """Every row of the AM ring, in place (``ptmi_am_expand``): the rows of rejected steps, which ``am_mode="rle"`` does not
        store, are copied forward from the row before them, for iterations ``it_lo .. it_hi`` of walkers ``w0 .. w0 + nw - 1``;
        default: the current covariance period up to the current iteration (``am_period``) -- once the ring wraps, the repeats of
        an older period have lost the row they hang on.  A no-op with ``am_mode="rows"``."""
        if not self.am_rle:
            return
        it_hi = self.iter if it_hi is None else int(it_hi)
        it_lo = self.am_period(it_hi)[0] if it_lo is None else int(it_lo)
        _lib.check(self.lib.ptmi_am_expand(self.h, int(w0), self.W - int(w0) if nw is None else int(nw), it_lo, it_hi))

    def am_period(self, it=None):
        """(first, last) iteration of the covariance period the ring holds at iteration ``it``: [E, it], E = the last multiple of
        covUpdate below ``it`` (row 0 of the ring, until iteration E + covUpdate overwrites it)."""
        it = self.iter if it is None else int(it)
        E = ((it - 1) // self.cov_update) * self.cov_update if it > 0 else 0
        return E + (1 if it - E >= self.cov_update else 0), it

    def _store_initial(self, i0=0):
        """updateChains(p0, lnlike0, lnprob0, i0), :491: row i0 % covUpdate of the AM ring holds the point."""
        torch = _torch()
        if self.owns_cold:
            ar = torch.arange(self.W, device=self.device)
            idx = self.t["slot_of"][:, 0].long()
            row = int(i0) % self.cov_update
            self.t["AM"][:, row, :] = self.am_rows(self.t["X"][ar, idx])
            if self.am_rle:
                self.t["AMflag"][:, row] = _lib.AMROW_KEY
            if self.t["AMaux"] is not None:
                self.t["AMaux"][:, row, 0] = self.t["lnL"][ar, idx]
                self.t["AMaux"][:, row, 1] = self.t["lp"][ar, idx]

    # ------------------------------------------------------------------ epochs
    def update_cov(self, it_done):
        """Covariance epoch after iteration ``it_done`` (:545-560): device Welford, host SVD."""
        if not self.owns_cold:
            return
        for r in self._ring:
            r.advance(self, it_done)                                  # before the statistics, and before stats_async switches rings
        # A factorization still pending from the epoch before (eig_lag >= the launches of a period) is finished here at the latest.
        # On the side stream (device factorizations) it goes on BESIDE this epoch's statistics, which do not read the table: they are
        # queued first, the wait for the old table comes behind them -- the same table in force for the same launches either way.
        late = self._eig_pending and self.late_finish
        if not late:
            self._eig_finish()
        self._check_sytrd_info()                                      # how the last finished factorization went
        if self.stats_async:
            self._update_cov_async(it_done)
            return
        _lib.check(self.lib.ptmi_update_cov(self.h, it_done))
        if late:
            self._eig_finish()
        if self.am_rle and self.t["DE"] is not None and self.burn % self.cov_update != 0:
            # a DE epoch (every `burn` iterations, :563-571) copies ALL covUpdate ring rows; unless burn is a multiple of covUpdate
            # some of them belong to the period that ends here, and am_expand only reaches back to the current period's start:
            # copy that period's repeats forward now, before the ring wraps (the statistics above have taken the run lengths)
            self.am_expand(it_lo=self.am_period(it_done)[0], it_hi=it_done)
        if self.eig_mode == "ql" and self.eig_lag:
            self._eig_begin_side()                                    # beside the launches that follow; run() puts it into force
            self._eig_wait = self.eig_lag
            return
        if self.eig_mode in ("jacobi", "ql"):                         # stays on the stream: no host synchronisation
            _lib.check(self.lib.ptmi_eig_jacobi(self.h) if self.eig_mode == "jacobi" else self.lib.ptmi_eig_ql(self.h))
            self.eig_epochs += 1
            return
        if self.eig_mode in ("hipsolver", "sytrd"):
            if self.eig_lag and not self.per_walker:
                self._eig_begin_side()                                # run() puts it into force eig_lag launches later
                self._eig_wait = self.eig_lag
                return
            if self.eig_mode == "sytrd":
                _lib.check(self.lib.ptmi_eig_sytrd(self.h, None, None, None))      # on the engine's stream, into Ut / S
            else:
                self._eig_hipsolver()
            self.eig_epochs += 1
            return
        if self.Wc == 1 and not self.per_walker and self.whole:
            if self.eig_lag:
                self._eig_begin()                                     # run() finishes it behind the eig_lag-th launch from here
                self._eig_wait = self.eig_lag
            else:
                self._eig_host_pooled()
            return
        elif self.Wc == 1:
            self._eig_host(0, self.get("cov")[0])
        else:
            self._eig_host_all(self.get("cov"))
        self.eig_epochs += 1

    def _update_cov_async(self, it_done):
        """The covariance epoch with the statistics BESIDE the launches that follow (stats_async): the period that ends here stays in
        its ring, the launches from here on write the other one, the side stream takes the statistics and the factorization."""
        torch = _torch()
        old = {k: self.t[k] for k in ("AM", "AMaux", "AMflag")}
        with torch.cuda.stream(self.stream):
            if self._stats_queued:
                self.stream.wait_event(self._ev_stats)                # the other ring is free once the statistics that read it are done (a period ago)
            # ring row 0 holds the period's last iteration: every reader of the next period starts from it (am_expand's walk back,
            # am_period); it moves along with its flag
            for k, v in old.items():
                if v is not None:
                    self._alt[k][:, 0] = v[:, 0]
            self._ev_period.record(self.stream)
        for k, v in old.items():
            self.t[k], self._alt[k] = self._alt[k], v
        ptr = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None      # noqa: E731
        _lib.check(self.lib.ptmi_set_am_buffers(self.h, ptr(self.t["AM"]), ptr(self.t["AMaux"]), ptr(self.t["AMflag"])))
        self._st.wait_event(self._ev_period)
        _lib.check(self.lib.ptmi_update_cov_on(self.h, it_done, C.c_void_p(self._st.cuda_stream), ptr(old["AM"]), ptr(old["AMflag"])))
        self._ev_stats.record(self._st)
        self._stats_queued = True
        if self.eig_mode in ("hipsolver", "sytrd"):
            self._eig_begin_side()
        else:
            self._eig_begin(self._st)
        self._eig_wait = self.eig_lag

    # ------------------------------------------------------------------ the ring's second readers (_RingReader)
    def _ring_reader(self, name, on, first, burn, update):
        """The reader of the stage ``name`` that is ``on`` joins ``_ring``, from iteration ``first`` (``<name>_from``; default ``burn``)."""
        _, hint, verb, _ = _RingReader.WORDS[name]
        if not on:
            if first is not None:
                raise ValueError("%s_from= goes with %s" % (name, hint))
            return
        first = int(burn) if first is None else int(first)
        if first < 0:
            raise ValueError("%s_from = %d: the first iteration %s is %s_from + 1 >= 1" % (name, first, verb, name))
        self._ring.append(_RingReader(name, first, update))

    def _reader(self, name):
        return next((r for r in self._ring if r.name == name), None)

    def _ring_sync(self, name, it):
        if self._reader(name) is None:
            raise ValueError("no %s: PTEngine.with_stages(..., %s)" % _RingReader.WORDS[name][:2])
        self._reader(name).sync(self, it)

    hist_from, hist_iter = _ring_attr("hist", "first"), _ring_attr("hist", "iter")
    pairs_from, pairs_iter = _ring_attr("pairs", "first"), _ring_attr("pairs", "iter")
    diag_from, diag_iter = _ring_attr("diag", "first"), _ring_attr("diag", "iter")
    samples_from, samples_iter = _ring_attr("samples", "first"), _ring_attr("samples", "iter")
    best_from, best_iter = _ring_attr("best", "first"), _ring_attr("best", "iter")

    # ------------------------------------------------------------------ posterior histograms
    def hist_sync(self, it):
        """Count iterations ``(hist_iter, it]`` of every walker's cold chain into ``t["hist"]`` (``ptmi_hist_update``: asynchronous, the
        ring is only read).  ``it`` lies in the covariance period the ring holds; ``update_cov`` calls this at every period's end, so
        a caller only needs it for counts up to an iteration inside a period.  Nothing to do up to ``hist_from``."""
        self._ring_sync("hist", it)

    def hist_counts(self, it=None):
        """The histograms up to iteration ``it`` (default: the current one): a dict of ``counts`` uint64 [d][nbins], ``under`` / ``over``
        [d] (below ``lo`` and NaN / at or above ``hi``), ``edges`` [d][nbins + 1], ``first_iter`` / ``last_iter`` (the iterations counted,
        of every one of ``nwalkers`` cold chains)."""
        self.hist_sync(self.iter if it is None else it)
        lo, hi, nbins = self.hist_spec
        a = self.t["hist"].cpu().numpy().view(np.uint64)
        return dict(counts=np.ascontiguousarray(a[:, :nbins]), under=a[:, nbins].copy(), over=a[:, nbins + 1].copy(),
                    edges=hist_edges(lo, hi, nbins), first_iter=np.int64(self.hist_from + 1), last_iter=np.int64(self.hist_iter),
                    nwalkers=np.int64(self.W))

    # ------------------------------------------------------------------ pair histograms
    def pairs_sync(self, it):
        """Count iterations ``(pairs_iter, it]`` of every walker's cold chain into ``t["pairs"]`` (``ptmi_pairs_update``: asynchronous,
        the ring is only read).  ``it`` lies in the covariance period the ring holds; ``update_cov`` calls this at every period's end,
        so a caller only needs it for counts up to an iteration inside a period.  Nothing to do up to ``pairs_from``."""
        self._ring_sync("pairs", it)

    def pairs_counts(self, it=None):
        """The pair histograms up to iteration ``it`` (default: the current one): a dict of ``counts`` uint64 [npairs][nbins][nbins]
        (``counts[p][a][b]``: parameter ``pairs[p][0]`` in bin ``a``, ``pairs[p][1]`` in bin ``b``), ``outside`` [npairs] (either coordinate
        NaN, below ``lo`` or at or above ``hi``), ``pairs`` [npairs][2], ``edges`` [ndim][nbins + 1], ``first_iter`` / ``last_iter`` (the
        iterations counted, of every one of ``nwalkers`` cold chains)."""
        self.pairs_sync(self.iter if it is None else it)
        pr, lo, hi, nbins = self.pairs_spec
        a = self.t["pairs"].cpu().numpy().view(np.uint64)
        return dict(counts=np.ascontiguousarray(a[:, :nbins * nbins]).reshape(len(pr), nbins, nbins), outside=a[:, nbins * nbins].copy(),
                    pairs=pr.copy(), edges=hist_edges(lo, hi, nbins), first_iter=np.int64(self.pairs_from + 1),
                    last_iter=np.int64(self.pairs_iter), nwalkers=np.int64(self.W))

    # ------------------------------------------------------------------ convergence diagnostics
    def diag_sync(self, it):
        """Fold iterations ``(diag_iter, it]`` of every walker's cold chain into ``t["diag"]`` (``ptmi_diag_update``: asynchronous, the ring
        is only read).  ``it`` lies in the covariance period the ring holds; ``update_cov`` calls this at every period's end, so a
        caller only needs it for sums up to an iteration inside a period.  Nothing to do up to ``diag_from``."""
        self._ring_sync("diag", it)

    def diag_moments(self, it=None):
        """The streaming sums up to iteration ``it`` (default: the current one): a dict of the planes ``c``, ``S1``, ``S2``, ``A`` [W][d],
        ``Q`` [levels][W][d], ``H`` [levels - 1][W][d] (parameter order; include/ptmi.h ``ptmi_diag_attach``), ``n`` (samples per stream),
        ``k = n // batch0``, ``batch0``, ``levels``, ``first_iter`` / ``last_iter`` (the iterations folded, of every one of ``nwalkers``
        cold chains)."""
        from .diagnostics import planes
        self.diag_sync(self.iter if it is None else it)
        out = {k: np.ascontiguousarray(v) for k, v in planes(self.t["diag"].cpu().numpy(), self.diag_levels).items()}
        n = self.diag_iter - self.diag_from
        out.update(n=np.int64(n), k=np.int64(n // self.diag_batch), batch0=np.int64(self.diag_batch), levels=np.int64(self.diag_levels),
                   first_iter=np.int64(self.diag_from + 1), last_iter=np.int64(self.diag_iter), nwalkers=np.int64(self.W))
        return out

    def diagnostics(self, it=None):
        """R-hat, the autocorrelation times and the effective sample size of every parameter from ALL cold chains up to iteration ``it``
        (default: the current one): ``diagnostics.estimates(diag_moments(it))`` with ``first_iter`` / ``last_iter``."""
        from .diagnostics import estimates
        mom = self.diag_moments(it)
        out = estimates(mom)
        out.update(first_iter=mom["first_iter"], last_iter=mom["last_iter"])
        return out

    # ------------------------------------------------------------------ thinned samples
    def _samples_take(self, lo, hi, n_done):
        """The samples reader's update: the plan's snapshots among iterations ``lo .. hi`` in one ``ptmi_samples_take``."""
        if not self.owns_cold:
            return                                                    # no cold ring: idle, and the plan holds nothing
        plan = self._splan
        before = (plan.level, plan.slot_iter.copy())
        pairs = plan.take(self.samples_from, lo, hi)
        if pairs:
            it = np.ascontiguousarray([i for i, _ in pairs], dtype=np.int64)
            sl = np.ascontiguousarray([s for _, s in pairs], dtype=np.int32)
            try:
                _lib.check(self.lib.ptmi_samples_take(self.h, it.ctypes.data_as(C.POINTER(C.c_int64)), sl.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs)))
            except Exception:
                plan.level, plan.slot_iter[:] = before                # nothing was gathered: the plan stays where the reader's iteration is
                raise

    def samples_sync(self, it):
        """Take the plan's snapshots among iterations ``(samples_iter, it]`` of every walker's cold chain into ``t["samples"]``
        (``ptmi_samples_take``: asynchronous, the ring is only read).  ``it`` lies in the covariance period the ring holds; ``update_cov``
        calls this at every period's end, so a caller only needs it for snapshots up to an iteration inside a period.  Nothing to do up
        to ``samples_from``."""
        self._ring_sync("samples", it)

    def samples_device(self, it=None):
        """The held snapshots up to iteration ``it`` (default: the current one) as device tensors, no copy to the host: ``(x [n][W][d],
        aux [n][W][2] (lnL, lp) or None, iters int64 [n] (host))``, by ascending iteration.  The tensors are gathered from ``t["samples"]``
        on the engine's stream; a later ``run`` does not change them."""
        torch = _torch()
        self.samples_sync(self.iter if it is None else it)
        iters, slots = self._splan.held()
        with torch.cuda.stream(self.stream):
            idx = torch.from_numpy(slots).to(self.device)
            aux = self.t["samples_aux"]
            return self.t["samples"][idx], (aux[idx] if aux is not None else None), iters

    def samples(self, it=None):
        """The held snapshots up to iteration ``it`` (default: the current one), by ascending iteration: a dict of ``x`` [n][W][d]
        (parameter order), ``iters`` [n], ``every``, ``stride`` (= ``every << level``: the iterations between two snapshots), ``first_iter`` /
        ``last_iter`` (the iterations the snapshots are spread over), ``nwalkers``, and, with ``keep_lnl=True``, ``lnlike`` [n][W] and
        ``lnprob`` [n][W] = ``lnlike / temps_mh[0] + lp`` (computed as the sampler's chain files compute it: ``(1 / temps_mh[0]) * lnlike + lp``)."""
        x, aux, iters = self.samples_device(it)
        out = dict(x=x.cpu().numpy(), iters=iters.copy(), every=np.int64(self._splan.every), stride=np.int64(self._splan.stride),
                   first_iter=np.int64(self.samples_from + 1), last_iter=np.int64(self.samples_iter), nwalkers=np.int64(self.W))
        if aux is not None:
            a = aux.cpu().numpy()
            out["lnlike"] = np.ascontiguousarray(a[..., 0])
            out["lnprob"] = (1.0 / self.temps_mh[0]) * a[..., 0] + a[..., 1]
        return out

    # ------------------------------------------------------------------ best-fit rows
    def best_sync(self, it):
        """Compare iterations ``(best_iter, it]`` of every walker's cold chain with the held MAP and ML rows in ``t["best"]``
        (``ptmi_best_update``: asynchronous, the ring is only read).  ``it`` lies in the covariance period the ring holds; ``update_cov``
        calls this at every period's end, so a caller only needs it for the best row up to an iteration inside a period.  Nothing to
        do up to ``best_from``."""
        self._ring_sync("best", it)

    def best_device(self, it=None):
        """The held rows up to iteration ``it`` (default: the current one) as the device tensors themselves, no copy to the host:
        ``(rows [2][W][d] (MAP, ML; parameter order), val [2][W][3] (score, lnL, lp), iters int64 [2][W] (-1: nothing held))``.  They
        are ``t["best"]``, ``t["best_val"]`` and ``t["best_iters"]``: a later ``run`` goes on updating them on the engine's stream."""
        self.best_sync(self.iter if it is None else it)
        return self.t["best"], self.t["best_val"], self.t["best_iters"]

    def best(self, it=None, per_walker=False):
        """The best-fit point of ALL cold chains up to iteration ``it`` (default: the current one): a dict of ``x_map`` [d], ``lnprob_map``,
        ``lnlike_map``, ``lp_map``, ``iter_map``, ``walker_map`` (the row with the largest ``lnprob = (1 / temps_mh[0]) * lnlike + lp``, the
        chain files' column) and ``x_ml`` [d], ``lnlike_ml``, ``lp_ml``, ``lnprob_ml``, ``iter_ml``, ``walker_ml`` (the row with the largest
        ``lnlike``), ``first_iter`` / ``last_iter`` (the iterations compared), ``nwalkers``.  Iteration 0, the starting point, is not in
        the ring and is not a candidate.  Among the walkers the rule is the device's over ascending walker index (``best_pick``): held,
        strict ``>``, the lowest index on ties.  Only ``val`` and ``iters`` and the ONE winning row per plane are read back; with
        ``per_walker=True`` also ``x`` [2][W][d], ``val`` [2][W][3] and ``iters`` [2][W] of every walker.  Where nothing is held yet
        ``iter_*`` and ``walker_*`` are -1 and the values NaN."""
        rows, val, iters = self.best_device(it)
        val, iters = val.cpu().numpy(), iters.cpu().numpy()
        d = rows.shape[-1]
        wm, wl = best_pick(val[0, :, 0], iters[0]), best_pick(val[1, :, 0], iters[1])
        nan = np.float64(np.nan)
        out = {}
        for p, w, tag in ((0, wm, "map"), (1, wl, "ml")):
            s, lnl, lp = (val[p, w] if w >= 0 else (nan, nan, nan))
            out["x_" + tag] = rows[p, w].cpu().numpy() if w >= 0 else np.full(d, np.nan)
            out["lnlike_" + tag], out["lp_" + tag] = np.float64(lnl), np.float64(lp)
            # plane 0's score IS lnprob; for the ML row it is computed as the chain files compute it
            with np.errstate(invalid="ignore"):
                out["lnprob_" + tag] = np.float64(s) if p == 0 else np.float64((1.0 / self.temps_mh[0]) * lnl + lp)
            out["iter_" + tag], out["walker_" + tag] = np.int64(iters[p, w] if w >= 0 else -1), np.int64(w)
        out.update(first_iter=np.int64(self.best_from + 1), last_iter=np.int64(self.best_iter), nwalkers=np.int64(self.W))
        if per_walker:
            out.update(x=rows.cpu().numpy(), val=val, iters=iters)
        return out

    def update_de(self, it_done=None):
        if self.owns_cold and self.t["DE"] is not None:
            if it_done is not None:
                self.am_expand(it_hi=it_done)                          # the DE history takes every row of the ring (a no-op with stored rows)
            _lib.check(self.lib.ptmi_update_de(self.h))
            self.de_head = (self.de_head + min(self.cov_update, self.burn)) % self.burn

    def set_de_active(self, on=True):
        _lib.check(self.lib.ptmi_set_de_active(self.h, int(on)))
        self.de_on = bool(on)

    def set_de_head(self, head):
        _lib.check(self.lib.ptmi_set_de_head(self.h, int(head)))
        self.de_head = int(head)

    # ------------------------------------------------------------------ checkpoint
    def checkpoint(self):
        """Everything needed to continue bit-identically: device arrays, ring head, DE flag, iteration.
        (The RNG is counter based: its whole state is the iteration number.)"""
        self.sync()
        st = {"t_" + k: v.cpu().numpy() for k, v in self.t.items() if v is not None and k not in ("Q", "qaux", "Q2", "sloc")}
        st.update(iter=self.iter, de_on=int(self.de_on), de_head=self.de_head, swap_proposed=self.swap_proposed,
                  eig_epochs=self.eig_epochs,
                  # eig_lag: an epoch's table that is not in force yet (its covariance is in t_cov; restore() factorizes it again)
                  eig_pending=int(self._eig_pending), eig_wait=int(self._eig_wait))
        st.update({r.name + "_iter": r.iter for r in self._ring})
        if self._splan is not None:
            st.update(samples_level=self._splan.level, samples_slot_iter=self._splan.slot_iter.copy(), samples_every=self._splan.every,
                      samples_from=self.samples_from)
        if self.best_on:
            st["best_from"] = self.best_from
        if self.evidence_on:
            st["ev_epochs"] = self.ev_epochs
        if self.adapt_on:
            hist = self.ladder_history()
            st.update(lad_calls=self.lad_calls, lad_epochs=self.lad_epochs, lad_tries=np.asarray(self.lad_tries, dtype=np.int64),
                      lad_hist_iter=hist["iter"], lad_hist_kappa=hist["kappa"], lad_hist_planes=self._lad_planes())
        if self.stats_async:
            st.update({"alt_" + k: v.cpu().numpy() for k, v in self._alt.items() if v is not None})
        return st

    def restore(self, st):
        torch = _torch()
        for r in self._ring:                                          # refused before anything is touched; the histogram's shape is not looked at
            if (r.name + "_iter" not in st or "t_" + r.name not in st
                    or r.name != "hist" and tuple(np.shape(st["t_" + r.name])) != tuple(self.t[r.name].shape)):
                raise ValueError(_RingReader.WORDS[r.name][3])
        if self._splan is not None and (any(k not in st for k in ("samples_level", "samples_slot_iter", "samples_every", "samples_from"))
                                        or np.shape(st["samples_slot_iter"]) != (self._splan.nslots,)
                                        or int(st["samples_every"]) != self._splan.every or int(st["samples_from"]) != self.samples_from
                                        or (self.t["samples_aux"] is not None) != ("t_samples_aux" in st)):
            raise ValueError(_RingReader.WORDS["samples"][3])
        if self.best_on and (any(k not in st for k in ("best_from", "t_best_val", "t_best_iters")) or int(st["best_from"]) != self.best_from
                             or tuple(np.shape(st["t_best_val"])) != tuple(self.t["best_val"].shape)
                             or tuple(np.shape(st["t_best_iters"])) != tuple(self.t["best_iters"].shape)):
            raise ValueError(_RingReader.WORDS["best"][3])
        if self.evidence_on and any(k not in st for k in ("ev_epochs", "t_ev_acc", "t_ev_cnt")):
            raise ValueError("the checkpoint carries no evidence accumulators: it was written by a run without evidence=True")
        if self.adapt_on and any(k not in st for k in ("t_lad", "t_lad_seen", "lad_calls", "lad_epochs", "lad_tries", "lad_hist_iter",
                                                       "lad_hist_kappa", "lad_hist_planes")):
            raise ValueError("the checkpoint carries no ladder state: it was written by a run without adapt_ladder")
        # whatever this engine has under way is void -- and is brought to an end FIRST: a factorization on the side stream (its thread
        # joined, its result dropped), statistics still running beside the launches (stats_async: they write cov / mu / M2)
        if self._eig_pending:
            try:
                self._eig_finish()
            except _lib.PtmiError:
                pass
        if self.stats_async:
            self._st.synchronize()
            self._stats_queued = False
        for k, v in self.t.items():
            if v is not None and "t_" + k in st:
                v.copy_(torch.from_numpy(np.ascontiguousarray(st["t_" + k])).to(v.dtype))
            elif v is not None and k == "cjstat":
                v.zero_()                                             # a checkpoint from before the counters existed
        if self.t.get("sloc") is not None:
            self.t["sloc"].zero_()                                    # every restored state is in X (a segment abandoned half way -- a callback that raised -- left it otherwise)
        if self.stats_async:                                          # the ring of the period before (readers of older rows: get("AM"))
            for k, v in self._alt.items():
                if v is not None and "alt_" + k in st:
                    v.copy_(torch.from_numpy(np.ascontiguousarray(st["alt_" + k])).to(v.dtype))
        self.iter, self.swap_proposed = int(st["iter"]), int(st["swap_proposed"])
        self.eig_epochs = int(st["eig_epochs"])                       # (behind _eig_finish, which counts the dropped table)
        for r in self._ring:
            r.iter = int(st[r.name + "_iter"])
        if self._splan is not None:
            self._splan.level = int(st["samples_level"])
            self._splan.slot_iter[:] = np.asarray(st["samples_slot_iter"], dtype=np.int64)
        if self.evidence_on:
            self.ev_epochs = int(st["ev_epochs"])
        if self.adapt_on:
            self.lad_calls, self.lad_epochs = int(st["lad_calls"]), int(st["lad_epochs"])
            self.lad_tries = [int(v) for v in st["lad_tries"]]
            planes = np.asarray(st["lad_hist_planes"], dtype=np.float64).reshape(-1, 3, self.ntg)
            self._lad_hist = [(int(i), float(k), p.copy()) for i, k, p in zip(st["lad_hist_iter"], st["lad_hist_kappa"], planes)]
            _lib.check(self.lib.ptmi_ladder_publish(self.h))          # the handle's tables are those of the restored plane T
            self._lad_stale = True
        if self.t["DE"] is not None:
            self.set_de_head(int(st["de_head"]))
            if int(st["de_on"]):
                self.set_de_active(True)
        if int(st.get("eig_pending", 0)):
            # the checkpoint fell between a covariance epoch and the launch its table takes effect at: the factorization is
            # issued again from the saved covariance and becomes effective after the same number of launches
            if self.eig_mode in ("hipsolver", "sytrd", "ql"):
                self._eig_begin_side()
            else:
                self._eig_begin()
            self._eig_wait = int(st["eig_wait"])

    # pieces of the swap for a ladder sharded over GPUs (see sharded.py)
    def gather_lnl(self, out):
        _lib.check(self.lib.ptmi_swap_gather_lnl(self.h, out.data_ptr()))

    def sweep(self, it, lnl_glob, map_out):
        _lib.check(self.lib.ptmi_swap_sweep(self.h, it, lnl_glob.data_ptr(), map_out.data_ptr()))

    def write_am(self, it):
        _lib.check(self.lib.ptmi_swap_write_am(self.h, it))

    # device-side exchange (no host synchronisation), see include/ptmi.h
    def sweep_blocks(self, it, lnl_blocks, map_out):
        _lib.check(self.lib.ptmi_swap_sweep_blocks(self.h, it, lnl_blocks.data_ptr(), map_out.data_ptr()))

    def exchange_pack(self, map_dev, send):
        _lib.check(self.lib.ptmi_exchange_pack(self.h, map_dev.data_ptr(), send.data_ptr()))

    def exchange_apply(self, recv):
        _lib.check(self.lib.ptmi_exchange_apply(self.h, recv.data_ptr()))

    def exchange_multihop(self):
        """After exchange_pack: does any row of this sweep travel beyond a neighbouring block? (same answer on every GPU)"""
        v = C.c_int32(0)
        _lib.check(self.lib.ptmi_exchange_multihop(self.h, C.byref(v)))
        return bool(v.value)

    def exchange_violations(self):
        v = C.c_int32(0)
        _lib.check(self.lib.ptmi_exchange_status(self.h, C.byref(v)))
        return v.value

    def _epochs(self, it):
        cu, burn = self.cov_update, self.burn
        de_now = (it - 1) % burn == 0 and it - 1 != 0
        if de_now and self.stats_async:
            self.update_de(it - 1)                                    # reads the ring of the period that ends here: before the switch
        if (it - 1) % cu == 0 and it - 1 != 0:
            self.update_cov(it - 1)
        if de_now and not self.stats_async:
            self.update_de(it - 1)                                    # :563-571
        if it - 1 == burn and self.weights[2] > 0 and self.t["DE"] is not None:
            self.set_de_active(True)                                  # :574-585

    def _segment_end(self, it, last):
        """Last iteration of the launch that starts at ``it``: no epoch inside, swap only at its end."""
        end = last
        pers = [self.cov_update, self.burn]
        if self.tskip > 0 and self.ntg > 1:
            pers.append(self.tskip)
        for per in pers:
            end = min(end, ((it - 1) // per + 1) * per)
        return end

    # ------------------------------------------------------------------ stepping
    def mh_steps(self, iter0, nsteps):
        if self.rows_logl:                                            # the split path with the built-in row kernels: the same chains
            return self.callback_segment(iter0, iter0 + nsteps - 1, *self._rows_callbacks())
        _lib.check(self.lib.ptmi_mh_steps(self.h, iter0, nsteps))

    def last_variant(self):
        """Flags of the fused-kernel instantiation the last ``mh_steps`` launched (``_lib.VAR_*``), lanes, slots."""
        v = C.c_int32(0)
        _lib.check(self.lib.ptmi_last_mh_variant(self.h, C.byref(v)))
        return (v.value & 0xFFF) | (v.value & _lib.VAR_UTPAD), (v.value >> 12) & 0xFF, (v.value >> 20) & 0xFF

    def last_gj_launch(self):
        """(layout | flags, LDS levels of the tree stack, dynamic LDS bytes, chain slots) of the last gradient-jump launch of ``mh_steps``
        (``_lib.GJL_*``; ``ptmi_last_gj_launch``): all zero before the first one."""
        v = [C.c_int32(0) for _ in range(4)]
        _lib.check(self.lib.ptmi_last_gj_launch(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def last_swap_launch(self):
        """(kernel, walkers per block, dynamic LDS bytes, multi-hop scan in the write-out) of the last swap launch -- ``swap``, ``sweep``
        or ``sweep_blocks`` (``_lib.SWL_*``; ``ptmi_last_swap_launch``): all zero before the first one."""
        v = [C.c_int32(0) for _ in range(4)]
        _lib.check(self.lib.ptmi_last_swap_launch(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def swap(self, it):
        """PT swap of iteration ``it`` with the whole ladder on this GPU (:631-697)."""
        _lib.check(self.lib.ptmi_swap(self.h, it))
        self.swap_proposed += 1
        if self.evidence_on and it > self.evidence_from and (it // self.tskip) % self.evidence_every == 0:
            _lib.check(self.lib.ptmi_ev_update(self.h))               # the post-swap lnL of every (walker, rank): one sample
            self.ev_epochs += 1
        if self.adapt_on and it <= self.adapt_until:
            # the window counts this epoch by the parity of the pairs it tried (the sweep tries both); `every` epochs in: one update
            if self._lad_sweep:
                self.lad_tries[0] += 1
                self.lad_tries[1] += 1
            else:
                self.lad_tries[(it // self.tskip) & 1] += 1
            self.lad_epochs += 1
            if self.lad_epochs >= self.adapt_every:
                kappa = self.adapt_kappa * self.adapt_t0 / (self.lad_calls + self.adapt_t0)
                _lib.check(self.lib.ptmi_ladder_update(self.h, kappa, self.lad_tries[0], self.lad_tries[1]))
                self._lad_hist.append((int(it), kappa, self.t["lad"].clone()))      # a device copy: it goes to the host only when asked for
                self.lad_calls += 1
                self.lad_epochs, self.lad_tries = 0, [0, 0]
                self._lad_stale = True

    # ------------------------------------------------------------------ ladder adaptation
    def _lad_planes(self):
        """The planes behind every update so far, ``[m][3][n]`` on the host (device copies are brought down once)."""
        self._lad_hist = [(i, k, p if isinstance(p, np.ndarray) else p.cpu().numpy()) for i, k, p in self._lad_hist]
        return np.stack([p for _, _, p in self._lad_hist]) if self._lad_hist else np.zeros((0, 3, self.ntg))

    def ladder_history(self):
        """The updates of ``adapt_ladder`` so far: ``iter [m]`` (the swap iteration each ran behind), ``kappa [m]`` (its gain), ``A [m][n - 1]``
        (the acceptance of every pair over its window) and ``ladder [m][n]`` (the ladder it left)."""
        if not self.adapt_on:
            raise ValueError("no ladder adaptation: PTEngine.with_stages(..., adapt_ladder=True)")
        planes = self._lad_planes()
        return dict(iter=np.asarray([i for i, _, _ in self._lad_hist], dtype=np.int64),
                    kappa=np.asarray([k for _, k, _ in self._lad_hist], dtype=np.float64),
                    A=planes[:, 1, :-1].copy(), ladder=planes[:, 2, :].copy())

    # ------------------------------------------------------------------ log-evidence
    def evidence_moments(self):
        """The accumulators of the evidence stage by ``[W][T]`` (T the ranks, coldest first): ``n`` / ``skipped`` (uint64: samples taken,
        and samples left out because lnL was not finite), ``shift``, ``s1``, ``s2`` (mean lnL = shift + s1 / n, sum (lnL - shift)^2 = s2),
        ``m``, ``es`` (sum exp(dbeta_r lnL) = exp(m) es), and ``betas [T]`` = 1 / ``temps_mh``."""
        if not self.evidence_on:
            raise ValueError("no evidence stage: PTEngine.with_stages(..., evidence=True)")
        acc = self.t["ev_acc"].cpu().numpy()
        cnt = self.t["ev_cnt"].cpu().numpy().view(np.uint64)
        return dict(n=cnt[0].copy(), skipped=cnt[1].copy(), shift=acc[0].copy(), s1=acc[1].copy(), s2=acc[2].copy(), m=acc[3].copy(),
                    es=acc[4].copy(), betas=1.0 / self.temps_mh)

    def evidence(self):
        """ln Z from the samples so far (``evidence.estimates``): ``lnZ_ti``, ``lnZ_ti_corrected``, ``lnZ_ss``, each per walker and with
        the standard error of the walkers' scatter, ``mean`` / ``var`` of lnL per rank, ``beta_min`` (the range below the hottest beta is
        not integrated; with ``hot_chain=True`` it is nil)."""
        from .evidence import estimates
        mo = self.evidence_moments()
        return estimates(mo["betas"], mo["n"], mo["shift"], mo["s1"], mo["s2"], mo["m"], mo["es"])

    def run(self, niter):
        """Advance ``niter`` iterations (:499-503 for every chain)."""
        last = self.iter + niter
        it = self.iter + 1
        while it <= last:
            self._epochs(it)
            end = self._segment_end(it, last)
            self.mh_steps(it, end - it + 1)
            if self.tskip > 0 and self.ntg > 1 and end % self.tskip == 0:
                self.swap(end)
            if self._eig_pending:                                     # eig_lag launches after the epoch its table takes effect
                self._eig_wait -= 1
                # (when the next iteration opens a covariance epoch, update_cov finishes it: behind that epoch's statistics)
                if self._eig_wait <= 0 and not (end % self.cov_update == 0 and end + 1 <= last and self.owns_cold):
                    self._eig_finish()
            it = end + 1
        self.iter = last

    # ------------------------------------------------------------------ timing
    def timer_start(self):
        _lib.check(self.lib.ptmi_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_double(0)
        _lib.check(self.lib.ptmi_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    def lnprob(self):
        """beta * lnL + lp of every slot (the reference's lnprob0)."""
        beta = (1 / self.temps_mh)[self.get("temp_of")]
        return beta * self.get("lnL") + self.get("lp")
