"""Convergence diagnostics of every cold chain from the device's streaming sums (pure NumPy: no torch, no GPU).

The engine's diagnostics stage (``PTEngine.with_stages(diag=True)``, csrc/ptmi_diag.hip, include/ptmi.h ``ptmi_diag_*``) keeps, for every
walker ``w`` and parameter ``j``, over the ``n`` counted iterations of the walker's cold chain: the shift ``c`` (the first counted
sample), ``S1 = sum (x - c)``, ``S2 = sum (x - c)^2``, the sum ``A`` of the level-0 batch under way, and for the levels ``l = 0 .. L - 1``
of a binary counter over the ``k = n // b0`` completed batches of ``b0`` samples the sum ``Q[l]`` of the SQUARED sums of the completed
batches of length ``b_l = b0 << l`` and the first half ``H[l]`` of the pair under way.  ``estimates`` turns them into, per parameter:

* ``mean_w``, ``var_w``  ``[W][d]``: ``c + S1 / n`` and ``(S2 - S1^2 / n) / (n - 1)`` of every chain;
* ``mean``, ``var``      the mean over the walkers of ``mean_w``, and the pooled within-chain variance ``Wv = mean_w(var_w)``;
* ``rhat``               Gelman & Rubin (1992): ``B = n var_over_walkers(mean_w, ddof=1)``, ``rhat = sqrt(((n - 1) / n Wv + B / n) / Wv)``;
                         NaN below two walkers;
* ``tau_walkers``        ``B / Wv``, the replica estimator of the integrated autocorrelation time: window-free and unbiased, relative
                         standard error ``sqrt(2 / (W - 1))``;
* ``tau_batch``          ``[L][d]``, batch means pooled over the walkers: at every level with ``m_l = k >> l >= 2`` completed batches the
                         samples inside them sum to ``T = S1 - A - sum_{l' < l, bit l' of k set} H[l']`` (``batch_total``), the
                         per-walker variance of the batch sums is ``vb = (Q[l] - T^2 / m_l) / (m_l - 1)`` and
                         ``tau_batch[l] = mean_w(vb) / (b_l Wv)``; NaN elsewhere;
* ``level``, ``tau``     ``level`` is the largest ``l`` with ``W (m_l - 1) >= 256`` -- that holds the relative standard error
                         ``sqrt(2 / (W (m_l - 1)))`` of ``tau_batch[l]`` to 9 % or less -- and ``tau = max(1, tau_batch[level])`` (1 too
                         where the chains do not move at all: ``Wv = 0``); -1 and NaN while no level has that many batches;
* ``reliable``           ``b_level >= 10 tau`` with a finite ``tau_batch[level]``: the bias of batch means is about ``tau / (2 b)`` of
                         ``tau``, so this bounds it at 5 %;
* ``ess``                ``W n / tau`` over the walkers that count;
* ``nonfinite``          the number of walkers whose sums for the parameter are not finite (a NaN or an infinity went through the
                         chain); they are left out of every mean over walkers above (``W`` is then the number left).

The assumption: ``rhat`` and ``tau_walkers`` treat the walkers as INDEPENDENT replicas.  With per-walker covariances
(``cov_mode="per_walker"``) they are; under ``cov_mode="pooled"`` they are weakly coupled through the shared jump table and DE history
-- the coupling vanishes as the table settles, but early in a run it pulls the walkers' means together and ``rhat`` / ``tau_walkers`` read
low.  ``tau_batch`` looks along every chain by itself and makes no such assumption: ``tau``, ``ess`` and ``reliable`` rest on it alone."""
import numpy as np

PLANES = ("c", "S1", "S2", "A")
KEYS = ("mean_w", "var_w", "mean", "var", "rhat", "tau_walkers", "tau_batch", "tau", "level", "reliable", "ess", "nonfinite", "n", "k",
        "batch0", "levels", "nwalkers")
MIN_BATCH_DOF = 256                    # W (m_l - 1) at the level tau is read from: relative standard error sqrt(2 / 256) = 9 %
MAX_LEVELS = 16


def nplanes(levels):
    return 2 * int(levels) + 3


def planes(acc, levels):
    """``acc [2 L + 3][W][d]`` as ``ptmi_diag_attach`` lays it out -> ``dict(c, S1, S2, A [W][d], Q [L][W][d], H [L - 1][W][d])``."""
    acc = np.asarray(acc, dtype=np.float64)
    L = int(levels)
    if acc.ndim != 3 or acc.shape[0] != nplanes(L):
        raise ValueError("acc has %d planes for %d levels (2 L + 3 = %d)" % (acc.shape[0] if acc.ndim == 3 else -1, L, nplanes(L)))
    out = {name: acc[i] for i, name in enumerate(PLANES)}
    out["Q"], out["H"] = acc[4:4 + L], acc[4 + L:]
    return out


def batch_total(S1, A, H, k, l):
    """The sum of the (shifted) samples inside the ``k >> l`` completed level-``l`` batches: everything but the level-0 batch under way
    and the halves waiting for their partner below level ``l``."""
    T = S1 - A
    for lp in range(int(l)):
        if (int(k) >> lp) & 1:
            T = T - H[lp]
    return T


def _mean(v, ok, cnt):
    """Mean over the walkers that count (axis 0), NaN where there are none."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, v, 0.0).sum(0) / cnt


def estimates(mom):
    """``mom``: ``c``, ``S1``, ``S2``, ``A`` ``[W][d]``, ``Q [L][W][d]``, ``H [L - 1][W][d]``, ``n``, ``batch0`` (``PTEngine.diag_moments()``)
    -> the dict the module docstring describes."""
    c, S1, S2, A = (np.asarray(mom[k], dtype=np.float64) for k in PLANES)
    Q, H = np.asarray(mom["Q"], dtype=np.float64), np.asarray(mom["H"], dtype=np.float64)
    n, b0 = int(mom["n"]), int(mom["batch0"])
    L, (W, d) = Q.shape[0], c.shape
    k = n // b0
    nan = np.full(d, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(c) & np.isfinite(S1) & np.isfinite(S2) & np.isfinite(A) & np.isfinite(Q).all(0)
        if L > 1:
            ok &= np.isfinite(H).all(0)
        cnt = ok.sum(0).astype(np.float64)
        cnt = np.where(cnt > 0, cnt, np.nan)
        mean_w = c + S1 / n if n > 0 else np.full((W, d), np.nan)
        var_w = (S2 - S1 * S1 / n) / (n - 1) if n > 1 else np.full((W, d), np.nan)
        mean, Wv = _mean(mean_w, ok, cnt), _mean(var_w, ok, cnt)
        dev = np.where(ok, mean_w - mean, 0.0)
        B = np.where(cnt > 1, n * (dev * dev).sum(0) / (cnt - 1), np.nan)
        rhat = np.sqrt(((n - 1) / n * Wv + B / n) / Wv) if n > 1 else nan.copy()
        tau_walkers = B / Wv
        tau_batch = np.full((L, d), np.nan)
        level = -1
        for l in range(L):
            m = k >> l
            if m < 2:
                break
            T = batch_total(S1, A, H, k, l)
            vb = (Q[l] - T * T / m) / (m - 1)
            tau_batch[l] = _mean(vb, ok, cnt) / ((b0 << l) * Wv)
            if W * (m - 1) >= MIN_BATCH_DOF:
                level = l
        if level >= 0:
            tb = tau_batch[level]
            tau = np.where(tb > 1.0, tb, 1.0)
            tau = np.where(np.isnan(cnt), np.nan, tau)
            reliable = np.isfinite(tb) & ((b0 << level) >= 10.0 * tau)
        else:
            tau, reliable = nan.copy(), np.zeros(d, dtype=bool)
        ess = cnt * n / tau
    return dict(mean_w=mean_w, var_w=var_w, mean=mean, var=Wv, rhat=rhat, tau_walkers=tau_walkers, tau_batch=tau_batch, tau=tau,
                level=np.int64(level), reliable=reliable, ess=ess, nonfinite=(~ok).sum(0).astype(np.int64), n=np.int64(n), k=np.int64(k),
                batch0=np.int64(b0), levels=np.int64(L), nwalkers=np.int64(W))


def converged(est, stop_ess=None, stop_rhat=None):
    """The stop rule of ``PTSampler.chain_diagnostics``: every parameter reliable, ``min_j ess >= stop_ess`` and ``max_j rhat <= stop_rhat``
    (each where it is given).  Never true while any parameter is unreliable."""
    if stop_ess is None and stop_rhat is None:
        return False
    if not bool(np.all(est["reliable"])):
        return False
    with np.errstate(invalid="ignore"):
        if stop_ess is not None and not bool(np.all(est["ess"] >= float(stop_ess))):
            return False
        if stop_rhat is not None and not bool(np.all(est["rhat"] <= float(stop_rhat))):
            return False
    return True
