"""Log-evidence from the ladder's per-temperature summaries (pure NumPy: no torch, no GPU).

The engine's evidence stage (``PTEngine.with_stages(evidence=True)``, csrc/ptmi_ev.hip) keeps, for every walker ``w`` and rank ``r`` of the
ladder, the count ``n``, the shift ``c`` (the cell's first sample), ``s1 = sum (lnL - c)``, ``s2 = sum (lnL - c)^2`` and the running
log-sum-exp ``(m, es)`` of ``dbeta_r * lnL`` with ``dbeta_r = beta_{r-1} - beta_r`` (``sum exp(dbeta_r lnL) = exp(m) es``).  ``estimates``
turns them into ln Z three ways, over the ladder AS GIVEN, ``betas[0] > betas[1] > ... > betas[-1] = beta_min``; below,
``D_r = betas[r] - betas[r + 1] > 0``:

* ``lnZ_ti``            the trapezoid of thermodynamic integration, ``sum_r D_r (mu_r + mu_{r+1}) / 2``, ``mu_r`` the mean of lnL at rank r;
* ``lnZ_ti_corrected``  ``lnZ_ti - sum_r D_r^2 (var_r - var_{r+1}) / 12``: the trapezoid's second-order term (Friel, Hurn & Wyse 2014),
                        from ``d<lnL>/dbeta = Var lnL``;
* ``lnZ_ss``            the stepping-stone value (Xie et al. 2011), ``sum_{r >= 1} log mean exp(dbeta_r lnL)`` sampled at rank r.

All three integrate from ``beta_min`` to ``betas[0]``: what lies below the hottest beta, ``ln Z(beta_min)``, is NOT in them (``beta_min`` is
returned).  With the reference's ``hotChain=True`` the hottest rank runs at T = 1e80, the last stone reaches the prior and that range is
nil.  The walkers are independent replicas: every value also comes per walker, and their scatter gives its standard error."""
import numpy as np

KEYS = ("mean", "var", "lnZ_ti", "lnZ_ti_corrected", "lnZ_ss", "lnZ_ti_per_walker", "lnZ_ti_corrected_per_walker", "lnZ_ss_per_walker",
        "lnZ_ti_sem", "lnZ_ti_corrected_sem", "lnZ_ss_sem", "beta_min")


def dbeta_of(temps, dbeta0=0.0):
    """``dbeta [T]`` of ``ptmi_ev_attach`` from the ranks' temperatures (``temps_mh``), in double precision: ``dbeta[r] = 1 / T[r - 1] -
    1 / T[r]``; ``dbeta[0] = dbeta0`` is the caller's (0 on one GPU: rank 0 has no colder neighbour)."""
    beta = 1.0 / np.asarray(temps, dtype=np.float64)
    out = np.empty_like(beta)
    out[0] = dbeta0
    out[1:] = beta[:-1] - beta[1:]
    return out


def _sem(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.std(v, ddof=1) / np.sqrt(len(v))) if len(v) > 1 else float("nan")


def _ti(betas, mu, var):
    """(trapezoid, corrected) along the last axis of mu / var."""
    D = betas[:-1] - betas[1:]
    ti = np.sum(D * (mu[..., :-1] + mu[..., 1:]) / 2, axis=-1)
    return ti, ti - np.sum(D * D * (var[..., :-1] - var[..., 1:]) / 12, axis=-1)


def estimates(betas, n, shift, s1, s2, m, es):
    """``betas [T]`` (decreasing) and the accumulators by ``[W][T]`` -> a dict of ``mean`` / ``var`` of lnL per rank (pooled over the walkers:
    Chan's combination of the per-walker shifted sums; ``var`` divides by the count), ``lnZ_ti``, ``lnZ_ti_corrected``, ``lnZ_ss`` (pooled
    over the walkers), each as ``*_per_walker [W]`` too, its standard error ``*_sem = std(per-walker, ddof=1) / sqrt(W)`` (NaN for
    W = 1), and ``beta_min`` (see the module docstring: the range below it is not integrated).  A rank without samples gives NaN."""
    betas = np.asarray(betas, dtype=np.float64)
    n, shift, s1, s2, m, es = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (n, shift, s1, s2, m, es))
    W, T = n.shape
    if betas.shape != (T,) or T < 2 or any(a.shape != (W, T) for a in (shift, s1, s2, m, es)):
        raise ValueError("estimates: betas [T] with T >= 2 and six arrays by [W][T] (got %r and %r)" % (betas.shape, n.shape))
    if not (np.all(np.isfinite(betas)) and np.all(betas[:-1] > betas[1:]) and betas[-1] >= 0):
        raise ValueError("estimates: betas decrease from the coldest rank to the hottest and are >= 0")
    with np.errstate(invalid="ignore", divide="ignore"):
        mu_w = shift + s1 / n                                         # [W][T]
        M2_w = s2 - s1 * s1 / n                                       # sum (lnL - mu_w)^2 of a walker
        var_w = M2_w / n
        has = n > 0
        N = n.sum(0)                                                  # [T]
        mu = np.where(has, n * mu_w, 0.0).sum(0) / N
        var = (np.where(has, M2_w, 0.0).sum(0) + np.where(has, n * (mu_w - mu) ** 2, 0.0).sum(0)) / N
        ti, tic = _ti(betas, mu, var)
        ti_w, tic_w = _ti(betas, mu_w, var_w)
        # stepping stones: log sum exp(dbeta_r lnL) = m + log es per cell; rank 0 has no colder neighbour on this ladder
        lse_w = np.where(has, m + np.log(es), -np.inf)[:, 1:]         # [W][T - 1]
        top = lse_w.max(0)
        top = np.where(np.isfinite(top), top, 0.0)
        ss = np.sum(top + np.log(np.exp(lse_w - top).sum(0)) - np.log(N[1:]))
        ss_w = np.sum(lse_w - np.log(n[:, 1:]), axis=1)
    return dict(mean=mu, var=var, lnZ_ti=float(ti), lnZ_ti_corrected=float(tic), lnZ_ss=float(ss),
                lnZ_ti_per_walker=ti_w, lnZ_ti_corrected_per_walker=tic_w, lnZ_ss_per_walker=ss_w,
                lnZ_ti_sem=_sem(ti_w), lnZ_ti_corrected_sem=_sem(tic_w), lnZ_ss_sem=_sem(ss_w), beta_min=float(betas[-1]))
