"""Joint posterior histograms of parameter pairs (csrc/ptmi_pairs.hip, include/ptmi.h ``ptmi_pairs_*``;
``PTEngine.with_stages(pairs=(pairs, lo, hi, nbins))``, ``PTSampler.posterior_pairs``): the host's side of the stage -- the spec
the engine and the sampler take, the counting rule restated in NumPy, and the thresholds a contour plot needs."""
import numpy as np

NBINS_MAX = 128
NPAIRS_MAX = 8192


def expand_pairs(ndim, pairs):
    """``pairs`` of a spec -> int32 [npairs][2]: an ``[npairs][2]`` integer array as it is, or ``{"params": [k indices]}`` = all
    ``k (k - 1) / 2`` pairs ``(a, b)`` with ``a`` before ``b`` in the list.  Two different parameters in ``0 .. ndim - 1`` each, and
    ``1 <= npairs <= 8192`` (``ptmi_pairs_attach``)."""
    if isinstance(pairs, dict):
        if set(pairs) != {"params"}:
            raise ValueError("pairs: a dict names the parameters, {\"params\": [indices]} (got keys %r)" % (sorted(pairs),))
        par = np.asarray(pairs["params"])
        if par.ndim != 1 or par.size < 2 or par.dtype.kind not in "iu":
            raise ValueError("pairs: {\"params\": [indices]} takes two or more integer indices")
        if len(set(par.tolist())) != par.size:
            raise ValueError("pairs: {\"params\": [indices]} names a parameter twice")
        k = par.size
        arr = np.array([(par[a], par[b]) for a in range(k) for b in range(a + 1, k)], dtype=np.int64)
    else:
        arr = np.asarray(pairs)
        if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind not in "iu":
            raise ValueError("pairs: an integer array [npairs][2] or {\"params\": [indices]} (got shape %r, dtype %s)" % (arr.shape, arr.dtype))
        arr = arr.astype(np.int64)
    if not 1 <= arr.shape[0] <= NPAIRS_MAX:
        raise ValueError("pairs: 1 <= npairs <= %d (got %d)" % (NPAIRS_MAX, arr.shape[0]))
    bad = (arr < 0).any(1) | (arr >= ndim).any(1) | (arr[:, 0] == arr[:, 1])
    if bad.any():
        p = int(np.flatnonzero(bad)[0])
        raise ValueError("pairs: pair %d = (%d, %d): two different parameters in 0 .. %d" % (p, arr[p, 0], arr[p, 1], ndim - 1))
    return np.ascontiguousarray(arr, dtype=np.int32)


def pairs_spec(ndim, spec):
    """``pairs=(pairs, lo, hi, nbins)`` of ``PTEngine.with_stages`` -> (pairs int32 [npairs][2], lo [ndim], hi [ndim], nbins), checked:
    ``expand_pairs``; ``lo`` / ``hi`` scalars or [ndim], lo < hi and finite; 2 <= nbins <= 128 (``ptmi_pairs_attach``)."""
    try:
        pairs, lo, hi, nbins = spec
    except (TypeError, ValueError):
        raise ValueError("pairs=(pairs, lo, hi, nbins)") from None
    if isinstance(nbins, bool) or not isinstance(nbins, (int, float, np.integer, np.floating)) or int(nbins) != nbins \
            or not 2 <= int(nbins) <= NBINS_MAX:
        raise ValueError("pairs: 2 <= nbins <= %d (got %r)" % (NBINS_MAX, nbins))
    out = []
    for name, v in (("lo", lo), ("hi", hi)):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(ndim, float(v))
        if v.shape != (ndim,):
            raise ValueError("pairs: %s is a scalar or has ndim = %d entries (got shape %r)" % (name, ndim, v.shape))
        out.append(np.ascontiguousarray(v))
    lo, hi = out
    bad = ~(np.isfinite(lo) & np.isfinite(hi) & (lo < hi))
    with np.errstate(over="ignore"):
        scale = int(nbins) / np.where(bad, 1.0, hi - lo)
    bad |= ~np.isfinite(scale)
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise ValueError("pairs: lo < hi, both finite (parameter %d: lo = %r, hi = %r)" % (j, lo[j], hi[j]))
    return expand_pairs(ndim, pairs), lo, hi, int(nbins)


def pairs_rule(x, pairs, lo, hi, nbins, weight=None):
    """The contract, restated: ``x [..., d]`` -> uint64 ``[npairs][nbins * nbins + 1]`` (``pairs`` as ``expand_pairs`` takes them).  Per axis ``t = (x - lo) * (nbins / (hi - lo))``
    (one subtraction, one multiplication), inside where ``t >= 0`` and not ``t >= nbins``; a row with both coordinates of a pair
    ``(i, j)`` inside goes to cell ``int(ti) * nbins + int(tj)``, any other (NaN, below ``lo``, at or above ``hi``, infinite) to the
    pair's last cell, "outside".  ``weight`` (integers, one per row; default 1) is how many iterations a row stands for."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[-1]
    nbins = int(nbins)
    pairs = expand_pairs(d, pairs).astype(np.int64)                  # (either form of a spec's pairs)
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (d,)), np.broadcast_to(np.asarray(hi, np.float64), (d,))
    scale = nbins / (hi - lo)
    x = x.reshape(-1, d)
    w = np.ones(x.shape[0], dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64).reshape(-1)
    cells = nbins * nbins
    # the bin of every needed column once: -1 = outside
    bins = {}
    for j in np.unique(pairs):
        with np.errstate(invalid="ignore"):
            t = (x[:, j] - lo[j]) * scale[j]
            inside = (t >= 0.0) & ~(t >= nbins)
        b = np.full(x.shape[0], -1, dtype=np.int64)
        b[inside] = t[inside].astype(np.int64)
        bins[int(j)] = b
    out = np.zeros((len(pairs), cells + 1), dtype=np.uint64)
    for p, (i, j) in enumerate(pairs):
        bi, bj = bins[int(i)], bins[int(j)]
        cell = np.where((bi < 0) | (bj < 0), cells, bi * nbins + bj)
        out[p] = np.bincount(cell, weights=w, minlength=cells + 1).astype(np.uint64)
    return out


def credible_levels(counts, probs=(0.68, 0.95)):
    """Highest-density count thresholds for contour drawing: ``counts [npairs][nbins][nbins]`` (or one table) -> float64
    ``[npairs][len(probs)]`` (or ``[len(probs)]``).  Per pair the cells are sorted in descending order and summed; the level of
    probability ``q`` is the count of the cell at which the cumulative sum first reaches ``q`` times the inside total: the cells with
    at least that count hold at least ``q`` of the samples.  A pair with no sample inside gets NaN."""
    c = np.asarray(counts)
    one = c.ndim == 2
    if one:
        c = c[None]
    if c.ndim != 3:
        raise ValueError("credible_levels: counts [npairs][nbins][nbins] (got shape %r)" % (c.shape,))
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    if not ((probs > 0.0) & (probs <= 1.0)).all():
        raise ValueError("credible_levels: 0 < probs <= 1")
    out = np.full((c.shape[0], probs.size), np.nan)
    for p in range(c.shape[0]):
        s = np.sort(c[p].reshape(-1))[::-1].astype(np.float64)
        total = s.sum()
        if total <= 0:
            continue
        idx = np.minimum(np.searchsorted(np.cumsum(s), probs * total, side="left"), s.size - 1)      # (integer sums: exact in f64)
        out[p] = s[idx]
    return out[0] if one else out
