"""The device's tridiagonal divide-and-conquer eigensolver and its Householder reduction (eig_mode "sytrd": csrc/ptmi_dc.inc.h and
sytrd_lds_kernel of csrc/ptmi_eig.hip), restated in numpy for the CPU: the same tree, the same leaf recurrence, the same deflation
rule, bisection, Loewner weights and ranking -- in a form a reader can hold against LAPACK's dstedc / dlaed2 / dsytd2.  It does NOT
aim at the device's last bits: the device sums over 64 lanes and over matrix-core tiles, this file in numpy's order.  What it shares
with the device is every decision: which eigenvalues deflate, which pole a root is measured from, how ties are ranked."""
import math

import numpy as np

EPS = 2.220446049250313e-16
LEAF = 16              # rows of a leaf (dc::LEAF)
SWEEPS = 60            # QL sweeps a leaf allows per eigenvalue
BISECT = 1200          # bisection steps a root allows (it ends by itself long before)
# A deflation test x <= tol "has a margin" when another summation order could not decide it the other way.  The error model: every
# component of a child's (unit) eigenvector and every child's eigenvalue, the latter relative to the node's norm, is known to
# ERR eps -- so rho |z_j| to rho ERR eps, and |dt c s| to |c s| ERR eps norm + |dt c s| ERR eps (1 / |z_p| + 1 / |z_j|) -- and tol
# itself to a few ulp.  A test whose value lies within that of tol is DOUBTFUL.
ERR = 8.0


def plan(n):
    """(leaves, levels) as dc_plan_get builds them: leaves [(off, rows)] left to right, all at one depth -- the smallest with
    ceil(n / 2**depth) <= LEAF --, levels bottom-up, each a list of merges (off, rows, n1) left to right with n1 = rows // 2 the
    first child's rows."""
    depth = 0
    while (n + (1 << depth) - 1) >> depth > LEAF:
        depth += 1
    by_depth = [[] for _ in range(depth)]
    leaves = []

    def go(off, nn, dep):
        if dep == depth:
            leaves.append((off, nn))
            return
        n1 = nn // 2
        by_depth[dep].append((off, nn, n1))
        go(off, n1, dep + 1)
        go(off + n1, nn - n1, dep + 1)

    go(0, n, 0)
    return leaves, by_depth[::-1]


def _hyp(a, b):
    """sqrt(a^2 + b^2) without overflow (dc::hyp)."""
    x, y = abs(a), abs(b)
    hi, lo = (x, y) if x > y else (y, x)
    if hi == 0.0:
        return 0.0
    q = lo / hi
    return hi * math.sqrt(1.0 + q * q)


def leaf(d, e):
    """Implicit QL with eigenvectors (the tql2 recurrence of leaf_kernel) on the tridiagonal matrix (d, e): returns (D, Z, converged)
    with Z vector-major (Z[c] belongs to D[c]) and D in the order the iteration leaves it -- the merge sorts."""
    m0 = len(d)
    dd = [float(x) for x in d]
    ee = [float(x) for x in e] + [0.0]
    z = np.eye(m0)                                             # z[r][c]: component r of vector c
    converged = True
    for l in range(m0):
        conv = False
        for it in range(SWEEPS + 1):
            m = l
            while m < m0 - 1:
                if abs(ee[m]) <= EPS * (abs(dd[m]) + abs(dd[m + 1])):
                    break
                m += 1
            if m == l:
                conv = True
                break
            if it == SWEEPS:
                break
            g = (dd[l + 1] - dd[l]) / (2.0 * ee[l])
            rr = _hyp(g, 1.0)
            g = dd[m] - dd[l] + ee[l] / (g + (rr if g >= 0.0 else -rr))
            s, c, p = 1.0, 1.0, 0.0
            under = False
            for i in range(m - 1, l - 1, -1):
                f = s * ee[i]
                b = c * ee[i]
                rr = _hyp(f, g)
                ee[i + 1] = rr
                if rr == 0.0:                                  # the underflow branch
                    dd[i + 1] -= p
                    ee[m] = 0.0
                    under = True
                    break
                s = f / rr
                c = g / rr
                g = dd[i + 1] - p
                rr = (dd[i] - g) * s + 2.0 * c * b
                p = s * rr
                dd[i + 1] = g + p
                g = c * rr - b
                fz = z[:, i + 1].copy()
                z[:, i + 1] = s * z[:, i] + c * fz
                z[:, i] = c * z[:, i] - s * fz
            if under:
                continue
            dd[l] -= p
            ee[l] = g
            ee[m] = 0.0
        converged = converged and conv
    return np.array(dd), np.ascontiguousarray(z.T), converged


def merge(Din, Qin, d, e, n1):
    """One merge of a node of nn rows: Din [nn] the children's eigenvalues (first child's, then second's), Qin [nn][nn] their
    vectors (vector-major, block diagonal), (d, e) the node's own tridiagonal matrix after the splits ([nn], [nn - 1]: its norm goes
    into the tolerance, e[n1 - 1] is the entry cut).  Returns (Dout ascending, Qout, k, ndefl, doubt): k secular roots, ndefl
    deflated eigenvalues, doubt the number of deflation tests without a margin (see ERR; each could move k by one)."""
    nn = len(Din)
    Q = np.array(Qin, dtype=float)
    e_cut = float(e[n1 - 1])
    sgn = -1.0 if e_cut < 0.0 else 1.0
    z = np.concatenate([Q[:n1, n1 - 1], sgn * Q[n1:, n1]]) * 0.70710678118654752440      # |z| = sqrt 2 -> 1 (rho doubles)
    perm = np.argsort(np.asarray(Din, dtype=float), kind="stable")                       # ties by index
    Ds, zs = np.array(Din, dtype=float)[perm], z[perm]
    rho = 2.0 * abs(e_cut)
    dmax, zmax = np.abs(Ds).max(), np.abs(zs).max()
    nrm = np.abs(d).max() + np.abs(e).max()
    znorm = zmax * nrm
    tol = 8.0 * EPS * max(dmax, znorm)
    doubt = 0

    def small(x, dx):
        nonlocal doubt
        if x != 0.0 and abs(x - tol) <= dx + 64.0 * EPS * tol:
            doubt += 1
        return x <= tol

    keep, defl, rots = [], [], []
    if small(rho * zmax, rho * ERR * EPS):
        defl = list(range(nn))                                 # nothing couples the halves
    else:
        pj = -1
        for j in range(nn):
            if small(rho * abs(zs[j]), rho * ERR * EPS):
                defl.append(j)
                continue
            if pj < 0:
                pj = j
                continue
            s, c = zs[pj], zs[j]
            tau, dt = _hyp(c, s), Ds[j] - Ds[pj]
            c /= tau
            s = -s / tau
            x = abs(dt * c * s)
            if small(x, ERR * EPS * (abs(c * s) * nrm + x * (1.0 / abs(zs[pj]) + 1.0 / abs(zs[j])))):      # close pair: rotate z[pj] away (dlaed2)
                zs[j], zs[pj] = tau, 0.0
                rots.append((pj, j, c, s))
                dp, dj = Ds[pj], Ds[j]
                Ds[pj] = dp * c * c + dj * s * s
                Ds[j] = dp * s * s + dj * c * c
                defl.append(pj)
            else:
                keep.append(pj)
            pj = j
        if pj >= 0:
            keep.append(pj)
    for pj, j, c, s in rots:
        vp, vj = Q[perm[pj]].copy(), Q[perm[j]].copy()
        Q[perm[pj]] = c * vp + s * vj
        Q[perm[j]] = -s * vp + c * vj
    k, ndf = len(keep), len(defl)
    dk, zk = Ds[keep], zs[keep]
    Ddefl = Ds[defl]
    Qout = np.zeros_like(Q)
    lam = np.zeros(0)
    if k:
        # the secular roots: root j in (d_j, d_j+1), the last in (d_k-1, d_k-1 + rho |z|^2), by bisection from the closer pole
        zz = zk * zk

        def f_at(o, m):                                        # 1 + rho sum_i zz_i / ((d_i - o) - m), one row per root
            with np.errstate(divide="ignore", invalid="ignore"):
                return 1.0 + rho * (zz[None, :] / ((dk[None, :] - o[:, None]) - m[:, None])).sum(axis=1)

        org = np.arange(k)
        o = dk.copy()
        lo, hi = np.zeros(k), np.zeros(k)
        hi[k - 1] = rho * zz.sum()
        if k > 1:
            mid = 0.5 * (dk[1:] - dk[:-1])
            near = f_at(dk[:-1], mid) > 0.0                    # the root is nearer to d_j
            hi[:-1] = np.where(near, mid, 0.0)
            lo[:-1] = np.where(near, 0.0, -mid)
            org[:-1] = np.where(near, org[:-1], org[:-1] + 1)
            o[:-1] = dk[org[:-1]]
        live = np.ones(k, dtype=bool)
        for _ in range(BISECT):
            m = 0.5 * (lo + hi)
            live &= ~((m == lo) | (m == hi))
            if not live.any():
                break
            pos = f_at(o, m) > 0.0
            hi = np.where(live & pos, m, hi)
            lo = np.where(live & ~pos, m, lo)
        mu = 0.5 * (lo + hi)
        lam = o + mu
        DM = (dk[:, None] - dk[org][None, :]) - mu[None, :]    # d_i - lambda_j from the shifted root
        # Loewner: z^_i = sign(z_i) sqrt(prod_j (lambda_j - d_i) / prod_{j != i} (d_j - d_i) / rho)
        den = dk[None, :] - dk[:, None]
        np.fill_diagonal(den, 1.0)
        zh = np.sqrt(np.abs(np.prod(-DM / den, axis=1)) / rho)
        zh = np.where(zk < 0.0, -zh, zh)
        U = (zh[:, None] / DM).T                               # U[j][i] = z^_i / (d_i - lambda_j)
        U = U * (1.0 / np.sqrt((U * U).sum(axis=1)))[:, None]
    val = np.concatenate([lam, Ddefl])
    rank = np.empty(nn, dtype=int)
    rank[np.argsort(val, kind="stable")] = np.arange(nn)       # ascending, ties by position: roots before deflated values
    Dout = np.empty(nn)
    Dout[rank] = val
    if k:
        Qout[rank[:k]] = U @ Q[perm[keep]]
    if ndf:
        Qout[rank[k:]] = Q[perm[defl]]
    return Dout, Qout, k, ndf, doubt


def solve(d, e, detail=False):
    """Eigenvalues (ascending) and eigenvectors (vector-major) of the symmetric tridiagonal matrix (d [n], e [n - 1]) as dc_solve
    computes them (as ptmi_eig_dc_tridiag returns them: a matrix of one leaf sorted too), and counts: (k, ndefl) of every merge in the plan's order (bottom level first).  detail=True adds the list of
    every merge's number of doubtful deflation tests (0: the merge has a margin) and whether every leaf converged."""
    d = np.array(d, dtype=float)
    e = np.array(e, dtype=float)
    n = len(d)
    leaves, levels = plan(n)
    for level in levels:                                       # the rank-one modifications of all splits
        for off, nn, n1 in level:
            r = abs(e[off + n1 - 1])
            d[off + n1 - 1] -= r
            d[off + n1] -= r
    D, Q = np.zeros(n), np.zeros((n, n))
    converged = True
    for off, m in leaves:
        D[off:off + m], Q[off:off + m, off:off + m], ok = leaf(d[off:off + m], e[off:off + m - 1])
        converged = converged and ok
    counts, margins = [], []
    for level in levels:
        for off, nn, n1 in level:
            sl = slice(off, off + nn)
            D[sl], Q[sl, sl], k, ndf, doubt = merge(D[sl], Q[sl, sl], d[sl], e[off:off + nn - 1], n1)
            counts.append((k, ndf))
            margins.append(doubt)
    if not levels:                                             # one leaf, no merge to sort it: ranked as ptmi_eig_dc_tridiag ranks it
        order = np.argsort(D, kind="stable")
        D, Q = D[order], Q[order]
    if detail:
        return D, Q, counts, margins, converged
    return D, Q, counts


def sytrd_lower(A):
    """Unblocked Householder tridiagonalization in LAPACK dsytd2's lower convention, with the dlarfg branch of sytrd_lds_kernel: a
    column whose tail below the subdiagonal is exactly zero gives tau = 0 and keeps its subdiagonal entry, else
    beta = -sign(alpha) |(alpha, tail)|.  Returns (D, E, tau, V): Q^T A Q = tridiag(D, E), Q = H(0) ... H(n - 2),
    H(m) = I - tau[m] v v^T, v = (0 .. 0, 1 at m + 1, V[m + 2:, m])."""
    A = np.array(A, dtype=float)
    n = A.shape[0]
    D, E, tau, V = np.zeros(n), np.zeros(max(n - 1, 0)), np.zeros(max(n - 1, 0)), np.zeros((n, n))
    for m in range(n - 1):
        alpha = A[m + 1, m]
        x = A[m + 2:, m].copy()
        xn2 = float(x @ x)
        beta, t = alpha, 0.0
        if xn2 != 0.0:
            nrm = math.sqrt(alpha * alpha + xn2)
            beta = -nrm if alpha >= 0.0 else nrm
            t = (beta - alpha) / beta
            x *= 1.0 / (alpha - beta)
        else:
            x[:] = 0.0
        D[m], E[m], tau[m] = A[m, m], beta, t
        V[m + 2:, m] = x
        if t != 0.0:
            v = np.concatenate([[1.0], x])
            sub = A[m + 1:, m + 1:]
            p = t * (sub @ v)
            w = p - 0.5 * t * (p @ v) * v
            sub -= np.outer(v, w) + np.outer(w, v)
    if n:
        D[n - 1] = A[n - 1, n - 1]
    return D, E, tau, V


def q_from_reflectors(V, tau):
    """Q = H(0) H(1) ... H(n - 2) from reflectors in the storage sytrd_lower returns."""
    n = V.shape[0]
    Q = np.eye(n)
    for m in range(n - 2, -1, -1):
        v = np.zeros(n)
        v[m + 1] = 1.0
        v[m + 2:] = V[m + 2:, m]
        Q -= tau[m] * np.outer(v, v @ Q)
    return Q
