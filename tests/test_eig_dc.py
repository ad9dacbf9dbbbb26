"""oracle/eig_dc.py -- the CPU restatement of eig_mode "sytrd" (Householder reduction, divide and conquer on the tridiagonal matrix:
csrc/ptmi_eig.hip sytrd_lds_kernel, csrc/ptmi_dc.inc.h) -- against LAPACK, and the matrices, metrics and bounds that
tests/test_eig_dc_gpu.py holds the device to.  No GPU here.

The metrics of a factorization (w, V) of a symmetric matrix A (V vector-major), all relative to max|A|:
  residual       max|A V^T - V^T diag(w)| / max|A|
  orthogonality  max|V V^T - I|
  eigenvalues    max|w - w_eigh| / max|A|
The yardstick of the first two is the same metric of numpy.linalg.eigh (LAPACK) on the same matrix -- n eps where LAPACK's own value
is 0 to rounding, that is below eps: a diagonal matrix, a 2 x 2 one (3e-18; the metrics are differences of numbers of order 1) --, of
the third n eps (LAPACK's distance from itself is 0).  A bound is FACTOR x yardstick, at most the 1e-12 the header documents; every
FACTOR is the next power of two above twice the worst ratio measured, on an MI355X for the device and here for the restatement
(profiles/r21_eig_dc.txt)."""
import numpy as np
import pytest

from oracle import eig_dc

from test_eig_jacobi import _sytrd_matrix

EPS = np.finfo(float).eps
CEILING = 1e-12
# measured, profiles/r21_eig_dc.txt: the worst ratios are 3.74 (residual, glued168), 2.6 (orthogonality, random15) and 0.414
# (eigenvalues, random16) for the restatement AND for the device (orders up to 16 are one leaf: the same recurrence)
ORACLE_FACTORS = dict(residual=8.0, orthogonality=8.0, eigenvalues=1.0)
DEVICE_FACTORS = dict(residual=8.0, orthogonality=8.0, eigenvalues=1.0)
PLAN_ORDERS = (1, 2, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 127, 129, 257, 1000, 1023, 1024)
RANDOM_ORDERS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 34, 63, 64, 65, 127, 129, 257)
POW2_SCALES = (2.0 ** -300, 2.0 ** -100, 2.0 ** -40, 2.0 ** 40, 2.0 ** 100, 2.0 ** 300)
SCALES = POW2_SCALES[:3] + (1e-10, 1.0) + POW2_SCALES[3:]
SCALE_MATRICES = (("scaled", 40), ("scaled", 130), ("isotropic", 130), ("clusters", 130))
# A merge's counts (k, ndefl) are compared EXACTLY with the restatement's where every deflation test of the restatement has a margin
# (eig_dc.ERR), and to within the number of its doubtful tests elsewhere.  At most a quarter of a case's merges may be of the second
# kind -- but for glued168: eight copies of W21 a 1e-8 apart are made of eigenvalue pairs that differ by about the tolerance itself,
# 5 of its 15 merges hold such a pair (measured here, on the CPU, before any device run).
MAX_INEXACT = 0.25
MAX_INEXACT_GLUED = 5
# ... and a merge with many doubtful tests (random127's top merge has 36: its rho is so large that tol / rho is below the 8 eps the
# error model allows a component, so every deflated component counts) may still move k by at most this many.  Not a measurement: a
# component at the tolerance that is kept instead of deflated meets the pair test next with c s ~ z_j / z_p tiny and is rotated
# away there, so a flipped test seldom moves k at all; a scan that is broken moves it by more than a few.
MAX_ALLOWANCE = 4


def dense(d, e):
    return np.diag(np.asarray(d, dtype=float)) + np.diag(e, 1) + np.diag(e, -1)


def clement(n):
    """Zero diagonal, e_i = sqrt(i (n - i)): the eigenvalues are exactly +-(n - 1), +-(n - 3), ..."""
    i = np.arange(1.0, n)
    return np.zeros(n), np.sqrt(i * (n - i))


def tridiag_cases():
    """name -> (d, e): what goes straight into the merges."""
    cases = {}
    for n in RANDOM_ORDERS:
        rng = np.random.default_rng(2000 + n)           # (seeds 2000 + n: every case inside MAX_INEXACT, found on the CPU; 1000 + 63 is not)
        cases["random%d" % n] = (rng.standard_normal(n), rng.standard_normal(n - 1))
    cases["toeplitz257"] = (np.full(257, 2.0), np.ones(256))
    cases["clement200"] = clement(200)
    w21 = np.abs(np.arange(21) - 10.0)
    cases["glued168"] = (np.tile(w21, 8), np.where(np.arange(1, 168) % 21 == 0, 1e-8, 1.0))
    cases["wilkinson65"] = (np.abs(np.arange(65) - 32.0), np.ones(64))
    rng = np.random.default_rng(7)
    d, e = rng.standard_normal(129), rng.standard_normal(128)            # off-diagonals of both signs ...
    cases["signs129"] = (d, e)
    cases["flipped129"] = (d, e * flip_signs(129)[1:] * flip_signs(129)[:-1])      # ... and D T D of the same matrix
    d, e = rng.standard_normal(65), rng.standard_normal(64)
    e[31] = 0.0                                                          # the top cut of 65 = 32 + 33
    cases["zerocut65"] = (d, e)
    d, e = rng.standard_normal(65), rng.standard_normal(64)
    e[3] = 0.0                                                           # inside the first leaf (rows 0 .. 7)
    cases["zeroleaf65"] = (d, e)
    cases["diagonal65"] = (rng.permutation(65) * 0.37 - 9.0, np.zeros(64))
    cases["identity65"] = (np.full(65, 0.01), np.zeros(64))
    return cases


def check_toeplitz(W, Z):
    """The 1-2-1 Toeplitz matrix in closed form: eigenvalues 2 - 2 cos(j pi / (n + 1)) ascending, sine eigenvectors."""
    n = len(W)
    j = np.arange(1, n + 1)
    assert np.abs(W - (2 - 2 * np.cos(j * np.pi / (n + 1)))).max() <= 8 * EPS * 4          # a few ulp of max|lambda| = 4
    S = np.sqrt(2 / (n + 1)) * np.sin(np.outer(n + 1 - j, j) * np.pi / (n + 1))            # row j - 1: the vector of the j-th smallest
    dots = np.einsum("vi,vi->v", Z, S)
    assert np.abs(np.abs(dots) - 1).max() <= 1e-13
    assert np.abs(Z * np.sign(dots)[:, None] - S).max() <= 1e-11                            # gaps of 1.5e-4 at the ends: eps / gap


def flip_signs(n):
    return np.where(np.random.default_rng(n).random(n) < 0.5, -1.0, 1.0)


def zero_rows(n=60, rows=(17, 41)):
    """A dense covariance with two parameters that never moved: two zero rows and columns."""
    A = _sytrd_matrix("scaled", n)
    for r in rows:
        A[r, :] = 0.0
        A[:, r] = 0.0
    return A


def block_diagonal():
    A = np.zeros((120, 120))
    A[:50, :50] = _sytrd_matrix("scaled", 50)
    A[50:, 50:] = _sytrd_matrix("scaled", 70)
    return A


def singular_cases():
    """name -> dense symmetric matrix: singular and indefinite input of the whole pipeline."""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((40, 130))
    X -= X.mean(axis=0)
    Q, _ = np.linalg.qr(rng.standard_normal((200, 200)))
    C = Q @ dense(*clement(200)) @ Q.T
    return {"rank39": X.T @ X / 39, "zerorows": zero_rows(130, (17, 41)), "clement_rotated": 0.5 * (C + C.T)}


def scaled_matrix(kind, d, scale):
    """_sytrd_matrix(kind, d) times scale, clear of overflow and underflow in the reduction's alpha^2 + |x|^2."""
    A = _sytrd_matrix(kind, d) * scale
    big = np.abs(A).max() ** 2 * d
    assert np.isfinite(big) and big < 1e300 and np.abs(A).max() ** 2 > 1e-280, (kind, d, scale)
    return A


def metrics(A, w, V):
    """(residual, orthogonality) of the factorization (w, V), V vector-major."""
    n = A.shape[0]
    amax = np.abs(A).max() or 1.0
    return np.abs(A @ V.T - V.T * w).max() / amax, np.abs(V @ V.T - np.eye(n)).max()


def yardsticks(A):
    """eigh's eigenvalues and the yardstick of every metric on A."""
    n = A.shape[0]
    w, v = np.linalg.eigh(A)
    res, orth = metrics(A, w, v.T)
    return w, dict(residual=res if res >= EPS else n * EPS, orthogonality=orth if orth >= EPS else n * EPS, eigenvalues=n * EPS)


def ratios(A, w, V, by_size=False):
    """metric / yardstick for the three metrics.  w ascending against eigh's, or (by_size) |w| descending against eigh's |w| sorted."""
    w_ref, ref = yardsticks(A)
    res, orth = metrics(A, w, V)
    amax = np.abs(A).max() or 1.0
    err = np.abs(np.abs(w) - np.sort(np.abs(w_ref))[::-1]).max() if by_size else np.abs(w - w_ref).max()
    got = dict(residual=res, orthogonality=orth, eigenvalues=err / amax)
    return {k: got[k] / ref[k] for k in got}, got, ref


def check(tag, A, w, V, factors, by_size=False):
    """Print every figure, then hold each metric to min(FACTOR x yardstick, 1e-12)."""
    r, got, ref = ratios(A, w, V, by_size)
    print("%-28s n=%4d  " % (tag, A.shape[0]) + "  ".join("%s %.2e / %.2e = %.3g" % (k[:4], got[k], ref[k], r[k]) for k in r))
    for k in r:
        assert got[k] <= min(factors[k] * ref[k], CEILING), (tag, k, got[k], ref[k], r[k])
    return r


@pytest.mark.parametrize("n", PLAN_ORDERS)
def test_plan_tiles_the_matrix(n):
    leaves, levels = eig_dc.plan(n)
    assert [off for off, _ in leaves] == list(np.cumsum([0] + [m for _, m in leaves])[:-1]) and sum(m for _, m in leaves) == n
    assert all(1 <= m <= eig_dc.LEAF for _, m in leaves)
    depth = len(levels)
    assert len(leaves) == 2 ** depth                                    # all leaves at one depth: a full binary tree
    assert depth == 0 or -(-n // 2 ** depth) <= 16 < -(-n // 2 ** (depth - 1))
    below = [(off, m) for off, m in leaves]
    for level in levels:                                                # bottom-up: a merge's children are the two nodes below it
        assert len(level) * 2 == len(below)
        for i, (off, nn, n1) in enumerate(level):
            assert n1 == nn // 2 and below[2 * i] == (off, n1) and below[2 * i + 1] == (off + n1, nn - n1)
        below = [(off, nn) for off, nn, _ in level]
    assert below == [(0, n)]


@pytest.fixture(scope="module")
def solved():
    """The restatement's answer for every tridiagonal case, computed once."""
    return {name: eig_dc.solve(d, e, detail=True) for name, (d, e) in tridiag_cases().items()}


@pytest.mark.parametrize("name", list(tridiag_cases()))
def test_restatement_solves_like_lapack(solved, name):
    d, e = tridiag_cases()[name]
    W, Z, counts, margins, converged = solved[name]
    assert converged and (np.diff(W) >= 0).all()
    check(name, dense(d, e), W, Z, ORACLE_FACTORS)
    _, levels = eig_dc.plan(len(d))
    nodes = [nd for level in levels for nd in level]
    assert len(counts) == len(nodes) and all(k + ndf == nn for (k, ndf), (_, nn, _) in zip(counts, nodes))
    inexact = sum(1 for u in margins if u)                              # the device's counts are compared exactly on the rest
    print("%-28s merges %d, without a margin %d (doubtful tests %d)" % (name, len(nodes), inexact, sum(margins)))
    assert inexact <= (MAX_INEXACT_GLUED if name == "glued168" else MAX_INEXACT * len(nodes)), margins


def test_restatement_on_special_matrices(solved):
    n = 257
    W, Z, counts, _, _ = solved["toeplitz257"]
    check_toeplitz(W, Z)
    # NOT "nothing deflates": two children of equal size inside a Toeplitz matrix are the same matrix, their eigenvalues tie
    # exactly (dt = 0) and dlaed2's rule rotates every such pair away -- half of such a merge deflates.  Children of different
    # size or at the matrix's edge share nothing: the top merges keep every root
    _, levels = eig_dc.plan(n)
    nodes = [nd for level in levels for nd in level]
    assert all(k == nn or (2 * k == nn and 2 * n1 == nn) for (k, _), (_, nn, n1) in zip(counts, nodes))
    assert [k for k, _ in counts[-3:]] == [128, 129, 257] and sum(2 * k == nn for (k, _), (_, nn, _) in zip(counts, nodes)) > 0
    W = solved["clement200"][0]
    assert np.abs(W - np.arange(-199.0, 200.0, 2.0)).max() <= 200 * EPS * 100
    for name in ("diagonal65", "identity65"):
        d, _ = tridiag_cases()[name]
        W, Z, counts, _, _ = solved[name]
        assert all(k == 0 for k, _ in counts) and np.array_equal(W, np.sort(d))
        assert ((Z == 0) | (Z == 1)).all() and (Z.sum(0) == 1).all() and (Z.sum(1) == 1).all()
    assert solved["zerocut65"][2][-1][0] == 0                                                # the merge at the zero cut


def test_restatement_sign_flip():
    """D T D of a tridiagonal matrix, D = diag(+-1): the same eigenvalues, the vectors times D."""
    (d, e), (_, ef) = tridiag_cases()["signs129"], tridiag_cases()["flipped129"]
    s = flip_signs(129)
    assert np.array_equal(dense(d, ef), dense(d, e) * np.outer(s, s))
    W, Z, _ = eig_dc.solve(d, e)
    Wf, Zf, _ = eig_dc.solve(d, ef)
    tmax = np.abs(dense(d, e)).max()
    print("sign flip (restatement): eigenvalues differ by %.3g ulp of max|T|" % (np.abs(W - Wf).max() / (EPS * tmax)))
    assert np.abs(W - Wf).max() <= SIGN_FLIP_ULP * EPS * tmax
    assert np.abs(np.abs(np.einsum("vi,vi->v", Z, Zf * s)) - 1).max() <= 1e-10          # (simple spectrum: gaps >> eps)


# measured: 0 ulp, on the device and here -- a sign commutes with every rounding, and the solver takes |e| wherever a sign could
# steer it (the split, rho) -- so "a few ulp" is none: the eigenvalues of D T D are those of T bit for bit
SIGN_FLIP_ULP = 0.0


@pytest.mark.parametrize("scale", [2.0 ** -300, 2.0 ** -40, 2.0 ** 40, 2.0 ** 300])
def test_restatement_commutes_with_powers_of_two(solved, scale):
    for name in ("random17", "random129", "glued168", "wilkinson65", "clement200", "zerocut65"):
        d, e = tridiag_cases()[name]
        W1, Z1, c1 = solved[name][:3]
        W, Z, c = eig_dc.solve(d * scale, e * scale)
        assert np.array_equal(W, scale * W1) and np.array_equal(Z, Z1) and c == c1, name


def restated_pipeline(tag, A):
    """sytrd_lower -> solve -> back-transformation of the restatement on a dense matrix, held to the metrics: (W, Z, counts)."""
    D, E, tau, V = eig_dc.sytrd_lower(A)
    W, Z, counts, doubt, converged = eig_dc.solve(D, E, detail=True)
    assert converged
    check(tag, A, W, Z @ eig_dc.q_from_reflectors(V, tau).T, ORACLE_FACTORS)
    return W, Z, counts, doubt


@pytest.mark.parametrize("kind,d", SCALE_MATRICES)
def test_restatement_whole_pipeline_at_every_scale(kind, d):
    """The matrices of the device's scale test: the metrics at every scale, and bit for bit the same vectors at the powers of two.
    (The device's merge counts are not held to the restatement's here, only to themselves across the scales: clusters130 has doubtful
    deflation tests in 10 of its 15 merges, isotropic130 deflates nearly everything at rounding level.)"""
    base = None
    for scale in (1.0,) + POW2_SCALES + (1e-10,):
        W, Z, counts, doubt = restated_pipeline("%s%d x %.3g" % (kind, d, scale), scaled_matrix(kind, d, scale))
        if scale == 1.0:
            base = (W, Z, counts)
            print("%-28s merges %d, without a margin %d (doubtful tests %d)" % ("%s%d" % (kind, d), len(doubt), sum(1 for u in doubt if u), sum(doubt)))
        elif scale != 1e-10:
            assert np.array_equal(W, scale * base[0]) and np.array_equal(Z, base[1]) and counts == base[2], (kind, d, scale)


def dense_cases():
    """name -> dense symmetric matrix: every other matrix the device's whole pipeline is given (tests/test_eig_dc_gpu.py)."""
    cases = dict(singular_cases())
    cases["clement"] = dense(*clement(200))
    cases.update(reduction_inputs())
    return cases


@pytest.mark.parametrize("name", ["rank39", "zerorows", "clement_rotated", "clement", "blocks50+70", "zerorows60", "tridiagonal45"])
def test_restatement_whole_pipeline_on_singular_indefinite_and_zero_input(name):
    A = dense_cases()[name]
    W, _, counts, _ = restated_pipeline(name, A)
    assert (np.diff(W) >= 0).all()
    nodes = [nd for level in eig_dc.plan(A.shape[0])[1] for nd in level]
    assert all(k + ndf == nn for (k, ndf), (_, nn, _) in zip(counts, nodes))
    if name == "rank39":
        assert (np.abs(W) <= 1e-13 * np.abs(W).max()).sum() == 130 - 39
    if name.startswith("clement"):
        assert np.abs(W - np.arange(-199.0, 200.0, 2.0)).max() <= 200 * EPS * 100


# against dsytrd, measured (profiles/r21_eig_dc.txt): D, E, Q T Q^T - A in units of n eps max|A|, Q Q^T - I in units of n eps ("T"), and
# tau and the reflectors in units of n eps ("V": a late column of an ill-scaled matrix is small beside max|A|, and its reflector
# only as good as the column's relative accuracy)
REDUCTION_FACTORS = dict(T=128.0, V=8192.0)            # the device: worst 33.1 (D) and 3020 (reflectors), both at scaled256
REDUCTION_FACTORS_ORACLE = dict(T=8.0, V=1024.0)       # the restatement: worst 2.82 (D, scaled129) and 320 (tau, scaled32)


def reduction_inputs():
    """name -> dense symmetric matrix: input with exact zeros, beside dense input.  Two diagonal blocks reach tau == 0 in the middle of
    the loop (columns 48 and 49 have nothing below the subdiagonal) with ordinary steps before and after; a tridiagonal matrix is tau == 0 at
    every step.  Two zero rows and columns do NOT reach it: when the zero row is the subdiagonal row of a step (alpha = 0, the tail
    not), the reflector's leading 1 mixes it with the others, as in LAPACK -- the case stays as dense input with exact zeros.  It is singular, so its last two columns are
    reduced from rounding noise: their tau and reflectors are nobody's to compare, Q T Q^T = A and Q Q^T = I are."""
    rng = np.random.default_rng(5)
    return {"blocks50+70": block_diagonal(), "zerorows60": zero_rows(), "tridiagonal45": dense(rng.standard_normal(45), rng.standard_normal(44))}


def zero_taus(name, tau):
    """Where the reduction of reduction_inputs()[name] takes the tau == 0 branch (the last step always does)."""
    zero = np.flatnonzero(tau[:-1] == 0)
    return {"blocks50+70": list(zero) == [48, 49], "zerorows60": len(zero) == 0, "tridiagonal45": len(zero) == len(tau) - 1}[name]


def check_reduction(tag, A, D, E, tau, V, factor, against_lapack=True):
    """(D, E, tau, V) in dsytrd's lower storage against scipy's dsytrd (D, E in units of n eps max|A|, tau and the reflectors in
    units of n eps), and Q T Q^T = A, Q Q^T = I in the same units."""
    from scipy.linalg import lapack
    n = A.shape[0]
    c, d_ref, e_ref, tau_ref, info = lapack.dsytrd(A, lower=1)
    assert info == 0
    amax = np.abs(A).max()
    unit = n * EPS * amax
    Q = eig_dc.q_from_reflectors(V, tau)
    figs = dict(D=np.abs(D - d_ref).max() / unit, E=np.abs(E - e_ref).max() / unit, tau=np.abs(tau - tau_ref).max() / (n * EPS),
                V=np.abs(np.tril(V, -2) - np.tril(c, -2)).max() / (n * EPS), QTQ=np.abs(Q @ dense(D, E) @ Q.T - A).max() / unit,
                QQ=np.abs(Q @ Q.T - np.eye(n)).max() / (n * EPS))
    print("%-24s n=%4d  " % (tag, n) + "  ".join("%s %.3g" % kv for kv in figs.items()))
    for k, v in figs.items():
        assert v <= factor["V" if k in ("tau", "V") else "T"] or not (against_lapack or k in ("QTQ", "QQ")), (tag, k, v)
    return figs


@pytest.mark.parametrize("n", [3, 4, 5, 31, 32, 33, 64, 129])
def test_restatement_reduces_like_dsytrd(n):
    A = _sytrd_matrix("scaled", n)
    check_reduction("scaled%d" % n, A, *eig_dc.sytrd_lower(A), REDUCTION_FACTORS_ORACLE)


@pytest.mark.parametrize("name", list(reduction_inputs()))
def test_restatement_reduces_through_zero_tau(name):
    A = reduction_inputs()[name]
    D, E, tau, V = eig_dc.sytrd_lower(A)
    assert zero_taus(name, tau)
    check_reduction(name, A, D, E, tau, V, REDUCTION_FACTORS_ORACLE, against_lapack=name != "zerorows60")
