"""eig_mode "sytrd" on the device, stage by stage and from 2^-300 to 2^300 times the matrix: the whole pipeline (ptmi_eig_sytrd_from),
the tridiagonal divide-and-conquer solver on its own (ptmi_eig_dc_tridiag: csrc/ptmi_dc.inc.h without the back-transformation) and
the Householder reduction on its own (ptmi_eig_sytrd_reduction: sytrd_lds_kernel's output).  The references are LAPACK --
numpy.linalg.eigh and scipy's dsytrd on the same matrix -- and, for the decisions of every merge, the CPU restatement
oracle/eig_dc.py.  Matrices, metrics and bounds: tests/test_eig_dc.py, which holds the restatement to the same.  Every order is 300
or less; one engine per order serves all its matrices; after every call the convergence word must be 0."""
import ctypes as C

import numpy as np
import pytest

import test_eig_dc as T
from oracle import eig_dc
from test_eig_jacobi import _sytrd_matrix
from test_gpu_parity import mods  # noqa: F401  (mods is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(mods):
    """engine(n): the handle of order n (pooled covariance, nothing stepped), made once."""
    made = {}

    def get(n):
        if n not in made:
            g = mods[2](n, 2, 2, np.eye(n) * 0.01, weights=(20, 0, 0), cov_update=100, burn=1000, tskip=10, seed=1, cov_mode="pooled",
                        use_de_buffer=False)
            g.init_state(np.zeros(n))
            made[n] = g
        return made[n]

    return get


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _info_is_zero(mods, g):
    import torch
    g.sync()
    torch.cuda.synchronize()
    v = C.c_int32(-1)
    mods[1].check(g.lib.ptmi_eig_sytrd_info(g.h, C.byref(v)))
    assert v.value == 0


def tridiag(mods, g, d, e):
    """ptmi_eig_dc_tridiag: (W, Z, counts) with counts [(k, ndefl)] in the plan's order."""
    import torch
    n = len(d)
    nnodes = sum(len(level) for level in eig_dc.plan(n)[1])
    dd, ee = _dev(d, np.float64), _dev(np.concatenate([e, [0.0]]), np.float64)
    W, Z = torch.full((n,), np.nan, dtype=torch.float64, device="cuda"), torch.full((n, n), np.nan, dtype=torch.float64, device="cuda")
    cnt = torch.full((2 * nnodes + 2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mods[1].check(g.lib.ptmi_eig_dc_tridiag(g.h, None, dd.data_ptr(), ee.data_ptr(), W.data_ptr(), Z.data_ptr(), cnt.data_ptr()))
    _info_is_zero(mods, g)
    c = cnt.cpu().numpy()
    assert (c[2 * nnodes:] == -7).all()                                  # nothing written past the plan's merges
    return W.cpu().numpy(), Z.cpu().numpy(), [(int(c[2 * i]), int(c[2 * i + 1])) for i in range(nnodes)]


def factorize(mods, g, A):
    """ptmi_eig_sytrd_from on the caller's matrix: (Ut, S)."""
    import torch
    n = A.shape[0]
    cov = _dev(A, np.float64)
    Ut, S = torch.full((n, n), np.nan, dtype=torch.float64, device="cuda"), torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mods[1].check(g.lib.ptmi_eig_sytrd_from(g.h, None, cov.data_ptr(), Ut.data_ptr(), S.data_ptr()))
    _info_is_zero(mods, g)
    return Ut.cpu().numpy(), S.cpu().numpy()


def reduction(mods, g):
    """ptmi_eig_sytrd_reduction after a factorization: (D, E, tau, V), V[i, m] the reflectors in dsytrd's lower storage."""
    import torch
    n = g.d
    D, E, tau = (torch.full((m,), np.nan, dtype=torch.float64, device="cuda") for m in (n, n - 1, n - 1))
    A = torch.full((n, n), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mods[1].check(g.lib.ptmi_eig_sytrd_reduction(g.h, None, D.data_ptr(), E.data_ptr(), tau.data_ptr(), A.data_ptr()))
    g.sync()
    torch.cuda.synchronize()
    return D.cpu().numpy(), E.cpu().numpy(), tau.cpu().numpy(), np.ascontiguousarray(A.cpu().numpy().T)


def signed(A, Ut, S):
    """S holds absolute values: the sign of every eigenvalue from its vector's Rayleigh quotient."""
    return np.sign(np.einsum("ki,ij,kj->k", Ut, A, Ut)) * S


def same_counts(name, got, want, doubt):
    """The device's (k, ndefl) of every merge against the restatement's: equal where the restatement's deflation tests all have a
    margin, within the number of its doubtful tests (at most T.MAX_ALLOWANCE) elsewhere."""
    inexact = sum(1 for u in doubt if u)
    print("%-28s merges %d, compared exactly %d, within the doubtful tests %d" % (name, len(want), len(want) - inexact, inexact))
    assert len(got) == len(want)
    for i, (g_, w_, u) in enumerate(zip(got, want, doubt)):
        if u:
            print("%-28s merge %d: k %d against %d, doubtful tests %d" % (name, i, g_[0], w_[0], u))
        assert g_ == w_ if u == 0 else abs(g_[0] - w_[0]) <= min(u, T.MAX_ALLOWANCE), (name, i, g_, w_, u)


@pytest.mark.parametrize("kind,d", T.SCALE_MATRICES)
def test_whole_pipeline_at_every_scale(mods, engine, kind, d):
    """2^-300 ... 2^300 (and 1e-10) times a covariance: the metrics relative to max|A| at every scale; at the powers of two the same
    Ut, that power of two times S and the same merge counts, bit for bit.  With the deflation tolerance that does not scale with the
    matrix (before this test) the residual was 1e-6 ... 3e-4 at 2^-40 and 1e-3 ... 0.13 from 2^-100 down, with orthogonality at
    2e-15 throughout (profiles/r21_eig_dc.txt)."""
    g = engine(d)
    base = None
    for scale in (1.0,) + tuple(s for s in T.SCALES if s != 1.0):
        A = T.scaled_matrix(kind, d, scale)
        Ut, S = factorize(mods, g, A)
        D, E, _, _ = reduction(mods, g)
        counts = tridiag(mods, g, D, E)[2]
        assert (np.diff(S) <= 0).all() and all(k + ndf == nn for (k, ndf), nn in zip(counts, [nd[1] for lv in eig_dc.plan(d)[1] for nd in lv]))
        w = signed(A, Ut, S)
        T.check("%s%d x %.3g" % (kind, d, scale), A, w, Ut, T.DEVICE_FACTORS, by_size=True)
        assert np.abs((Ut.T * w) @ Ut - A).max() <= T.CEILING * np.abs(A).max()
        if scale == 1.0:
            base = (Ut, S, counts)
        elif scale in T.POW2_SCALES:
            assert np.array_equal(Ut, base[0]), (kind, d, scale, np.abs(Ut - base[0]).max())
            assert np.array_equal(S, scale * base[1]), (kind, d, scale)
            assert counts == base[2], (kind, d, scale)


@pytest.fixture(scope="module")
def restated():
    return {name: eig_dc.solve(d, e, detail=True) for name, (d, e) in T.tridiag_cases().items()}


@pytest.mark.parametrize("name", list(T.tridiag_cases()))
def test_tridiagonal_solver_alone(mods, engine, restated, name):
    """ptmi_eig_dc_tridiag against eigh of the same matrix (the metrics) and against the restatement (eigenvalues, the counts of
    every merge); what each special matrix is there for."""
    d, e = T.tridiag_cases()[name]
    n = len(d)
    W, Z, counts = tridiag(mods, engine(n), d, e)
    A = T.dense(d, e)
    assert (np.diff(W) >= 0).all()
    T.check(name, A, W, Z, T.DEVICE_FACTORS)
    oW, _, ocounts, doubt, _ = restated[name]
    nodes = [nd for level in eig_dc.plan(n)[1] for nd in level]
    assert len(counts) == len(nodes) and all(k + ndf == nn for (k, ndf), (_, nn, _) in zip(counts, nodes))
    same_counts(name, counts, ocounts, doubt)
    amax = np.abs(A).max()
    both = min(T.DEVICE_FACTORS["eigenvalues"] + T.ORACLE_FACTORS["eigenvalues"], T.CEILING / (n * T.EPS))
    assert np.abs(W - oW).max() <= both * n * T.EPS * amax                # each within its bound of eigh's
    if name == "toeplitz257":
        T.check_toeplitz(W, Z)
    if name == "clement200":
        assert np.abs(W - np.arange(-199.0, 200.0, 2.0)).max() <= 200 * T.EPS * 100
    if name in ("zerocut65", "diagonal65", "identity65"):
        assert counts[-1][0] == 0                                          # nothing couples the halves of the top merge
    if name in ("diagonal65", "identity65"):
        assert all(k == 0 for k, _ in counts) and np.array_equal(W, np.sort(d))
        assert ((Z == 0) | (Z == 1)).all() and (Z.sum(0) == 1).all() and (Z.sum(1) == 1).all()      # a permutation matrix


def test_tridiagonal_solver_sign_flip(mods, engine):
    """D T D with D = diag(+-1): the same eigenvalues to a few ulp of max|T|, the vectors times D."""
    (d, e), (_, ef) = T.tridiag_cases()["signs129"], T.tridiag_cases()["flipped129"]
    s = T.flip_signs(129)
    g = engine(129)
    W, Z, _ = tridiag(mods, g, d, e)
    Wf, Zf, _ = tridiag(mods, g, d, ef)
    tmax = np.abs(T.dense(d, e)).max()
    print("sign flip (device): eigenvalues differ by %.3g ulp of max|T|" % (np.abs(W - Wf).max() / (T.EPS * tmax)))
    assert np.abs(W - Wf).max() <= T.SIGN_FLIP_ULP * T.EPS * tmax
    assert np.abs(np.abs(np.einsum("vi,vi->v", Z, Zf * s)) - 1).max() <= 1e-10


def _nb():
    """Blocks of sytrd_lds_kernel for n <= 16 CUs / 4 (the rule of ptmi_eig_sytrd_from): a quarter of the CUs, at most n."""
    import torch
    return max(torch.cuda.get_device_properties(0).multi_processor_count // 4, 1)


ORDERS = {"3": lambda nb: 3, "4": lambda nb: 4, "5": lambda nb: 5, "nb-1": lambda nb: nb - 1, "nb": lambda nb: nb, "nb+1": lambda nb: nb + 1,
          "4*nb": lambda nb: 4 * nb, "4*nb+1": lambda nb: 4 * nb + 1}


@pytest.mark.parametrize("order", list(ORDERS))
def test_reduction_alone_on_dense_input(mods, engine, order):
    """sytrd_lds_kernel's (D, E, tau, reflectors) against dsytrd and Q T Q^T = A with Q from the device's reflectors: one column per
    block (n <= nb), a block with one more column than the rest (nb + 1, 4 nb + 1), four columns a block and the fifth, the first
    that falls to a wave's second accumulator."""
    nb = _nb()
    n = ORDERS[order](nb)
    if not 3 <= n <= 300:
        pytest.skip("order %d on a device of %d CUs" % (n, 4 * nb))
    g = engine(n)
    A = _sytrd_matrix("scaled", n)
    factorize(mods, g, A)
    T.check_reduction("device scaled%d (%s)" % (n, order), A, *reduction(mods, g), T.REDUCTION_FACTORS)


@pytest.mark.parametrize("name", list(T.reduction_inputs()))
def test_reduction_alone_through_zero_tau(mods, engine, name):
    """Exact zeros in the input: tau == 0 in the middle of the loop (the sy_fetch branch) with ordinary steps around it."""
    A = T.reduction_inputs()[name]
    g = engine(A.shape[0])
    Ut, S = factorize(mods, g, A)
    D, E, tau, V = reduction(mods, g)
    assert T.zero_taus(name, tau)
    T.check_reduction("device " + name, A, D, E, tau, V, T.REDUCTION_FACTORS, against_lapack=name != "zerorows60")
    T.check("device " + name, A, signed(A, Ut, S), Ut, T.DEVICE_FACTORS, by_size=True)


def test_reduction_needs_a_factorization(mods):
    import torch
    g = mods[2](5, 2, 2, np.eye(5) * 0.01, weights=(20, 0, 0), cov_update=100, burn=1000, tskip=10, seed=1, cov_mode="pooled", use_de_buffer=False)
    buf = torch.zeros(25, dtype=torch.float64, device="cuda")
    assert g.lib.ptmi_eig_sytrd_reduction(g.h, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr()) == -1      # PTMI_EINVAL
    assert g.lib.ptmi_eig_dc_tridiag(g.h, None, None, None, None, None, None) == -1


@pytest.mark.parametrize("name", ["rank39", "zerorows", "clement_rotated", "clement"])
def test_whole_pipeline_on_singular_and_indefinite_input(mods, engine, name):
    """Ut^T diag(+-S) Ut = A with the signs from the Rayleigh quotients, the residual of every pair, orthonormal rows, S not
    increasing -- where the test of the positive definite case skips the reconstruction."""
    A = T.dense_cases()[name]                                            # (clement: +-199 ... +-1, ties in absolute value for eig_sort_rows_kernel)
    Ut, S = factorize(mods, engine(A.shape[0]), A)
    w = signed(A, Ut, S)
    if name == "rank39":
        w = np.where(S <= 1e-13 * S[0], S, w)                              # (the sign of a zero eigenvalue is nobody's)
    assert (np.diff(S) <= 0).all() and (S >= 0).all()
    T.check(name, A, w, Ut, T.DEVICE_FACTORS, by_size=True)
    rec = np.abs((Ut.T * w) @ Ut - A).max() / np.abs(A).max()
    print("%-28s reconstruction %.2e" % (name, rec))
    assert rec <= T.CEILING
    if name.startswith("clement"):
        assert np.abs(S - np.repeat(np.arange(199.0, 0.0, -2.0), 2)).max() <= 200 * T.EPS * 100
        assert (w[0::2] * w[1::2] < 0).all()                               # each tied pair is one +, one -
