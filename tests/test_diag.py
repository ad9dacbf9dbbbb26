"""Convergence diagnostics of every cold chain -- R-hat and ESS from streaming sums accumulated on the device (csrc/ptmi_diag.hip,
include/ptmi.h ptmi_diag_attach / ptmi_diag_update; ``PTEngine.with_stages(diag=True)``, ``PTSampler.chain_diagnostics``,
ptmcmcsampler_amd/diagnostics.py) -- what can be checked without a GPU: the accumulation rule restated in NumPy (``diag_rule``, what
tests/test_diag_gpu.py holds the device to, bit for bit) against brute force, the estimators on series with known autocorrelation
time, degenerate inputs, the refusals of the Python surface before a library is loaded, the C ABI's two entry points, and the new
unit cross-compiled for gfx950 into a kernel without scratch."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_diag_attach", "ptmi_diag_update")


def diag_rule(X, b0, L, state=None):
    """The contract, restated one iteration at a time: ``X [W][n][d]`` folded into ``state`` (None: a fresh one) -> the new state, a
    dict of ``c``, ``S1``, ``S2``, ``A`` [W][d], ``Q`` [L][W][d], ``H`` [L - 1][W][d], ``n``, ``batch0``.  Every operation is one NumPy call:
    rounded on its own, as the device rounds it."""
    X = np.asarray(X, dtype=np.float64)
    W, nx, d = X.shape
    if state is None:
        st = dict(c=np.zeros((W, d)), S1=np.zeros((W, d)), S2=np.zeros((W, d)), A=np.zeros((W, d)), Q=np.zeros((L, W, d)),
                  H=np.zeros((max(L - 1, 0), W, d)), n=0, batch0=int(b0))
    else:
        st = {k: (np.array(v, dtype=np.float64) if k not in ("n", "batch0") else int(v)) for k, v in state.items()
              if k in ("c", "S1", "S2", "A", "Q", "H", "n", "batch0")}
        assert st["batch0"] == b0 and st["Q"].shape[0] == L
    c, S1, S2, A, Q, H, n = st["c"], st["S1"], st["S2"], st["A"], st["Q"], st["H"], st["n"]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nx):
            x = X[:, i]
            if n == 0:
                c = x.copy()
            y = x - c
            S1 = S1 + y
            S2 = S2 + y * y
            A = A + y
            n += 1
            if n % b0 == 0:
                k = n // b0
                t = A
                A = np.zeros((W, d))
                for l in range(L):
                    Q[l] = Q[l] + t * t
                    if l == L - 1:
                        break
                    if (k >> l) & 1:
                        H[l] = t
                        break
                    t = H[l] + t
    st.update(c=c, S1=S1, S2=S2, A=A, Q=Q, H=H, n=n)
    return st


def assert_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    bad = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), "%s: %d of %d differ" % (what, bad.sum(), bad.size)


def assert_state_bits(a, b, what=""):
    assert a["n"] == b["n"] and a["batch0"] == b["batch0"], what
    for k in ("c", "S1", "S2", "A", "Q", "H"):
        assert_bits(a[k], b[k], "%s %s" % (what, k))


def test_binary_counter_against_brute_force():
    from ptmcmcsampler_amd.diagnostics import batch_total
    rs = np.random.RandomState(0)
    W, d = 2, 3
    X = rs.randn(W, 70, d) + 5.0
    for b0 in (1, 3):
        for L in (1, 2, 4):
            for n in range(1, 71):
                st = diag_rule(X[:, :n], b0, L)
                y = X[:, :n] - X[:, :1]
                k = n // b0
                assert st["n"] == n
                np.testing.assert_allclose(st["S1"], y.sum(1), rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(st["S2"], (y * y).sum(1), rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(st["A"], y[:, k * b0:].sum(1), rtol=1e-12, atol=1e-12)
                for l in range(L):
                    b, m = b0 << l, k >> l
                    sums = y[:, :m * b].reshape(W, m, b, d).sum(2)                    # the completed level-l batches
                    np.testing.assert_allclose(st["Q"][l], (sums * sums).sum(1), rtol=1e-12, atol=1e-300, err_msg="Q[%d] n=%d b0=%d L=%d" % (l, n, b0, L))
                    T = batch_total(st["S1"], st["A"], st["H"], k, l)
                    np.testing.assert_allclose(T, sums.sum(1), rtol=1e-12, atol=1e-11, err_msg="T[%d] n=%d b0=%d L=%d" % (l, n, b0, L))
            whole = diag_rule(X, b0, L)
            for cut in range(0, 71):                                     # two calls split at any point: one call, bit for bit
                two = diag_rule(X[:, cut:], b0, L, diag_rule(X[:, :cut], b0, L))
                assert_state_bits(two, whole, "cut %d b0 %d L %d" % (cut, b0, L))


def ar1(W, n, phi, seed, d=1, offset=5.0):
    """Stationary AR(1) series x_t = phi x_{t-1} + eps with unit innovations, plus a constant: [W][n][d]."""
    rs = np.random.RandomState(seed)
    x = np.empty((W, n, d))
    x[:, 0] = rs.randn(W, d) / np.sqrt(1.0 - phi * phi)
    eps = rs.randn(W, n, d)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + eps[:, t]
    return x + offset


AR1_CASES = [(128, 1536, 0.8, 4, 7), (64, 4096, 0.9, 8, 8), (32, 4096, 0.5, 4, 8)]


@pytest.mark.parametrize("W,n,phi,b0,L", AR1_CASES)
def test_estimators_on_ar1(W, n, phi, b0, L):
    from ptmcmcsampler_amd.diagnostics import estimates
    x = ar1(W, n, phi, seed=int(1000 * phi) + W)
    e = estimates(diag_rule(x, b0, L))
    tau = (1.0 + phi) / (1.0 - phi)
    k = n // b0
    checked = 0
    for l in range(L):
        m, b = k >> l, b0 << l
        if m < 2:
            assert np.isnan(e["tau_batch"][l]).all()
            continue
        assert np.isfinite(e["tau_batch"][l]).all()
        if W * (m - 1) < 256:
            continue
        want = tau - 2.0 * phi * (1.0 - phi ** b) / (b * (1.0 - phi) ** 2)      # E[var of a batch sum] / (b sigma^2)
        se = np.sqrt(2.0 / (W * (m - 1)))
        got = float(e["tau_batch"][l, 0])
        print("level %d b %d m %d: tau_batch %.4f, expected %.4f, %.2f standard errors" % (l, b, m, got, want, (got / want - 1) / se))
        assert abs(got / want - 1.0) <= 5.0 * se, (l, got, want, se)
        checked += 1
        assert int(e["level"]) >= l
    assert checked >= 3 and W * ((k >> int(e["level"])) - 1) >= 256
    assert int(e["level"]) == L - 1 or W * ((k >> (int(e["level"]) + 1)) - 1) < 256
    tw = float(e["tau_walkers"][0])
    print("tau_walkers %.4f, tau %.4f, rhat %.5f" % (tw, tau, float(e["rhat"][0])))
    assert abs(tw / tau - 1.0) <= 5.0 * np.sqrt(2.0 / (W - 1))
    assert float(e["rhat"][0]) < 1.01
    assert float(e["tau"][0]) == max(1.0, float(e["tau_batch"][int(e["level"]), 0]))
    assert float(e["ess"][0]) == W * n / float(e["tau"][0])
    assert bool(e["reliable"][0]) == ((b0 << int(e["level"])) >= 10.0 * float(e["tau"][0]))
    # the moments themselves, against NumPy's own
    np.testing.assert_allclose(e["mean_w"], x.mean(1), rtol=1e-12)
    np.testing.assert_allclose(e["var_w"], x.var(1, ddof=1), rtol=1e-9)
    np.testing.assert_allclose(e["mean"], x.mean((0, 1)), rtol=1e-12)
    np.testing.assert_allclose(e["var"], x.var(1, ddof=1).mean(0), rtol=1e-9)
    assert int(e["n"]) == n and int(e["k"]) == k and int(e["nwalkers"]) == W and not e["nonfinite"].any()


def test_disagreeing_walkers():
    from ptmcmcsampler_amd.diagnostics import converged, estimates
    W, n, phi, b0, L = 128, 1536, 0.8, 4, 7
    x = ar1(W, n, phi, seed=7)
    x[: W // 2] += 1.0 / np.sqrt(1.0 - phi * phi)                     # half the walkers one standard deviation off
    e = estimates(diag_rule(x, b0, L))
    assert float(e["rhat"][0]) > 1.1
    assert np.isfinite(e["tau_batch"][:5]).all()                      # the batch means look along each chain: the shift is nothing to them
    assert not converged(e, stop_rhat=1.05)
    same = estimates(diag_rule(ar1(W, n, phi, seed=7), b0, L))
    np.testing.assert_allclose(e["tau_batch"][:5], same["tau_batch"][:5], rtol=1e-9)      # ... the same values as without it, to rounding


def test_degenerate_inputs():
    from ptmcmcsampler_amd.diagnostics import converged, estimates
    e = estimates(diag_rule(np.full((8, 200, 2), 3.25), 2, 5))
    assert (e["tau"] == 1.0).all() and not e["reliable"].any() and (e["var"] == 0.0).all() and (e["mean"] == 3.25).all()
    assert not converged(e, stop_ess=1) and not converged(e, stop_rhat=2.0) and not converged(e)
    x = ar1(16, 400, 0.5, seed=3, d=2)
    x[5, 17, 1] = np.nan
    st = diag_rule(x, 2, 5)
    e = estimates(st)
    assert e["nonfinite"].tolist() == [0, 1]
    for k in ("mean", "var", "rhat", "tau_walkers", "tau", "ess"):
        assert np.isfinite(e[k]).all(), k
    clean = estimates(diag_rule(np.delete(x, 5, axis=0), 2, 5))        # parameter 1: the estimates of the other fifteen walkers
    for k in ("mean", "var", "rhat", "tau_walkers", "tau", "ess"):
        np.testing.assert_allclose(e[k][1], clean[k][1], rtol=1e-12, err_msg=k)
    assert np.isnan(st["S1"][5, 1]) and np.isfinite(st["S1"][5, 0])   # confined to its own stream
    # too few batches for any level: no tau yet, never reliable; one walker: no rhat
    e = estimates(diag_rule(ar1(4, 20, 0.5, seed=1), 4, 3))
    assert int(e["level"]) == -1 and np.isnan(e["tau"]).all() and not e["reliable"].any() and np.isnan(e["ess"]).all()
    e = estimates(diag_rule(ar1(1, 2000, 0.5, seed=1), 1, 6))
    assert np.isnan(e["rhat"]).all() and np.isnan(e["tau_walkers"]).all() and np.isfinite(e["tau"]).all()


def test_planes_layout():
    from ptmcmcsampler_amd.diagnostics import nplanes, planes
    L, W, d = 4, 2, 3
    acc = np.arange(nplanes(L) * W * d, dtype=np.float64).reshape(nplanes(L), W, d)
    p = planes(acc, L)
    assert nplanes(L) == 11 and [int(p[k][0, 0]) // (W * d) for k in ("c", "S1", "S2", "A")] == [0, 1, 2, 3]
    assert p["Q"].shape == (L, W, d) and p["Q"][0, 0, 0] == 4 * W * d and p["H"].shape == (L - 1, W, d) and p["H"][0, 0, 0] == (4 + L) * W * d
    assert planes(np.zeros((5, W, d)), 1)["H"].shape == (0, W, d)
    with pytest.raises(ValueError, match="planes"):
        planes(acc, 3)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from ptmcmcsampler_amd import _lib
    if not os.path.exists(_lib.SO):
        ge.build()
    return _lib


def test_header_binding_and_library_carry_the_entry_points(lib):
    import ctypes as C
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_diag_\w+)\(([^;]*)\);", hdr)}
    assert decl == {
        "ptmi_diag_attach": "ptmi_handle h, double *acc , int32_t nlevels, int32_t batch0",
        "ptmi_diag_update": "ptmi_handle h, int64_t iter_lo, int64_t iter_hi, int64_t n_done"}
    assert "PTMCMCSampler.py:510-521" in open(os.path.join(ROOT, "include", "ptmi.h")).read()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS, s
        assert s in exported, s
    H = C.c_void_p
    assert L.ptmi_diag_attach.argtypes == [H, C.c_void_p, C.c_int32, C.c_int32]
    assert L.ptmi_diag_update.argtypes == [H, C.c_int64, C.c_int64, C.c_int64]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_diag.hip" for src in _build.deps())
    assert re.search(r'"ptmi_diag\.hip"\), os\.path\.join\(OBJ, "diag\.o"\)', inspect.getsource(_build.build))


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTSampler.chain_diagnostics is False and PTSampler.diagnostics is None
    assert _sampler(tmp_path, "default").chain_diagnostics is False
    sig = inspect.signature(PTEngine.with_stages).parameters
    assert sig["diag"].default is False
    for name in ("diag", "diag_from", "diag_batch", "diag_levels"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert name not in inspect.signature(PTEngine.__init__).parameters
    for name in ("diag", "chain_diagnostics"):
        assert name not in inspect.signature(PTSampler.__init__).parameters
        assert name not in inspect.signature(PTSampler.sample).parameters
    with pytest.raises(TypeError, match="diag"):                     # the plain constructors keep their parameters
        PTEngine(6, 1, 1, np.eye(6), diag=True)
    with pytest.raises(TypeError, match="chain_diagnostics"):
        _sampler(tmp_path, "kw", chain_diagnostics=True)


def test_refusals_fall_before_any_library_is_loaded(monkeypatch, tmp_path):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    d = 4
    make = lambda **kw: PTEngine.with_stages(d, 1, 2, np.eye(d), **kw)      # noqa: E731
    for L in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="diag_levels"):
            make(diag=True, diag_levels=L)
    for b0 in (0, -2, 1.5):
        with pytest.raises(ValueError, match="diag_batch"):
            make(diag=True, diag_batch=b0)
    with pytest.raises(ValueError, match="diag_from"):
        make(diag=True, diag_from=-1)
    for kw in (dict(diag_from=5), dict(diag_batch=2), dict(diag_levels=4)):      # they go with diag=True
        with pytest.raises(ValueError, match="diag=True"):
            make(**kw)
    with pytest.raises(ValueError, match="no cold ring"):             # a block of a sharded ladder without rank 0
        PTEngine.with_stages(d, 2, 2, np.eye(d), ntemps_global=4, temp0=2, diag=True)
    # good arguments: the constructor gets as far as loading the library
    for kw in (dict(diag=True), dict(diag=True, diag_levels=1, diag_batch=7, diag_from=0), dict(diag=True, diag_levels=16)):
        with pytest.raises(AssertionError, match="library was loaded"):
            make(**kw)
    # the sampler's attribute
    for bad in ({"batches": 4}, {"batch": 2, "stop": 1}, "yes", {"stop_rhat": 0.9}, {"stop_ess": 0}):
        s = _sampler(tmp_path, "bad%d" % abs(hash(repr(bad))))
        s.chain_diagnostics = bad
        with pytest.raises(ValueError, match="chain_diagnostics"):
            s.sample(np.zeros(3), 10, isave=10, thin=1)


def test_a_replayed_resume_names_the_checkpoint(tmp_path):
    s = _sampler(tmp_path, "replay", resume=True, checkpoint=False)
    os.makedirs(s.outDir, exist_ok=True)
    np.savetxt(os.path.join(s.outDir, "chain_1.txt"), np.zeros((1, 3 + 4)))      # a chain file and no device checkpoint
    s.chain_diagnostics = True
    with pytest.raises(NotImplementedError, match="checkpoint=True"):
        s.sample(np.zeros(3), 10, isave=10, thin=1)


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "ptmi_diag.s")
    cmd = [_build.hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_diag.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def test_the_unit_compiles_for_gfx950_without_scratch_or_spills(unit_asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    names = [k for k, _ in kernels]
    assert len(names) == 1 and "diag_rows_kernel" in names[0], names
    for name, desc in kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name      # Q / H live in registers
    spills = re.findall(r"\.(sgpr|vgpr)_spill_count:\s*(\d+)", unit_asm)
    assert len(spills) == 2 * len(kernels) and all(int(v) == 0 for _, v in spills), spills
    body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(names[0]), unit_asm, re.S | re.M).group(1)
    assert "v_fma_f64" not in body and "v_fmac_f64" not in body       # every operation rounded on its own
    assert "global_atomic" not in body and "scratch_" not in body    # a stream is one thread's: no atomics, nothing in scratch
