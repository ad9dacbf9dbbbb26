"""Log-evidence from the ladder (csrc/ptmi_ev.hip, include/ptmi.h ptmi_ev_attach / ptmi_ev_update; ``PTEngine.with_stages(evidence=True)``,
``PTSampler.log_evidence``, ``ptmcmcsampler_amd/evidence.py``) -- what can be checked without a GPU: the accumulation rule restated in NumPy
(``ev_rule``, which tests/test_evidence_gpu.py holds the device to, bit for bit) against plain means, variances and log-sum-exps; the
estimators on the EXACT moments of a Gaussian in a box, where the trapezoid's bias and the payoff of its correction are known numbers;
per-walker values and standard errors on a hand-made case; the C ABI; the refusals that fall before a library is loaded; and the new
unit's code object."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_ev_attach", "ptmi_ev_update")
LNZ_BOX = -5.53459                                                     # iso Gaussian -|x|^2 / 2, flat prior on [-5, 5]^4: 4 ln(sqrt(2 pi) erf(5 / sqrt 2) / 10)


def ev_rule(lnl_seq, dbeta, state=None):
    """The contract of ptmi_ev_update, restated cell by cell: ``lnl_seq [n][W][T]`` -- lnL BY RANK at each of n calls -- and ``dbeta [T]`` ->
    ``(acc [5][W][T], cnt [2][W][T])``: planes shift, s1, s2, m, es and taken, skipped.  Every operation is one IEEE double operation;
    the exponential is the oracle's (the one the device's is held to bit for bit).  ``state``: (acc, cnt) to continue from."""
    from oracle import oracle as orc
    exp = orc.lib().orc_exp
    lnl_seq = np.asarray(lnl_seq, dtype=np.float64)
    dbeta = np.asarray(dbeta, dtype=np.float64)
    n, W, T = lnl_seq.shape
    acc, cnt = (np.zeros((5, W, T)), np.zeros((2, W, T), dtype=np.uint64)) if state is None else (state[0].copy(), state[1].copy())
    with np.errstate(all="ignore"):
        for k in range(n):
            for w in range(W):
                for r in range(T):
                    l = lnl_seq[k, w, r]
                    if not np.isfinite(l):
                        cnt[1, w, r] += np.uint64(1)
                        continue
                    a = dbeta[r] * l
                    if cnt[0, w, r] == 0:
                        acc[:, w, r] = (l, 0.0, 0.0, a, 1.0)
                    else:
                        t = l - acc[0, w, r]
                        acc[1, w, r] = acc[1, w, r] + t
                        acc[2, w, r] = acc[2, w, r] + t * t
                        m, es = acc[3, w, r], acc[4, w, r]
                        if a <= m:
                            acc[4, w, r] = es + np.float64(exp(float(a - m)))
                        else:
                            acc[4, w, r] = es * np.float64(exp(float(m - a))) + 1.0
                            acc[3, w, r] = a
                    cnt[0, w, r] += np.uint64(1)
    return acc, cnt


def box_moments(betas, d=4, a=5.0):
    """Exact ln Z(beta), mean and variance of lnL = -|x|^2 / 2 under exp(beta lnL) on [-a, a]^d, by composite Gauss-Legendre quadrature
    (16 nodes on each of 800 panels: 0.4 standard deviations of the narrowest Gaussian here, beta = 1024, per panel)."""
    x0, w0 = np.polynomial.legendre.leggauss(16)
    edges = np.linspace(-a, a, 801)
    h = (edges[1:] - edges[:-1]) / 2
    x = (edges[:-1, None] + h[:, None] * (x0[None, :] + 1)).ravel()
    w = (h[:, None] * w0[None, :]).ravel()
    lnZ, mean, var = [], [], []
    for b in np.asarray(betas, dtype=np.float64):
        f = np.exp(-0.5 * b * x * x) * w
        z = f.sum()
        e2, e4 = (f * x ** 2).sum() / z, (f * x ** 4).sum() / z
        lnZ.append(d * np.log(z / (2 * a)))
        mean.append(-0.5 * d * e2)
        var.append(0.25 * d * (e4 - e2 * e2))
    return np.array(lnZ), np.array(mean), np.array(var)


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
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_ev_\w+)\(([^;]*)\);", hdr)}
    assert decl == {"ptmi_ev_attach": "ptmi_handle h, double *acc , uint64_t *cnt , const double *dbeta", "ptmi_ev_update": "ptmi_handle h"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS and s in exported, s
    H = C.c_void_p
    assert L.ptmi_ev_attach.argtypes == [H, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    assert L.ptmi_ev_update.argtypes == [H]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_ev.hip" for src in _build.deps())
    assert re.search(r'"ptmi_ev\.hip"\), os\.path\.join\(OBJ, "ev\.o"\)', inspect.getsource(_build.build))


def test_the_rule_against_plain_moments():
    rs = np.random.RandomState(11)
    n, W, T = 200, 2, 4
    dbeta = np.array([0.0, 0.5, 0.25, 0.125])
    for centre, spread in ((0.0, 3.0), (-1.0e7, 2.0), (4.0e9, 50.0)):      # |lnL| far above its spread: what the shift is for
        seq = centre + spread * rs.randn(n, W, T)
        acc, cnt = ev_rule(seq, dbeta)
        assert (cnt[0] == n).all() and not cnt[1].any()
        assert np.array_equal(acc[0], seq[0])                            # the shift is the first sample
        mean = acc[0] + acc[1] / n
        var = (acc[2] - acc[1] ** 2 / n) / n
        assert np.allclose(mean, seq.mean(0), rtol=1e-12, atol=0)
        assert np.allclose(var, seq.var(0), rtol=1e-12, atol=0)
        a = dbeta[None, None, :] * seq
        top = a.max(0)
        assert np.array_equal(acc[3], top)                               # m is the largest exponent so far
        assert np.allclose(acc[3] + np.log(acc[4]), top + np.log(np.exp(a - top).sum(0)), rtol=1e-12, atol=1e-12)
    # moderate values: against the textbook expression itself
    seq = 2.0 * rs.randn(n, W, T)
    acc, cnt = ev_rule(seq, dbeta)
    assert np.allclose(acc[3] + np.log(acc[4]), np.log(np.exp(dbeta * seq).sum(0)), rtol=1e-12, atol=1e-12)
    assert np.array_equal(acc[4][:, 0], np.full(W, float(n))) and not acc[3][:, 0].any()      # dbeta = 0: es counts, m = 0
    # continuing from a state is the same recurrence
    half = ev_rule(seq[:77], dbeta)
    both = ev_rule(seq[77:], dbeta, half)
    assert np.array_equal(both[0], acc) and np.array_equal(both[1], cnt)


def test_the_rule_skips_what_is_not_finite_and_survives_the_extremes():
    dbeta = np.array([0.0, 1.0, 1e-300])
    seq = np.array([[[np.nan, -np.inf, np.inf]],                        # skipped before the first sample
                    [[1.0, -2.0, 1e300]],                                # first samples
                    [[np.inf, -800.0, -1e300]],                          # a - m = -798 < -745.13: the exponential is 0
                    [[2.0, 900.0, np.nan]],                              # a rises by 1700: es * 0 + 1
                    [[2.0, 900.0, 1e300]]])                              # equal values: es += 1
    acc, cnt = ev_rule(seq, dbeta)
    assert cnt[0, 0].tolist() == [3, 4, 3] and cnt[1, 0].tolist() == [2, 1, 2] and (cnt.sum(0) == 5).all()
    assert acc[0, 0].tolist() == [1.0, -2.0, 1e300]
    assert acc[3, 0].tolist() == [0.0, 900.0, 1e-300 * 1e300] and acc[4, 0, :2].tolist() == [3.0, 2.0]
    assert np.isclose(acc[4, 0, 2], 2.0 + np.exp(-2.0), rtol=1e-14)
    assert acc[1, 0, 1] == 2 * 902.0 - 798.0 and acc[2, 0, 1] == 2 * 902.0 ** 2 + 798.0 ** 2
    assert np.isfinite(acc[1, 0, 2]) and acc[2, 0, 2] == np.inf          # (2e300)^2: the rule does not hide an overflow


def test_estimates_on_the_exact_moments_of_a_gaussian_in_a_box():
    from ptmcmcsampler_amd import evidence
    temps = np.concatenate([2.0 ** np.arange(11), [1e80]])             # ladder 2^k, k = 0 .. 10, and the hot rank
    betas = 1.0 / temps
    lnZ, mean, var = box_moments(betas)
    assert abs(lnZ[0] - LNZ_BOX) < 1e-5 and abs(lnZ[-1]) < 1e-12
    n = 1.0e6
    T = len(betas)
    one = lambda v: np.asarray(v, dtype=np.float64).reshape(1, T)      # noqa: E731
    # stepping stones: sum exp(dbeta_r lnL) over n samples at rank r is n Z(beta_{r-1}) / Z(beta_r)
    ratio = np.concatenate([[0.0], lnZ[:-1] - lnZ[1:]])
    est = evidence.estimates(betas, one(np.full(T, n)), one(mean), one(np.zeros(T)), one(n * var), one(ratio), one(np.full(T, n)))
    assert sorted(est) == sorted(evidence.KEYS)
    assert np.allclose(est["mean"], mean, rtol=1e-14) and np.allclose(est["var"], var, rtol=1e-14)
    assert abs(est["lnZ_ti"] - (-5.7386)) < 1e-3 and abs(est["lnZ_ti_corrected"] - (-5.5240)) < 1e-3
    assert abs(est["lnZ_ti"] - LNZ_BOX - (-0.204)) < 1e-3 and abs(est["lnZ_ti_corrected"] - LNZ_BOX - 0.011) < 1e-3
    assert abs(est["lnZ_ss"] - (lnZ[0] - lnZ[-1])) < 1e-10 and abs(est["lnZ_ss"] - LNZ_BOX) < 1e-5
    assert est["beta_min"] == 1e-80
    for k in ("lnZ_ti", "lnZ_ti_corrected", "lnZ_ss"):                  # one walker: its value is the pooled one, and no standard error
        assert est[k + "_per_walker"].shape == (1,) and abs(est[k + "_per_walker"][0] - est[k]) < 1e-12 and np.isnan(est[k + "_sem"])
    # 16 ranks at step 1.6 (no hot rank: the range below beta_min = 1.6^-15 is left out of all three)
    b16 = 1.6 ** -np.arange(16.0)
    lz, mu, va = box_moments(b16)
    T = 16
    e16 = evidence.estimates(b16, one(np.full(T, n)), one(mu), one(np.zeros(T)), one(n * va),
                             one(np.concatenate([[0.0], lz[:-1] - lz[1:]])), one(np.full(T, n)))
    exact = lz[0] - lz[-1]
    assert abs(e16["lnZ_ti"] - exact - (-0.094)) < 2e-3 and abs(e16["lnZ_ti_corrected"] - exact - 0.002) < 2e-3
    assert abs(e16["lnZ_ss"] - exact) < 1e-10 and e16["beta_min"] == b16[-1]


def test_per_walker_values_standard_errors_and_pooling():
    from ptmcmcsampler_amd import evidence
    rs = np.random.RandomState(5)
    betas = np.array([1.0, 0.5, 0.125])
    dbeta = evidence.dbeta_of(1.0 / betas)
    assert dbeta.tolist() == [0.0, 0.5, 0.375]
    W, T = 3, 3
    counts = (40, 25, 60)
    seqs = [rs.randn(c, T) * (1.0 + np.arange(T)) - 3.0 * np.arange(T) - 10.0 * w for w, c in enumerate(counts)]      # walkers differ
    planes = [ev_rule(s[:, None, :], dbeta) for s in seqs]
    acc = np.concatenate([p[0] for p in planes], axis=1)
    n = np.concatenate([p[1][0] for p in planes], axis=0)
    est = evidence.estimates(betas, n, *acc)
    allrows = np.concatenate(seqs)
    assert np.allclose(est["mean"], allrows.mean(0), rtol=1e-12) and np.allclose(est["var"], allrows.var(0), rtol=1e-12)      # Chan's combination
    D = betas[:-1] - betas[1:]
    for k, name in enumerate(("lnZ_ti", "lnZ_ti_corrected", "lnZ_ss")):
        per = []
        for s in seqs + [allrows]:
            mu, va = s.mean(0), s.var(0)
            ti = sum(D[r] * (mu[r] + mu[r + 1]) / 2 for r in range(T - 1))
            tic = ti - sum(D[r] ** 2 * (va[r] - va[r + 1]) / 12 for r in range(T - 1))
            ss = sum(np.log(np.mean(np.exp(dbeta[r] * s[:, r]))) for r in range(1, T))
            per.append((ti, tic, ss)[k])
        assert np.allclose(est[name + "_per_walker"], per[:W], rtol=1e-11)
        assert np.isclose(est[name], per[W], rtol=1e-11)
        assert np.isclose(est[name + "_sem"], np.std(per[:W], ddof=1) / np.sqrt(W), rtol=1e-9)
    # one walker: NaN standard errors; a rank without samples: NaN values, no exception
    e1 = evidence.estimates(betas, n[:1], *acc[:, :1])
    assert all(np.isnan(e1[k + "_sem"]) for k in ("lnZ_ti", "lnZ_ti_corrected", "lnZ_ss")) and np.isfinite(e1["lnZ_ss"])
    n0 = n.copy()
    n0[:, 1] = 0
    assert np.isnan(evidence.estimates(betas, n0, *acc)["lnZ_ti"])
    for bad in (betas[::-1], np.array([1.0, 0.5]), np.array([1.0, 0.5, 0.5])):
        with pytest.raises(ValueError, match="betas"):
            evidence.estimates(bad, n, *acc)


def test_the_module_needs_neither_torch_nor_a_gpu():
    code = ("import sys; import ptmcmcsampler_amd.evidence as e; "
            "assert 'torch' not in sys.modules and 'ptmcmcsampler_amd.engine' not in sys.modules; print(len(e.KEYS))")
    out = subprocess.check_output([os.sys.executable, "-c", code], cwd=ROOT, text=True)
    assert out.strip() == "12"


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTSampler.log_evidence is False and PTSampler.evidence is None
    assert _sampler(tmp_path, "default").log_evidence is False
    sig = inspect.signature(PTEngine.with_stages).parameters
    for name, default in (("evidence", False), ("evidence_from", None), ("evidence_every", 1)):
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert name not in inspect.signature(PTEngine.__init__).parameters
    for name in ("evidence", "log_evidence"):
        assert name not in inspect.signature(PTSampler.__init__).parameters
        assert name not in inspect.signature(PTSampler.sample).parameters
    with pytest.raises(TypeError, match="evidence"):                 # the plain constructors keep their parameters
        PTEngine(6, 2, 1, np.eye(6), evidence=True)
    with pytest.raises(TypeError, match="log_evidence"):
        _sampler(tmp_path, "kw", log_evidence=True)
    s = _sampler(tmp_path, "kw2")
    assert s._evidence_kw() == {}
    s.log_evidence = True
    assert s._evidence_kw() == dict(evidence=True)
    s.log_evidence = {"every": 3}
    assert s._evidence_kw() == dict(evidence=True, evidence_every=3)
    for bad in ({"each": 2}, 3, "yes"):
        s.log_evidence = bad
        with pytest.raises(ValueError, match="log_evidence"):
            s._evidence_kw()


def test_refusals_fall_before_any_library_is_loaded(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    d = 4
    make = lambda nt=3, **kw: PTEngine.with_stages(d, nt, 2, np.eye(d), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="one temperature"):
        make(nt=1, evidence=True)
    with pytest.raises(ValueError, match="tskip"):
        make(evidence=True, tskip=0)
    with pytest.raises(ValueError, match="evidence_from"):
        make(evidence=True, evidence_from=-1)
    for every in (0, -2, 1.5):
        with pytest.raises(ValueError, match="evidence_every"):
            make(evidence=True, evidence_every=every)
    with pytest.raises(ValueError, match="evidence=True"):
        make(evidence_from=5)
    with pytest.raises(ValueError, match="evidence=True"):
        make(evidence_every=2)
    for kw in (dict(ntemps_global=6), dict(ntemps_global=6, temp0=3)):      # a block of a sharded ladder: dbeta[0] is not the engine's to know
        with pytest.raises(ValueError, match="sharded ladder"):
            make(evidence=True, **kw)
    # a good request: the constructor gets as far as loading the library
    for kw in (dict(evidence=True), dict(evidence=True, evidence_from=0, evidence_every=4), dict(nt=2, evidence=True, tskip=1)):
        with pytest.raises(AssertionError, match="library was loaded"):
            make(**kw)


def test_a_replayed_resume_names_the_checkpoint(tmp_path):
    s = _sampler(tmp_path, "replay", resume=True, checkpoint=False)
    os.makedirs(s.outDir, exist_ok=True)
    np.savetxt(os.path.join(s.outDir, "chain_1.txt"), np.zeros((1, 3 + 4)))      # a chain file and no device checkpoint
    s.log_evidence = True
    with pytest.raises(NotImplementedError, match="checkpoint=True"):
        s.sample(np.zeros(3), 10, isave=10, thin=1)


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "ptmi_ev.s")
    cmd = [_build.hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_ev.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def test_the_unit_compiles_for_gfx950_without_scratch_lds_or_atomics(unit_asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    assert len(kernels) == 1 and "ev_update_kernel" in kernels[0][0], [k for k, _ in kernels]
    name, desc = kernels[0]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)) == 0
    spills = re.findall(r"\.(sgpr|vgpr)_spill_count:\s*(\d+)", unit_asm)
    assert len(spills) == 2 and all(int(v) == 0 for _, v in spills), spills
    body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), unit_asm, re.S | re.M).group(1)
    assert "_atomic_" not in body and "ds_" not in body               # a cell has one owner: plain loads and stores
    # every operation rounds on its own: the only fused multiply-adds are the correctly rounded division inside det_exp
    # (v_div_scale .. v_div_fixup, the sequence the compiler emits for one IEEE division)
    assert len(re.findall(r"v_div_fixup_f64", body)) == 1
    outside = re.sub(r"v_div_scale_f64.*?v_div_fixup_f64", "", body, flags=re.S)
    assert "v_fma_f64" not in outside and "v_fmac_f64" not in outside
    assert "v_mul_f64" in outside and "v_add_f64" in outside
