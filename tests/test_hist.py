"""Posterior histograms of every cold chain, accumulated on the device from the AM ring (csrc/ptmi_hist.hip, include/ptmi.h
ptmi_hist_attach / ptmi_hist_update; ``PTEngine.with_stages(hist=(lo, hi, nbins))``, ``PTSampler.posterior_hist``) -- what can be
checked without a GPU: the C ABI carries the two entry points, the Python surface takes the stage as an opt-in and refuses bad bins
before a library is loaded, the binning rule itself on edge values, and the new unit cross-compiles for gfx950 into kernels without
scratch.  The runs themselves: tests/test_hist_gpu.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_hist_attach", "ptmi_hist_update")


def hist_rule(x, lo, hi, nbins, weight=None):
    """The contract, restated: x [..., d] -> uint64 [d][nbins + 2] (bins, under, over).  One subtraction, one multiplication."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[-1]
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (d,)), np.broadcast_to(np.asarray(hi, np.float64), (d,))
    scale = nbins / (hi - lo)
    x = x.reshape(-1, d)
    w = np.ones(x.shape[0], dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64).reshape(-1)
    out = np.zeros((d, nbins + 2), dtype=np.uint64)
    for j in range(d):
        with np.errstate(invalid="ignore"):
            t = (x[:, j] - lo[j]) * scale[j]
            under = ~(t >= 0.0)
            over = ~under & (t >= nbins)
        inside = ~under & ~over
        out[j, :nbins] = np.bincount(t[inside].astype(np.int64), weights=w[inside], minlength=nbins).astype(np.uint64)
        out[j, nbins] = w[under].sum()
        out[j, nbins + 1] = w[over].sum()
    return out


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
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_hist_\w+)\(([^;]*)\);", hdr)}
    assert decl == {
        "ptmi_hist_attach": "ptmi_handle h, uint64_t *counts , const double *lo , const double *scale , int32_t nbins",
        "ptmi_hist_update": "ptmi_handle h, int64_t iter_lo, int64_t iter_hi"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS, s
        assert s in exported, s
    H = C.c_void_p
    assert L.ptmi_hist_attach.argtypes == [H, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32]
    assert L.ptmi_hist_update.argtypes == [H, C.c_int64, C.c_int64]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_hist.hip" for src in _build.deps())
    assert re.search(r'"ptmi_hist\.hip"\), os\.path\.join\(OBJ, "hist\.o"\)', inspect.getsource(_build.build))


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTSampler.posterior_hist is None and PTSampler.hist is None
    assert _sampler(tmp_path, "default").posterior_hist is None
    sig = inspect.signature(PTEngine.with_stages).parameters
    for name in ("hist", "hist_from"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert name not in inspect.signature(PTEngine.__init__).parameters
    for name in ("hist", "posterior_hist"):
        assert name not in inspect.signature(PTSampler.__init__).parameters
        assert name not in inspect.signature(PTSampler.sample).parameters
    with pytest.raises(TypeError, match="hist"):                     # the plain constructors keep their parameters
        PTEngine(6, 1, 1, np.eye(6), hist=(-1.0, 1.0, 10))
    with pytest.raises(TypeError, match="posterior_hist"):
        _sampler(tmp_path, "kw", posterior_hist=(-1.0, 1.0, 10))


def test_refusals_fall_before_any_library_is_loaded(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    d = 4
    make = lambda **kw: PTEngine.with_stages(d, 1, 1, np.eye(d), **kw)      # noqa: E731
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (np.zeros(d), np.array([1.0, 1.0, 0.0, 1.0])), (0.0, np.inf), (np.nan, 1.0), (-np.inf, 0.0)):
        with pytest.raises(ValueError, match="lo < hi"):
            make(hist=(lo, hi, 8))
    for nbins in (1, 0, -3, 1025, 2.5):
        with pytest.raises(ValueError, match="nbins"):
            make(hist=(0.0, 1.0, nbins))
    for lo, hi in ((np.zeros(d - 1), 1.0), (0.0, np.ones(d + 1)), (np.zeros((d, 1)), 1.0)):
        with pytest.raises(ValueError, match="ndim = 4"):
            make(hist=(lo, hi, 8))
    with pytest.raises(ValueError, match="hist_from"):
        make(hist=(0.0, 1.0, 8), hist_from=-1)
    with pytest.raises(ValueError, match="hist_from"):
        make(hist_from=5)                                            # goes with hist=
    with pytest.raises(ValueError, match="lo, hi, nbins"):
        make(hist=(0.0, 1.0))
    # good bins: the constructor gets as far as loading the library
    for kw in (dict(hist=(0.0, 1.0, 2)), dict(hist=(-np.ones(d), np.ones(d), 1024), hist_from=0), dict(hist=(0.0, np.arange(1.0, d + 1), 8), hist_from=7)):
        with pytest.raises(AssertionError, match="library was loaded"):
            make(**kw)


def test_a_replayed_resume_names_the_checkpoint(tmp_path):
    s = _sampler(tmp_path, "replay", resume=True, checkpoint=False)
    os.makedirs(s.outDir, exist_ok=True)
    np.savetxt(os.path.join(s.outDir, "chain_1.txt"), np.zeros((1, 3 + 4)))      # a chain file and no device checkpoint
    s.posterior_hist = (-1.0, 1.0, 10)
    with pytest.raises(NotImplementedError, match="checkpoint=True"):
        s.sample(np.zeros(3), 10, isave=10, thin=1)


def test_the_rule_on_edge_values():
    lo, hi, nbins = np.array([0.0, -1.3]), np.array([1.0, 2.9]), 7
    edges = lo[:, None] + np.arange(nbins + 1)[None, :] * ((hi - lo) / nbins)[:, None]
    for j in range(2):
        one = lambda v: hist_rule(np.array([[v, v]]), lo, hi, nbins)[j]      # noqa: E731
        assert one(lo[j])[0] == 1                                    # lo itself: bin 0
        assert one(np.nextafter(lo[j], -np.inf))[nbins] == 1         # just below: under
        assert one(hi[j])[nbins + 1] == 1                            # hi: over
        assert one(np.nextafter(hi[j], -np.inf))[nbins - 1] == 1     # just below: the last bin
        for v, col in ((np.nan, nbins), (-np.inf, nbins), (np.inf, nbins + 1)):
            assert one(v)[col] == 1 and one(v).sum() == 1
        for k in range(1, nbins):                                    # an interior edge lands in bin k or, as the product rounds, k - 1
            c = one(edges[j, k])
            assert c.sum() == 1 and (c[k] == 1 or c[k - 1] == 1)
    assert hist_rule(np.array([[-0.0, 0.0]]), lo, hi, nbins)[0, 0] == 1      # -0.0 with lo = 0: t = -0.0 >= 0.0
    x = np.random.default_rng(0).uniform(-2, 4, (50, 3, 2))
    w = np.random.default_rng(1).integers(0, 5, (50, 3))
    c = hist_rule(x, lo, hi, nbins, w)
    assert c.dtype == np.uint64 and c.shape == (2, nbins + 2) and (c.sum(1) == w.sum()).all()
    ref = np.stack([np.histogram(x[..., j].ravel(), bins=nbins, range=(lo[j], hi[j]), weights=w.ravel())[0] for j in range(2)])
    assert np.abs(c[:, :nbins].astype(np.int64) - ref.astype(np.int64)).sum() <= 4      # np.histogram closes the last bin and rounds its own way
    from ptmcmcsampler_amd.engine import hist_edges, hist_spec
    l2, h2, nb = hist_spec(2, (lo, hi, nbins))
    e = hist_edges(l2, h2, nb)
    assert e.shape == (2, nbins + 1) and np.array_equal(e[:, 0], lo) and np.array_equal(e[:, -1], hi) and np.allclose(e, edges, rtol=1e-15)


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "ptmi_hist.s")
    cmd = [_build.hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_hist.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def test_the_unit_compiles_for_gfx950_without_scratch_or_spills(unit_asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    names = [k for k, _ in kernels]
    for want in ("hist_weight_kernel", "hist_rows_kernel"):
        assert any(want in n for n in names), (want, names)
    for name, desc in kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
    spills = re.findall(r"\.(sgpr|vgpr)_spill_count:\s*(\d+)", unit_asm)
    assert len(spills) == 2 * len(kernels) and all(int(v) == 0 for _, v in spills), spills
    # the elements go into the block's LDS tile; global atomics only where a block hands its tile over: one instruction in the unit
    rows = next(n for n in names if "hist_rows_kernel" in n)
    body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(rows), unit_asm, re.S | re.M).group(1)
    assert "ds_add_u32" in body and len(re.findall(r"global_atomic_add_x2", body)) == 1
    assert "v_fma_f64" not in body and "v_fmac_f64" not in body       # one subtraction, one multiplication
