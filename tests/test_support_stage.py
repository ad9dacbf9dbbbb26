"""The likelihood callback only inside the prior's support (csrc/ptmi_sup.hip, include/ptmi.h ptmi_sup_*; the reference calls logl(y) only
when logp(y) != -inf, PTMCMCSampler.py:605-612 and :479-487) -- what can be checked without a GPU: the C ABI carries the four entry points,
the Python surface takes ``logl_in_support`` as an opt-in and refuses what it does not serve before a library is loaded, and the new unit
cross-compiles for gfx950 into kernels without scratch or spilled registers.  The runs themselves: tests/test_support_stage_gpu.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_sup_work_bytes", "ptmi_sup_begin", "ptmi_sup_rows", "ptmi_sup_end")


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
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_sup_\w+)\(([^;]*)\);", hdr)}
    assert decl == {
        "ptmi_sup_work_bytes": "ptmi_handle h, int64_t n_in, size_t *bytes",
        "ptmi_sup_begin": "ptmi_handle h, void *work, const double *lp , int64_t n_in, int64_t *n",
        "ptmi_sup_rows": "ptmi_handle h, void *work, const double *rows_in , double *rows",
        "ptmi_sup_end": "ptmi_handle h, void *work, const double *vals , double *out"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS, s
        assert s in exported, s
    H = C.c_void_p
    assert L.ptmi_sup_work_bytes.argtypes == [H, C.c_int64, C.POINTER(C.c_size_t)]
    assert L.ptmi_sup_begin.argtypes == [H, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    assert L.ptmi_sup_rows.argtypes == [H, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.ptmi_sup_end.argtypes == [H, C.c_void_p, C.c_void_p, C.c_void_p]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_sup.hip" for src in _build.deps())
    # ... and the work list of build() compiles the unit into an object of its own
    assert re.search(r'"ptmi_sup\.hip"\), os\.path\.join\(OBJ, "sup\.o"\)', inspect.getsource(_build.build))


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTEngine.logl_in_support is False and PTSampler.logl_in_support is False
    assert _sampler(tmp_path, "default").logl_in_support is False
    sig = inspect.signature(PTEngine.with_stages).parameters
    assert sig["logl_in_support"].default is False and sig["logl_in_support"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "logl_in_support" not in inspect.signature(PTEngine.__init__).parameters
    assert "logl_in_support" not in inspect.signature(PTSampler.__init__).parameters
    assert "logl_in_support" not in inspect.signature(PTSampler.sample).parameters
    with pytest.raises(TypeError, match="logl_in_support"):          # the plain constructors keep their parameters
        PTEngine(6, 1, 1, np.eye(6), split=True, logl_in_support=True)
    with pytest.raises(TypeError, match="logl_in_support"):
        _sampler(tmp_path, "kw", logl_in_support=True)


def test_refusals_fall_before_any_library_is_loaded(tmp_path, monkeypatch):
    from ptmcmcsampler_amd import PTSampler, _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    # the engine: the stage belongs to the callback path
    with pytest.raises(ValueError, match="callback path") as e:
        PTEngine.with_stages(6, 1, 1, np.eye(6), logl_in_support=True)
    assert "split=True" in str(e.value) and "rows_logl=True" in str(e.value)
    # with the callback path the refusal is gone: the constructor gets as far as loading the library
    for kw in (dict(split=True), dict(rows_logl=True)):
        with pytest.raises(AssertionError, match="library was loaded"):
            PTEngine.with_stages(6, 1, 1, np.eye(6), logl_in_support=True, **kw)
    # a sampler that calls logl per chain: it already behaves this way
    s = _sampler(tmp_path, "per_chain")
    s.logl_in_support = True
    with pytest.raises(ValueError, match="per chain") as e:
        s.sample(np.zeros(3), 10)
    assert "batched=True" in str(e.value) and "rows_logl=True" in str(e.value)
    # a device likelihood in the fused kernels: no callback
    s = PTSampler(3, ("iso",), ("box", -np.ones(3), np.ones(3)), np.eye(3), outDir=str(tmp_path / "fused"), verbose=False)
    s.logl_in_support = True
    with pytest.raises(ValueError, match="fused step kernels") as e:
        s.sample(np.zeros(3), 10)
    assert "rows_logl=True" in str(e.value)
    # served: a batched sampler and a device likelihood as row kernels get as far as the engine
    for name, args, kw in (("batched", (lambda X: -0.5 * (X * X).sum(-1), lambda X: 0.0 * X[:, 0]), dict(batched=True)),
                           ("rows", (("iso",), ("box", -np.ones(3), np.ones(3))), dict(rows_logl=True))):
        s = PTSampler(3, args[0], args[1], np.eye(3), outDir=str(tmp_path / name), verbose=False, **kw)
        s.logl_in_support = True
        with pytest.raises(AssertionError, match="library was loaded"):
            s.sample(np.zeros(3), 10)


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "ptmi_sup.s")
    cmd = [_build.hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_sup.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def test_the_unit_compiles_for_gfx950_without_scratch_or_spills(unit_asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    names = [k for k, _ in kernels]
    for want in ("sup_count_kernel", "sup_scan_kernel", "sup_rank_kernel", "sup_rows_kernelILi2E", "sup_rows_kernelILi1E", "sup_end_kernel"):
        assert any(want in n for n in names), (want, names)
    for name, desc in kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
    spills = re.findall(r"\.(sgpr|vgpr)_spill_count:\s*(\d+)", unit_asm)
    assert len(spills) == 2 * len(kernels) and all(int(v) == 0 for _, v in spills), spills
    private = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", unit_asm)
    assert len(private) == len(kernels) and all(int(v) == 0 for v in private), private
    # row copies in 16-byte pieces for even ndim
    for stem, piece in (("sup_rows_kernelILi2E", "dwordx4"), ("sup_rows_kernelILi1E", "dwordx2")):
        name = next(n for n in names if stem in n)
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), unit_asm, re.S | re.M).group(1)
        assert "global_load_" + piece in body and "global_store_" + piece in body, stem
