"""Auxiliary jumps as batched device callbacks (csrc/ptmi_aux.hip, include/ptmi.h ptmi_aux_*; the reference's addAuxilaryJump,
PTMCMCSampler.py:1017-1028, run on every jump's result at :1062-1065) -- what can be checked without a GPU: the C ABI carries the three
entry points, the Python surface takes ``batched_aux`` / ``with_stages(aux=)`` and refuses what it does not serve, and the new unit cross-compiles
for gfx950 into kernels without scratch or spilled registers.  The runs themselves: tests/test_aux_jump_gpu.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_aux_attach", "ptmi_aux_begin", "ptmi_aux_end")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from ptmcmcsampler_amd import _lib
    if not os.path.exists(_lib.SO):
        ge.build()
    return _lib


def test_header_binding_and_library_carry_the_entry_points(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ptmi_[a-z0-9_]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in declared, s
        assert s in lib.SYMBOLS, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, s
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_aux.hip" for src in _build.deps())


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_batched_aux_is_opt_in_and_refuses_what_is_not_served(tmp_path):
    """Every refusal below is decided before an engine is built: no GPU needed."""
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTSampler.batched_aux is False and _sampler(tmp_path, "default").batched_aux is False
    assert inspect.signature(PTSampler.addAuxilaryJump).parameters["batched"].default is False
    sig = inspect.signature(PTEngine.with_stages).parameters
    assert sig["jumps_with_grad"].default is False and sig["aux"].default is None and PTEngine.jumps_with_grad is False
    with pytest.raises(TypeError, match="aux"):                      # the plain constructors keep their parameters
        PTEngine(6, 1, 1, np.eye(6), split=True, aux=[])
    with pytest.raises(TypeError, match="batched_aux"):
        _sampler(tmp_path, "kw", batched_aux=True)

    def myAux(X, Q, it, beta):
        return Q, None

    # without the flag: today's refusal, which says why and how to opt in
    s = _sampler(tmp_path, "a", batched=True)
    with pytest.raises(NotImplementedError, match="state") as e:
        s.addAuxilaryJump(myAux, batched=True)
    assert "batched_aux = True" in str(e.value)
    # with it the function is stored, apart from the per-chain ones, and nothing is raised
    s = _sampler(tmp_path, "b", batched=True)
    s.batched_aux = True
    s.addAuxilaryJump(myAux, batched=True)
    assert s._batched_aux == [myAux] and s.aux == []
    # a per-chain auxiliary jump: unchanged on a per-chain sampler, still refused on a batched one
    s = _sampler(tmp_path, "c")
    s.addAuxilaryJump(lambda x, q, it, beta: (q, 0))
    assert len(s.aux) == 1 and s._batched_aux == []
    s = _sampler(tmp_path, "d", batched=True)
    s.batched_aux = True
    s.addAuxilaryJump(lambda x, q, it, beta: (q, 0))
    with pytest.raises(NotImplementedError, match="batched=True"):
        s.sample(np.zeros(3), 10)
    # a batched one on a sampler that calls its jumps per chain
    s = _sampler(tmp_path, "e")
    s.batched_aux = True
    s.addAuxilaryJump(myAux, batched=True)
    with pytest.raises(ValueError, match="batched"):
        s.sample(np.zeros(3), 10)
    # engine: aux= needs the callback path, and takes callables; custom jumps beside gradient jumps need the keyword
    with pytest.raises(ValueError, match="split"):
        PTEngine.with_stages(6, 1, 1, np.eye(6), aux=[myAux])
    with pytest.raises(ValueError, match="callables"):
        PTEngine.with_stages(6, 1, 1, np.eye(6), split=True, aux=[3])
    with pytest.raises(ValueError, match="jumps_with_grad"):
        PTEngine(6, 1, 1, np.eye(6), split=True, jumps=[(lambda X, it, beta: (X, None), 2)], grad_weights=(0, 5))
    # host-served entries beside gradient jumps without jumps=: nothing would serve those picks (the library used to refuse the handle)
    for kw in (dict(split=True), dict()):
        with pytest.raises(ValueError, match="w_host"):
            PTEngine.with_stages(6, 1, 1, np.eye(6), w_host=2, grad_weights=(0, 5), jumps_with_grad=True, **kw)


def test_the_engine_refuses_aux_before_any_library_is_loaded(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(ValueError, match="callback path"):
        PTEngine.with_stages(6, 1, 1, np.eye(6), aux=[lambda X, Q, it, beta: (Q, None)])


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "ptmi_aux.s")
    cmd = [_build.hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_aux.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def test_the_unit_compiles_for_gfx950_without_scratch_or_spills(unit_asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    names = [k for k, _ in kernels]
    for want in ("aux_gather_kernelILi2E", "aux_gather_kernelILi1E", "aux_copy_kernelILi2E", "aux_copy_kernelILi1E", "aux_qxy_kernel"):
        assert any(want in n for n in names), (want, names)
    for name, desc in kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
    # the kernels' metadata records: one per kernel, no spilled register of either kind, no private segment
    spills = re.findall(r"\.(sgpr|vgpr)_spill_count:\s*(\d+)", unit_asm)
    assert len(spills) == 2 * len(kernels) and all(int(v) == 0 for _, v in spills), spills
    private = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", unit_asm)
    assert len(private) == len(kernels) and all(int(v) == 0 for v in private), private
