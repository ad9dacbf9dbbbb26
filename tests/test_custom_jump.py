"""Custom jump proposals in the cycle as batched device callbacks (csrc/ptmi_cj.hip, include/ptmi.h ptmi_cj_*; the reference's
addProposalToCycle, PTMCMCSampler.py:988-1014, dispatched at :1058-1059) -- what can be checked without a GPU: the C ABI carries the
five entry points, the Python surface takes ``batched=`` and refuses what it does not serve, and the new unit cross-compiles for gfx950
into kernels without scratch whose row copies are 16-byte instructions.  The runs themselves: tests/test_custom_jump_gpu.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_cj_attach", "ptmi_cj_work_bytes", "ptmi_cj_begin", "ptmi_cj_end", "ptmi_cj_box_draw")


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
    assert any(os.path.basename(src) == "ptmi_cj.hip" for src in _build.deps())


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_add_proposal_to_cycle_takes_batched_and_refuses_what_is_not_served(tmp_path):
    """Every refusal below is decided before an engine is built: no GPU needed."""
    import inspect
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert inspect.signature(PTSampler.addProposalToCycle).parameters["batched"].default is False

    def myJump(X, it, beta):
        return X, None

    # a batched jump on a sampler that calls its jumps per chain
    s = _sampler(tmp_path, "a")
    s.addProposalToCycle(myJump, 3, batched=True)
    assert s.propCycle.count(myJump) == 3 and "myJump" in s.jumpDict
    with pytest.raises(ValueError, match="batched"):
        s.sample(np.zeros(3), 10)
    # a per-chain jump on a batched sampler: as before
    s = _sampler(tmp_path, "b", batched=True)
    s.addProposalToCycle(lambda x, it, beta: (x, 0), 3)
    with pytest.raises(NotImplementedError, match="batched=True"):
        s.sample(np.zeros(3), 10)
    # one of each: the per-chain one still cannot ride the device path
    s = _sampler(tmp_path, "c", batched=True)
    s.addProposalToCycle(myJump, 2, batched=True)
    s.addProposalToCycle(lambda x, it, beta: (x, 0), 1)
    with pytest.raises(NotImplementedError, match="batched=True"):
        s.sample(np.zeros(3), 10)
    # auxiliary jumps stay per chain, and the message says why
    s = _sampler(tmp_path, "d", batched=True)
    with pytest.raises(NotImplementedError, match="state"):
        s.addAuxilaryJump(lambda x, q, it, beta: (q, 0), batched=True)
    # the library's box draw is a named jump
    assert PTSampler.boxDrawJump(-1.0, 1.0).__name__ == "boxDrawJump"
    # engine: w_host with rows_logl needs jumps=; jumps= do not mix with gradient jumps; they need the callback path
    with pytest.raises(ValueError, match="w_host"):
        PTEngine(6, 1, 1, np.eye(6), w_host=2, rows_logl=True)
    with pytest.raises(ValueError, match="gradient"):
        PTEngine(6, 1, 1, np.eye(6), split=True, jumps=[(myJump, 2)], grad_weights=(0, 5))
    with pytest.raises(ValueError, match="split"):
        PTEngine(6, 1, 1, np.eye(6), jumps=[(myJump, 2)])
    with pytest.raises(ValueError, match="w_host"):
        PTEngine(6, 1, 1, np.eye(6), split=True, w_host=3, jumps=[(myJump, 2)])


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "ptmi_cj.s")
    cmd = [_build.hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_cj.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def _kernel_body(asm, name):
    lines = asm.split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start:end + 1]


def test_the_unit_compiles_for_gfx950_without_scratch(unit_asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    names = [k for k, _ in kernels]
    for want in ("cj_count_kernel", "cj_gather_kernelILi2E", "cj_gather_kernelILi1E", "cj_scatter_kernelILi2E", "cj_scatter_kernelILi1E",
                 "cj_box_kernel"):
        assert any(want in n for n in names), (want, names)
    for name, desc in kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name


def test_even_ndim_moves_rows_in_16_byte_pieces(unit_asm):
    names = re.findall(r"\.amdhsa_kernel (\S+)", unit_asm)
    for stem in ("cj_gather_kernelILi2E", "cj_scatter_kernelILi2E"):
        body = _kernel_body(unit_asm, next(n for n in names if stem in n))
        assert any("global_load_dwordx4" in ln for ln in body), stem
        assert any("global_store_dwordx4" in ln for ln in body), stem
