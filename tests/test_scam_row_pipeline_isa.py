"""The persistent exact-shape SCAM kernel (mh_steps_kernel<4, 25, iso, ..., ULDS, 512, flat>, ptmi_mh.inc.h) keeps its register budget:
compiled for gfx950 with the library's flags it fits the 256 vector registers of two waves per SIMD, and its pass loop -- the loop
whose body is the draw pass and four straight-line steps, each with the 12 16-byte LDS reads of a direction row -- holds no scratch
access.  Needs hipcc, no GPU (the unit cross-compiles to assembly in a quarter of a minute)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT_PERSISTENT = "_Z15mh_steps_kernelILi4ELi25ELi0ELb0ELb0ELb0ELb1ELi512ELi0ELb0ELb0EEv5KArgs"


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "shape_4_25_0.s")
    cmd = [_build.hipcc()] + _build.FLAGS + _build.shape_defs(4, 25, 0, 0) + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_shape.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def _kernel_body(asm, name):
    lines = asm.split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start:end + 1]


def _loops(body):
    """(header line, last back-edge line) of every loop: a label that a later branch jumps back to."""
    labels = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", ln)] if m}
    last = {}
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and labels.get(m.group(1), i) < i:
            last[labels[m.group(1)]] = i
    return sorted(last.items())


def test_flat_persistent_kernel_fits_two_waves_per_simd(unit_asm):
    m = re.search(r"\.amdhsa_kernel " + FLAT_PERSISTENT + r"\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    assert m, "the flat-prior persistent kernel of shape (4, 25) is not in the unit"
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(1)).group(1))
    print("next_free_vgpr %d, private segment %s bytes" % (vgpr, re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(1)).group(1)))
    assert vgpr <= 256


def test_no_scratch_access_in_the_pass_loop(unit_asm):
    body = _kernel_body(unit_asm, FLAT_PERSISTENT)
    # the pass loop: the innermost loop that holds the row reads of four steps (4 x 12 ds_read_b128)
    with_rows = [(a, b) for a, b in _loops(body) if sum("ds_read_b128" in ln for ln in body[a:b + 1]) >= 48]
    assert with_rows, "no loop with four steps' row reads: the full pass is not straight-line code"
    a, b = min(with_rows, key=lambda ab: ab[1] - ab[0])
    scratch = [ln.strip() for ln in body[a:b + 1] if re.match(r"\s+scratch_", ln)]
    valu = sum(bool(re.match(r"\s+v_", ln)) for ln in body[a:b + 1])
    print("pass loop: %d lines, %d vector instructions (static), %d v_mov_b64, %d scratch accesses" % (
        b - a + 1, valu, sum("v_mov_b64" in ln for ln in body[a:b + 1]), len(scratch)))
    assert not scratch, scratch
