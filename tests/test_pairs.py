"""Joint posterior histograms of parameter pairs of every cold chain, accumulated on the device from the AM ring (csrc/ptmi_pairs.hip,
include/ptmi.h ptmi_pairs_attach / ptmi_pairs_update; ``PTEngine.with_stages(pairs=(pairs, lo, hi, nbins))``,
``PTSampler.posterior_pairs``, ptmcmcsampler_amd/pairs.py) -- what can be checked without a GPU: the C ABI carries the two entry
points, the counting rule against ``np.histogram2d`` and on its edge cases, the contour thresholds, the spec and its refusals before
a library is loaded, the sampler's refusals, and the new unit cross-compiles for gfx950 into kernels without scratch.  The runs
themselves: tests/test_pairs_gpu.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ptmcmcsampler_amd.pairs import credible_levels, expand_pairs, pairs_rule, pairs_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_pairs_attach", "ptmi_pairs_update")


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
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_pairs_\w+)\(([^;]*)\);", hdr)}
    assert decl == {
        "ptmi_pairs_attach": "ptmi_handle h, uint64_t *counts, const int32_t *pairs, int32_t npairs, const double *lo, const double *scale, "
                             "int32_t nbins",
        "ptmi_pairs_update": "ptmi_handle h, int64_t iter_lo, int64_t iter_hi"}
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", lib.SO], text=True).splitlines() if ln.strip()}
    L = lib.load()
    for s in NEW:
        assert s in lib.SYMBOLS, s
        assert s in exported, s
    H = C.c_void_p
    assert L.ptmi_pairs_attach.argtypes == [H, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.c_int32]
    assert L.ptmi_pairs_update.argtypes == [H, C.c_int64, C.c_int64]
    from ptmcmcsampler_amd import _build
    assert any(os.path.basename(src) == "ptmi_pairs.hip" for src in _build.deps())
    assert re.search(r'"ptmi_pairs\.hip"\), os\.path\.join\(OBJ, "pairs\.o"\)', inspect.getsource(_build.build))


def test_the_rule_equals_histogram2d_where_every_edge_is_exact():
    lo, hi, nbins = -4.0, 4.0, 16                                    # scale = 2 and every edge k / 2 - 4 are exact in binary
    x = np.random.default_rng(20).normal(0.0, 1.5, (4000, 3))
    assert not np.isin(x, -4.0 + 0.5 * np.arange(nbins + 1)).any()   # no draw on an edge: the two roundings cannot differ
    pairs = np.array([[0, 1], [1, 2], [2, 0]])
    got = pairs_rule(x, pairs, lo, hi, nbins)
    assert got.dtype == np.uint64 and got.shape == (3, nbins * nbins + 1)
    edges = np.linspace(lo, hi, nbins + 1)
    for p, (i, j) in enumerate(pairs):
        ref = np.histogram2d(x[:, i], x[:, j], bins=(edges, edges))[0]
        assert np.array_equal(got[p, :-1].reshape(nbins, nbins), ref.astype(np.uint64)), (i, j)
        assert got[p, -1] == len(x) - int(ref.sum()) and got[p, -1] > 0      # 1.5 sigma draws leave the box


def test_transposes_sums_and_weights():
    rs = np.random.default_rng(3)
    x = rs.uniform(-2, 4, (50, 3, 4))
    w = rs.integers(0, 5, (50, 3))
    lo, hi, nbins = np.array([0.0, -1.3, 0.1, -2.0]), np.array([1.0, 2.9, 3.7, 5.0]), 7
    pairs = np.array([[0, 1], [1, 0], [3, 2], [2, 3]])
    c = pairs_rule(x, pairs, lo, hi, nbins, w)
    assert (c.sum(1) == w.sum()).all()                               # each pair's cells sum to the weights
    t = lambda row: row[:-1].reshape(nbins, nbins)      # noqa: E731
    assert np.array_equal(t(c[0]), t(c[1]).T) and np.array_equal(t(c[2]), t(c[3]).T) and c[0, -1] == c[1, -1] and c[2, -1] == c[3, -1]
    assert (pairs_rule(x, pairs, lo, hi, nbins).sum(1) == 150).all()
    # a weight is a repeat
    assert np.array_equal(c, pairs_rule(np.repeat(x.reshape(-1, 4), w.reshape(-1), axis=0), pairs, lo, hi, nbins))


def test_edge_values_and_non_finite_coordinates():
    lo, hi, nbins = np.array([0.0, -1.3]), np.array([1.0, 2.9]), 7
    mid = np.array([0.5, 0.0])
    cells = nbins * nbins
    one = lambda a, b: pairs_rule(np.array([[a, b]]), [[0, 1]], lo, hi, nbins)[0]      # noqa: E731
    inside = one(*mid)
    assert inside.sum() == 1 and inside[-1] == 0 and inside[3 * nbins + 2] == 1      # t = 3.5 and 1.3 * 7 / 4.2 = 2.17
    for bad in (np.nan, np.inf, -np.inf):
        for a, b in ((bad, mid[1]), (mid[0], bad), (bad, bad)):
            c = one(a, b)
            assert c[cells] == 1 and c.sum() == 1, (a, b)
    assert one(lo[0], lo[1])[0] == 1                                 # lo itself: bin 0 on both axes
    assert one(-0.0, lo[1])[0] == 1                                  # -0.0 with lo = 0: t = -0.0 >= 0.0
    assert one(np.nextafter(lo[0], -np.inf), mid[1])[cells] == 1 and one(mid[0], np.nextafter(lo[1], -np.inf))[cells] == 1
    assert one(hi[0], mid[1])[cells] == 1 and one(mid[0], hi[1])[cells] == 1      # hi: outside
    assert one(np.nextafter(hi[0], -np.inf), np.nextafter(hi[1], -np.inf))[cells - 1] == 1      # just below: the last cell


def test_credible_levels_on_a_hand_made_table():
    tab = np.array([[50, 20, 1],
                    [10, 5, 2],
                    [8, 3, 1]], dtype=np.uint64)                     # total 100; descending: 50 20 10 8 5 3 2 1 1 -> 50 70 80 88 93 96 98 99 100
    lv = credible_levels(tab, probs=(0.5, 0.68, 0.7, 0.95, 1.0))
    assert lv.shape == (5,) and lv.tolist() == [50.0, 20.0, 20.0, 3.0, 1.0]
    assert credible_levels(tab).tolist() == [20.0, 3.0]              # the defaults: 68 % and 95 %
    two = credible_levels(np.stack([tab, tab.T * 2, np.zeros_like(tab)]), probs=(0.68,))
    assert two.shape == (3, 1) and two[0, 0] == 20.0 and two[1, 0] == 40.0 and np.isnan(two[2, 0])
    # the cells at or above a level hold at least that share
    assert tab[tab >= 20].sum() >= 68 and tab[tab >= 3].sum() >= 95 and tab[tab > 3].sum() < 95
    for bad in ((0.0,), (1.5,)):
        with pytest.raises(ValueError, match="probs"):
            credible_levels(tab, probs=bad)
    with pytest.raises(ValueError, match="counts"):
        credible_levels(np.zeros(9))


def test_spec_parsing_and_every_refusal():
    d = 6
    assert expand_pairs(d, {"params": [4, 1, 3]}).tolist() == [[4, 1], [4, 3], [1, 3]]      # a before b in the list, in list order
    assert expand_pairs(d, {"params": np.arange(5)}).shape == (10, 2)
    pr = expand_pairs(d, [[0, 1], [1, 0], [5, 2]])
    assert pr.dtype == np.int32 and pr.flags.c_contiguous and pr.tolist() == [[0, 1], [1, 0], [5, 2]]
    pr, lo, hi, nbins = pairs_spec(d, ({"params": [0, 5]}, -1.0, np.arange(1.0, d + 1), 128.0))
    assert pr.tolist() == [[0, 5]] and lo.tolist() == [-1.0] * d and hi.tolist() == list(range(1, d + 1)) and nbins == 128 and type(nbins) is int
    for bad in ([[0, 0]], [[0, 6]], [[-1, 2]], [[0, 1], [3, 3]], {"params": [0, 9]}, {"params": [-1, 2]}):
        with pytest.raises(ValueError, match="two different parameters"):
            expand_pairs(d, bad)
    for bad in ([0, 1], [[0, 1, 2]], [[0.0, 1.0]], np.zeros((0, 2), dtype=int), {"params": [1]}, {"params": [1.0, 2.0]}, {"params": [1, 2, 1]},
                {"parms": [1, 2]}, {"params": [[0, 1]]}, np.zeros((8193, 2), dtype=int)):
        with pytest.raises(ValueError, match="pairs"):
            expand_pairs(d, bad)
    assert expand_pairs(200, {"params": np.arange(128)}).shape == (8128, 2)
    with pytest.raises(ValueError, match="npairs <= 8192"):
        expand_pairs(200, {"params": np.arange(129)})                # 8256 pairs


def test_refusals_fall_before_any_library_is_loaded(monkeypatch):
    from ptmcmcsampler_amd import _lib
    from ptmcmcsampler_amd.engine import PTEngine

    def no_load():
        raise AssertionError("the library was loaded before the refusal")

    monkeypatch.setattr(_lib, "load", no_load)
    d = 4
    make = lambda **kw: PTEngine.with_stages(d, 1, 1, np.eye(d), **kw)      # noqa: E731
    pr = [[0, 1], [2, 3]]
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (np.zeros(d), np.array([1.0, 1.0, 0.0, 1.0])), (0.0, np.inf), (np.nan, 1.0), (-np.inf, 0.0)):
        with pytest.raises(ValueError, match="lo < hi"):
            make(pairs=(pr, lo, hi, 8))
    for nbins in (1, 0, -3, 129, 1024, 2.5, "8", None):
        with pytest.raises(ValueError, match="nbins"):
            make(pairs=(pr, 0.0, 1.0, nbins))
    for lo, hi in ((np.zeros(d - 1), 1.0), (0.0, np.ones(d + 1)), (np.zeros((d, 1)), 1.0)):
        with pytest.raises(ValueError, match="ndim = 4"):
            make(pairs=(pr, lo, hi, 8))
    with pytest.raises(ValueError, match="two different parameters"):
        make(pairs=([[0, 4]], 0.0, 1.0, 8))
    with pytest.raises(ValueError, match="pairs_from"):
        make(pairs=(pr, 0.0, 1.0, 8), pairs_from=-1)
    with pytest.raises(ValueError, match="pairs_from"):
        make(pairs_from=5)                                           # goes with pairs=
    with pytest.raises(ValueError, match="pairs, lo, hi, nbins"):
        make(pairs=(0.0, 1.0, 8))
    # good specs: the constructor gets as far as loading the library
    for kw in (dict(pairs=(pr, 0.0, 1.0, 2)), dict(pairs=({"params": [3, 0, 1]}, -np.ones(d), np.ones(d), 128), pairs_from=0),
               dict(pairs=(pr, 0.0, 1.0, 8), hist=(0.0, 1.0, 8))):
        with pytest.raises(AssertionError, match="library was loaded"):
            make(**kw)


def _sampler(tmp_path, name, **kw):
    from ptmcmcsampler_amd import PTSampler
    d = 3
    return PTSampler(d, lambda x: -0.5 * float(np.dot(x, x)), lambda x: 0.0, np.eye(d), outDir=str(tmp_path / name), verbose=False, **kw)


def test_the_stage_is_opt_in(tmp_path):
    from ptmcmcsampler_amd import PTSampler
    from ptmcmcsampler_amd.engine import PTEngine
    assert PTSampler.posterior_pairs is None and PTSampler.pairs2d is None
    assert _sampler(tmp_path, "default").posterior_pairs is None
    sig = inspect.signature(PTEngine.with_stages).parameters
    for name in ("pairs", "pairs_from"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert name not in inspect.signature(PTEngine.__init__).parameters
    with pytest.raises(TypeError, match="pairs"):                    # the plain constructors keep their parameters
        PTEngine(6, 1, 1, np.eye(6), pairs=([[0, 1]], -1.0, 1.0, 10))
    with pytest.raises(TypeError, match="posterior_pairs"):
        _sampler(tmp_path, "kw", posterior_pairs=([[0, 1]], -1.0, 1.0, 10))


def test_a_replayed_resume_names_the_checkpoint(tmp_path):
    s = _sampler(tmp_path, "replay", resume=True, checkpoint=False)
    os.makedirs(s.outDir, exist_ok=True)
    np.savetxt(os.path.join(s.outDir, "chain_1.txt"), np.zeros((1, 3 + 4)))      # a chain file and no device checkpoint
    s.posterior_pairs = ([[0, 1]], -1.0, 1.0, 10)
    with pytest.raises(NotImplementedError, match="checkpoint=True"):
        s.sample(np.zeros(3), 10, isave=10, thin=1)


def test_set_after_the_engine_is_built_is_refused(tmp_path):
    class Built:                                                     # an engine that was built without any stage
        pairs_spec = hist_spec = None
        adapt_on = evidence_on = diag_on = False

    s = _sampler(tmp_path, "late")
    s.engine = Built()
    s.posterior_pairs = ([[0, 1]], -1.0, 1.0, 10)
    with pytest.raises(ValueError, match="posterior_pairs was set after the engine was built"):
        s.writeOutput(0)


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    from ptmcmcsampler_amd import _build
    out = str(tmp_path_factory.mktemp("isa") / "ptmi_pairs.s")
    cmd = [_build.hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "ptmi_pairs.hip"), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def test_the_unit_compiles_for_gfx950_without_scratch_or_spills(unit_asm):
    kernels = re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", unit_asm, re.S)
    names = [k for k, _ in kernels]
    for want in ("hist_weight_kernel", "pairs_rows_kernel"):
        assert any(want in n for n in names), (want, names)
    for name, desc in kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1)) <= 163840, name
    spills = re.findall(r"\.(sgpr|vgpr)_spill_count:\s*(\d+)", unit_asm)
    assert len(spills) == 2 * len(kernels) and all(int(v) == 0 for _, v in spills), spills
    # the dynamic LDS the launch asks for: the unit's budget, room for one pair at 128 bins within a CU's 160 KB
    src = open(os.path.join(ROOT, "ptmcmcsampler_amd", "csrc", "ptmi_pairs.hip")).read()
    budget = int(re.search(r"constexpr int LDS_BYTES = (\d+);", src).group(1))
    assert 65540 + 4096 + 2048 <= budget <= 163840
    # the elements go into the block's LDS tile; global atomics only where a block hands its tile over: one instruction in the unit
    rows = next(n for n in names if "pairs_rows_kernel" in n)
    body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(rows), unit_asm, re.S | re.M).group(1)
    assert "ds_add_u32" in body and len(re.findall(r"global_atomic_add_x2", body)) == 1
    assert "v_fma_f64" not in body and "v_fmac_f64" not in body       # one subtraction, one multiplication
