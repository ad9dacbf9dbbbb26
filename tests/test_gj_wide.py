"""HMC beyond 512 parameters on the callback path (csrc/ptmi_gjcb_wide.hip) at the C ABI and in the Python signatures -- no GPU
needed.  The device side is tests/test_gj_wide_gpu.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from ptmcmcsampler_amd import _lib
    if not os.path.exists(_lib.SO):
        ge.build()
    return _lib


def _create(lib, names, **over):
    """ptmi_create on host memory that is never touched: argument validation ends at the search for a device."""
    L = lib.load()
    d = over.get("ndim", 600)
    ladder = np.array([1.0, 2.0])
    temps = ladder.copy()
    one = np.zeros(8)
    tab = np.zeros(3)                                                   # (read only once a device is found)
    kw = dict(ndim=d, ntemps=2, nwalkers=2, ntemps_global=2, w_scam=20, cov_update=10, de_size=10, tskip=10, cov_per_walker=1,
              ladder=ladder.ctypes.data_as(lib._dp), temps_mh=temps.ctypes.data_as(lib._dp),
              w_hmc=5, gj_tab=tab.ctypes.data_as(lib._dp), hmc_min=2, hmc_max=30, hmc_eps=0.1, nuts_maxdepth=24)
    kw.update(over)
    cfg = lib.Config(**kw)
    buf = lib.Buffers(**{k: C.c_void_p(one.ctypes.data) for k in names})
    h = C.c_void_p()
    rc = L.ptmi_create(C.byref(cfg), C.byref(buf), C.byref(h))
    assert rc != 0 and not h
    return rc, L.ptmi_last_error().decode()


BASE = ("X", "lnL", "lp", "temp_of", "slot_of", "Ut", "S", "nacc", "jstat", "gj")
SPLIT = BASE + ("Q", "qaux")


def test_create_takes_hmc_beyond_512_on_a_split_handle(lib):
    """ndim = 600 with w_hmc > 0, the tables and the Q / qaux buffers passes every argument check and gets as far as looking for a
    device; NUTS there, a handle without Q, the interval family and ndim > 2048 stay refused."""
    nodev = lib.device_count() == 0                                     # (with a device a valid configuration would be created on host memory)
    for d in (513, 600, 2048):
        rc, msg = _create(lib, SPLIT, ndim=d) if nodev else (-4, "no HIP device")
        assert rc == -4 and "no HIP device" in msg, (d, rc, msg)        # PTMI_ENODEVICE
    rc, msg = _create(lib, SPLIT, w_nuts=5)
    assert rc == -3 and "ndim <= 512" in msg                            # PTMI_EUNSUPPORTED
    rc, msg = _create(lib, BASE)
    assert rc == -3 and "ndim <= 512" in msg
    ipar = np.ones(3 * 600)
    rc, msg = _create(lib, SPLIT, logl_kind=lib.LOGL["interval"], logl_par=ipar.ctypes.data_as(lib._dp), logl_par_len=3 * 600)
    assert rc == -3 and "ndim <= 512" in msg
    rc, msg = _create(lib, SPLIT, w_hmc=0, logl_kind=lib.LOGL["interval"], logl_par=ipar.ctypes.data_as(lib._dp), logl_par_len=3 * 600)
    assert rc == -3 and "ndim <= 512" in msg
    rc, msg = _create(lib, SPLIT, ndim=2049)
    assert rc == -3 and "2048" in msg and "ndim <= 512" not in msg      # a message of its own
    # at and below the limit nothing changed
    rc, msg = _create(lib, BASE, ndim=512) if nodev else (-4, "no HIP device")
    assert rc == -4 and "no HIP device" in msg


def test_lanes_for_grad(lib):
    L = lib.load()
    for d, lanes in ((512, 64), (513, 64), (1024, 64), (2048, 64), (2049, 0), (32, 4), (112, 16), (113, 64)):
        assert lib.lanes_for(d, grad=True) == lanes == L.ptmi_lanes_for_grad(d), d
    # the buffers' row formats of a 64-lane handle whatever the gradient flag says
    st, ep = C.c_int(-1), C.c_int(-1)
    assert L.ptmi_de_row_stride(600, 1, C.byref(st), C.byref(ep)) == 0 and (st.value, ep.value) == (600, 0)
    assert L.ptmi_am_row_format(600, 1, C.byref(ep)) == 0 and ep.value == 0


def test_signatures_are_unchanged(lib):
    """The wide stage needs no new keyword, argument or call: the public signatures are the parent's."""
    from ptmcmcsampler_amd.engine import PTEngine
    from ptmcmcsampler_amd.sampler import PTSampler
    assert list(inspect.signature(PTEngine.__init__).parameters) == [
        "self", "ndim", "ntemps", "nwalkers", "cov0", "ladder", "logl", "logp", "weights", "cov_update", "burn", "tskip", "seed", "cov_mode",
        "hot_chain", "Tmin", "Tmax", "ntemps_global", "temp0", "walker0", "device", "split", "use_de_buffer", "w_host", "keep_lnl", "groups",
        "swap_mode", "grad_weights", "hmc", "nuts_delta", "nuts_maxdepth", "pick_mode", "eig_mode", "am_mode", "eig_lag", "stats_async",
        "split_nuts", "rows_logl", "jumps"]
    assert list(inspect.signature(PTSampler.__init__).parameters) == [
        "self", "ndim", "logl", "logp", "cov", "groups", "loglargs", "loglkwargs", "logpargs", "logpkwargs", "logl_grad", "logp_grad", "comm",
        "outDir", "verbose", "resume", "seed", "nwalkers", "ntemps", "device", "cov_mode", "keep_walkers", "swap_mode", "pick_mode", "eig_mode",
        "checkpoint", "batched", "nuts_maxdepth", "batched_nuts", "rows_logl"]
    assert list(inspect.signature(PTSampler.sample).parameters) == [
        "self", "p0", "Niter", "ladder", "Tmin", "Tmax", "Tskip", "isave", "covUpdate", "SCAMweight", "AMweight", "DEweight", "NUTSweight",
        "MALAweight", "HMCweight", "burn", "HMCstepsize", "HMCsteps", "maxIter", "thin", "i0", "neff", "writeHotChains", "hotChain"]
    assert list(inspect.signature(PTSampler.resolve_rows_logl).parameters) == ["ndim", "logl", "logp", "rows_logl"]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (ptmi_gj_\w+)\(([^;]*)\);", hdr)}
    assert decl == {
        "ptmi_gj_work_bytes": "ptmi_handle h, size_t *bytes",
        "ptmi_gj_begin": "ptmi_handle h, int64_t iter, void *work, double *rows , int64_t *n",
        "ptmi_gj_step": "ptmi_handle h, void *work, const double *lnl , const double *dlnl , const double *lp , const double *dlp , "
                        "double *rows, int64_t *n"}
    L = lib.load()
    H = C.c_void_p
    assert L.ptmi_gj_work_bytes.argtypes == [H, C.POINTER(C.c_size_t)]
    assert L.ptmi_gj_begin.argtypes == [H, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    assert L.ptmi_gj_step.argtypes == [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]


def test_sampler_decides_the_row_path_and_refuses_nuts(tmp_path):
    """Device gradients beyond 512-d: the sampler takes the row path by itself (resolve_rows_logl's own answers stay); NUTS there is
    refused with the way out, before an engine is built."""
    from ptmcmcsampler_amd.sampler import PTSampler
    assert PTSampler.resolve_rows_logl(600, ("iso",), ("flat",)) is False          # (unchanged: the iso family alone stays fused)
    assert PTSampler.resolve_rows_logl(600, ("dense", 0, 0), ("flat",)) is True
    kw = dict(outDir=str(tmp_path), verbose=False)
    s = PTSampler(600, ("iso",), ("flat",), np.eye(600), logl_grad=True, logp_grad=True, **kw)
    assert s.rows_logl is True
    assert PTSampler(600, ("iso",), ("flat",), np.eye(600), **kw).rows_logl is False
    assert PTSampler(512, ("iso",), ("flat",), np.eye(512), logl_grad=True, logp_grad=True, **kw).rows_logl is False
    assert PTSampler(600, ("iso",), ("flat",), np.eye(600), logl_grad=True, logp_grad=True, rows_logl=False, **kw).rows_logl is False
    with pytest.raises(NotImplementedError, match="NUTSweight=0"):
        s.initialize(10, NUTSweight=20, HMCweight=20)
    f = lambda X: X.sum(-1)          # noqa: E731
    g = lambda X: (X.sum(-1), X)     # noqa: E731
    with pytest.raises(ValueError, match="512"):
        PTSampler(600, f, f, np.eye(600), logl_grad=g, logp_grad=g, batched=True, batched_nuts=True, **kw)
    b = PTSampler(600, f, f, np.eye(600), logl_grad=g, logp_grad=g, batched=True, **kw)
    with pytest.raises(NotImplementedError, match="NUTSweight=0"):
        b.initialize(10, NUTSweight=20, HMCweight=20)
