"""Gradient jumps (NUTS / HMC) together with parameter groups (PTMCMCSampler.py:129-145 with :225-258) at the C ABI and in the
Python signatures -- no GPU needed.  The device side is tests/test_gj_groups_gpu.py."""
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from ptmcmcsampler_amd import _lib
    if not os.path.exists(_lib.SO):
        ge.build()
    return _lib


def test_create_accepts_groups_with_gradient_jumps(lib):
    """ngroups = 2 with w_hmc > 0 passes every argument check of ptmi_create and gets as far as looking for a device; the interval
    family with groups stays refused."""
    import ctypes as C
    import numpy as np
    L = lib.load()
    d = 4
    ladder = np.array([1.0, 2.0])
    one = np.zeros(8)
    keep = dict(ladder=ladder, temps=ladder.copy(), tab=np.zeros(3 * d * d), gsize=np.array([2, 2], dtype=np.int32),
                gmask=np.array([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]]), ipar=np.ones(3 * d))

    def cfg(**over):
        kw = dict(ndim=d, ntemps=2, nwalkers=2, ntemps_global=2, w_scam=20, cov_update=10, de_size=10, tskip=10, cov_per_walker=1,
                  ladder=keep["ladder"].ctypes.data_as(lib._dp), temps_mh=keep["temps"].ctypes.data_as(lib._dp),
                  ngroups=2, group_size=keep["gsize"].ctypes.data_as(C.POINTER(C.c_int32)), group_mask=keep["gmask"].ctypes.data_as(lib._dp),
                  w_hmc=5, gj_tab=keep["tab"].ctypes.data_as(lib._dp), hmc_min=2, hmc_max=30, hmc_eps=0.1, nuts_maxdepth=24)
        kw.update(over)
        return lib.Config(**kw)

    buf = lib.Buffers(**{k: C.c_void_p(one.ctypes.data) for k in ("X", "lnL", "lp", "temp_of", "slot_of", "Ut", "S", "nacc", "jstat", "gj")})
    h = C.c_void_p()

    def err(c):
        rc = L.ptmi_create(C.byref(c), C.byref(buf), C.byref(h))
        assert rc != 0 and not h
        return rc, L.ptmi_last_error().decode()

    # the other refusals of the gradient stage stand
    rc, msg = err(cfg(logl_kind=lib.LOGL["interval"], logl_par=keep["ipar"].ctypes.data_as(lib._dp), logl_par_len=3 * d))
    assert rc == -3 and "one parameter group" in msg                             # PTMI_EUNSUPPORTED
    rc, msg = err(cfg(w_host=1))
    assert rc == -3 and "host-served" in msg
    rc, msg = err(cfg(ndim=600))
    assert rc == -3 and "ndim <= 512" in msg
    assert "group_size" in err(cfg(group_size=None))[1]
    # groups + HMC (and + NUTS) is a valid configuration: it gets as far as looking for a device
    for over in (dict(), dict(w_nuts=5), dict(w_am=20)):
        rc, msg = err(cfg(**over)) if lib.device_count() == 0 else (-4, "no HIP device")
        assert rc == -4 and "no HIP device" in msg, (over, rc, msg)


def test_signatures_are_unchanged():
    """Groups with gradient jumps need no new keyword: the public signatures are the parent's."""
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
