"""eig_mode="ql" beyond 128 parameters (ptmi_eig_ql's wide kernels, csrc/ptmi_eig_wide.hip): the yardstick at the new sizes -- the
oracle's orc_eig_ql against LAPACK at 129, 257 and 513 -- and what the public interface promises (no GPU needed)."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spd(d, rs, floor=0.1):
    A = rs.randn(d, d)
    c = A @ A.T / d + floor * np.eye(d)
    return (c + c.T) / 2


@pytest.mark.parametrize("d", [129, 257, 513])
def test_oracle_ql_factorizes_like_lapack_beyond_128(d):
    rs = np.random.RandomState(d)
    cov = _spd(d, rs) * 10.0 ** rs.uniform(-6, 3)
    Ut, S, iters = orc.eig_ql(cov)
    assert iters > 0
    scale = np.abs(cov).max()
    assert np.abs(Ut.T @ np.diag(S) @ Ut - cov).max() <= 1e-12 * scale
    assert np.abs(Ut @ Ut.T - np.eye(d)).max() <= 1e-12
    assert (np.diff(S) <= 0).all() and (S >= 0).all()
    w = np.linalg.svd(cov, compute_uv=False)
    assert np.abs(S - w).max() <= 1e-12 * w.max()
    big = np.abs(Ut).argmax(axis=1)
    assert (Ut[np.arange(d), big] > 0).all()                                    # the sign rule
    # the nearly degenerate spectrum an isotropic target adapts to
    X = rs.randn(3000, d)
    C = np.cov(X.T)
    Ut, S, iters = orc.eig_ql(C)
    assert np.abs(Ut.T @ np.diag(S) @ Ut - C).max() <= 1e-12 * np.abs(C).max()
    assert np.abs(Ut @ Ut.T - np.eye(d)).max() <= 1e-12
    assert (np.diff(S) <= 0).all()
    assert 0 < iters <= 3 * d + 3


def test_header_names_the_bound_the_budget_and_the_hook():
    txt = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    doc = txt[txt.index("int ptmi_eig_jacobi(ptmi_handle h);"):txt.index("int ptmi_eig_ql_from(")]
    assert "1024" in doc and "4096 MB" in doc and "PTMI_QL_SPLIT = 0" in doc
    assert not re.search(r"ndim <= 128\)", doc)


def test_constructor_signatures_are_unchanged():
    from ptmcmcsampler_amd.engine import PTEngine
    from ptmcmcsampler_amd.sampler import PTSampler
    eng = inspect.signature(PTEngine.__init__).parameters
    smp = inspect.signature(PTSampler.__init__).parameters
    assert eng["eig_mode"].default == "lapack" and smp["eig_mode"].default == "lapack"
    assert list(eng) == ["self", "ndim", "ntemps", "nwalkers", "cov0", "ladder", "logl", "logp", "weights", "cov_update", "burn", "tskip", "seed",
                         "cov_mode", "hot_chain", "Tmin", "Tmax", "ntemps_global", "temp0", "walker0", "device", "split", "use_de_buffer",
                         "w_host", "keep_lnl", "groups", "swap_mode", "grad_weights", "hmc", "nuts_delta", "nuts_maxdepth", "pick_mode",
                         "eig_mode", "am_mode", "eig_lag", "stats_async", "split_nuts", "rows_logl", "jumps"]
    assert list(smp) == ["self", "ndim", "logl", "logp", "cov", "groups", "loglargs", "loglkwargs", "logpargs", "logpkwargs", "logl_grad",
                         "logp_grad", "comm", "outDir", "verbose", "resume", "seed", "nwalkers", "ntemps", "device", "cov_mode", "keep_walkers",
                         "swap_mode", "pick_mode", "eig_mode", "checkpoint", "batched", "nuts_maxdepth", "batched_nuts", "rows_logl"]
