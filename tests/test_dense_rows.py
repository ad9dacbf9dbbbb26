"""The dense-rows feature's surface, checked without a GPU: the C ABI's new entry points are declared and bound, PTEngine takes
``rows_logl``, and PTSampler decides by itself when the built-in likelihood runs as a row kernel on the split path."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_points_are_declared_and_bound():
    from ptmcmcsampler_amd import _lib
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    for name in ("ptmi_rows_logl_grad", "ptmi_rows_logp"):
        assert name in _lib.SYMBOLS
        assert re.search(r"^int %s\(ptmi_handle h, const double \*rows" % name, header, re.M), name
    src = open(os.path.join(ROOT, "ptmcmcsampler_amd", "_build.py")).read()
    assert "ptmi_dense_rows.hip" in src and os.path.isfile(os.path.join(ROOT, "ptmcmcsampler_amd", "csrc", "ptmi_dense_rows.hip"))


def test_engine_accepts_rows_logl():
    from ptmcmcsampler_amd.engine import PTEngine
    p = inspect.signature(PTEngine.__init__).parameters
    assert "rows_logl" in p and p["rows_logl"].default is False
    for name in ("builtin_logl", "builtin_logl_grad", "builtin_logp", "builtin_logp_grad"):
        assert callable(getattr(PTEngine, name))


def _sampler(tmp_path, ndim, logl, logp, **kw):
    from ptmcmcsampler_amd import PTSampler
    return PTSampler(ndim, logl, logp, np.eye(ndim), outDir=str(tmp_path), verbose=False, **kw)


def test_sampler_resolves_rows_logl(tmp_path):
    dense = lambda d: ("dense", np.zeros(d), np.eye(d))  # noqa: E731
    box = lambda d: ("box", -np.ones(d), np.ones(d))  # noqa: E731
    assert _sampler(tmp_path, 100, dense(100), ("flat",)).rows_logl is False
    assert _sampler(tmp_path, 104, dense(104), box(104)).rows_logl is False
    assert _sampler(tmp_path, 105, dense(105), ("flat",)).rows_logl is True
    assert _sampler(tmp_path, 105, dense(105), box(105)).rows_logl is True
    assert _sampler(tmp_path, 1000, ("iso",), ("flat",)).rows_logl is False
    # opt out / force
    assert _sampler(tmp_path, 105, dense(105), ("flat",), rows_logl=False).rows_logl is False
    assert _sampler(tmp_path, 10, dense(10), ("flat",), rows_logl=True).rows_logl is True
    assert _sampler(tmp_path, 1000, ("iso",), ("flat",), rows_logl=True).rows_logl is True
    # a Python-callable likelihood has no row kernel: refused before any engine is built
    for kw in (dict(), dict(batched=True)):
        with pytest.raises(ValueError, match="rows_logl"):
            _sampler(tmp_path, 105, lambda x: 0.0, lambda x: 0.0, rows_logl=True, **kw)
    with pytest.raises(ValueError, match="rows_logl"):
        _sampler(tmp_path, 6, ("curved",), ("flat",), rows_logl=True)
    s = _sampler(tmp_path, 105, lambda x: 0.0, lambda x: 0.0)
    assert s.rows_logl is False and s.engine is None
