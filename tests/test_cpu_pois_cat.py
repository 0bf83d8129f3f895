"""Poisson regression on the categorical-code layout without a GPU: the C-ABI
and Python surface of dlsa_poisson_fit_categorical and
dlsa_poisson_loglik_categorical, and the argument checks that come before the
GPU.
"""

import ctypes
import inspect

import numpy as np
import pytest

from test_cpu_weighted import _CTYPES, _header_prototype

PAIRS = [("dlsa_poisson_fit_categorical", "dlsa_logistic_fit_categorical"),
         ("dlsa_poisson_loglik_categorical", "dlsa_logistic_loglik_categorical")]
_CTYPES = dict(_CTYPES, **{"const uint8_t*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p})
EXTRAS = ("eta_offset", "row_weight")


@pytest.mark.parametrize("new,old", PAIRS)
def test_entries_exported_bound_and_prototyped(new, old):
    """Exported, bound in _hip.SIGNATURES with the header's types, and the
    prototype is the logistic sibling's plus eta_offset and row_weight (both
    const double*, the offset first) after y."""
    from dlsa_amd import _hip

    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, new), f"libdlsa_hip.so does not export {new}"
    assert new in _hip.SIGNATURES, f"_hip.py does not bind {new}"
    proto = _header_prototype(new)
    res, argtypes = _hip.SIGNATURES[new]
    assert res is ctypes.c_int
    want = [ctypes.POINTER(_hip.FitOptions) if t == "const dlsa_fit_options*" else _CTYPES[t]
            for t, _ in proto]
    assert argtypes == want, (new, [n for _, n in proto])
    assert [n for _, n in proto][:6] == ["Xn", "codes", "y", "eta_offset", "row_weight", "offsets"]
    assert proto[3][0] == proto[4][0] == "const double*"
    assert [x for x in proto if x[1] not in EXTRAS] == _header_prototype(old)
    # the logistic binding is what it was
    assert _hip.SIGNATURES[old][1] == argtypes[:3] + argtypes[5:]


def _names(fn):
    return [p.name for p in inspect.signature(fn).parameters.values()
            if p.kind is not inspect.Parameter.VAR_KEYWORD]


def test_python_surface():
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    assert _names(M.poisson_model_batched_categorical) == [
        "Xn", "codes", "y", "offsets", "levels", "sample_weight", "eta_offset", "exposure",
        "fit_intercept", "center", "scale", "max_iter", "tol", "record_timing", "rows_per_chunk",
        "zero_partitions", "device"]
    assert _names(M.poisson_loglik_batched_categorical) == [
        "Xn", "codes", "y", "offsets", "levels", "betas", "sample_weight", "eta_offset",
        "exposure", "fit_intercept", "center", "scale", "rows_per_chunk", "device", "return_sum"]
    d = {k: v.default for k, v in
         inspect.signature(M.poisson_model_batched_categorical).parameters.items()}
    assert (d["sample_weight"], d["eta_offset"], d["exposure"], d["fit_intercept"], d["center"],
            d["scale"], d["max_iter"], d["tol"], d["record_timing"], d["rows_per_chunk"],
            d["zero_partitions"], d["device"]) == (None, None, None, False, None, None, 100,
                                                   1e-10, False, 0, None, None)
    # sample_weight stays the last named parameter of the sharded drivers;
    # loglik_sharded's new parameters come before it
    assert _names(D.dlsa_fit_sharded)[-1] == "sample_weight"
    ls = _names(D.loglik_sharded)
    assert ls[-4:] == ["family", "eta_offset", "exposure", "sample_weight"]
    p = inspect.signature(D.loglik_sharded).parameters
    assert p["family"].default == "logistic"
    assert p["eta_offset"].default is None and p["exposure"].default is None
    # the logistic functions keep their parameter lists
    assert "eta_offset" not in _names(M.logistic_model_batched_categorical_weighted)
    assert _names(M.logistic_loglik_batched_categorical)[-1] == "sample_weight"


def _calls(M, D, Xn, codes, y, off, levels, betas, **kw):
    return [
        lambda: M.poisson_model_batched_categorical(Xn, codes, y, off, levels, **kw),
        lambda: M.poisson_model_batched_categorical(Xn, codes, y, off, levels, fit_intercept=True,
                                                    **kw),
        lambda: M.poisson_loglik_batched_categorical(Xn, codes, y, off, levels, betas, **kw),
        lambda: D.dlsa_fit_sharded(Xn, y, off, codes=codes, levels=levels, family="poisson", **kw),
        lambda: D.loglik_sharded(Xn, y, off, betas, codes=codes, levels=levels, family="poisson",
                                 **kw),
    ]


@pytest.mark.parametrize("what,bad", [
    ("sample_weight", "length"), ("sample_weight", "negative"), ("sample_weight", "nan"),
    ("sample_weight", "inf"), ("eta_offset", "length"), ("exposure", "length"),
    ("exposure", "zero"), ("exposure", "negative"), ("exposure", "nan"), ("exposure", "inf"),
    ("both", None), ("Xn", None)])
def test_arguments_checked_before_the_gpu(what, bad, monkeypatch):
    """Every new call path raises ValueError before _require_gpu for a bad
    weight, offset, exposure or Xn."""
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def no_gpu(device=None):
        raise AssertionError(f"the GPU was touched before the {what} check")

    monkeypatch.setattr(M, "_require_gpu", no_gpu)
    n, q = 40, 2
    Xn, y = np.zeros((n, q)), np.zeros(n)
    codes = np.zeros((n, 2), np.uint8)
    levels = [3, 2]
    off = np.array([0, n])
    betas = np.zeros((1, q + 3))
    kw, match = {}, what
    if what == "both":
        kw, match = dict(eta_offset=np.zeros(n), exposure=np.ones(n)), "not both"
    elif what == "Xn":
        Xn, match = np.zeros(n), "Xn must be 2-D"
    else:
        v = np.ones(n - 1 if bad == "length" else n)
        if bad != "length":
            v[7] = {"negative": -1.0, "nan": np.nan, "inf": np.inf, "zero": 0.0}[bad]
        kw = {what: v}
        if what != "sample_weight":
            match = "eta_offset / exposure" if bad == "length" else "exposure"
    for c in _calls(M, D, Xn, codes, y, off, levels, betas, **kw):
        with pytest.raises(ValueError, match=match):
            c()


def test_dense_poisson_loglik_sharded_checked_before_the_gpu(monkeypatch):
    """loglik_sharded(family="poisson") without codes is the dense weighted
    Poisson evaluation, with its checks; the offset needs that family."""
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def no_gpu(device=None):
        raise AssertionError("the GPU was touched before the argument check")

    monkeypatch.setattr(M, "_require_gpu", no_gpu)
    n = 30
    X, y, off, betas = np.zeros((n, 3)), np.zeros(n), np.array([0, n]), np.zeros((1, 3))
    with pytest.raises(ValueError, match="exposure"):
        D.loglik_sharded(X, y, off, betas, family="poisson", exposure=np.zeros(n))
    with pytest.raises(ValueError, match="sample_weight"):
        D.loglik_sharded(X, y, off, betas, family="poisson", sample_weight=-np.ones(n))
    with pytest.raises(ValueError, match="family='poisson'"):
        D.loglik_sharded(X, y, off, betas, eta_offset=np.zeros(n))
    with pytest.raises(ValueError, match="family must be"):
        D.loglik_sharded(X, y, off, betas, family="gamma")
