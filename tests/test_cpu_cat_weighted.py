"""Prior weights on the categorical-code layout without a GPU: the C-ABI and
Python surface of dlsa_logistic_fit_categorical_weighted and
dlsa_logistic_loglik_categorical_weighted, the argument check that comes
before the GPU.
"""

import ctypes
import inspect

import numpy as np
import pytest

from test_cpu_weighted import _CTYPES, _header_prototype

PAIRS = [("dlsa_logistic_fit_categorical_weighted", "dlsa_logistic_fit_categorical"),
         ("dlsa_logistic_loglik_categorical_weighted", "dlsa_logistic_loglik_categorical")]
_CTYPES = dict(_CTYPES, **{"const uint8_t*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p})


@pytest.mark.parametrize("new,old", PAIRS)
def test_entries_exported_bound_and_prototyped(new, old):
    """Exported, bound in _hip.SIGNATURES with the header's types, and the
    prototype is the unweighted one plus row_weight after y."""
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
    names = [n for _, n in proto]
    assert names[:5] == ["Xn", "codes", "y", "row_weight", "offsets"]
    assert [x for x in proto if x[1] != "row_weight"] == _header_prototype(old)
    # the unweighted binding is what it was
    assert _hip.SIGNATURES[old][1] == argtypes[:3] + argtypes[4:]


def test_python_surface():
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def names(fn):
        return [p.name for p in inspect.signature(fn).parameters.values()
                if p.kind is not inspect.Parameter.VAR_KEYWORD]

    old = names(M.logistic_model_batched_categorical)
    assert "sample_weight" not in old
    assert old[:5] == ["Xn", "codes", "y", "offsets", "levels"]
    new = names(M.logistic_model_batched_categorical_weighted)
    assert new == old[:5] + ["sample_weight"] + old[5:]
    ev = names(M.logistic_loglik_batched_categorical)
    assert ev[-1] == "sample_weight" and ev[:6] == old[:5] + ["betas"]
    for fn in (M.logistic_model_batched_categorical_weighted,
               M.logistic_loglik_batched_categorical, D.dlsa_fit_sharded, D.loglik_sharded):
        assert inspect.signature(fn).parameters["sample_weight"].default is None, fn.__name__
    # the reference's pandas signatures stay as they are
    for fn in (M.logistic_model, M.logistic_model_eval):
        assert "sample_weight" not in names(fn), fn.__name__


@pytest.mark.parametrize("bad", ["length", "negative", "nan", "inf"])
def test_sample_weight_checked_before_the_gpu(bad, monkeypatch):
    """Every new call path raises ValueError before _require_gpu."""
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def no_gpu(device=None):
        raise AssertionError("the GPU was touched before the sample_weight check")

    monkeypatch.setattr(M, "_require_gpu", no_gpu)
    n, q = 40, 2
    Xn, y = np.zeros((n, q)), np.zeros(n)
    codes = np.zeros((n, 2), np.uint8)
    levels = [3, 2]
    off = np.array([0, n])
    w = np.ones(n)
    if bad == "length":
        w = np.ones(n - 1)
    else:
        w[7] = {"negative": -1.0, "nan": np.nan, "inf": np.inf}[bad]
    betas = np.zeros((1, q + 3))
    calls = [
        lambda: M.logistic_model_batched_categorical_weighted(Xn, codes, y, off, levels, w),
        lambda: M.logistic_model_batched_categorical_weighted(Xn, codes, y, off, levels,
                                                              sample_weight=w, fit_intercept=True),
        lambda: M.logistic_loglik_batched_categorical(Xn, codes, y, off, levels, betas,
                                                      sample_weight=w),
        lambda: D.dlsa_fit_sharded(Xn, y, off, codes=codes, levels=levels, sample_weight=w),
        lambda: D.loglik_sharded(Xn, y, off, betas, codes=codes, levels=levels, sample_weight=w),
    ]
    for c in calls:
        with pytest.raises(ValueError, match="sample_weight"):
            c()
