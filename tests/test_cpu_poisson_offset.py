"""Poisson regression with a per-row offset, CPU side: the numpy yardstick of
tests/_glm_ref.py (Poisson with an offset) against scikit-learn, the C-ABI declarations of
the two new entry points and the Python surface."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import _glm_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("p,fi", [(1, True), (16, False), (33, False)])
def test_reference_vs_sklearn(p, fi):
    """A Poisson fit with offset log E has the MLE of the rate model: y / E
    with sample_weight E."""
    lm = pytest.importorskip("sklearn.linear_model")
    X, y, o = G.simulate_offset(3001, p, fit_intercept=fi)
    E = np.exp(o)
    assert E.min() >= 0.2 * (1 - 1e-12) and E.max() <= 5.0 * (1 + 1e-12)
    ref = G.fit("poisson", X, y, o=o, fit_intercept=fi)
    sk = lm.PoissonRegressor(alpha=0, solver="newton-cholesky", tol=1e-10, max_iter=1000,
                             fit_intercept=fi).fit(X, y / E, sample_weight=E)
    coef = np.concatenate([[sk.intercept_], sk.coef_]) if fi else sk.coef_
    print("rel", _rel(ref["theta"], coef), "iters", ref["iters"], "halvings", ref["halvings"])
    assert _rel(ref["theta"], coef) < 1e-9
    # the offset matters on this data: the fit that ignores it is somewhere else
    assert _rel(G.fit("poisson", X, y, fit_intercept=fi)["theta"], ref["theta"]) > 1e-3


def test_reference_start_and_outputs():
    X, y, o = G.simulate_offset(2000, 5, fit_intercept=True)
    Z = G.design(X, True)
    t0 = G.start("poisson", y, 6, True, o=o)
    # the intercept-only rate MLE: its score sum(y - exp(t0 + o)) vanishes
    assert abs(np.sum(y - np.exp(t0[0] + o))) < 1e-9 * y.sum() and not t0[1:].any()
    assert not G.start("poisson", y, 5, False, o=o).any()
    ref = G.fit("poisson", X, y, o=o, fit_intercept=True)
    mu = np.exp(Z @ ref["theta"] + o)
    assert np.abs(Z.T @ (y - mu)).max() < 1e-7 * y.sum()
    assert _rel(ref["sig_inv"], Z.T @ (Z * mu[:, None])) < 1e-14
    ll = G.loglik("poisson", Z, y, ref["theta"], o=o)
    assert abs(ref["loglik"] - ll) < 1e-12 * abs(ref["loglik"])


def _decl(name):
    txt = open(os.path.join(ROOT, "include", "dlsa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/dlsa_hip.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("new,old", [
    ("dlsa_poisson_fit_batched_offset", "dlsa_poisson_fit_batched_ex"),
    ("dlsa_poisson_loglik_batched_sum_offset", "dlsa_poisson_loglik_batched_sum")])
def test_header_and_binding(new, old):
    from dlsa_amd import _hip

    want = _decl(old)
    assert want[1] == "const double* y"
    want.insert(2, "const double* eta_offset")  # right after y
    assert _decl(new) == want
    assert new in _hip.SIGNATURES
    res, args = _hip.SIGNATURES[old]
    assert _hip.SIGNATURES[new] == (res, args[:2] + [ctypes.c_void_p] + args[2:])
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, new), f"{new} not exported"


def test_python_surface():
    from dlsa_amd import distributed, models

    old = list(inspect.signature(models.poisson_model_batched).parameters)
    assert old == ["X", "y", "offsets", "fit_intercept", "center", "scale", "max_iter", "tol",
                   "hessian", "switch_tol", "record_timing", "rows_per_chunk", "workspace",
                   "device", "exact_waves"]  # unchanged
    sig = inspect.signature(models.poisson_model_batched_offset)
    assert list(sig.parameters) == old[:3] + ["eta_offset", "exposure"] + old[3:]
    for k in old[3:]:
        assert sig.parameters[k].default == \
            inspect.signature(models.poisson_model_batched).parameters[k].default
    assert sig.parameters["eta_offset"].default is None
    assert sig.parameters["exposure"].default is None
    old_ll = list(inspect.signature(models.poisson_loglik_batched).parameters)
    assert old_ll == ["X", "y", "offsets", "betas", "fit_intercept", "center", "scale", "device",
                      "return_sum"]
    sig = inspect.signature(models.poisson_loglik_batched_offset)
    assert list(sig.parameters) == old_ll[:4] + ["eta_offset", "exposure"] + old_ll[4:]
    sh = inspect.signature(distributed.dlsa_fit_sharded).parameters
    assert sh["eta_offset"].default is None and sh["exposure"].default is None
    assert sh["family"].default == "logistic"


def test_value_errors():
    from dlsa_amd import distributed, models

    X, y, off = np.zeros((6, 2)), np.ones(6), [0, 6]
    E = np.full(6, 2.0)
    betas = np.zeros((1, 2))
    fits = [lambda **kw: models.poisson_model_batched_offset(X, y, off, **kw),
            lambda **kw: models.poisson_loglik_batched_offset(X, y, off, betas, **kw),
            lambda **kw: distributed.dlsa_fit_sharded(X, y, off, family="poisson", **kw)]
    for f in fits:
        with pytest.raises(ValueError):
            f(eta_offset=np.log(E), exposure=E)  # both
        with pytest.raises(ValueError):
            f(eta_offset=np.zeros(5))  # wrong length
        with pytest.raises(ValueError):
            f(exposure=np.full(7, 1.0))
        for bad in (0.0, -1.0, np.nan, np.inf):
            Eb = E.copy()
            Eb[3] = bad
            with pytest.raises(ValueError):
                f(exposure=Eb)
    # the offset is the Poisson family's
    with pytest.raises(ValueError):
        distributed.dlsa_fit_sharded(X, y, off, eta_offset=np.zeros(6))
    with pytest.raises(ValueError):
        distributed.dlsa_fit_sharded(X, y, off, family="logistic", exposure=E)


def test_fails_loudly_without_gpu():
    import torch

    from dlsa_amd import DlsaHipError, distributed, models

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    X, y, off = np.zeros((6, 2)), np.ones(6), [0, 6]
    with pytest.raises(DlsaHipError):
        models.poisson_model_batched_offset(X, y, off, exposure=np.full(6, 2.0))
    with pytest.raises(DlsaHipError):
        models.poisson_model_batched_offset(X, y, off)
    with pytest.raises(DlsaHipError):
        models.poisson_loglik_batched_offset(X, y, off, np.zeros((1, 2)), eta_offset=np.zeros(6))
    with pytest.raises(DlsaHipError):
        distributed.dlsa_fit_sharded(X, y, off, family="poisson", eta_offset=np.zeros(6))
