"""Poisson family, CPU side: the numpy yardstick of tests/_glm_ref.py
against scikit-learn, and the C-ABI declarations of the new entry points."""

import ctypes
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


@pytest.mark.parametrize("p,fi", [(16, False), (33, False), (64, True)])
def test_reference_vs_sklearn(p, fi):
    lm = pytest.importorskip("sklearn.linear_model")
    X, y = G.simulate(1500, p, seed=7, fit_intercept=fi)
    ref = G.fit("poisson", X, y, fit_intercept=fi)
    sk = lm.PoissonRegressor(alpha=0, solver="newton-cholesky", tol=1e-10, max_iter=1000,
                             fit_intercept=fi).fit(X, y)
    coef = np.concatenate([[sk.intercept_], sk.coef_]) if fi else sk.coef_
    print("rel", _rel(ref["theta"], coef), "iters", ref["iters"], "halvings", ref["halvings"])
    assert _rel(ref["theta"], coef) < 1e-9
    # the log-likelihood is the full one: it matches the definition at sklearn's coef
    Z = G.design(X, fi)
    assert abs(ref["loglik"] - G.loglik("poisson", Z, y, coef)) <= 1e-9 * abs(ref["loglik"])
    assert ref["loglik"] >= G.loglik("poisson", Z, y, coef) - 1e-9 * abs(ref["loglik"])


def test_reference_start_and_halving():
    """The overshoot design of the GPU test: the reference has to halve."""
    th = np.zeros(10)
    th[0] = 1.2
    X, y = G.simulate(8000, 10, seed=11, shift0=3.0, theta_true=th)
    ref = G.fit("poisson", X, y)
    print("mean y", y.mean(), "halvings", ref["halvings"], "iters", ref["iters"])
    assert ref["halvings"] >= 1
    assert _rel(ref["theta"], th) < 0.1


def _decl(name):
    txt = open(os.path.join(ROOT, "include", "dlsa_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/dlsa_hip.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("new,old", [
    ("dlsa_poisson_fit_batched_ex", "dlsa_logistic_fit_batched_ex"),
    ("dlsa_poisson_loglik_batched_sum", "dlsa_logistic_loglik_batched_sum")])
def test_header_and_binding(new, old):
    from dlsa_amd import _hip

    assert _decl(new) == _decl(old)  # exactly the logistic argument list
    assert new in _hip.SIGNATURES
    assert _hip.SIGNATURES[new] == _hip.SIGNATURES[old]
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, new), f"{new} not exported"


def test_python_surface():
    import inspect

    from dlsa_amd import distributed, models

    sig = inspect.signature(models.poisson_model_batched)
    assert list(sig.parameters) == [
        "X", "y", "offsets", "fit_intercept", "center", "scale", "max_iter", "tol", "hessian",
        "switch_tol", "record_timing", "rows_per_chunk", "workspace", "device", "exact_waves"]
    assert sig.parameters["hessian"].default == "mixed" and sig.parameters["tol"].default == 1e-10
    # the logistic signature is unchanged
    assert list(inspect.signature(models.logistic_model_batched).parameters)[-3:] == [
        "exact", "exact_waves", "oz_max_bytes"]
    assert inspect.signature(distributed.dlsa_fit_sharded).parameters["family"].default == "logistic"
    with pytest.raises(ValueError):
        distributed.dlsa_fit_sharded(None, None, None, codes=object(), levels=[2], family="poisson")
    with pytest.raises(ValueError):
        distributed.dlsa_fit_sharded(None, None, None, family="gamma")


_LGAMMA_MAIN = r"""
#include <cmath>
#include <cstdio>
#include "dlsa_internal.hpp"
int main() {
  double worst = 0.0;
  for (int i = 0; i <= 600000; ++i) {
    // y in [0, 20] by 1e-4, [20, 1020] by 1e-2, then geometric to ~1e12
    const double y = i < 200000 ? i * 1e-4
                   : i < 300000 ? 20.0 + (i - 200000) * 1e-2
                                : 1020.0 * std::pow(1.00007, i - 300000);
    const double a = dlsa::lgamma1p(y), b = std::lgamma(y + 1.0);
    worst = std::fmax(worst, std::fabs(a - b) / std::fmax(std::fabs(b), 1.0));
  }
  std::printf("%.3e %.17g %.17g\n", worst, dlsa::lgamma1p(0.0), dlsa::lgamma1p(1.0));
  return 0;
}
"""


def test_lgamma1p_host(tmp_path):
    """The kernels' lgamma(y + 1) (dlsa_internal.hpp, host + device code)
    against the C library's on a grid of real y: within 1e-13 of
    max(1, |value|) -- the library's own error is a few ulps, the shifted
    Stirling series' ~1e-14 absolute -- and exactly 0 at y = 0 and y = 1."""
    import subprocess

    from dlsa_amd import build

    src = tmp_path / "lg.cpp"
    src.write_text(_LGAMMA_MAIN)
    exe = tmp_path / "lg"
    subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", "-O2", "-std=c++17", "-x", "hip",
                    "-I" + build.CSRC, "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    print("lgamma1p worst", out)
    assert float(out[0]) < 1e-13
    assert float(out[1]) == 0.0 and float(out[2]) == 0.0
