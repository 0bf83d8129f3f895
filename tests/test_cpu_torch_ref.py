"""CPU: tests/_torch_ref.py, the torch fp64 yardstick of the tests whose data
stays on the device, pinned against the numpy yardsticks it restates
(tests/_glm_ref.py, _gram_ref.py, _gof_ref.py) on data small enough for both:
n = 5000 rows (78 slabs of 64 and a tail of 8), p = 7, both families, with and
without the row extras and the intercept.  Agreement to 1e-13 relative: both
sides are fp64 sums of a few thousand terms in different orders."""

import numpy as np
import pytest
import torch

import _glm_ref as G
import _gof_ref as GOF
import _gram_ref as GR
import _torch_ref as T

N, P_COLS, REL = 5000, 7, 1e-13


def _case(family, extras, fi):
    rng = np.random.default_rng(3)
    X = rng.uniform(-0.5, 0.5, (N, P_COLS))
    theta = rng.uniform(-1, 1, P_COLS + fi)
    o = rng.uniform(np.log(0.2), np.log(5.0), N) if extras and family == "poisson" else None
    w = G.weights(N, "real") if extras else None
    Z = G.design(X, fi)
    eta = Z @ theta + (0.0 if o is None else o)
    y = rng.poisson(np.exp(eta)).astype(float) if family == "poisson" else \
        (rng.uniform(size=N) < G._expit(eta)).astype(float)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return (Z, y, theta, w, o), (t(X), t(y), 0, N, t(theta), bool(fi), t(w), t(o))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("fi", [0, 1])
@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_against_numpy(family, extras, fi):
    (Z, y, theta, w, o), targs = _case(family, extras, fi)
    H, g, ll = T.fit_quantities(family, *targs)
    gw, Hw = G.grad_hess(family, Z, y, theta, w, o)
    assert _rel(H, Hw) < REL and np.abs(g.numpy() - gw).max() < REL * np.abs(Z).T.dot(np.ones(N)).max()
    assert abs(ll / G.loglik(family, Z, y, theta, w, o) - 1) < REL
    assert abs(T.loglik(family, *targs) / G.loglik(family, Z, y, theta, w, o) - 1) < REL
    for kind in ("score", "information"):
        Gm, sc, scale = T.gram(family, *targs, kind=kind)
        Gn, sn, scale_n = GR.gram(family, Z, y, theta, w, o, kind)
        assert _rel(Gm, Gn) < REL and np.abs(sc.numpy() - sn).max() < REL * scale_n
        assert abs(scale / scale_n - 1) < REL
    dev, chi, npos = T.gof(family, *targs)
    dn, cn, nn = GOF.gof(family, Z, y, theta, w, o)
    assert abs(dev / dn - 1) < REL and abs(chi / cn - 1) < REL and npos == nn
    if not extras:
        X, yt, a, b, th, fit_i = targs[:6]
        g2, ll2 = T.score_and_loglik(family, X, yt, a, b, th, fit_i)
        assert torch.equal(g2, g) and ll2 == ll


def test_ols_quantities():
    (Z, y, theta, _, _), targs = _case("logistic", False, 1)
    g, rss = T.score_and_loglik("ols", *targs[:6])
    r = y - Z @ theta
    assert np.abs(g.numpy() - Z.T @ r).max() < REL * N and abs(rss / (r @ r) - 1) < REL
