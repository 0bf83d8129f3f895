"""Yardstick of the Poisson-with-offset tests (not a test module).

The model is log mu_i = x_i . theta + o_i with a known per-row offset o
(log exposure).  The reference project has no Poisson model, so the reference
is the numpy fp64 full-Newton fit of tests/_poisson_ref.py with three
differences: eta = Z theta + o, the start point log(sum y / sum exp(o)) on the
intercept (else 0), and otherwise the same halving and stopping rules.
tests/test_cpu_poisson_offset.py pins it against scikit-learn's
PoissonRegressor on y / E with sample_weight = E, which has the same MLE.
"""

import functools

import numpy as np

import _poisson_ref as R

design = R.design


def start(y, o, P, fit_intercept):
    """The documented start point of the fit."""
    theta = np.zeros(P)
    if fit_intercept:
        theta[0] = np.log(y.sum() / np.exp(o).sum())
    return theta


def loglik(Z, y, o, theta):
    """Full log-likelihood sum y eta - mu - lgamma(y + 1), eta = Z theta + o."""
    from scipy.special import gammaln

    eta = Z @ theta + o
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0)))


def hessian(Z, o, theta):
    mu = np.exp(Z @ theta + o)
    return Z.T @ (Z * mu[:, None])


def newton_step(Z, y, o, theta):
    """The exact fp64 Newton step at theta."""
    mu = np.exp(Z @ theta + o)
    return np.linalg.solve(Z.T @ (Z * mu[:, None]), Z.T @ (y - mu))


def fit(X, y, o, fit_intercept=False, center=None, scale=None, max_iter=200):
    """One partition.  Returns a dict: theta, sig_inv, sig_inv_theta, loglik,
    iters, halvings."""
    from scipy.special import gammaln

    Z = design(X, fit_intercept, center, scale)
    y = np.asarray(y, dtype=np.float64)
    o = np.asarray(o, dtype=np.float64)
    const = float(np.sum(gammaln(y + 1.0)))

    def ll_of(t):
        eta = Z @ t + o
        with np.errstate(over="ignore", invalid="ignore"):
            return float(np.sum(y * eta - np.exp(eta)))

    theta = start(y, o, Z.shape[1], fit_intercept)
    ll = ll_of(theta)
    halvings = 0
    it = 0
    for it in range(1, max_iter + 1):
        d = newton_step(Z, y, o, theta)
        sc = 1.0
        for _ in range(60):
            cand = theta + sc * d
            llc = ll_of(cand)
            if np.isfinite(llc) and llc >= ll - 1e-13 * (1.0 + abs(ll)):
                break
            sc *= 0.5
            halvings += 1
        theta, ll = cand, llc
        if np.abs(sc * d).max() <= 1e-12 * (1.0 + np.abs(theta).max()):
            break
    H = hessian(Z, o, theta)
    return {"theta": theta, "sig_inv": H, "sig_inv_theta": H @ theta,
            "loglik": ll_of(theta) - const, "iters": it, "halvings": halvings}


def fit_partitions(X, y, o, offsets, **kw):
    outs = [fit(X[a:b], y[a:b], o[a:b], **kw) for a, b in zip(offsets[:-1], offsets[1:])]
    return {k: np.stack([np.asarray(v[k]) for v in outs]) for k in outs[0]}


def simulate(n, p, fit_intercept=False, seed=7):
    """X of R.simulate(seed); o = log E with log E ~ U(log 0.2, log 5) from
    default_rng(1000 + p); y ~ Poisson(exp(x . beta* + [1] + o)) from
    default_rng(7), beta* = 0.5 on the first max(1, floor(0.4 p)) columns."""
    X, _ = R.simulate(n, p, seed, fit_intercept)
    o = np.random.default_rng(1000 + p).uniform(np.log(0.2), np.log(5.0), n)
    beta = np.zeros(p)
    beta[:max(1, int(0.4 * p))] = 0.5
    eta = X @ beta + (1.0 if fit_intercept else 0.0) + o
    y = np.random.default_rng(7).poisson(np.exp(eta)).astype(np.float64)
    return X, y, o


@functools.lru_cache(maxsize=None)
def case(p, fit_intercept, sizes):
    """(X, y, o, offsets, reference fits) of one shape, computed once per process."""
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X, y, o = simulate(int(offsets[-1]), p, fit_intercept)
    ref = fit_partitions(X, y, o, offsets, fit_intercept=fit_intercept)
    return X, y, o, offsets, ref
