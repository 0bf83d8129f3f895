"""Poisson-regression yardstick of the Poisson tests (not a test module).

The reference project has no Poisson model, so the reference is this numpy
fp64 full-Newton fit: log link, the start point of the HIP fit (log mean y on
the intercept, else 0), the step halved whenever the log-likelihood falls or
is not finite, stopped at max|step| <= 1e-12 (1 + max|theta|);
``scipy.special.gammaln`` for the constant term.  tests/test_cpu_poisson.py
pins it against scikit-learn's PoissonRegressor.
"""

import functools

import numpy as np

import oracle as O


def design(X, fit_intercept=False, center=None, scale=None):
    X = np.asarray(X, dtype=np.float64)
    if center is not None:
        X = (X - np.asarray(center, np.float64)) / np.asarray(scale, np.float64)
    if fit_intercept:
        X = np.column_stack([np.ones(X.shape[0]), X])
    return X


def loglik(Z, y, theta):
    """Full Poisson log-likelihood sum y eta - mu - lgamma(y + 1)."""
    from scipy.special import gammaln

    eta = Z @ theta
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0)))


def fit(X, y, fit_intercept=False, center=None, scale=None, max_iter=200):
    """One partition.  Returns a dict: theta, sig_inv, sig_inv_theta, loglik,
    iters, halvings."""
    from scipy.special import gammaln

    Z = design(X, fit_intercept, center, scale)
    y = np.asarray(y, dtype=np.float64)
    P = Z.shape[1]
    const = float(np.sum(gammaln(y + 1.0)))

    def ll_of(t):
        eta = Z @ t
        with np.errstate(over="ignore", invalid="ignore"):
            return float(np.sum(y * eta - np.exp(eta)))

    theta = np.zeros(P)
    if fit_intercept:
        theta[0] = np.log(y.mean())
    ll = ll_of(theta)
    halvings = 0
    it = 0
    for it in range(1, max_iter + 1):
        mu = np.exp(Z @ theta)
        H = Z.T @ (Z * mu[:, None])
        g = Z.T @ (y - mu)
        d = np.linalg.solve(H, g)
        sc = 1.0
        for _ in range(60):
            cand = theta + sc * d
            llc = ll_of(cand)
            # "falls": by more than the rounding of the sum (at the optimum two
            # evaluations differ in the last bits)
            if np.isfinite(llc) and llc >= ll - 1e-13 * (1.0 + abs(ll)):
                break
            sc *= 0.5
            halvings += 1
        theta, ll = cand, llc
        if np.abs(sc * d).max() <= 1e-12 * (1.0 + np.abs(theta).max()):
            break
    mu = np.exp(Z @ theta)
    H = Z.T @ (Z * mu[:, None])
    return {"theta": theta, "sig_inv": H, "sig_inv_theta": H @ theta,
            "loglik": ll_of(theta) - const, "iters": it, "halvings": halvings}


def fit_partitions(X, y, offsets, **kw):
    """Stacked per-partition fits: theta [K, P], sig_inv [K, P, P],
    sig_inv_theta [K, P], loglik [K], halvings [K]."""
    outs = [fit(X[a:b], y[a:b], **kw) for a, b in zip(offsets[:-1], offsets[1:])]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}


def simulate(n, p, seed, fit_intercept=False, beta=0.5, intercept=1.0, shift0=0.0,
             theta_true=None):
    """X from the counter generator; beta* = ``beta`` on the first
    max(1, floor(0.4 p)) columns (or ``theta_true`` [p]); intercept
    ``intercept`` when fitted; y ~ Poisson(exp(eta)) from default_rng(seed).
    ``shift0`` is added to column 0."""
    X, _ = O.simulate_counter(n, p, seed)
    X = np.ascontiguousarray(X)
    if shift0:
        X[:, 0] += shift0
    if theta_true is None:
        theta_true = np.zeros(p)
        theta_true[:max(1, int(0.4 * p))] = beta
    eta = X @ np.asarray(theta_true, np.float64) + (intercept if fit_intercept else 0.0)
    y = np.random.default_rng(seed).poisson(np.exp(eta)).astype(np.float64)
    return X, y


@functools.lru_cache(maxsize=None)
def case(p, fit_intercept, sizes, seed=7):
    """(X, y, offsets, reference fits) of one shape, computed once per process."""
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X, y = simulate(int(offsets[-1]), p, seed, fit_intercept)
    ref = fit_partitions(X, y, offsets, fit_intercept=fit_intercept)
    return X, y, offsets, ref
