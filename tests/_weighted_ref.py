"""Yardstick of the prior-weight tests (not a test module).

Per-row prior weights omega_i >= 0 (R's ``glm(weights=)``): eta and mu are
unchanged, the IRLS weight is omega_i w_i, the score sum omega_i (y_i - mu_i)
x_i, Sig_inv = X^T diag(omega w) X at the estimate and the log-likelihood
sum omega_i l_i.  The reference is a numpy fp64 full Newton with step halving
in the style of tests/_poisson_offset_ref.py, for

* the logistic family (y used as given: y = s / m with omega = m is the
  grouped-binomial fit without the binomial-coefficient constant), start 0;
* the Poisson family with an optional per-row offset o, started at
  log(sum omega y / sum omega exp(o)) on the intercept (else 0); l_i includes
  -lgamma(y_i + 1).

tests/test_cpu_weighted.py pins it: omega = 1 against the unweighted
references, integer omega against row replication, grouped binomial against
the expanded 0/1 rows.
"""

import functools

import numpy as np

import _poisson_ref as R

design = R.design


def _softplus(eta):
    return np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta)))


def _expit(t):
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def logistic_loglik(Z, y, w, theta):
    """sum omega (y eta - log(1 + exp(eta)))."""
    eta = Z @ theta
    return float(np.sum(w * (y * eta - _softplus(eta))))


def poisson_loglik(Z, y, w, theta, o=None):
    """sum omega (y eta - mu - lgamma(y + 1)), eta = Z theta (+ o)."""
    from scipy.special import gammaln

    eta = Z @ theta + (0.0 if o is None else o)
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sum(w * (y * eta - np.exp(eta) - gammaln(y + 1.0))))


def poisson_start(y, w, o, P, fit_intercept):
    """The documented start point of the weighted Poisson fit."""
    theta = np.zeros(P)
    if fit_intercept:
        e = np.ones_like(y) if o is None else np.exp(o)
        theta[0] = np.log(np.sum(w * y) / np.sum(w * e))
    return theta


def _newton(Z, theta, ll_of, grad_hess, max_iter):
    """Full Newton, the step halved whenever the log-likelihood falls (by more
    than the rounding of the sum) or is not finite, to max|step| <= 1e-12 (1 +
    max|theta|)."""
    ll = ll_of(theta)
    it = 0
    halvings = 0
    for it in range(1, max_iter + 1):
        g, H = grad_hess(theta)
        d = np.linalg.solve(H, g)
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
    return theta, it, halvings


def logistic_hessian(Z, w, theta):
    mu = _expit(Z @ theta)
    return Z.T @ (Z * (w * mu * (1.0 - mu))[:, None])


def poisson_hessian(Z, w, theta, o=None):
    mu = np.exp(Z @ theta + (0.0 if o is None else o))
    return Z.T @ (Z * (w * mu)[:, None])


def fit_logistic(X, y, w, fit_intercept=False, center=None, scale=None, max_iter=200):
    """One partition.  Returns a dict: theta, sig_inv, sig_inv_theta, loglik, iters."""
    Z = design(X, fit_intercept, center, scale)
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)

    def grad_hess(t):
        mu = _expit(Z @ t)
        return Z.T @ (w * (y - mu)), Z.T @ (Z * (w * mu * (1.0 - mu))[:, None])

    theta, it, _ = _newton(Z, np.zeros(Z.shape[1]), lambda t: logistic_loglik(Z, y, w, t),
                           grad_hess, max_iter)
    H = logistic_hessian(Z, w, theta)
    return {"theta": theta, "sig_inv": H, "sig_inv_theta": H @ theta,
            "loglik": logistic_loglik(Z, y, w, theta), "iters": it}


def fit_poisson(X, y, w, o=None, fit_intercept=False, center=None, scale=None, max_iter=200):
    """One partition, with or without the offset o.  Returns a dict: theta,
    sig_inv, sig_inv_theta, loglik, iters."""
    from scipy.special import gammaln

    Z = design(X, fit_intercept, center, scale)
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    oo = np.zeros_like(y) if o is None else np.asarray(o, dtype=np.float64)
    const = float(np.sum(w * gammaln(y + 1.0)))

    def ll_of(t):  # constant-free, like the fit's step control
        eta = Z @ t + oo
        with np.errstate(over="ignore", invalid="ignore"):
            return float(np.sum(w * (y * eta - np.exp(eta))))

    def grad_hess(t):
        mu = np.exp(Z @ t + oo)
        return Z.T @ (w * (y - mu)), Z.T @ (Z * (w * mu)[:, None])

    theta, it, _ = _newton(Z, poisson_start(y, w, o, Z.shape[1], fit_intercept), ll_of,
                           grad_hess, max_iter)
    H = poisson_hessian(Z, w, theta, oo)
    return {"theta": theta, "sig_inv": H, "sig_inv_theta": H @ theta,
            "loglik": ll_of(theta) - const, "iters": it}


def fit_partitions(family, X, y, w, offsets, o=None, **kw):
    """Stacked per-partition fits of the non-empty partitions (an empty one
    gets zeros): theta [K, P], sig_inv [K, P, P], sig_inv_theta [K, P],
    loglik [K], iters [K]."""
    outs = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b <= a:
            outs.append(None)
        elif family == "logistic":
            outs.append(fit_logistic(X[a:b], y[a:b], w[a:b], **kw))
        else:
            outs.append(fit_poisson(X[a:b], y[a:b], w[a:b],
                                    None if o is None else o[a:b], **kw))
    first = next(v for v in outs if v is not None)
    zero = {k: np.zeros_like(np.asarray(v)) for k, v in first.items()}
    return {k: np.stack([np.asarray((v or zero)[k]) for v in outs]) for k in first}


def replicate(w, *arrays):
    """The row-replicated data of integer weights: row i repeated w_i times
    (rows with w_i = 0 left out)."""
    idx = np.repeat(np.arange(len(w)), np.asarray(w).astype(np.int64))
    return tuple(a[idx] for a in arrays)


def replicate_offsets(w, offsets):
    """Partition boundaries of the replicated rows."""
    cw = np.concatenate([[0], np.cumsum(np.asarray(w).astype(np.int64))])
    return cw[np.asarray(offsets)].astype(np.int64)


def expand_binomial(X, s, m, offsets):
    """Grouped binomial rows (s successes of m trials) as 0/1 rows: row i
    becomes s_i rows with y = 1 then m_i - s_i rows with y = 0."""
    s = np.asarray(s).astype(np.int64)
    m = np.asarray(m).astype(np.int64)
    idx = np.repeat(np.arange(len(m)), m)
    start = np.concatenate([[0], np.cumsum(m)])
    pos = np.arange(idx.size) - start[idx]
    y = (pos < s[idx]).astype(np.float64)
    return X[idx], y, start[np.asarray(offsets)].astype(np.int64)


@functools.lru_cache(maxsize=None)
def weights(n, kind, seed=11):
    """Deterministic weights: "int" in {0, 1, 2, 3}, "spread" in {0, 1, 50},
    "real" ~ U(0.2, 5) with one row in 50 set to exactly 0.

    "spread" puts 50 on one row in 50 (mean weight 1.78), not more: the
    replication tests compare iteration counts, and the fit's schedule depends
    on the row count -- a warm-start level (Newton on a 2048-row prefix of each
    partition first) runs once the prefixes are at most half of all rows.  At
    the suite's partition sizes (7704 rows, P <= 14) that is from 16384 rows
    on, so the replicated rows must stay below a mean weight of 2.1 for both
    sides to run the same schedule (DESIGN.md 4.5f records the counts of a
    heavier spread)."""
    rng = np.random.default_rng(seed + n)
    if kind == "int":
        return rng.integers(0, 4, n).astype(np.float64)
    if kind == "spread":
        return rng.choice([0.0, 1.0, 50.0], n, p=[0.2, 0.78, 0.02])
    w = rng.uniform(0.2, 5.0, n)
    w[rng.integers(0, n, max(1, n // 50))] = 0.0
    return w
