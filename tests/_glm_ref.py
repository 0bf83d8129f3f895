"""The numpy yardstick of the GLM tests (not a test module): logistic and
Poisson regression with optional per-row prior weights and, for Poisson, an
optional per-row offset -- one implementation in every configuration.

The reference project has no Poisson model and no prior weights, so the
reference is this fp64 full-Newton fit:

* eta = Z theta (+ o, a known per-row offset: log exposure); logistic mu =
  expit(eta), Poisson mu = exp(eta);
* per-row prior weights omega_i >= 0 (R's ``glm(weights=)``): the IRLS weight
  is omega_i w_i, the score sum omega_i (y_i - mu_i) x_i, Sig_inv = X^T
  diag(omega w) X at the estimate and the log-likelihood sum omega_i l_i
  (Poisson l_i includes -lgamma(y_i + 1), ``scipy.special.gammaln``; logistic
  y is used as given: y = s / m with omega = m is the grouped-binomial fit
  without the binomial-coefficient constant);
* the start point of the HIP fit: logistic 0; Poisson log(sum omega y / sum
  omega exp(o)) on the intercept, else 0;
* the step halved whenever the log-likelihood falls (by more than the rounding
  of the sum) or is not finite, stopped at max|step| <= 1e-12 (1 + max|theta|).

No weights means omega = 1 and no offset o = 0, which change no bit of any
product or sum.  tests/test_cpu_poisson.py, test_cpu_poisson_offset.py and
test_cpu_weighted.py pin it: against scikit-learn's PoissonRegressor with and
without exposure, omega = 1 against the unweighted fit, integer omega against
row replication, grouped binomial against the expanded 0/1 rows.
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


def _softplus(eta):
    return np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta)))


def _expit(t):
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _omega(w, n):
    return np.ones(n) if w is None else np.asarray(w, dtype=np.float64)


def _terms(family, y, eta):
    """The rows' log-likelihood terms without the Poisson constant."""
    if family == "logistic":
        return y * eta - _softplus(eta)
    with np.errstate(over="ignore", invalid="ignore"):
        return y * eta - np.exp(eta)


def loglik(family, Z, y, theta, w=None, o=None):
    """The full log-likelihood sum omega l_i at theta: logistic l = y eta -
    log(1 + exp(eta)), Poisson l = y eta - mu - lgamma(y + 1); eta = Z theta (+ o)."""
    eta = Z @ theta + (0.0 if o is None else o)
    t = _terms(family, y, eta)
    if family == "poisson":
        from scipy.special import gammaln

        t = t - gammaln(y + 1.0)
    return float(np.sum(_omega(w, len(y)) * t))


def _mu_w(family, Z, theta, om, o):
    """(mu, omega times the IRLS weight) of the rows at theta."""
    eta = Z @ theta + (0.0 if o is None else o)
    if family == "logistic":
        mu = _expit(eta)
        return mu, om * mu * (1.0 - mu)
    mu = np.exp(eta)
    return mu, om * mu


def grad_hess(family, Z, y, theta, w=None, o=None):
    om = _omega(w, len(y))
    mu, v = _mu_w(family, Z, theta, om, o)
    return Z.T @ (om * (y - mu)), Z.T @ (Z * v[:, None])


def hessian(family, Z, theta, w=None, o=None):
    """Sig_inv = Z^T diag(omega w) Z at theta."""
    _, v = _mu_w(family, Z, theta, _omega(w, Z.shape[0]), o)
    return Z.T @ (Z * v[:, None])


def newton_step(family, Z, y, theta, w=None, o=None):
    """The exact fp64 Newton step at theta."""
    g, H = grad_hess(family, Z, y, theta, w, o)
    return np.linalg.solve(H, g)


def start(family, y, P, fit_intercept, w=None, o=None):
    """The documented start point of the fit."""
    theta = np.zeros(P)
    if family == "poisson" and fit_intercept:
        om = _omega(w, len(y))
        e = np.ones_like(y) if o is None else np.exp(o)
        theta[0] = np.log(np.sum(om * y) / np.sum(om * e))
    return theta


def fit(family, X, y, w=None, o=None, fit_intercept=False, center=None, scale=None,
        max_iter=200):
    """One partition.  Returns a dict: theta, sig_inv, sig_inv_theta, loglik,
    iters, halvings."""
    Z = design(X, fit_intercept, center, scale)
    y = np.asarray(y, dtype=np.float64)
    om = _omega(w, len(y))
    oo = None if o is None else np.asarray(o, dtype=np.float64)

    def ll_of(t):  # constant-free, like the fit's step control
        return float(np.sum(om * _terms(family, y, Z @ t + (0.0 if oo is None else oo))))

    theta = start(family, y, Z.shape[1], fit_intercept, om, oo)
    ll = ll_of(theta)
    halvings = 0
    it = 0
    for it in range(1, max_iter + 1):
        d = newton_step(family, Z, y, theta, om, oo)
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
    H = hessian(family, Z, theta, om, oo)
    const = 0.0
    if family == "poisson":
        from scipy.special import gammaln

        const = float(np.sum(om * gammaln(y + 1.0)))
    return {"theta": theta, "sig_inv": H, "sig_inv_theta": H @ theta,
            "loglik": ll_of(theta) - const, "iters": it, "halvings": halvings}


def fit_partitions(family, X, y, offsets, w=None, o=None, **kw):
    """Stacked per-partition fits of the non-empty partitions (an empty one
    gets zeros): theta [K, P], sig_inv [K, P, P], sig_inv_theta [K, P],
    loglik [K], iters [K], halvings [K]."""
    outs = [fit(family, X[a:b], y[a:b], None if w is None else w[a:b],
                None if o is None else o[a:b], **kw) if b > a else None
            for a, b in zip(offsets[:-1], offsets[1:])]
    first = next(v for v in outs if v is not None)
    zero = {k: np.zeros_like(np.asarray(v)) for k, v in first.items()}
    return {k: np.stack([np.asarray((v or zero)[k]) for v in outs]) for k in first}


def simulate(n, p, seed, fit_intercept=False, beta=0.5, intercept=1.0, shift0=0.0,
             theta_true=None):
    """Poisson data.  X from the counter generator; beta* = ``beta`` on the
    first max(1, floor(0.4 p)) columns (or ``theta_true`` [p]); intercept
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


def simulate_offset(n, p, fit_intercept=False, seed=7):
    """Poisson data with an offset.  X of simulate(seed); o = log E with log E
    ~ U(log 0.2, log 5) from default_rng(1000 + p); y ~ Poisson(exp(x . beta*
    + [1] + o)) from default_rng(7), beta* = 0.5 on the first max(1, floor(0.4
    p)) columns."""
    X, _ = simulate(n, p, seed, fit_intercept)
    o = np.random.default_rng(1000 + p).uniform(np.log(0.2), np.log(5.0), n)
    beta = np.zeros(p)
    beta[:max(1, int(0.4 * p))] = 0.5
    eta = X @ beta + (1.0 if fit_intercept else 0.0) + o
    y = np.random.default_rng(7).poisson(np.exp(eta)).astype(np.float64)
    return X, y, o


@functools.lru_cache(maxsize=None)
def case(p, fit_intercept, sizes, seed=7):
    """(X, y, offsets, reference fits) of one Poisson shape, computed once per process."""
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X, y = simulate(int(offsets[-1]), p, seed, fit_intercept)
    ref = fit_partitions("poisson", X, y, offsets, fit_intercept=fit_intercept)
    return X, y, offsets, ref


@functools.lru_cache(maxsize=None)
def case_offset(p, fit_intercept, sizes):
    """(X, y, o, offsets, reference fits) of one Poisson shape with an offset,
    computed once per process."""
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X, y, o = simulate_offset(int(offsets[-1]), p, fit_intercept)
    ref = fit_partitions("poisson", X, y, offsets, o=o, fit_intercept=fit_intercept)
    return X, y, o, offsets, ref


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
