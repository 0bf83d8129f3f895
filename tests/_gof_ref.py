"""The numpy yardstick of the goodness-of-fit tests (not a test module): the
fp64 statements of a GLM row's deviance and Pearson chi-square in the forms the
kernels use, which do not cancel where the fit is good, their per-partition
sums, the count of rows with a positive weight and the Pearson dispersion
estimate.  Designs, fits and data are tests/_glm_ref.py's.

With eta = Z theta (+ o), prior weights omega (1 without), y as given:

* Poisson, mu = exp(eta): d = 2 omega (y (log y - eta) - (y - mu)), which is
  2 omega mu at y = 0; chi = omega (y - mu)^2 / mu.
* logistic, y in [0, 1] (a grouped row is y = s / m with omega = m):
  d = 2 omega (y log y + (1 - y) log(1 - y) - (y eta - softplus(eta))) with
  0 log 0 = 0, which is -2 omega l for 0/1 data; with ea = exp(-|eta|),
  chi = omega (y (1 + ea) - [1 if eta >= 0 else ea])^2 / ea = omega (y - mu)^2 /
  (mu (1 - mu)), 1 - mu never formed.

tests/test_cpu_gof.py pins them: against scikit-learn's mean_poisson_deviance
and log_loss, the textbook Pearson form in long double, row replication,
grouped against expanded binomial rows, and a known dispersion.
"""

import numpy as np

import _glm_ref as G


def _xlogy(x, y):
    """x log y with 0 log 0 = 0 (NaN for negative y, as log gives it)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 0.0, x * np.log(y))


def row_terms(family, y, eta, w=None):
    """(d, chi): the rows' deviance and Pearson chi-square terms at eta."""
    y = np.asarray(y, dtype=np.float64)
    eta = np.asarray(eta, dtype=np.float64)
    om = G._omega(w, len(y))
    if family == "poisson":
        mu = np.exp(eta)
        with np.errstate(divide="ignore"):
            ly = np.where(y == 0.0, 0.0, np.log(y))
        r = y - mu
        return 2.0 * om * (y * (ly - eta) - r), om * (r * r / mu)
    ea = np.exp(-np.abs(eta))
    with np.errstate(divide="ignore", invalid="ignore"):
        sat = _xlogy(y, y) + np.where(y == 1.0, 0.0, (1.0 - y) * np.log1p(-y))
    t = y * (1.0 + ea) - np.where(eta >= 0, 1.0, ea)
    return 2.0 * om * (sat - (y * eta - G._softplus(eta))), om * (t * t / ea)


def gof(family, Z, y, theta, w=None, o=None):
    """(deviance, pearson, n_pos) of one partition at theta: the sums of the
    rows' terms and the rows with omega > 0."""
    eta = Z @ np.asarray(theta, np.float64) + (0.0 if o is None else o)
    d, c = row_terms(family, y, eta, w)
    return float(np.sum(d)), float(np.sum(c)), int(np.sum(G._omega(w, len(y)) > 0))


def gof_partitions(family, Z, y, offsets, betas=None, thetas=None, w=None, o=None):
    """deviance [K, B], pearson [K, B], n_pos [K]: ``betas`` [B, P] every
    partition at the same candidates, or ``thetas`` [K, P] partition k at its
    own row (B = 1)."""
    K = len(offsets) - 1
    B = 1 if thetas is not None else len(betas)
    dev, chi, npos = np.zeros((K, B)), np.zeros((K, B)), np.zeros(K, dtype=np.int64)
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        cands = [thetas[k]] if thetas is not None else betas
        for j, t in enumerate(cands):
            dev[k, j], chi[k, j], npos[k] = gof(
                family, Z[a:b], y[a:b], t, None if w is None else w[a:b],
                None if o is None else o[a:b])
    return dev, chi, npos


def dispersion(pearson_k, n_pos_k, P, ok=None):
    """phi = sum_k chi^2_k / (sum_k n+_k - K_ok P) over the partitions ``ok``
    (all by default), each evaluated at its own estimate."""
    ok = np.ones(len(n_pos_k), bool) if ok is None else np.asarray(ok, bool)
    return float(np.sum(np.asarray(pearson_k)[ok]) / (np.sum(np.asarray(n_pos_k)[ok]) - ok.sum() * P))
