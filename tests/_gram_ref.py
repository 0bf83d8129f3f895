"""The numpy yardstick of the score outer-product pass and the sandwich
covariance (not a test module), on tests/_glm_ref.py's design and (mu, omega
w):

* s = omega (y - mu), the rows' score residuals;
* M = Z^T diag(s^2) Z, the meat (``kind`` = "score");
* I = Z^T diag(omega w) Z, the information matrix ("information"), the very
  expression of ``_glm_ref.hessian``;
* g = Z^T s, the score vector.

tests/test_cpu_gram.py pins it: M against the sum of outer products of
single-row gradients, g against a finite difference of the log-likelihood, I
against ``_glm_ref.hessian`` bit for bit.
"""

import numpy as np

import _glm_ref as G


def gram(family, Z, y, theta, w=None, o=None, kind="score"):
    """(gram [P, P], score [P], max |Z|^T |s| -- the scale the score's error
    is measured against) of one partition at theta."""
    om = G._omega(w, len(y))
    mu, v = G._mu_w(family, Z, theta, om, o)
    s = om * (y - mu)
    d = s * s if kind == "score" else v
    return Z.T @ (Z * d[:, None]), Z.T @ s, float((np.abs(Z).T @ np.abs(s)).max(initial=0.0))


def gram_partitions(family, Z, y, offsets, thetas=None, beta=None, w=None, o=None, kind="score"):
    """Stacked over the partitions (an empty one: zeros): gram [K, P, P],
    score [K, P], the scores' scales [K].  ``thetas`` [K, P]: partition k at
    its own row; ``beta`` [P]: every partition at it."""
    K, P = len(offsets) - 1, Z.shape[1]
    Gm, sc, scale = np.zeros((K, P, P)), np.zeros((K, P)), np.zeros(K)
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        if b > a:
            th = np.asarray(beta if thetas is None else thetas[k], dtype=np.float64)
            Gm[k], sc[k], scale[k] = gram(family, Z[a:b], y[a:b], th,
                                          None if w is None else w[a:b],
                                          None if o is None else o[a:b], kind)
    return Gm, sc, scale


def sandwich(A, M):
    """(cov, info) = (A^-1 M A^-1, A M^-1 A) by explicit inverses: the
    textbook expressions ``distributed.sandwich_cov`` is checked against."""
    Ai = np.linalg.inv(A)
    return Ai @ M @ Ai, A @ np.linalg.inv(M) @ A


def negbin_job(seed, K=64, n_k=1500, p=4):
    """The over-dispersed set-up of the Monte-Carlo check: NB2 counts with
    Var y = mu + mu^2, K partitions of n_k rows, p columns of
    ``oracle.simulate_counter`` and an intercept, the coefficients of
    ``_glm_ref.simulate`` (intercept 1, 0.5 on the first max(1, floor(0.4 p))
    columns: mu around e, so Var y / mu = 1 + mu is 3 to 4).  Returns X, y,
    offsets."""
    import oracle as O

    n = K * n_k
    X, _ = O.simulate_counter(n, p, seed)
    X = np.ascontiguousarray(X)
    rng = np.random.default_rng(seed)
    theta = np.zeros(p + 1)
    theta[0] = 1.0
    theta[1:1 + max(1, int(0.4 * p))] = 0.5
    mu = np.exp(G.design(X, True) @ theta)
    y = rng.negative_binomial(1.0, 1.0 / (1.0 + mu)).astype(np.float64)
    return X, y, (np.arange(K + 1) * n_k).astype(np.int64)
