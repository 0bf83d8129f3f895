"""The torch fp64 yardstick of the tests whose data does not fit a host-side
numpy evaluation (not a test module): tests/_glm_ref.py's, _gram_ref.py's and
_gof_ref.py's formulas written out again in plain torch fp64 elementwise
operations and library GEMMs on the device that holds X -- no code of the
library under test.  Used by tests/test_gpu_long_chunks.py, whose partitions
cover more than 2^31 bytes of X.

* eta = Z theta (+ o), Z = [1, X] with an intercept; logistic mu = expit(eta),
  Poisson mu = exp(eta); prior weights omega (1 without);
* the score g = Z^T omega (y - mu), the information H = Z^T diag(omega w) Z
  (w = mu (1 - mu) or mu), the log-likelihood sum omega l_i (Poisson with the
  constant -lgamma(y + 1));
* the meat M = Z^T diag(s^2) Z, s = omega (y - mu);
* the deviance and Pearson terms of _gof_ref.row_terms.

Sums over rows are taken in slabs of 64 rows (a batched GEMM per 65536 rows
gives every slab's partial, the partials are then added): the partials of a
sum of n terms stay n / 64 times smaller than the total, which keeps the
yardstick's own summation error at a few eps of the total whatever the GEMM's
inner order.  tests/test_gpu_long_chunks.py measures it against numpy on a
1e5-row prefix.
"""

import torch

SLAB = 64
GROUP = 1024 * SLAB  # rows of one batched GEMM


def design(X, a, b, fi):
    """Rows [a, b) of the design, the ones column first."""
    Xk = X[a:b]
    if not fi:
        return Xk
    return torch.cat([torch.ones((b - a, 1), dtype=X.dtype, device=X.device), Xk], 1)


def _sl(v, a, b):
    return None if v is None else v[a:b]


def _eta(Z, theta, o):
    eta = Z @ theta
    return eta if o is None else eta + o


def _expit(t):
    e = torch.exp(-t.abs())
    return torch.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _softplus(t):
    return t.clamp_min(0.0) + torch.log1p(torch.exp(-t.abs()))


def mu_w(family, eta, om):
    """(mu, omega times the IRLS weight)."""
    if family == "logistic":
        mu = _expit(eta)
        return mu, om * mu * (1.0 - mu)
    mu = torch.exp(eta)
    return mu, om * mu


def loglik_terms(family, y, eta):
    if family == "logistic":
        return y * eta - _softplus(eta)
    return y * eta - torch.exp(eta) - torch.lgamma(y + 1.0)


def gof_terms(family, y, eta, om):
    """_gof_ref.row_terms: the rows' (deviance, Pearson) terms."""
    if family == "poisson":
        mu = torch.exp(eta)
        ly = torch.where(y == 0, torch.zeros_like(y), torch.log(y.clamp_min(1e-300)))
        r = y - mu
        return 2.0 * om * (y * (ly - eta) - r), om * (r * r / mu)
    ea = torch.exp(-eta.abs())
    xlogy = torch.where(y == 0, torch.zeros_like(y), y * torch.log(y.clamp_min(1e-300)))
    sat = xlogy + torch.where(y == 1, torch.zeros_like(y),
                              (1.0 - y) * torch.log1p(-y.clamp_max(1.0 - 1e-17)))
    t = y * (1.0 + ea) - torch.where(eta >= 0, torch.ones_like(ea), ea)
    return 2.0 * om * (sat - (y * eta - _softplus(eta))), om * (t * t / ea)


def _omega(w, n, like):
    return torch.ones(n, dtype=like.dtype, device=like.device) if w is None else w


def _slab_sum(v):
    """sum of a [m] or [m, c] tensor over rows: 64-row slab partials first."""
    m = v.shape[0]
    full = m // SLAB * SLAB
    head = v[:full].reshape(m // SLAB, SLAB, *v.shape[1:]).sum(1).sum(0)
    return head + v[full:].sum(0)


def _slab_gram(Z, d):
    """Z^T diag(d) Z of at most GROUP rows: one batched GEMM over the 64-row
    slabs, the slabs' partials added."""
    m, P = Z.shape
    full = m // SLAB * SLAB
    out = torch.zeros((P, P), dtype=Z.dtype, device=Z.device)
    if full:
        Zs = Z[:full].reshape(m // SLAB, SLAB, P)
        out += torch.bmm(Zs.transpose(1, 2), Zs * d[:full].reshape(-1, SLAB, 1)).sum(0)
    if full < m:
        out += Z[full:].T @ (Z[full:] * d[full:, None])
    return out


def fit_quantities(family, X, y, a, b, theta, fi, w=None, o=None):
    """(H, g, loglik) over rows [a, b) at theta, whole-partition GEMMs: what a
    converged fit's theta, sig_inv and loglik are checked against."""
    Z = design(X, a, b, fi)
    yk, om = y[a:b], _omega(_sl(w, a, b), b - a, X)
    eta = _eta(Z, theta, _sl(o, a, b))
    mu, v = mu_w(family, eta, om)
    g = Z.T @ (om * (yk - mu))
    H = Z.T @ (v[:, None] * Z)
    return H, g, float((om * loglik_terms(family, yk, eta)).sum())


def score_and_loglik(family, X, y, a, b, theta, fi):
    """(g, loglik) of the unweighted fits whose H is oracle.device_check's."""
    Z = design(X, a, b, fi)
    eta = Z @ theta
    if family == "ols":
        r = y[a:b] - eta
        return Z.T @ r, float((r * r).sum())
    mu, _ = mu_w(family, eta, 1.0)
    return Z.T @ (y[a:b] - mu), float(loglik_terms(family, y[a:b], eta).sum())


def gram(family, X, y, a, b, theta, fi, w=None, o=None, kind="score"):
    """_gram_ref.gram over rows [a, b) in 64-row slabs: (gram [P, P], score
    [P], max |Z|^T |s|)."""
    P = X.shape[1] + int(fi)
    Gm = torch.zeros((P, P), dtype=X.dtype, device=X.device)
    sc = torch.zeros(P, dtype=X.dtype, device=X.device)
    scale = torch.zeros(P, dtype=X.dtype, device=X.device)
    for r0 in range(a, b, GROUP):
        r1 = min(b, r0 + GROUP)
        Z = design(X, r0, r1, fi)
        om = _omega(_sl(w, r0, r1), r1 - r0, X)
        mu, v = mu_w(family, _eta(Z, theta, _sl(o, r0, r1)), om)
        s = om * (y[r0:r1] - mu)
        Gm += _slab_gram(Z, s * s if kind == "score" else v)
        sc += _slab_sum(Z * s[:, None])
        scale += _slab_sum(Z.abs() * s.abs()[:, None])
    return Gm, sc, float(scale.max())


def gof(family, X, y, a, b, theta, fi, w=None, o=None):
    """_gof_ref.gof over rows [a, b) in 64-row slabs: (deviance, pearson,
    n_pos)."""
    dev = chi = 0.0
    npos = 0
    for r0 in range(a, b, GROUP):
        r1 = min(b, r0 + GROUP)
        om = _omega(_sl(w, r0, r1), r1 - r0, X)
        d, c = gof_terms(family, y[r0:r1], _eta(design(X, r0, r1, fi), theta, _sl(o, r0, r1)), om)
        dev, chi = dev + _slab_sum(d), chi + _slab_sum(c)
        npos += int((om > 0).sum())
    return float(dev), float(chi), npos


def loglik(family, X, y, a, b, theta, fi, w=None, o=None):
    """_glm_ref.loglik over rows [a, b) in 64-row slabs."""
    ll = 0.0
    for r0 in range(a, b, GROUP):
        r1 = min(b, r0 + GROUP)
        om = _omega(_sl(w, r0, r1), r1 - r0, X)
        eta = _eta(design(X, r0, r1, fi), theta, _sl(o, r0, r1))
        ll = ll + _slab_sum(om * loglik_terms(family, y[r0:r1], eta))
    return float(ll)
