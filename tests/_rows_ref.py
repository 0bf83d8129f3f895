"""The numpy yardstick of the row diagnostics pass (not a test module), on
tests/_glm_ref.py's design: per row of one partition at theta

* eta = Z theta (+ o) and mu;
* dev and chi, the row's deviance and Pearson terms by tests/_gof_ref.py's
  row expressions (the logistic t = y (1 + ea) - [1 | ea] taken as a + b ea,
  (a, b) = (y - 1, y) at eta >= 0 and (y, y - 1) below: the same expression
  without the cancellation of (1 + ea) - 1, which costs 2e-11 at |eta| = 12);
* the signed residuals sign(y - mu) sqrt(dev), sign(y - mu) sqrt(chi), the
  sign taken from r = y - mu (Poisson) or t (logistic);
* q = |R z|^2 from a GIVEN factor R (R^T R = S^-1) and h = omega w q, the
  logistic w = ea / (1 + ea)^2 (mu (1 - mu) loses 1 - mu);
* the HC3 meat sum_i (s_i / (1 - h_i))^2 z_i z_i^T,

each with its per-row error bound, from the operation and not from the code
under test (eps = 2^-53):

* eta: (P + 4) eps (sum_f |z_f theta_f| + |o|) -- a P-term fma chain, the
  8-lane tree, the offset's add;
* mu: mu (that eta bound + 8 eps) -- d mu / d eta <= mu for both families,
  plus exp and the division;
* dev, chi (against dev_res^2, pearson_res^2): tests/_sat_ref.py's per-row
  ``deviance_bound`` and ``class_bound`` at the yardstick's eta, plus what
  the mu bound moves them by -- with d mu = mu delta, delta = the eta bound +
  8 eps, |d dev| = 2 omega |y - mu| delta and |d chi| <= (2 omega |y - mu| +
  chi) delta (y - mu cancels where the fit is good: the rounding of mu is
  then the whole error of chi, which a relative bound alone cannot hold),
  each doubled for the second order -- plus 4 eps of the value for the square
  root squared again;
* h: 4 (P + 24) eps omega w | |R| |z| |^2 -- P from the fma chain of a z
  component, the factor 3 from the squaring and the sum, the rest from the
  standardisation, w and the product.

tests/test_cpu_rows.py pins it: h against the hat matrix's diagonal, sum h =
P, the residuals' squares against ``_gof_ref``'s sums, fp64 against a long
double evaluation, and how few rows fall under the sign check's bound.
"""

import functools

import numpy as np

import _glm_ref as G
import _gof_ref as GOF
import _gram_ref as GR
import _sat_ref as SAT

EPS = SAT.EPS
STREAMS = ("eta", "mu", "dev_res", "pearson_res", "leverage")

# the shapes of tests/test_gpu_gram.py, and p = 128 (p = 0 mod 32)
SIZES = (3001, 1500, 0, 4096, 1, 2003)
EMPTY, SINGLE = 2, 4
SMALL = [(1, False), (1, True), (15, True), (16, True), (33, False)]
LARGE = [(100, True), (127, True), (128, False), (129, False), (191, True), (192, False)]
FAMILY_MASKS = [("logistic", "none"), ("logistic", "wgt"), ("poisson", "none"),
                ("poisson", "ofs"), ("poisson", "wgt"), ("poisson", "both")]
CASES = [(p, fi, f, m) for p, fi in SMALL for f, m in FAMILY_MASKS] + \
        [(p, fi, f, m) for p, fi in LARGE for f, m in (("logistic", "wgt"), ("poisson", "both"))]
CASE_IDS = [f"p{p}-ic{int(fi)}-{f}-{m}" for p, fi, f, m in CASES]


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def dense(p, fi, sizes=SIZES):
    """tests/test_gpu_gram.py's data recipe: X, the two families' y, offset,
    weights, offsets, per-partition thetas (the shared beta is row 1) with
    |eta| <= 12, center / scale; once per process, read-only."""
    import oracle as O

    off = offsets_of(sizes)
    n, K, P = int(off[-1]), len(sizes), p + fi
    X, _ = O.simulate_counter(n, p, seed=60 + p)
    X = np.ascontiguousarray(X)
    rng = np.random.default_rng(p)
    o = rng.uniform(np.log(0.2), np.log(5.0), n)
    star = np.concatenate([[0.5] * fi, rng.uniform(-1, 1, p) * 1.5 / np.sqrt(p)])
    Z = G.design(X, fi)
    ypois = rng.poisson(np.exp(Z @ star + o)).astype(np.float64)
    ylog = (rng.uniform(size=n) < G._expit(Z @ star)).astype(np.float64)
    thetas = star + rng.standard_normal((K, P)) * 0.5 / np.sqrt(P)
    c, s = X.mean(0), X.std(0, ddof=1) * 0.5 + 0.1
    Zs = G.design(X, fi, c, s)
    for z, scale in ((Z, 1.0), (Zs, 0.4)):
        assert np.abs(z @ (thetas * scale).T).max() + np.abs(o).max() <= 12.0
    w = G.weights(n, "real")
    for a in (X, ylog, ypois, o, w, thetas, Z, Zs):
        a.setflags(write=False)
    return dict(X=X, logistic=ylog, poisson=ypois, o=o, w=w, off=off, thetas=thetas, Z=Z, Zs=Zs,
                center=c, scale=s)


def extras(d, mask):
    return (d["o"] if mask in ("ofs", "both") else None,
            d["w"] if mask in ("wgt", "both") else None)


def information(family, Z, theta, w=None, o=None):
    """Z^T diag(omega w) Z with the w of ``rows`` (the logistic one without
    1 - mu)."""
    v = _w(family, Z @ np.asarray(theta, np.float64) + (0.0 if o is None else o),
           G._omega(w, Z.shape[0]))
    return Z.T @ (Z * v[:, None])


def factor(S):
    """R = L^-1 of S = L L^T by numpy (NaN where S is not positive definite)."""
    S = np.asarray(S, np.float64)
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return np.full_like(S, np.nan)
    return np.tril(np.linalg.solve(L, np.eye(S.shape[0])))


def _w(family, eta, om):
    if family == "poisson":
        return om * np.exp(eta)
    ea = np.exp(-np.abs(eta))
    return om * (ea / ((1.0 + ea) * (1.0 + ea)))


def _sign_of(family, y, eta):
    """What carries the sign of y - mu: r = y - mu (Poisson), t = a + b ea."""
    if family == "poisson":
        return y - np.exp(eta)
    ea = np.exp(-np.abs(eta))
    pos = eta >= 0
    return np.where(pos, y - 1.0, y) + np.where(pos, y, y - 1.0) * ea


def rows(family, Z, y, theta, R=None, w=None, o=None):
    """The rows' values of one partition at theta: a dict of eta, mu, dev, chi,
    sign, dev_res, pearson_res, d = omega w, and with R also q, qabs =
    | |R| |z| |^2 and leverage."""
    y = np.asarray(y, np.float64)
    theta = np.asarray(theta, np.float64)
    om = G._omega(w, len(y))
    eta = Z @ theta + (0.0 if o is None else o)
    mu = np.exp(eta) if family == "poisson" else G._expit(eta)
    sg = _sign_of(family, y, eta)
    dev, chi = GOF.row_terms(family, y, eta, w)
    if family == "logistic":
        chi = om * (sg * (sg / np.exp(-np.abs(eta))))
    out = dict(eta=eta, mu=mu, dev=dev, chi=chi, sign=sg, d=_w(family, eta, om),
               dev_res=np.copysign(np.sqrt(np.maximum(dev, 0.0)), sg),
               pearson_res=np.copysign(np.sqrt(chi), sg),
               eta_scale=np.abs(Z) @ np.abs(theta) + (0.0 if o is None else np.abs(o)))
    if R is not None:
        zr = Z @ R.T
        out["q"] = (zr * zr).sum(1)
        za = np.abs(Z) @ np.abs(R).T
        out["qabs"] = (za * za).sum(1)
        out["leverage"] = out["d"] * out["q"]
    return out


def bounds(family, Z, y, theta, w=None, o=None, ref=None, R=None):
    """The per-row bounds of the module docstring for ``ref`` = rows(...): a
    dict of eta, mu, dev, chi and with R leverage."""
    ref = rows(family, Z, y, theta, R, w, o) if ref is None else ref
    om = G._omega(w, len(y))
    P = Z.shape[1]
    be = (P + 4) * EPS * ref["eta_scale"]
    r = np.abs(np.asarray(y, np.float64) - ref["mu"])
    tiny = ref["mu"] if family == "poisson" else np.exp(-np.abs(ref["eta"]))
    out = dict(
        eta=be, mu=ref["mu"] * (be + 8 * EPS),
        dev=SAT.deviance_bound(family, y, ref["eta"], w) + 2 * (2 * om * r) * (be + 8 * EPS)
        + 4 * EPS * np.abs(ref["dev"]),
        chi=SAT.class_bound(ref["chi"], tiny, om)
        + 2 * (2 * om * r + ref["chi"]) * (be + 8 * EPS) + 4 * EPS * ref["chi"])
    if "qabs" in ref:
        out["leverage"] = 4 * (P + 24) * EPS * ref["d"] * ref["qabs"]
    return out


def ratio(err, bound):
    """err over its bound, entry by entry (<= 1 passes): 0 where the error is
    0 (a row of weight 0 has the bound 0), inf where it is not but the bound
    is, and where the error is NaN."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
    r = np.where((err != 0) & ~(bound > 0), np.inf, r)
    return np.where(np.isnan(err), np.inf, r)


def rows_ld(family, Z, y, theta, R=None, w=None, o=None):
    """``rows`` in long double (tests/_sat_ref.py's non-cancelling forms), not
    rounded: eta, mu, dev, chi, d, and with R q and leverage."""
    LD = SAT.LD
    eta = SAT.eta_ld(Z, theta, o)
    t = SAT.row_terms_ld(family, y, eta, w)
    out = dict(eta=eta, mu=t["mu"], dev=t["deviance"], chi=t["pearson"], d=t["w"])
    if R is not None:
        zr = np.asarray(Z, LD) @ np.asarray(R, LD).T
        out["q"] = (zr * zr).sum(1)
        out["leverage"] = out["d"] * out["q"]
    return out


def partitions(family, Z, y, offsets, thetas=None, beta=None, R=None, w=None, o=None):
    """``rows`` and ``bounds`` over the partitions, concatenated to [n] arrays:
    (ref, bnd).  ``thetas`` [K, P] or ``beta`` [P]; ``R`` [K, P, P], [P, P] or
    None."""
    refs, bnds = [], []
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        if b == a:
            continue
        th = np.asarray(beta if thetas is None else thetas[k], np.float64)
        Rk = None if R is None else (R if R.ndim == 2 else R[k])
        args = (family, Z[a:b], y[a:b], th)
        kw = dict(w=None if w is None else w[a:b], o=None if o is None else o[a:b])
        with np.errstate(invalid="ignore"):
            ref = rows(*args, R=Rk, **kw)
            refs.append(ref)
            bnds.append(bounds(*args, ref=ref, **kw))
    cat = lambda ds: {k: np.concatenate([d[k] for d in ds]) for k in ds[0]}
    return cat(refs), cat(bnds)


def own_factors(family, Z, offsets, thetas, w=None, o=None):
    """[K, P, P]: the information of every partition at its own theta."""
    K, P = len(offsets) - 1, Z.shape[1]
    S = np.zeros((K, P, P))
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        S[k] = information(family, Z[a:b], thetas[k], None if w is None else w[a:b],
                           None if o is None else o[a:b])
    return S


def hc3_meat(family, Z, y, theta, h, w=None, o=None):
    """sum_i (s_i / (1 - h_i))^2 z_i z_i^T: the score pass's meat with the
    weight omega / (1 - h)."""
    om = G._omega(w, len(y))
    return GR.gram(family, Z, y, theta, om / (1.0 - h), o)[0]
