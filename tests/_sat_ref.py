"""The long-double yardstick of the GLM row terms at saturated linear
predictors (not a test module), and the bounds the saturation tests hold the
kernels to.

tests/_gof_ref.py and tests/_glm_ref.py state the row terms in fp64, in the
forms the kernels use; where such a form breaks (0 / 0 once exp(-|eta|) has
underflowed, y (1 + ea) - 1 cancelling from |eta| = 37 on, inf * inf / inf)
yardstick and kernel break together.  Here every term is formed in
``np.longdouble`` (x87 extended: 64-bit significand, exponents to 2^16384, so
exp(-800) and exp(800) are normal numbers) in a form that does not cancel, and
rounded once to fp64 -- overflow to +-inf, underflow to a subnormal or 0:

* logistic, ea = exp(-|eta|): mu and 1 - mu are 1 / (1 + ea) and ea / (1 + ea),
  whichever side eta is on; log mu and log(1 - mu) are -log1p(ea) minus |eta| on
  the far side, so l = y log mu + (1 - y) log(1 - mu) is a sum of terms of one
  sign; Pearson is (1 - mu) / mu = ea or 1 / ea at y = 1, mu / (1 - mu) at
  y = 0, and (y - mu)^2 (1 + ea)^2 / ea for a grouped y; w = ea / (1 + ea)^2;
* Poisson, mu = exp(eta): l = y eta - mu - lgamma(y + 1) with lgamma(y + 1) =
  sum log k (y an integer), d = 2 (y (log y - eta) - (y - mu)) and 2 mu at
  y = 0, Pearson (y - mu) ((y - mu) / mu) and mu at y = 0, w = mu;
* s = omega (y - mu), taken from 1 - mu at y = 1.

tests/test_cpu_saturated.py pins it against mpmath at 50 digits and ties it to
the fp64 yardsticks where those are sound (|eta| <= 20).
"""

import numpy as np

LD = np.longdouble
assert np.finfo(LD).maxexp >= 16384, "the yardstick needs x87 extended long double"

EPS = 2.0 ** -53          # fp64 unit roundoff
TINY = 2.0 ** -1022       # the smallest fp64 normal
HUGE = 2.0 ** 1022
DENORM = 4.94e-324        # the fp64 subnormal spacing (its absolute rounding is half of it)
REL = 1e-12
KEYS = ("loglik", "deviance", "pearson", "mu", "w", "s")


def to64(v):
    """One rounding to fp64: +-inf on overflow, a subnormal or 0 on underflow."""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(v, dtype=LD).astype(np.float64)


def _lgamma1p(y):
    """lgamma(y + 1) = sum_{k <= y} log k in long double, y integers >= 0."""
    yi = np.asarray(y).astype(np.int64)
    assert (yi == np.asarray(y)).all() and (yi >= 0).all(), "Poisson y must be integers >= 0"
    table = np.concatenate([[LD(0)], np.cumsum(np.log(np.arange(1, max(2, yi.max() + 1), dtype=LD)))])
    return table[yi]


def row_terms_ld(family, y, eta, w=None):
    """The rows' terms in long double (not yet rounded): a dict of KEYS, and
    "tiny", the exponential whose fp64 image goes subnormal and then 0
    (logistic exp(-|eta|), Poisson exp(eta)).  ``eta`` may be long double."""
    y = np.asarray(y, dtype=LD)
    eta = np.asarray(eta, dtype=LD)
    om = np.ones(len(y), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    one = LD(1)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        if family == "poisson":
            mu = np.exp(eta)
            lg = _lgamma1p(y)
            ly = np.where(y == 0, LD(0), np.log(np.where(y == 0, one, y)))
            r = y - mu
            return dict(loglik=om * (y * eta - mu - lg),
                        deviance=np.where(y == 0, 2 * om * mu, 2 * om * (y * (ly - eta) - r)),
                        pearson=om * np.where(y == 0, mu, r * (r / mu)),
                        mu=mu, w=om * mu, s=om * r, tiny=mu, lgamma=lg, sat=np.abs(y * ly) + y)
        pos = eta >= 0
        ae = np.abs(eta)
        ea = np.exp(-ae)
        big, small = one / (one + ea), ea / (one + ea)       # the mean's near and far side
        mu, omu = np.where(pos, big, small), np.where(pos, small, big)
        lp = np.log1p(ea)
        # l = y log mu + (1 - y) log(1 - mu): every term <= 0
        ll = -(lp + y * np.where(pos, LD(0), ae) + (one - y) * np.where(pos, ae, LD(0)))
        sat = np.where(y == 0, LD(0), y * np.log(np.where(y == 0, one, y))) + \
            np.where(y == 1, LD(0), (one - y) * np.log1p(-np.where(y == 1, LD(0), y)))
        odds_up, odds_dn = np.where(pos, one / ea, ea), np.where(pos, ea, one / ea)  # mu/(1-mu), inverse
        grouped = (y - mu) * (y - mu) * (one + ea) * (one + ea) / ea
        chi = np.where(y == 1, odds_dn, np.where(y == 0, odds_up, grouped))
        s = np.where(y == 1, omu, np.where(y == 0, -mu, y - mu))
        return dict(loglik=om * ll, deviance=2 * om * (sat - ll), pearson=om * chi, mu=mu,
                    w=om * ea / ((one + ea) * (one + ea)), s=om * s, tiny=ea,
                    lgamma=np.zeros(len(y), LD), sat=np.abs(sat))


def row_terms(family, y, eta, w=None):
    """The rows' terms rounded once to fp64: a dict of KEYS and "tiny"."""
    t = row_terms_ld(family, y, eta, w)
    return {k: to64(t[k]) for k in KEYS + ("tiny",)}


# ---- bounds: from the operation, not from the code under test ------------------------------------

def loglik_bound(family, y, eta, w=None):
    """|got - ref| of a row's log-likelihood term.  Logistic: y eta and max(eta,
    0) are each rounded at size |eta|, the remainder is at most log 2: 8 eps
    omega max(1, |eta|).  Poisson: 8 eps omega (|y eta| + mu + |lgamma(y + 1)|).
    Both plus 8 * 4.94e-324 max(1, omega): a term formed below 2^-1022 (a Poisson
    mu at eta < -708) is rounded at the subnormal spacing whatever its size, and
    then multiplied by omega."""
    y, eta = np.asarray(y, np.float64), np.asarray(eta, np.float64)
    om = np.ones(len(y)) if w is None else np.asarray(w, np.float64)
    floor = 8 * DENORM * np.maximum(1.0, om)
    with np.errstate(over="ignore"):
        if family == "poisson":
            t = row_terms_ld(family, y, eta)
            return 8 * EPS * om * to64(np.abs(y * eta) + t["mu"] + np.abs(t["lgamma"])) + floor
        return 8 * EPS * om * np.maximum(1.0, np.abs(eta)) + floor


def deviance_bound(family, y, eta, w=None):
    """Twice the log-likelihood's bound plus 8 eps omega |saturated term| (the
    logistic y log y + (1 - y) log(1 - y); the Poisson |y log y| + y)."""
    om = np.ones(len(y)) if w is None else np.asarray(w, np.float64)
    sat = to64(row_terms_ld(family, y, eta)["sat"])
    return 2 * loglik_bound(family, y, eta, w) + 8 * EPS * om * sat


def class_bound(ref, tiny, om):
    """The absolute bound of a term without a cancelling part (Pearson, the
    information's w) by the class of its reference value: relative 1e-12, plus
    4 * 4.94e-324 / tiny where ``tiny`` (the exponential it is a quotient by or
    a multiple of) is subnormal; a reference below 2^-1022 asks |got| <=
    2^-1000 omega; an infinite one, and a NaN, ask for exactly that (bound 0:
    see ``class_ratio``)."""
    ref, tiny = np.asarray(ref, np.float64), np.asarray(tiny, np.float64)
    sub = (tiny > 0) & (tiny < TINY)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rel = REL + np.where(sub, 4 * DENORM / np.where(sub, tiny, 1.0), 0.0)
        b = rel * np.abs(ref)
    b = np.where(np.abs(ref) < TINY, 2.0 ** -1000 * np.asarray(om, np.float64), b)
    return np.where(np.isfinite(ref), b, 0.0)


def class_ratio(got, ref, tiny, om):
    """The error of every entry over its ``class_bound`` (<= 1 passes): an
    infinite reference passes only by that infinity, one above 2^1022 also by
    +inf of its sign, and a NaN passes nowhere."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert not np.isnan(ref).any(), "the reference is undefined at a posed row"
    b = class_bound(ref, tiny, om)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        err = np.abs(got - ref)
        ratio = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1.0))
        ratio = np.where((b == 0) & (err != 0), np.inf, ratio)
    same_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
    ratio = np.where(np.isinf(ref), np.where(same_inf, 0.0, np.inf), ratio)
    ratio = np.where((np.abs(ref) > HUGE) & same_inf, 0.0, ratio)
    return np.where(np.isnan(got), np.inf, ratio)


def abs_ratio(got, ref, bound):
    """|got - ref| over an absolute ``bound``; equal infinities pass, a NaN or a
    wrong infinity does not."""
    got, ref, bound = (np.asarray(v, np.float64) for v in (got, ref, bound))
    assert not np.isnan(ref).any(), "the reference is undefined at a posed row"
    same = (got == ref)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ratio = np.abs(got - ref) / np.where(bound > 0, bound, 1.0)
        ratio = np.where((bound == 0) & ~same, np.inf, ratio)
    ratio = np.where(same, 0.0, ratio)
    return np.where(np.isnan(ratio), np.inf, ratio)


def score_delta(om):
    """d = 4 eps omega: the matched side rounds mu at eps by design."""
    return 4 * EPS * np.asarray(om, np.float64)


def score_bound(s_ref, om):
    """|s - s_ref| <= 4 eps omega + 1e-12 |s_ref|."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(s_ref), score_delta(om) + REL * np.abs(s_ref), 0.0)


def score_sq_bound(s_ref, om):
    """|s^2 - s_ref^2| <= 2 |s_ref| d + d^2 + 1e-12 s_ref^2."""
    d = score_delta(om)
    with np.errstate(invalid="ignore", over="ignore"):
        b = 2 * np.abs(s_ref) * d + d * d + REL * np.abs(s_ref) ** 2
    return np.where(np.isfinite(s_ref), b, 0.0)


# ---- the steep design ---------------------------------------------------------------------------

def steep_design(n, p, seed, wide=130.0, slope=6.0, intercept=0.3):
    """X [n, p], 0/1 y, theta* [p + 1]: half the rows have x0 ~ U(-1, 1), half
    x0 ~ U(-wide, wide) (interleaved by a fixed permutation), the other columns
    ~ U(-1, 1); theta* = (intercept, slope, U(-1, 1) 2 / sqrt(p) ...); y drawn
    from the logistic model.  The fit is well conditioned and converges in
    some 15 Newton steps, yet hundreds of fitted |eta| lie in (40, 700) and
    some past 745.13, where exp(-|eta|) is 0 in fp64."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (n, p))
    widen = rng.permutation(n) < n // 2
    X[widen, 0] = rng.uniform(-wide, wide, int(widen.sum()))
    theta = np.concatenate([[intercept, slope], rng.uniform(-1, 1, p - 1) * 2.0 / np.sqrt(p)])
    eta = X @ theta[1:] + theta[0]
    with np.errstate(over="ignore"):
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return np.ascontiguousarray(X), y, theta


def eta_ld(Z, theta, o=None):
    """Z theta (+ o) accumulated in long double."""
    e = np.asarray(Z, dtype=LD) @ np.asarray(theta, dtype=LD)
    return e if o is None else e + np.asarray(o, dtype=LD)


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------

GRID = (0.0, 1.0, 20.0, 36.0, 37.0, 40.0, 100.0, 500.0, 700.0, 708.0, 709.0, 710.0, 744.0, 745.0,
        745.5, 746.0, 800.0, 1e5)
POISSON_Y = (0.0, 1.0, 3.0, 351.0)


def grid_rows(family):
    """(y, eta, omega) of the posed rows.  Logistic: y in {0, 1} at both signs
    of every GRID value, and the grouped y = 0.25 with weight 4 at |eta| >= 20,
    where y - mu does not cancel.  Poisson: y in POISSON_Y at the signed GRID
    values in [-800, 709], then at the overflow rows eta = 710 and 800."""
    signed = np.array([s * e for e in GRID for s in (1.0, -1.0)])
    if family == "logistic":
        far = signed[np.abs(signed) >= 20.0]
        y = np.concatenate([np.zeros(len(signed)), np.ones(len(signed)), np.full(len(far), 0.25)])
        eta = np.concatenate([signed, signed, far])
        om = np.concatenate([np.ones(2 * len(signed)), np.full(len(far), 4.0)])
        return y, eta, om
    inside = np.concatenate([signed[(signed >= -800.0) & (signed <= 709.0)], [710.0, 800.0]])
    y = np.repeat(POISSON_Y, len(inside))
    return y, np.tile(inside, len(POISSON_Y)), np.ones(len(y))


STEEP = {  # name: (p, partition sizes, seed); P = p + 1
    "P4": (3, (2000, 600, 2000), 1),
    "P100": (99, (3001, 3001), 2),
    "P132": (131, (6001,), 3),
}


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
