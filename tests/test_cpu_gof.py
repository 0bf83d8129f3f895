"""CPU: the pins of the goodness-of-fit yardstick (tests/_gof_ref.py) and the
host side of the feature -- no GPU.

statsmodels is not a dependency of the project, so the independent references
are scikit-learn's ``mean_poisson_deviance`` and ``log_loss``, the textbook
Pearson form in long double, row replication, the expanded rows of a grouped
binomial and simulated negative-binomial data of known dispersion.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _glm_ref as G
import _gof_ref as R

HEADER = Path(__file__).resolve().parents[1] / "include" / "dlsa_hip.h"
REL = 1e-12  # two fp64 statements of the same sum of a few thousand terms


def _rel(a, b):
    return abs(a - b) / abs(b)


def _poisson_case(n=3000, p=4, seed=5):
    X, y, o = G.simulate_offset(n, p, True, seed)
    Z = G.design(X, True)
    theta = np.concatenate([[0.9], 0.45 * np.ones(p)])
    theta[3:] = 0.0
    return Z, y, o, theta


@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_poisson_deviance_is_sklearns(with_offset, weighted):
    from sklearn.metrics import mean_poisson_deviance

    Z, y, o, theta = _poisson_case()
    o = o if with_offset else None
    w = G.weights(len(y), "real") if weighted else None
    mu = np.exp(Z @ theta + (0.0 if o is None else o))
    dev, _, npos = R.gof("poisson", Z, y, theta, w, o)
    n_eff = len(y) if w is None else w.sum()
    want = n_eff * mean_poisson_deviance(y, mu, sample_weight=w)
    assert (y == 0).any() and _rel(dev, want) < REL
    assert npos == (len(y) if w is None else int((w > 0).sum()))


@pytest.mark.parametrize("weighted", [False, True])
def test_logistic_deviance_of_01_data_is_twice_sklearns_log_loss(weighted):
    from sklearn.metrics import log_loss

    import oracle as O

    X, y = O.simulate_counter(3000, 5, seed=3)
    Z = G.design(X, True)
    theta = np.array([-0.2, 0.8, -0.5, 0.3, 0.0, 0.1])
    w = G.weights(len(y), "real") if weighted else None
    dev, _, _ = R.gof("logistic", Z, y, theta, w)
    want = 2.0 * log_loss(y, G._expit(Z @ theta), normalize=False, sample_weight=w)
    assert _rel(dev, want) < REL
    assert _rel(dev, -2.0 * G.loglik("logistic", Z, y, theta, w)) < REL


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_pearson_forms_equal_the_textbook_form_in_long_double(family):
    """Row by row at |eta| <= 20.  The textbook form loses digits itself where
    the logistic mu nears 0 or 1: 1 - mu, formed in long double, carries a
    relative error eps_ld exp(|eta|), and it enters (y - mu)^2 twice and V(mu)
    once.  The bound is that, 8 eps_ld exp(|eta|), plus 32 eps of fp64 for the
    yardstick's own handful of operations, plus the conditioning of y - mu
    where a fractional y comes close to mu."""
    ld = np.longdouble
    rng = np.random.default_rng(12)
    n = 4000
    eta = np.concatenate([rng.uniform(-20, 20, n - 4), [-20.0, 20.0, 0.0, 1e-9]])
    w = rng.uniform(0.2, 5.0, n)
    if family == "logistic":
        y = np.where(rng.random(n) < 0.5, np.round(rng.random(n)), rng.random(n))
        mu = 1 / (1 + np.exp(-eta.astype(ld)))
        want = w.astype(ld) * (y.astype(ld) - mu) ** 2 / (mu * (1 - mu))
        slack = 8 * np.finfo(ld).eps * np.exp(np.abs(eta))
    else:
        eta = eta / 4.0  # mu up to e^5
        y = rng.poisson(np.exp(eta)).astype(np.float64)
        mu = np.exp(eta.astype(ld))
        want = w.astype(ld) * (y.astype(ld) - mu) ** 2 / mu
        slack = 0.0
    _, chi = R.row_terms(family, y, eta, w)
    err = np.abs(chi.astype(ld) - want)
    # y - mu itself, a difference of fp64 numbers, is conditioned like (y + mu) /
    # |y - mu| in any fp64 form, and it is squared
    eps = np.finfo(np.float64).eps
    cond = 8 * eps * (y + mu) / np.maximum(np.abs(y - mu), np.finfo(ld).tiny)
    assert (err <= (slack + 32 * eps + cond) * np.abs(want) + 1e-300).all()


@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_integer_weights_reproduce_row_replication(family):
    Z, y, o, theta = _poisson_case(n=1500)
    if family == "logistic":
        y, o = (y > 2).astype(np.float64), None
        theta = theta * 0.3
    w = G.weights(len(y), "int")
    got = R.gof(family, Z, y, theta, w, o)
    Zr, yr, orr = G.replicate(w, Z, y, np.zeros(len(y)) if o is None else o)
    want = R.gof(family, Zr, yr, theta, None, orr)
    assert _rel(got[0], want[0]) < REL and _rel(got[1], want[1]) < REL
    assert got[2] == int((w > 0).sum()) and want[2] == int(w.sum())


def test_grouped_binomial_against_its_expanded_rows():
    """y = s / m with omega = m.  At m = 1 the rows are the 0/1 rows.  At m > 1
    the expanded rows' saturated log-likelihood is 0 and the grouped rows' is
    sum s log(s/m) + (m - s) log(1 - s/m), so the grouped deviance is the
    expanded one minus -2 times that sum."""
    rng = np.random.default_rng(4)
    n, p = 800, 3
    X = rng.standard_normal((n, p))
    theta = np.array([0.4, -0.7, 0.2])
    for m in (np.ones(n, np.int64), rng.integers(1, 9, n)):
        s = rng.binomial(m, G._expit(X @ theta))
        assert (s == 0).any() and (s == m).any()
        Xe, ye, _ = G.expand_binomial(X, s, m, [0, n])
        dev_g, chi_g, _ = R.gof("logistic", X, s / m, theta, m.astype(np.float64))
        dev_e, chi_e, _ = R.gof("logistic", Xe, ye, theta)
        sat = -2.0 * float(np.sum(R._xlogy(s, s / m) + R._xlogy(m - s, 1.0 - s / m)))
        assert abs(dev_g - (dev_e - sat)) < REL * dev_e
        if (m == 1).all():
            assert sat == 0.0 and _rel(chi_g, chi_e) < REL


def test_dispersion_of_negative_binomial_data_is_recovered():
    """y ~ NB(mean mu, size r): Var y = phi mu with phi = 1 + mu / r.  At the
    Poisson MLE phi_hat = chi^2 / (n - P) estimates the row average of phi.
    With q = mu / r the NB cumulants are k2 = mu (1 + q) and k4 = k2 (1 + 6 q +
    6 q^2), so Var[(y - mu)^2 / mu] = (k4 + 2 k2^2) / mu^2; the bound is five
    standard deviations of the mean of n such terms (n = 20000: about 4% of
    phi) plus P / n for the fitted parameters."""
    n, p, r = 20000, 3, 2.0
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, p)) * 0.4
    theta = np.array([1.0, 0.5, -0.3, 0.0])
    Z = G.design(X, True)
    mu = np.exp(Z @ theta)
    y = rng.negative_binomial(r, r / (r + mu)).astype(np.float64)
    fit = G.fit("poisson", X, y, fit_intercept=True)
    _, chi, npos = R.gof("poisson", Z, y, fit["theta"])
    phi_hat = R.dispersion([chi], [npos], p + 1)
    q = mu / r
    k2 = mu * (1 + q)
    k4 = k2 * (1 + 6 * q + 6 * q * q)
    phi = float(np.mean(1 + q))
    sd = float(np.sqrt(np.sum((k4 + 2 * k2 * k2) / mu ** 2))) / n
    print(f"phi_hat {phi_hat:.4f} row-average phi {phi:.4f} sd {sd:.4f}")
    assert phi > 2.0 and abs(phi_hat - phi) <= 5 * sd + phi * (p + 1) / n


def test_finish_on_the_scaled_sums():
    """The host side of dispersion="pearson": finish(S / phi, v / phi, ..).
    With phi a power of two the scaling is exact and the WLSE keeps its bits;
    with phi = 7 it agrees to rounding and the DBIC drops the coefficient whose
    chi-square theta_j^2 S_jj = 14.4 > log N = 6.9 falls to 2.06."""
    from dlsa_amd.distributed import finish

    N, K = 1000, 4
    theta = np.array([1.0, 0.5, 0.12, 0.0])
    rng = np.random.default_rng(0)
    A = rng.standard_normal((4, 4)) * 1e-3
    S = N * (np.eye(4) + A + A.T)
    v = S @ theta
    base = finish(S, v, K * theta, K, N)
    assert base["dbic_support"].tolist() == [0, 1, 2]
    exact = finish(S / 4.0, v / 4.0, K * theta, K, N)
    assert exact["wlse"].tobytes() == base["wlse"].tobytes()
    scaled = finish(S / 7.0, v / 7.0, K * theta, K, N)
    assert np.abs(scaled["wlse"] - base["wlse"]).max() < 1e-13
    assert scaled["dbic_support"].tolist() == [0, 1]


def test_argument_validation_needs_no_gpu():
    from dlsa_amd import models as M

    X, y, off = np.zeros((6, 2)), np.zeros(6), [0, 6]
    b = np.zeros((1, 2))
    for fn, lead in ((M.glm_gof_batched, (X, y, off)),
                     (M.glm_gof_batched_categorical, (X, np.zeros((6, 1), np.uint8), y, off, [2]))):
        with pytest.raises(ValueError, match="exactly one"):
            fn("poisson", *lead)
        with pytest.raises(ValueError, match="exactly one"):
            fn("poisson", *lead, betas=b, thetas=b)
        with pytest.raises(ValueError, match="family='poisson'"):
            fn("logistic", *lead, betas=b, eta_offset=np.zeros(6))
        with pytest.raises(ValueError, match="n entries"):
            fn("poisson", *lead, betas=b, sample_weight=np.ones(5))
        with pytest.raises(ValueError, match="n entries"):
            fn("poisson", *lead, betas=b, exposure=np.ones(7))
        with pytest.raises(ValueError, match="family must be"):
            fn("gaussian", *lead, betas=b)
    from dlsa_amd.distributed import dlsa_fit_sharded
    with pytest.raises(ValueError, match="dispersion"):
        dlsa_fit_sharded(X, y, off, dispersion="deviance")


def test_abi_declares_and_binds_the_two_entries():
    from dlsa_amd import _hip

    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name in ("dlsa_glm_gof_batched", "dlsa_glm_gof_categorical"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/dlsa_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        assert _hip.SIGNATURES[name] == (ctypes.c_int, want)
        assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name)
    defs = dict(re.findall(r"#define\s+(DLSA_\w+)\s+(\d+)", txt))
    assert (int(defs["DLSA_FAMILY_LOGISTIC"]), int(defs["DLSA_FAMILY_POISSON"])) == \
        (_hip.FAMILY_LOGISTIC, _hip.FAMILY_POISSON) == (0, 2)
    assert 1 <= int(defs["DLSA_MAX_GOF_CANDIDATES"]) == _hip.MAX_GOF_CANDIDATES <= 16
