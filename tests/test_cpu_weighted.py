"""Per-row prior weights without a GPU: the numpy yardstick of
tests/_glm_ref.py with weights pinned against itself without them and against
row replication, and the C-ABI / Python surface of the weighted entries.

Both sides of every comparison are the same fp64 Newton run to convergence
(max|step| <= 1e-12), so they agree to 1e-12 relative to the largest entry in
theta, Sig_inv and the log-likelihood.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _glm_ref as G
import oracle as O

TOL = 1e-12
SIZES = (700, 0, 513)
HEADER = Path(__file__).resolve().parents[1] / "include" / "dlsa_hip.h"
NEW_ENTRIES = ("dlsa_logistic_fit_batched_weighted", "dlsa_poisson_fit_batched_weighted",
               "dlsa_logistic_loglik_batched_sum_weighted",
               "dlsa_poisson_loglik_batched_sum_weighted")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _same(got, want, parts, tag):
    for k in parts:
        e = [_rel(got[f][k], want[f][k]) for f in ("theta", "sig_inv", "loglik")]
        print(f"{tag} k={k} theta {e[0]:.2e} sig_inv {e[1]:.2e} loglik {e[2]:.2e}")
        assert max(e) < TOL, (tag, k, e)


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _logistic_data(p, sizes, seed=3):
    off = _offsets(sizes)
    X, y = O.simulate_counter(int(off[-1]), p, seed=seed)
    return np.ascontiguousarray(X), y, off


NONEMPTY = [k for k, s in enumerate(SIZES) if s > 0]


# ---- omega = 1 is the unweighted reference ------------------------------------

@pytest.mark.parametrize("fi", [False, True])
def test_unit_weights_logistic_is_the_oracle(fi):
    X, y, off = _logistic_data(6, SIZES)
    got = G.fit_partitions("logistic", X, y, off, w=np.ones(len(y)), fit_intercept=fi)
    for k in NONEMPTY:
        o = O.logistic_fit(X[off[k]:off[k + 1]], y[off[k]:off[k + 1]], fit_intercept=fi,
                           tol=1e-12)
        want = {"theta": {k: o["coef"]}, "sig_inv": {k: o["Sig_inv"]}, "loglik": {k: o["loglik"]}}
        _same(got, want, [k], f"logistic unit fi={fi}")


@pytest.mark.parametrize("fi,with_offset", [(False, False), (True, False), (True, True)])
def test_unit_weights_poisson_is_the_offset_reference(fi, with_offset):
    X, y, o = G.simulate_offset(int(sum(SIZES)), 5, fit_intercept=fi)
    off = _offsets(SIZES)
    if not with_offset:
        o0 = np.zeros_like(o)
        y = np.random.default_rng(5).poisson(np.exp(X[:, :2].sum(1) * 0.5 + fi)).astype(float)
    else:
        o0 = o
    got = G.fit_partitions("poisson", X, y, off, w=np.ones(len(y)),
                           o=o0 if with_offset else None, fit_intercept=fi)
    want = {f: {} for f in ("theta", "sig_inv", "loglik")}
    for k in NONEMPTY:
        a, b = off[k], off[k + 1]
        r = G.fit("poisson", X[a:b], y[a:b], o=o0[a:b], fit_intercept=fi)
        for f in want:
            want[f][k] = r[f]
    _same(got, want, NONEMPTY, f"poisson unit fi={fi} ofs={with_offset}")


# ---- integer omega is row replication -----------------------------------------

@pytest.mark.parametrize("family", ["logistic", "poisson", "poisson_offset"])
def test_integer_weights_are_replication(family):
    fi = True
    off = _offsets(SIZES)
    n = int(off[-1])
    w = G.weights(n, "int")
    if family == "logistic":
        X, y, _ = _logistic_data(6, SIZES)
        o = None
    else:
        X, y, o = G.simulate_offset(n, 5, fit_intercept=fi)
        if family == "poisson":
            o = None
            y = np.random.default_rng(5).poisson(np.exp(X[:, :2].sum(1) * 0.5 + 1.0)).astype(float)
    fam = "logistic" if family == "logistic" else "poisson"
    got = G.fit_partitions(fam, X, y, off, w=w, o=o, fit_intercept=fi)
    arrays = (X, y) if o is None else (X, y, o)
    rep = G.replicate(w, *arrays)
    roff = G.replicate_offsets(w, off)
    want = G.fit_partitions(fam, rep[0], rep[1], roff, w=np.ones(len(rep[1])),
                            o=None if o is None else rep[2], fit_intercept=fi)
    _same(got, want, NONEMPTY, f"{family} replication")
    # and the replicated side is the unweighted reference itself
    k = NONEMPTY[0]
    a, b = roff[k], roff[k + 1]
    if family == "logistic":
        r = O.logistic_fit(rep[0][a:b], rep[1][a:b], fit_intercept=fi, tol=1e-12)
        assert _rel(want["theta"][k], r["coef"]) < TOL
    else:
        oo = np.zeros(b - a) if o is None else rep[2][a:b]
        r = G.fit("poisson", rep[0][a:b], rep[1][a:b], o=oo, fit_intercept=fi)
        assert _rel(want["theta"][k], r["theta"]) < TOL


def test_grouped_binomial_is_the_expanded_fit():
    """y = s / m with omega = m against the 0/1 rows: the same theta and
    Sig_inv; the log-likelihoods agree because the binomial-coefficient
    constant is in neither."""
    fi = True
    X, _, off = _logistic_data(4, SIZES, seed=9)
    n = int(off[-1])
    rng = np.random.default_rng(2)
    m = rng.integers(1, 6, n)
    prob = 1.0 / (1.0 + np.exp(-(0.3 + X[:, 0] - 0.5 * X[:, 1])))
    s = rng.binomial(m, prob)
    got = G.fit_partitions("logistic", X, s / m, off, w=m.astype(float), fit_intercept=fi)
    Xe, ye, offe = G.expand_binomial(X, s, m, off)
    want = G.fit_partitions("logistic", Xe, ye, offe, w=np.ones(len(ye)), fit_intercept=fi)
    _same(got, want, NONEMPTY, "grouped binomial")
    k = NONEMPTY[0]
    r = O.logistic_fit(Xe[offe[k]:offe[k + 1]], ye[offe[k]:offe[k + 1]], fit_intercept=fi,
                       tol=1e-12)
    assert _rel(want["theta"][k], r["coef"]) < TOL
    assert _rel(want["loglik"][k], r["loglik"]) < TOL


# ---- the C-ABI and the Python surface (fails without the feature) ---------------

_CTYPES = {"const double*": ctypes.c_void_p, "double*": ctypes.c_void_p,
           "const int64_t*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p,
           "void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "double": ctypes.c_double}


def _header_prototype(name):
    """[(C type, argument name)] of `int name(...)` in include/dlsa_hip.h."""
    text = HEADER.read_text()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/dlsa_hip.h"
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        t, nm = a.rsplit(" ", 1)
        args.append((t.replace(" *", "*"), nm))
    return args


@pytest.mark.parametrize("name", NEW_ENTRIES)
def test_weighted_entries_exported_and_bound(name):
    from dlsa_amd import _hip

    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, name), f"libdlsa_hip.so does not export {name}"
    assert name in _hip.SIGNATURES, f"_hip.py does not bind {name}"
    proto = _header_prototype(name)
    res, argtypes = _hip.SIGNATURES[name]
    assert res is ctypes.c_int
    want = []
    for t, nm in proto:
        if t == "const dlsa_fit_options*":
            want.append(ctypes.POINTER(_hip.FitOptions))
        else:
            want.append(_CTYPES[t])
    assert argtypes == want, (name, [n for _, n in proto])
    # row_weight sits after y, in the Poisson entries after eta_offset
    names = [n for _, n in proto]
    i = names.index("row_weight")
    assert names[:2] == ["X", "y"]
    if "poisson" in name:
        assert names[2] == "eta_offset" and i == 3
    else:
        assert i == 2
    assert names[i + 1] == "offsets"


def test_existing_prototypes_unchanged():
    """The entries the weighted ones extend keep their argument lists: each
    weighted prototype is the unweighted one plus row_weight."""
    pairs = [("dlsa_logistic_fit_batched_weighted", "dlsa_logistic_fit_batched_ex"),
             ("dlsa_poisson_fit_batched_weighted", "dlsa_poisson_fit_batched_offset"),
             ("dlsa_logistic_loglik_batched_sum_weighted", "dlsa_logistic_loglik_batched_sum"),
             ("dlsa_poisson_loglik_batched_sum_weighted", "dlsa_poisson_loglik_batched_sum_offset")]
    for new, old in pairs:
        a = [x for x in _header_prototype(new) if x[1] != "row_weight"]
        assert a == _header_prototype(old), (new, old)


def test_python_surface():
    """The entries whose parameter lists earlier tests pin (the fits, the
    Poisson evaluations) keep them and gain ``*_weighted`` siblings that take
    ``sample_weight`` after the data; the others take it as a trailing keyword.
    It defaults to None everywhere."""
    import inspect

    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def names(fn):
        return [p.name for p in inspect.signature(fn).parameters.values()
                if p.kind is not inspect.Parameter.VAR_KEYWORD]

    for fn in (M.logistic_loglik_batched, D.dlsa_fit_sharded, D.loglik_sharded):
        assert names(fn)[-1] == "sample_weight", fn.__name__
    old = names(M.logistic_model_batched)
    assert "sample_weight" not in old
    new = names(M.logistic_model_batched_weighted)
    assert new[:4] == old[:3] + ["sample_weight"]
    assert set(new[4:]) == set(old[3:]) - {"exact", "oz_max_bytes"}  # no int8 pass to choose
    old = names(M.poisson_model_batched_offset)
    assert names(M.poisson_model_batched_weighted) == old[:3] + ["sample_weight"] + old[3:]
    old = names(M.poisson_loglik_batched_offset)
    assert names(M.poisson_loglik_batched_weighted) == old[:4] + ["sample_weight"] + old[4:]
    for fn in (M.logistic_loglik_batched, D.dlsa_fit_sharded, D.loglik_sharded,
               M.logistic_model_batched_weighted, M.poisson_model_batched_weighted,
               M.poisson_loglik_batched_weighted):
        assert inspect.signature(fn).parameters["sample_weight"].default is None, fn.__name__


@pytest.mark.parametrize("bad", ["length", "negative", "nan", "inf"])
def test_sample_weight_checked_before_the_gpu(bad, monkeypatch):
    """The ValueError comes before anything touches the GPU: _require_gpu is
    replaced by a function that fails the test."""
    from dlsa_amd import models as M

    def no_gpu(device=None):
        raise AssertionError("the GPU was touched before the sample_weight check")

    monkeypatch.setattr(M, "_require_gpu", no_gpu)
    n, p = 40, 3
    X, y = np.zeros((n, p)), np.zeros(n)
    off = np.array([0, n])
    w = np.ones(n)
    if bad == "length":
        w = np.ones(n - 1)
    else:
        w[7] = {"negative": -1.0, "nan": np.nan, "inf": np.inf}[bad]
    betas = np.zeros((1, p))
    calls = [lambda: M.logistic_model_batched_weighted(X, y, off, sample_weight=w),
             lambda: M.poisson_model_batched_weighted(X, y, off, sample_weight=w),
             lambda: M.poisson_model_batched_weighted(X, y, off, sample_weight=w,
                                                      eta_offset=np.zeros(n)),
             lambda: M.logistic_loglik_batched(X, y, off, betas, sample_weight=w),
             lambda: M.poisson_loglik_batched_weighted(X, y, off, betas, sample_weight=w),
             lambda: M.poisson_loglik_batched_weighted(X, y, off, betas, sample_weight=w,
                                                       exposure=np.ones(n))]
    from dlsa_amd import distributed as D
    calls += [lambda: D.dlsa_fit_sharded(X, y, off, sample_weight=w),
              lambda: D.loglik_sharded(X, y, off, betas, sample_weight=w)]
    for c in calls:
        with pytest.raises(ValueError, match="sample_weight"):
            c()
