"""The pre-pass of the fused fits: the statuses it decides before any Newton
pass and the start point it writes, for the five fits that run it -- Poisson,
Poisson with an offset, logistic with prior weights, Poisson with weights,
Poisson with offset and weights.

One data set of K = 6 partitions of (0, 1, 63, 257, 700, 300) rows, p = 3
with an intercept: the empty case, a single thread, less than one wave, one
row past one 256-row stride, several strides and a plain partition.

Statuses.  Per fit a data set is built from copies of those partitions, each
copy spoilt in one way (the offending row is the copy's last) beside
untouched ones; the expected status of a copy is the documented rule
(include/dlsa_hip.h, csrc/dlsa_internal.hpp):
  a negative or non-finite y, o or omega        NONFINITE
  sum omega = 0, or (Poisson) sum omega y = 0   SINGULAR
  sum omega exp(o) = 0 (o = -800 on every row)  NONFINITE
and where sum omega y = 0 meets sum omega exp(o) = 0 the weighted entries
report SINGULAR, the unweighted ones NONFINITE.  An ended
partition has all-zero outputs and iters = 0; the untouched ones end OK, an
empty one EMPTY.  The untouched 1-row partition is left out there: X^T W X of
one row has rank 1 of P = 4, and what becomes of it is the Newton solve's
verdict on rounded pivots, not the pre-pass's (1-row copies are among the
spoilt ones).  The Python layer refuses a negative or NaN weight with a
ValueError, so the library's own verdict on those two is reached through the
C-ABI entry, as in tests/test_gpu_weighted.py; everything else is the public
Python API.

Start point.  These sizes run no warm-start level, so a fit with hessian =
"fp64" and max_iter = 1 returns the documented start point plus one exact
Newton step: theta against _glm_ref's start + step at the per-entry tolerance
of an exact-phase iterate in tests/test_gpu_newton_steps.py, 1e-8 s + 1e-13
(1 + max |theta|) with s = max |step|.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import oracle as O
from _poison import STATUS_EMPTY, STATUS_NONFINITE, STATUS_SINGULAR

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 257, 700, 300)
P_COLS, FI = 3, True
REL, FLOOR = 1e-8, 1e-13  # tests/test_gpu_newton_steps.py: fp64 iterates
OK, MAXITER = 0, 1
# fit: (family, has an offset, has weights)
FITS = {"poisson": ("poisson", False, False), "poisson_offset": ("poisson", True, False),
        "logistic_weighted": ("logistic", False, True),
        "poisson_weighted": ("poisson", False, True),
        "poisson_offset_weighted": ("poisson", True, True)}
OUTPUTS = ("theta", "sig_inv", "sig_inv_theta", "loglik", "iters")
FIELDS = OUTPUTS + ("status",)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


@functools.lru_cache(maxsize=None)
def _data(name):
    """(X, y, o or None, w or None, offsets) of one fit on the six partitions."""
    family, ofs, wgt = FITS[name]
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(off[-1])
    if family == "logistic":
        X, y = O.simulate_counter(n, P_COLS, seed=103)
        X, o = np.ascontiguousarray(X), None
    elif ofs:
        X, y, o = G.simulate_offset(n, P_COLS, fit_intercept=FI)
    else:
        X, y = G.simulate(n, P_COLS, 7, fit_intercept=FI)
        o = None
    w = None
    if wgt:
        w = G.weights(n, "real").copy()
        w[0] = 1.5  # the 1-row partition keeps its row
    return X, y, o, w, off


def _fit(M, name, X, y, o, w, off, **kw):
    family, ofs, wgt = FITS[name]
    kw = dict(fit_intercept=FI, **kw)
    if ofs:
        kw["eta_offset"] = o
    if wgt:
        kw["sample_weight"] = w
    fn = {"poisson": M.poisson_model_batched, "poisson_offset": M.poisson_model_batched_offset,
          "logistic_weighted": M.logistic_model_batched_weighted,
          "poisson_weighted": M.poisson_model_batched_weighted,
          "poisson_offset_weighted": M.poisson_model_batched_weighted}[name]
    fit = fn(X, y, off, **kw)
    return {f: getattr(fit, f).cpu().numpy() for f in FIELDS}, fit.stats


# ---- statuses -------------------------------------------------------------------------

def _spoil(kind, y, o, w):
    """Spoil one partition's copies of y, o, w in place; the status it must end with."""
    last = len(y) - 1
    if kind == "negative y":
        y[last] = -1.0
    elif kind == "nan y":
        y[last] = np.nan
    elif kind == "zero y":
        y[:] = 0.0
        return STATUS_SINGULAR
    elif kind == "nan o":
        o[last] = np.nan
    elif kind == "o = -800":
        assert y.sum() > 0 and (w is None or (w * y).sum() > 0)
        o[:] = -800.0
    elif kind == "zero y, o = -800":
        y[:] = 0.0
        o[:] = -800.0
        return STATUS_NONFINITE if w is None else STATUS_SINGULAR
    elif kind == "negative w":
        w[last] = -1.0
    elif kind == "nan w":
        w[last] = np.nan
    elif kind == "zero w":
        w[:] = 0.0
        return STATUS_SINGULAR
    elif kind == "w = 0 where y > 0":
        w[y > 0] = 0.0
        assert w.sum() > 0, "the copy needs a row with y = 0 and omega > 0"
        return STATUS_SINGULAR
    else:
        raise ValueError(kind)
    return STATUS_NONFINITE


def _spoilt_kinds(name, refused):
    """(kind, partition of SIZES it is applied to) of one fit; ``refused``: the
    two the Python layer does not let through."""
    family, ofs, wgt = FITS[name]
    kinds = []
    if family == "poisson":
        kinds += [("negative y", 3), ("nan y", 1), ("zero y", 2), ("zero y", 1)]
    if ofs:
        kinds += [("nan o", 2), ("o = -800", 3), ("o = -800", 1), ("zero y, o = -800", 4),
                  ("zero y, o = -800", 1)]
    if wgt:
        kinds += [("zero w", 3), ("zero w", 1)]
        if family == "poisson":
            kinds += [("w = 0 where y > 0", 4), ("w = 0 where y > 0", 5)]
        if refused:
            kinds += [("negative w", 3), ("nan w", 4), ("negative w", 1), ("nan w", 2)]
    return kinds


def _status_data(name, refused):
    """The six partitions' rows rearranged: an empty partition, the untouched
    63-, 257-, 700- and 300-row ones with a second empty one between them, then
    the spoilt copies.  Returns (X, y, o, w, offsets, expected statuses)."""
    X, y, o, w, off = _data(name)
    blocks, want = [], []

    def add(k, kind=None):
        a, b = off[k], off[k + 1]
        blk = [X[a:b].copy(), y[a:b].copy(), None if o is None else o[a:b].copy(),
               None if w is None else w[a:b].copy()]
        st = OK if b > a else STATUS_EMPTY
        if kind is not None:
            st = _spoil(kind, blk[1], blk[2], blk[3])
        blocks.append(blk)
        want.append(st)

    for k in (0, 2, 3, 0, 4, 5):
        add(k)
    for kind, k in _spoilt_kinds(name, refused):
        add(k, kind)
    cat = [None if blocks[0][i] is None else np.concatenate([b[i] for b in blocks])
           for i in range(4)]
    offs = np.concatenate([[0], np.cumsum([len(b[1]) for b in blocks])]).astype(np.int64)
    return cat[0], cat[1], cat[2], cat[3], offs, want


def _check_statuses(tag, got, want):
    print(tag, "status", got["status"].tolist(), "expected", want)
    assert got["status"].tolist() == want, tag
    for k, st in enumerate(want):
        if st != OK:
            for f in OUTPUTS:
                assert not got[f][k].any(), (tag, k, f)
        else:
            assert got["iters"][k] > 0 and np.isfinite(got["theta"][k]).all(), (tag, k)


@pytest.mark.parametrize("name", list(FITS))
def test_statuses(M, name):
    X, y, o, w, off, want = _status_data(name, refused=False)
    got, _ = _fit(M, name, X, y, o, w, off)
    _check_statuses(name, got, want)


@pytest.mark.parametrize("name", [n for n in FITS if FITS[n][2]])
def test_statuses_of_refused_weights(M, name):
    """A negative and a NaN weight: a ValueError from the Python layer, the
    statuses from the library through the C-ABI entry."""
    import torch

    from test_gpu_weighted import _abi_fit

    family, ofs, _ = FITS[name]
    X, y, o, w, off, want = _status_data(name, refused=True)
    with pytest.raises(ValueError, match="sample_weight"):
        _fit(M, name, X, y, o, w, off)
    wd = torch.from_numpy(w).cuda()
    if family == "logistic":
        rc, got = _abi_fit(M, "dlsa_logistic_fit_batched_weighted", X, y, off, FI, [wd])
    else:
        od = torch.from_numpy(o).cuda() if ofs else None
        rc, got = _abi_fit(M, "dlsa_poisson_fit_batched_weighted", X, y, off, FI, [od, wd])
    assert rc == 0
    _check_statuses(name + " (C-ABI)", got, want)


# ---- start point ------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FITS))
def test_start_point_plus_one_step(M, name):
    family = FITS[name][0]
    X, y, o, w, off = _data(name)
    got, stats = _fit(M, name, X, y, o, w, off, hessian="fp64", max_iter=1)
    assert stats["iterations"] == 1  # no warm-start level
    assert got["status"][0] == STATUS_EMPTY
    for k in range(2, len(SIZES)):  # (the 1-row partition: rank 1, the module docstring)
        a, b = off[k], off[k + 1]
        wk = None if w is None else w[a:b]
        ok = None if o is None else o[a:b]
        Z = G.design(X[a:b], FI)
        th0 = G.start(family, y[a:b], Z.shape[1], FI, wk, ok)
        d = G.newton_step(family, Z, y[a:b], th0, wk, ok)
        want = th0 + d
        s = np.abs(d).max()
        tol = REL * s + FLOOR * (1.0 + np.abs(want).max())
        dist = np.abs(got["theta"][k] - want).max()
        print(f"{name} k={k} n={b - a}: start {th0[0]:.6f} |step| {s:.2e} dist {dist:.2e} "
              f"(dist/s {dist / s:.2e}, tolerance {tol:.2e})")
        assert dist <= tol, (name, k, dist, tol)
        assert got["status"][k] == MAXITER and got["iters"][k] == 1, (name, k)
