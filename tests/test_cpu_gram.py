"""CPU: the yardstick of the score outer-product pass (tests/_gram_ref.py)
pinned three ways, ``distributed.sandwich_cov``, a Monte-Carlo check of the
DLSA sandwich formula on over-dispersed counts, the Python surface and its
argument checks, and the two-rank combine of ``gram_sharded`` under gloo."""

import ctypes
import inspect
import os

import numpy as np
import pytest

import _glm_ref as G
import _gram_ref as R

CASES = [("logistic", False, False), ("logistic", True, False), ("poisson", False, False),
         ("poisson", True, False), ("poisson", True, True)]
CASE_IDS = ["logistic", "logistic-wgt", "poisson", "poisson-wgt", "poisson-wgt-ofs"]


def _small(family, wgt, ofs, n=200, p=3):
    rng = np.random.default_rng(5)
    Z = G.design(rng.standard_normal((n, p)) * 0.6, True)
    theta = np.array([0.3, 0.5, -0.4, 0.2])
    o = rng.uniform(np.log(0.5), np.log(2.0), n) if ofs else None
    eta = Z @ theta + (0.0 if o is None else o)
    y = (rng.poisson(np.exp(eta)) if family == "poisson"
         else (rng.uniform(size=n) < G._expit(eta))).astype(np.float64)
    w = G.weights(n, "real") if wgt else None
    return Z, y, theta + 0.1, w, o  # away from the truth: a score that is not ~0


# ---- the yardstick ----------------------------------------------------------------------------

@pytest.mark.parametrize("family,wgt,ofs", CASES, ids=CASE_IDS)
def test_meat_is_the_sum_of_single_row_gradient_outer_products(family, wgt, ofs):
    Z, y, theta, w, o = _small(family, wgt, ofs)
    M, g, _ = R.gram(family, Z, y, theta, w, o)
    want, gsum = np.zeros_like(M), np.zeros_like(g)
    for i in range(len(y)):
        gi, _ = G.grad_hess(family, Z[i:i + 1], y[i:i + 1], theta,
                            None if w is None else w[i:i + 1], None if o is None else o[i:i + 1])
        want += np.outer(gi, gi)
        gsum += gi
    assert np.abs(M - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(g - gsum).max() <= 1e-12 * np.abs(gsum).max()


@pytest.mark.parametrize("family,wgt,ofs", CASES, ids=CASE_IDS)
def test_score_is_the_gradient_of_the_loglik(family, wgt, ofs):
    Z, y, theta, w, o = _small(family, wgt, ofs)
    _, g, _ = R.gram(family, Z, y, theta, w, o)
    h = 1e-5
    fd = np.array([(G.loglik(family, Z, y, theta + h * e, w, o) -
                    G.loglik(family, Z, y, theta - h * e, w, o)) / (2 * h)
                   for e in np.eye(len(theta))])
    assert np.abs(g - fd).max() <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("family,wgt,ofs", CASES, ids=CASE_IDS)
def test_information_is_the_hessian_bit_for_bit(family, wgt, ofs):
    Z, y, theta, w, o = _small(family, wgt, ofs)
    info, _, _ = R.gram(family, Z, y, theta, w, o, kind="information")
    assert np.array_equal(info, G.hessian(family, Z, theta, w, o))


def test_gram_partitions_stacks_and_zeroes_the_empty_one():
    Z, y, theta, w, o = _small("poisson", True, True)
    off = np.array([0, 70, 70, 200])
    th = np.stack([theta, theta * 0, theta * 1.1])
    Gm, sc, scale = R.gram_partitions("poisson", Z, y, off, thetas=th, w=w, o=o)
    assert not Gm[1].any() and not sc[1].any() and scale[1] == 0.0
    M2, g2, s2 = R.gram("poisson", Z[70:], y[70:], th[2], w[70:], o[70:])
    assert np.array_equal(Gm[2], M2) and np.array_equal(sc[2], g2) and scale[2] == s2
    Gb, _, _ = R.gram_partitions("poisson", Z, y, off, beta=theta, w=w, o=o)
    assert np.array_equal(Gb[0], R.gram("poisson", Z[:70], y[:70], theta, w[:70], o[:70])[0])


# ---- sandwich_cov -----------------------------------------------------------------------------

def _spd(P, seed):
    B = np.random.default_rng(seed).standard_normal((4 * P, P))
    return B.T @ B / (4 * P) + np.eye(P)


def test_sandwich_cov_reduces_to_the_dispersion_scaling():
    from dlsa_amd.distributed import sandwich_cov

    A, phi = _spd(7, 1), 3.7
    cov, info = sandwich_cov(A, phi * A)
    assert np.abs(info - A / phi).max() <= 1e-12 * np.abs(A / phi).max()
    want = phi * np.linalg.inv(A)
    assert np.abs(cov - want).max() <= 1e-12 * np.abs(want).max()


def test_sandwich_cov_general_symmetric_and_rank_deficient():
    from dlsa_amd.distributed import sandwich_cov

    A, M = _spd(6, 2), _spd(6, 3) * 2.5
    cov, info = sandwich_cov(A, M)
    wc, wi = R.sandwich(A, M)
    assert np.abs(cov - wc).max() <= 1e-12 * np.abs(wc).max()
    assert np.abs(info - wi).max() <= 1e-12 * np.abs(wi).max()
    assert np.array_equal(cov, cov.T) and np.array_equal(info, info.T)
    assert np.abs(cov @ info - np.eye(6)).max() <= 1e-12
    B = np.random.default_rng(4).standard_normal((6, 4))  # 4 rows' outer products at P = 6
    with pytest.raises(ValueError, match="positive definite"):
        sandwich_cov(A, B @ B.T)
    with pytest.raises(ValueError, match="positive definite"):
        sandwich_cov(A, np.zeros((6, 6)))
    with pytest.raises(ValueError):
        sandwich_cov(A, M[:5, :5])


# ---- Monte Carlo: the DLSA formula on over-dispersed counts -----------------------------------

def test_sandwich_matches_the_spread_of_the_partition_estimates():
    """NB2 counts (Var y = mu + mu^2), K = 64 partitions of 1500 rows, p = 4 and
    an intercept, seed 3.  diag(A^-1 sum M A^-1) over the empirical variance of
    the theta_k across partitions divided by K lies in [0.6, 1.7] (0.98-1.33
    where the formula was first checked, 0.88-1.25 here; the band adds the
    +-18 % sampling error of a variance on 63 degrees of freedom), the
    model-based diag(A^-1) ratio below 0.5 (0.25-0.35 there, 0.23-0.34 here)."""
    from dlsa_amd.distributed import sandwich_cov

    X, y, off = R.negbin_job(3)
    K = len(off) - 1
    fits = G.fit_partitions("poisson", X, y, off, fit_intercept=True)
    Z = G.design(X, True)
    Mk, _, _ = R.gram_partitions("poisson", Z, y, off, thetas=fits["theta"])
    A, M = fits["sig_inv"].sum(0), Mk.sum(0)
    cov, _ = sandwich_cov(A, M)
    emp = fits["theta"].var(axis=0, ddof=1) / K
    robust = np.diag(cov) / emp
    model = np.diag(np.linalg.inv(A)) / emp
    print("HC0 / empirical", np.round(robust, 3), "model / empirical", np.round(model, 3))
    assert robust.min() >= 0.6 and robust.max() <= 1.7
    assert model.max() < 0.5


# ---- Python surface ---------------------------------------------------------------------------

def test_signatures():
    from dlsa_amd import _hip
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    ps = inspect.signature(M.glm_gram_batched).parameters
    assert list(ps)[:4] == ["family", "X", "y", "offsets"]
    for name, default in (("thetas", None), ("beta", None), ("kind", "score"),
                          ("eta_offset", None), ("exposure", None), ("sample_weight", None),
                          ("fit_intercept", False), ("center", None), ("scale", None),
                          ("return_sum", False), ("rows_per_chunk", 0), ("device", None)):
        assert ps[name].default == default, name
    ps = inspect.signature(D.gram_sharded).parameters
    assert "group" in ps and ps["kind"].default == "score" and ps["family"].default == "logistic"
    assert list(inspect.signature(D.sandwich_cov).parameters) == ["A", "M"]
    assert inspect.signature(D.dlsa_fit_sharded).parameters["cov_type"].default is None
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    want = [I32, I32, P, P, P, P, P, I32, I32, I32, P, P, P, I64, P, P, P, P, P]
    assert _hip.SIGNATURES["dlsa_glm_gram_batched"] == (ctypes.c_int, want)
    assert _hip.SIGNATURES["dlsa_glm_gram_batched_chunked"] == (
        ctypes.c_int, want[:14] + [I32] + want[14:])
    assert (_hip.GRAM_SCORE, _hip.GRAM_INFORMATION) == (0, 1)
    lib = ctypes.CDLL(_hip.LIB_PATH)  # exported (the library loads without a GPU)
    assert lib.dlsa_glm_gram_batched and lib.dlsa_glm_gram_batched_chunked


def test_entry_rejects_bad_arguments_before_any_launch():
    """The C entry's argument errors need no GPU: they come before any HIP call."""
    from dlsa_amd import _hip

    lib = _hip.load()
    off = np.array([0, 0], dtype=np.int64)
    offp = off.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(200 * 200)
    b = buf.ctypes.data_as(ctypes.c_void_p)

    def call(family=_hip.FAMILY_POISSON, kind=0, o=None, p=3, ic=1, stride=0):
        return lib.dlsa_glm_gram_batched(family, kind, None, None, o, None, offp, 1, p, ic, None,
                                         None, b, stride, b, b, None, None, None)

    assert call(family=1) == -3  # DLSA_E_UNSUPPORTED: the Gaussian family's code
    assert call(p=192, ic=1) == -3 and "DLSA_MAX_P_FUSED" in _hip.last_error()
    assert call(stride=3) == -1  # DLSA_E_INVALID: neither 0 nor P = 4
    assert call(family=_hip.FAMILY_LOGISTIC, o=b) == -1 and "Poisson" in _hip.last_error()
    assert call(kind=2) == -1


def test_arguments_checked_before_the_gpu(monkeypatch):
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    def no_gpu(device=None):
        raise AssertionError("the GPU was touched before the argument check")

    monkeypatch.setattr(M, "_require_gpu", no_gpu)
    n, p = 40, 2
    X, y, off = np.zeros((n, p)), np.zeros(n), np.array([0, 25, n])
    th, be = np.zeros((2, p)), np.zeros(p)
    bad = [
        (dict(thetas=th, kind="meat"), "kind"),
        (dict(), "exactly one"),
        (dict(thetas=th, beta=be), "exactly one"),
        (dict(thetas=th, family="gaussian"), "family"),
        (dict(thetas=th, eta_offset=np.zeros(n)), "poisson"),
        (dict(thetas=th, family="poisson", eta_offset=np.zeros(n), exposure=np.ones(n)),
         "not both"),
        (dict(thetas=th, family="poisson", exposure=np.zeros(n)), "exposure"),
        (dict(thetas=th, sample_weight=-np.ones(n)), "sample_weight"),
        (dict(thetas=th, sample_weight=np.ones(n - 1)), "n entries"),
        (dict(thetas=np.zeros((3, p))), "thetas must be"),
        (dict(beta=np.zeros(p + 1)), "beta must be"),
        (dict(thetas=th, rows_per_chunk=-1), "rows_per_chunk"),
        (dict(thetas=th, center=np.zeros(p)), "center and scale"),
    ]
    for kw, match in bad:
        kw = dict(kw)
        family = kw.pop("family", "logistic")
        with pytest.raises(ValueError, match=match):
            M.glm_gram_batched(family, X, y, off, **kw)
        with pytest.raises(ValueError, match=match):
            D.gram_sharded(X, y, off, family=family, **kw)
    codes = np.zeros((n, 1), np.uint8)
    for kw, match in [
        (dict(cov_type="HC2"), "cov_type"),
        (dict(cov_type="HC0", dispersion="pearson"), "absorbs"),
        (dict(cov_type="HC1", dispersion="pearson"), "absorbs"),
        (dict(cov_type="HC0", codes=codes, levels=[3]), "dense layout only"),
        (dict(cov_type="HC1", codes=codes, levels=[3]), "dense layout only"),
    ]:
        with pytest.raises(ValueError, match=match):
            D.dlsa_fit_sharded(X, y, off, **kw)


def test_cov_type_none_leaves_the_result_unchanged(monkeypatch):
    """cov_type=None takes today's path: the same calls with the same
    arguments, no new key (a stubbed fit and reduction; the GPU comparison is
    in tests/test_gpu_gram.py)."""
    from dlsa_amd import distributed as D
    from dlsa_amd import models as M

    P = 3
    A = _spd(P, 9)

    class Fit:
        pass

    fit = Fit()
    fit.P = P
    import torch

    monkeypatch.setattr(M, "logistic_model_batched", lambda *a, **k: fit)
    buf = np.concatenate([A.ravel(), A @ np.ones(P), 2 * np.ones(P), [2.0, 5000.0]])
    monkeypatch.setattr(D, "reduce_partitions_device",
                        lambda f, n_rows=False: torch.from_numpy(buf.copy()))
    X, y, off = np.zeros((10, P)), np.zeros(10), [0, 10]
    plain = D.dlsa_fit_sharded(X, y, off)
    none = D.dlsa_fit_sharded(X, y, off, cov_type=None)
    assert set(none) == set(plain) and "cov" not in none
    assert np.array_equal(none["wlse"], plain["wlse"])
    model = D.dlsa_fit_sharded(X, y, off, cov_type="model")
    assert set(model) - set(plain) == {"cov", "std_err", "z", "p_value"}
    assert np.array_equal(model["wlse"], plain["wlse"])
    want = np.linalg.inv(A)
    assert np.abs(model["cov"] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.allclose(model["std_err"], np.sqrt(np.diag(want)), rtol=1e-12)
    assert np.allclose(model["z"], model["wlse"] / model["std_err"], rtol=1e-15)
    import math
    assert model["p_value"][0] == math.erfc(abs(model["z"][0]) / math.sqrt(2.0))


# ---- the combine of gram_sharded under gloo, world_size 2 ------------------------------------

def _gloo_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    from dlsa_amd.distributed import combine_gram

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    P = 5
    rng = np.random.default_rng(100 + rank)
    Gl, sl = rng.standard_normal((P, P)), rng.standard_normal(P)
    calls = []
    orig = dist.all_reduce

    def counting(t, *a, **k):
        calls.append(t.numel())
        return orig(t, *a, **k)

    dist.all_reduce = counting
    try:
        Gt, st = combine_gram(torch.from_numpy(Gl), torch.from_numpy(sl))
    finally:
        dist.all_reduce = orig
    q.put((rank, Gt, st, calls))
    dist.destroy_process_group()


def test_gram_combine_gloo_two_ranks():
    """ONE all-reduce of P^2 + P doubles gives every rank the sum of the two
    ranks' [gram_sum | score_sum]."""
    import multiprocessing as mp
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p_ in ps:
        p_.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p_ in ps:
        p_.join(timeout=60)
        assert p_.exitcode == 0
    P = 5
    rngs = [np.random.default_rng(100 + r) for r in range(2)]
    loc = [(g.standard_normal((P, P)), g.standard_normal(P)) for g in rngs]
    wantG, wants = loc[0][0] + loc[1][0], loc[0][1] + loc[1][1]
    for rank, Gt, st, calls in res:
        assert calls == [P * P + P], calls
        assert np.array_equal(Gt, wantG) and np.array_equal(st, wants)
