"""GPU: partitions whose rows, posed as ONE chunk (``rows_per_chunk`` = n_k),
cover more than 2^31 bytes of X -- the 32-bit ranges of the pass kernels.

The fused passes read a chunk's X through one raw buffer resource of at most
0x7FFFFFF0 bytes with 32-bit offsets, and a bounds-checked load past its end
returns zeros: before ``make_plan`` (csrc/fit_plan.hpp) capped a chunk at
``max_chunk_rows(p)`` = (2^31 - 2^20) / (8 p) rows, such a partition was
fitted, status ok, with its later rows read as zero rows.  A longer request is
now split evenly (the caller's value is a hint), so every fit test also reads
the chunk count the plan is documented to produce.

Shapes, the smallest that cover 2^31 bytes: n_k = ceil(1.07 * 2^31 / (8 p)), so
6.5 % of the partition's rows lie past the chunk's 2^31-byte point (each test
asserts both), followed by a second partition of 3001 rows.  p = 191 with an
intercept (P = 192, NT = 12: the cooperative bf16 pass and the cooperative
fp64 exact pass; odd p, so odd rows start 8 modulo 16), p = 99 with an
intercept (NT = 7: the per-wave exact pass, which serves P <= 128 only), p =
63 with an intercept (NT = 4: the OLS stream kernel) and p = 512 (the wide
path).  X and y are generated on the device, once per shape.

The yardstick is never the library at another chunking.  Fits: at the returned
theta the information H, the score g and the log-likelihood are evaluated over
all rows independently of the library (oracle/device_check.py's
``partition_hessians`` for the unweighted logistic and OLS fits, tests/
_torch_ref.py -- tests/_glm_ref.py's formulas in torch fp64 -- for the rest),
and

* the Newton correction H^-1 g is at most 1e-8 max(1, max |theta|): Newton
  converges quadratically, so this is the project's 1e-8 contract on theta
  against the MLE;
* ``sig_inv`` per entry |d_ij| / sqrt(H_ii H_jj) < 1e-10 (fits at tol = 1e-12,
  for the reason in tests/test_gpu_weighted.py's docstring), ``sig_inv_theta``
  within 1e-8, ``loglik`` within 1e-9 relative;
* OLS: tests/test_gpu_dispatch.py::test_ols's three bounds.

Gram, goodness-of-fit and log-likelihood sums: the same torch fp64 evaluation
in 64-row slabs at the tolerances of tests/test_gpu_gram.py (1e-10) and
tests/test_gpu_gof.py / the evaluation tests (1e-12).  That summation order is
not numpy's; ``test_yardstick_reordering`` measures the two against each other
on a 1e5-row prefix and requires a tenth of each tolerance.  The rows pass:
three windows of 4096 rows (the chunk's first rows, those straddling its
2^31-byte point, its last) and one around the middle of the partition, where
the plan now splits it, against tests/_rows_ref.py and its per-row bounds.

On the commit before the cap (its library, this module) every fused fit of a
long chunk came back with status ok and failed: the Newton correction at the
returned theta was 5.9e-3 (logistic P = 192, both modes), 3.5e-3 (P = 100,
both modes), 2.1e-3 and 1.8e-3 (Poisson) against the 1e-8 bound, the OLS theta
6.1e-4 off, and sig_inv 6.6e-2 per entry everywhere: the 6.5 % of the rows
that were read as zeros.  The wide fit, the largest unsplit chunk and the
evaluation-type passes, which use 64-bit pointers, passed; one row more than
the largest chunk was fitted correctly as one chunk (it still ends inside the
buffer range) and failed its chunk count alone.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import _gof_ref as GOF
import _gram_ref as GR
import _rows_ref as RR

pytestmark = pytest.mark.gpu

REL = 1e-8       # theta (through the Newton correction), sig_inv_theta
REL_S = 1e-10    # sig_inv per entry; gram and score (tests/test_gpu_gram.py)
REL_LL = 1e-9    # a fit's loglik
REL_SUM = 1e-12  # deviance, Pearson, evaluated loglik (tests/test_gpu_gof.py)
TOL = 1e-12      # of the fits
TWO31 = 2**31
MAX_CHUNK_BYTES = 2**31 - 2**20  # csrc/fit_plan.hpp: kMaxChunkBytes
SECOND = 3001    # rows of the short partition behind the long one
WINDOW = 4096


def max_chunk_rows(p):
    return MAX_CHUNK_BYTES // (8 * p)


def long_rows(p):
    return -(-int(1.07 * TWO31) // (8 * p))


def _assert_long(n_k, p):
    """The test's precondition: one chunk of n_k rows covers more than 2^31
    bytes of X and at least 5 % of the rows lie wholly past that point."""
    assert n_k * p * 8 > TWO31
    assert n_k - -(-TWO31 // (8 * p)) >= 0.05 * n_k


def _planned_chunks(sizes, p, rpc, limit=None):
    """Chunks of make_plan for rows_per_chunk = rpc: ceil(n / min(rpc, limit))
    per partition, limit = max_chunk_rows(p)."""
    lim = min(rpc, max_chunk_rows(p) if limit is None else limit)
    return sum(-(-n // lim) for n in sizes if n > 0)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


@functools.lru_cache(maxsize=None)
def _data(p):
    """X [n, p], the logistic y and the offsets [0, n_k, n_k + 3001] of one
    shape, on the device, once per process."""
    from dlsa_amd import models

    n_k = long_rows(p)
    X, y = models.simulate_logistic_device(n_k + SECOND, p, seed=1000 + p)
    return X, y, np.array([0, n_k, n_k + SECOND], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _extras(p, fi=True):
    """Of _data(p): a log exposure o ~ U(log 0.2, log 5), weights ~ U(0.2, 5)
    with every 50th row 0, Poisson counts y ~ Poisson(exp(z . b + o)) and a
    Gaussian response z . b + 0.3 N(0, 1); K = 2 coefficient vectors near b
    and two candidates, |eta| <= 12 throughout."""
    import torch

    X, _, off = _data(p)
    n, dev = X.shape[0], X.device
    g = torch.Generator(device=dev).manual_seed(50 + p)
    f64 = dict(dtype=torch.float64, device=dev)
    o = torch.rand(n, generator=g, **f64) * (np.log(5.0) - np.log(0.2)) + np.log(0.2)
    w = torch.rand(n, generator=g, **f64) * 4.8 + 0.2
    w[::50] = 0.0
    rng = np.random.default_rng(p)
    b = np.concatenate([[0.5] * fi, rng.uniform(-1, 1, p) * 1.5 / np.sqrt(p)])
    bd = torch.from_numpy(b).to(dev)
    eta = X @ bd[fi:] + (bd[0] if fi else 0.0)
    ypois = torch.poisson(torch.exp(eta + o), generator=g)
    yols = eta + 0.3 * torch.randn(n, generator=g, **f64)
    thetas = b + rng.standard_normal((2, p + fi)) * 0.5 / np.sqrt(p + fi)
    betas = b + rng.standard_normal((2, p + fi)) * 0.5 / np.sqrt(p + fi)
    assert float(eta.abs().max()) + np.abs(np.vstack([thetas, betas]) - b).sum(1).max() \
        + np.log(5.0) <= 12.0  # |z_f| <= 1
    return dict(o=o, w=w, poisson=ypois, ols=yols, thetas=thetas, betas=betas)


def _check_fit(fit, k, H, g, ll, what):
    """Partition k of a fit against (H, g, loglik) evaluated at its theta;
    prints the figures before it asserts."""
    import torch

    theta = fit.theta[k]
    delta = torch.linalg.solve(H, g)
    d = torch.sqrt(torch.diagonal(H))
    Ht = H @ theta
    e = (float(delta.abs().max() / max(1.0, float(theta.abs().max()))),
         float(((fit.sig_inv[k] - H).abs() / (d[:, None] * d[None, :])).max()),
         float((fit.sig_inv_theta[k] - Ht).abs().max() / Ht.abs().max()),
         abs(float(fit.loglik[k]) - ll) / abs(ll))
    print(f"{what} k={k}: newton correction {e[0]:.2e} sig_inv/entry {e[1]:.2e} "
          f"sig_inv_theta {e[2]:.2e} loglik {e[3]:.2e} iters {int(fit.iters[k])}")
    assert e[0] <= REL, (what, k, "theta: newton correction", e[0])
    assert e[1] < REL_S, (what, k, "sig_inv", e[1])
    assert e[2] < REL, (what, k, "sig_inv_theta", e[2])
    assert e[3] < REL_LL, (what, k, "loglik", e[3])


def _check_logistic(M, fit, X, y, off, what, n_chunks):
    import torch

    import _torch_ref as T
    from oracle import device_check as DC

    assert fit.status.cpu().tolist() == [0] * (len(off) - 1), (what, fit.status)
    H = DC.partition_hessians(X, y, off, fit.theta, family="logistic", fit_intercept=True)
    for k in range(len(off) - 1):
        g, ll = T.score_and_loglik("logistic", X, y, int(off[k]), int(off[k + 1]), fit.theta[k],
                                   True)
        _check_fit(fit, k, H[k], g, ll, what)
    assert torch.equal(fit.sig_inv, fit.sig_inv.transpose(1, 2))
    assert fit.stats["n_chunks"] == n_chunks, (what, fit.stats["n_chunks"], n_chunks)


# ---- the fits ----------------------------------------------------------------------------------

@pytest.mark.parametrize("hessian", ["mixed", "fp64"])
@pytest.mark.parametrize("p", [191, 99])
def test_logistic_fit(M, p, hessian):
    """P = 192: the cooperative bf16 pass (mixed) and the cooperative fp64
    pass; P = 100: the cooperative bf16 pass and the per-wave fp64 pass."""
    X, y, off = _data(p)
    n_k = int(off[1])
    _assert_long(n_k, p)
    fit = M.logistic_model_batched(X, y, off, fit_intercept=True, hessian=hessian, tol=TOL,
                                   rows_per_chunk=n_k)
    _check_logistic(M, fit, X, y, off, f"logistic p={p} {hessian}",
                    _planned_chunks([n_k, SECOND], p, n_k))
    assert fit.stats["n_chunks"] == 3


@pytest.mark.parametrize("p", [191, 99])
def test_poisson_offset_weights_fit(M, p):
    """EX_OFS | EX_WGT in mixed mode: the row streams' 32-bit block offsets
    beside X's."""
    import _torch_ref as T

    X, _, off = _data(p)
    d = _extras(p)
    n_k = int(off[1])
    _assert_long(n_k, p)
    fit = M.poisson_model_batched_weighted(X, d["poisson"], off, sample_weight=d["w"],
                                           eta_offset=d["o"], fit_intercept=True, hessian="mixed",
                                           tol=TOL, rows_per_chunk=n_k)
    assert fit.status.cpu().tolist() == [0, 0], fit.status
    for k in range(2):
        H, g, ll = T.fit_quantities("poisson", X, d["poisson"], int(off[k]), int(off[k + 1]),
                                    fit.theta[k], True, d["w"], d["o"])
        _check_fit(fit, k, H, g, ll, f"poisson ofs+wgt p={p}")
    assert fit.stats["n_chunks"] == _planned_chunks([n_k, SECOND], p, n_k) == 3


def test_ols_fit(M):
    """P = 64 (NT = 4): the OLS stream kernel, whose guard used to hand a
    chunk of 2^31 bytes to a kernel with the same 32-bit range."""
    import torch

    import _torch_ref as T
    from oracle import device_check as DC

    p = 63
    X, _, off = _data(p)
    y = _extras(p)["ols"]
    n_k = int(off[1])
    _assert_long(n_k, p)
    fit = M.ols_model_batched(X, y, off, fit_intercept=True, rows_per_chunk=n_k)
    assert fit.status.cpu().tolist() == [0, 0]
    H = DC.partition_hessians(X, y, off, fit.theta, family="ols", fit_intercept=True)
    for k in range(2):
        a, b = int(off[k]), int(off[k + 1])
        coef = torch.linalg.solve(H[k], T.design(X, a, b, True).T @ y[a:b])
        _, rss = T.score_and_loglik("ols", X, y, a, b, coef, True)
        e = (float((fit.theta[k] - coef).abs().max() / coef.abs().max()),
             float((fit.sig_inv[k] - H[k]).abs().max() / H[k].abs().max()),
             abs(float(fit.loglik[k]) - rss) / rss)
        print(f"ols p={p} k={k} theta {e[0]:.2e} sig_inv {e[1]:.2e} rss {e[2]:.2e}")
        assert e[0] < 1e-8
        assert e[1] < 1e-12
        assert e[2] < 1e-6
    assert fit.stats["n_chunks"] == _planned_chunks([n_k, SECOND], p, n_k) == 3


def test_wide_logistic_fit(M):
    """p = 512: the wide path's row plan (one chunk per partition as asked,
    now capped) and its Gram row groups (2^30 bytes at most, as before)."""
    p = 512
    X, y, off = _data(p)
    n_k = int(off[1])
    _assert_long(n_k, p)
    fit = M.logistic_model_batched(X, y, off, fit_intercept=False, tol=TOL, rows_per_chunk=n_k)
    import torch

    import _torch_ref as T
    from oracle import device_check as DC

    assert fit.status.cpu().tolist() == [0, 0], fit.status
    H = DC.partition_hessians(X, y, off, fit.theta, family="logistic", fit_intercept=False)
    for k in range(2):
        g, ll = T.score_and_loglik("logistic", X, y, int(off[k]), int(off[k + 1]), fit.theta[k],
                                   False)
        _check_fit(fit, k, H[k], g, ll, "wide logistic p=512")
    assert torch.equal(fit.sig_inv, fit.sig_inv.transpose(1, 2))
    # stats.n_chunks of the wide path counts the Gram row groups
    assert fit.stats["n_chunks"] == _planned_chunks([n_k, SECOND], p, n_k, 2**30 // (8 * p)) == 4


@pytest.mark.parametrize("extra", [0, 1], ids=["largest", "one-more"])
@pytest.mark.parametrize("p,hessian", [(191, "mixed"), (99, "fp64")])
def test_largest_unsplit_chunk(M, p, hessian, extra):
    """max_chunk_rows(p) rows are honoured as one chunk, one row more is
    two: both within the bounds."""
    X, y, _ = _data(p)
    n = max_chunk_rows(p) + extra
    assert n * 8 * p <= MAX_CHUNK_BYTES if not extra else n * 8 * p > MAX_CHUNK_BYTES
    assert n <= X.shape[0]
    off = np.array([0, n], dtype=np.int64)
    fit = M.logistic_model_batched(X[:n], y[:n], off, fit_intercept=True, hessian=hessian,
                                   tol=TOL, rows_per_chunk=n)
    _check_logistic(M, fit, X[:n], y[:n], off, f"logistic p={p} {hessian} n={n}", 1 + extra)


# ---- the evaluation-type passes ---------------------------------------------------------------

def _host_prefix(p, m):
    X, y, _ = _data(p)
    d = _extras(p)
    return (X[:m].cpu().numpy(), y[:m].cpu().numpy(), d["poisson"][:m].cpu().numpy(),
            d["o"][:m].cpu().numpy(), d["w"][:m].cpu().numpy())


def test_yardstick_reordering():
    """tests/_torch_ref.py's 64-row-slab sums against numpy's on the first 1e5
    rows: a tenth of each tolerance at the most, so no bound of this module is
    tighter than the yardstick's own summation error.  Measured on an MI355X:
    gram 4.0e-16 (score) and 1.9e-16 (information) of the largest entry,
    score 1.1e-16 and its scale 2.0e-15 relative, deviance and Pearson equal
    to the last bit, loglik 2.2e-16."""
    import _torch_ref as T

    p, m = 191, 100000
    X, _, _ = _data(p)
    d = _extras(p)
    Xh, _, yh, oh, wh = _host_prefix(p, m)
    Z = G.design(Xh, True)
    th = d["thetas"][0]
    thd = X.new_tensor(th)
    for kind in ("score", "information"):
        Gw, sw, scale = GR.gram("poisson", Z, yh, th, wh, oh, kind)
        Gt, st, scale_t = T.gram("poisson", X, d["poisson"], 0, m, thd, True, d["w"], d["o"], kind)
        e = (np.abs(Gt.cpu().numpy() - Gw).max() / np.abs(Gw).max(),
             np.abs(st.cpu().numpy() - sw).max() / scale, abs(scale_t / scale - 1))
        print(f"torch slabs vs numpy, {kind}: gram {e[0]:.2e} score {e[1]:.2e} scale {e[2]:.2e}")
        assert max(e) <= 0.1 * REL_S
    want = GOF.gof("poisson", Z, yh, th, wh, oh)
    got = T.gof("poisson", X, d["poisson"], 0, m, thd, True, d["w"], d["o"])
    ll = (T.loglik("poisson", X, d["poisson"], 0, m, thd, True, d["w"], d["o"]),
          G.loglik("poisson", Z, yh, th, wh, oh))
    e = (abs(got[0] / want[0] - 1), abs(got[1] / want[1] - 1), abs(ll[0] / ll[1] - 1))
    print(f"torch slabs vs numpy: deviance {e[0]:.2e} pearson {e[1]:.2e} loglik {e[2]:.2e}")
    assert got[2] == want[2] and max(e) <= 0.1 * REL_SUM


@pytest.mark.parametrize("kind", ["score", "information"])
def test_gram(M, kind):
    """Poisson with both row extras, each partition at its own theta."""
    import _torch_ref as T

    p = 191
    X, _, off = _data(p)
    d = _extras(p)
    n_k = int(off[1])
    _assert_long(n_k, p)
    g = M.glm_gram_batched("poisson", X, d["poisson"], off, thetas=d["thetas"], kind=kind,
                           eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True,
                           rows_per_chunk=n_k)
    for k in range(2):
        Gw, sw, scale = T.gram("poisson", X, d["poisson"], int(off[k]), int(off[k + 1]),
                               X.new_tensor(d["thetas"][k]), True, d["w"], d["o"], kind)
        a = g["gram"][k]
        assert bool((a == a.T).all()), (kind, k, "gram is not exactly symmetric")
        e = (float((a - Gw).abs().max() / Gw.abs().max()),
             float((g["score"][k] - sw).abs().max() / scale))
        print(f"gram {kind} k={k}: gram {e[0]:.3e} score {e[1]:.3e}")
        assert e[0] <= REL_S, (kind, k, "gram", e[0])
        assert e[1] <= REL_S, (kind, k, "score", e[1])


def test_gof_and_loglik(M):
    """B = 2 candidates: deviance, Pearson, n_pos and the weighted Poisson
    log-likelihood with the offset."""
    import _torch_ref as T

    p = 191
    X, _, off = _data(p)
    d = _extras(p)
    _assert_long(int(off[1]), p)
    kw = dict(eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True)
    got = M.glm_gof_batched("poisson", X, d["poisson"], off, betas=d["betas"], **kw)
    ll = M.poisson_loglik_batched_weighted(X, d["poisson"], off, d["betas"], **kw)
    assert ll.shape == (2, 2)
    for k in range(2):
        for j in range(2):
            a, b, bt = int(off[k]), int(off[k + 1]), X.new_tensor(d["betas"][j])
            dev, chi, npos = T.gof("poisson", X, d["poisson"], a, b, bt, True, d["w"], d["o"])
            want_ll = T.loglik("poisson", X, d["poisson"], a, b, bt, True, d["w"], d["o"])
            e = (abs(float(got["deviance"][k, j]) / dev - 1),
                 abs(float(got["pearson"][k, j]) / chi - 1), abs(float(ll[k, j]) / want_ll - 1))
            print(f"gof k={k} B={j}: deviance {e[0]:.3e} pearson {e[1]:.3e} loglik {e[2]:.3e}")
            assert max(e) <= REL_SUM, (k, j, e)
            assert int(got["n_pos"][k]) == npos


def test_rows(M, monkeypatch):
    """All five streams (and Cook's distances) in four windows of 4096 rows of
    the long partition, and all of the short one, at their global indices."""
    from test_gpu_rows import _check

    p, P, K = 191, 192, 2
    X, _, off = _data(p)
    d = _extras(p)
    n_k = int(off[1])
    _assert_long(n_k, p)
    kw = dict(eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True)
    info = M.glm_gram_batched("poisson", X, d["poisson"], off, thetas=d["thetas"],
                              kind="information", **kw)["gram"].cpu().numpy()
    R = M.rows_factor(info, K, P)  # once, for both sides
    assert np.isfinite(R).all()
    monkeypatch.setattr(M, "rows_factor", lambda *a: R)
    got = M.glm_rows_batched("poisson", X, d["poisson"], off, thetas=d["thetas"], info=info,
                             rows_per_chunk=n_k, **kw)
    monkeypatch.undo()
    cross = -(-TWO31 // (8 * p))  # the first row wholly past the chunk's 2^31-byte point
    starts = {"first": 0, "2^31 bytes": cross - WINDOW // 2, "middle": n_k // 2 - WINDOW // 2,
              "last": n_k - WINDOW, "second partition": n_k}
    assert 0 < starts["2^31 bytes"] and cross + WINDOW // 2 < n_k - WINDOW
    for name, a in starts.items():
        k = int(a >= n_k)
        b = a + (SECOND if k else WINDOW)
        h = {s: v[a:b].cpu().numpy() for s, v in got.items()}
        Z = G.design(X[a:b].cpu().numpy(), True)
        args = ("poisson", Z, d["poisson"][a:b].cpu().numpy(), d["thetas"][k])
        ex = dict(w=d["w"][a:b].cpu().numpy(), o=d["o"][a:b].cpu().numpy())
        ref = RR.rows(*args, R=R[k], **ex)
        bnd = RR.bounds(*args, ref=ref, **ex)
        _check(h, ref, bnd, np.array([0, b - a]), R[k], f"rows window {name} [{a}, {b})")
