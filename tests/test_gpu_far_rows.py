"""GPU: rows past the first 4 GiB of X -- the 64-bit address arithmetic of the
fits and of the evaluation-type passes (Gram, goodness of fit, log-likelihood,
rows), which no other module shows a row whose offset needs more than 32 bits
(tests/test_gpu_scale.py::test_config2_full_K1024 does, for the plain logistic
fit alone).

One X of a little more than 2^31 doubles, generated on the device once per
module: p = 191 with an intercept (P = 192; odd p, so odd rows start 8 modulo
16), n = 11.3 million rows (17.3 GB), with y for both families, a log exposure
and prior weights.  Small partitions lie where a row's offset crosses a power
of two -- their rows are computed from p and asserted:

* 3001 rows straddling byte 2^32 of X, then a partition of one row;
* 3001 rows straddling element 2^31 of X (byte 2^34);
* 2003 rows ending at the last row of the allocation,

with ordinary filler partitions of about 1e5 rows and automatic chunks in
between.  The small partitions are copied to the host and compared with the
numpy yardsticks of the modules that test each pass at small n, at those
modules' own tolerances: tests/_glm_ref.py (the contracts of
tests/test_gpu_weighted.py), _gram_ref.py (test_gpu_gram.py), _gof_ref.py
(test_gpu_gof.py, and 1e-12 for the log-likelihood) and _rows_ref.py (its
per-row bounds; the outputs are read at the partitions' global indices).  Of
the fillers only status 0 and the exact symmetry of sig_inv / gram are asserted.

Out of scope: the categorical-code layout.  Its code stream reaches 2^32
bytes only at 8.6e8 rows with F = 5 factors, and its numeric block at q = 9
needs 3e7 rows in one workgroup for a chunk of 2^31 bytes -- both beyond a
test of seconds -- and its addressing is plain 64-bit pointer arithmetic.
"""

import functools

import numpy as np
import pytest

import _glm_ref as G
import _gof_ref as GOF
import _gram_ref as GR
import _rows_ref as RR

pytestmark = pytest.mark.gpu

P_COLS, P = 191, 192
TOL = 1e-12  # of the fits (tests/test_gpu_weighted.py's docstring)
REL, REL_S, REL_LL = 1e-8, 1e-10, 1e-9  # tests/test_gpu_weighted.py
FILLER = 100000


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    from dlsa_amd import models
    return models


@functools.lru_cache(maxsize=None)
def _layout(p=P_COLS):
    """(offsets [K + 1], the small partitions' indices by name)."""
    r32 = 2**32 // (8 * p)  # the row that holds byte 2^32 of X
    r31 = 2**31 // p        # the row that holds element 2^31
    a0, a1 = r32 - 1500, r32 + 1501
    b0, b1 = r31 - 1500, r31 + 1501
    n = b1 + FILLER // 2 + 2003
    assert a0 * 8 * p < r32 * 8 * p <= 2**32 < (r32 + 1) * 8 * p < a1 * 8 * p
    assert b0 * p < r31 * p <= 2**31 < (r31 + 1) * p < b1 * p and n * p > 2**31
    edges, small = [0], {}

    def fillers(end):
        m = max(1, round((end - edges[-1]) / FILLER))
        edges.extend(int(v) for v in np.linspace(edges[-1], end, m + 1)[1:])

    def part(name, end):
        small[name] = len(edges) - 1
        edges.append(end)

    fillers(a0)
    part("byte 2^32", a1)
    part("one row", a1 + 1)
    fillers(b0)
    part("element 2^31", b1)
    fillers(n - 2003)
    part("last rows", n)
    off = np.array(edges, dtype=np.int64)
    assert (np.diff(off) > 0).all() and off[-1] == n
    assert [int(off[k + 1] - off[k]) for k in small.values()] == [3001, 1, 3001, 2003]
    return off, small


@functools.lru_cache(maxsize=None)
def _data():
    """Device: X, the logistic y, a log exposure o ~ U(log 0.2, log 5), weights
    ~ U(0.2, 5) with every 50th row 0, Poisson counts y ~ Poisson(exp(z . b +
    o)); host: [K, P] coefficients near b and three candidates, |eta| <= 12."""
    import torch

    from dlsa_amd import models

    off, _ = _layout()
    n, p, K = int(off[-1]), P_COLS, len(off) - 1
    X, ylog = models.simulate_logistic_device(n, p, seed=31)
    g = torch.Generator(device=X.device).manual_seed(32)
    f64 = dict(dtype=torch.float64, device=X.device)
    o = torch.rand(n, generator=g, **f64) * (np.log(5.0) - np.log(0.2)) + np.log(0.2)
    w = torch.rand(n, generator=g, **f64) * 4.8 + 0.2
    w[::50] = 0.0
    assert float(w[int(off[_layout()[1]["one row"]])]) > 0  # the one-row partition weighs
    rng = np.random.default_rng(p)
    b = np.concatenate([[0.5], rng.uniform(-1, 1, p) * 1.5 / np.sqrt(p)])
    bd = torch.from_numpy(b).to(X.device)
    eta = X @ bd[1:] + bd[0]
    ypois = torch.poisson(torch.exp(eta + o), generator=g)
    thetas = b + rng.standard_normal((K, P)) * 0.5 / np.sqrt(P)
    betas = b + rng.standard_normal((3, P)) * 0.5 / np.sqrt(P)
    assert float(eta.abs().max()) + np.abs(np.vstack([thetas, betas]) - b).sum(1).max() \
        + np.log(5.0) <= 12.0  # |z_f| <= 1
    return dict(X=X, logistic=ylog, poisson=ypois, o=o, w=w, thetas=thetas, betas=betas)


@functools.lru_cache(maxsize=None)
def _small():
    """The small partitions' rows on the host, concatenated: X, Z, both y, o, w,
    their offsets, their indices among the K partitions and, per row, its
    global index."""
    off, small = _layout()
    d = _data()
    ks = list(small.values())
    rows = np.concatenate([np.arange(off[k], off[k + 1]) for k in ks])
    cat = lambda t: np.concatenate([t[int(off[k]):int(off[k + 1])].cpu().numpy() for k in ks])  # noqa: E731
    X = cat(d["X"])
    out = dict(X=X, Z=G.design(X, True), logistic=cat(d["logistic"]), poisson=cat(d["poisson"]),
               o=cat(d["o"]), w=cat(d["w"]), ks=ks, rows=rows,
               off=np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in ks])]).astype(np.int64))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _per_entry(S, H):
    d = np.sqrt(np.abs(np.diag(H)))
    return (np.abs(S - H) / np.outer(d, d)).max()


def _check_fit(fit, ref, what):
    """The small partitions of `fit` against `ref` (_glm_ref.fit_partitions of
    all but the one-row partition, which cannot carry P = 192 coefficients and
    must not come back ok); the fillers: status 0, sig_inv exactly symmetric."""
    import torch

    off, small = _layout()
    status = fit.status.cpu().numpy()
    assert status[small["one row"]] != 0, (what, "a one-row partition with status ok")
    rest = np.delete(np.arange(len(off) - 1), small["one row"])
    assert (status[rest] == 0).all(), (what, np.flatnonzero(status != 0), status[status != 0])
    assert torch.equal(fit.sig_inv, fit.sig_inv.transpose(1, 2)), (what, "sig_inv symmetry")
    names = [nm for nm in small if nm != "one row"]
    for j, nm in enumerate(names):
        k = small[nm]
        got = {f: getattr(fit, f)[k].cpu().numpy() for f in
               ("theta", "sig_inv", "sig_inv_theta", "loglik")}
        e = (_rel(got["theta"], ref["theta"][j]), _per_entry(got["sig_inv"], ref["sig_inv"][j]),
             _rel(got["sig_inv_theta"], ref["sig_inv_theta"][j]),
             abs(got["loglik"] - ref["loglik"][j]) / abs(ref["loglik"][j]))
        print(f"{what} [{nm}] k={k}: theta {e[0]:.2e} sig_inv/entry {e[1]:.2e} "
              f"sig_inv_theta {e[2]:.2e} loglik {e[3]:.2e}")
        assert e[0] < REL and e[1] < REL_S and e[2] < REL and e[3] < REL_LL, (what, nm, e)


def _without_one_row(s):
    """(row mask, offsets) of the small partitions less the one-row one."""
    j = list(_layout()[1]).index("one row")
    keep = np.ones(len(s["rows"]), bool)
    keep[s["off"][j]:s["off"][j + 1]] = False
    sizes = np.delete(np.diff(s["off"]), j)
    return keep, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_poisson_offset_weights_fit(M):
    d, s = _data(), _small()
    off, _ = _layout()
    fit = M.poisson_model_batched_weighted(d["X"], d["poisson"], off, sample_weight=d["w"],
                                           eta_offset=d["o"], fit_intercept=True, hessian="mixed",
                                           tol=TOL)
    keep, soff = _without_one_row(s)
    ref = G.fit_partitions("poisson", s["X"][keep], s["poisson"][keep], soff, w=s["w"][keep],
                           o=s["o"][keep], fit_intercept=True)
    _check_fit(fit, ref, "poisson ofs+wgt mixed")


def test_logistic_fp64_fit(M):
    d, s = _data(), _small()
    off, _ = _layout()
    fit = M.logistic_model_batched(d["X"], d["logistic"], off, fit_intercept=True, hessian="fp64",
                                   tol=TOL)
    keep, soff = _without_one_row(s)
    ref = G.fit_partitions("logistic", s["X"][keep], s["logistic"][keep], soff,
                           fit_intercept=True)
    _check_fit(fit, ref, "logistic fp64")


@pytest.mark.parametrize("kind", ["score", "information"])
def test_gram(M, kind):
    import torch

    from test_gpu_gram import _check

    d, s = _data(), _small()
    off, _ = _layout()
    g = M.glm_gram_batched("poisson", d["X"], d["poisson"], off, thetas=d["thetas"], kind=kind,
                           eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True)
    assert torch.equal(g["gram"], g["gram"].transpose(1, 2)), "gram is not exactly symmetric"
    assert bool(torch.isfinite(g["gram"]).all()) and bool(torch.isfinite(g["score"]).all())
    got = {k: v[s["ks"]].cpu().numpy() for k, v in g.items()}
    want = GR.gram_partitions("poisson", s["Z"], s["poisson"], s["off"], thetas=d["thetas"][s["ks"]],
                              w=s["w"], o=s["o"], kind=kind)
    _check(got, want, f"far rows {kind}")


def test_gof_and_weighted_loglik(M):
    import torch

    from test_gpu_gof import _check

    d, s = _data(), _small()
    off, _ = _layout()
    kw = dict(eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True)
    g = M.glm_gof_batched("poisson", d["X"], d["poisson"], off, betas=d["betas"][:2], **kw)
    got = {k: v[s["ks"]].cpu().numpy() for k, v in g.items()}
    _check(got, GOF.gof_partitions("poisson", s["Z"], s["poisson"], s["off"], betas=d["betas"][:2],
                                   w=s["w"], o=s["o"]), "far rows gof")
    ll = M.poisson_loglik_batched_weighted(d["X"], d["poisson"], off, d["betas"], **kw)
    assert ll.shape == (len(off) - 1, 3) and bool(torch.isfinite(ll).all())
    ll = ll[s["ks"]].cpu().numpy()
    for j, (a, b) in enumerate(zip(s["off"][:-1], s["off"][1:])):
        want = np.array([G.loglik("poisson", s["Z"][a:b], s["poisson"][a:b], bt, s["w"][a:b],
                                  s["o"][a:b]) for bt in d["betas"]])
        nz = want != 0  # the one-row partition's row may weigh 0
        e = float(np.abs(ll[j][nz] / want[nz] - 1).max(initial=0.0))
        print(f"far rows weighted loglik, small partition {j}: {e:.3e}")
        assert e < 1e-12 and not ll[j][~nz].any()


def test_rows(M, monkeypatch):
    """All five streams and Cook's distances of the small partitions, read at
    their global row indices; the one-row partition's factor is NaN, and so
    are its leverages alone."""
    import torch

    from test_gpu_rows import _check

    d, s = _data(), _small()
    off, small = _layout()
    K = len(off) - 1
    kw = dict(eta_offset=d["o"], sample_weight=d["w"], fit_intercept=True)
    info = M.glm_gram_batched("poisson", d["X"], d["poisson"], off, thetas=d["thetas"],
                              kind="information", **kw)["gram"].cpu().numpy()
    R = M.rows_factor(info, K, P)  # once, for both sides
    nan_parts = np.flatnonzero(np.isnan(R).any(axis=(1, 2)))
    assert nan_parts.tolist() == [small["one row"]]
    monkeypatch.setattr(M, "rows_factor", lambda *a: R)
    g = M.glm_rows_batched("poisson", d["X"], d["poisson"], off, thetas=d["thetas"], info=info, **kw)
    monkeypatch.undo()
    assert all(v.shape == (int(off[-1]),) for v in g.values())
    one = int(off[small["one row"]])
    lev = g["leverage"]
    assert bool(torch.isnan(lev[one])) and int(torch.isnan(lev).sum()) == 1
    idx = torch.from_numpy(s["rows"].copy()).to(lev.device)
    got = {k: v[idx].cpu().numpy() for k, v in g.items()}
    Rs = R[s["ks"]]
    ref, bnd = RR.partitions("poisson", s["Z"], s["poisson"], s["off"], thetas=d["thetas"][s["ks"]],
                             R=Rs, w=s["w"], o=s["o"])
    _check(got, ref, bnd, s["off"], Rs, "far rows")
