"""The yardstick of the score outer-product pass on the categorical-code layout
(not a test module).  Per partition, on ``oracle.expand_codes`` and
``_glm_ref.design``:

* ``gram`` -- tests/_gram_ref.py's ``gram_partitions`` on the dummy-expanded
  design, unchanged;
* ``bound`` -- the a-priori bound of the pass's fixed-point histograms
  (dlsa_amd/csrc/cat_gram_impl.hpp).  Each term is rounded once to a grid step
  h = 2^-E, E = floor(60 - log2(B R)), so h <= 2 B R 2^-60 (the factor 2 is the
  grid's floor) and the error of a sum of n_k terms is at most n_k h / 2 <=
  n_k R 2^-60 B; the bound stated here carries the issue's 2 B, n_k R 2^-60 2 B
  per entry class: B = max |d| for the dummy x dummy entries (and the
  intercept's row where it is folded into the histograms), max |d x~_j| for
  dummy x numeric column j, max |s| for the dummy part of the score.  R is the
  most rows of a chunk of the call's plan, at least 1024.  The gram bound is
  relative to the block's largest entry, the score bound to max |Z|^T |s|.

The cases are those of tests/test_gpu_pois_cat.py: its nine SHAPES and its
data, built by its own functions (three partitions of 3000-9000 rows plus an
empty one), with ``_glm_ref.weights(n, "real")``, 0/1 responses for the
logistic family and coefficient vectors of N(0, 0.3^2) entries.
"""

import functools

import numpy as np

import _glm_ref as G
import _gram_ref as R
import oracle as O
from test_gpu_pois_cat import SHAPE_IDS, SHAPES, _data, _ref_kw

FAMILY_MASKS = [("logistic", "none"), ("logistic", "wgt"), ("poisson", "none"),
                ("poisson", "ofs"), ("poisson", "wgt"), ("poisson", "both")]
KINDS = ("score", "information")
TOL = 1e-10  # tests/test_gpu_gram.py's tolerance
BOUND_MAX = 2.5e-11  # the a-priori bound of every GPU case: TOL >= 4 x this


def n_params(shape):
    q, levels, fi, _, _ = shape
    return int(fi) + q + sum(L - 1 for L in levels)


@functools.lru_cache(maxsize=None)
def case(shape):
    """The inputs of one shape, once per process: Xn, codes, the two families'
    y, o, w, offsets, center, scale, levels, the design Z of the yardstick,
    thetas [K, P] and the shared beta [P]."""
    q, levels, fi, std, rpc = shape
    Xn, codes, ypois, o, off, c, s = _data(shape)
    n, K, P = len(ypois), len(off) - 1, n_params(shape)
    ylog = (ypois >= 2.0).astype(np.float64)
    w = G.weights(n, "real")
    rng = np.random.default_rng(1000 + SHAPES.index(shape))
    thetas = 0.3 * rng.standard_normal((K, P))
    kw = _ref_kw(shape)
    Z = G.design(O.expand_codes(Xn, codes, list(levels)), kw["fit_intercept"], kw.get("center"),
                 kw.get("scale"))
    for a in (ylog, w, thetas, Z):
        a.setflags(write=False)
    return dict(Xn=Xn, codes=codes, poisson=ypois, logistic=ylog, o=o, w=w, off=off, center=c,
                scale=s, levels=list(levels), Z=Z, thetas=thetas, beta=thetas[2], fi=fi, q=q,
                rpc=rpc, P=P, K=K)


def extras(d, mask):
    return (d["o"] if mask in ("ofs", "both") else None,
            d["w"] if mask in ("wgt", "both") else None)


def call_kw(d, mask):
    """The keywords of ``glm_gram_batched_categorical`` for one case."""
    o, w = extras(d, mask)
    return dict(eta_offset=o, sample_weight=w, fit_intercept=d["fi"], center=d["center"],
                scale=d["scale"], rows_per_chunk=d["rpc"])


def gram(family, d, mask, kind, own):
    """(gram [K, P, P], score [K, P], score scales [K]) of the yardstick."""
    o, w = extras(d, mask)
    sel = dict(thetas=d["thetas"]) if own else dict(beta=d["beta"])
    return R.gram_partitions(family, d["Z"], d[family], d["off"], w=w, o=o, kind=kind, **sel)


def max_chunk_rows(offsets, rows_per_chunk):
    """R of the grids: the most rows of a chunk of the categorical plan (about
    512 chunks over all partitions, at least 1024 rows each, every partition
    split evenly), at least 1024."""
    sizes = np.diff(np.asarray(offsets, dtype=np.int64))
    K = len(sizes)
    rpc = int(rows_per_chunk)
    if rpc <= 0:
        per = max(1, 512 // max(K, 1))
        rpc = max(1024, min(-(-int(sizes.max(initial=0)) // per), 1 << 24))
    most = 0
    for n in sizes:
        if n > 0:
            nc = -(-int(n) // rpc)
            most = max(most, -(-int(n) // nc))
    return max(1024, most)


def bound(family, Z, y, offsets, thetas, q, fit_intercept, rows_per_chunk, w=None, o=None,
          kind="score", Rmax=None):
    """(gram bound [K], score bound [K]) -- n_k R 2^-60 2 B per entry class, the
    worst class relative to the block's largest entry (the score: to max
    |Z|^T |s|); 0 for an empty partition.  ``thetas`` [K, P] or [P]."""
    K = len(offsets) - 1
    Rm = max_chunk_rows(offsets, rows_per_chunk) if Rmax is None else Rmax
    ic = int(bool(fit_intercept))
    bg, bs = np.zeros(K), np.zeros(K)
    thetas = np.asarray(thetas, dtype=np.float64)
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        if b <= a:
            continue
        th = thetas if thetas.ndim == 1 else thetas[k]
        Zk, yk = Z[a:b], y[a:b]
        om = G._omega(None if w is None else w[a:b], b - a)
        mu, v = G._mu_w(family, Zk, th, om, None if o is None else o[a:b])
        s = om * (yk - mu)
        d = s * s if kind == "score" else v
        Gk = Zk.T @ (Zk * d[:, None])
        B = [np.abs(d).max()] + [np.abs(d * Zk[:, ic + j]).max() for j in range(q)]
        unit = (b - a) * Rm * 2.0 ** -60 * 2.0
        bg[k] = unit * max(B) / np.abs(Gk).max()
        scale = float((np.abs(Zk).T @ np.abs(s)).max())
        bs[k] = unit * np.abs(s).max() / scale if scale > 0 else 0.0
    return bg, bs
