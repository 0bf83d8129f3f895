"""The categorical-code layout at its documented limits (not a test module):
the shapes, their data, their numpy yardsticks and a transcription of the LDS
layout the host picks for them.

include/dlsa_hip.h promises F <= 16 factors, levels[f] in 1..256, intercept +
q <= 16 and P <= 192.  The shape table every other test of this layout draws
from (tests/test_gpu_pois_cat.py::SHAPES) stays below 11 factors, 70 levels and
P = 183, and none of its layouts needs a pass of ``cat_layout``'s shrink loop
(dlsa_amd/csrc/fit_plan.hpp).  The ten shapes here, (q, levels, fit_intercept,
standardise, rows_per_chunk) as there, sit on the limits.  ``layout`` is a
line-by-line transcription of ``cat_layout`` / ``cat_lds_bytes`` /
``cat_exact_bucket`` / ``cat_threads_t``; it gives, and
tests/test_cpu_cat_limits.py pins (QN: the numeric column bucket; FM: the
kernel family; thr: threads; fold: the factor that takes the intercept row in
an exact-bucket kernel; shrinks: halvings of the replica caps nd_cap / pr_cap;
nd / pair: the distinct replica counts of the numeric x dummy and the pair
histograms; bytes: the dynamic LDS, of 163 840 - 2 272 for the static tables):

    id   P  QN FM thr fold shrinks nd_cap pr_cap  nd     pair     bytes
    A  192  16 16 256   -     4      16     32    1      1        149 416
    B  192  16 16 256   -     4      16     32    1      1        149 416
    C  177   4 16 512   -     2      64    128    4      1        130 296
    D  177   4 16 512   -     2      64    128    1, 16  1, 2, 8  134 208
    E  180  10 16 256   -     3      32     64    2, 16  1, 2     148 624
    F  184   8  8 512   0     2      64    128    2      1        141 768
    G  192  12  8 256   0     0     256    512    1      -         25 704
    H  192   4  8 512   -     0     256    512    1      -          5 944
    I  192   4  8 512   -     0     256    512    2      1         87 232
    J  192   8 16 256   -     3      32     64    2      1        161 520

A and B: every one of the 16 x 15 / 2 = 120 pair slots of the 16-factor
kernel's table is in use, every histogram unreplicated after four halvings,
intercept + q = 16 with and without an intercept.  C: the 16-factor kernel at
512 threads.  D holds 16-fold replicated 2-level factors (the cap of 16) beside
unreplicated 40-level ones, and pair replicas 8, 2 and 1, in one layout.  E:
F = 13, an odd code-row width, in the 16-factor kernel.  F: the widest
exact-bucket kernel, 8 factors of 23 levels, the fold factor's 23 slots beside
22.  G: ns = 181 level slots (180 dummies and the fold factor's baseline slot)
> 128, so R = 1 under the initial 256-slot cap; codes up to 180.  H: codes up
to 192 without any numeric column or intercept.  I: one 95 x 95 pair block of
9 025 cells, R = 1 under the initial 512-cell cap.  J: the tightest layout of
the even splits of 192 - intercept - q dummy columns over F factors, for every
F, q and intercept inside the limits (the pair cells of a given number of dummy
columns are the most when the levels are equal): nine factors of 13 levels and
seven of 12 beside 7 numeric columns end 48 bytes under the budget.

Data: tests/test_gpu_pois_cat.py::_cat_case with three changes that keep the
*reference* well behaved at these widths --

* two partitions of 12 000-16 000 rows (and the empty one at EMPTY_AT);
* codes of a factor with L >= 64 are uniform (the L u^2 skew would leave the
  top level of 181 about 0.28 % of the rows); the others keep the skew;
* dummy effects 0.4 / sqrt(max(1, F / 3)) N(0, 1): 16 factors give the linear
  predictor the spread that 3 give there.

The row extras (o, ``_glm_ref.weights(n, "real")``), the logistic response
(y >= 2), thetas = 0.3 N(0, 1) and beta = thetas[2] are those of
tests/_cat_gram_ref.py::case; ``betas`` [16, P] = 0.3 N(0, 1) are the
candidates of the evaluation passes.
"""

import functools

import numpy as np

import _glm_ref as G
import oracle as O
from test_gpu_pois_cat import _ref_kw

EMPTY_AT = 1  # the empty partition
N_BETAS = 16  # candidates of one evaluation / goodness-of-fit pass

# (q, levels, fit_intercept, standardise, rows_per_chunk)
SHAPES = {
    "A": (15, (12,) * 16, True, False, 0),
    "B": (16, (12,) * 16, False, False, 0),
    "C": (0, (12,) * 16, True, False, 0),
    "D": (3, (2,) * 8 + (3,) * 4 + (40, 40, 40, 41), True, True, 1500),
    "E": (9, (15,) * 12 + (3,), True, False, 0),
    "F": (7, (23,) * 8, True, False, 0),
    "G": (11, (181,), True, False, 0),
    "H": (0, (193,), False, False, 0),
    "I": (1, (96, 96), True, False, 0),
    "J": (7, (13,) * 9 + (12,) * 7, False, False, 0),
}
IDS = list(SHAPES)

# the limits of include/dlsa_hip.h and the constants of dlsa_amd/csrc
MAX_FACTORS, MAX_LEVELS, Q_MAX, P_MAX = 16, 256, 16, 192
MAX_PAIRS = MAX_FACTORS * (MAX_FACTORS - 1) // 2
LDS_BYTES = 160 * 1024
STATIC_LDS = 16 * (MAX_FACTORS + 1) + 16 * (MAX_PAIRS + 1) + 4 * MAX_FACTORS  # kCatStaticLds

# what ``layout`` gives (the table above): shrinks, nd replicas, pair replicas,
# dynamic LDS bytes
REACHES = {
    "A": (4, {1}, {1}, 149416),
    "B": (4, {1}, {1}, 149416),
    "C": (2, {4}, {1}, 130296),
    "D": (2, {1, 16}, {1, 2, 8}, 134208),
    "E": (3, {2, 16}, {1, 2}, 148624),
    "F": (2, {2}, {1}, 141768),
    "G": (0, {1}, set(), 25704),
    "H": (0, {1}, set(), 5944),
    "I": (0, {2}, {1}, 87232),
    "J": (3, {2}, {1}, 161520),
}


def n_params(shape):
    q, levels, fi, _, _ = shape
    return int(fi) + q + sum(L - 1 for L in levels)


def _qn(Qn):  # cat_qn
    return 4 if Qn <= 4 else 8 if Qn <= 8 else 10 if Qn <= 10 else 12 if Qn <= 12 else 16


def _threads(QN, FM):  # cat_threads_t
    return 512 if QN <= 4 or (QN <= 10 and FM <= 8) else 256


def layout(shape, caps=(256, 512)):
    """``cat_layout`` (fit_plan.hpp) with ``cat_lds_bytes`` and
    ``cat_exact_bucket`` (cat_pass.hip) for one shape: a dict of QN, FM,
    threads, fold (-1: none), shrinks (attempts before the layout fits), nd_cap,
    pr_cap, nd_rep [F], pr_rep [pairs], hist_doubles, lds_bytes (dynamic plus
    static); ``fits`` False when twelve attempts do not fit.  ``caps``: the
    replica caps of the first attempt ((1, 1): the loop's last resort, one
    replica of every histogram)."""
    q, levels, fi, _, _ = shape
    F, ic = len(levels), int(fi)
    QN = _qn(ic + q)
    FM = 8 if F <= 8 else 16
    thr = _threads(QN, FM)
    NR = QN * (QN + 1) // 2 + QN + 1
    NW = thr // 64
    Qw = (q + 1) | 1
    fold = -1
    if ic == 1 and 1 <= F <= 8 and q + 1 == _qn(1 + q):
        for f in range(F):
            if fold < 0 or levels[f] > levels[fold]:
                fold = f
    nd_cap, pr_cap = caps
    out = dict(QN=QN, FM=FM, threads=thr, fold=fold, fits=False)
    for attempt in range(12):
        o, nd_rep, nd_lev, pr_rep = 0, [], [], []
        for f in range(F):
            ns = levels[f] - 1 + (1 if f == fold else 0)
            R = 1
            while R < 16 and ns * R * 2 <= nd_cap:
                R *= 2
            nd_rep.append(R)
            nd_lev.append(ns)
            o += R * ns * Qw
        for f in range(F):
            o += nd_rep[f] * nd_lev[f]
        for f in range(F):
            for g in range(f + 1, F):
                cells = (levels[f] - 1) * (levels[g] - 1)
                R = 1
                while R < 8 and cells * R * 2 <= pr_cap:
                    R *= 2
                pr_rep.append(R)
                o += R * cells
        lds = 8 * (o + P_MAX + 2 * Q_MAX + (NW + 1) * NR) + STATIC_LDS
        out.update(shrinks=attempt, nd_cap=nd_cap, pr_cap=pr_cap, nd_rep=nd_rep, pr_rep=pr_rep,
                   hist_doubles=o, lds_bytes=lds)
        if lds <= LDS_BYTES:
            out["fits"] = True
            return out
        if nd_cap == 1 and pr_cap == 1:
            break
        nd_cap, pr_cap = max(1, nd_cap // 2), max(1, pr_cap // 2)
    return out


def _codes(rs, n, levels):
    cols = [rs.randint(0, L, n) if L >= 64 else
            np.minimum((L * rs.rand(n) ** 2).astype(np.int64), L - 1) for L in levels]
    return np.stack(cols, 1).astype(np.uint8) if levels else np.zeros((n, 0), np.uint8)


@functools.lru_cache(maxsize=None)
def data(sid):
    """(Xn, codes, y, o, offsets, center, scale) of shape ``sid``, once per
    process, read-only: y the Poisson counts, offsets with the empty partition."""
    q, levels, fi, std, rpc = SHAPES[sid]
    rs = np.random.RandomState(100 + IDS.index(sid))
    sizes = [int(s) for s in rs.randint(12000, 16001, size=2)]
    n = sum(sizes)
    Xn = rs.randn(n, q) * 2.0 + 1.0 if std else rs.rand(n, q) - 0.5
    codes = _codes(rs, n, levels)
    F, D = len(levels), sum(L - 1 for L in levels)
    beta = np.concatenate([rs.uniform(-1, 1, q) * (0.5 if std else 1.0),
                           0.4 / np.sqrt(max(1.0, F / 3.0)) * rs.randn(D)])
    Xs = (Xn - 1.0) / 2.0 if std else Xn
    o = rs.uniform(np.log(0.2), np.log(5.0), n)
    y = rs.poisson(np.exp(O.expand_codes(Xs, codes, list(levels)) @ beta + 0.3 + o)).astype(
        np.float64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    off = np.insert(off, EMPTY_AT, off[EMPTY_AT])
    for a in (Xn, codes, y, o, off):
        a.setflags(write=False)
    c = np.full(q, 1.0) if std else None
    s = np.full(q, 2.0) if std else None
    return Xn, codes, y, o, off, c, s


@functools.lru_cache(maxsize=None)
def case(sid):
    """tests/_cat_gram_ref.py::case for shape ``sid``, with ``betas`` [16, P]."""
    shape = SHAPES[sid]
    q, levels, fi, std, rpc = shape
    Xn, codes, ypois, o, off, c, s = data(sid)
    n, K, P = len(ypois), len(off) - 1, n_params(shape)
    ylog = (ypois >= 2.0).astype(np.float64)
    w = G.weights(n, "real")
    rng = np.random.default_rng(2000 + IDS.index(sid))
    thetas = 0.3 * rng.standard_normal((K, P))
    betas = 0.3 * rng.standard_normal((N_BETAS, P))
    kw = _ref_kw(shape)
    Z = G.design(O.expand_codes(Xn, codes, list(levels)), kw["fit_intercept"], kw.get("center"),
                 kw.get("scale"))
    for a in (ylog, w, thetas, betas, Z):
        a.setflags(write=False)
    return dict(Xn=Xn, codes=codes, poisson=ypois, logistic=ylog, o=o, w=w, off=off, center=c,
                scale=s, levels=list(levels), Z=Z, thetas=thetas, beta=thetas[2], betas=betas,
                fi=fi, q=q, rpc=rpc, P=P, K=K, shape=shape, sid=sid)


def extras(d, mask):
    """(o, w) of a mask: the offset and the "real" weights, or None."""
    return (d["o"] if mask in ("ofs", "both") else None,
            d["w"] if mask in ("wgt", "both") else None)


@functools.lru_cache(maxsize=None)
def ref_fit(sid, family, mask):
    """``_glm_ref.fit_partitions`` on the dummy-expanded design, read-only."""
    d = case(sid)
    o, w = extras(d, mask)
    ref = G.fit_partitions(family, O.expand_codes(d["Xn"], d["codes"], d["levels"]), d[family],
                           d["off"], w=w, o=o, **_ref_kw(d["shape"]))
    for v in ref.values():
        v.setflags(write=False)
    return ref
