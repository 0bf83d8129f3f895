"""The limit shapes of the categorical-code layout (tests/_cat_limits.py):
conditions on the inputs of tests/test_gpu_cat_limits.py, checked in numpy.

* the shape table reaches the limits of include/dlsa_hip.h -- F = 16, P = 192,
  q = 16, a code >= 128 that occurs in the data -- and stays inside them;
* the transcription of ``cat_layout`` reaches the shrink depths, replica counts
  and LDS sizes the module's table records, and every layout fits;
* the data can carry the project's tolerances: every dummy column has >= 30
  rows with a positive weight in every partition, both logistic outcomes occur
  in every level, the numpy fit of either family converges without a halved
  step (but the first one of a Poisson fit without an intercept, which starts
  at theta = 0), and the a-priori bound of the Gram pass's fixed-point
  histograms is at most ``_cat_gram_ref.BOUND_MAX`` in both kinds.
"""

import numpy as np
import pytest

import _cat_gram_ref as CR
import _cat_limits as L
import _glm_ref as G
import oracle as O
from test_gpu_pois_cat import _ref_kw

FITS = CR.FAMILY_MASKS  # every fit tests/test_gpu_cat_limits.py compares with


def test_the_table_reaches_the_documented_limits():
    shapes = list(L.SHAPES.values())
    assert max(len(s[1]) for s in shapes) == L.MAX_FACTORS == 16
    assert max(L.n_params(s) for s in shapes) == L.P_MAX == 192
    assert max(s[0] for s in shapes) == L.Q_MAX == 16
    assert max(int(s[2]) + s[0] for s in shapes) == L.Q_MAX
    for sid, s in L.SHAPES.items():
        q, levels, fi, _, rpc = s
        assert len(levels) <= L.MAX_FACTORS and int(fi) + q <= L.Q_MAX and rpc >= 0, sid
        assert all(1 <= v <= L.MAX_LEVELS for v in levels), sid
        assert L.n_params(s) <= L.P_MAX, sid
    # q = 16 only without an intercept; F = 16 with P = 192 in one shape
    assert any(s[0] == 16 and not s[2] for s in shapes)
    assert any(len(s[1]) == 16 and L.n_params(s) == 192 for s in shapes)
    # codes >= 128 that the data holds: the top code of G and of H
    for sid in ("G", "H"):
        codes = L.data(sid)[1]
        top = L.SHAPES[sid][1][0] - 1
        assert top >= 128 and int(codes.max()) == top, (sid, int(codes.max()))


@pytest.mark.parametrize("sid", L.IDS)
def test_layout_transcription_reaches_what_the_table_says(sid):
    r = L.layout(L.SHAPES[sid])
    shrinks, nd, pr, dyn = L.REACHES[sid]
    assert r["fits"], sid
    got = (r["shrinks"], set(r["nd_rep"]), set(r["pr_rep"]), r["lds_bytes"] - L.STATIC_LDS)
    assert got == (shrinks, nd, pr, dyn), got
    assert r["lds_bytes"] <= L.LDS_BYTES
    assert (r["nd_cap"], r["pr_cap"]) == (256 >> shrinks, 512 >> shrinks)
    F = len(L.SHAPES[sid][1])
    assert len(r["pr_rep"]) == F * (F - 1) // 2


def test_the_loop_the_full_pair_table_and_both_kernel_families_are_reached():
    lay = {sid: L.layout(s) for sid, s in L.SHAPES.items()}
    assert {r["shrinks"] for r in lay.values()} >= {0, 2, 3, 4}
    assert len(lay["A"]["pr_rep"]) == L.MAX_PAIRS == 120
    assert {r["FM"] for r in lay.values()} == {8, 16}
    assert {r["QN"] for r in lay.values()} == {4, 8, 10, 12, 16}
    assert {r["threads"] for r in lay.values()} == {256, 512}
    assert lay["F"]["fold"] == 0 and lay["G"]["fold"] == 0  # the exact-bucket kernels
    assert all(lay[s]["fold"] < 0 for s in "ABCDEHIJ")
    assert max(lay["D"]["nd_rep"]) == 16 and min(lay["D"]["nd_rep"]) == 1


def test_no_shape_inside_the_limits_overflows_the_lds():
    """include/dlsa_hip.h says so.  The shrink loop ends, at the latest, with
    one replica of every histogram: D (Qw + 1) doubles plus one per pair cell,
    D the dummy columns.  The pair cells, (D^2 - sum nl_f^2) / 2, are the most
    when the levels are equal, so the even splits of D = 192 - intercept - q
    over F factors are the largest layouts of every (F, q, intercept): at most
    153 240 bytes, and A and B the largest with intercept + q = 16.  Shape J is
    the tightest of the layouts the loop picks for those splits."""
    most, most_r1, most_r1_q16 = 0, 0, 0
    for F in range(1, L.MAX_FACTORS + 1):
        for ic in (0, 1):
            for q in range(0, L.Q_MAX - ic + 1):
                D = L.P_MAX - ic - q
                if D > F * (L.MAX_LEVELS - 1):
                    continue
                levels = tuple(1 + D // F + (1 if f < D % F else 0) for f in range(F))
                shape = (q, levels, bool(ic), False, 0)
                r, r1 = L.layout(shape), L.layout(shape, caps=(1, 1))
                assert r["fits"] and r1["fits"] and r1["shrinks"] == 0, (F, q, ic)
                assert r["lds_bytes"] >= r1["lds_bytes"]
                most, most_r1 = max(most, r["lds_bytes"]), max(most_r1, r1["lds_bytes"])
                if q + ic == L.Q_MAX:
                    most_r1_q16 = max(most_r1_q16, r1["lds_bytes"])
    assert most == L.REACHES["J"][3] + L.STATIC_LDS == L.LDS_BYTES - 48
    assert most_r1 == 153240
    assert most_r1_q16 == L.REACHES["A"][3] + L.STATIC_LDS


@pytest.mark.parametrize("sid", L.IDS)
def test_every_level_is_populated(sid):
    d = L.case(sid)
    off, codes, w, ylog = d["off"], d["codes"], d["w"], d["logistic"]
    assert len(off) == 4 and off[L.EMPTY_AT] == off[L.EMPTY_AT + 1]
    least = None
    for a, b in zip(off[:-1], off[1:]):
        if b == a:
            continue
        assert 12000 <= b - a <= 16000
        for f, nl in enumerate(d["levels"]):
            c = codes[a:b, f]
            assert int(c.max()) == nl - 1
            pos = np.bincount(c[w[a:b] > 0], minlength=nl)
            ones = np.bincount(c, weights=ylog[a:b], minlength=nl)
            tot = np.bincount(c, minlength=nl)
            least = int(pos.min()) if least is None else min(least, int(pos.min()))
            assert pos.min() >= 30, (sid, f, int(pos.min()))
            assert (ones >= 1).all() and (tot - ones >= 1).all(), (sid, f)
    print(f"{sid}: the smallest level holds {least} rows with a positive weight")


@pytest.mark.parametrize("family,mask", FITS, ids=[f"{f}-{m}" for f, m in FITS])
@pytest.mark.parametrize("sid", L.IDS)
def test_the_reference_fit_converges(sid, family, mask):
    ref = L.ref_fit(sid, family, mask)
    live = [k for k in range(3) if k != L.EMPTY_AT]
    print(f"{sid} {family}-{mask}: iters {ref['iters'][live].tolist()} max|theta| "
          f"{np.abs(ref['theta']).max():.2f} cond "
          f"{max(np.linalg.cond(ref['sig_inv'][k]) for k in live):.1e}")
    halvings = ref["halvings"].copy()
    d = L.case(sid)
    if family == "poisson" and not d["fi"]:
        # Without an intercept the documented start of a Poisson fit is theta =
        # 0, mu = exp(o), a factor e^0.3 E e^(x beta) below the counts, more in
        # the levels with a large effect; a full Newton step from there moves a
        # level's coefficient by (mean y / mean mu) - 1 where log(mean y / mean
        # mu) is wanted and overshoots for any seed of this recipe (shapes B and
        # H).  That first step may be halved once; no step behind it.
        o, w = L.extras(d, mask)
        X = O.expand_codes(d["Xn"], d["codes"], d["levels"])
        for k in live:
            a, b = d["off"][k], d["off"][k + 1]
            first = G.fit(family, X[a:b], d[family][a:b], None if w is None else w[a:b],
                            None if o is None else o[a:b], max_iter=1,
                            **_ref_kw(d["shape"]))["halvings"]
            assert first <= 1, (sid, k, first)
            halvings[k] -= first
    assert halvings.max() == 0, ref["halvings"]
    # (quadratic convergence from a start within e of the optimum: the 200
    # iterations the reference allows are never approached)
    assert 1 <= ref["iters"][live].min() and ref["iters"].max() <= 12, ref["iters"]
    for v in ref.values():
        assert np.isfinite(v).all()
    assert not ref["theta"][L.EMPTY_AT].any()


@pytest.mark.parametrize("sid", L.IDS)
def test_gram_bound(sid):
    d = L.case(sid)
    worst = 0.0
    for family, mask in CR.FAMILY_MASKS:
        o, w = L.extras(d, mask)
        for kind in CR.KINDS:
            for th in (d["thetas"], d["beta"]):
                bg, bs = CR.bound(family, d["Z"], d[family], d["off"], th, d["q"], d["fi"],
                                  d["rpc"], w=w, o=o, kind=kind)
                worst = max(worst, float(bg.max()), float(bs.max()))
                assert bg.max() <= CR.BOUND_MAX and bs.max() <= CR.BOUND_MAX, \
                    (sid, family, mask, kind, bg, bs)
    print(f"{sid}: the largest a-priori bound {worst:.2e}")
