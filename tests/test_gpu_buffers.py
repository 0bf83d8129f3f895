"""GPU: what every C-ABI entry point does to memory it must not depend on and
must not touch (tests/_poison.py; the region table of DESIGN.md 3.1 is the map
these tests check).

Fits.  Every case of ``_poison.FIT_CASES`` makes the same call through the C
ABI with the inputs, the outputs and a workspace of exactly the reported size
inside a 0xFF-filled arena (4 KiB guards around every region, X at an address
that is 8 modulo 16):

  A  workspace and outputs zero-filled       -> the case's existing yardstick
  B  workspace and outputs 0xFF-filled       -> every output array bit-equal to A
  C  workspace = what another fit left       -> bit-equal to A
     behind, outputs 0xFF
  N  a NULL workspace, outputs 0xFF          -> bit-equal to A

The stale image of run C is the final workspace of a fit of the other family
(``_poison.STALE_POISSON`` / ``STALE_LOGISTIC``, run once per module): more
partitions, a larger P and more chunks than the fused cases, max_iter = 2, a
NaN partition, an empty one, an all-zero-y Poisson partition and a halved
step.  It is copied into the case's workspace (repeated to length for the
wide workspaces, which are larger), so every case meets the same image.

Run A is compared with the yardstick of the test the case was taken from
(``oracle.logistic_fit``, ``oracle.ols_fit``, ``_glm_ref.fit``) at the suite's
tolerances: theta, Sig_inv and
Sig_inv theta within 1e-8 of the largest entry, the log-likelihood within
1e-10 (the OLS rss within 1e-6, test_ols_vs_oracle: it is a difference of
two sums).  That is the only numerical tolerance here; everything else is
bitwise: the project asserts bit-identical repeats on these paths
(test_determinism, test_reduce_partitions_and_determinism,
test_categorical_bit_identical_runs_and_column_ranges,
test_ozaki_bit_identical_runs), so a run that differs from A read something
the call did not write.  After B, C and N every guard byte and every input
is unchanged, every output element is written, and the partitions that end
EMPTY, SINGULAR or NONFINITE have all-zero outputs and iters == 0.  The
regions a case claims to reach are asserted from dlsa_last_fit_stats.

The one defect these tests found is pinned by cases of its own: with X ending
8 bytes short of a 16-byte boundary the fused passes fetch one double past X,
gave it the weight 0 and multiplied -- 0 * NaN -- so the last partition ended
NONFINITE in every run, the clean one included (every Poisson case, ols-P129,
fused-warm-start-level, fused-stalled-escalation: the cases whose last
partition is a good one).  The same lanes read the first row of the next
partition behind every partition's last chunk: the ``*-nan-behind-*`` cases put
a NaN there and require that it fails its own partition only.

What a caller cannot poison -- a NULL workspace, the Poisson side allocation,
the scratch of the evaluation passes, dlsa_partition_rows and
dlsa_column_moments, and the categorical fit's own buffer when the caller's
is too small -- is covered by run N (and the too-small categorical cases)
only through the results; beyond that by the audit table alone.
"""

import ctypes

import numpy as np
import pytest

import _poison as P
import oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-8       # theta, Sig_inv, Sig_inv theta: relative to the largest entry
REL_LL = 1e-10   # log-likelihoods
REL_RSS = 1e-6   # OLS residual sum of squares (test_gpu_parity.test_ols_vs_oracle)
EVAL_SIZES = (5000, 3001, 0, 777, 1)
INT_STATS = ("iterations", "passes_fp32", "passes_fp64", "n_chunks", "rows_fp32", "rows_fp64",
             "passes_f32x", "polish_partitions", "passes_oz", "oz_fallbacks",
             "oz_stale_partitions")


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class Env:
    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
        from dlsa_amd import _hip
        self.torch, self.hip, self.lib = torch, _hip, _hip.load()
        self.device = torch.device("cuda")

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def done(self, rc, what):
        """Wait for the call and raise on its error.  A poisoned index or phase
        word could send a kernel out of range: after a device fault nothing more
        is launched -- the session ends there."""
        try:
            self.torch.cuda.synchronize()
            self.hip.check(rc, what)
        except Exception as e:
            if any(s in str(e) for s in ("illegal memory access", "hipErrorLaunchFailure",
                                         "unspecified launch failure", "HSA_STATUS_ERROR")):
                pytest.exit(f"GPU fault in {what}: {e}", returncode=3)
            raise


@pytest.fixture(scope="module")
def env():
    return Env()


def _run_fit(env, case, A, ws_bytes, ws_fill, out_fill, null_ws=False):
    """One call on the arena: the workspace filled with a byte or an image,
    the outputs with a byte.  Returns (outputs, integer stats)."""
    if isinstance(ws_fill, int):
        A.fill("ws", ws_fill)
    else:
        A.put_bytes("ws", ws_fill)
    for name in P.out_names(case):
        A.fill(name, out_fill)
    before = A.snapshot("ws") if (null_ws or case.small_ws) else None
    rc = P.fit_call(env.lib, env.hip, case, A, ws_bytes, env.stream, null_ws=null_ws)
    env.done(rc, f"{case.id}: {case.entry} fit")
    stats = env.hip.last_fit_stats()
    A.guards_intact()
    A.inputs_unchanged()
    if before is not None:  # the call had to allocate its own scratch
        assert A.same_as("ws", before), "a workspace the call must not use was written"
    return P.read_outputs(case, A), {k: stats[k] for k in INT_STATS}


@pytest.fixture(scope="module")
def stale(env):
    """The final workspaces of the two stale fits, as host bytes."""
    images = {}
    for sc in (P.STALE_POISSON, P.STALE_LOGISTIC):
        data = P.problem(sc)
        need = P.workspace_bytes(env.lib, sc)
        A = P.fit_arena(sc, data, need, env.device)
        out, stats = _run_fit(env, sc, A, need, P.POISON, P.POISON)
        st = out["status"].tolist()
        want = data["status"].tolist()
        for k, s in enumerate(want):
            # max_iter = 2 leaves the good partitions MAXITER (a Poisson one whose
            # halved step still overflows exp is polished at a non-finite point)
            ok = (s,) if s != P.STATUS_OK else (P.STATUS_MAXITER, P.STATUS_NONFINITE)
            assert st[k] in ok, (sc.id, st)
        assert {P.STATUS_MAXITER, P.STATUS_EMPTY, P.STATUS_NONFINITE} <= set(st)
        assert stats["polish_partitions"] >= 3 and stats["iterations"] == 2, stats
        images[sc.id] = A.raw("ws")
        assert (images[sc.id] != P.POISON).any()
    assert P.STATUS_SINGULAR in P.problem(P.STALE_POISSON)["status"]
    return images


def _check_yardstick(case, data, out):
    assert out["status"].tolist() == data["status"].tolist(), (out["status"], data["status"])
    assert data["ref"], "a case without a good partition checks nothing"
    for k, r in data["ref"].items():
        e = {n: _rel(out[n][k], r[n]) for n in ("theta", "sig_inv", "sig_inv_theta")}
        e["loglik"] = abs(out["loglik"][k] - r["loglik"]) / abs(r["loglik"])
        print(f"{case.id} k={k} " + " ".join(f"{n} {v:.2e}" for n, v in e.items()))
        for n in case.check:
            bound = REL if n != "loglik" else (REL_RSS if case.entry == "ols" else REL_LL)
            assert e[n] < bound, (k, n, e[n])


@pytest.mark.parametrize("case", P.FIT_CASES, ids=P.FIT_CASE_IDS)
def test_fit_buffers(env, stale, case):
    data = P.problem(case)
    need = P.workspace_bytes(env.lib, case)
    assert need > 0
    ws_bytes = need - 1 if case.small_ws else need
    A = P.fit_arena(case, data, ws_bytes, env.device)
    image = stale[P.stale_case_for(case).id]
    n_total = int(case.offsets[-1])

    out_a, st_a = _run_fit(env, case, A, ws_bytes, 0x00, 0x00)
    print(case.id, st_a)
    _check_yardstick(case, data, out_a)
    P.check_expect(case, st_a, n_total)
    P.check_zero_blocks(out_a, data["status"])
    if case.entry == "cat" and not case.small_ws:
        # the size worked out in _poison.workspace_bytes holds the call: it was used
        assert A.raw("ws").any(), "the categorical fit did not use the caller's workspace"

    for tag, ws_fill, null_ws in (("B", P.POISON, False), ("C", image, False),
                                  ("N", P.POISON, True)):
        out, st = _run_fit(env, case, A, ws_bytes, ws_fill, P.POISON, null_ws=null_ws)
        for name in P.out_names(case):
            A.fully_written(name, P.OUT_DTYPES[name])
            assert P.bits_equal(out[name], out_a[name]), \
                f"run {tag}: '{name}' differs from the clean run (max |diff| " \
                f"{np.nanmax(np.abs(out[name].astype(np.float64) - out_a[name])):.3e})"
        P.check_zero_blocks(out, data["status"])
        assert st == st_a, (tag, st, st_a)


def test_wide_skewed_levels_buffers(env, stale):
    """``_poison.SKEW_CASE``: a warm-start level with more Gram row groups (347)
    than the all-rows plan (346), whose tables and slabs must fit the regions
    make_wide_layout sized over every level.  X (1.2 GB, at 8 modulo 16) and y
    are generated in the arena by dlsa_simulate_logistic.  Yardstick of
    test_gpu_scale.test_wide_skewed_partitions_level_plans: two small
    partitions (the last one among them) against the oracle, the big one
    through the score equation; runs B, C and N as in test_fit_buffers."""
    torch = env.torch
    case = P.SKEW_CASE
    K, p, off = case.K, case.p, case.offsets
    n = int(off[-1])
    need = P.workspace_bytes(env.lib, case)
    A = P.Arena(env.device)
    A.add("X", n * p * 8, 16, 8).add("y", n * 8)
    for name in P.out_names(case):
        cnt = {"theta": K * p, "sig_inv": K * p * p, "sig_inv_theta": K * p}.get(name, K)
        A.add(name, cnt * np.dtype(P.OUT_DTYPES[name]).itemsize)
    A.add("ws", need).build()
    rc = env.lib.dlsa_simulate_logistic(A.ptr("X"), A.ptr("y"), n, p, case.seed, 0, env.stream)
    env.done(rc, "dlsa_simulate_logistic")
    A.guards_intact()
    x_in, y_in = A.snapshot("X"), A.snapshot("y")

    def run(ws_fill, out_fill, null_ws=False):
        out, st = _run_fit(env, case, A, need, ws_fill, out_fill, null_ws=null_ws)
        assert A.same_as("X", x_in) and A.same_as("y", y_in), "an input was written to"
        return out, st

    out_a, st_a = run(0x00, 0x00)
    print(case.id, st_a)
    assert st_a["n_chunks"] == 346, st_a  # Gram row groups of the all-rows plan
    P.check_expect(case, st_a, n)
    assert out_a["status"].tolist() == [0] * K
    # X is misaligned for torch views: work on copies of the partitions used
    Xb = A.buf[A.regions["X"][0]:][:n * p * 8].clone().view(torch.float64).view(n, p)
    yb = A.tensor("y", torch.float64, (n,))
    th0 = torch.from_numpy(out_a["theta"][0]).to(env.device)
    a, b = int(off[0]), int(off[1])
    g = Xb[a:b].T @ (yb[a:b] - torch.sigmoid(Xb[a:b] @ th0))
    assert g.abs().max().item() < 1e-5
    for k in (1, K - 1):
        a, b = int(off[k]), int(off[k + 1])
        o = O.logistic_fit(Xb[a:b].cpu().numpy(), yb[a:b].cpu().numpy())
        assert _rel(out_a["theta"][k], o["coef"]) < REL
        assert _rel(out_a["sig_inv"][k], o["Sig_inv"]) < REL
    del Xb
    for tag, ws_fill, null_ws in (("B", P.POISON, False), ("C", stale["stale-poisson"], False),
                                  ("N", P.POISON, True)):
        out, st = run(ws_fill, P.POISON, null_ws=null_ws)
        for name in P.out_names(case):
            A.fully_written(name, P.OUT_DTYPES[name])
            assert P.bits_equal(out[name], out_a[name]), f"run {tag}: '{name}' differs"
        assert st == st_a, (tag, st, st_a)


# ---------------------------------------------------------------------------
# evaluation passes
# ---------------------------------------------------------------------------

def _eval_problem(kind, B):
    """Data, candidates and the oracle's [K, B] log-likelihoods; the loops of
    test_gpu_eval.py (categorical), test_gpu_poisson.py and
    test_gpu_poisson_offset.py (test_evaluation), oracle.logistic_loglik."""
    import _glm_ref as G

    off = np.concatenate([[0], np.cumsum(EVAL_SIZES)]).astype(np.int64)
    n = int(off[-1])
    parts = list(zip(off[:-1], off[1:]))
    d = dict(off=off, codes=None, eta_offset=None, row_weight=None, levels=(), fi=True)
    if kind == "cat":
        rs = np.random.RandomState(3070 + B)
        q, levels = 3, (7, 4)
        X = rs.randn(n, q) * 2.0 + 1.0
        codes = np.stack([rs.randint(0, L, n) for L in levels], 1).astype(np.uint8)
        for f, L in enumerate(levels):
            codes[f, f] = L - 1
        y = (rs.rand(n) < 0.4).astype(np.float64)
        D = sum(L - 1 for L in levels)
        c, s = rs.randn(q) * 0.5 + 1.0, rs.rand(q) + 1.5
        betas = rs.randn(B, 1 + q + D) * 0.4
        Xd = O.expand_codes(X, codes, levels)
        kw = dict(center=np.concatenate([c, np.zeros(D)]), scale=np.concatenate([s, np.ones(D)]))
        ref = np.array([O.logistic_loglik(Xd[a:b], y[a:b], betas, fit_intercept=True, **kw)
                        for a, b in parts])
        d.update(codes=codes, levels=levels)
    else:
        p = 37
        rng = np.random.default_rng(B)
        betas = 0.2 * rng.standard_normal((B, p + 1))
        if kind.startswith("logistic"):
            X, y = O.simulate_counter(n, p, seed=9)
        else:
            X, y = G.simulate(n, p, seed=9, fit_intercept=True)
        X = np.ascontiguousarray(X)
        c, s = X.mean(0), X.std(0, ddof=1)
        Z = G.design(X, True, c, s)
        if kind.endswith("weighted_nan_behind"):
            # a NaN weight in the first row of partition 1: the last block of
            # partition 0 (5000 rows: 8 of a 32-row block) reads it as a padded row
            fam = kind.split("_")[0]
            w = G.weights(n, "real").copy()
            o = P._eta_offset(n, p) if fam == "poisson" else None
            ref = np.array([[G.loglik(fam, Z[a:b], y[a:b], bt, w[a:b],
                                      None if o is None else o[a:b]) for bt in betas]
                            for a, b in parts])
            w[off[1]] = np.nan
            d.update(eta_offset=o, row_weight=w)
        elif kind.startswith("logistic"):
            ref = np.array([O.logistic_loglik(Z[a:b], y[a:b], betas) for a, b in parts])
        elif kind == "poisson":
            ref = np.array([[G.loglik("poisson", Z[a:b], y[a:b], bt) for bt in betas]
                            for a, b in parts])
        else:
            o = P._eta_offset(n, p)
            ref = np.array([[G.loglik("poisson", Z[a:b], y[a:b], bt, o=o[a:b]) for bt in betas]
                            for a, b in parts])
            if kind == "poisson_offset_nan_behind":  # the same row, a NaN offset
                o = o.copy()
                o[off[1]] = np.nan
            d["eta_offset"] = o
    d.update(X=X, y=np.ascontiguousarray(y, dtype=np.float64), center=c, scale=s,
             betas=np.ascontiguousarray(betas), ref=ref, p=X.shape[1])
    return d


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("kind", ["logistic", "logistic_sum", "poisson", "poisson_offset", "cat",
                                  "poisson_offset_nan_behind", "logistic_weighted_nan_behind",
                                  "poisson_weighted_nan_behind"])
def test_eval_buffers(env, kind, B):
    """[K, B] and [B] outputs poisoned, candidates in groups of at most 16 (the
    ABI's limit, as the Python layer calls it), an empty partition whose row is
    exactly 0, a one-row partition at the buffers' end.  The ``*_nan_behind``
    kinds put a NaN offset / prior weight directly behind partition 0's last
    row: partition 1 is NaN, every other partition is the yardstick's."""
    nan_part = 1 if kind.endswith("nan_behind") else -1
    d = _eval_problem(kind, B)
    K, off = len(EVAL_SIZES), d["off"]
    offp = off.ctypes.data_as(ctypes.c_void_p)
    has_sum = kind != "logistic"
    groups = [(g0, min(16, B - g0)) for g0 in range(0, B, 16)]
    A = P.Arena(env.device)
    A.add("X", d["X"].nbytes, 16, 8).add("y", d["y"].nbytes)
    A.add("center", d["center"].nbytes).add("scale", d["scale"].nbytes)
    for name in ("codes", "eta_offset", "row_weight"):
        if d[name] is not None:
            A.add(name, d[name].nbytes)
    for g0, nb in groups:
        A.add(f"betas{g0}", nb * d["betas"].shape[1] * 8)
        A.add(f"ll{g0}", K * nb * 8)
        if has_sum:
            A.add(f"tot{g0}", nb * 8)
    A.build()
    for name in ("X", "y", "center", "scale", "codes", "eta_offset", "row_weight"):
        if d[name] is not None:
            A.put(name, d[name])
    got = np.empty((K, B))
    tot = np.empty(B)
    for g0, nb in groups:
        A.put(f"betas{g0}", d["betas"][g0:g0 + nb])
        common = (offp, K, d["p"], 1, A.ptr("center"), A.ptr("scale"), A.ptr(f"betas{g0}"), nb)
        ll, ts = A.ptr(f"ll{g0}"), (A.ptr(f"tot{g0}") if has_sum else None)
        if kind == "logistic":
            rc = env.lib.dlsa_logistic_loglik_batched(A.ptr("X"), A.ptr("y"), *common, ll,
                                                      env.stream)
        elif kind == "logistic_sum":
            rc = env.lib.dlsa_logistic_loglik_batched_sum(A.ptr("X"), A.ptr("y"), *common, ll, ts,
                                                          env.stream)
        elif kind == "poisson":
            rc = env.lib.dlsa_poisson_loglik_batched_sum(A.ptr("X"), A.ptr("y"), *common, ll, ts,
                                                         env.stream)
        elif kind.startswith("poisson_offset"):
            rc = env.lib.dlsa_poisson_loglik_batched_sum_offset(
                A.ptr("X"), A.ptr("y"), A.ptr("eta_offset"), *common, ll, ts, env.stream)
        elif kind == "logistic_weighted_nan_behind":
            rc = env.lib.dlsa_logistic_loglik_batched_sum_weighted(
                A.ptr("X"), A.ptr("y"), A.ptr("row_weight"), *common, ll, ts, env.stream)
        elif kind == "poisson_weighted_nan_behind":
            rc = env.lib.dlsa_poisson_loglik_batched_sum_weighted(
                A.ptr("X"), A.ptr("y"), A.ptr("eta_offset"), A.ptr("row_weight"), *common, ll, ts,
                env.stream)
        else:
            levels = np.asarray(d["levels"], dtype=np.int32)
            rc = env.lib.dlsa_logistic_loglik_categorical(
                A.ptr("X"), A.ptr("codes"), A.ptr("y"), offp, K, d["p"], len(levels),
                levels.ctypes.data_as(ctypes.c_void_p), 1, A.ptr("center"), A.ptr("scale"),
                A.ptr(f"betas{g0}"), nb, 1500, ll, ts, env.stream)
        env.done(rc, kind)
        A.guards_intact()
        A.inputs_unchanged()
        A.fully_written(f"ll{g0}", np.float64)
        got[:, g0:g0 + nb] = A.get(f"ll{g0}", np.float64, (K, nb))
        if has_sum:
            A.fully_written(f"tot{g0}", np.float64)
            tot[g0:g0 + nb] = A.get(f"tot{g0}", np.float64)
    ref = d["ref"]
    assert not got[2].view(np.uint64).any(), "the empty partition's row is not exactly 0"
    for k in range(K):
        if k == nan_part:
            assert np.isnan(got[k]).all(), "the partition that holds the NaN"
            continue
        err, bound = np.abs(got[k] - ref[k]).max(), REL_LL * np.abs(ref[k]).max()
        print(f"{kind} B={B} partition {k}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, k
    if has_sum and nan_part >= 0:
        assert np.isnan(tot).all()
    elif has_sum:
        rs = ref.sum(0)
        assert np.abs(tot - rs).max() <= REL_LL * np.abs(rs).max()
        acc = np.zeros(B)
        for k in range(K):  # k ascending, as the header states
            acc = acc + got[k]
        assert P.bits_equal(tot, acc)


# ---------------------------------------------------------------------------
# the short entry points
# ---------------------------------------------------------------------------

def test_reduce_partitions_buffers(env):
    """K = 4 with one failed partition (its zero block), the output poisoned:
    sums in partition order, exactly (test_reduce_partitions_and_determinism)."""
    K, p = 4, 20
    rs = np.random.RandomState(4)
    S, v, th = rs.randn(K, p, p), rs.randn(K, p), rs.randn(K, p)
    S[2], v[2], th[2] = 0.0, 0.0, 0.0
    n_out = p * p + 2 * p + 1
    A = P.Arena(env.device)
    A.add("S", S.nbytes).add("v", v.nbytes).add("th", th.nbytes).add("out", n_out * 8).build()
    A.put("S", S)
    A.put("v", v)
    A.put("th", th)
    rc = env.lib.dlsa_reduce_partitions(A.ptr("S"), A.ptr("v"), A.ptr("th"), K, p, A.ptr("out"),
                                        env.stream)
    env.done(rc, "dlsa_reduce_partitions")
    A.guards_intact()
    A.inputs_unchanged()
    A.fully_written("out", np.float64)
    out = A.get("out", np.float64)
    want = np.concatenate([x.reshape(K, -1) for x in (S, v, th)], axis=1)
    acc = np.zeros(want.shape[1])
    for k in range(K):
        acc = acc + want[k]
    assert np.array_equal(out[:-1], acc) and out[-1] == K


@pytest.mark.parametrize("phase16", [0, 8], ids=["aligned", "rows16-at-8-mod-16"])
def test_partition_rows_buffers(env, phase16):
    """n = 20001, K = 37, rows of 16, 12, 56 and 3 bytes (the 16-, 4-, 8- and
    1-byte copy paths of part_scatter_kernel; with the 16-byte rows at an
    address that is only 8-aligned they take the 8-byte path).  Sources,
    destinations and `order` sit in a device arena, the host offsets in a host
    arena; compared with numpy's stable argsort like test_repartition_bit_exact."""
    n, K = 20001, 37
    rs = np.random.RandomState(n % 1000 + K)
    pid = rs.randint(0, K, size=n).astype(np.int32)
    arrays = [rs.randn(n, 2), rs.randn(n, 3).astype(np.float32), rs.randn(n, 7),
              rs.randint(0, 256, size=(n, 3)).astype(np.uint8)]
    widths = [16, 12, 56, 3]
    aligns = [(16, phase16), (4, 0), (8, 0), (1, 0)]
    A = P.Arena(env.device)
    A.add("pid", pid.nbytes)
    for i, (a, (al, ph)) in enumerate(zip(arrays, aligns)):
        assert a.nbytes == n * widths[i]
        A.add(f"src{i}", a.nbytes, al, ph)
    for i, (a, (al, ph)) in enumerate(zip(arrays, aligns)):
        A.add(f"dst{i}", a.nbytes, al, ph)
    A.add("order", n * 8).build()
    A.put("pid", pid)
    for i, a in enumerate(arrays):
        A.put(f"src{i}", a)
    H = P.Arena().add("offsets", (K + 1) * 8, 8).build()
    src = (ctypes.c_void_p * 4)(*[A.ptr(f"src{i}") for i in range(4)])
    dst = (ctypes.c_void_p * 4)(*[A.ptr(f"dst{i}") for i in range(4)])
    rb = (ctypes.c_int64 * 4)(*widths)
    rc = env.lib.dlsa_partition_rows(A.ptr("pid"), n, K, 4, src, dst, rb, H.ptr("offsets"),
                                     A.ptr("order"), env.stream)
    env.done(rc, "dlsa_partition_rows")
    A.guards_intact()
    A.inputs_unchanged()
    H.guards_intact()
    H.fully_written("offsets", np.int64)
    A.fully_written("order", np.int64)
    perm = np.argsort(pid, kind="stable")
    assert np.array_equal(A.get("order", np.int64), perm)
    assert np.array_equal(H.get("offsets", np.int64),
                          np.concatenate([[0], np.cumsum(np.bincount(pid, minlength=K))]))
    for i, a in enumerate(arrays):
        assert P.bits_equal(A.get(f"dst{i}", a.dtype, a.shape), a[perm]), i


@pytest.mark.parametrize("n,p", [(10007, 130), (1, 3), (0, 2)])
def test_column_moments_buffers(env, n, p):
    """The [5, p] output poisoned, X at 8 modulo 16; compared as in
    test_column_moments_vs_oracle.  n = 0 returns NaN by contract (a column
    without values), so it gets the guard check and the counts only."""
    rs = np.random.RandomState(n + p)
    X = rs.randn(n, p) * np.linspace(1e-3, 1e3, p) + np.linspace(-5.0, 5.0, p)
    if n > 10:
        X[rs.choice(n, 9), rs.choice(p, 9)] = np.nan
        X[:, 1] = 4.25
    A = P.Arena(env.device)
    A.add("X", X.nbytes, 16, 8).add("out", 5 * p * 8).build()
    A.put("X", X)
    rc = env.lib.dlsa_column_moments(A.ptr("X") if n else None, n, p, A.ptr("out"), env.stream)
    env.done(rc, "dlsa_column_moments")
    A.guards_intact()
    A.inputs_unchanged()
    got = A.get("out", np.float64, (5, p))
    ref = O.column_moments(X)
    assert np.array_equal(got[0], ref[0])
    if n == 0:
        return
    A.fully_written("out", np.float64)
    assert np.array_equal(got[3:], ref[3:])
    scale = np.nanmax(np.abs(X), axis=0)
    assert (np.abs(got[1] - ref[1]) <= 1e-14 * scale).all()
    assert np.allclose(got[2], ref[2], rtol=1e-12, atol=1e-300)


def test_simulate_logistic_buffers(env):
    """X and y written in full and nothing else; bit-equal to the host generator."""
    n, p = 5000, 37
    A = P.Arena(env.device)
    A.add("X", n * p * 8, 16, 8).add("y", n * 8).build()
    rc = env.lib.dlsa_simulate_logistic(A.ptr("X"), A.ptr("y"), n, p, 123, 777, env.stream)
    env.done(rc, "dlsa_simulate_logistic")
    A.guards_intact()
    A.fully_written("X", np.float64)
    A.fully_written("y", np.float64)
    Xh, yh = O.simulate_counter(n, p, seed=123, row0=777)
    assert np.array_equal(A.get("X", np.float64, (n, p)), Xh)
    assert np.array_equal(A.get("y", np.float64), yh)
