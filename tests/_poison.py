"""Poisoned buffers for the C-ABI tests (a helper module, not a test module).

Every test of tests/test_gpu_buffers.py hands the library device memory it
carved from an ``Arena``: one uint8 buffer filled with 0xFF in which the
inputs, the outputs and the workspace of a call sit as named regions with at
least 4 KiB of guard on both sides.  0xFF bytes read as NaN in fp64, fp32 and
bf16, as -1 in int32 / int64 and as the invalid level code 255 in uint8, so

  * a read before or after an input, or of a workspace element no kernel of
    this call wrote, that reaches a result turns it into NaN (or an
    invalid-code error, or a wild index);
  * ``guards_intact`` (byte-exact) sees any write outside a region;
  * ``fully_written`` sees an output element the call left alone.

The checks run on host copies as numpy, and an Arena without a device is a
numpy buffer, so tests/test_cpu_poison.py shows on the CPU that the checks
fail when they should.

The module also holds the list of fit cases of the GPU file (``FIT_CASES``:
shapes and options only, data is generated on demand and cached), their
yardsticks, and ``fit_call``, the ctypes caller of the five fit entry points
(it generalises ``_abi_fit`` of tests/test_gpu_ozaki.py).
"""

import ctypes
import dataclasses
import functools

import numpy as np

POISON = 0xFF
GUARD = 4096

STATUS_OK, STATUS_MAXITER, STATUS_SINGULAR, STATUS_EMPTY, STATUS_NONFINITE = 0, 1, 2, 3, 4
FAILED = (STATUS_SINGULAR, STATUS_EMPTY, STATUS_NONFINITE)


# ---------------------------------------------------------------------------
# the arena
# ---------------------------------------------------------------------------

class Arena:
    """Named regions inside one 0xFF-filled uint8 buffer.

    ``add(name, nbytes, align, phase)`` reserves a region whose address is
    ``phase`` modulo ``align``; ``build()`` allocates the buffer -- on
    ``device`` through torch, or as a numpy array when device is None -- and
    places the regions in the order they were added, each with at least
    GUARD bytes of 0xFF before and after it.  Every byte outside the regions
    is guard."""

    def __init__(self, device=None):
        self.device = device
        self._specs = []
        self.regions = {}     # name -> (offset, nbytes)
        self._inputs = {}     # name -> the bytes put() wrote (uint8 numpy)
        self.buf = None
        self.base = 0

    def add(self, name, nbytes, align=256, phase=0):
        assert self.buf is None and name not in [s[0] for s in self._specs]
        assert nbytes >= 0 and align >= 1 and 0 <= phase < align
        self._specs.append((name, int(nbytes), int(align), int(phase)))
        return self

    def build(self):
        total = GUARD + sum(n + a + GUARD for _, n, a, _ in self._specs)
        if self.device is None:
            self.buf = np.full(total, POISON, dtype=np.uint8)
            self.base = self.buf.ctypes.data
        else:
            import torch
            self.buf = torch.full((total,), POISON, dtype=torch.uint8, device=self.device)
            self.base = self.buf.data_ptr()
        off = GUARD
        for name, n, align, phase in self._specs:
            addr = self.base + off
            addr = (addr - phase + align - 1) // align * align + phase
            off = addr - self.base
            self.regions[name] = (off, n)
            off += n + GUARD
        assert off <= total
        return self

    # -- access -------------------------------------------------------------
    def ptr(self, name):
        return self.base + self.regions[name][0]

    def nbytes(self, name):
        return self.regions[name][1]

    def _slice(self, off, n):
        return self.buf[off:off + n]

    def _to_host(self, off, n):
        s = self._slice(off, n)
        return s.copy() if self.device is None else s.cpu().numpy()

    def _from_host(self, off, raw):
        if self.device is None:
            self.buf[off:off + raw.size] = raw
        else:
            import torch
            self.buf[off:off + raw.size].copy_(torch.from_numpy(raw))

    def fill(self, name, byte):
        off, n = self.regions[name]
        if self.device is None:
            self.buf[off:off + n] = byte
        else:
            self.buf[off:off + n].fill_(byte)

    def put(self, name, array):
        """Copy an input into its region (which it fills exactly) and keep
        its bytes for ``inputs_unchanged``."""
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        off, n = self.regions[name]
        assert raw.size == n, (name, raw.size, n)
        self._from_host(off, raw)
        self._inputs[name] = raw.copy()

    def put_bytes(self, name, raw):
        """Overwrite a region with the first nbytes of ``raw`` repeated to
        length (the stale workspace image); not tracked as an input."""
        off, n = self.regions[name]
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        if n == 0:
            return
        reps = -(-n // raw.size)
        if self.device is None:
            self.buf[off:off + n] = np.tile(raw, reps)[:n]
        else:
            import torch
            t = torch.from_numpy(raw[:n]).to(self.device)
            self.buf[off:off + n].copy_(t.repeat(reps)[:n] if reps > 1 else t)

    def snapshot(self, name):
        """A copy of a region where the arena lives (no host round trip)."""
        off, n = self.regions[name]
        return self.buf[off:off + n].copy() if self.device is None else \
            self.buf[off:off + n].clone()

    def same_as(self, name, snap):
        off, n = self.regions[name]
        if self.device is None:
            return np.array_equal(self.buf[off:off + n], snap)
        import torch
        return torch.equal(self.buf[off:off + n], snap)

    def raw(self, name):
        off, n = self.regions[name]
        return self._to_host(off, n)

    def get(self, name, dtype, shape=None):
        a = self.raw(name).view(dtype)
        return a if shape is None else a.reshape(shape)

    def tensor(self, name, dtype, shape):
        """A torch view of a region (device arenas), for device-side use."""
        off, n = self.regions[name]
        return self.buf[off:off + n].view(dtype).view(*shape)

    # -- checks ---------------------------------------------------------------
    def _bands(self):
        """(offset, length, name of the region after it or None) of every guard band."""
        end = int(self.buf.shape[0])
        spans = sorted((off, n, name) for name, (off, n) in self.regions.items())
        pos, out = 0, []
        for off, n, name in spans:
            assert off - pos >= GUARD, (name, off - pos)
            out.append((pos, off - pos, name))
            pos = off + n
        assert end - pos >= GUARD
        out.append((pos, end - pos, None))
        return out

    def guards_intact(self):
        """Every guard byte still holds 0xFF (byte-exact); raises AssertionError
        naming the first changed byte and the region next to it."""
        prev = None
        for off, n, name in self._bands():
            band = self._to_host(off, n)
            bad = np.nonzero(band != POISON)[0]
            if bad.size:
                i = int(bad[0])
                where = (f"{n - i} bytes before '{name}'" if name is not None and
                         (prev is None or n - i <= i + 1) else f"{i} bytes after '{prev}'")
                raise AssertionError(
                    f"guard byte changed: {bad.size} bytes in the band at {off}, the first "
                    f"{where} (now 0x{int(band[i]):02x})")
            prev = name
        return True

    def inputs_unchanged(self):
        for name, want in self._inputs.items():
            got = self.raw(name)
            if not np.array_equal(got, want):
                i = int(np.nonzero(got != want)[0][0])
                raise AssertionError(f"input '{name}' was written to (byte {i})")
        return True

    def fully_written(self, name, dtype):
        """No element of the region still holds the all-ones pattern."""
        a = self.raw(name)
        size = np.dtype(dtype).itemsize
        assert a.size % size == 0, (name, a.size, size)
        left = np.nonzero((a.reshape(-1, size) == POISON).all(axis=1))[0]
        if left.size:
            raise AssertionError(f"output '{name}': {left.size} of {a.size // size} elements "
                                 f"unwritten, the first at index {int(left[0])}")
        return True


# ---------------------------------------------------------------------------
# the fit cases
# ---------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class FitCase:
    """Shape and options of one fit (data comes from ``problem``)."""
    id: str
    entry: str                 # logistic | poisson | poisson_offset | ols | cat
    data: str                  # generator name, see problem()
    sizes: tuple
    p: int                     # columns of X (cat: numeric columns q)
    fi: bool
    rpc: int = 1000            # dlsa_fit_options.rows_per_chunk
    hessian: str = "mixed"
    max_iter: int = 100
    std: bool = False
    levels: tuple = ()         # cat: levels per factor
    nan_part: int = -1         # this partition gets a NaN in X ...
    nan_first: bool = False    # ... in column 0 of its first row (else somewhere inside)
    oz_max_bytes: int = 0
    small_ws: bool = False     # cat: a caller workspace one byte too small
    expect: tuple = ()         # preconditions on last_fit_stats, see check_expect()
    seed: int = 0
    warm_start: int = 1
    ref: bool = True           # compute the yardstick (the stale-image fits have none)
    check: tuple = ("theta", "sig_inv", "sig_inv_theta", "loglik")  # compared with it

    @property
    def K(self):
        return len(self.sizes)

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)

    @property
    def P(self):
        return self.p + int(self.fi) + sum(L - 1 for L in self.levels)


FUSED_SIZES = (3001, 0, 1500, 2003, 1200)      # the last partition gets the NaN
FUSED_SIZES_BIG = (12005, 0, 6001, 8013, 4801)  # P > 128: n_k / P as in the parity tests
POISSON_SIZES = (3001, 1500, 4096, 2003)
POISSON_SIZES_BIG = tuple(4 * s + 1 for s in POISSON_SIZES)
WIDE_SIZES = (6000, 5001, 4000)                 # _wide_problem of tests/test_gpu_ozaki.py
OLS_SIZES = (4000, 0, 2501, 3333)


def _fused(id_, p, fi, **kw):
    sizes = FUSED_SIZES if p + fi <= 128 else FUSED_SIZES_BIG
    return FitCase(id_, "logistic", "counter", sizes, p, fi, nan_part=4, seed=11 * p + fi, **kw)


def _poisson_cases(entry):
    t = "pois" if entry == "poisson" else "poisofs"
    return [
        FitCase(f"{t}-P16-mixed", entry, "poisson", POISSON_SIZES, 16, False),
        FitCase(f"{t}-P100-mixed", entry, "poisson", POISSON_SIZES, 99, True),
        FitCase(f"{t}-P100-fp64", entry, "poisson", POISSON_SIZES, 99, True, hessian="fp64"),
        FitCase(f"{t}-P129-mixed", entry, "poisson", POISSON_SIZES_BIG, 129, False),
        # [good, one y = -1, all y = 0, good] of test_gpu_poisson.test_bad_partitions
        FitCase(f"{t}-bad-partitions", entry, "poisson_bad", (2000,) * 4, 8, False, rpc=0),
        FitCase(f"{t}-P16-nan-behind-chunk", entry, "poisson", POISSON_SIZES, 16, False,
                nan_part=2, nan_first=True),
        # test_gpu_poisson.test_overflowing_step: exp overflows after the first step
        FitCase(f"{t}-overflowing-step", entry, "poisson_overflow", (4000,), 5, False, rpc=0),
    ]


FIT_CASES = [
    # ---- fused logistic ------------------------------------------------------
    _fused("fused-P13-mixed", 13, False),
    _fused("fused-P100-mixed", 99, True, expect=("oz",)),
    _fused("fused-P100-mixed_f32", 99, True, hessian="mixed_f32"),
    _fused("fused-P100-fp64", 99, True, hessian="fp64"),
    _fused("fused-P129-mixed", 129, False),
    _fused("fused-P192-mixed", 192, False),
    _fused("fused-P41-standardised", 40, True, std=True, expect=("oz",)),
    # test_gpu_parity.test_warm_start_level_runs_vs_oracle (fused shape)
    FitCase("fused-warm-start-level", "logistic", "counter", (6000, 5000, 0), 12, True, rpc=0,
            expect=("level",), seed=15),
    # test_gpu_robustness.test_stalled_bf16_partition_escalates
    FitCase("fused-stalled-escalation", "logistic", "collinear", (30000,), 10, True, rpc=0,
            max_iter=40, expect=("f32x",), check=("theta",)),
    # A NaN in the first row of partition 1 sits in the LDS block that ends
    # partition 0 (its rows past the chunk's end, and what the padded feature
    # lanes of the chunk's last row read): it must fail partition 1 alone.
    # 3001 rows: inside the last block; 3008: right behind a full block.
    FitCase("fused-P13-nan-behind-chunk", "logistic", "counter", (3001, 1500, 2003), 13, False,
            nan_part=1, nan_first=True, seed=143),
    FitCase("fused-P13-fp64-nan-behind-block", "logistic", "counter", (3008, 1504, 2003), 13,
            False, hessian="fp64", nan_part=1, nan_first=True, seed=143),
    FitCase("fused-P129-nan-behind-chunk", "logistic", "counter", (12005, 6001, 8013), 129, False,
            nan_part=1, nan_first=True, seed=1419),
    # ---- wide logistic -------------------------------------------------------
    FitCase("wide-P201-int8", "logistic", "counter", WIDE_SIZES, 201, False, rpc=2000,
            expect=("oz", "no_fallback"), seed=241),
    FitCase("wide-P201-fp64-gram", "logistic", "counter", WIDE_SIZES, 201, False, rpc=2000,
            oz_max_bytes=4096, expect=("fallback",), seed=241),
    FitCase("wide-P300-int8", "logistic", "counter", WIDE_SIZES, 300, False, rpc=2000,
            expect=("oz", "no_fallback"), seed=77),
    FitCase("wide-P300-fp64-gram", "logistic", "counter", WIDE_SIZES, 300, False, rpc=2000,
            oz_max_bytes=4096, expect=("fallback",), seed=77),
    # ---- categorical fit: two layouts of test_categorical_edge_layouts ---------
    FitCase("cat-q0-F2", "cat", "cat", (0,) * 2, 0, True, rpc=1500, levels=(6, 4), seed=5),
    FitCase("cat-q0-F2-small-ws", "cat", "cat", (0,) * 2, 0, True, rpc=1500, levels=(6, 4),
            seed=5, small_ws=True),
    FitCase("cat-q5-F0", "cat", "cat", (0,) * 2, 5, True, rpc=1500, seed=10),
    FitCase("cat-q5-F0-small-ws", "cat", "cat", (0,) * 2, 5, True, rpc=1500, seed=10,
            small_ws=True),
    # ---- OLS -----------------------------------------------------------------
    FitCase("ols-P13", "ols", "ols", OLS_SIZES, 13, False, rpc=900),
    FitCase("ols-P64", "ols", "ols", OLS_SIZES, 63, True, rpc=900),
    FitCase("ols-P129", "ols", "ols", OLS_SIZES, 129, False, rpc=900),
    FitCase("ols-wide-P300", "ols", "ols", WIDE_SIZES, 300, False, rpc=2000),
] + _poisson_cases("poisson") + _poisson_cases("poisson_offset")


def _cat_sizes(seed, n_parts=2):
    """The partition sizes of tests/test_gpu_parity.py::_cat_case."""
    rs = np.random.RandomState(seed)
    return tuple(int(s) for s in rs.randint(3000, 9000, size=n_parts))


FIT_CASES = [dataclasses.replace(c, sizes=_cat_sizes(c.seed)) if c.entry == "cat" else c
             for c in FIT_CASES]
FIT_CASE_IDS = [c.id for c in FIT_CASES]
assert len(set(FIT_CASE_IDS)) == len(FIT_CASE_IDS)


def align_up(v, a):
    return (v + a - 1) // a * a


def workspace_bytes(lib, case):
    """The caller workspace of a case: dlsa_logistic_workspace_bytes for the
    dense fits.  The categorical fit has no size query: its workspace is the
    fused layout of the dummy-expanded shape (which the query reports: an
    explicit rows_per_chunk, no warm-start level at these sizes) followed by
    the presence pass's counts, bad-code counters and column maxima and the
    fixed-point grids (fit_cat.hip), every region rounded up to 256 bytes."""
    off = case.offsets
    ic = int(case.fi)
    need = lib.dlsa_logistic_workspace_bytes(off.ctypes.data_as(ctypes.c_void_p), case.K,
                                             case.P - ic, ic, case.rpc)
    if case.entry != "cat" or need <= 0:
        return need
    assert case.rpc > 0 and need % 256 == 0
    nc = max(1, sum(-(-s // case.rpc) for s in case.sizes))
    D = sum(L - 1 for L in case.levels)
    qmax = 16  # kCatQMax
    for b in (4 * nc * max(D, 1), 4 * nc, 4 * case.K, 8 * qmax * nc, 8 * (qmax + 2) * case.K):
        need += align_up(b, 256)
    return need


def check_expect(case, stats, n_total):
    """The preconditions a case claims (never skipped on)."""
    for e in case.expect:
        if e == "oz":
            assert stats["passes_oz"] >= 1, stats
        elif e == "no_fallback":
            assert stats["oz_fallbacks"] == 0, stats
        elif e == "fallback":
            assert stats["oz_fallbacks"] == 1 and stats["passes_oz"] == 0, stats
        elif e == "level":  # a warm-start level ran: its passes stream a row prefix
            assert stats["passes_fp32"] > 0, stats
            assert stats["rows_fp32"] < stats["passes_fp32"] * n_total, stats
        elif e == "f32x":
            assert stats["passes_f32x"] >= 1, stats
        else:
            raise KeyError(e)


# ---- data and yardsticks -------------------------------------------------------

def _collinear(n, p, rho, seed):
    """tests/test_gpu_robustness.py::_collinear"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (n, p))
    z = rng.uniform(-0.5, 0.5, n)
    X[:, 1] = rho * X[:, 0] + np.sqrt(1 - rho * rho) * z
    eta = X[:, :4].sum(1)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return X, y


def _eta_offset(n, seed):
    return np.random.default_rng(1000 + seed).uniform(np.log(0.2), np.log(5.0), n)


@functools.lru_cache(maxsize=None)
def problem(c):
    """Data, expected statuses and yardstick of a case, computed once per
    process: a dict with X, y, (eta_offset, center, scale, codes), `status`
    [K] and `ref`: partition -> dict(theta, sig_inv, sig_inv_theta, loglik)."""
    import _glm_ref as G
    import oracle as O

    off = c.offsets
    n = int(off[-1])
    d = dict(center=None, scale=None, eta_offset=None, codes=None)
    status = np.array([STATUS_OK if s else STATUS_EMPTY for s in c.sizes], dtype=np.int32)
    ofs = c.entry == "poisson_offset"
    pref = None
    if c.data == "counter":
        X, y = O.simulate_counter(n, c.p, seed=c.seed)
        X = np.ascontiguousarray(X)
        if c.std:
            X = X * 3.0 - 0.7
            d["center"], d["scale"] = X.mean(0), X.std(0)
    elif c.data == "collinear":
        X, y = _collinear(n, c.p, 1 - 1e-7, seed=21)
    elif c.data == "ols":
        rs = np.random.RandomState(c.p)
        X = rs.rand(n, c.p) - 0.5
        y = X @ rs.randn(c.p) + 0.3 + 0.1 * rs.randn(n)
    elif c.data == "poisson":  # the cached cases (and fits) of the Poisson test modules
        if ofs:
            X, y, o, _, pref = G.case_offset(c.p, c.fi, c.sizes)
            d["eta_offset"] = o
        else:
            X, y, _, pref = G.case(c.p, c.fi, c.sizes)
    elif c.data == "poisson_bad":
        X, y = G.simulate(n, c.p, seed=3)
        y = y.copy()
        y[2000 + 777] = -1.0
        y[4000:6000] = 0.0
        status[1], status[2] = STATUS_NONFINITE, STATUS_SINGULAR
    elif c.data == "poisson_overflow":
        th = np.zeros(c.p)
        th[0] = 2.3
        X, y = G.simulate(n, c.p, seed=13, shift0=3.0, theta_true=th)
    elif c.data == "poisson_dirty":
        # the overshoot design of test_gpu_poisson.test_overshoot (no intercept,
        # mean y ~ 39: the step from theta = 0 is halved), one all-zero-y partition
        th = np.zeros(c.p)
        th[0] = 1.2
        X, y = G.simulate(n, c.p, seed=11, shift0=3.0, theta_true=th)
        y = y.copy()
        y[int(off[4]):int(off[5])] = 0.0
        status[4] = STATUS_SINGULAR
    elif c.data == "cat":
        # tests/test_gpu_parity.py::_cat_case(q, levels, 2, seed), not centred
        rs = np.random.RandomState(c.seed)
        rs.randint(3000, 9000, size=c.K)  # the sizes drawn by _cat_sizes
        q, levels = c.p, list(c.levels)
        X = rs.rand(n, q) - 0.5
        codes = np.stack([np.minimum((L * rs.rand(n) ** 2).astype(np.int64), L - 1)
                          for L in levels], 1).astype(np.uint8) if levels else \
            np.zeros((n, 0), np.uint8)
        D = sum(L - 1 for L in levels)
        beta = np.concatenate([rs.uniform(-1, 1, q), 0.4 * rs.randn(D)])
        Xd = O.expand_codes(X, codes, levels)
        y = (rs.rand(n) < 1 / (1 + np.exp(-(Xd @ beta - 0.2)))).astype(np.float64)
        d["codes"] = codes
    else:
        raise KeyError(c.data)
    if ofs and d["eta_offset"] is None:
        d["eta_offset"] = _eta_offset(n, c.p)
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    Xref = X
    if c.nan_part >= 0:
        X = X.copy()
        a, b = int(off[c.nan_part]), int(off[c.nan_part + 1])
        if c.nan_first:
            X[a, 0] = np.nan
        else:
            X[a + (b - a) // 3, c.p // 2] = np.nan
        status[c.nan_part] = STATUS_NONFINITE
    d.update(X=X, y=y, status=status)

    ref = {}
    d["ref"] = ref
    if not c.ref:
        return d
    std = dict(center=d["center"], scale=d["scale"]) if c.std else {}
    for k in range(c.K):
        if status[k] != STATUS_OK:
            continue
        a, b = int(off[k]), int(off[k + 1])
        if pref is not None:
            ref[k] = {name: pref[name][k] for name in ("theta", "sig_inv", "sig_inv_theta",
                                                       "loglik")}
        elif c.entry == "logistic":
            o = O.logistic_fit(Xref[a:b], y[a:b], fit_intercept=c.fi, **std)
            Z = G.design(Xref[a:b], c.fi, d["center"], d["scale"])
            ll = float(O.logistic_loglik(Z, y[a:b], o["coef"])[0])
            ref[k] = dict(theta=o["coef"], sig_inv=o["Sig_inv"], sig_inv_theta=o["Sig_invMcoef"],
                          loglik=ll)
        elif c.entry == "cat":
            Xd = O.expand_codes(X[a:b], d["codes"][a:b], list(c.levels))
            o = O.logistic_fit(Xd, y[a:b], fit_intercept=c.fi)
            ll = float(O.logistic_loglik(Xd, y[a:b], o["coef"], fit_intercept=c.fi)[0])
            ref[k] = dict(theta=o["coef"], sig_inv=o["Sig_inv"], sig_inv_theta=o["Sig_invMcoef"],
                          loglik=ll)
        elif c.entry == "ols":
            o = O.ols_fit(X[a:b], y[a:b], fit_intercept=c.fi)
            Z = G.design(X[a:b], c.fi)
            rss = float(((y[a:b] - Z @ o["coef"]) ** 2).sum())
            ref[k] = dict(theta=o["coef"], sig_inv=o["Sig_inv"], sig_inv_theta=o["Sig_invMcoef"],
                          loglik=rss)
        elif ofs:
            ref[k] = G.fit("poisson", X[a:b], y[a:b], o=d["eta_offset"][a:b], fit_intercept=c.fi)
        else:
            ref[k] = G.fit("poisson", X[a:b], y[a:b], fit_intercept=c.fi)
    d["ref"] = ref
    return d


# ---------------------------------------------------------------------------
# the ctypes caller of the fit entry points
# ---------------------------------------------------------------------------

HESSIAN = {"mixed": 0, "fp64": 1, "mixed_f32": 2}
OUT_DTYPES = dict(theta=np.float64, sig_inv=np.float64, sig_inv_theta=np.float64,
                  loglik=np.float64, iters=np.int32, status=np.int32)


def out_names(case):
    return [n for n in OUT_DTYPES if not (case.entry == "ols" and n == "iters")]


def fit_arena(case, data, ws_bytes, device):
    """The arena of one fit: X at an address that is 8 modulo 16 (the LDS-DMA
    shift path of test_misaligned_x_view), the other inputs, the six outputs
    and a workspace of exactly ws_bytes."""
    K, P = case.K, case.P
    A = Arena(device)
    A.add("X", data["X"].nbytes, 16, 8)
    A.add("y", data["y"].nbytes)
    for name in ("eta_offset", "center", "scale", "codes"):
        if data[name] is not None:
            A.add(name, data[name].nbytes)
    for name in out_names(case):
        n = {"theta": K * P, "sig_inv": K * P * P, "sig_inv_theta": K * P}.get(name, K)
        A.add(name, n * np.dtype(OUT_DTYPES[name]).itemsize)
    A.add("ws", ws_bytes)
    A.build()
    for name in ("X", "y", "eta_offset", "center", "scale", "codes"):
        if data.get(name) is not None:
            A.put(name, data[name])
    return A


def fit_call(lib, hip, case, A, ws_bytes, stream, null_ws=False):
    """One call of the case's entry point on the arena's regions; returns the
    return code.  null_ws: a NULL workspace instead of the arena's."""
    opt = hip.default_options()
    opt.hessian_mode = HESSIAN[case.hessian]
    opt.rows_per_chunk = case.rpc
    opt.oz_max_bytes = case.oz_max_bytes
    opt.warm_start = case.warm_start
    if not null_ws:
        opt.workspace = A.ptr("ws")
        opt.workspace_bytes = ws_bytes
    off = case.offsets
    offp = off.ctypes.data_as(ctypes.c_void_p)
    opt_in = lambda name: A.ptr(name) if name in A.regions else None  # noqa: E731
    outs = [A.ptr(n) for n in out_names(case)]
    ic = int(case.fi)
    tol = 1e-10
    if case.entry == "logistic":
        return lib.dlsa_logistic_fit_batched_ex(
            A.ptr("X"), A.ptr("y"), offp, case.K, case.p, ic, opt_in("center"), opt_in("scale"),
            case.max_iter, tol, *outs, ctypes.byref(opt), stream)
    if case.entry == "poisson":
        return lib.dlsa_poisson_fit_batched_ex(
            A.ptr("X"), A.ptr("y"), offp, case.K, case.p, ic, opt_in("center"), opt_in("scale"),
            case.max_iter, tol, *outs, ctypes.byref(opt), stream)
    if case.entry == "poisson_offset":
        return lib.dlsa_poisson_fit_batched_offset(
            A.ptr("X"), A.ptr("y"), A.ptr("eta_offset"), offp, case.K, case.p, ic,
            opt_in("center"), opt_in("scale"), case.max_iter, tol, *outs, ctypes.byref(opt),
            stream)
    if case.entry == "ols":
        return lib.dlsa_ols_fit_batched(
            A.ptr("X"), A.ptr("y"), offp, case.K, case.p, ic, opt_in("center"), opt_in("scale"),
            *outs, ctypes.byref(opt), stream)
    if case.entry == "cat":
        levels = np.asarray(case.levels, dtype=np.int32)
        return lib.dlsa_logistic_fit_categorical(
            A.ptr("X") if case.p else None, A.ptr("codes") if len(case.levels) else None,
            A.ptr("y"), offp, case.K, case.p, len(case.levels),
            levels.ctypes.data_as(ctypes.c_void_p), ic, opt_in("center"), opt_in("scale"),
            case.max_iter, tol, *outs, ctypes.byref(opt), stream)
    raise KeyError(case.entry)


def read_outputs(case, A):
    K, P = case.K, case.P
    shapes = dict(theta=(K, P), sig_inv=(K, P, P), sig_inv_theta=(K, P))
    return {n: A.get(n, OUT_DTYPES[n], shapes.get(n, (K,))) for n in out_names(case)}


def bits_equal(a, b):
    """Bit-for-bit equality of two arrays (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_zero_blocks(out, status):
    """include/dlsa_hip.h: a partition that ends EMPTY, SINGULAR or NONFINITE
    before any step has all-zero outputs and iters == 0."""
    for k, st in enumerate(status):
        if st not in FAILED:
            continue
        for name in ("theta", "sig_inv", "sig_inv_theta", "loglik"):
            assert not (out[name][k] != 0).any(), (name, k, int(st))
        if "iters" in out:
            assert out["iters"][k] == 0, (k, int(st), int(out["iters"][k]))


# The fits whose final workspace is the stale image of run C: more partitions,
# a larger P and more chunks than the fused cases they precede, the other
# family, max_iter = 2 (partitions end MAXITER with their Newton state, slabs
# and counters live), a NaN partition, an empty one, and for the Poisson one an
# all-zero-y partition and the overshoot design without a warm-start level, so
# that its second iteration halves the first step (backtracks = 1 stays behind).
STALE_POISSON = FitCase("stale-poisson", "poisson", "poisson_dirty",
                        (3000, 2500, 0, 3000, 2600, 3100, 2800), 150, False, rpc=500,
                        max_iter=2, nan_part=3, warm_start=0, ref=False)
STALE_LOGISTIC = FitCase("stale-logistic", "logistic", "counter",
                         (4000, 0, 3000, 3500, 3000, 3200), 150, False, rpc=500, max_iter=2,
                         nan_part=2, ref=False, seed=150)


# A level with MORE Gram row groups than the final plan (the case
# make_wide_layout sizes its tables and slabs for, fit_plan.hpp): by
# make_wide_plans the all-rows plan has ceil(n / 256) = 3063-row groups, 346 of
# them, while the 1/4 level (142 000 + 16 x 13 500 = 358 000 rows, the small
# partitions whole by the 64 P floor) has 1399-row groups, 347 of them.  X is
# generated on the device (1.2 GB).
SKEW_CASE = FitCase("wide-skewed-levels", "logistic", "device", (568000,) + (13500,) * 16, 193,
                    False, rpc=0, expect=("level", "oz", "no_fallback"), seed=31, ref=False)


def stale_case_for(case):
    """The other family's stale fit."""
    return STALE_LOGISTIC if case.entry.startswith("poisson") else STALE_POISSON
