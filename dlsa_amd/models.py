"""Map stage of DLSA on MI355X: per-partition logistic fits.

Drop-in for dlsa/models.py of the reference (Vicky-Lamperouge/dlsa):

* ``simulate_logistic``      -- models.py:6-40 (same legacy-RNG stream);
* ``logistic_model``         -- models.py:42-147, same signature and output
  frame; the fit itself runs on the GPU through ``logistic_model_batched``;
* ``logistic_model_batched`` -- K partitions in one batched Newton/IRLS run
  (the Spark ``groupby("partition_id").apply(udf)`` of
  projects/logistic_dlsa.py:314-325, without Spark);
* ``simulate_logistic_device`` -- synthetic data generated directly in HBM.

There is no CPU implementation of the fit: without libdlsa_hip.so or a GPU
these functions raise ``DlsaHipError``.
"""

from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass, field

import numpy as np

from . import _hip
from ._hip import DlsaHipError

try:  # torch is the HBM allocator / stream provider only
    import torch
except ImportError:  # pragma: no cover
    torch = None


# ---------------------------------------------------------------------------
# device helpers
# ---------------------------------------------------------------------------


def _require_gpu(device=None):
    if torch is None or not torch.cuda.is_available():
        raise DlsaHipError(
            "no ROCm GPU visible: the DLSA map stage runs only as HIP kernels on "
            "MI355X; there is no CPU fallback")
    _hip.load()
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _dev_f64(a, device):
    if isinstance(a, torch.Tensor):
        t = a.to(device=device, dtype=torch.float64)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
    return t.contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ---------------------------------------------------------------------------
# synthetic data
# ---------------------------------------------------------------------------


def simulate_logistic(sample_size, p, partition_method, partition_num):
    """Simulate data based on the logistic model (dlsa/models.py:6-40).

    Same draws as the reference for the same ``np.random.seed``: ``rand(n, p)``
    then one Bernoulli draw per row in row order (the reference's per-row
    ``binomial(n=1, p=prob[i], size=1)`` loop, models.py:28-30, consumes the
    legacy stream exactly like one vectorised call).  Unlike the reference the
    frame is built once (the reference rebuilds it inside the row loop,
    models.py:37-38, which is O(n^2)).
    """
    import pandas as pd

    if partition_method != "systematic":
        raise Exception("No such partition method implemented!")
    n = int(sample_size)
    n_true = int(p * 0.4)
    coef_true = np.zeros((p, 1))
    coef_true[:n_true] = 1.0
    feats = np.random.rand(n, p) - 0.5
    prob = 1 / (1 + np.exp(-feats.dot(coef_true)))
    label = np.random.binomial(1, prob[:, 0])
    pid = np.arange(n) % partition_num
    data = np.column_stack([pid.astype(np.float64), label.astype(np.float64), feats])
    return pd.DataFrame(data, columns=["partition_id", "label"] + [f"x{i}" for i in range(p)])


def simulate_logistic_device(n, p, seed=2019, row0=0, device=None):
    """Synthetic logistic data written straight into HBM:
    X[i, j] ~ U(-1/2, 1/2), beta* = 1 on the first floor(0.4 p) columns,
    y ~ Bernoulli(sigmoid(X beta*)), from counter-based streams (seed, row0 +
    i).  Returns (X [n, p] fp64, y [n] fp64) on ``device``."""
    dev = _require_gpu(device)
    X = torch.empty((int(n), int(p)), dtype=torch.float64, device=dev)
    y = torch.empty((int(n),), dtype=torch.float64, device=dev)
    lib = _hip.load()
    _hip.check(lib.dlsa_simulate_logistic(_ptr(X), _ptr(y), int(n), int(p), int(seed) & (2**64 - 1),
                                          int(row0), _stream(dev)), "dlsa_simulate_logistic")
    return X, y


#: airline-like design of BASELINE config 3: numeric columns + dummy-coded
#: factors (levels per factor; the first level of each is the dropped baseline,
#: models.py:65-69 with ``dummy_factors_baseline``) -> 9 + 11 + 6 + 19 + 68 + 68
#: = 181 columns, 182 parameters with the intercept.
AIRLINE_NUMERIC = 9
AIRLINE_FACTORS = (12, 7, 20, 69, 69)  # Month, DayOfWeek, UniqueCarrier, Origin, Dest


def simulate_categorical(n, seed=2019, numeric=AIRLINE_NUMERIC, factors=AIRLINE_FACTORS,
                         device=None):
    """Synthetic airline-like logistic data (BASELINE config 3) in the
    categorical-code layout, generated with torch ops on ``device`` ("cpu"
    allowed: test and baseline plumbing).

    ``numeric`` U(-1/2, 1/2) columns and, per factor with L levels, a uint8 code
    skewed towards low levels (code = floor(L u^2), like airport and carrier
    frequencies; code 0 is the baseline level).  y ~ Bernoulli(sigmoid(-0.3 +
    x beta*_num + sum_f beta*_f[code_f])) with beta*_num ~ U(-1, 1) and dummy
    effects ~ 0.3 N(0, 1) (fixed by ``seed``; the rows by ``seed`` too).
    Returns (Xn [n, numeric] fp64, codes [n, F] uint8, y [n] fp64, levels
    [F] int32 numpy); fit with ``fit_intercept=True``."""
    dev = torch.device(device) if device is not None else torch.device("cuda")
    n = int(n)
    D = sum(L - 1 for L in factors)
    gb = torch.Generator(device="cpu").manual_seed(int(seed) ^ 0x5EED)
    beta = torch.cat([torch.rand(numeric, generator=gb, dtype=torch.float64) * 2 - 1,
                      0.3 * torch.randn(D, generator=gb, dtype=torch.float64)]).to(dev)
    g = torch.Generator(device=dev).manual_seed(int(seed))
    Xn = torch.rand((n, numeric), generator=g, dtype=torch.float64, device=dev) - 0.5
    codes = torch.empty((n, len(factors)), dtype=torch.uint8, device=dev)
    eta = Xn @ beta[:numeric] - 0.3
    col = numeric
    for f, L in enumerate(factors):
        u = torch.rand((n,), generator=g, dtype=torch.float64, device=dev)
        code = torch.clamp((L * u * u).long(), max=L - 1)
        codes[:, f] = code.to(torch.uint8)
        eff = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), beta[col:col + L - 1]])
        eta = eta + eff[code]
        col += L - 1
    y = (torch.rand((n,), generator=g, dtype=torch.float64, device=dev) < torch.sigmoid(eta)).double()
    return Xn, codes, y, np.asarray(factors, dtype=np.int32)


def expand_categorical(Xn, codes, levels):
    """Dense dummy design [n, q + sum(L_f - 1)] of a categorical-code layout
    (the columns pd.get_dummies + the baseline drop of models.py:62-69 give).
    Works on torch tensors (any device) -- the dense baseline layout, not the
    product path."""
    n, q = Xn.shape
    levels = [int(L) for L in levels]
    X = torch.zeros((n, q + sum(L - 1 for L in levels)), dtype=torch.float64, device=Xn.device)
    X[:, :q] = Xn
    rows = torch.arange(n, device=Xn.device)
    col = q
    for f, L in enumerate(levels):
        c = codes[:, f].long()
        m = c > 0
        X[rows[m], col + c[m] - 1] = 1.0
        col += L - 1
    return X


def simulate_dummy_design(n, seed=2019, numeric=AIRLINE_NUMERIC, factors=AIRLINE_FACTORS,
                          device=None):
    """The same data as ``simulate_categorical`` as a dense dummy-coded design
    (the reference's layout after models.py:56-91).  Returns (X [n, p] fp64,
    y [n] fp64); fit it with ``fit_intercept=True``."""
    Xn, codes, y, levels = simulate_categorical(n, seed, numeric, factors, device)
    return expand_categorical(Xn, codes, levels), y


def encode_categorical(sample_df, Y_name, dummy_info, dummy_factors_baseline=()):
    """Categorical-code layout of one data chunk with the reference's dummy
    semantics (dlsa/models.py:56-91): dropped levels -> "000_OTHERS"
    (models.py:59), one column per sorted selected dummy name except the
    baselines (models.py:66-79), numeric columns sorted by name (models.py:70).

    Returns a dict: ``Xn`` [n, q] fp64, ``codes`` [n, F] uint8 (0 = baseline),
    ``levels`` [F] int32 (= dummy columns + 1), ``numeric`` / ``cols`` (the
    reference's column names, intercept excluded), ``unknown`` (a value outside
    the selected and baseline names: the reference's column-set check fails,
    models.py:84), ``unknown_rows`` ([n] bool: the rows holding such a value)
    and ``counts`` (rows per dummy column)."""
    factors = list(dummy_info["factor_selected"].keys())
    dropped = {k: v for k, v in dummy_info["factor_dropped"].items() if len(v) > 0}
    df = sample_df.replace(dropped, "000_OTHERS") if dropped else sample_df
    numeric = sorted(set(df.columns.drop(["partition_id", Y_name])) - set(factors))
    base = set(dummy_factors_baseline)
    n = len(df)
    codes = np.zeros((n, len(factors)), dtype=np.uint8)
    levels = np.zeros(len(factors), dtype=np.int32)
    cols = list(numeric)
    unknown = False
    unknown_rows = np.zeros(n, dtype=bool)
    counts = []
    for fi, f in enumerate(factors):
        names = [c for c in sorted(dummy_info["factor_selected_names"][f]) if c not in base]
        if len(names) > 255:
            raise ValueError(f"factor {f}: {len(names)} dummy columns > 255 (uint8 codes)")
        lut = {nm: j + 1 for j, nm in enumerate(names)}
        for b in base:
            if b.startswith(f + "_"):
                lut.setdefault(b, 0)
        import pandas as pd

        inv, uniq = pd.factorize(df[f], sort=False)  # one name per distinct value
        # a missing value (factorize code -1) has no dummy column in
        # pd.get_dummies (dummy_na=False): all-zero block = code 0
        mapped = np.array([lut.get(f"{f}_{u}", -1) for u in uniq] + [0], dtype=np.int64)
        c = mapped[inv] if n else np.zeros(0, dtype=np.int64)
        if (c < 0).any():
            unknown = True
            unknown_rows |= c < 0
            c = np.where(c < 0, 0, c)
        codes[:, fi] = c
        levels[fi] = len(names) + 1
        counts.append(np.bincount(c, minlength=len(names) + 1)[1:])
        cols.extend(names)
    Xn = np.ascontiguousarray(df[numeric].to_numpy(dtype=np.float64)) if numeric else \
        np.zeros((n, 0), dtype=np.float64)
    return {"Xn": Xn, "codes": codes, "levels": levels, "numeric": numeric, "cols": cols,
            "unknown": unknown, "unknown_rows": unknown_rows,
            "counts": np.concatenate(counts) if counts else np.zeros(0, dtype=np.int64)}


def partition_offsets(partition_id, num_partitions=None):
    """Group rows by partition id: returns (order, offsets) so that rows
    ``order[offsets[k]:offsets[k+1]]`` are partition k in their original order
    (what Spark's repartition + groupby hand to each UDF call,
    projects/logistic_dlsa.py:303-325)."""
    pid = np.asarray(partition_id).astype(np.int64)
    K = int(num_partitions) if num_partitions is not None else (int(pid.max()) + 1 if pid.size else 0)
    order = np.argsort(pid, kind="stable")
    offsets = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(np.bincount(pid, minlength=K), out=offsets[1:])
    return order, offsets


# ---------------------------------------------------------------------------
# batched fit (the hot path)
# ---------------------------------------------------------------------------


@dataclass
class BatchedFit:
    """Result of one batched fit; tensors live in HBM."""
    theta: "torch.Tensor"          # [K, P]  coef (intercept first)
    sig_inv: "torch.Tensor"        # [K, P, P] X^T W X at theta
    sig_inv_theta: "torch.Tensor"  # [K, P]  Sig_inv @ theta
    loglik: "torch.Tensor"         # [K]
    iters: "torch.Tensor"          # [K] int32
    status: "torch.Tensor"         # [K] int32 (0 ok, 1 maxiter, 2 singular, 3 empty, 4 nonfinite)
    offsets: np.ndarray            # [K+1] host
    fit_intercept: bool
    stats: dict = field(default_factory=dict)

    @property
    def K(self):
        return int(self.theta.shape[0])

    @property
    def P(self):
        return int(self.theta.shape[1])

    @property
    def n_rows(self):
        return int(self.offsets[-1])

    def status_counts(self):
        s = self.status.cpu().numpy()
        return {_hip.STATUS_NAMES.get(int(v), str(v)): int((s == v).sum()) for v in np.unique(s)}


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _size(v):
    is_t = torch is not None and isinstance(v, torch.Tensor)
    return int(v.numel()) if is_t else int(np.size(v))


def _check_row_extra(name, v, n, pred=None, must=None):
    """The argument check of a per-row extra ``v`` (None: not given), before
    anything touches the GPU: n entries, and with ``pred`` every one finite
    and satisfying it (``must``: the ValueError's text)."""
    if v is None:
        return
    if _size(v) != n:
        raise ValueError(f"{name} must have n entries (one per row of X)")
    if pred is not None:
        is_t = torch is not None and isinstance(v, torch.Tensor)
        a = v if is_t else np.asarray(v, dtype=np.float64)
        if not bool(((torch if is_t else np).isfinite(a) & pred(a)).all()):
            raise ValueError(must)


def _check_row_extras(X, with_offset, eta_offset, exposure, sample_weight):
    """The checks of a family's offset and weight arguments: one of
    ``eta_offset`` / ``exposure`` at most (its log is the offset, so an
    exposure is finite and > 0), weights finite and >= 0."""
    n = _shape(X)[0]
    if with_offset:
        if eta_offset is not None and exposure is not None:
            raise ValueError("give eta_offset or exposure (eta_offset = log exposure), not both")
        _check_row_extra("eta_offset / exposure", eta_offset, n)
        _check_row_extra("eta_offset / exposure", exposure, n, lambda a: a > 0,
                         "exposure must be finite and > 0 (drop the rows with none)")
    _check_row_extra("sample_weight", sample_weight, n, lambda a: a >= 0,
                     "sample_weight must be finite and >= 0")


def _entry_and_extras(entry, weighted_entry, with_offset, eta_offset, exposure, sample_weight,
                      dev):
    """The C-ABI symbol of a family's call and the device tensors it takes
    between y and offsets (None: a null pointer): with ``with_offset``,
    ``entry`` takes the [n] offset (log exposure taken on the device; null
    when neither is given); with ``sample_weight`` the call is
    ``weighted_entry``, which takes the weights behind that."""
    extras = []
    if with_offset:
        od = None
        if exposure is not None:
            od = torch.log(_dev_f64(exposure, dev).reshape(-1))
        elif eta_offset is not None:
            od = _dev_f64(eta_offset, dev).reshape(-1)
        extras.append(od)
    if sample_weight is not None:
        entry = weighted_entry
        extras.append(_dev_f64(sample_weight, dev).reshape(-1))
    return entry, extras


def _check_rows(offsets, n, y):
    """Host offsets [K+1] int64 of n rows, checked together with y's length."""
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if offs.ndim != 1 or offs.size < 2 or offs[0] != 0 or offs[-1] != n or \
            np.any(np.diff(offs) < 0):
        raise ValueError("offsets must be non-decreasing, start at 0 and end at n")
    if _size(y) != n:
        raise ValueError("y must have n entries")
    return offs


def _center_scale(center, scale, ncols, what, dev=None):
    """center / scale: both or neither, ``ncols`` entries each (``what``: the
    count in words).  With ``dev`` their [ncols] device copies (None, None
    without them)."""
    if center is None and scale is None:
        return None, None
    if center is None or scale is None or _size(center) != ncols or _size(scale) != ncols:
        raise ValueError(f"center and scale must both be given, with {what} entries each")
    if dev is None:
        return None, None
    return _dev_f64(center, dev).reshape(-1), _dev_f64(scale, dev).reshape(-1)


def _dense_inputs(X, y, offsets, center, scale, device):
    """Checked device copies of a dense layout, the dense counterpart of
    ``_cat_inputs``: (device, X [n, p] fp64, y [n], host offsets [K+1] int64,
    center, scale ([p] or None)).  Every check comes before the GPU is
    touched."""
    if len(_shape(X)) != 2:
        raise ValueError("X must be 2-D [n, p]")
    n, p = _shape(X)
    offs = _check_rows(offsets, n, y)
    _center_scale(center, scale, p, "p")
    dev = _require_gpu(device)
    return (dev, _dev_f64(X, dev), _dev_f64(y, dev).reshape(-1), offs,
            *_center_scale(center, scale, p, "p", dev))


def _alloc_outputs(K, P, dev):
    """The six output tensors of a fit: theta, sig_inv, sig_inv_theta, loglik,
    iters, status."""
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    return (torch.empty((K, P), **f64), torch.empty((K, P, P), **f64), torch.empty((K, P), **f64),
            torch.empty((K,), **f64), torch.empty((K,), **i32), torch.empty((K,), **i32))


def _glm_model_batched(entry, X, y, offsets, fit_intercept, center, scale, max_iter, tol,
                       hessian, switch_tol, record_timing, rows_per_chunk, workspace, device,
                       exact, exact_waves, oz_max_bytes, with_offset=False, eta_offset=None,
                       exposure=None, sample_weight=None, weighted_entry=None):
    """The body the iterative families share: checked device copies, outputs,
    options and workspace, then the C-ABI call ``entry`` (an ``*_fit_batched_ex``
    symbol, or with ``with_offset`` one that takes ``eta_offset`` after y: the
    pointer is null when neither ``eta_offset`` nor ``exposure`` is given).
    With ``sample_weight`` the call is ``weighted_entry`` instead, which takes
    the weights after y (after ``eta_offset`` when ``with_offset``).
    Returns a BatchedFit."""
    _check_row_extras(X, with_offset, eta_offset, exposure, sample_weight)
    dev, Xd, yd, offs, cd, sd = _dense_inputs(X, y, offsets, center, scale, device)
    entry, extras = _entry_and_extras(entry, weighted_entry, with_offset, eta_offset, exposure,
                                      sample_weight, dev)
    p, K = Xd.shape[1], offs.size - 1
    P = p + (1 if fit_intercept else 0)
    if P > _hip.MAX_P:
        raise DlsaHipError(f"P = {P} > {_hip.MAX_P} is not supported")
    theta, sig, sigt, ll, iters, status = _alloc_outputs(K, P, dev)

    lib = _hip.load()
    opt = _hip.default_options()
    opt.hessian_mode = {"mixed": _hip.HESSIAN_MIXED, "fp64": _hip.HESSIAN_FP64,
                        "mixed_f32": _hip.HESSIAN_MIXED_F32}[hessian]
    opt.switch_tol = float(switch_tol)
    opt.record_timing = 1 if record_timing else 0
    opt.rows_per_chunk = int(rows_per_chunk)
    opt.exact_pass = {"auto": _hip.EXACT_AUTO, "fp64": _hip.EXACT_FP64}[exact]
    opt.exact_waves = int(exact_waves)
    opt.oz_max_bytes = int(oz_max_bytes)
    offs_p = offs.ctypes.data_as(ctypes.c_void_p)
    need = lib.dlsa_logistic_workspace_bytes(offs_p, K, p, int(bool(fit_intercept)),
                                             opt.rows_per_chunk)
    if need < 0:
        raise DlsaHipError(_hip.last_error())
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(int(need), 1),), dtype=torch.uint8, device=dev)
    opt.workspace = workspace.data_ptr()
    opt.workspace_bytes = workspace.numel()
    rc = getattr(lib, entry)(
        _ptr(Xd), _ptr(yd), *map(_ptr, extras), offs_p, K, p,
        int(bool(fit_intercept)), _ptr(cd), _ptr(sd),
        int(max_iter), float(tol), _ptr(theta), _ptr(sig), _ptr(sigt), _ptr(ll), _ptr(iters),
        _ptr(status), ctypes.byref(opt), _stream(dev))
    _hip.check(rc, entry)
    stats = _hip.last_fit_stats()
    stats["workspace_bytes"] = int(need)
    return BatchedFit(theta, sig, sigt, ll, iters, status, offs, bool(fit_intercept), stats)


def logistic_model_batched(X, y, offsets, fit_intercept=False, center=None, scale=None,
                           max_iter=100, tol=1e-10, hessian="mixed", switch_tol=1e-6,
                           record_timing=False, rows_per_chunk=0, workspace=None,
                           device=None, exact="auto", exact_waves=0, oz_max_bytes=0):
    """Fit K row partitions at once on the GPU (batched Newton/IRLS).

    Per partition k (rows ``offsets[k]:offsets[k+1]`` of X) this computes what
    ``logistic_model`` returns for one Spark group (models.py:94-131): the
    unpenalised MLE ``theta_k`` (intercept first when ``fit_intercept``),
    ``Sig_inv_k = X_k^T diag(p(1-p)) X_k`` at theta_k and
    ``Sig_inv_k theta_k``.  ``center``/``scale`` standardise the columns like
    models.py:99-101.

    X: [n, p] fp64 (torch tensor on the GPU, or array-like, copied once);
    y: [n] 0/1; offsets: K+1 host ints.  ``hessian`` = "mixed" (bf16-MFMA
    Hessian until the Newton step is below ``switch_tol``, then fp64-MFMA
    passes; the gradient and the returned Sig_inv are always fp64),
    "mixed_f32" (fp32-MFMA approximate Hessian) or "fp64".  ``exact`` =
    "auto" (the exact pass that publishes Sig_inv on the int8 matrix cores,
    as int8 digit slices, wherever it applies; ~1e-12 per entry) or "fp64"
    (fp64 MFMA); ``exact_waves`` (0, 1, 2) the fp64 exact pass's geometry
    for P <= 128 and ``oz_max_bytes`` a cap on the wide path's int8 digit
    records (include/dlsa_hip.h, dlsa_fit_options).
    """
    return _glm_model_batched("dlsa_logistic_fit_batched_ex", X, y, offsets, fit_intercept, center,
                              scale, max_iter, tol, hessian, switch_tol, record_timing,
                              rows_per_chunk, workspace, device, exact, exact_waves, oz_max_bytes)


def logistic_model_batched_weighted(X, y, offsets, sample_weight=None, fit_intercept=False,
                                    center=None, scale=None, max_iter=100, tol=1e-10,
                                    hessian="mixed", switch_tol=1e-6, record_timing=False,
                                    rows_per_chunk=0, workspace=None, device=None, exact_waves=0):
    """``logistic_model_batched`` with per-row prior weights.

    ``sample_weight`` [n] (None: exactly the unweighted call): per-row prior
    weights omega, finite and >= 0 (``ValueError`` otherwise, or for a wrong
    length), as R's ``glm(weights=)``: the IRLS weight is omega w, the score
    sum omega (y - mu) x, ``Sig_inv = X^T diag(omega w) X`` and ``loglik = sum
    omega l_i``.  omega = 0 drops a row (its x and y must still be finite).  y
    is used as given: y = s / m with omega = m is the grouped-binomial fit
    (without the binomial-coefficient constant in loglik).  A partition whose
    weights sum to 0 gets status "singular".  Weighted fits run on the fused
    path only (P <= 192, ``DlsaHipError`` above) and take their exact passes
    on the fp64 MFMA (there is no ``exact``; stats ``passes_oz`` stays 0)
    (``dlsa_logistic_fit_batched_weighted``).
    """
    return _glm_model_batched("dlsa_logistic_fit_batched_ex", X, y, offsets, fit_intercept, center,
                              scale, max_iter, tol, hessian, switch_tol, record_timing,
                              rows_per_chunk, workspace, device, "auto", exact_waves, 0,
                              sample_weight=sample_weight,
                              weighted_entry="dlsa_logistic_fit_batched_weighted")


def poisson_model_batched(X, y, offsets, fit_intercept=False, center=None, scale=None,
                          max_iter=100, tol=1e-10, hessian="mixed", switch_tol=1e-6,
                          record_timing=False, rows_per_chunk=0, workspace=None, device=None,
                          exact_waves=0):
    """Fit K row partitions of count data at once on the GPU: Poisson
    regression with the log link (``dlsa_poisson_fit_batched_ex``).

    Per partition k: eta = x . theta, mu = exp(eta); ``theta_k`` the
    unpenalised MLE (intercept first when ``fit_intercept``), ``Sig_inv_k =
    X_k^T diag(mu) X_k`` at theta_k, ``Sig_inv_k theta_k`` and the full
    log-likelihood ``sum y eta - mu - lgamma(y + 1)``.  y is real, finite and
    >= 0.  Arguments as ``logistic_model_batched``; the exact passes always run
    on the fp64 MFMA (the weights are unbounded: no int8 pass).  The fit starts
    at the intercept-only MLE (log mean y); a partition with a negative or
    non-finite y gets status "nonfinite", one with sum y = 0 "singular", both
    with all-zero outputs.  P = p + intercept <= 192 (``DlsaHipError`` above).
    The BatchedFit feeds ``dlsa_mapred`` / ``reduce_partitions_device`` like a
    logistic one: the combine step never looks at the likelihood."""
    return _glm_model_batched("dlsa_poisson_fit_batched_ex", X, y, offsets, fit_intercept, center,
                              scale, max_iter, tol, hessian, switch_tol, record_timing,
                              rows_per_chunk, workspace, device, "auto", exact_waves, 0)


def poisson_model_batched_offset(X, y, offsets, eta_offset=None, exposure=None,
                                 fit_intercept=False, center=None, scale=None, max_iter=100,
                                 tol=1e-10, hessian="mixed", switch_tol=1e-6,
                                 record_timing=False, rows_per_chunk=0, workspace=None,
                                 device=None, exact_waves=0):
    """``poisson_model_batched`` for rate data: ``eta = x . theta + eta_offset``
    with a known per-row ``eta_offset`` [n] (R's ``glm(offset=)``), or
    ``exposure`` [n] > 0 whose log, taken on the device, is the offset
    (statsmodels' ``exposure=``); both raise ``ValueError``, as does a wrong
    length or an exposure that is not finite and positive.  (``offsets`` stays
    the partition boundaries.)  Neither given: exactly ``poisson_model_batched``.
    Sig_inv and the log-likelihood are taken at mu = exp(eta) with the offset.
    With an intercept the fit starts at log(sum y / sum exp(eta_offset)); a
    partition with a non-finite ``eta_offset`` gets status "nonfinite" and
    all-zero outputs, the others are unaffected
    (``dlsa_poisson_fit_batched_offset``).  The other arguments, the limit
    P <= 192 and the result as ``poisson_model_batched``."""
    return _glm_model_batched("dlsa_poisson_fit_batched_offset", X, y, offsets, fit_intercept,
                              center, scale, max_iter, tol, hessian, switch_tol, record_timing,
                              rows_per_chunk, workspace, device, "auto", exact_waves, 0,
                              with_offset=True, eta_offset=eta_offset, exposure=exposure)


def poisson_model_batched_weighted(X, y, offsets, sample_weight=None, eta_offset=None,
                                   exposure=None, fit_intercept=False, center=None, scale=None,
                                   max_iter=100, tol=1e-10, hessian="mixed", switch_tol=1e-6,
                                   record_timing=False, rows_per_chunk=0, workspace=None,
                                   device=None, exact_waves=0):
    """``poisson_model_batched`` / ``poisson_model_batched_offset`` with per-row
    prior weights omega = ``sample_weight`` [n], finite and >= 0 (``ValueError``
    otherwise, or for a wrong length; None: exactly the unweighted call), as
    in ``logistic_model_batched_weighted``: ``Sig_inv = X^T diag(omega mu) X``,
    ``loglik = sum omega (y eta - mu - lgamma(y + 1))``.  With an intercept the
    fit starts at log(sum omega y / sum omega exp(eta_offset)); a partition
    with sum omega = 0 or sum omega y = 0 gets status "singular", all-zero
    outputs (``dlsa_poisson_fit_batched_weighted``).  ``eta_offset`` /
    ``exposure`` are optional, as in ``poisson_model_batched_offset``."""
    return _glm_model_batched("dlsa_poisson_fit_batched_offset", X, y, offsets, fit_intercept,
                              center, scale, max_iter, tol, hessian, switch_tol, record_timing,
                              rows_per_chunk, workspace, device, "auto", exact_waves, 0,
                              with_offset=True, eta_offset=eta_offset, exposure=exposure,
                              sample_weight=sample_weight,
                              weighted_entry="dlsa_poisson_fit_batched_weighted")


def _cat_inputs(Xn, codes, y, offsets, levels, center, scale, dev):
    """Checked device copies of a categorical-code layout: (Xn [n, q] fp64,
    codes [n, F] uint8, y [n], host offsets [K+1] int64, host levels [F]
    int32, center, scale ([q] or None))."""
    if len(_shape(Xn)) != 2:
        raise ValueError("Xn must be 2-D [n, q]")
    n, q = _shape(Xn)
    if isinstance(codes, torch.Tensor):
        cd8 = codes.to(device=dev, dtype=torch.uint8).contiguous()
    else:
        cd8 = torch.from_numpy(np.ascontiguousarray(np.asarray(codes, dtype=np.uint8))).to(dev)
    if cd8.dim() != 2 or cd8.shape[0] != n:
        raise ValueError("codes must be [n, F]")
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.int32).reshape(-1))
    if lv.size != cd8.shape[1]:
        raise ValueError("levels must have F entries")
    offs = _check_rows(offsets, n, y)
    cen, sca = _center_scale(center, scale, q, "q (the numeric columns)", dev)
    return _dev_f64(Xn, dev), cd8, _dev_f64(y, dev).reshape(-1), offs, lv, cen, sca


def logistic_model_batched_categorical(Xn, codes, y, offsets, levels, fit_intercept=False,
                                       center=None, scale=None, max_iter=100, tol=1e-10,
                                       record_timing=False, rows_per_chunk=0, zero_partitions=None,
                                       device=None):
    """Batched local logistic fit on the categorical-code layout (the dummy
    branch of dlsa/models.py:56-91, BASELINE config 3) without materialising
    the dummy matrix: the one-hot blocks of X^T W X are LDS histograms in the
    HIP pass (``dlsa_logistic_fit_categorical``).

    Xn: [n, q] fp64 numeric columns; codes: [n, F] uint8 level codes (0 =
    baseline, c = dummy column c of the factor); levels: F ints (dummy columns
    + 1); ``center``/``scale`` [q] standardise the numeric columns only
    (models.py:99-101).  Parameters: [intercept] [numeric] [factor 0 dummies]
    ...  A partition with a dummy column that has no rows gets status
    "missing_level" and all-zero outputs (the reference's zero frame), and so
    does every partition listed in ``zero_partitions`` (the partitions holding
    a factor value outside dummy_info, ``read_csv_partitioned``'s
    ``zero_partitions``: the reference's column-set check fails there too,
    models.py:84-91)."""
    return logistic_model_batched_categorical_weighted(
        Xn, codes, y, offsets, levels, None, fit_intercept, center, scale, max_iter, tol,
        record_timing, rows_per_chunk, zero_partitions, device)


def logistic_model_batched_categorical_weighted(Xn, codes, y, offsets, levels, sample_weight=None,
                                                fit_intercept=False, center=None, scale=None,
                                                max_iter=100, tol=1e-10, record_timing=False,
                                                rows_per_chunk=0, zero_partitions=None,
                                                device=None):
    """``logistic_model_batched_categorical`` with per-row prior weights.

    ``sample_weight`` [n] (None: exactly the unweighted call): prior weights
    omega, finite and >= 0 (``ValueError`` otherwise, or for a wrong length),
    with the semantics of ``logistic_model_batched_weighted`` on the
    dummy-expanded design.  The canonical use is a design made of factors
    collapsed to its distinct cells: rows (cell, s successes, m trials) with
    y = s / m and omega = m give the MLE and Sig_inv of the replicated 0/1
    rows.  omega = 0 drops a row: a dummy column whose rows all have omega = 0
    makes the partition "missing_level"; a negative or non-finite weight met on
    the device "nonfinite", weights that sum to 0 "singular"
    (``dlsa_logistic_fit_categorical_weighted``)."""
    _check_row_extras(Xn, False, None, None, sample_weight)
    dev = _require_gpu(device)
    Xd, cd8, yd, offs, lv, cen, sca = _cat_inputs(Xn, codes, y, offsets, levels, center, scale,
                                                  dev)
    entry, extras = _entry_and_extras("dlsa_logistic_fit_categorical",
                                      "dlsa_logistic_fit_categorical_weighted", False, None, None,
                                      sample_weight, dev)
    return _cat_fit(entry, extras, Xd, cd8, yd, offs, lv, cen, sca, fit_intercept, max_iter, tol,
                    record_timing, rows_per_chunk, zero_partitions, dev)


def _cat_fit(entry, extras, Xd, cd8, yd, offs, lv, cen, sca, fit_intercept, max_iter, tol,
             record_timing, rows_per_chunk, zero_partitions, dev):
    """The C-ABI call of a fit on the categorical-code layout (``entry`` takes
    ``extras`` between y and offsets) on ``_cat_inputs``' tensors."""
    q, F, K = Xd.shape[1], cd8.shape[1], offs.size - 1
    P = int(bool(fit_intercept)) + q + int((lv - 1).sum())
    theta, sig, sigt, ll, iters, status = _alloc_outputs(K, P, dev)
    lib = _hip.load()
    opt = _hip.default_options()
    opt.record_timing = 1 if record_timing else 0
    opt.rows_per_chunk = int(rows_per_chunk)
    rc = getattr(lib, entry)(
        _ptr(Xd), _ptr(cd8), _ptr(yd), *map(_ptr, extras), offs.ctypes.data_as(ctypes.c_void_p),
        K, q, F,
        lv.ctypes.data_as(ctypes.c_void_p), int(bool(fit_intercept)), _ptr(cen), _ptr(sca),
        int(max_iter), float(tol), _ptr(theta), _ptr(sig), _ptr(sigt), _ptr(ll), _ptr(iters),
        _ptr(status), ctypes.byref(opt), _stream(dev))
    _hip.check(rc, entry)
    stats = _hip.last_fit_stats()
    if zero_partitions is not None and len(zero_partitions):
        idx = torch.as_tensor(np.asarray(zero_partitions, dtype=np.int64), device=dev)
        for t in (theta, sig, sigt, ll):
            t[idx] = 0
        status[idx] = 5
    return BatchedFit(theta, sig, sigt, ll, iters, status, offs, bool(fit_intercept), stats)


def _pois_cat_extras(entry, Xn, eta_offset, exposure, sample_weight, device):
    """The argument checks of a Poisson call on the code layout, in their
    order (Xn 2-D, then the row extras; all before the GPU), then the device
    and the two tensors ``entry`` takes after y (None: a null pointer)."""
    if len(_shape(Xn)) != 2:
        raise ValueError("Xn must be 2-D [n, q]")
    _check_row_extras(Xn, True, eta_offset, exposure, sample_weight)
    dev = _require_gpu(device)
    _, extras = _entry_and_extras(entry, entry, True, eta_offset, exposure, sample_weight, dev)
    return dev, (extras + [None])[:2]


def poisson_model_batched_categorical(Xn, codes, y, offsets, levels, sample_weight=None,
                                      eta_offset=None, exposure=None, fit_intercept=False,
                                      center=None, scale=None, max_iter=100, tol=1e-10,
                                      record_timing=False, rows_per_chunk=0, zero_partitions=None,
                                      device=None):
    """Poisson regression (log link) on the categorical-code layout of
    ``logistic_model_batched_categorical`` (same Xn / codes / levels / center /
    scale, parameter order, limits and "missing_level" rule): count data with
    an exposure on a design made of factors, a claim table, without the dummy
    matrix (``dlsa_poisson_fit_categorical``).

    Per partition exactly ``poisson_model_batched_weighted`` on the
    dummy-expanded design: ``eta = x . theta + eta_offset``, ``Sig_inv = X^T
    diag(omega mu) X``, ``loglik = sum omega (y eta - mu - lgamma(y + 1))``.
    ``eta_offset`` [n] or ``exposure`` [n] > 0 (its log, taken on the device,
    is the offset) and ``sample_weight`` [n] (finite, >= 0; 0 drops the row)
    are optional, in any combination, with the ``ValueError`` cases of that
    function.  Collapsing raw rows to their distinct cells with y = sum y and
    exposure = sum exposure leaves theta and Sig_inv unchanged.  Statuses: a
    negative or non-finite y or offset "nonfinite", sum omega y = 0 "singular",
    a dummy column without a row of omega > 0 "missing_level".  There is no
    warm-start level for this family on this layout."""
    dev, extras = _pois_cat_extras("dlsa_poisson_fit_categorical", Xn, eta_offset, exposure,
                                   sample_weight, device)
    Xd, cd8, yd, offs, lv, cen, sca = _cat_inputs(Xn, codes, y, offsets, levels, center, scale,
                                                  dev)
    return _cat_fit("dlsa_poisson_fit_categorical", extras, Xd, cd8, yd, offs, lv, cen, sca,
                    fit_intercept, max_iter, tol, record_timing, rows_per_chunk, zero_partitions,
                    dev)


def ols_model_batched(X, y, offsets, fit_intercept=False, center=None, scale=None,
                      rows_per_chunk=0, record_timing=False, device=None, exact_waves=0):
    """Batched local OLS (linear DLSA path): per
    partition theta_k = (X_k^T X_k)^-1 X_k^T y_k and Sig_inv_k = X_k^T X_k from
    one fused fp64 pass.  Returns a BatchedFit whose ``loglik`` field holds the
    residual sum of squares of each partition."""
    dev, Xd, yd, offs, cd, sd = _dense_inputs(X, y, offsets, center, scale, device)
    p, K = Xd.shape[1], offs.size - 1
    P = p + (1 if fit_intercept else 0)
    if P > _hip.MAX_P:
        raise DlsaHipError(f"P = {P} > {_hip.MAX_P} is not supported")
    theta, sig, sigt, rss, iters, status = _alloc_outputs(K, P, dev)
    iters.fill_(1)
    lib = _hip.load()
    opt = _hip.default_options()
    opt.rows_per_chunk = int(rows_per_chunk)
    opt.record_timing = 1 if record_timing else 0
    opt.exact_waves = int(exact_waves)
    rc = lib.dlsa_ols_fit_batched(_ptr(Xd), _ptr(yd), offs.ctypes.data_as(ctypes.c_void_p), K, p,
                                  int(bool(fit_intercept)), _ptr(cd), _ptr(sd), _ptr(theta),
                                  _ptr(sig), _ptr(sigt), _ptr(rss), _ptr(status),
                                  ctypes.byref(opt), _stream(dev))
    _hip.check(rc, "dlsa_ols_fit_batched")
    return BatchedFit(theta, sig, sigt, rss, iters, status, offs, bool(fit_intercept),
                      _hip.last_fit_stats())


MAX_LOGLIK_CANDIDATES = 16  # candidates of one evaluation pass (n_beta of the C-ABI)


def _loglik_groups(call, betas, P, K, dev, return_sum):
    """Run ``call(betas_group, g, out [K, g], total [g])`` over the candidates
    in groups of at most 16 (one pass over the data per group) and assemble
    the [K, B] log-likelihoods and their [B] sum over k."""
    bd = _dev_f64(betas, dev)
    if bd.dim() == 1:
        bd = bd.reshape(1, -1)
    if bd.dim() != 2 or bd.shape[0] < 1 or bd.shape[1] != P:
        raise ValueError("betas must be [B, P] with B >= 1 and P = the design's parameters")
    B = bd.shape[0]
    out = torch.empty((K, B), dtype=torch.float64, device=dev)
    total = torch.empty((B,), dtype=torch.float64, device=dev)
    for b0 in range(0, B, MAX_LOGLIK_CANDIDATES):
        g = min(MAX_LOGLIK_CANDIDATES, B - b0)
        part = out if g == B else torch.empty((K, g), dtype=torch.float64, device=dev)
        call(bd[b0:b0 + g].contiguous(), g, part, total[b0:b0 + g])
        if part is not out:
            out[:, b0:b0 + g] = part
    return (out, total) if return_sum else out


def _loglik_dense(entry, X, y, offsets, betas, fit_intercept, center, scale, device, return_sum,
                  with_offset=False, eta_offset=None, exposure=None, sample_weight=None,
                  weighted_entry=None):
    """The dense evaluation pass of one family (``entry``: a
    ``*_loglik_batched_sum`` symbol, or with ``with_offset`` one that takes
    ``eta_offset`` after y; with ``sample_weight`` ``weighted_entry``, which
    takes the weights behind those) through ``_loglik_groups``."""
    _check_row_extras(X, with_offset, eta_offset, exposure, sample_weight)
    dev, Xd, yd, offs, cd, sd = _dense_inputs(X, y, offsets, center, scale, device)
    entry, extras = _entry_and_extras(entry, weighted_entry, with_offset, eta_offset, exposure,
                                      sample_weight, dev)
    p, K = Xd.shape[1], offs.size - 1
    fn = getattr(_hip.load(), entry)

    def call(bd, g, out, total):
        rc = fn(_ptr(Xd), _ptr(yd), *map(_ptr, extras), offs.ctypes.data_as(ctypes.c_void_p), K, p,
                int(bool(fit_intercept)), _ptr(cd), _ptr(sd), _ptr(bd), g, _ptr(out), _ptr(total),
                _stream(dev))
        _hip.check(rc, entry)

    return _loglik_groups(call, betas, p + (1 if fit_intercept else 0), K, dev, return_sum)


def logistic_loglik_batched(X, y, offsets, betas, fit_intercept=False, center=None, scale=None,
                            device=None, return_sum=False, sample_weight=None):
    """Per-partition log-likelihood of candidate coefficient vectors in one
    pass over X (the evaluation step of dlsa/models.py:151-225 /
    dlsa/model_eval.py:10-42).  betas: [B, P], intercept first; more than 16
    candidates are evaluated 16 to a pass.  Returns a [K, B] fp64 tensor on
    the device; with ``return_sum`` also its [B] sum over the partitions (the
    group-by sum of model_eval.py:38, fixed order, on the device).
    ``sample_weight`` [n] (None: exactly the unweighted call): every row's term
    is multiplied by its prior weight, the log-likelihood of the weighted fit
    (finite and >= 0, n entries, else ``ValueError``)."""
    return _loglik_dense("dlsa_logistic_loglik_batched_sum", X, y, offsets, betas, fit_intercept,
                         center, scale, device, return_sum, sample_weight=sample_weight,
                         weighted_entry="dlsa_logistic_loglik_batched_sum_weighted")


def poisson_loglik_batched(X, y, offsets, betas, fit_intercept=False, center=None, scale=None,
                           device=None, return_sum=False):
    """``logistic_loglik_batched`` for the Poisson family: per partition and
    candidate ``sum y eta - exp(eta) - lgamma(y + 1)`` with eta = x . beta
    (the log-likelihood ``poisson_model_batched`` returns).  Same arguments,
    limits (P <= 512, 16 candidates to a pass) and outputs."""
    return _loglik_dense("dlsa_poisson_loglik_batched_sum", X, y, offsets, betas, fit_intercept,
                         center, scale, device, return_sum)


def poisson_loglik_batched_offset(X, y, offsets, betas, eta_offset=None, exposure=None,
                                  fit_intercept=False, center=None, scale=None, device=None,
                                  return_sum=False):
    """``poisson_loglik_batched`` with the per-row offset of
    ``poisson_model_batched_offset``: eta = x . beta + eta_offset for every
    candidate (``eta_offset`` [n], or ``exposure`` [n] > 0 whose log is taken on
    the device; the same ``ValueError`` cases).  Neither given: exactly
    ``poisson_loglik_batched``."""
    return _loglik_dense("dlsa_poisson_loglik_batched_sum_offset", X, y, offsets, betas,
                         fit_intercept, center, scale, device, return_sum, with_offset=True,
                         eta_offset=eta_offset, exposure=exposure)


def poisson_loglik_batched_weighted(X, y, offsets, betas, sample_weight=None, eta_offset=None,
                                    exposure=None, fit_intercept=False, center=None, scale=None,
                                    device=None, return_sum=False):
    """``poisson_loglik_batched`` / ``poisson_loglik_batched_offset`` with the
    prior weights of ``poisson_model_batched_weighted``: every row's term, the
    constant -lgamma(y + 1) included, is multiplied by ``sample_weight`` [n]
    (finite and >= 0, else ``ValueError``; None: exactly the unweighted call)
    (``dlsa_poisson_loglik_batched_sum_weighted``)."""
    return _loglik_dense("dlsa_poisson_loglik_batched_sum_offset", X, y, offsets, betas,
                         fit_intercept, center, scale, device, return_sum, with_offset=True,
                         eta_offset=eta_offset, exposure=exposure, sample_weight=sample_weight,
                         weighted_entry="dlsa_poisson_loglik_batched_sum_weighted")


def logistic_loglik_batched_categorical(Xn, codes, y, offsets, levels, betas, fit_intercept=False,
                                        center=None, scale=None, rows_per_chunk=0, device=None,
                                        return_sum=False, sample_weight=None):
    """``logistic_loglik_batched`` on the categorical-code layout of
    ``logistic_model_batched_categorical`` (same Xn / codes / levels / center /
    scale and parameter order): the log-likelihood of the dummy-expanded design
    without building it -- 8 q + F + 8 bytes per row, the dummy coefficients a
    table in LDS (``dlsa_logistic_loglik_categorical``).  betas: [B, P]; more
    than 16 candidates are evaluated 16 to a pass.  Returns a [K, B] fp64
    device tensor, with ``return_sum`` also its [B] sum over the partitions.
    A code >= levels[f] raises ``DlsaHipError``.  ``sample_weight`` [n] (None:
    exactly the unweighted call): every row's term is multiplied by its prior
    weight (finite and >= 0, n entries, else ``ValueError``), the
    log-likelihood of ``logistic_model_batched_categorical_weighted``
    (``dlsa_logistic_loglik_categorical_weighted``)."""
    _check_row_extras(Xn, False, None, None, sample_weight)
    dev = _require_gpu(device)
    Xd, cd8, yd, offs, lv, cen, sca = _cat_inputs(Xn, codes, y, offsets, levels, center, scale,
                                                  dev)
    entry, extras = _entry_and_extras("dlsa_logistic_loglik_categorical",
                                      "dlsa_logistic_loglik_categorical_weighted", False, None,
                                      None, sample_weight, dev)
    return _cat_loglik(entry, extras, Xd, cd8, yd, offs, lv, cen, sca, betas, fit_intercept,
                       rows_per_chunk, dev, return_sum)


def _cat_loglik(entry, extras, Xd, cd8, yd, offs, lv, cen, sca, betas, fit_intercept,
                rows_per_chunk, dev, return_sum):
    """The evaluation pass on the categorical-code layout (``entry`` takes
    ``extras`` between y and offsets) through ``_loglik_groups``."""
    q, F, K = Xd.shape[1], cd8.shape[1], offs.size - 1
    fn = getattr(_hip.load(), entry)

    def call(bd, g, out, total):
        rc = fn(_ptr(Xd), _ptr(cd8), _ptr(yd), *map(_ptr, extras),
                offs.ctypes.data_as(ctypes.c_void_p), K, q, F,
                lv.ctypes.data_as(ctypes.c_void_p), int(bool(fit_intercept)), _ptr(cen), _ptr(sca),
                _ptr(bd), g, int(rows_per_chunk), _ptr(out), _ptr(total), _stream(dev))
        _hip.check(rc, entry)

    P = int(bool(fit_intercept)) + q + int((lv - 1).sum())
    return _loglik_groups(call, betas, P, K, dev, return_sum)


def poisson_loglik_batched_categorical(Xn, codes, y, offsets, levels, betas, sample_weight=None,
                                       eta_offset=None, exposure=None, fit_intercept=False,
                                       center=None, scale=None, rows_per_chunk=0, device=None,
                                       return_sum=False):
    """``logistic_loglik_batched_categorical`` for the Poisson family, the
    log-likelihood ``poisson_model_batched_categorical`` returns: per partition
    and candidate ``sum omega (y eta - exp(eta) - lgamma(y + 1))`` with eta =
    x . beta + eta_offset on the dummy-expanded design, without building it.
    ``sample_weight``, ``eta_offset`` / ``exposure`` as there
    (``dlsa_poisson_loglik_categorical``)."""
    dev, extras = _pois_cat_extras("dlsa_poisson_loglik_categorical", Xn, eta_offset, exposure,
                                   sample_weight, device)
    Xd, cd8, yd, offs, lv, cen, sca = _cat_inputs(Xn, codes, y, offsets, levels, center, scale,
                                                  dev)
    return _cat_loglik("dlsa_poisson_loglik_categorical", extras, Xd, cd8, yd, offs, lv, cen, sca,
                       betas, fit_intercept, rows_per_chunk, dev, return_sum)


# ---------------------------------------------------------------------------
# goodness of fit: deviance, Pearson chi-square, rows with a positive weight
# ---------------------------------------------------------------------------

MAX_GOF_CANDIDATES = _hip.MAX_GOF_CANDIDATES  # candidates of one goodness-of-fit pass
_GOF_FAMILIES = {"logistic": _hip.FAMILY_LOGISTIC, "poisson": _hip.FAMILY_POISSON}


def _check_gof_args(family, X, betas, thetas, eta_offset, exposure, sample_weight):
    """The argument checks of a goodness-of-fit call that need no GPU; returns
    the family's code."""
    if family not in _GOF_FAMILIES:
        raise ValueError(f"family must be 'logistic' or 'poisson', not {family!r}")
    if (betas is None) == (thetas is None):
        raise ValueError("give exactly one of betas [B, P] (the same candidates for every "
                         "partition) and thetas [K, P] (each partition at its own row)")
    if len(_shape(X)) != 2:
        raise ValueError("X must be 2-D [n, p]")
    if family != "poisson" and (eta_offset is not None or exposure is not None):
        raise ValueError("eta_offset / exposure need family='poisson'")
    _check_row_extras(X, family == "poisson", eta_offset, exposure, sample_weight)
    return _GOF_FAMILIES[family]


def _gof_groups(call, betas, thetas, P, K, dev, return_sum):
    """Run ``call(coef, g, stride, deviance [K, g], pearson [K, g], n_pos [K],
    sums [2g + 1])`` and assemble the result dict.  ``betas`` [B, P]: in
    groups of at most ``MAX_GOF_CANDIDATES`` (one pass over the data each,
    stride 0).  ``thetas`` [K, P]: one pass, B = 1, partition k at row k."""
    f64 = dict(dtype=torch.float64, device=dev)
    cd = _dev_f64(betas if thetas is None else thetas, dev)
    if cd.dim() == 1:
        cd = cd.reshape(1, -1)
    if thetas is not None:
        if cd.dim() != 2 or tuple(cd.shape) != (K, P):
            raise ValueError("thetas must be [K, P]: one row per partition")
        B = 1
    elif cd.dim() != 2 or cd.shape[0] < 1 or cd.shape[1] != P:
        raise ValueError("betas must be [B, P] with B >= 1 and P = the design's parameters")
    else:
        B = cd.shape[0]
    dv, ch = torch.empty((K, B), **f64), torch.empty((K, B), **f64)
    npos = torch.empty((K,), **f64)
    tot = torch.empty((2, B), **f64)
    for b0 in range(0, B, MAX_GOF_CANDIDATES):
        g = min(MAX_GOF_CANDIDATES, B - b0)
        whole = g == B
        d, c = (dv, ch) if whole else (torch.empty((K, g), **f64), torch.empty((K, g), **f64))
        sums = torch.empty((2 * g + 1,), **f64)
        coef = cd.contiguous() if thetas is not None else cd[b0:b0 + g].contiguous()
        call(coef, g, P if thetas is not None else 0, d, c, npos, sums)
        if not whole:
            dv[:, b0:b0 + g], ch[:, b0:b0 + g] = d, c
        tot[0, b0:b0 + g], tot[1, b0:b0 + g] = sums[:g], sums[g:2 * g]
    out = {"deviance": dv, "pearson": ch, "n_pos": npos.to(torch.int64)}
    if return_sum:
        out.update(deviance_sum=tot[0], pearson_sum=tot[1], n_pos_sum=sums[-1].to(torch.int64))
    return out


def glm_gof_batched(family, X, y, offsets, betas=None, thetas=None, eta_offset=None,
                    exposure=None, sample_weight=None, fit_intercept=False, center=None,
                    scale=None, device=None, return_sum=False):
    """Goodness of fit of a GLM in one more pass over X (the bytes per row of
    ``*_loglik_batched``): per partition and candidate the residual deviance
    and the Pearson chi-square, per partition the rows with a positive weight
    (``dlsa_glm_gof_batched``).  ``family``: "logistic" or "poisson".

    Exactly one of ``betas`` [B, P] (every partition at the same candidates:
    the job-level deviance of the combined or selected estimates; more than
    ``MAX_GOF_CANDIDATES`` are evaluated in groups) and ``thetas`` [K, P]
    (partition k at its own row, "at the fit's own theta_k", B = 1: what the
    degrees of freedom of the dispersion estimate chi^2 / (n - P) assume).
    ``eta_offset`` / ``exposure`` (Poisson only) and ``sample_weight`` as in
    the fits, with their ``ValueError`` cases.  The logistic y is taken as
    given in [0, 1], so grouped rows y = s / m with weight m work; it is not
    checked, and outside [0, 1] the sums are NaN.

    At saturated linear predictors every row term takes its limit instead of
    0 / 0: a logistic row on its own side (y = 1 at eta >= 0, y = 0 below) has
    the Pearson term omega exp(-|eta|), 0 once that has underflowed (|eta| >
    745.13), so a separated or steep fit keeps a finite ``pearson`` and
    dispersion; a row on the wrong side grows like exp(|eta|) and is +inf from
    there.  Poisson: y = 0 gives omega mu (0 for a dead row, e.g. an offset of
    -800), y > 0 over an underflowed mu +inf, and an overflowed mu (eta >
    709.78) +inf in both sums.  With y in [0, 1] (y >= 0) and positive weights
    no sum is NaN.

    Returns a dict of device tensors: ``deviance`` [K, B], ``pearson`` [K, B]
    (fp64), ``n_pos`` [K] (int64); with ``return_sum`` also their sums over the
    partitions, ``deviance_sum`` [B], ``pearson_sum`` [B], ``n_pos_sum``.
    Fixed summation order: two calls give the same bits."""
    fam = _check_gof_args(family, X, betas, thetas, eta_offset, exposure, sample_weight)
    dev, Xd, yd, offs, cd, sd = _dense_inputs(X, y, offsets, center, scale, device)
    od, wd = _gof_extras(family, eta_offset, exposure, sample_weight, dev)
    p, K = Xd.shape[1], offs.size - 1
    fn = _hip.load().dlsa_glm_gof_batched

    def call(coef, g, stride, d, c, npos, sums):
        rc = fn(fam, _ptr(Xd), _ptr(yd), _ptr(od), _ptr(wd), offs.ctypes.data_as(ctypes.c_void_p),
                K, p, int(bool(fit_intercept)), _ptr(cd), _ptr(sd), _ptr(coef), g, stride,
                _ptr(d), _ptr(c), _ptr(npos), _ptr(sums), _stream(dev))
        _hip.check(rc, "dlsa_glm_gof_batched")

    return _gof_groups(call, betas, thetas, p + (1 if fit_intercept else 0), K, dev, return_sum)


def _gof_extras(family, eta_offset, exposure, sample_weight, dev):
    """The device offset and weight of a goodness-of-fit call (None: a null
    pointer)."""
    _, extras = _entry_and_extras(None, None, family == "poisson", eta_offset, exposure,
                                  sample_weight, dev)
    od = extras[0] if family == "poisson" else None
    wd = extras[-1] if sample_weight is not None else None
    return od, wd


def glm_gof_batched_categorical(family, Xn, codes, y, offsets, levels, betas=None, thetas=None,
                                eta_offset=None, exposure=None, sample_weight=None,
                                fit_intercept=False, center=None, scale=None, rows_per_chunk=0,
                                device=None, return_sum=False):
    """``glm_gof_batched`` on the categorical-code layout of
    ``logistic_model_batched_categorical`` (same Xn / codes / levels / center /
    scale and parameter order): the deviance and Pearson chi-square of the
    dummy-expanded design without building it, the dummy coefficients a table
    in LDS (``dlsa_glm_gof_categorical``).  A code >= levels[f] raises
    ``DlsaHipError``."""
    fam = _check_gof_args(family, Xn, betas, thetas, eta_offset, exposure, sample_weight)
    dev = _require_gpu(device)
    Xd, cd8, yd, offs, lv, cen, sca = _cat_inputs(Xn, codes, y, offsets, levels, center, scale,
                                                  dev)
    od, wd = _gof_extras(family, eta_offset, exposure, sample_weight, dev)
    q, F, K = Xd.shape[1], cd8.shape[1], offs.size - 1
    fn = _hip.load().dlsa_glm_gof_categorical

    def call(coef, g, stride, d, c, npos, sums):
        rc = fn(fam, _ptr(Xd), _ptr(cd8), _ptr(yd), _ptr(od), _ptr(wd),
                offs.ctypes.data_as(ctypes.c_void_p), K, q, F, lv.ctypes.data_as(ctypes.c_void_p),
                int(bool(fit_intercept)), _ptr(cen), _ptr(sca), _ptr(coef), g, stride,
                int(rows_per_chunk), _ptr(d), _ptr(c), _ptr(npos), _ptr(sums), _stream(dev))
        _hip.check(rc, "dlsa_glm_gof_categorical")

    P = int(bool(fit_intercept)) + q + int((lv - 1).sum())
    return _gof_groups(call, betas, thetas, P, K, dev, return_sum)


_GRAM_KINDS = {"score": _hip.GRAM_SCORE, "information": _hip.GRAM_INFORMATION}


def glm_gram_batched(family, X, y, offsets, thetas=None, beta=None, kind="score",
                     eta_offset=None, exposure=None, sample_weight=None, fit_intercept=False,
                     center=None, scale=None, return_sum=False, rows_per_chunk=0, device=None):
    """Score outer products of a GLM in one more pass over X (8 (p + 1) bytes
    per row plus 8 per row extra; ``dlsa_glm_gram_batched``, fp64 MFMA): per
    partition k at its coefficient vector, with s_i = omega_i (y_i - mu_i),

    * ``gram`` [K, P, P] = sum_i d_i x_i x_i^T, exactly symmetric, and
    * ``score`` [K, P] = sum_i s_i x_i (zero at a converged fit's own theta).

    ``kind`` = "score": d = s^2, the meat M_k of the sandwich (Huber-White,
    HC0) covariance; omega enters squared, the precision / survey-weight
    convention of R's ``sandwich::estfun`` -- frequency weights are not
    replicated rows here.  ``kind`` = "information": d = omega w (w = mu (1 -
    mu) or mu), the information matrix, a fit's ``sig_inv``, at any beta.

    Exactly one of ``thetas`` [K, P] (partition k at its own row) and ``beta``
    [P] (every partition at the same vector, e.g. the WLSE).  ``family``:
    "logistic" or "poisson"; ``eta_offset`` / ``exposure`` (Poisson only) and
    ``sample_weight`` as in the fits, with their ``ValueError`` cases; P =
    p + intercept <= 192 (a wider one raises ``DlsaHipError``).  ``rows_per_chunk``: 0 (automatic) or the rows one
    workgroup sums; the sums' last bits depend on it.

    Returns a dict of device tensors ``gram``, ``score``; with ``return_sum``
    also ``gram_sum`` [P, P] and ``score_sum`` [P], the sums over k ascending.
    Fixed summation order: two calls give the same bits."""
    if kind not in _GRAM_KINDS:
        raise ValueError(f"kind must be 'score' or 'information', not {kind!r}")
    if (beta is None) == (thetas is None):
        raise ValueError("give exactly one of thetas [K, P] (each partition at its own row) and "
                         "beta [P] (every partition at the same vector)")
    fam = _check_gof_args(family, X, beta, thetas, eta_offset, exposure, sample_weight)
    if int(rows_per_chunk) < 0:
        raise ValueError("rows_per_chunk must be >= 0")
    p = _shape(X)[1]
    P = p + (1 if fit_intercept else 0)
    K = _size(offsets) - 1
    coef = thetas if beta is None else beta
    if beta is not None and _size(coef) != P:
        raise ValueError("beta must be [P]: one coefficient vector for every partition")
    if thetas is not None and (_size(coef) != K * P or
                               (len(_shape(coef)) == 2 and _shape(coef) != (K, P))):
        raise ValueError("thetas must be [K, P]: one row per partition")
    dev, Xd, yd, offs, cd, sd = _dense_inputs(X, y, offsets, center, scale, device)
    od, wd = _gof_extras(family, eta_offset, exposure, sample_weight, dev)
    bd = _dev_f64(coef, dev).reshape(-1)
    f64 = dict(dtype=torch.float64, device=dev)
    gram, score = torch.empty((K, P, P), **f64), torch.empty((K, P), **f64)
    gsum = torch.empty((P, P), **f64) if return_sum else None
    ssum = torch.empty((P,), **f64) if return_sum else None
    rc = _hip.load().dlsa_glm_gram_batched_chunked(
        fam, _GRAM_KINDS[kind], _ptr(Xd), _ptr(yd), _ptr(od), _ptr(wd),
        offs.ctypes.data_as(ctypes.c_void_p), K, p, int(bool(fit_intercept)), _ptr(cd), _ptr(sd),
        _ptr(bd), P if thetas is not None else 0, int(rows_per_chunk), _ptr(gram), _ptr(score),
        _ptr(gsum), _ptr(ssum), _stream(dev))
    _hip.check(rc, "dlsa_glm_gram_batched")
    out = {"gram": gram, "score": score}
    if return_sum:
        out.update(gram_sum=gsum, score_sum=ssum)
    return out


def glm_gram_batched_categorical(family, Xn, codes, y, offsets, levels, thetas=None, beta=None,
                                 kind="score", eta_offset=None, exposure=None,
                                 sample_weight=None, fit_intercept=False, center=None,
                                 scale=None, return_sum=False, rows_per_chunk=0, device=None):
    """``glm_gram_batched`` on the categorical-code layout of
    ``logistic_model_batched_categorical`` (same Xn / codes / levels / center /
    scale and parameter order): the meat or the information matrix and the
    score of the dummy-expanded design without building it
    (``dlsa_glm_gram_categorical``), at 8 q + F + 8 bytes per row, streamed
    twice, instead of 8 P.  The arguments, their ``ValueError`` cases and the
    returned dict are ``glm_gram_batched``'s; the limits are the categorical
    fit's (P <= 192, intercept + q <= 16, F <= 16, histograms that fit the
    LDS), and a code >= levels[f] raises ``DlsaHipError``.

    The one-hot blocks are fixed-point histogram sums on grids measured from
    the rows' own terms at the given coefficients: an entry of a dummy row or
    column of partition k is within n_k R 2^-60 B of the fp64-exact sum (R the
    rows of the largest chunk, at least 1024; B the partition's largest |d|,
    |s| or |d x_j|), the numeric block is summed in fp64, and two calls give
    the same bits.  A partition with a term that is not finite (a NaN weight or
    offset) gets an all-NaN ``gram`` and ``score``; no other partition is
    touched."""
    if kind not in _GRAM_KINDS:
        raise ValueError(f"kind must be 'score' or 'information', not {kind!r}")
    if (beta is None) == (thetas is None):
        raise ValueError("give exactly one of thetas [K, P] (each partition at its own row) and "
                         "beta [P] (every partition at the same vector)")
    fam = _check_gof_args(family, Xn, beta, thetas, eta_offset, exposure, sample_weight)
    if int(rows_per_chunk) < 0:
        raise ValueError("rows_per_chunk must be >= 0")
    q = _shape(Xn)[1]
    lv = np.asarray(levels, dtype=np.int64).reshape(-1)
    if len(_shape(codes)) != 2 or _shape(codes)[0] != _shape(Xn)[0]:
        raise ValueError("codes must be [n, F]")
    if lv.size != _shape(codes)[1]:
        raise ValueError("levels must have F entries")
    P = (1 if fit_intercept else 0) + q + int((lv - 1).sum())
    K = _size(offsets) - 1
    coef = thetas if beta is None else beta
    if beta is not None and _size(coef) != P:
        raise ValueError("beta must be [P]: one coefficient vector for every partition")
    if thetas is not None and (_size(coef) != K * P or
                               (len(_shape(coef)) == 2 and _shape(coef) != (K, P))):
        raise ValueError("thetas must be [K, P]: one row per partition")
    _check_rows(offsets, _shape(Xn)[0], y)
    _center_scale(center, scale, q, "q (the numeric columns)")
    dev = _require_gpu(device)
    Xd, cd8, yd, offs, lv, cen, sca = _cat_inputs(Xn, codes, y, offsets, levels, center, scale,
                                                  dev)
    od, wd = _gof_extras(family, eta_offset, exposure, sample_weight, dev)
    bd = _dev_f64(coef, dev).reshape(-1)
    F = cd8.shape[1]
    f64 = dict(dtype=torch.float64, device=dev)
    gram, score = torch.empty((K, P, P), **f64), torch.empty((K, P), **f64)
    gsum = torch.empty((P, P), **f64) if return_sum else None
    ssum = torch.empty((P,), **f64) if return_sum else None
    rc = _hip.load().dlsa_glm_gram_categorical(
        fam, _GRAM_KINDS[kind], _ptr(Xd), _ptr(cd8), _ptr(yd), _ptr(od), _ptr(wd),
        offs.ctypes.data_as(ctypes.c_void_p), K, q, F, lv.ctypes.data_as(ctypes.c_void_p),
        int(bool(fit_intercept)), _ptr(cen), _ptr(sca), _ptr(bd),
        P if thetas is not None else 0, int(rows_per_chunk), _ptr(gram), _ptr(score), _ptr(gsum),
        _ptr(ssum), _stream(dev))
    _hip.check(rc, "dlsa_glm_gram_categorical")
    out = {"gram": gram, "score": score}
    if return_sum:
        out.update(gram_sum=gsum, score_sum=ssum)
    return out


_ROWS_STREAMS = ("eta", "mu", "dev_res", "pearson_res", "leverage")  # the C entry's order
_ROWS_OUTPUTS = _ROWS_STREAMS + ("cooks",)


def rows_factor(info, K, P):
    """The factors R_k of the leverage pass from information matrices, on the
    host (batched numpy): ``info`` [K, P, P] or [P, P] (symmetric; the lower
    triangle is used), S_k = L L^T, R_k = L^-1, so that R_k^T R_k = S_k^-1 and
    x^T S_k^-1 x = |R_k x|^2.  Returns [K, P, P] or [P, P], lower triangular
    with an exactly zero upper triangle.  A matrix that is not finite or not
    positive definite (an empty or failed partition's zeros) gives a NaN
    factor: its partition's leverages are NaN, the others untouched."""
    S = np.array(info, dtype=np.float64)
    shared = S.ndim == 2
    S = S.reshape(-1, P, P)
    R = np.full_like(S, np.nan)
    idx = np.flatnonzero(np.isfinite(S).all(axis=(1, 2)))
    try:  # all at once; one by one only when some matrix is not positive definite
        Ls = dict(zip(idx, np.linalg.cholesky(S[idx]))) if idx.size else {}
    except np.linalg.LinAlgError:
        Ls = {}
        for k in idx:
            try:
                Ls[k] = np.linalg.cholesky(S[k])
            except np.linalg.LinAlgError:
                pass
    # a pivot at rounding level: a rank-deficient matrix that rounding let through
    tiny = P * np.finfo(np.float64).eps
    idx = np.array([k for k, L in Ls.items()
                    if np.min(np.diag(L)) ** 2 > tiny * np.max(np.diag(S[k]))], dtype=np.int64)
    if idx.size:
        Rs = np.tril(np.linalg.solve(np.stack([Ls[k] for k in idx]), np.eye(P)))
        fin = np.isfinite(Rs).all(axis=(1, 2))
        R[idx[fin]] = Rs[fin]
    return R[0] if shared else R


def glm_rows_batched(family, X, y, offsets, thetas=None, beta=None, info=None, outputs=None,
                     eta_offset=None, exposure=None, sample_weight=None, fit_intercept=False,
                     center=None, scale=None, rows_per_chunk=0, device=None):
    """Per-row diagnostics of a GLM in one more pass over X (8 (p + 1) bytes
    per row plus 8 per row extra read, 8 per output written;
    ``dlsa_glm_rows_batched``, fp64 MFMA): what R's ``predict``, ``residuals``,
    ``hatvalues`` and ``cooks.distance`` return, for the rows that were fitted.
    A dict of [n] device tensors out of

    * ``eta`` (the linear predictor, offset included) and ``mu``;
    * ``dev_res``, ``pearson_res``: the signed deviance and Pearson residuals,
      the square roots of ``glm_gof_batched``'s row terms (omega included)
      with the sign of y - mu;
    * ``leverage`` h_i = omega_i w_i x_i^T S_k^-1 x_i and ``cooks`` =
      pearson_res^2 h / (P (1 - h)^2) -- only with ``info``, the information
      matrix S_k the leverage is taken against: [K, P, P] (each partition
      against its own, e.g. ``fit.sig_inv``: the local leverage of DLSA) or
      [P, P] (one for all).  It is factored on the host (``rows_factor``); a
      partition whose matrix is not finite or not positive definite gets NaN
      leverages, the others are untouched.

    ``outputs``: the names wanted (None: all that ``info`` allows).  Exactly one
    of ``thetas`` [K, P] and ``beta`` [P]; ``family``, ``eta_offset`` /
    ``exposure``, ``sample_weight``, ``center`` / ``scale``, the limit P <= 192
    and the ``ValueError`` cases as in ``glm_gram_batched``.  Every value of a
    row depends on that row, its partition's coefficients and factor alone:
    the bits are the same from call to call and for every ``rows_per_chunk``."""
    if (beta is None) == (thetas is None):
        raise ValueError("give exactly one of thetas [K, P] (each partition at its own row) and "
                         "beta [P] (every partition at the same vector)")
    fam = _check_gof_args(family, X, beta, thetas, eta_offset, exposure, sample_weight)
    if int(rows_per_chunk) < 0:
        raise ValueError("rows_per_chunk must be >= 0")
    if outputs is None:
        outputs = _ROWS_OUTPUTS if info is not None else _ROWS_STREAMS[:4]
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    unknown = [o for o in outputs if o not in _ROWS_OUTPUTS]
    if unknown or not outputs:
        raise ValueError(f"outputs must be names out of {_ROWS_OUTPUTS}, not {unknown}")
    if info is None and ("leverage" in outputs or "cooks" in outputs):
        raise ValueError("leverage and cooks need info, the information matrix they are taken "
                         "against ([K, P, P] or [P, P], e.g. fit.sig_inv)")
    n, p = _shape(X)
    P = p + (1 if fit_intercept else 0)
    K = _size(offsets) - 1
    coef = thetas if beta is None else beta
    if beta is not None and _size(coef) != P:
        raise ValueError("beta must be [P]: one coefficient vector for every partition")
    if thetas is not None and (_size(coef) != K * P or
                               (len(_shape(coef)) == 2 and _shape(coef) != (K, P))):
        raise ValueError("thetas must be [K, P]: one row per partition")
    if info is not None and _shape(info) not in ((K, P, P), (P, P)):
        raise ValueError("info must be [K, P, P] (one information matrix per partition) or [P, P]")
    dev, Xd, yd, offs, cd, sd = _dense_inputs(X, y, offsets, center, scale, device)
    od, wd = _gof_extras(family, eta_offset, exposure, sample_weight, dev)
    bd = _dev_f64(coef, dev).reshape(-1)
    want = set(outputs)
    if "cooks" in want:
        want |= {"pearson_res", "leverage"}
    rd, rstride = None, 0
    if "leverage" in want:
        host = info.detach().cpu().numpy() if isinstance(info, torch.Tensor) else info
        R = rows_factor(host, K, P)
        rstride = P * P if R.ndim == 3 else 0
        rd = _dev_f64(R, dev).reshape(-1)
    f64 = dict(dtype=torch.float64, device=dev)
    bufs = {name: (torch.empty((n,), **f64) if name in want else None) for name in _ROWS_STREAMS}
    rc = _hip.load().dlsa_glm_rows_batched_chunked(
        fam, _ptr(Xd), _ptr(yd), _ptr(od), _ptr(wd), offs.ctypes.data_as(ctypes.c_void_p), K, p,
        int(bool(fit_intercept)), _ptr(cd), _ptr(sd), _ptr(bd), P if thetas is not None else 0,
        _ptr(rd), rstride, int(rows_per_chunk), *[_ptr(bufs[name]) for name in _ROWS_STREAMS],
        _stream(dev))
    _hip.check(rc, "dlsa_glm_rows_batched")
    if "cooks" in want:
        h, r = bufs["leverage"], bufs["pearson_res"]
        bufs["cooks"] = r * r * h / (P * (1.0 - h) ** 2)
    return {name: bufs[name] for name in outputs}


# ---------------------------------------------------------------------------
# reference-signature wrapper (one Spark group)
# ---------------------------------------------------------------------------


def _describe_row(data_info, col, row):
    # Spark DataFrame.describe().toPandas(): rows count/mean/stddev/min/max,
    # values as strings (models.py:99-101 reads rows 1 and 2)
    return float(data_info[col][row])


def _center_scale_from_info(data_info, cols, numeric):
    """center / scale [len(cols)] of models.py:99-101: the mean and stddev of
    ``data_info`` on the numeric columns, 0 and 1 on the others; (None, None)
    without ``data_info`` or columns."""
    if len(data_info) == 0 or len(cols) == 0:
        return None, None
    center = np.zeros(len(cols))
    scale = np.ones(len(cols))
    for j, c in enumerate(cols):
        if c in numeric:
            center[j] = _describe_row(data_info, c, 1)
            scale[j] = _describe_row(data_info, c, 2)
    return center, scale


def _result_frame(icpt, cols, fit=None):
    """The reference's output frame ``par_id | coef | Sig_invMcoef | <Sig_inv
    columns>`` of partition 0 of ``fit``; without one its all-zero frame
    (models.py:84-91)."""
    import pandas as pd

    names = ["coef", "Sig_invMcoef"] + icpt + cols
    P = len(icpt) + len(cols)
    if fit is None:
        return pd.DataFrame(0, index=np.arange(P), columns=["par_id"] + names)
    out = pd.DataFrame(np.column_stack([fit.theta[0].cpu().numpy(),
                                        fit.sig_inv_theta[0].cpu().numpy(),
                                        fit.sig_inv[0].cpu().numpy()]), columns=pd.Index(names))
    out.insert(0, "par_id", np.arange(P))
    if out.isna().values.any():
        warnings.warn("NAs appear in the final output")
    return out


def _design(sample_df, Y_name, dummy_info, dummy_factors_baseline):
    """Host-side design matrix of one partition, models.py:56-104.  Returns
    (x_train DataFrame, usecols_x0 numeric columns, usecols_x all columns,
    zero_frame_or_None)."""
    import pandas as pd

    if len(dummy_info) > 0:
        factors = list(dummy_info["factor_selected"].keys())
        dropped = {k: v for k, v in dummy_info["factor_dropped"].items() if len(v) > 0}
        df = sample_df.replace(dropped, "000_OTHERS")
        wide = pd.get_dummies(data=df, drop_first=False, columns=factors, sparse=True)
        x_train = wide.drop(["partition_id", Y_name] + list(dummy_factors_baseline), axis=1)
        numeric = sorted(set(df.columns.drop(["partition_id", Y_name])) - set(factors))
        cols = list(numeric)
        for f in factors:
            cols.extend(sorted(dummy_info["factor_selected_names"][f]))
        cols = [c for c in cols if c not in dummy_factors_baseline]
        if set(x_train.columns) != set(cols):
            return x_train, numeric, cols, True
        return x_train, numeric, cols, False
    x_train = sample_df.drop(["partition_id", Y_name] + list(dummy_factors_baseline), axis=1)
    return x_train, list(x_train.columns), list(x_train.columns), False


def _logistic_model_codes(sample_df, Y_name, fit_intercept, dummy_info, dummy_factors_baseline,
                          data_info):
    """Dummy branch of logistic_model on the categorical-code layout (no dense
    dummy matrix).  None when the design exceeds the kernel's limits (F <= 16
    factors, intercept + numeric <= 16, P <= 192): the caller then builds the
    dense design."""
    icpt = ["intercept"] if fit_intercept else []
    enc = encode_categorical(sample_df, Y_name, dummy_info, dummy_factors_baseline)
    q, F = enc["Xn"].shape[1], enc["codes"].shape[1]
    P = len(icpt) + len(enc["cols"])
    if F > 16 or len(icpt) + q > 16 or P > _hip.MAX_P_FUSED:
        return None
    cols = enc["cols"]
    if enc["unknown"] or (enc["counts"] == 0).any():
        absent = [c for c, m in zip(cols[q:], enc["counts"]) if m == 0]
        warnings.warn("Dummies:" + str(set(absent)) + "missing in this data chunk "
                      + str((len(sample_df), len(cols))) + "Skip modeling this part of data.")
        return _result_frame(icpt, cols)
    center, scale = _center_scale_from_info(data_info, enc["numeric"], enc["numeric"])
    y = np.asarray(sample_df[Y_name], dtype=np.float64)
    fit = logistic_model_batched_categorical(enc["Xn"], enc["codes"], y, np.array([0, y.size]),
                                             enc["levels"], fit_intercept=fit_intercept,
                                             center=center, scale=scale)
    return _result_frame(icpt, cols, fit)


def logistic_model(sample_df, Y_name, fit_intercept=False, dummy_info=[], dummy_factors_baseline=[],
                   data_info=[]):
    """Run the logistic model on one partition (dlsa/models.py:42-147).

    Same inputs and the same p x (p+3) output frame as the reference:
    ``par_id | coef | Sig_invMcoef | <Sig_inv columns>``, intercept first.
    A partition that lacks a selected dummy level returns the reference's
    all-zero frame (models.py:84-91).  The estimate is the converged MLE (the
    reference stops sklearn at its default tol=1e-4); the fit runs on the GPU.
    """
    icpt = ["intercept"] if fit_intercept else []
    if len(dummy_info) > 0:
        out = _logistic_model_codes(sample_df, Y_name, fit_intercept, dummy_info,
                                    dummy_factors_baseline, data_info)
        if out is not None:
            return out
    x_train, numeric, cols, missing = _design(sample_df, Y_name, dummy_info, dummy_factors_baseline)
    if missing:
        warnings.warn("Dummies:" + str(set(cols) - set(x_train.columns))
                      + "missing in this data chunk " + str(x_train.shape)
                      + "Skip modeling this part of data.")
        return _result_frame(icpt, cols)
    x_train = x_train.reindex(columns=cols)
    X = np.ascontiguousarray(x_train.to_numpy(dtype=np.float64))
    y = np.asarray(sample_df[Y_name], dtype=np.float64)
    center, scale = _center_scale_from_info(data_info, cols, numeric)
    fit = logistic_model_batched(X, y, np.array([0, X.shape[0]]), fit_intercept=fit_intercept,
                                 center=center, scale=scale)
    return _result_frame(icpt, cols, fit)


def logistic_model_eval(sample_df, Y_name, par, fit_intercept=False, dummy_info=[],
                        dummy_factors_baseline=[], data_info=[]):
    """Log-likelihood of each coefficient column of ``par`` on one partition
    (dlsa/models.py:151-225).  ``par`` is a P-row DataFrame (one column per
    method, e.g. beta_byAIC / beta_byBIC / beta_byOLS / beta_byONESHOT).
    Returns a one-row DataFrame with the same columns.  A partition missing a
    dummy level is evaluated with that dummy column set to 0, as the
    reference does (models.py:185-193).  The pass runs on the GPU; with
    ``dummy_info`` on the categorical-code layout (no dense dummy matrix)
    while the design is within that kernel's limits."""
    import pandas as pd

    betas = np.ascontiguousarray(np.asarray(par, dtype=np.float64).T)
    base = set(dummy_factors_baseline)
    # uint8 codes: at most 255 dummy columns per factor, else the dense design
    if len(dummy_info) > 0 and all(sum(c not in base for c in names) <= 255
                                   for names in dummy_info["factor_selected_names"].values()):
        enc = encode_categorical(sample_df, Y_name, dummy_info, dummy_factors_baseline)
        q, F = enc["Xn"].shape[1], enc["codes"].shape[1]
        P = int(bool(fit_intercept)) + len(enc["cols"])
        if F <= 16 and int(bool(fit_intercept)) + q <= 16 and P <= _hip.MAX_P:
            if enc["unknown"] or (enc["counts"] == 0).any():
                absent = [c for c, m in zip(enc["cols"][q:], enc["counts"]) if m == 0]
                warnings.warn("Dummies:" + str(set(absent)) + "missing in this data chunk "
                              + str((len(sample_df), len(enc["cols"]))))
            center, scale = _center_scale_from_info(data_info, enc["numeric"], enc["numeric"])
            y = np.asarray(sample_df[Y_name], dtype=np.float64)
            ll = logistic_loglik_batched_categorical(
                enc["Xn"], enc["codes"], y, np.array([0, y.size]), enc["levels"], betas,
                fit_intercept=fit_intercept, center=center, scale=scale)
            return pd.DataFrame(ll.cpu().numpy(), columns=list(par.columns))
    x_train, numeric, cols, missing = _design(sample_df, Y_name, dummy_info, dummy_factors_baseline)
    if missing:
        warnings.warn("Dummies:" + str(set(cols) - set(x_train.columns))
                      + "missing in this data chunk " + str(x_train.shape))
    x_train = x_train.reindex(columns=cols, fill_value=0)
    X = np.ascontiguousarray(x_train.to_numpy(dtype=np.float64))
    y = np.asarray(sample_df[Y_name], dtype=np.float64)
    center, scale = _center_scale_from_info(data_info, cols, numeric)
    ll = logistic_loglik_batched(X, y, np.array([0, X.shape[0]]), betas,
                                 fit_intercept=fit_intercept, center=center, scale=scale)
    return pd.DataFrame(ll.cpu().numpy(), columns=list(par.columns))
