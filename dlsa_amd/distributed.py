"""Multi-GPU DLSA: partitions sharded over ranks, one collective.

The reference's only exchange is the Spark shuffle + collect of every
partition's p x (p+3) frame to the driver (dlsa/dlsa.py:30-34; K*p*(p+3)
doubles over the network).  Here each rank (one process per GPU) fits its own
partitions in HBM, pre-reduces them on the device into
``[sum Sig_inv | sum Sig_inv theta | sum theta | K]`` (P^2 + 2P + 1 fp64,
81.6 KB at P = 100) and ONE ``all_reduce(SUM)`` over RCCL/xGMI combines the
ranks.  Every rank then holds the global sums and can solve the WLSE and run
the LARS/DBIC path locally (dlsa/dlsa.py:44-52, :70-100).  The global row
count N (for the DBIC) rides in the same buffer: one collective in all.
"""

from __future__ import annotations

import numpy as np

from .dlsa import reduce_partitions_device, split_reduced


def combine(buf, group=None):
    """Sum the per-rank reduced buffers in place (RCCL when the process group
    backend is "nccl", gloo on CPU tensors).  No-op without a process group;
    with one (even of one rank) the all-reduce runs, so a single-GPU job under
    ``torch.distributed`` takes the same collective path as the 8-GPU one."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        if buf.is_cuda and dist.get_backend(group) == "gloo":
            # gloo (CPU test / fallback transport): reduce a host copy
            tmp = buf.cpu()
            dist.all_reduce(tmp, op=dist.ReduceOp.SUM, group=group)
            buf.copy_(tmp)
        else:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf


def finish(S, v, sum_theta, K, n_global, fit_intercept=False, lars_type="lasso"):
    """Host tail of DLSA from the global sums: WLSE (lstsq as dlsa.py:48),
    ONESHOT (dlsa.py:51-52), LSA path and the AIC/BIC argmin (dlsa.py:83-98).
    """
    from .lsa import lars_lsa

    wlse = np.linalg.lstsq(S, v, rcond=None)[0]
    oneshot = sum_theta / K
    path = lars_lsa(S, wlse, intercept=fit_intercept, n=n_global, type=lars_type)
    ia = int(np.argmin(path["AIC"]))
    ib = int(np.argmin(path["BIC"]))
    if fit_intercept:
        b0 = path["beta0"] + wlse[0]
        b_aic = np.hstack([b0[ia], path["beta"][ia]])
        b_bic = np.hstack([b0[ib], path["beta"][ib]])
        support = np.nonzero(path["beta"][ib])[0] + 1
    else:
        b_aic = path["beta"][ia].copy()
        b_bic = path["beta"][ib].copy()
        support = np.nonzero(b_bic)[0]
    return {"wlse": wlse, "oneshot": oneshot, "beta_byAIC": b_aic, "beta_byBIC": b_bic,
            "dbic_support": support, "path": path, "Sig_inv_sum": S}


def combine_and_finish(buf, P, fit_intercept=False, lars_type="lasso", group=None):
    """The exchange step and the host tail of the sharded path: ONE
    all-reduce of this rank's ``[sum Sig_inv | sum Sig_inv theta | sum theta |
    K | N]`` buffer (P^2 + 2P + 2 fp64, the layout of
    ``reduce_partitions_device(fit, n_rows=True)``), then WLSE / ONESHOT /
    LARS / DBIC from the global sums on every rank."""
    combine(buf, group)
    b = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    S, v, st, K = split_reduced(b[:-1], P)
    return finish(S, v, st, K, int(round(float(b[-1]))), fit_intercept, lars_type)


def reduce_loglik(ll_kb, group=None):
    """Job-level log-likelihoods from this rank's [K, B] per-partition values
    (CPU or device tensor, or array-like): the sum over k in fixed order, then
    ONE ``combine`` of the B doubles.  Returns a numpy [B] array, the same on
    every rank; without a process group the plain local sum."""
    import torch

    t = ll_kb if isinstance(ll_kb, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(ll_kb, dtype=np.float64))
    tot = np.zeros(t.shape[1], dtype=np.float64)
    for row in t.detach().cpu().numpy():  # K x B doubles: summed on the host, k ascending
        tot += row
    # the exchange runs where the values live: RCCL on a device buffer, gloo on a host one
    return combine(torch.from_numpy(tot).to(t.device), group).cpu().numpy()


def loglik_sharded(X, y, offsets, betas, fit_intercept=False, center=None, scale=None,
                   codes=None, levels=None, group=None, family="logistic", eta_offset=None,
                   exposure=None, sample_weight=None):
    """Second pass of a sharded job (dlsa/model_eval.py:10-42): the
    log-likelihood of each candidate row of ``betas`` [B, P] over the whole
    data set.  X, y, offsets describe the LOCAL shard as in
    ``dlsa_fit_sharded`` (with ``codes``/``levels`` X holds the numeric columns
    of the categorical-code layout).  The local pass leaves the [B] total of
    this rank's partitions on the device; ONE all-reduce of those B doubles
    gives every rank the global sums.  Returns a numpy [B] array.
    ``sample_weight``: the prior weights of the local shard's rows
    (``logistic_loglik_batched`` / ``logistic_loglik_batched_categorical``).
    ``family`` = "poisson": the Poisson log-likelihood, with ``eta_offset`` /
    ``exposure`` of the local shard's rows (``poisson_loglik_batched_weighted``
    / ``poisson_loglik_batched_categorical``)."""
    from .models import (logistic_loglik_batched, logistic_loglik_batched_categorical,
                         poisson_loglik_batched_categorical, poisson_loglik_batched_weighted)

    if family not in ("logistic", "poisson"):
        raise ValueError(f"family must be 'logistic' or 'poisson', not {family!r}")
    if (eta_offset is not None or exposure is not None) and family != "poisson":
        raise ValueError("eta_offset / exposure need family='poisson'")
    if family == "poisson":
        kw = dict(sample_weight=sample_weight, eta_offset=eta_offset, exposure=exposure,
                  fit_intercept=fit_intercept, center=center, scale=scale, return_sum=True)
        if codes is not None:
            _, tot = poisson_loglik_batched_categorical(X, codes, y, offsets, levels, betas, **kw)
        else:
            _, tot = poisson_loglik_batched_weighted(X, y, offsets, betas, **kw)
    elif codes is not None:
        _, tot = logistic_loglik_batched_categorical(
            X, codes, y, offsets, levels, betas, fit_intercept=fit_intercept, center=center,
            scale=scale, return_sum=True, sample_weight=sample_weight)
    else:
        _, tot = logistic_loglik_batched(X, y, offsets, betas, fit_intercept=fit_intercept,
                                         center=center, scale=scale, return_sum=True,
                                         sample_weight=sample_weight)
    return combine(tot, group).cpu().numpy()


def gof_sharded(X, y, offsets, betas, fit_intercept=False, center=None, scale=None,
                codes=None, levels=None, group=None, family="logistic", eta_offset=None,
                exposure=None, sample_weight=None):
    """``loglik_sharded`` for the goodness-of-fit pass (``glm_gof_batched`` /
    ``glm_gof_batched_categorical``, the same arguments): the residual deviance
    and the Pearson chi-square of each candidate row of ``betas`` [B, P] over
    the whole data set, and the rows with a positive weight.  ONE all-reduce of
    this rank's 2B + 1 totals.  Returns a dict, the same on every rank:
    ``deviance`` and ``pearson`` numpy [B], ``n_pos`` an int."""
    import torch

    from .models import glm_gof_batched, glm_gof_batched_categorical

    kw = dict(betas=betas, eta_offset=eta_offset, exposure=exposure, sample_weight=sample_weight,
              fit_intercept=fit_intercept, center=center, scale=scale, return_sum=True)
    if codes is not None:
        g = glm_gof_batched_categorical(family, X, codes, y, offsets, levels, **kw)
    else:
        g = glm_gof_batched(family, X, y, offsets, **kw)
    B = g["deviance_sum"].numel()
    tot = torch.cat([g["deviance_sum"], g["pearson_sum"],
                     g["n_pos_sum"].to(torch.float64).reshape(1)])
    tot = combine(tot, group).cpu().numpy()
    return {"deviance": tot[:B], "pearson": tot[B:2 * B], "n_pos": int(round(float(tot[-1])))}


def combine_gram(gram_sum, score_sum, group=None):
    """The exchange step of ``gram_sharded``: ONE ``combine`` of this rank's
    ``[gram_sum | score_sum]`` (P^2 + P doubles; host or device tensors).
    Returns numpy ``(gram_sum [P, P], score_sum [P])``, the same on every
    rank."""
    import torch

    P = score_sum.numel()
    tot = combine(torch.cat([gram_sum.reshape(-1), score_sum.reshape(-1)]), group).cpu().numpy()
    return tot[:P * P].reshape(P, P).copy(), tot[P * P:].copy()


def gram_sharded(X, y, offsets, thetas=None, beta=None, kind="score", family="logistic",
                 eta_offset=None, exposure=None, sample_weight=None, fit_intercept=False,
                 center=None, scale=None, rows_per_chunk=0, group=None, codes=None, levels=None):
    """``loglik_sharded`` for the score outer-product pass
    (``glm_gram_batched``, the same arguments; X, y, offsets describe the LOCAL
    shard): the sum over every partition of the job of the meat (``kind`` =
    "score") or the information matrix ("information") and of the score
    vector.  With ``codes``/``levels`` X holds the numeric columns of the
    categorical-code layout (``glm_gram_batched_categorical``).  ONE all-reduce
    of this rank's P^2 + P totals.  Returns a dict of numpy arrays, the same on
    every rank: ``gram_sum`` [P, P], ``score_sum`` [P]."""
    from .models import glm_gram_batched, glm_gram_batched_categorical

    kw = dict(thetas=thetas, beta=beta, kind=kind, eta_offset=eta_offset, exposure=exposure,
              sample_weight=sample_weight, fit_intercept=fit_intercept, center=center,
              scale=scale, return_sum=True, rows_per_chunk=rows_per_chunk)
    if codes is not None:
        g = glm_gram_batched_categorical(family, X, codes, y, offsets, levels, **kw)
    else:
        g = glm_gram_batched(family, X, y, offsets, **kw)
    G, sc = combine_gram(g["gram_sum"], g["score_sum"], group)
    return {"gram_sum": G, "score_sum": sc}


def sandwich_cov(A, M):
    """The sandwich (Huber-White) covariance of the combined estimate and the
    information matrix it implies, from A = sum_k Sig_inv_k and the meat M =
    sum_k M_k (both [P, P], symmetric):

    * ``cov``  = A^-1 M A^-1, symmetrised -- Cov(theta~) for theta~ = A^-1
      sum_k S_k theta_k with independent partitions, Cov(theta_k) = S_k^-1 M_k
      S_k^-1 (the per-partition inverses cancel);
    * ``info`` = A M^-1 A = cov^-1, what LARS / DBIC take in place of A.  With
      M = phi A these are phi A^-1 and A / phi: the quasi-likelihood scaling.

    Both come from the Cholesky factor of M and solves with A, never from
    explicit inverses multiplied together.  A meat that is not positive
    definite (fewer rows with a positive weight than P over the whole job)
    raises ``ValueError``.  Returns ``(cov, info)``."""
    A = np.asarray(A, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or M.shape != A.shape:
        raise ValueError("A and M must be square matrices of one shape")
    P = A.shape[0]
    M = 0.5 * (M + M.T)
    bad = "the meat M is not positive definite (fewer rows with a positive weight than P?)"
    if not np.all(np.isfinite(M)) or not np.all(np.isfinite(A)):
        raise ValueError("A or M is not finite")
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError as e:
        raise ValueError(bad) from e
    # a rank-deficient M that rounding let through: a pivot at rounding level
    if not np.min(np.diag(L)) ** 2 > P * np.finfo(np.float64).eps * np.max(np.diag(M)):
        raise ValueError(bad)
    Y = np.linalg.solve(A, M)        # A^-1 M
    cov = np.linalg.solve(A, Y.T)    # A^-1 (A^-1 M)^T = A^-1 M A^-1 (A, M symmetric)
    cov = 0.5 * (cov + cov.T)
    Z = np.linalg.solve(L, A)        # L^-1 A;  info = Z^T Z = A L^-T L^-1 A
    info = Z.T @ Z
    return cov, 0.5 * (info + info.T)


_COV_TYPES = (None, "model", "HC0", "HC1", "HC3")


def _cov_summary(out, cov, wlse):
    """cov and what a coefficient table prints from it: std_err, z = wlse /
    std_err and the two-sided normal p_value = erfc(|z| / sqrt 2)."""
    import math

    se = np.sqrt(np.diag(cov))
    z = wlse / se
    out["cov"] = cov
    out["std_err"] = se
    out["z"] = z
    out["p_value"] = np.array([math.erfc(abs(float(v)) / math.sqrt(2.0)) for v in z])


def _meat_sum(fit, X, y, offsets, family, eta_offset, exposure, sample_weight, fit_intercept,
              center, scale, group, meat_weight=None, codes=None, levels=None):
    """sum_k M_k over the partitions the combine counts (status ok or maxiter)
    and over the ranks -- one score pass at each partition's own ``fit.theta``
    row, the others zeroed before the sum, one all-reduce -- with, in the same
    buffer, n+ (the rows with omega > 0 of those partitions; one more
    goodness-of-fit pass only when weights are given) and their count K_ok.
    ``meat_weight``: None, or the weight the score pass takes in place of
    ``sample_weight`` (HC3's omega / (1 - h)); n+ keeps counting omega > 0.
    ``codes`` / ``levels``: X holds the numeric columns of the categorical-code
    layout, and the two passes are that layout's.
    Returns (M [P, P], n+, K_ok)."""
    import torch

    from .models import (glm_gof_batched, glm_gof_batched_categorical, glm_gram_batched,
                         glm_gram_batched_categorical)

    kw = dict(thetas=fit.theta, eta_offset=eta_offset, exposure=exposure,
              sample_weight=sample_weight, fit_intercept=fit_intercept, center=center,
              scale=scale)
    if codes is not None:
        g = glm_gram_batched_categorical(
            family, X, codes, y, offsets, levels, kind="score",
            **(kw if meat_weight is None else dict(kw, sample_weight=meat_weight)))
    elif meat_weight is None:
        g = glm_gram_batched(family, X, y, offsets, kind="score", **kw)
    else:
        g = glm_gram_batched(family, X, y, offsets, kind="score",
                             **dict(kw, sample_weight=meat_weight))
    ok = fit.status <= 1
    zero = torch.zeros((), dtype=torch.float64, device=ok.device)
    M = torch.where(ok[:, None, None], g["gram"], zero).sum(0)
    if sample_weight is not None and codes is not None:
        rows = glm_gof_batched_categorical(family, X, codes, y, offsets, levels,
                                           **kw)["n_pos"].to(torch.float64)
    elif sample_weight is not None:
        rows = glm_gof_batched(family, X, y, offsets, **kw)["n_pos"].to(torch.float64)
    else:
        rows = torch.from_numpy(np.diff(np.asarray(offsets, dtype=np.int64)).astype(np.float64)
                                ).to(ok.device)
    npos = torch.where(ok, rows, zero).sum()
    tot = combine(torch.cat([M.reshape(-1), torch.stack([npos, ok.sum().to(torch.float64)])]),
                  group).cpu().numpy()
    P = fit.P
    return tot[:P * P].reshape(P, P).copy(), float(tot[-2]), float(tot[-1])


def _hc3_weight(fit, X, y, offsets, family, eta_offset, exposure, sample_weight, fit_intercept,
                center, scale):
    """omega / (1 - h), the row weight whose score pass gives the HC3 meat
    sum_i s_i^2 / (1 - h_i)^2 x_i x_i^T (mu does not depend on omega): one rows
    pass at each partition's own ``fit.theta`` and ``fit.sig_inv``, the local
    leverage.  A partition the combine counts (status ok or maxiter) with a
    row where omega > 0 and h is not finite or 1 - h <= 0 raises
    ``ValueError``: HC3 is undefined there.  The rows of the other partitions
    get the weight 0 (their meat is not counted)."""
    import torch

    from .models import glm_rows_batched

    h = glm_rows_batched(family, X, y, offsets, thetas=fit.theta, info=fit.sig_inv,
                         outputs=("leverage",), eta_offset=eta_offset, exposure=exposure,
                         sample_weight=sample_weight, fit_intercept=fit_intercept, center=center,
                         scale=scale)["leverage"]
    f64 = dict(dtype=torch.float64, device=h.device)
    om = (torch.ones_like(h) if sample_weight is None
          else torch.as_tensor(sample_weight, **f64).reshape(-1))
    offs = torch.as_tensor(np.asarray(offsets, dtype=np.int64), device=h.device)
    part = torch.repeat_interleave(torch.arange(offs.numel() - 1, device=h.device),
                                   offs[1:] - offs[:-1])
    counted = (fit.status <= 1).to(h.device)[part]
    bad = counted & (om > 0) & ~(torch.isfinite(h) & (h < 1.0))
    if bool(bad.any()):
        k = int(part[bad][0])
        raise ValueError(f"cov_type='HC3': partition {k} has a row with a positive weight whose "
                         "leverage h is not finite or not below 1; HC3 is undefined there")
    zero = torch.zeros((), **f64)
    return torch.where(counted & (om > 0), om / (1.0 - h), zero)


def _pearson_dispersion(fit, X, y, offsets, codes, levels, family, eta_offset, exposure,
                        sample_weight, fit_intercept, center, scale, group):
    """phi = sum_k chi^2_k / (sum_k n+_k - K_ok P): the Pearson chi-square of
    every partition at its own ``fit.theta`` row (one goodness-of-fit pass in
    per-partition mode) over the residual degrees of freedom, summed over the
    partitions the combine counts (status ok or maxiter; K_ok of them) and over
    the ranks (one all-reduce of three doubles)."""
    import torch

    from .models import glm_gof_batched, glm_gof_batched_categorical

    kw = dict(thetas=fit.theta, eta_offset=eta_offset, exposure=exposure,
              sample_weight=sample_weight, fit_intercept=fit_intercept, center=center,
              scale=scale)
    if codes is not None:
        g = glm_gof_batched_categorical(family, X, codes, y, offsets, levels, **kw)
    else:
        g = glm_gof_batched(family, X, y, offsets, **kw)
    ok = fit.status <= 1
    zero = torch.zeros((), dtype=torch.float64, device=ok.device)
    chi = torch.where(ok, g["pearson"][:, 0], zero).sum()
    npos = torch.where(ok, g["n_pos"].to(torch.float64), zero).sum()
    tot = combine(torch.stack([chi, npos, ok.sum().to(torch.float64)]), group).cpu().numpy()
    dof = tot[1] - tot[2] * fit.P
    if not dof > 0:
        raise ValueError(f"dispersion='pearson': residual degrees of freedom {dof:g} = rows with "
                         "a positive weight - fitted partitions x P is not positive")
    return float(tot[0] / dof)


def _sandwich_tail(fit, buf, M, npos, k_ok, cov_type, fit_intercept, lars_type, group):
    """The robust tail of ``dlsa_fit_sharded`` and ``sandwich_sharded`` from
    this rank's reduced buffer and the job's meat: the all-reduce, HC1's
    factor, ``sandwich_cov``, ``finish`` on A M^-1 A and the coefficient
    table."""
    b = combine(buf, group).cpu().numpy()
    S, v, st, K = split_reduced(b[:-1], fit.P)
    factor = 1.0
    if cov_type == "HC1":
        dof = npos - k_ok * fit.P
        if not dof > 0:
            raise ValueError(f"cov_type='HC1': residual degrees of freedom {dof:g} = rows "
                             "with a positive weight - fitted partitions x P is not positive")
        factor = npos / dof
    wlse = np.linalg.lstsq(S, v, rcond=None)[0]
    cov, info = sandwich_cov(S, M * factor)
    out = finish(info, info @ wlse, st, K, int(round(float(b[-1]))), fit_intercept, lars_type)
    out.update(wlse=wlse, Sig_inv_sum=S, info=info, meat_sum=M)
    _cov_summary(out, cov, wlse)
    return out


def sandwich_sharded(fit, X, y, offsets, cov_type="HC0", codes=None, levels=None,
                     family="logistic", eta_offset=None, exposure=None, sample_weight=None,
                     fit_intercept=False, center=None, scale=None, lars_type="lasso", group=None):
    """The robust branch of ``dlsa_fit_sharded`` for an existing ``BatchedFit``
    of this rank's partitions, on either layout: ``reduce_partitions_device``,
    the meat at each partition's own ``fit.theta`` row over the partitions the
    combine counts (status ok or maxiter), the all-reduces, ``sandwich_cov``,
    the LARS / DBIC tail on A M^-1 A and the coefficient table.  X, y, offsets
    and the keywords describe the LOCAL shard exactly as they were given to the
    fit.  Returns the keys ``dlsa_fit_sharded(cov_type=...)`` returns except
    ``"fit"``; on the dense layout they are the same bits.

    With ``codes``/``levels`` X holds the numeric columns of the
    categorical-code layout and the passes are
    ``glm_gram_batched_categorical`` (and, for HC1's n+ with weights,
    ``glm_gof_batched_categorical``).  ``dlsa_fit_sharded`` itself still
    refuses ``cov_type`` with ``codes=``; the route on codes is

        out = dlsa_fit_sharded(X, y, offsets, codes=codes, levels=levels, ...)
        out.update(sandwich_sharded(out["fit"], X, y, offsets, codes=codes,
                                    levels=levels, ...))

    ``cov_type``: "HC0", "HC1" or, on the dense layout only, "HC3" (leverages
    on the code layout are not computed yet: ``ValueError``); anything else
    raises ``ValueError``."""
    if cov_type not in ("HC0", "HC1", "HC3"):
        raise ValueError(f"cov_type must be 'HC0', 'HC1' or 'HC3', not {cov_type!r}")
    if family not in ("logistic", "poisson"):
        raise ValueError(f"family must be 'logistic' or 'poisson', not {family!r}")
    if (eta_offset is not None or exposure is not None) and family != "poisson":
        raise ValueError("eta_offset / exposure need family='poisson'")
    if cov_type == "HC3" and codes is not None:
        raise ValueError("cov_type='HC3' with codes=: the leverages cover the dense layout only "
                         "(the categorical-code layout is not supported yet)")
    buf = reduce_partitions_device(fit, n_rows=True)
    mw = None
    if cov_type == "HC3":
        mw = _hc3_weight(fit, X, y, offsets, family, eta_offset, exposure, sample_weight,
                         fit_intercept, center, scale)
    M, npos, k_ok = _meat_sum(fit, X, y, offsets, family, eta_offset, exposure, sample_weight,
                              fit_intercept, center, scale, group, meat_weight=mw, codes=codes,
                              levels=levels)
    return _sandwich_tail(fit, buf, M, npos, k_ok, cov_type, fit_intercept, lars_type, group)


def dlsa_fit_sharded(X, y, offsets, fit_intercept=False, lars_type="lasso",
                     group=None, codes=None, levels=None, family="logistic", eta_offset=None,
                     exposure=None, dispersion=None, cov_type=None, sample_weight=None,
                     **fit_kw):
    """Fit this rank's partitions on its GPU and return the global DLSA result.

    X, y, offsets describe the LOCAL shard (rows already on this rank's
    device).  With ``codes``/``levels`` X holds the numeric columns of the
    categorical-code layout (``logistic_model_batched_categorical``).  The
    row count N of the DBIC is summed in the same single collective as the
    partition sums (reference: the shuffle + collect of dlsa/dlsa.py:30-34).
    ``family`` = "logistic" or "poisson" (``poisson_model_batched``, with
    ``codes`` ``poisson_model_batched_categorical``); everything after the
    local fits is the same for both.
    ``eta_offset`` / ``exposure`` (family="poisson" only): the per-row offset
    of the local shard's rows (``poisson_model_batched_offset``); the combine
    step never sees it.
    ``sample_weight``: per-row prior weights of the local shard's rows
    (``logistic_model_batched_weighted`` / ``poisson_model_batched_weighted``,
    with ``codes`` ``logistic_model_batched_categorical_weighted``).  N, the
    DBIC's sample size, stays the ROW count: weights that are
    precision or survey weights leave the number of observations unchanged.  A
    frequency-weights user who wants N = sum of the weights calls
    ``finish(..., n_global=)`` on the reduced sums directly.
    ``dispersion``: None (the default: exactly the call without the keyword),
    or "pearson", the quasi-likelihood correction of an over-dispersed fit (R's
    quasipoisson / quasibinomial): after the local fits one goodness-of-fit
    pass at each partition's own ``fit.theta`` and one more all-reduce of
    three doubles give phi = Pearson chi^2 / residual degrees of freedom
    (``_pearson_dispersion``), and the tail runs on ``S / phi``, ``v / phi``.
    The WLSE is unchanged; LARS / DBIC see the scaled information matrix.  The
    result gains ``"dispersion"``.  Non-positive degrees of freedom raise
    ``ValueError``.
    ``cov_type``: None (the default: exactly the call without the keyword, no
    new keys), or the covariance of the WLSE the result gains as ``"cov"``
    with ``"std_err"`` = sqrt(diag cov), ``"z"`` = wlse / std_err and
    ``"p_value"`` = erfc(|z| / sqrt 2):

    * "model": (sum_k Sig_inv_k)^-1, times phi with ``dispersion="pearson"``;
      no new pass.  Right when Var(y) = phi V(mu).
    * "HC0": the sandwich A^-1 (sum_k M_k) A^-1 (Huber-White; R's
      ``sandwich::vcovHC(type="HC0")``), A = sum_k Sig_inv_k, M_k = sum_i s_i^2
      x_i x_i^T with s_i = omega_i (y_i - mu_i(theta_k)): one score pass at
      each partition's own ``fit.theta`` (``glm_gram_batched``), summed over
      the partitions the combine counts, and one more all-reduce of P^2 + 2
      doubles.  omega enters the meat squared, the precision / survey-weight
      convention of R's ``sandwich::estfun``: frequency weights are not
      replicated rows here.  The WLSE and ONESHOT are unchanged; LARS / DBIC
      run on ``info`` = A M^-1 A in place of A (``sandwich_cov``; with M = phi
      A today's S / phi).  The result also gains ``"meat_sum"`` (sum_k M_k)
      and ``"info"``.
    * "HC1": HC0 times n+ / (n+ - K_ok P), n+ the rows with omega > 0 of the
      K_ok counted partitions (the degrees of freedom of ``dispersion=``; with
      weights one more goodness-of-fit pass counts them).  A non-positive
      denominator raises ``ValueError``.

    * "HC3": HC0 with every row's s_i^2 divided by (1 - h_i)^2 (R's
      ``sandwich::vcovHC`` default), h_i = omega_i w_i x_i^T Sig_inv_k^-1 x_i
      the leverage against the row's own partition: with n split over K
      partitions it is K times a pooled fit's, so the correction matters
      exactly here.  One rows pass (``glm_rows_batched``, leverages only) and
      the score pass with the weight omega / (1 - h).  A counted partition
      with a row where omega > 0 and 1 - h <= 0 or h is not finite raises
      ``ValueError``.  (HC2: ``glm_rows_batched``'s ``leverage`` and a score
      pass with ``sample_weight = omega / sqrt(1 - h)``.)

    "HC0" / "HC1" / "HC3" with ``dispersion="pearson"`` raise ``ValueError`` (the
    sandwich already absorbs phi), and with ``codes=`` too: on the
    categorical-code layout the robust covariance is one more call,
    ``out.update(sandwich_sharded(out["fit"], X, y, offsets, codes=codes,
    levels=levels, ...))`` ("HC0" / "HC1"; ``glm_gram_batched_categorical``).
    """
    from .models import (logistic_model_batched, logistic_model_batched_categorical,
                         logistic_model_batched_categorical_weighted,
                         logistic_model_batched_weighted, poisson_model_batched,
                         poisson_model_batched_categorical, poisson_model_batched_offset,
                         poisson_model_batched_weighted)

    if family not in ("logistic", "poisson"):
        raise ValueError(f"family must be 'logistic' or 'poisson', not {family!r}")
    if (eta_offset is not None or exposure is not None) and family != "poisson":
        raise ValueError("eta_offset / exposure need family='poisson'")
    if dispersion not in (None, "pearson"):
        raise ValueError(f"dispersion must be None or 'pearson', not {dispersion!r}")
    if cov_type not in _COV_TYPES:
        raise ValueError("cov_type must be None, 'model', 'HC0', 'HC1' or 'HC3', not "
                         f"{cov_type!r}")
    robust = cov_type in ("HC0", "HC1", "HC3")
    if robust and dispersion is not None:
        raise ValueError(f"cov_type={cov_type!r} with dispersion='pearson': the sandwich already "
                         "absorbs the dispersion; give one of them")
    if robust and codes is not None:
        raise ValueError(f"cov_type={cov_type!r} with codes=: the score pass covers the dense "
                         "layout only (the categorical-code layout is not supported yet)")
    if family == "poisson" and codes is not None:
        fit = poisson_model_batched_categorical(X, codes, y, offsets, levels,
                                                sample_weight=sample_weight,
                                                eta_offset=eta_offset, exposure=exposure,
                                                fit_intercept=fit_intercept, **fit_kw)
    elif sample_weight is not None:  # (None: exactly the unweighted calls below)
        if family == "poisson":
            fit = poisson_model_batched_weighted(X, y, offsets, sample_weight=sample_weight,
                                                 eta_offset=eta_offset, exposure=exposure,
                                                 fit_intercept=fit_intercept, **fit_kw)
        elif codes is not None:
            fit = logistic_model_batched_categorical_weighted(
                X, codes, y, offsets, levels, sample_weight=sample_weight,
                fit_intercept=fit_intercept, **fit_kw)
        else:
            fit = logistic_model_batched_weighted(X, y, offsets, sample_weight=sample_weight,
                                                  fit_intercept=fit_intercept, **fit_kw)
    elif family == "poisson":
        if eta_offset is not None or exposure is not None:
            fit = poisson_model_batched_offset(X, y, offsets, eta_offset=eta_offset,
                                               exposure=exposure, fit_intercept=fit_intercept,
                                               **fit_kw)
        else:
            fit = poisson_model_batched(X, y, offsets, fit_intercept=fit_intercept, **fit_kw)
    elif codes is not None:
        fit = logistic_model_batched_categorical(X, codes, y, offsets, levels,
                                                 fit_intercept=fit_intercept, **fit_kw)
    else:
        fit = logistic_model_batched(X, y, offsets, fit_intercept=fit_intercept, **fit_kw)
    buf = reduce_partitions_device(fit, n_rows=True)
    if robust:
        cs = (fit_kw.get("center"), fit_kw.get("scale"))
        if cov_type == "HC3":
            mw = _hc3_weight(fit, X, y, offsets, family, eta_offset, exposure, sample_weight,
                             fit_intercept, *cs)
            M, npos, k_ok = _meat_sum(fit, X, y, offsets, family, eta_offset, exposure,
                                      sample_weight, fit_intercept, *cs, group, meat_weight=mw)
        else:
            M, npos, k_ok = _meat_sum(fit, X, y, offsets, family, eta_offset, exposure,
                                      sample_weight, fit_intercept, *cs, group)
        out = _sandwich_tail(fit, buf, M, npos, k_ok, cov_type, fit_intercept, lars_type, group)
    elif dispersion is None:
        out = combine_and_finish(buf, fit.P, fit_intercept, lars_type, group)
    else:
        phi = _pearson_dispersion(fit, X, y, offsets, codes, levels, family, eta_offset, exposure,
                                  sample_weight, fit_intercept, fit_kw.get("center"),
                                  fit_kw.get("scale"), group)
        b = combine(buf, group).cpu().numpy()
        S, v, st, K = split_reduced(b[:-1], fit.P)
        out = finish(S / phi, v / phi, st, K, int(round(float(b[-1]))), fit_intercept, lars_type)
        out["dispersion"] = phi
    if cov_type == "model":
        S = out["Sig_inv_sum"]  # (with a dispersion S / phi: its inverse is phi S^-1)
        cov = np.linalg.solve(S, np.eye(fit.P))
        _cov_summary(out, 0.5 * (cov + cov.T), out["wlse"])
    out["fit"] = fit
    return out
