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


def dlsa_fit_sharded(X, y, offsets, fit_intercept=False, lars_type="lasso",
                     group=None, codes=None, levels=None, family="logistic", eta_offset=None,
                     exposure=None, dispersion=None, sample_weight=None, **fit_kw):
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
    if dispersion is None:
        out = combine_and_finish(buf, fit.P, fit_intercept, lars_type, group)
    else:
        phi = _pearson_dispersion(fit, X, y, offsets, codes, levels, family, eta_offset, exposure,
                                  sample_weight, fit_intercept, fit_kw.get("center"),
                                  fit_kw.get("scale"), group)
        b = combine(buf, group).cpu().numpy()
        S, v, st, K = split_reduced(b[:-1], fit.P)
        out = finish(S / phi, v / phi, st, K, int(round(float(b[-1]))), fit_intercept, lars_type)
        out["dispersion"] = phi
    out["fit"] = fit
    return out
