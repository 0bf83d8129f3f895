"""Job-level evaluation pass of DLSA on MI355X.

Drop-in for dlsa/model_eval.py of the reference: ``logistic_model_eval_sdf``
(model_eval.py:10-42, called from projects/logistic_dlsa.py:366-372) scores the
coefficient columns of ``par`` (AIC / BIC / WLSE / ONESHOT) on the whole data
set -- every partition's log-likelihoods (dlsa/models.py:151-225) summed in one
group-by.  Here all partitions go through ONE batched pass on the GPU, on the
categorical-code layout when there are factors, the per-partition values are
summed on the device in partition order, and under ``torch.distributed`` one
all-reduce of the B sums gives every rank the job's totals.

There is no CPU implementation: without libdlsa_hip.so or a GPU this raises
``DlsaHipError``.
"""

from __future__ import annotations

import numpy as np

from . import _hip
from .distributed import reduce_loglik
from .models import (_describe_row, _require_gpu, encode_categorical, logistic_loglik_batched,
                     logistic_loglik_batched_categorical, logistic_model_eval, partition_offsets)


def _center_scale(data_info, columns):
    if len(data_info) == 0 or len(columns) == 0:
        return None, None
    return (np.array([_describe_row(data_info, c, 1) for c in columns]),
            np.array([_describe_row(data_info, c, 2) for c in columns]))


def _eval_dict(data, betas, fit_intercept, data_info):
    """Per-partition log-likelihoods [K, B] of a ``read_csv_partitioned``
    result (rows already in HBM, dense or code layout)."""
    if "codes" in data:
        center, scale = _center_scale(data_info, data["numeric"])
        return logistic_loglik_batched_categorical(
            data["Xn"], data["codes"], data["y"], data["offsets"], data["levels"], betas,
            fit_intercept=fit_intercept, center=center, scale=scale)
    center, scale = _center_scale(data_info, data["columns"])
    return logistic_loglik_batched(data["X"], data["y"], data["offsets"], betas,
                                   fit_intercept=fit_intercept, center=center, scale=scale)


def _eval_frame(df, betas, par, fit_intercept, Y_name, dummy_info, dummy_factors_baseline,
                data_info):
    """Per-partition log-likelihoods [K, B] of a pandas frame with a
    ``partition_id`` column, partitions in ascending id order."""
    import torch

    ids, inverse = np.unique(df["partition_id"].to_numpy(), return_inverse=True)
    order, offsets = partition_offsets(inverse, len(ids))
    df = df.iloc[order]
    y = df[Y_name].to_numpy(dtype=np.float64)
    ic = int(bool(fit_intercept))
    if len(dummy_info) == 0:
        x = df.drop(["partition_id", Y_name] + list(dummy_factors_baseline), axis=1)
        center, scale = _center_scale(data_info, list(x.columns))
        return logistic_loglik_batched(np.ascontiguousarray(x.to_numpy(dtype=np.float64)), y,
                                       offsets, betas, fit_intercept=fit_intercept,
                                       center=center, scale=scale)
    base = set(dummy_factors_baseline)
    if all(sum(c not in base for c in names) <= 255
           for names in dummy_info["factor_selected_names"].values()):
        enc = encode_categorical(df, Y_name, dummy_info, dummy_factors_baseline)
        q, F = enc["Xn"].shape[1], enc["codes"].shape[1]
        if F <= 16 and ic + q <= 16 and ic + len(enc["cols"]) <= _hip.MAX_P:
            center, scale = _center_scale(data_info, enc["numeric"])
            return logistic_loglik_batched_categorical(
                enc["Xn"], enc["codes"], y, offsets, enc["levels"], betas,
                fit_intercept=fit_intercept, center=center, scale=scale)
    # beyond the code layout's limits: the dense design, one partition at a time
    rows = [logistic_model_eval(df.iloc[offsets[k]:offsets[k + 1]], Y_name, par, fit_intercept,
                                dummy_info, dummy_factors_baseline, data_info).to_numpy()[0]
            for k in range(len(ids))]
    return torch.from_numpy(np.array(rows, dtype=np.float64).reshape(len(ids), betas.shape[0]))


def logistic_model_eval_sdf(data_sdf, par, fit_intercept, Y_name, dummy_info=[],
                            dummy_factors_baseline=[], data_info=[], group=None):
    """Log-likelihood of each coefficient column of ``par`` over the whole data
    set (dlsa/model_eval.py:10-42; the reference's argument order).

    ``data_sdf``: a pandas DataFrame with a ``partition_id`` column (the
    stand-in for the Spark frame, as in ``logistic_model``), or the dict
    ``ingest.read_csv_partitioned`` returns (rows already in HBM, dense or
    code layout -- ``dummy_info`` was applied by the ingest).  ``par``: a
    P-row DataFrame, one column per method, intercept first.  A factor level
    missing from a partition is an all-zero dummy column there, as in
    ``logistic_model_eval``.  Returns a one-row DataFrame with ``par``'s
    columns: the sum over all partitions; with a process group initialised
    (each rank holding its shard), the global sums on every rank."""
    import pandas as pd

    _require_gpu()
    betas = np.ascontiguousarray(np.asarray(par, dtype=np.float64).T)
    if isinstance(data_sdf, dict):
        ll = _eval_dict(data_sdf, betas, fit_intercept, data_info)
    else:
        ll = _eval_frame(data_sdf, betas, par, fit_intercept, Y_name, dummy_info,
                         dummy_factors_baseline, data_info)
    return pd.DataFrame(reduce_loglik(ll, group)[None, :], columns=list(par.columns))
