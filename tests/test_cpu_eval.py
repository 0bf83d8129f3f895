"""CPU tests of the job-level evaluation pass's host side: the exchange of the
per-partition log-likelihoods (distributed.reduce_loglik) under gloo with
world_size 2, the C-ABI bindings of the new entry points, and the loud
failure of model_eval.logistic_model_eval_sdf without a GPU."""

import os

import numpy as np
import pytest


def _gloo_worker(rank, world, port, golden_dir, q, shards):
    import torch
    import torch.distributed as dist

    from dlsa_amd.distributed import reduce_loglik

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ll = np.load(os.path.join(golden_dir, "eval.npz"))["ll_int_std"]  # [4 partitions, 4]
        mine = torch.from_numpy(np.ascontiguousarray(ll[shards[rank]]))
        calls = []
        orig = dist.all_reduce

        def counting(*a, **k):
            calls.append(1)
            return orig(*a, **k)

        dist.all_reduce = counting
        try:
            tot = reduce_loglik(mine)
        finally:
            dist.all_reduce = orig
        q.put((rank, tot, len(calls)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("shards", [([0, 2], [1, 3]), ([0, 1, 3], [2])])
def test_reduce_loglik_gloo(golden_dir, shards):
    """Each rank feeds its partitions' rows of the reference's per-partition
    log-likelihoods (eval.npz, intercept + data_info); ONE all-reduce gives
    both ranks the job's sums (dlsa/model_eval.py:38)."""
    import multiprocessing as mp
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, golden_dir, q, shards))
          for r in range(2)]
    for p_ in ps:
        p_.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p_ in ps:
        p_.join(timeout=60)
        assert p_.exitcode == 0
    ref = np.load(os.path.join(golden_dir, "eval.npz"))["ll_int_std"].sum(0)
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, tot, n_calls in res:
        assert n_calls == 1
        assert tot.shape == ref.shape
        assert np.abs(tot - ref).max() <= 1e-12 * np.abs(ref).max()


def test_reduce_loglik_without_process_group(golden_dir):
    import torch

    from dlsa_amd.distributed import reduce_loglik

    ll = np.load(os.path.join(golden_dir, "eval.npz"))["ll_int_std"]
    ref = ll.sum(0)
    for arg in (ll, torch.from_numpy(ll)):
        tot = reduce_loglik(arg)
        assert isinstance(tot, np.ndarray) and tot.shape == (ll.shape[1],)
        assert np.abs(tot - ref).max() <= 1e-12 * np.abs(ref).max()


def test_eval_bindings_declared_and_exported():
    import ctypes

    from dlsa_amd import _hip

    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name, nargs in (("dlsa_logistic_loglik_categorical", 17),
                        ("dlsa_logistic_loglik_batched_sum", 13)):
        assert name in _hip.SIGNATURES
        res, args = _hip.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert hasattr(lib, name)
    # the existing entry keeps its signature
    assert len(_hip.SIGNATURES["dlsa_logistic_loglik_batched"][1]) == 12


def test_eval_sdf_imports_and_fails_loudly_without_gpu():
    import pandas as pd
    import torch

    from dlsa_amd import DlsaHipError
    from dlsa_amd.distributed import loglik_sharded
    from dlsa_amd.model_eval import logistic_model_eval_sdf
    from dlsa_amd.models import logistic_loglik_batched_categorical

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    df = pd.DataFrame({"partition_id": [0.0, 0.0, 1.0, 1.0], "label": [0.0, 1.0, 1.0, 0.0],
                       "x0": [0.1, 0.2, 0.3, 0.4], "x1": [1.0, -1.0, 0.5, 0.0]})
    par = pd.DataFrame({"beta_byAIC": [0.5, -0.25], "beta_byBIC": [0.0, 0.0]})
    with pytest.raises(DlsaHipError):
        logistic_model_eval_sdf(df, par, False, "label", [], [], [])
    with pytest.raises(DlsaHipError):
        logistic_loglik_batched_categorical(np.zeros((4, 1)), np.zeros((4, 1), np.uint8),
                                            np.zeros(4), [0, 4], [2], np.zeros((1, 2)))
    with pytest.raises(DlsaHipError):
        loglik_sharded(np.zeros((4, 2)), np.zeros(4), [0, 4], np.zeros((1, 2)))
