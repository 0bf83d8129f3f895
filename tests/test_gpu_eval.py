"""Job-level log-likelihood evaluation on the GPU: the code-layout pass
(dlsa_logistic_loglik_categorical) against the pinned oracle on the dense
dummy expansion, the job-level sums against the reference's own numbers
(tests/golden/eval.npz), and the sharded exchange with two ranks on the one
GPU.  Tolerance: the project's for this quantity, max |ll - ref| <= 1e-10
max |ref| (test_gpu_parity.test_loglik_eval_vs_oracle)."""

import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-10
SIZES = [5000, 3001, 0, 777, 1]  # an empty partition, one row, ragged tails, the buffers' end
NAMES = ["beta_byAIC", "beta_byBIC", "beta_byOLS", "beta_byONESHOT"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def M():
    from dlsa_amd import models
    return models


def _case(q, levels, fi, std, B, sizes=SIZES, seed=0):
    """Numpy data in the code layout + the oracle's [K, B] log-likelihoods on
    the dense dummy expansion."""
    rs = np.random.RandomState(1000 * q + 10 * len(levels) + B + seed)
    n = sum(sizes)
    Xn = rs.randn(n, q) * 2.0 + 1.0 if std else rs.rand(n, q) - 0.5
    codes = np.stack([rs.randint(0, L, n) for L in levels], 1).astype(np.uint8) if levels else \
        np.zeros((n, 0), np.uint8)
    for f, L in enumerate(levels):  # the top code of every factor is present
        codes[f % n, f] = L - 1
    y = (rs.rand(n) < 0.4).astype(np.float64)
    D = sum(L - 1 for L in levels)
    P = int(fi) + q + D
    betas = rs.randn(B, P) * 0.4
    c = rs.randn(q) * 0.5 + 1.0 if std else None
    s = rs.rand(q) + 1.5 if std else None
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = O.expand_codes(Xn, codes, levels)
    kw = dict(center=np.concatenate([c, np.zeros(D)]), scale=np.concatenate([s, np.ones(D)])) \
        if std else {}
    ref = np.array([O.logistic_loglik(X[off[k]:off[k + 1]], y[off[k]:off[k + 1]], betas,
                                      fit_intercept=fi, **kw) for k in range(len(sizes))])
    return dict(Xn=Xn, codes=codes, y=y, off=off, levels=list(levels), betas=betas, c=c, s=s,
                fi=fi, ref=ref)


def _check(ll, tot, ref):
    ll, tot = ll.cpu().numpy(), tot.cpu().numpy()
    assert ll.shape == ref.shape and tot.shape == (ref.shape[1],)
    for k in range(ref.shape[0]):
        err, bound = np.abs(ll[k] - ref[k]).max(), TOL * np.abs(ref[k]).max()
        print(f"partition {k}: max err {err:.3e} bound {bound:.3e}")
        assert err <= bound, k
    rs = ref.sum(0)
    print(f"sum: max err {np.abs(tot - rs).max():.3e} bound {TOL * np.abs(rs).max():.3e}")
    assert np.abs(tot - rs).max() <= TOL * np.abs(rs).max()


def _run(M, d, **kw):
    return M.logistic_loglik_batched_categorical(
        d["Xn"], d["codes"], d["y"], d["off"], d["levels"], d["betas"], fit_intercept=d["fi"],
        center=d["c"], scale=d["s"], return_sum=True, **kw)


CASES = [
    (0, (3,), False, False, 1),                   # no numeric column, no intercept
    (1, (2, 1, 5), True, True, 4),                # a one-level factor has no column
    (9, (12, 7, 20, 69, 69), True, True, 4),      # the airline design (config 3)
    (15, (2,) * 16, True, False, 16),             # intercept + q = 16, F = 16, B = 16
    (1, (256, 256), True, False, 3),              # code 255, P = 512 (> 192, the fit's limit)
    (3, (7,), False, True, 37),                   # B = 37: candidates in groups of 16
]


@pytest.fixture(scope="module")
def cases():
    return {c: _case(*c) for c in CASES}


@pytest.mark.parametrize("rpc", [0, 1500])  # 1500: the 5000-row partition spans 4 chunks
@pytest.mark.parametrize("case", CASES, ids=[f"q{c[0]}-F{len(c[1])}-B{c[4]}" for c in CASES])
def test_loglik_categorical_vs_oracle(torch_cuda, M, cases, case, rpc):
    d = cases[case]
    ll, tot = _run(M, d, rows_per_chunk=rpc)
    _check(ll, tot, d["ref"])


def test_loglik_categorical_deterministic(torch_cuda, M, cases):
    d = cases[CASES[2]]
    a, at = _run(M, d, rows_per_chunk=1500)
    b, bt = _run(M, d, rows_per_chunk=1500)
    assert torch_cuda.equal(a, b) and torch_cuda.equal(at, bt)


def test_loglik_categorical_invalid_code_fails_loudly(torch_cuda, M, cases):
    from dlsa_amd._hip import DlsaHipError

    d = dict(cases[CASES[2]])
    bad = d["codes"].copy()
    bad[4321, 1] = d["levels"][1]  # levels[1] = 7 -> valid codes 0..6
    d["codes"] = bad
    with pytest.raises(DlsaHipError, match="level codes"):
        _run(M, d)
    d = cases[CASES[2]]
    _check(*_run(M, d), d["ref"])


def test_loglik_categorical_limits(torch_cuda, M):
    from dlsa_amd._hip import DlsaHipError

    n = 64
    y = np.zeros(n)
    with pytest.raises(DlsaHipError):  # F = 17
        M.logistic_loglik_batched_categorical(np.zeros((n, 1)), np.zeros((n, 17), np.uint8), y,
                                              [0, n], [2] * 17, np.zeros((1, 18)))
    with pytest.raises(DlsaHipError):  # intercept + q = 17
        M.logistic_loglik_batched_categorical(np.zeros((n, 16)), np.zeros((n, 1), np.uint8), y,
                                              [0, n], [2], np.zeros((1, 18)), fit_intercept=True)


def test_logistic_model_eval_beyond_limits_takes_dense_path(torch_cuda, M):
    """17 numeric columns + intercept exceed the code layout's limit:
    logistic_model_eval still returns the dense design's values."""
    import pandas as pd

    rs = np.random.RandomState(5)
    n = 1500
    num = [f"x{i:02d}" for i in range(17)]
    df = pd.DataFrame(rs.rand(n, 17) - 0.5, columns=num)
    df.insert(0, "label", (rs.rand(n) < 0.5).astype(np.float64))
    df.insert(0, "partition_id", 0.0)
    df["G"] = rs.choice(["a", "b", "c"], n)
    dinfo = {"factor_selected": {"G": ["a", "b", "c"]}, "factor_dropped": {"G": []},
             "factor_selected_names": {"G": ["G_a", "G_b", "G_c"]}}
    par = pd.DataFrame(rs.randn(1 + 17 + 2, 4) * 0.5, columns=NAMES)
    out = M.logistic_model_eval(df, "label", par, True, dinfo, ["G_a"], [])
    X = np.column_stack([df[num].to_numpy(), df["G"] == "b", df["G"] == "c"]).astype(np.float64)
    ref = O.logistic_loglik(X, df["label"].to_numpy(), par.to_numpy().T, fit_intercept=True)
    assert list(out.columns) == NAMES and out.shape == (1, 4)
    assert np.abs(out.to_numpy()[0] - ref).max() <= TOL * np.abs(ref).max()


@pytest.mark.parametrize("fi", [False, True])
@pytest.mark.parametrize("std", [False, True])
def test_eval_sdf_config1_vs_reference(golden_dir, torch_cuda, fi, std):
    """logistic_model_eval_sdf on the 4-partition config-1 frame: the sums of
    the reference's own per-partition values (eval.npz)."""
    import pandas as pd
    from test_oracle_golden import _eval_inputs

    from dlsa_amd.model_eval import logistic_model_eval_sdf

    E, pid, lab, feat, info = _eval_inputs(golden_dir)
    tag = f"{'int' if fi else 'noint'}_{'std' if std else 'raw'}"
    par = pd.DataFrame(E["par_" + tag], columns=NAMES)
    df = pd.DataFrame(np.column_stack([pid, lab, feat]),
                      columns=["partition_id", "label"] + [f"x{i}" for i in range(10)])
    out = logistic_model_eval_sdf(df, par, fi, "label", [], [], info if std else [])
    ref = E["ll_" + tag].sum(0)
    assert list(out.columns) == NAMES and out.shape == (1, 4)
    assert np.abs(out.to_numpy()[0] - ref).max() <= TOL * np.abs(ref).max()


def test_eval_sdf_dummy_branch_vs_reference(golden_dir, torch_cuda):
    import pandas as pd
    from test_oracle_golden import _dummy_fixture

    from dlsa_amd.model_eval import logistic_model_eval_sdf

    E = np.load(os.path.join(golden_dir, "eval.npz"))
    g, df, dinfo, base, info = _dummy_fixture(golden_dir)
    par = pd.DataFrame(E["par_dummy"], columns=NAMES)
    df = df[["partition_id", "label", "DepTime", "Distance", "Month", "UniqueCarrier", "Origin"]]
    df = df[df["partition_id"] < 4].reset_index(drop=True)
    out = logistic_model_eval_sdf(df, par, True, "label", dinfo, base, info)
    ref = E["ll_dummy"][:4].sum(0)
    assert list(out.columns) == NAMES and out.shape == (1, 4)
    assert np.abs(out.to_numpy()[0] - ref).max() <= TOL * np.abs(ref).max()


def test_loglik_categorical_vs_dense_kernel(torch_cuda, M):
    """The code-layout kernel and the dense kernel on expand_categorical of
    the same rows, K = 3."""
    d = _case(9, (12, 7, 20), True, True, 4, sizes=[2000, 1501, 333], seed=7)
    ll = M.logistic_loglik_batched_categorical(
        d["Xn"], d["codes"], d["y"], d["off"], d["levels"], d["betas"], fit_intercept=True,
        center=d["c"], scale=d["s"]).cpu().numpy()
    Xn = torch_cuda.from_numpy(d["Xn"]).cuda()
    X = M.expand_categorical(Xn, torch_cuda.from_numpy(d["codes"]).cuda(), d["levels"])
    D = X.shape[1] - 9
    dense = M.logistic_loglik_batched(
        X, d["y"], d["off"], d["betas"], fit_intercept=True,
        center=np.concatenate([d["c"], np.zeros(D)]),
        scale=np.concatenate([d["s"], np.ones(D)])).cpu().numpy()
    assert ll.shape == dense.shape == (3, 4)
    assert np.abs(ll - dense).max() <= TOL * np.abs(dense).max()


def test_eval_sdf_dict_input_equals_frame(torch_cuda, tmp_path):
    """CSV -> read_csv_partitioned (code layout in HBM) -> logistic_model_eval_sdf
    on the dict == the pandas-frame call on the same rows."""
    import pandas as pd

    from dlsa_amd.ingest import read_csv_partitioned
    from dlsa_amd.model_eval import logistic_model_eval_sdf

    rs = np.random.RandomState(11)
    n, K = 2000, 3
    df = pd.DataFrame({"a": rs.randn(n) * 3 + 1, "b": rs.rand(n),
                       "Carrier": rs.choice(["AA", "BB", "CC", "DD"], n),
                       "Month": rs.randint(1, 7, n), "label": (rs.rand(n) < 0.4).astype(float)})
    df.to_csv(tmp_path / "e.csv", index=False)
    dinfo = {"factor_selected": {"Carrier": ["AA", "BB", "CC", "DD"],
                                 "Month": [1, 2, 3, 4, 5, 6]},
             "factor_dropped": {"Carrier": [], "Month": []},
             "factor_selected_names": {"Carrier": [f"Carrier_{c}" for c in ("AA", "BB", "CC", "DD")],
                                       "Month": [f"Month_{m}" for m in range(1, 7)]}}
    base = ["Carrier_AA", "Month_1"]
    lay = read_csv_partitioned(str(tmp_path / "e.csv"), "label", ["a", "b", "Carrier", "Month"],
                               K=K, dummy_info=dinfo, dummy_factors_baseline=base)
    assert lay["cols"] == ["a", "b", "Carrier_BB", "Carrier_CC", "Carrier_DD"] + \
        [f"Month_{m}" for m in range(2, 7)]
    par = pd.DataFrame(rs.randn(1 + len(lay["cols"]), 4) * 0.4, columns=NAMES)
    info = lay["data_info"]
    got = logistic_model_eval_sdf(lay, par, True, "label", dinfo, base, info)
    frame = df.copy()
    frame.insert(0, "partition_id", (np.arange(n) % K).astype(float))
    ref = logistic_model_eval_sdf(frame, par, True, "label", dinfo, base, info)
    assert list(got.columns) == NAMES and got.shape == (1, 4)
    r = ref.to_numpy()[0]
    assert np.abs(got.to_numpy()[0] - r).max() <= TOL * np.abs(r).max()
    # and both equal the oracle on the dense design
    c = np.array([float(info[k][1]) for k in ("a", "b")])
    s = np.array([float(info[k][2]) for k in ("a", "b")])
    X = np.column_stack([(df[["a", "b"]].to_numpy() - c) / s] +
                        [df["Carrier"] == v for v in ("BB", "CC", "DD")] +
                        [df["Month"] == m for m in range(2, 7)]).astype(np.float64)
    o = O.logistic_loglik(X, df["label"].to_numpy(), par.to_numpy().T, fit_intercept=True)
    assert np.abs(r - o).max() <= TOL * np.abs(o).max()


# ---- two ranks on the one GPU ------------------------------------------------


def _shard(arrs, off, mine):
    out = [np.concatenate([a[off[k]:off[k + 1]] for k in mine]) for a in arrs]
    offl = np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in mine])])
    return out, offl


def _worker(rank, world, port, golden_dir, shards, layout, q, backend):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dlsa_amd.distributed import loglik_sharded

        mine = shards[rank]
        if layout == "dense":
            from test_oracle_golden import _eval_inputs

            E, pid, lab, feat, info = _eval_inputs(golden_dir)
            order, off = O.systematic_partition(pid)
            (Xl, yl), offl = _shard([feat[order], lab[order]], off, mine)
            kw = dict(X=torch.from_numpy(Xl).cuda(), y=torch.from_numpy(yl).cuda(), offsets=offl,
                      betas=E["par_noint_raw"].T)
        else:
            d = _case(4, (5, 7), True, True, 4, sizes=[1500, 1001, 700, 333], seed=3)
            (Xl, cl, yl), offl = _shard([d["Xn"], d["codes"], d["y"]], d["off"], mine)
            kw = dict(X=Xl, y=yl, offsets=offl, betas=d["betas"], fit_intercept=True,
                      center=d["c"], scale=d["s"], codes=cl, levels=d["levels"])
        calls = []
        orig = dist.all_reduce

        def spy(t, *a, **k):
            calls.append((t.is_cuda, dist.get_backend(), tuple(t.shape)))
            return orig(t, *a, **k)

        dist.all_reduce = spy
        try:
            tot = loglik_sharded(**kw)
        finally:
            dist.all_reduce = orig
        q.put((rank, tot, calls))
    finally:
        dist.destroy_process_group()


def _run_ranks(golden_dir, shards, layout, backend):
    import multiprocessing as mp
    import socket

    world = len(shards)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")  # children touch the GPU only after they start
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker,
                      args=(r, world, port, golden_dir, shards, layout, q, backend))
          for r in range(world)]
    for p_ in ps:
        p_.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p_ in ps:
        p_.join(timeout=60)
        assert p_.exitcode == 0
    return res


def _expected(golden_dir, layout):
    if layout == "dense":
        return np.load(os.path.join(golden_dir, "eval.npz"))["ll_noint_raw"].sum(0)
    return _case(4, (5, 7), True, True, 4, sizes=[1500, 1001, 700, 333], seed=3)["ref"].sum(0)


@pytest.mark.parametrize("layout", ["dense", "codes"])
def test_loglik_sharded_two_ranks_one_gpu(golden_dir, layout):
    res = _run_ranks(golden_dir, ([0, 2], [1, 3]), layout, "gloo")
    ref = _expected(golden_dir, layout)
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, tot, calls in res:
        assert calls == [(False, "gloo", (4,))], calls  # gloo reduces a host copy: one all_reduce
        assert np.abs(tot - ref).max() <= TOL * np.abs(ref).max()


def test_loglik_sharded_rccl_one_rank(golden_dir):
    """A one-rank "nccl" group: the all_reduce runs over RCCL on the device
    buffer of the B sums."""
    res = _run_ranks(golden_dir, ([0, 1, 2, 3],), "dense", "nccl")
    ref = _expected(golden_dir, "dense")
    (rank, tot, calls), = res
    assert calls == [(True, "nccl", (4,))], calls
    assert np.abs(tot - ref).max() <= TOL * np.abs(ref).max()
