"""csrc/kernels/explain_forest.hip against the float64 oracle (models/explain_forest.py).

Tolerance.  Errors are in units u = 2^-24 * sum_t max |leaf_t| of each case's ensemble, as in
tests/test_explain_gpu.py.  The constants do not come from the kernel: the emulator of its
algorithm (``table_shapley_forest(..., dtype=np.float32)``) was run on the CPU on exactly the
inputs of ``CASES`` below, and its worst error against the float64 oracle is MEASURED_PHI_U for
one attribution and MEASURED_LOCAL_U for local accuracy (base_value + sum_j phi_j against the
float64 raw score); the kernel is allowed 4x each, because its association order (fused
multiply-adds) differs from the emulator's.
Measured: 3.360 u (chain_16; 0.11 u for oblivious_100x6, 0.31 u for slices, at most 0.50 u for the
others) and 3.748 u (chain_16; at most 0.73 u for the others), so the bounds are 13.48 u and 15.00 u.
Features that are no player of any path and stale rows are compared exactly (0.0 and NaN).
"""
import numpy as np
import pytest

from test_explain_forest_cpu import forest_unit, gpu_cases, player_features

from ccfd_demo_summit_amd.models.explain_forest import shapley_forest

MEASURED_PHI_U = 3.37     # worst |phi_f32 - phi_f64| / u of the float32 emulator over CASES
MEASURED_LOCAL_U = 3.75   # worst |base_value + sum_j phi_f32 - raw_f64| / u over CASES
TOL_PHI_U = 4 * MEASURED_PHI_U
TOL_LOCAL_U = 4 * MEASURED_LOCAL_U

CASES = gpu_cases()
_ORACLE = {}


def oracle(name):
    """(rows u8 [n,32], phi float64 [n,30], base_value, raw float64 [n]) of a case, computed once."""
    if name not in _ORACLE:
        m, spec, X = CASES[name]
        rows = spec.encode(X)
        phi, bv = shapley_forest(m, rows, bins=spec)
        phi.setflags(write=False)
        raw = m.base + m.value[m.leaf_node_binned(rows, spec)].astype(np.float64).sum(1)
        _ORACLE[name] = (rows, phi, bv, raw)
    return _ORACLE[name]


def check(name, got, rows_ok=None):
    m = CASES[name][0]
    _rows, phi, bv, raw = oracle(name)
    sel = slice(None) if rows_ok is None else rows_ok
    got = np.asarray(got, np.float64)[sel]
    u = forest_unit(m)
    err = np.abs(got - phi[sel]).max() / u
    loc = np.abs(bv + got.sum(1) - raw[sel]).max() / u
    print(f"{name}: max |phi_gpu - phi_f64| = {err:.3f} u, local accuracy {loc:.3f} u")
    unused = np.setdiff1d(np.arange(30), player_features(m))
    assert (got[:, unused] == 0.0).all()
    assert err <= TOL_PHI_U and loc <= TOL_LOCAL_U


def run(name, gpu, **kw):
    import torch
    from ccfd_demo_summit_amd.ops.kernels import DeviceExplainer, explain_forest
    m, spec, _X = CASES[name]
    ex = DeviceExplainer(m, bins=spec, device=gpu)
    rows = torch.from_numpy(oracle(name)[0]).to(gpu)
    return ex, rows, explain_forest(ex, rows, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_matches_oracle(gpu, name):
    ex, _rows, phi = run(name, gpu)
    check(name, phi.cpu().numpy())
    if name in ("slices", "oblivious_100x6"):
        assert ex.slices >= 2
    if name == "chain_16":
        assert ex.width == 16
    if name == "odd_7_trees":
        assert ex.trees == 7 and ex.paths % 4 != 0


@pytest.mark.gpu
def test_expanded_oblivious_model_agrees_with_explain_gbdt(gpu):
    """The 100 x 6 model: the forest kernel on its expansion and the oblivious kernel on the model
    itself explain the same rows; each is within its own bound of the same float64 values."""
    import torch
    from test_explain_cpu import random_case, unit
    from test_explain_gpu import TOL_PHI_U as TOL_GBDT_U
    from ccfd_demo_summit_amd.ops.kernels import DeviceExplainer, explain_forest, explain_gbdt
    _ex, rows, phi = run("oblivious_100x6", gpu)
    obl = random_case(100, 6, seed=606)
    exg = DeviceExplainer(obl, bins=CASES["oblivious_100x6"][1], device=gpu)
    other = explain_gbdt(exg, rows)
    assert unit(obl) == forest_unit(CASES["oblivious_100x6"][0])
    assert (phi - other).abs().max().item() <= (TOL_PHI_U + TOL_GBDT_U) * unit(obl)
    assert abs(exg.base_value - oracle("oblivious_100x6")[2]) < 1e-12
    with pytest.raises(ValueError, match="explain_forest"):
        explain_gbdt(_ex, rows)
    with pytest.raises(ValueError, match="explain_gbdt"):
        explain_forest(exg, rows)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_no_rows(gpu):
    import torch
    from ccfd_demo_summit_amd.ops.kernels import DeviceExplainer, explain_forest
    m, spec, _ = CASES["slices"]
    phi = explain_forest(DeviceExplainer(m, bins=spec, device=gpu), torch.empty((0, 32), dtype=torch.uint8, device=gpu))
    assert tuple(phi.shape) == (0, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse_d8", "slices"])            # one slice; slices on grid.y
def test_stale_row_is_nan_and_the_rest_untouched(gpu, name):
    import torch
    from ccfd_demo_summit_amd.ops.kernels import explain_forest
    ex, rows, clean = run(name, gpu)
    bad = rows.clone()
    bad[37, 31] = bad[37, 31] ^ 0x5a
    phi = explain_forest(ex, bad).cpu().numpy()
    assert np.isnan(phi[37]).all()
    keep = np.arange(65) != 37
    assert not np.isnan(phi[keep]).any() and (phi[keep] == clean.cpu().numpy()[keep]).all()
    check(name, phi, rows_ok=keep)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse_d8", "slices"])
def test_a_row_alone_gets_the_bits_of_the_batch(gpu, name):
    """Row 37 alone, in its batch of 65, and in the smallest batch (256 workgroups) whose slices
    are walked inside one workgroup instead of on grid.y: the same bits."""
    import torch
    from ccfd_demo_summit_amd.ops._lib import lib
    from ccfd_demo_summit_amd.ops.kernels import explain_forest
    ex, rows, batch = run(name, gpu)
    alone = explain_forest(ex, rows[37:38].clone())
    assert torch.equal(alone.view(torch.int32)[0], batch.view(torch.int32)[37])
    big_n = 255 * 64 + 1
    assert lib().ccfd_forest_explain_workspace_bytes(big_n, ex.slices) == 0
    assert (lib().ccfd_forest_explain_workspace_bytes(big_n - 1, ex.slices) > 0) == (ex.slices > 1)
    idx = torch.arange(big_n, device=gpu) % 65
    big = explain_forest(ex, rows[idx].contiguous())
    assert torch.equal(big.view(torch.int32), batch.view(torch.int32)[idx])


@pytest.mark.gpu
def test_bit_reproducible_out_and_stream(gpu):
    import torch
    from ccfd_demo_summit_amd.ops.kernels import explain_forest
    ex, rows, first = run("rows_257", gpu)
    again = explain_forest(ex, rows)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    ex2, rows2, first2 = run("slices", gpu)
    out = torch.full((65, 30), 7.0, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    got = explain_forest(ex2, rows2, out=out, stream=side)
    side.synchronize()
    assert got is out and torch.equal(out.view(torch.int32), first2.view(torch.int32))
    assert len(ex2._workspace) == 2                           # one partial-sum buffer a stream
    with pytest.raises(ValueError):
        explain_forest(ex, rows, out=torch.empty((257, 29), device=gpu))
    with pytest.raises(ValueError):
        explain_forest(ex, rows.cpu())
    with pytest.raises(ValueError):
        explain_forest(ex, rows[:, :30])


@pytest.mark.gpu
def test_device_explainer_on_feature_rows(gpu):
    from ccfd_demo_summit_amd.ops.kernels import DeviceExplainer
    m, _spec, X = CASES["odd_7_trees"]
    phi, bv = DeviceExplainer(m, device=gpu).explain(X)
    want, bv64 = shapley_forest(m, X)
    u = forest_unit(m)
    assert phi.dtype == np.float32 and phi.shape == (65, 30) and bv == bv64
    assert np.abs(phi - want).max() <= TOL_PHI_U * u
    raw = m.base + m.leaf_values(X).astype(np.float64).sum(1)
    assert np.abs(bv + phi.astype(np.float64).sum(1) - raw).max() <= TOL_LOCAL_U * u
    with pytest.raises(ValueError, match="fit_cover"):
        from ccfd_demo_summit_amd.models.forest import TreeEnsemble
        DeviceExplainer(TreeEnsemble(m.feat, m.value, m.child, m.leaf, m.root), device=gpu)


@pytest.mark.gpu
def test_gpu_scorer_explains_a_forest_through_the_kernel(gpu):
    from ccfd_demo_summit_amd.serving.scorers import GpuScorer
    m, _spec, X = CASES["odd_7_trees"]
    sc = GpuScorer(m, max_batch=256)
    try:
        phi, bv = sc.explain(X)
        again, _ = sc.explain(X[:7])                      # the uploaded table is reused
    finally:
        sc.close()
    want, bv64 = shapley_forest(m, X)
    assert bv == bv64 and phi.dtype == np.float32
    assert np.abs(phi - want).max() <= TOL_PHI_U * forest_unit(m) and (again == phi[:7]).all()


@pytest.mark.gpu
def test_launch_refuses_bad_arguments(gpu):
    import ctypes as C
    import torch
    from ccfd_demo_summit_amd.ops._lib import ForestExplainArgs, last_error, lib
    ex, rows, phi = run("slices", gpu)
    s = torch.cuda.current_stream(gpu)
    sp = C.c_void_p(s.cuda_stream)
    ws = ex.workspace(rows.shape[0], s)

    def args(**kw):
        a = ForestExplainArgs()
        a.rows, a.blob, a.phi, a.workspace = rows.data_ptr(), ex.blob.data_ptr(), phi.data_ptr(), ws.data_ptr()
        a.n, a.blob_bytes, a.workspace_bytes = rows.shape[0], ex.blob.numel(), ws.numel() * 4
        a.paths, a.width, a.slices, a.rec_words = ex.paths, ex.width, ex.slices, ex.rec_words
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw, word in ((dict(width=5), "width"), (dict(width=20), "width"), (dict(slices=0), "slices"),
                     (dict(slices=17), "slices"), (dict(paths=-1), "paths"), (dict(rec_words=-1), "rec_words"),
                     (dict(n=-1), "n < 0"), (dict(rec_words=ex.rec_words + 64), "blob"),
                     (dict(blob_bytes=ex.blob.numel() - 16), "blob"), (dict(rows=rows.data_ptr() + 8), "aligned"),
                     (dict(blob=ex.blob.data_ptr() + 8), "aligned"), (dict(phi=None), "null"),
                     (dict(workspace=None), "workspace"), (dict(workspace_bytes=ws.numel() * 4 - 4), "workspace")):
        assert lib().ccfd_forest_explain_launch(C.byref(args(**kw)), sp) != 0
        assert word in last_error()
    assert lib().ccfd_forest_explain_launch(None, sp) != 0 and "null" in last_error()
    assert lib().ccfd_forest_explain_launch(C.byref(args()), sp) == 0
    assert lib().ccfd_forest_explain_launch(C.byref(args(n=0, rows=None, phi=None)), sp) == 0
    torch.cuda.synchronize()
