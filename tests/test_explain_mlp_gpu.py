"""csrc/kernels/explain_mlp.hip against models/explain_mlp.py.

The kernel is checked in three separable steps, none with a tuned number:

* bookkeeping, exact: ``recombine(z_out, table, float32)``, the documented order of the sum on the
  kernel's own coalition logits, equals the kernel's ``phi`` bit for bit (masks, permutations,
  shuffles and accumulation, apart from MLP numerics);
* numerics: ``sigmoid(z_out)`` against ``sigmoid`` of the oracle's coalition logits
  (``shapley_mlp_table``, i.e. ``MLPModel.wire_logits`` of every masked row) within 2e-4, the bound
  tests/test_kernels_gpu.py holds this MFMA chain to against ``wire_proba``;
* end to end: ``|phi - oracle phi| <= 2 max|z_out - z_oracle| + (P + 2) 2^-24 max|d|``.  The first
  term is the triangle inequality on ``d = z[k+1] - z[k]`` averaged over ``P``; the second is the
  float32 rounding of one difference, ``P`` additions and one division (first-order bound
  ``(P + 1) u max|d|``, ``u = 2^-24``).

Measured on one MI355X (the tests print their figures): ``sigmoid`` differences 3.7e-9 .. 8.3e-5
(largest: 67 rows, P = 64), ``|z_out - z_oracle|`` up to 3.4e-4, ``|phi - oracle phi|`` 4.7e-9 ..
6.0e-6 against bounds of 4.3e-8 .. 6.7e-4.
"""
import ctypes as C

import numpy as np
import pytest

from test_explain_mlp_cpu import integer_rows, linear_case, mlp_case, rows, sparse_rows, two_feature_closed_form

from ccfd_demo_summit_amd.contracts.transaction import WIRE_PERM, encode_wire
from ccfd_demo_summit_amd.models import build_model
from ccfd_demo_summit_amd.models.explain_mlp import (MlpExplainTable, mlp_base_value, recombine, shapley_mlp_table)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

# name -> (log_amount, P, n): under, at and over one workgroup's four rows, a strided tail
CASES = {"n1": (True, 64, 1), "n3": (True, 2, 3), "n4": (False, 64, 4), "n5": (True, 256, 5),
         "n67": (True, 64, 67), "n67_raw_p2": (False, 2, 67)}
_MODELS, _INPUT, _ORACLE, _EX, _RUN = {}, {}, {}, {}, {}


def model(log_amount):
    if log_amount not in _MODELS:
        _MODELS[log_amount] = mlp_case(log_amount)
    return _MODELS[log_amount]


def inputs(name):
    """float32 [n,30]: dataset rows; every third row differs from the baseline in 5 features only."""
    if name not in _INPUT:
        la, P, n = CASES[name]
        X = rows()[200:200 + n].copy()
        sp = sparse_rows(model(la), 5, n, seed=n)
        X[::3] = sp[::3]
        X.setflags(write=False)
        _INPUT[name] = X
    return _INPUT[name]


def oracle(name):
    """(table bytes, unpacked table, phi float64 [n,30], z float32 [n,P,32]) of a case, computed once."""
    if name not in _ORACLE:
        la, P, n = CASES[name]
        blob = MlpExplainTable.pack(model(la), P, seed=P + n)
        phi, z = shapley_mlp_table(model(la), blob, encode_wire(inputs(name)))
        phi.setflags(write=False)
        z.setflags(write=False)
        _ORACLE[name] = (blob, MlpExplainTable.unpack(blob), phi, z)
    return _ORACLE[name]


def explainer(gpu, name):
    from ccfd_demo_summit_amd.ops.kernels import DeviceMlpExplainer
    if name not in _EX:
        la, P, n = CASES[name]
        _EX[name] = DeviceMlpExplainer(model(la), perms=P, seed=P + n, device=gpu)
    return _EX[name]


def launch(gpu, ex, X, **kw):
    import torch
    from ccfd_demo_summit_amd.ops.kernels import explain_mlp
    xw = torch.from_numpy(encode_wire(np.asarray(X, np.float32))).to(gpu)
    z = torch.full((len(X), ex.perms, 32), float("nan"), dtype=torch.float32, device=gpu)
    phi = explain_mlp(ex, xw, z_out=z, **kw)
    torch.cuda.synchronize()
    return phi.cpu().numpy(), z.cpu().numpy()


def run(gpu, name, max_workgroups=None):
    key = (name, max_workgroups)
    if key not in _RUN:
        kw = {} if max_workgroups is None else {"max_workgroups": max_workgroups}
        _RUN[key] = launch(gpu, explainer(gpu, name), inputs(name), **kw)
    return _RUN[key]


def rounding_term(z, P):
    """(P + 2) u max|d| of a run's own coalition logits (module docstring)."""
    return (P + 2) * U * np.abs(np.diff(z.astype(np.float64), axis=2)).max()


@pytest.mark.parametrize("mwg", [None, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_bookkeeping_is_exact(gpu, name, mwg):
    phi, z = run(gpu, name, mwg)
    assert np.isfinite(z).all() and np.isfinite(phi).all()
    assert (z[:, :, 30] == z[:, :, 31]).all()
    np.testing.assert_array_equal(phi, recombine(z, oracle(name)[1], np.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_coalition_logits_within_the_chain_s_bound(gpu, name):
    _, z = run(gpu, name)
    zo = oracle(name)[3]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v.astype(np.float64)))
    dp, dz = np.abs(sig(z) - sig(zo)).max(), np.abs(z - zo).max()
    print(f"{name}: max |sigmoid(z_out) - sigmoid(z_oracle)| {dp:.3g}, max |z_out - z_oracle| {dz:.3g}")
    assert dp < 2e-4


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end_against_the_oracle(gpu, name):
    phi, z = run(gpu, name)
    _, _, phio, zo = oracle(name)
    P = CASES[name][1]
    bound = 2.0 * np.abs(z.astype(np.float64) - zo).max() + rounding_term(z, P)
    err = np.abs(phi - phio).max()
    print(f"{name}: max |phi - oracle phi| {err:.3g}, bound {bound:.3g}, max |phi| {np.abs(phio).max():.3g}")
    assert err <= bound


@pytest.mark.parametrize("name", list(CASES))
def test_efficiency_and_dummies(gpu, name):
    phi, z = run(gpu, name)
    la, P, n = CASES[name]
    m, X = model(la), inputs(name)
    want = z[:, 0, 30].astype(np.float64) - z[:, 0, 0]
    assert (z[:, :, 0] == z[:, :1, 0]).all() and (z[:, :, 30] == z[:, :1, 30]).all()
    # 30 float32 attributions, each within the rounding term of its exact sum
    assert np.abs(phi.astype(np.float64).sum(1) - want).max() <= 30 * rounding_term(z, P)
    same = encode_wire(X).view(np.uint16) == encode_wire(m.baseline[None]).view(np.uint16)
    same_feat = np.empty((n, 30), bool)
    same_feat[:, WIRE_PERM[:28]] = same[:, :28]
    same_feat[:, 0] = same[:, 28] & same[:, 29]
    same_feat[:, 29] = same[:, 30] & same[:, 31]
    assert same_feat[::3].sum() >= 25 * len(X[::3])
    assert (phi[same_feat] == 0.0).all() and not np.signbit(phi[same_feat]).any()
    assert (phi[~same_feat] != 0.0).mean() > 0.9


def test_exact_linear_case(gpu):
    from ccfd_demo_summit_amd.ops.kernels import DeviceMlpExplainer
    m, w = linear_case()
    X = integer_rows(9)
    ex = DeviceMlpExplainer(m, perms=64, seed=0, device=gpu)
    phi, z = launch(gpu, ex, X)
    np.testing.assert_array_equal(z[:, :, 30], np.broadcast_to((X @ w + 2.0)[:, None], (9, 64)))
    np.testing.assert_array_equal(z[:, :, 0], np.full((9, 64), m.baseline @ w + 2.0, np.float32))
    np.testing.assert_array_equal(phi, w[None, :] * (X - m.baseline[None, :]))
    assert ex.base_value == float(m.baseline @ w + 2.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_feature_rows_match_their_closed_form(gpu, seed):
    from ccfd_demo_summit_amd.ops.kernels import DeviceMlpExplainer
    m = model(True)
    X = sparse_rows(m, 2, 6, seed=20 + seed)
    ex = DeviceMlpExplainer(m, perms=64, seed=seed, device=gpu)
    phi, z = launch(gpu, ex, X)
    t = MlpExplainTable.unpack(MlpExplainTable.pack(m, 64, seed))
    wire_of = np.argsort(WIRE_PERM)                                       # canonical feature -> wire position
    for i, x in enumerate(X):
        fa, fb = np.nonzero(x != m.baseline)[0]
        a, b = wire_of[fa], wire_of[fb]
        p = 0 if t.inv[0, a] < t.inv[0, b] else 1                         # a permutation with a before b
        v00, vab = z[i, 0, 0], z[i, 0, 30]
        va, vb = z[i, p, t.inv[p, a] + 1], z[i, p ^ 1, t.inv[p ^ 1, b] + 1]
        assert set(np.unique(z[i])) <= {v00, va, vb, vab}                 # four coalition rows, four logits
        pa, pb = two_feature_closed_form(*(float(v) for v in (v00, va, vb, vab)))
        tol = rounding_term(z[i:i + 1], 64)
        assert abs(phi[i, fa] - pa) <= tol and abs(phi[i, fb] - pb) <= tol
        assert np.count_nonzero(phi[i]) == np.count_nonzero([pa, pb])


def test_reproducible_and_independent_of_the_batch(gpu):
    import torch
    from ccfd_demo_summit_amd.ops.kernels import explain_mlp
    name = "n67"
    ex, X = explainer(gpu, name), inputs(name)
    phi, z = run(gpu, name)
    for mwg in (1, 3):
        again, zagain = run(gpu, name, mwg)
        np.testing.assert_array_equal(again, phi)
        np.testing.assert_array_equal(zagain, z)
    second, _ = launch(gpu, ex, X)
    np.testing.assert_array_equal(second, phi)
    for i in (0, 5, 66):
        alone, zal = launch(gpu, ex, X[i:i + 1])
        np.testing.assert_array_equal(alone[0], phi[i])
        np.testing.assert_array_equal(zal[0], z[i])
    # out= and a side stream, without z_out
    xw = torch.from_numpy(encode_wire(X)).to(gpu)
    out = torch.full((67, 30), float("nan"), dtype=torch.float32, device=gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    assert explain_mlp(ex, xw, out=out, stream=side) is out
    side.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), phi)
    host, bv = ex.explain(X)
    np.testing.assert_array_equal(host, phi)
    assert bv == mlp_base_value(model(True))


def test_python_argument_checks(gpu):
    import torch
    from ccfd_demo_summit_amd.ops.kernels import DeviceExplainer, DeviceMlpExplainer, explain_mlp
    ex = explainer(gpu, "n3")
    xw = torch.from_numpy(encode_wire(inputs("n3"))).to(gpu)
    with pytest.raises(ValueError, match="W64 rows"):
        explain_mlp(ex, xw.cpu())
    with pytest.raises(ValueError, match="W64 rows"):
        explain_mlp(ex, xw[:, :32].contiguous())
    with pytest.raises(ValueError, match="out must be"):
        explain_mlp(ex, xw, out=torch.empty((3, 31), dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="z_out must be"):
        explain_mlp(ex, xw, z_out=torch.empty((3, 4, 32), dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="DeviceMlpExplainer"):
        explain_mlp(object(), xw)
    with pytest.raises(ValueError, match="fit_baseline"):
        DeviceMlpExplainer(build_model("mlp", seed=0), device=gpu)
    with pytest.raises(ValueError, match="P must be"):
        DeviceMlpExplainer(model(True), perms=3, device=gpu)
    with pytest.raises(ValueError, match="MLP only"):
        DeviceMlpExplainer(build_model("lr", seed=0), device=gpu)
    with pytest.raises(ValueError, match="no explain kernel"):
        DeviceExplainer(model(True), device=gpu)                          # the tree explainer stays as it is
    assert explain_mlp(ex, xw[:0]).shape == (0, 30)


def test_launcher_refusals(gpu):
    import torch
    from ccfd_demo_summit_amd.ops._lib import MlpExplainArgs, last_error, lib
    ex = explainer(gpu, "n3")
    xw = torch.from_numpy(encode_wire(inputs("n3"))).to(gpu)
    odd = torch.zeros(3 * 64 + 16, dtype=torch.uint8, device=gpu)
    phi = torch.full((3, 30), -7.0, dtype=torch.float32, device=gpu)
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def args(**kw):
        a = MlpExplainArgs()
        a.rows, a.blob, a.table, a.phi, a.z_out = xw.data_ptr(), ex.blob.data_ptr(), ex.table.data_ptr(), phi.data_ptr(), None
        a.n, a.table_bytes, a.blob_bytes, a.perms, a.max_workgroups = 3, ex.table.numel(), ex.blob.numel(), ex.perms, 8
        a.table_head[0], a.table_head[1] = ex.table_head
        for k, v in kw.items():
            if k == "table_head":
                a.table_head[0], a.table_head[1] = v
            else:
                setattr(a, k, v)
        return a

    bad = {"n < 0": dict(n=-1), "null rows": dict(rows=None), "null blob": dict(blob=None),
           "null table": dict(table=None), "null phi": dict(phi=None),
           "rows off 16 bytes": dict(rows=odd.data_ptr() + 8),
           "perms odd": dict(perms=3, table_bytes=128 + 160 * 3, table_head=(ex.table_head[0], 3)),
           "perms < 2": dict(perms=0, table_bytes=128, table_head=(ex.table_head[0], 0)),
           "perms > 256": dict(perms=258, table_bytes=128 + 160 * 258, table_head=(ex.table_head[0], 258)),
           "magic": dict(table_head=(0x31584c4e, ex.perms)),
           "table P": dict(table_head=(ex.table_head[0], ex.perms + 2)),
           "table length": dict(table_bytes=ex.table.numel() - 16),
           "perms against the table": dict(perms=ex.perms + 2),
           "blob length": dict(blob_bytes=ex.blob.numel() - 2048),
           "max_workgroups < 1": dict(max_workgroups=0)}
    for what, kw in bad.items():
        rc = lib().ccfd_mlp_explain_launch(C.byref(args(**kw)), stream)
        assert rc != 0, what
        assert last_error().startswith("mlp explain:"), what
    torch.cuda.synchronize()
    assert (phi == -7.0).all()
    assert lib().ccfd_mlp_explain_launch(C.byref(args(n=0)), stream) == 0
    assert lib().ccfd_mlp_explain_launch(C.byref(args(n=0, rows=None, phi=None)), stream) == 0
    torch.cuda.synchronize()
    assert (phi == -7.0).all()
    assert lib().ccfd_mlp_explain_launch(C.byref(args()), stream) == 0     # and the same arguments, whole, run
    torch.cuda.synchronize()
    np.testing.assert_array_equal(phi.cpu().numpy(), run(gpu, "n3")[0])


def test_gpu_scorer_explains_mlp_and_lr(gpu):
    from ccfd_demo_summit_amd.models.explain_mlp import shapley_lr
    from ccfd_demo_summit_amd.ops.kernels import DeviceMlpExplainer
    from ccfd_demo_summit_amd.serving import GpuScorer
    m, X = model(True), inputs("n5")
    sc = GpuScorer(m, max_batch=256)
    try:
        phi, bv = sc.explain(X)
        want, wbv = DeviceMlpExplainer(m, perms=64, seed=0, device=gpu).explain(X)
        np.testing.assert_array_equal(phi, want)
        assert bv == wbv == mlp_base_value(m)
        p, _ = sc.score(X)
        assert np.abs(1.0 / (1.0 + np.exp(-(bv + phi.astype(np.float64).sum(1)))) - p).max() < 1e-2
    finally:
        sc.close()
    lr = build_model("lr", seed=2, X_ref=rows(), calibrate_rate=0.01)
    for plain in (build_model("mlp", seed=0, X_ref=rows()), lr):
        sc = GpuScorer(plain, max_batch=256)
        try:
            with pytest.raises(ValueError, match="no explanation.*fit_baseline"):
                sc.explain(X)
        finally:
            sc.close()
    sc = GpuScorer(lr.fit_baseline(rows()), max_batch=256)
    try:
        np.testing.assert_array_equal(sc.explain(X)[0], shapley_lr(sc.model, X)[0])
    finally:
        sc.close()
