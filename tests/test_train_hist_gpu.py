"""GBDT training kernels on the GPU (csrc/kernels/train_hist.hip): the level histograms and
the per-tree update against the float64 numpy oracle of test_train_hist_cpu.py, the library's
refusals, and ``train_oblivious_gbdt(hist="hip")`` end to end."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate
from test_train_hist_cpu import encode_rows, first_tree_ref, histograms_ref, leaves_ref

pytestmark = pytest.mark.gpu

F = 30
PROFILE_DIR = Path(__file__).resolve().parents[1] / "profiles" / "train_gbdt"
SIZES = [1, 63, 64, 65, 1000, 4097]


def _splits(B: int, d: int):
    """d splits: features 0 and 29 and bins 0 and B - 2 come first."""
    feats = [0, 29, 7, 29, 13, 0, 21]
    bins = [0, B - 2, (B - 1) // 2, 0, B - 2, B // 3, (2 * B) // 3]
    return [(f, min(max(b, 0), B - 2)) for f, b in zip(feats[:d], bins[:d])]


def _exact_inputs(n: int, B: int, seed: int):
    """grad = k / 256, k in [-128, 127]; hess = k / 256, k in [1, 128]: every partial sum over
    n <= 4097 rows is a multiple of 2^-8 below 2^12, exact in f32 in any order."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 32), np.uint8)
    rows[:, :F] = rng.integers(0, B, (n, F))
    grad = (rng.integers(-128, 128, n) / 256.0).astype(np.float32)
    hess = (rng.integers(1, 129, n) / 256.0).astype(np.float32)
    return rows, grad, hess


def _run_hist(gpu, rows, grad, hess, B, splits, out=None):
    from ccfd_demo_summit_amd.ops.kernels import gbdt_histogram
    G, H = gbdt_histogram(torch.from_numpy(rows).to(gpu), torch.from_numpy(grad).to(gpu),
                          torch.from_numpy(hess).to(gpu), B, splits, out=out)
    torch.cuda.synchronize()
    return G, H


def _assert_exact(G, H, rows, grad, hess, splits, B):
    G64, H64 = histograms_ref(rows, grad, hess, splits, B)
    assert G.shape == G64.shape and H.shape == H64.shape
    assert torch.equal(G.cpu(), torch.from_numpy(G64.astype(np.float32)))
    assert torch.equal(H.cpu(), torch.from_numpy(H64.astype(np.float32)))


# ---------------------------------------------------------------------- 1. exact histograms
@pytest.mark.parametrize("d", [0, 1, 3, 5, 7])
@pytest.mark.parametrize("B", [2, 32, 64])
def test_histogram_exact(gpu, B, d):
    splits = _splits(B, d)
    for n in SIZES:
        rows, grad, hess = _exact_inputs(n, B, seed=100 * B + 10 * d + n % 7)
        G, H = _run_hist(gpu, rows, grad, hess, B, splits)
        _assert_exact(G, H, rows, grad, hess, splits, B)


@pytest.mark.parametrize("B", [2, 32, 64])
def test_histogram_exact_single_split_on_last_feature(gpu, B):
    splits = [(29, B - 2)]
    rows, grad, hess = _exact_inputs(4097, B, seed=B)
    G, H = _run_hist(gpu, rows, grad, hess, B, splits)
    _assert_exact(G, H, rows, grad, hess, splits, B)


@pytest.mark.parametrize("B,d", [(32, 0), (64, 3), (2, 5)])
def test_histogram_exact_maximum_contention(gpu, B, d):
    """Every row of feature 4 (and of split feature 29) in bin B - 1: one LDS cell per leaf."""
    splits = _splits(B, d)
    rows, grad, hess = _exact_inputs(4097, B, seed=3)
    rows[:, 4] = B - 1
    rows[:, 29] = B - 1
    G, H = _run_hist(gpu, rows, grad, hess, B, splits)
    _assert_exact(G, H, rows, grad, hess, splits, B)
    assert float(G[:, 4, :B - 1].abs().sum()) == 0.0


def test_histogram_ignores_bytes_30_and_31(gpu):
    B, splits = 32, _splits(32, 3)
    rows, grad, hess = _exact_inputs(4097, B, seed=8)
    rows[:, 30:] = np.random.default_rng(1).integers(0, 256, (4097, 2))
    G, H = _run_hist(gpu, rows, grad, hess, B, splits)
    _assert_exact(G, H, rows, grad, hess, splits, B)


def test_histogram_overwrites_its_outputs(gpu):
    B, splits = 32, _splits(32, 3)
    rows, grad, hess = _exact_inputs(1000, B, seed=9)
    out = (torch.full((8, F, B), float("nan"), device=gpu), torch.full((8, F, B), float("nan"), device=gpu))
    G, H = _run_hist(gpu, rows, grad, hess, B, splits, out=out)
    assert G is out[0] and H is out[1]
    _assert_exact(G, H, rows, grad, hess, splits, B)


def test_histogram_skips_bins_past_the_table(gpu):
    """A bin byte >= B is a caller error: that (row, feature) is dropped, nothing else moves."""
    B, splits = 32, _splits(32, 1)
    rows, grad, hess = _exact_inputs(1000, B, seed=10)
    rows[::7, 12] = 200
    rows[::5, 3] = B
    G, H = _run_hist(gpu, rows, grad, hess, B, splits)
    _assert_exact(G, H, rows, grad, hess, splits, B)


# ------------------------------------------------------------------ 2. real-valued gradients
def test_histogram_real_gradients_within_summation_bound(gpu):
    """|G - G64| <= count * 2^-23 * sum|g| per bin: the any-order f32 summation bound
    ((count - 1) * 2^-24 * sum|g| to first order) with a factor 2 of slack for the two-stage
    sum (LDS inside a workgroup, global atomics across them)."""
    rng = np.random.default_rng(21)
    n, B, d = 20000, 32, 5
    rows = np.zeros((n, 32), np.uint8)
    rows[:, :F] = rng.integers(0, B, (n, F))
    p = 1 / (1 + np.exp(-2 * rng.standard_normal(n)))
    y = (rng.random(n) < 0.05).astype(np.float64)
    grad = (p - y).astype(np.float32)
    hess = np.maximum(p * (1 - p), 1e-6).astype(np.float32)
    splits = _splits(B, d)
    G, H = _run_hist(gpu, rows, grad, hess, B, splits)
    G64, H64 = histograms_ref(rows, grad, hess, splits, B)
    cnt, sabs_g = histograms_ref(rows, np.ones(n), np.abs(grad), splits, B)
    _, sabs_h = histograms_ref(rows, np.ones(n), np.abs(hess), splits, B)
    for got, ref, sabs, name in ((G, G64, sabs_g, "G"), (H, H64, sabs_h, "H")):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        bound = cnt * 2.0 ** -23 * sabs
        print(f"{name}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()


# ------------------------------------------------------------------------- 3. update kernel
@pytest.mark.parametrize("depth", [1, 8])
def test_update_leaf_index(gpu, depth):
    """leaf_val = 0, 1, 2, ... and raw = 0: raw afterwards IS the leaf index."""
    from ccfd_demo_summit_amd.ops.kernels import gbdt_apply_tree
    B = 32
    splits = (_splits(B, 7) + [(17, 11)])[:depth] if depth > 1 else [(29, B - 2)]
    rows, _, _ = _exact_inputs(4097, B, seed=depth)
    rows[:, 30:] = 255
    raw = torch.zeros(4097, device=gpu)
    leaf_val = torch.arange(1 << depth, dtype=torch.float32, device=gpu)
    out = gbdt_apply_tree(torch.from_numpy(rows).to(gpu), raw, leaf_val, splits)
    torch.cuda.synchronize()
    assert out[0] is raw and out[1] is None and out[2] is None          # NULL grad / hess accepted
    np.testing.assert_array_equal(raw.cpu().numpy().astype(np.int64), leaves_ref(rows, splits))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_update_raw_gradients_and_hessians(gpu, n):
    from ccfd_demo_summit_amd.ops.kernels import gbdt_apply_tree
    rng = np.random.default_rng(n)
    B, depth = 32, 6
    splits = _splits(B, depth)
    rows, _, _ = _exact_inputs(n, B, seed=n + 1)
    raw0 = (4 * rng.standard_normal(n)).astype(np.float32)
    raw0[: min(n, 4)] = np.array([-30.0, 30.0, 0.0, -88.0], np.float32)[: min(n, 4)]
    leaf_val = (0.3 * rng.standard_normal(1 << depth)).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    rt, yt = torch.from_numpy(rows).to(gpu), torch.from_numpy(y).to(gpu)
    raw = torch.from_numpy(raw0).to(gpu)
    lv = torch.from_numpy(leaf_val).to(gpu)
    leaf = torch.from_numpy(leaves_ref(rows, splits)).to(gpu)
    want_raw = torch.from_numpy(raw0).to(gpu) + lv[leaf]                 # one f32 add: exact
    _, grad, hess = gbdt_apply_tree(rt, raw, lv, splits, y=yt)
    torch.cuda.synchronize()
    assert torch.equal(raw, want_raw)

    z = want_raw.cpu().numpy().astype(np.float64)
    p64 = 1 / (1 + np.exp(-z))
    g64, h64 = p64 - y, np.maximum(p64 * (1 - p64), 1e-6)
    pt = torch.sigmoid(want_raw)                                          # torch's own f32 path
    E_g = float(np.abs((pt - yt).cpu().numpy().astype(np.float64) - g64).max())
    E_h = float(np.abs((pt * (1 - pt)).clamp_min(1e-6).cpu().numpy().astype(np.float64) - h64).max())
    err_g = float(np.abs(grad.cpu().numpy().astype(np.float64) - g64).max())
    err_h = float(np.abs(hess.cpu().numpy().astype(np.float64) - h64).max())
    rec = {"n": n, "torch_f32_err_grad": E_g, "torch_f32_err_hess": E_h, "kernel_err_grad": err_g,
           "kernel_err_hess": err_h, "floor": 2.0 ** -22}
    print(json.dumps(rec))
    if n == 4097:
        try:
            PROFILE_DIR.mkdir(parents=True, exist_ok=True)
            (PROFILE_DIR / "update_error.json").write_text(json.dumps(rec, indent=1) + "\n")
        except OSError:
            pass
    assert err_g <= max(4 * E_g, 2.0 ** -22)
    assert err_h <= max(4 * E_h, 2.0 ** -22)


# ------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("level,B,n,word", [(8, 32, 100, "level"), (3, 65, 100, "n_bins"), (3, 1, 100, "n_bins"),
                                            (3, 32, 0, "n < 1")])
def test_histogram_refusals(gpu, level, B, n, word):
    """Refused on the host with a negative code and a message; nothing is launched, so the
    NaN-filled outputs stay as they are."""
    from ccfd_demo_summit_amd.ops._lib import GbdtHistArgs, last_error, lib
    rows = torch.zeros((100, 32), dtype=torch.uint8, device=gpu)
    g = torch.ones(100, device=gpu)
    G = torch.full((256 * F * 65,), float("nan"), device=gpu)
    H = torch.full((256 * F * 65,), float("nan"), device=gpu)
    a = GbdtHistArgs()
    a.rows, a.grad, a.hess, a.G, a.H = rows.data_ptr(), g.data_ptr(), g.data_ptr(), G.data_ptr(), H.data_ptr()
    a.n, a.n_bins, a.level = n, B, level
    rc = lib().ccfd_gbdt_hist_launch(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc < 0
    assert word in last_error()
    assert bool(torch.isnan(G).all()) and bool(torch.isnan(H).all())


def test_wrappers_check_their_tensors(gpu):
    from ccfd_demo_summit_amd.ops.kernels import gbdt_apply_tree, gbdt_histogram
    rows = torch.zeros((10, 32), dtype=torch.uint8, device=gpu)
    g = torch.ones(10, device=gpu)
    with pytest.raises(ValueError, match="G32"):
        gbdt_histogram(rows.cpu(), g, g, 32)
    with pytest.raises(ValueError, match="G32"):
        gbdt_histogram(rows[:, :30], g, g, 32)
    with pytest.raises(ValueError, match="grad"):
        gbdt_histogram(rows, g.double(), g, 32)
    with pytest.raises(ValueError, match="hess"):
        gbdt_histogram(rows, g, g[:9], 32)
    with pytest.raises(RuntimeError, match="n_bins"):
        gbdt_histogram(rows, g, g, 65)
    with pytest.raises(ValueError, match="leaf_val"):
        gbdt_apply_tree(rows, g, torch.zeros(3, device=gpu), [(0, 0), (1, 1)])
    with pytest.raises(RuntimeError, match="depth"):
        gbdt_apply_tree(rows, g, torch.zeros(1, device=gpu), [])


# ---------------------------------------------------------------------------- 5. end to end
@pytest.fixture(scope="module")
def e2e_data():
    X, y = generate(20000, seed=1, fraud_rate=0.02)
    Xv, yv = generate(10000, seed=2, fraud_rate=0.02)
    return np.asarray(X, np.float32), np.asarray(y), np.asarray(Xv, np.float32), np.asarray(yv)


def test_train_hip_end_to_end(gpu, e2e_data):
    """The f32 histograms pick tree 0's splits of the float64 oracle.  That rests on the typical
    f32 error of a bin sum, about sqrt(n) * 2^-24 ~ 1e-5 relative, against leads >= 1e-3 (asserted
    below as a condition on this input) -- not on the worst-case summation bound, which is of
    the order of the smallest lead."""
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, score
    from ccfd_demo_summit_amd.train import evaluate, train_oblivious_gbdt
    from ccfd_demo_summit_amd.train.trainer import _quantile_borders
    X, y, Xv, yv = e2e_data
    borders = _quantile_borders(X, 32)
    splits, leads = first_tree_ref(encode_rows(X, borders), y, 6, 32)
    assert min(leads) >= 1e-3, leads

    m, info = train_oblivious_gbdt(X, y, n_trees=5, depth=6, n_bins=32, hist="hip", device="cuda")
    assert info["hist"] == "hip"
    assert evaluate(m, Xv, yv)["roc_auc"] > 0.9
    assert [int(f) for f in m.feat[0]] == [f for f, _ in splits]
    np.testing.assert_array_equal(m.thr[0], np.array([borders[f, b] for f, b in splits], np.float32))

    p, _ = score(DeviceModel(m, gpu), torch.from_numpy(Xv).to(gpu), 0.5)
    torch.cuda.synchronize()
    assert np.abs(p.cpu().numpy() - m.predict_proba(Xv)).max() < 1e-5


def test_train_auto_picks_hip_on_the_gpu(gpu, e2e_data):
    from ccfd_demo_summit_amd.train import train_oblivious_gbdt
    X, y, _, _ = e2e_data
    _, info = train_oblivious_gbdt(X[:4097], y[:4097], n_trees=1, depth=3, hist="auto", device="cuda")
    assert info["hist"] == "hip"
    _, info = train_oblivious_gbdt(X[:4097], y[:4097], n_trees=1, depth=3, n_bins=128, hist="auto", device="cuda")
    assert info["hist"] == "torch"
    with pytest.raises(ValueError, match="64"):
        train_oblivious_gbdt(X[:4097], y[:4097], n_trees=1, depth=3, n_bins=128, hist="hip", device="cuda")


# ------------------------------------------------------------------ 6. torch path unchanged
def test_train_torch_path_on_the_gpu(gpu, e2e_data):
    from ccfd_demo_summit_amd.train import evaluate, train_oblivious_gbdt
    X, y, Xv, yv = e2e_data
    m, info = train_oblivious_gbdt(X, y, n_trees=5, depth=6, n_bins=32, hist="torch", device="cuda")
    assert info["hist"] == "torch"
    assert evaluate(m, Xv, yv)["roc_auc"] > 0.9
    m2, info2 = train_oblivious_gbdt(X, y, n_trees=5, depth=6, n_bins=32, device="cuda")
    assert info2["hist"] == "torch" and m2.feat.shape == m.feat.shape
