"""GBDT training on G32 rows, host side: the ABI mirrors of the two training launches, the
native encoder as the trainer's binning, the ``hist=`` switch of ``train_oblivious_gbdt`` and
the float64 numpy oracle the GPU tests (test_train_hist_gpu.py) compare the kernels with."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate

F = 30


# ------------------------------------------------------------------ float64 oracle (shared)
def leaves_ref(rows: np.ndarray, splits) -> np.ndarray:
    """leaf(i) = sum_k (rows[i, feat_k] > bin_k) << k  (the bit order of the trainer)."""
    leaf = np.zeros(len(rows), np.int64)
    for k, (f, b) in enumerate(splits):
        leaf |= (rows[:, f].astype(np.int64) > b).astype(np.int64) << k
    return leaf


def histograms_ref(rows: np.ndarray, grad: np.ndarray, hess: np.ndarray, splits, B: int):
    """float64 (G, H), each [2^d, 30, B]: G[leaf(i), f, rows[i, f]] += grad[i].  Bytes 30 / 31 of a
    row are ignored; a bin byte >= B is skipped."""
    L = 1 << len(splits)
    bins = rows[:, :F].astype(np.int64)
    key = (leaves_ref(rows, splits)[:, None] * F + np.arange(F)[None, :]) * B + bins
    ok = (bins < B).reshape(-1)
    key = key.reshape(-1)[ok]
    out = []
    for v in (grad, hess):
        w = np.repeat(np.asarray(v, np.float64), F)[ok]
        out.append(np.bincount(key, weights=w, minlength=L * F * B).reshape(L, F, B))
    return out[0], out[1]


def best_split_ref(G: np.ndarray, H: np.ndarray, l2: float):
    """The trainer's gain scan in float64: ((feature, bin), best gain, runner-up gain)."""
    Gl, Hl = G.cumsum(-1)[..., :-1], H.cumsum(-1)[..., :-1]
    Gt, Ht = G.sum(-1, keepdims=True), H.sum(-1, keepdims=True)
    Gr, Hr = Gt - Gl, Ht - Hl
    gain = (Gl ** 2 / (Hl + l2) + Gr ** 2 / (Hr + l2) - Gt ** 2 / (Ht + l2)).sum(0)
    order = np.argsort(gain.reshape(-1))
    f, b = divmod(int(order[-1]), G.shape[-1] - 1)
    return (f, b), float(gain.reshape(-1)[order[-1]]), float(gain.reshape(-1)[order[-2]])


def first_tree_ref(rows: np.ndarray, y: np.ndarray, depth: int, B: int, l2: float = 1.0):
    """Tree 0 of train_oblivious_gbdt in float64: its splits and, per level, the relative lead of
    the best gain over the runner-up."""
    p0 = float(np.clip(y.sum() / max(len(y), 1), 1e-6, 1 - 1e-6))
    grad = p0 - y.astype(np.float64)
    hess = np.full(len(y), max(p0 * (1 - p0), 1e-6))
    splits, leads = [], []
    for _ in range(depth):
        G, H = histograms_ref(rows, grad, hess, splits, B)
        s, g1, g2 = best_split_ref(G, H, l2)
        splits.append(s)
        leads.append((g1 - g2) / abs(g1))
    return splits, leads


def encode_rows(X: np.ndarray, borders: np.ndarray) -> np.ndarray:
    from ccfd_demo_summit_amd.train.trainer import _encode_training_rows
    return _encode_training_rows(X, borders)


# ------------------------------------------------------------------------------------ ABI
def test_abi_layout_of_training_structs(tmp_path):
    from ccfd_demo_summit_amd.ops import _lib
    from ccfd_demo_summit_amd.ops.build import CSRC
    hist_fields = ["rows", "grad", "hess", "G", "H", "n", "n_bins", "level", "split_feat", "split_bin"]
    upd_fields = ["rows", "leaf_val", "raw", "y", "grad", "hess", "n", "depth", "pad", "split_feat", "split_bin"]
    items = ["sizeof(ccfd_gbdt_hist_args)", "sizeof(ccfd_gbdt_update_args)"]
    items += [f"offsetof(ccfd_gbdt_hist_args,{f})" for f in hist_fields]
    items += [f"offsetof(ccfd_gbdt_update_args,{f})" for f in upd_fields]
    items += ["CCFD_GBDT_HIST_MAX_LEVEL", "CCFD_GBDT_HIST_MAX_BINS", "CCFD_GBDT_MAX_SPLITS"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccfd_abi.h"\nint main(){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    r = subprocess.run(["gcc", str(src), "-I", str(CSRC / "include"), "-o", str(exe)], capture_output=True)
    if r.returncode != 0:
        pytest.skip("no C compiler")
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.GbdtHistArgs), C.sizeof(_lib.GbdtUpdateArgs)]
    want += [getattr(_lib.GbdtHistArgs, f).offset for f in hist_fields]
    want += [getattr(_lib.GbdtUpdateArgs, f).offset for f in upd_fields]
    want += [_lib.GBDT_HIST_MAX_LEVEL, _lib.GBDT_HIST_MAX_BINS, _lib.GBDT_MAX_SPLITS]
    assert out == want
    assert out[:2] == [120, 128]
    from ccfd_demo_summit_amd.train import trainer
    assert trainer.HIP_HIST_MAX_BINS == _lib.GBDT_HIST_MAX_BINS
    assert trainer.HIP_HIST_MAX_DEPTH == _lib.GBDT_MAX_SPLITS == _lib.GBDT_HIST_MAX_LEVEL + 1


# ------------------------------------------------------------------------------- encoding
def _searchsorted_bins(X, borders):
    return np.stack([np.searchsorted(borders[f], X[:, f], side="left") for f in range(F)], axis=1)


@pytest.mark.parametrize("n,seed", [(20000, 1), (4097, 3)])
@pytest.mark.parametrize("B", [32, 64])
def test_g32_encoding_is_the_trainers_binning(n, seed, B):
    from ccfd_demo_summit_amd.train.trainer import _quantile_borders
    X, _ = generate(n, seed=seed)
    X = np.asarray(X, np.float32)
    assert not np.isnan(X).any()
    borders = _quantile_borders(X, B)
    rows = encode_rows(X, borders)
    assert rows.shape == (n, 32) and rows.dtype == np.uint8
    np.testing.assert_array_equal(rows[:, :F].astype(np.int64), _searchsorted_bins(X, borders))
    assert rows[:, :F].max() <= B - 1


def test_g32_encoding_with_a_duplicated_border():
    rng = np.random.default_rng(5)
    edges = np.array([-1.5, -0.25, 0.5, 0.5, 0.5, 1.0, 2.0], np.float32)      # 0.5 three times
    borders = np.tile(edges, (F, 1))
    borders[7] = np.array([0, 0, 1, 1, 2, 2, 3], np.float32)
    X = rng.standard_normal((3000, F)).astype(np.float32)
    X[rng.integers(0, 3000, 400), rng.integers(0, F, 400)] = 0.5              # exactly on the repeated edge
    X[rng.integers(0, 3000, 400), 7] = rng.integers(0, 4, 400).astype(np.float32)
    rows = encode_rows(X, borders)
    want = _searchsorted_bins(X, borders)
    np.testing.assert_array_equal(rows[:, :F].astype(np.int64), want)
    # a value past the repeated edge skips all of its copies: bins 3 and 4 of feature 0 stay empty
    assert set(np.unique(want[:, 0])) <= {0, 1, 2, 5, 6, 7}


def test_g32_encoding_sends_nan_to_bin_zero():
    borders = np.tile(np.linspace(-1, 1, 31, dtype=np.float32), (F, 1))
    X = np.zeros((4, F), np.float32)
    X[1, 3] = np.nan
    rows = encode_rows(X, borders)
    assert rows[1, 3] == 0 and rows[0, 3] == np.searchsorted(borders[3], 0.0, side="left")


# ------------------------------------------------------------------------ the hist= switch
@pytest.fixture(scope="module")
def small():
    return generate(3000, seed=4, fraud_rate=0.05)


def test_hist_hip_on_cpu_is_refused(small):
    from ccfd_demo_summit_amd.train import train_oblivious_gbdt
    X, y = small
    with pytest.raises(ValueError, match="CUDA"):
        train_oblivious_gbdt(X, y, n_trees=1, depth=2, device="cpu", hist="hip")


def test_hist_hip_with_128_bins_is_refused(small):
    from ccfd_demo_summit_amd.train import train_oblivious_gbdt
    X, y = small
    with pytest.raises(ValueError, match="64"):
        train_oblivious_gbdt(X, y, n_trees=1, depth=2, n_bins=128, device="cpu", hist="hip")
    with pytest.raises(ValueError, match="64"):
        train_oblivious_gbdt(X, y, n_trees=1, depth=2, device="cpu", hist="hip",
                             borders=np.tile(np.linspace(-3, 3, 127, dtype=np.float32), (F, 1)))


def test_hist_unknown_backend_is_refused(small):
    from ccfd_demo_summit_amd.train import train_oblivious_gbdt
    X, y = small
    with pytest.raises(ValueError, match="hist"):
        train_oblivious_gbdt(X, y, n_trees=1, depth=2, device="cpu", hist="rocm")


def test_hist_auto_on_cpu_is_the_torch_path(small):
    from ccfd_demo_summit_amd.train import train_oblivious_gbdt
    X, y = small
    m_t, info_t = train_oblivious_gbdt(X, y, n_trees=3, depth=4, device="cpu", hist="torch")
    m_a, info_a = train_oblivious_gbdt(X, y, n_trees=3, depth=4, device="cpu", hist="auto")
    m_d, info_d = train_oblivious_gbdt(X, y, n_trees=3, depth=4, device="cpu")
    assert info_t["hist"] == info_a["hist"] == info_d["hist"] == "torch"
    for m in (m_a, m_d):
        assert np.array_equal(m.feat, m_t.feat) and np.array_equal(m.thr, m_t.thr)
        assert np.array_equal(m.leaves, m_t.leaves)


def test_train_cli_takes_hist(tmp_path):
    from ccfd_demo_summit_amd.train.__main__ import main
    out = tmp_path / "m.safetensors"
    assert main(["--model", "gbdt", "--rows", "4000", "--fraud-rate", "0.05", "--trees", "2", "--depth", "3",
                 "--device", "cpu", "--hist", "auto", "--out", str(out)]) == 0
    assert out.exists()
    with pytest.raises(ValueError, match="CUDA"):
        main(["--model", "gbdt", "--rows", "4000", "--trees", "1", "--depth", "2", "--device", "cpu",
              "--hist", "hip", "--out", str(out)])


# ------------------------------------------------------------------------------ the oracle
def test_histograms_ref_agrees_with_scatter_add():
    """The float64 oracle against the trainer's scatter_add_ formulation (f32, CPU).  Bound per
    bin: |G32 - G64| <= count * 2^-23 * sum|g| over the bin's rows -- any-order f32 summation of
    `count` terms is within (count - 1) * 2^-24 * sum|g| to first order; the factor 2 covers the
    higher-order terms and is the slack the GPU test grants a two-stage sum."""
    rng = np.random.default_rng(9)
    n, B = 6000, 32
    rows = rng.integers(0, B, (n, 32), dtype=np.uint8)
    p = 1 / (1 + np.exp(-rng.standard_normal(n) * 2))
    y = (rng.random(n) < 0.1).astype(np.float64)
    grad = (p - y).astype(np.float32)
    hess = np.maximum(p * (1 - p), 1e-6).astype(np.float32)
    splits = [(0, 0), (29, B - 2), (11, 13)]
    G64, H64 = histograms_ref(rows, grad, hess, splits, B)
    cnt, sabs_g = histograms_ref(rows, np.ones(n), np.abs(grad), splits, B)
    _, sabs_h = histograms_ref(rows, np.ones(n), np.abs(hess), splits, B)
    assert cnt.sum() == n * F and G64.shape == (8, F, B)
    np.testing.assert_allclose(G64.sum((0, 2)), np.full(F, grad.astype(np.float64).sum()), rtol=0, atol=1e-9)

    bt = torch.from_numpy(rows[:, :F].astype(np.int64))
    leaf = torch.from_numpy(leaves_ref(rows, splits))
    L = 8
    key = ((leaf[:, None] * F + torch.arange(F)[None, :]) * B + bt).reshape(-1)
    for v, ref, sabs in ((grad, G64, sabs_g), (hess, H64, sabs_h)):
        t = torch.from_numpy(v)
        got = torch.zeros(L * F * B).scatter_add_(0, key, t[:, None].expand(n, F).reshape(-1)).view(L, F, B)
        err = np.abs(got.numpy().astype(np.float64) - ref)
        assert (err <= cnt * 2.0 ** -23 * sabs).all()


def test_first_tree_ref_matches_the_trainer_on_cpu():
    """The float64 oracle picks the splits of the trainer's first tree where no gain is nearly
    tied (this input's leads, all >= 1e-3, are asserted first)."""
    from ccfd_demo_summit_amd.train import train_oblivious_gbdt
    from ccfd_demo_summit_amd.train.trainer import _quantile_borders
    X, y = generate(20000, seed=1, fraud_rate=0.02)
    X = np.asarray(X, np.float32)
    borders = _quantile_borders(X, 32)
    splits, leads = first_tree_ref(encode_rows(X, borders), np.asarray(y), 6, 32)
    assert min(leads) >= 1e-3, leads
    m, _ = train_oblivious_gbdt(X, y, n_trees=1, depth=6, n_bins=32, device="cpu")
    assert [int(f) for f in m.feat[0]] == [f for f, _ in splits]
    np.testing.assert_array_equal(m.thr[0], np.array([borders[f, b] for f, b in splits], np.float32))
