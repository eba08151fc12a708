"""Shadow scoring of a GBDT challenger, host side (no GPU): the pair check for binned rows,
``ObliviousGBDT.padded``, training against a given bin table, and the fixtures the GPU tests
(test_shadow_gbdt_gpu.py) rely on."""
import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate
from tests.helpers.gbdt_pairs import make_pair


def _dm(model, spec):
    """A DeviceModel of ``model`` packed against ``spec``, blob on the CPU."""
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    blob = torch.from_numpy(np.frombuffer(model.pack(bins=spec), np.uint8).copy())
    return DeviceModel.from_blob("gbdt", blob, trees=model.n_trees, depth=model.depth, bins=spec)


@pytest.fixture(scope="module")
def X():
    return generate(70001, seed=11)[0]


@pytest.fixture(scope="module")
def g32(X):
    return make_pair(X[:20000])


@pytest.fixture(scope="module")
def g20(X):
    return make_pair(X[:20000], trees=30, depth=5, seeds=(5, 6), bits=5)


def test_check_shadow_pair_binned(g32, g20):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, check_shadow_pair
    A, B, spec = g32
    check_shadow_pair(_dm(A, spec), _dm(B, spec))
    check_shadow_pair(_dm(A, spec), _dm(B, spec), persist_items=1)
    A5, B5, spec5 = g20
    assert spec5.bits == 5
    check_shadow_pair(_dm(A5, spec5), _dm(B5, spec5))

    def refused(*args, **kw):
        with pytest.raises(ValueError) as e:
            check_shadow_pair(*args, **kw)
        return str(e.value)

    # another bin table: A's own (its thresholds only), both stamps named
    own = A.bin_spec()
    m = refused(_dm(A, spec), _dm(A, own))
    assert "bin tables differ" in m and str(spec.stamp) in m and str(own.stamp) in m
    # another shape, both shapes named
    m = refused(_dm(A, spec), _dm(A.padded(n_trees=101), spec))
    assert "100 trees x depth 6" in m and "101 trees x depth 6" in m
    m = refused(_dm(A.padded(depth=7), spec), _dm(B, spec))
    assert "depth 7" in m and "depth 6" in m
    # G32 against G20, both formats named
    m = refused(_dm(A5, spec5.with_bits(8)), _dm(B5, spec5))
    assert "g32" in m and "g20" in m
    m = refused(_dm(A, spec), DeviceModel.from_blob("gbdt", torch.zeros(64, dtype=torch.uint8), trees=100, depth=6))
    assert "g32" in m and "f32" in m
    # f32 rows: still no kernel, and the sentence says what is supported
    f32 = DeviceModel.from_blob("gbdt", torch.zeros(64, dtype=torch.uint8), trees=100, depth=6)
    m = refused(f32, f32)
    assert "'gbdt' models have no shadow kernel" in m and "G32 / G20" in m
    # the common refusals are unchanged for a binned pair
    assert "routing rules" in refused(_dm(A, spec), _dm(B, spec), rules=object())
    assert "pipelined" in refused(_dm(A, spec), _dm(B, spec), persist_items=2)
    mlp = DeviceModel.from_blob("mlp", torch.zeros(64, dtype=torch.uint8), wire=True)
    assert "kind mismatch" in refused(_dm(A, spec), mlp)


def test_pair_fixtures_are_non_trivial(X, g32, g20):
    """The flag counts the GPU tests build on (f32 oracle; the binned kernels choose the same
    leaves): every shadow counter is non-trivial, 0 < both < min."""
    for (A, B, spec), n, want in ((g32, 14288, (128, 398, 24)), (g20, 14288, (170, 439, 39)),
                                  (g32, 4097, (23, 83, 4))):
        fa, fb = A.predict_proba(X[:n]) >= 0.5, B.predict_proba(X[:n]) >= 0.5
        assert (int(fa.sum()), int(fb.sum()), int((fa & fb).sum())) == want
        assert spec.contains(A.bin_spec()) and spec.contains(B.bin_spec())
    assert max(e.size for e in g32[2].edges) <= 40 and max(e.size for e in g20[2].edges) <= 15


def test_padded_is_exactly_equivalent():
    from ccfd_demo_summit_amd.models.gbdt import MAX_BINS, ObliviousGBDT
    Xs = generate(5000, seed=2)[0]
    m = ObliviousGBDT.random_init(10, 4, seed=1, X_ref=Xs)
    m.base = 0.25
    p = m.padded(n_trees=13, depth=6)
    assert (p.n_trees, p.depth) == (13, 6) and p.base == m.base
    np.testing.assert_array_equal(p.raw_score(Xs).view(np.uint32), m.raw_score(Xs).view(np.uint32))
    np.testing.assert_array_equal(p.leaves[:10, :16], m.leaves)
    assert not p.leaves[:10, 16:].any() and not p.leaves[10:].any()
    assert np.isnan(p.thr[:, 4:]).all() and np.isnan(p.thr[10:]).all() and not p.feat[:, 4:].any()
    # packs against its own table; the added levels can never fire
    spec = p.bin_spec()
    assert spec.contains(m.bin_spec()) and m.bin_spec().contains(spec)
    p.pack(bins=spec)
    k = spec.bin_index(p.feat, p.thr)
    assert (k[:, 4:] == MAX_BINS).all() and (k[10:] == MAX_BINS).all()
    np.testing.assert_array_equal(p.leaf_index_g32(spec.encode(Xs))[:, :10], m.leaf_index(Xs))
    q = m.padded()
    assert (q.n_trees, q.depth) == (10, 4)
    for kw in ({"n_trees": 9}, {"depth": 3}, {"n_trees": 13, "depth": 2}):
        with pytest.raises(ValueError, match="shrink"):
            m.padded(**kw)
    with pytest.raises(ValueError):
        m.padded(depth=9)


def test_train_against_a_bin_table():
    from ccfd_demo_summit_amd.models.gbdt import BinSpec
    from ccfd_demo_summit_amd.train.trainer import _quantile_borders, train_oblivious_gbdt
    Xs, y = generate(4000, seed=7, fraud_rate=0.05)
    q = _quantile_borders(Xs, 12)                              # [30, 11]
    # ragged: feature f keeps 1 + f % 11 of its quantiles, feature 3 has no edge at all
    edges = [np.unique(q[f, :1 + f % 11]) for f in range(30)]
    edges[3] = np.zeros(0, np.float32)
    spec = BinSpec(edges)
    assert len({e.size for e in spec.edges}) > 2
    model, info = train_oblivious_gbdt(Xs, y, n_trees=5, depth=3, device="cpu", hist="torch", bin_spec=spec)
    assert info["hist"] == "torch" and (model.n_trees, model.depth) == (5, 3)
    assert np.isfinite(model.thr).all()
    assert not (model.feat == 3).any()
    assert spec.contains(model.bin_spec())
    assert len(model.pack(bins=spec)) > 64
    # the chosen splits separate something: the trained model beats the base rate
    p0 = y.mean()
    base_ll = -(p0 * np.log(p0) + (1 - p0) * np.log(1 - p0))
    assert info["train_logloss"] < base_ll
    with pytest.raises(ValueError, match="bin_spec"):
        train_oblivious_gbdt(Xs, y, n_trees=1, depth=1, device="cpu", borders=q, bin_spec=spec)
    with pytest.raises(ValueError, match="no edge"):
        train_oblivious_gbdt(Xs, y, n_trees=1, depth=1, device="cpu",
                             bin_spec=BinSpec([np.zeros(0, np.float32)] * 30))


def test_api_doc_gbdt_shadow_block_runs():
    """The train -> pad -> pack block of docs/API.md (fenced ``py``) runs as written."""
    import re
    from pathlib import Path
    doc = (Path(__file__).resolve().parents[1] / "docs" / "API.md").read_text()
    blocks = [b for b in re.findall(r"```py\n(.*?)```", doc, re.S) if "bin_spec=spec" in b]
    assert len(blocks) == 1
    ns = {}
    exec(blocks[0], ns)
    assert len(ns["blob"]) > 64 and ns["info"]["hist"] == "torch"


def test_broadcast_model_packs_against_a_given_table(g32, g20):
    """``broadcast_model(..., bins=)``: the live table and its format win over the ensemble's
    own table and the requested format (single rank: nothing is sent)."""
    from ccfd_demo_summit_amd.engine.stream_engine import same_bins
    from ccfd_demo_summit_amd.ops.kernels import check_shadow_pair
    from ccfd_demo_summit_amd.parallel import DistContext
    from ccfd_demo_summit_amd.parallel.dp import broadcast_model
    ctx = DistContext(0, 1, 0, torch.device("cpu"), "none")
    A5, B5, spec5 = g20
    dm = broadcast_model(ctx, B5, "gbdt", "g32", bins=spec5)
    assert dm.row_format == "g20" and same_bins(dm.bins, spec5) and (dm.trees, dm.depth) == (30, 5)
    assert bytes(dm.blob.numpy()) == B5.pack(bins=spec5)
    check_shadow_pair(_dm(A5, spec5), dm)
    own = broadcast_model(ctx, B5, "gbdt", "g20")                # without bins=: the ensemble's own table
    assert own.row_format == "g20" and not same_bins(own.bins, spec5)
    with pytest.raises(ValueError, match="not a bin edge"):
        broadcast_model(ctx, g32[1], "gbdt", "g20", bins=spec5)


def test_train_cli_bin_spec_from(tmp_path, capsys):
    """``train --bin-spec-from LIVE``: the trained ensemble packs against the live model's table."""
    from ccfd_demo_summit_amd.models import build_model, load_model, save_model
    from ccfd_demo_summit_amd.train.__main__ import main
    live = build_model("gbdt", seed=2, X_ref=generate(3000, seed=4)[0], gbdt_trees=12, gbdt_depth=3)
    save_model(live, str(tmp_path / "live.safetensors"))
    out = tmp_path / "cand.safetensors"
    assert main(["--model", "gbdt", "--rows", "3000", "--fraud-rate", "0.05", "--trees", "3", "--depth", "2",
                 "--device", "cpu", "--bin-spec-from", str(tmp_path / "live.safetensors"), "--out", str(out)]) == 0
    cand = load_model(str(out))
    assert (cand.n_trees, cand.depth) == (3, 2) and live.bin_spec().contains(cand.bin_spec())
    cand.padded(n_trees=12, depth=3).pack(bins=live.bin_spec())
    with pytest.raises(SystemExit, match="gbdt"):
        main(["--model", "lr", "--bin-spec-from", str(tmp_path / "live.safetensors"), "--out", str(out), "--rows", "100",
              "--device", "cpu"])
