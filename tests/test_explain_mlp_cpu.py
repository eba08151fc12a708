"""Sampled Shapley values of the MLP and the closed form for LR (models/explain_mlp.py): the MLX1
table, the documented properties of the estimator, the baseline key of saved models, the scorers,
the /explain route and the router's ``reasons``.

The builders at the top are shared with tests/test_explain_mlp_gpu.py."""
import asyncio
import re
from pathlib import Path

import numpy as np
import pytest

from ccfd_demo_summit_amd.contracts import seldon
from ccfd_demo_summit_amd.contracts.transaction import (AMOUNT_COL, FEATURE_NAMES, N_FEATURES, WIRE_PERM,
                                                        decode_wire, encode_wire)
from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import build_model, load_model, save_model
from ccfd_demo_summit_amd.models.common import Normalizer
from ccfd_demo_summit_amd.models.explain import top_reasons
from ccfd_demo_summit_amd.models.explain_mlp import (MlpExplainTable, coalition_logits, coalition_rows,
                                                     differing_positions, mlp_base_value, permutation_table,
                                                     recombine, shapley_lr, shapley_mlp_exact, shapley_mlp_sampled,
                                                     shapley_mlp_table)
from ccfd_demo_summit_amd.models.mlp import H1, H2, MLPModel

_X = {}


def rows(n=4000, seed=1):
    if (n, seed) not in _X:
        X = generate(n, seed=seed)[0]
        X.setflags(write=False)
        _X[(n, seed)] = X
    return _X[(n, seed)]


def mlp_case(log_amount=True, seed=0, how="median"):
    """A random-init, calibrated MLP with a baseline, fitted on ``rows()``."""
    X = rows()
    m = build_model("mlp", seed=seed, X_ref=X, calibrate_rate=0.01)
    if not log_amount:
        m.norm = Normalizer.fit(X, log_amount=False)
    return m.fit_baseline(X, how)


def linear_case(seed=0):
    """An MLP whose wire logit is exactly ``x . w + b3`` on small integers: unit 2j of layer 1 is
    +x_j and unit 2j+1 is -x_j, layer 2 passes the 60 units through, layer 3 weighs them +-w_j
    (w_j integer in -3..3); identity normaliser.  Returns (model with an integer baseline, w)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-3, 4, N_FEATURES).astype(np.float32)
    W1 = np.zeros((H1, N_FEATURES), np.float32)
    W2 = np.zeros((H2, H1), np.float32)
    w3 = np.zeros(H2, np.float32)
    for j in range(N_FEATURES):
        W1[2 * j, j], W1[2 * j + 1, j] = 1.0, -1.0
        W2[2 * j, 2 * j] = W2[2 * j + 1, 2 * j + 1] = 1.0
        w3[2 * j], w3[2 * j + 1] = w[j], -w[j]
    m = MLPModel(W1, np.zeros(H1, np.float32), W2, np.zeros(H2, np.float32), w3, 2.0, Normalizer.identity())
    m.baseline = rng.integers(-8, 9, N_FEATURES).astype(np.float32)
    return m, w


def integer_rows(n, seed=3):
    return np.random.default_rng(seed).integers(-8, 9, (n, N_FEATURES)).astype(np.float32)


def sparse_rows(m, k, n, seed):
    """``n`` rows equal to the baseline except in ``k`` random features, taken from ``rows()``."""
    rng = np.random.default_rng(seed)
    X = rows()
    out = np.tile(m.baseline, (n, 1))
    for r in out:
        f = rng.choice(N_FEATURES, k, replace=False)
        r[f] = X[rng.integers(len(X)), f]
    return out


def two_feature_closed_form(v00, va, vb, vab):
    """Exact Shapley values of a two-player game from its four values."""
    return 0.5 * ((va - v00) + (vab - vb)), 0.5 * ((vb - v00) + (vab - va))


# --------------------------------------------------------------------------------- table
@pytest.mark.parametrize("P,seed", [(2, 0), (64, 7), (256, 1)])
def test_table_layout_and_round_trip(P, seed):
    m = mlp_case()
    blob = MlpExplainTable.pack(m, P, seed)
    assert len(blob) % 16 == 0 and len(blob) == 128 + 160 * P and blob[:4] == b"MLX1"
    t = MlpExplainTable.unpack(blob)
    assert t.P == P and t.seed == seed and t.to_bytes() == blob
    perms = permutation_table(P, seed)
    assert (t.perms == perms).all() and (np.sort(perms, axis=1) == np.arange(30)).all()
    assert (perms[1::2] == perms[0::2, ::-1]).all()                       # antithetic pairs
    if P > 2:
        assert (perms[0] != perms[2]).any()
    assert (t.baseline_w64 == encode_wire(m.baseline[None])[0]).all()
    full = np.uint32((1 << 30) - 1)
    for p in range(P):
        assert t.masks[p, 0] == 0 and t.masks[p, 30] == full and t.masks[p, 31] == full
        for s in range(30):                                               # a prefix chain
            assert t.masks[p, s + 1] == t.masks[p, s] | np.uint32(1 << int(perms[p, s]))
            assert t.inv[p, perms[p, s]] == s                             # inv inverts the permutation
        assert (t.inv[p, 30:] == 30).all()


def test_table_refusals():
    m = mlp_case()
    for P in (0, 1, 3, 65, 258, 1024):
        with pytest.raises(ValueError, match="P must be"):
            MlpExplainTable.pack(m, P, 0)
    with pytest.raises(ValueError, match="fit_baseline"):
        MlpExplainTable.pack(build_model("mlp", seed=0), 64, 0)
    blob = MlpExplainTable.pack(m, 4, 0)
    with pytest.raises(ValueError, match="MLX1"):
        MlpExplainTable.unpack(b"MLX0" + blob[4:])
    with pytest.raises(ValueError, match="MLX1"):
        MlpExplainTable.unpack(blob[:-16])
    assert (permutation_table(4, 5) == permutation_table(4, 5)).all()
    assert (permutation_table(4, 5) != permutation_table(4, 6)).any()


def test_coalition_rows_follow_the_mask_words():
    m = mlp_case()
    X = rows()[:3]
    t = MlpExplainTable.build(m, 4, 2)
    w = coalition_rows(t, encode_wire(X))                                 # [3, 4, 32, 64]
    xd, bd = decode_wire(encode_wire(X)), decode_wire(encode_wire(m.baseline[None]))[0]
    for p in range(4):
        for s in range(32):
            want = np.tile(bd, (3, 1))
            feats = WIRE_PERM[t.perms[p, :min(s, 30)]]
            want[:, feats] = xd[:, feats]
            assert (decode_wire(w[:, p, s]) == want).all()
    # the oracle scores each distinct slot once; same logits as scoring every built row
    z = coalition_logits(m, t, encode_wire(X))
    np.testing.assert_allclose(z, m.wire_logits(decode_wire(w.reshape(-1, 64))).reshape(3, 4, 32), rtol=0, atol=1e-6)


# --------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("log_amount", [True, False])
@pytest.mark.parametrize("P", [2, 64])
def test_efficiency(P, log_amount):
    m = mlp_case(log_amount)
    X = rows()[100:116]
    phi, bv = shapley_mlp_sampled(m, X, P, seed=3)
    assert phi.dtype == np.float64 and phi.shape == (16, 30) and bv == mlp_base_value(m)
    want = m.wire_logits(X).astype(np.float64)
    # every term is a float32 logit, |z| < 2^5: the float64 sums are exact to ~ 31 * P * 2^-53 * 2^5
    np.testing.assert_allclose(phi.sum(1) + bv, want, rtol=0, atol=1e-12)
    assert np.abs(phi).max() > 1e-3                                       # and they are not all nothing


def test_dummy_positions_get_exact_zero():
    m = mlp_case()
    X = sparse_rows(m, 5, 12, seed=11)
    X[0] = m.baseline                                                     # a row that is the baseline
    phi, bv = shapley_mlp_sampled(m, X, 64, seed=1)
    same = encode_wire(X).view(np.uint16) == encode_wire(m.baseline[None]).view(np.uint16)
    same_feat = np.empty((12, 30), bool)
    same_feat[:, WIRE_PERM[:28]] = same[:, :28]
    same_feat[:, 0] = same[:, 28] & same[:, 29]
    same_feat[:, AMOUNT_COL] = same[:, 30] & same[:, 31]
    assert same_feat.sum() >= 12 * 25 and (~same_feat).sum() > 30
    assert (phi[same_feat] == 0.0).all() and (phi[0] == 0.0).all()
    assert (phi[~same_feat] != 0.0).mean() > 0.9
    for i in range(12):
        assert set(WIRE_PERM[differing_positions(m, X[i])]) == set(np.nonzero(~same_feat[i])[0])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_feature_rows_are_exact(seed):
    m = mlp_case()
    X = sparse_rows(m, 2, 6, seed=20 + seed)
    phi, bv = shapley_mlp_sampled(m, X, 64, seed=seed)
    for i, x in enumerate(X):
        fa, fb = np.nonzero(x != m.baseline)[0]
        xa, xb = m.baseline.copy(), m.baseline.copy()
        xa[fa], xb[fb] = x[fa], x[fb]
        v = m.wire_logits(np.stack([m.baseline, xa, xb, x])).astype(np.float64)
        pa, pb = two_feature_closed_form(*v)
        # 64 float64 additions of the same two numbers against one: a few ulps of |v| < 32
        np.testing.assert_allclose([phi[i, fa], phi[i, fb]], [pa, pb], rtol=0, atol=1e-13)
        np.testing.assert_allclose(shapley_mlp_exact(m, x), phi[i], rtol=0, atol=1e-13)
        assert np.count_nonzero(phi[i]) <= 2


def test_exact_linear_case():
    m, w = linear_case()
    X = integer_rows(9)
    np.testing.assert_array_equal(m.wire_logits(X), X @ w + 2.0)          # the construction is exact
    phi, bv = shapley_mlp_sampled(m, X, 64, seed=0)
    assert bv == float(m.baseline @ w + 2.0)
    np.testing.assert_array_equal(phi, w[None, :] * (X - m.baseline[None, :]))
    phi32, z = shapley_mlp_table(m, MlpExplainTable.pack(m, 64, 0), encode_wire(X), dtype=np.float32)
    assert phi32.dtype == np.float32 and z.dtype == np.float32 and z.shape == (9, 64, 32)
    np.testing.assert_array_equal(phi32, w[None, :] * (X - m.baseline[None, :]))


def test_table_oracle_matches_sampled_and_recombine_order():
    m = mlp_case()
    X = rows()[7:12]
    blob = MlpExplainTable.pack(m, 16, 9)
    phi64, z = shapley_mlp_table(m, blob, encode_wire(X))
    np.testing.assert_array_equal(phi64, shapley_mlp_sampled(m, X, 16, 9)[0])
    assert (z[:, :, 30] == z[:, :, 31]).all() and (z[:, :, 0] == np.float32(mlp_base_value(m))).all()
    np.testing.assert_array_equal(z[:, :, 30], np.broadcast_to(m.wire_logits(X)[:, None], (5, 16)))
    # the documented order, spelled out
    t = MlpExplainTable.unpack(blob)
    acc = np.zeros((5, 30), np.float32)
    for p in range(16):
        d = z[:, p, 1:] - z[:, p, :-1]
        acc += d[:, t.inv[p, :30]]
    want = np.empty_like(acc)
    want[:, WIRE_PERM] = acc / np.float32(16)
    np.testing.assert_array_equal(recombine(z, t, np.float32), want)


def test_convergence_against_enumeration():
    m = mlp_case()
    X = sparse_rows(m, 6, 12, seed=5)
    exact = np.stack([shapley_mlp_exact(m, x) for x in X])
    np.testing.assert_allclose(exact.sum(1) + mlp_base_value(m), m.wire_logits(X), rtol=0, atol=1e-12)
    err = {P: np.abs(shapley_mlp_sampled(m, X, P, seed=3)[0] - exact).max() for P in (16, 1024)}
    print(f"max |phi - exact|: P=16 {err[16]:.3g}, P=1024 {err[1024]:.3g}")
    assert 0 < err[1024] < 0.5 * err[16]
    with pytest.raises(ValueError, match="enumeration stops"):
        shapley_mlp_exact(m, rows()[0])


@pytest.mark.parametrize("log_amount", [True, False])
def test_lr_closed_form(log_amount):
    X = rows()
    m = build_model("lr", seed=2, X_ref=X, calibrate_rate=0.01)
    if not log_amount:
        m.norm = Normalizer.fit(X, log_amount=False)
    with pytest.raises(ValueError, match="fit_baseline"):
        shapley_lr(m, X[:4])
    m = m.fit_baseline(X, "mean")
    np.testing.assert_allclose(m.baseline, X.astype(np.float64).mean(0), rtol=1e-6)
    phi, bv = shapley_lr(m, X[:50])
    lx, lb = m.logits(X[:50]).astype(np.float64), float(m.logits(m.baseline[None])[0])
    assert bv == pytest.approx(lb, abs=1e-6)
    np.testing.assert_allclose(phi.sum(1), lx - lb, rtol=0, atol=1e-5)    # logits() rounds to float32
    Xb = X[:3].copy()
    Xb[:, 5] = m.baseline[5]
    assert (shapley_lr(m, Xb)[0][:, 5] == 0.0).all()


# --------------------------------------------------------------------------------- model state
@pytest.mark.parametrize("kind", ["mlp", "lr"])
def test_baseline_key_in_state_dict(kind, tmp_path):
    X = rows()
    m = build_model(kind, seed=1, X_ref=X)
    assert m.baseline is None and f"{kind}.baseline" not in m.state_dict()
    mb = m.fit_baseline(X)
    assert m.baseline is None and mb.baseline.dtype == np.float32 and mb.baseline.shape == (30,)
    np.testing.assert_allclose(mb.baseline, np.median(X.astype(np.float64), 0), rtol=1e-6)
    assert set(mb.state_dict()) == set(m.state_dict()) | {f"{kind}.baseline"}
    assert mb.pack() == m.pack() and mb.pack(wire=True) == m.pack(wire=True)
    save_model(m, str(tmp_path / "a.st"))
    save_model(mb, str(tmp_path / "b.st"))
    assert load_model(str(tmp_path / "a.st")).baseline is None
    back = load_model(str(tmp_path / "b.st"))
    np.testing.assert_array_equal(back.baseline, mb.baseline)
    np.testing.assert_array_equal(back.predict_proba(X[:9]), m.predict_proba(X[:9]))
    with pytest.raises(ValueError, match="median"):
        m.fit_baseline(X, "mode")


def test_train_cli_explain_baseline(tmp_path):
    from ccfd_demo_summit_amd.train.__main__ import main
    out = tmp_path / "lr.st"
    common = ["--model", "lr", "--rows", "3000", "--epochs", "1", "--device", "cpu", "--out", str(out)]
    assert main(common) == 0 and load_model(str(out)).baseline is None
    assert main(common + ["--explain-baseline", "median"]) == 0
    m = load_model(str(out))
    assert m.baseline is not None and m.baseline.shape == (30,)
    phi, bv = shapley_lr(m, rows()[:4])
    np.testing.assert_allclose(phi.sum(1) + bv, m.logits(rows()[:4]), atol=1e-5)


# --------------------------------------------------------------------------------- serving
def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1 - p))


def test_scorers_and_explain_route():
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.serving import CpuScorer
    from ccfd_demo_summit_amd.serving.scorers import _explainable
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    X = rows()[:6]
    mlp = mlp_case()
    lr = build_model("lr", seed=2, X_ref=rows(), calibrate_rate=0.01).fit_baseline(rows())
    for m in (mlp, lr):
        _explainable(m)
    for kind in ("mlp", "lr"):
        with pytest.raises(ValueError, match="no explanation.*fit_baseline"):
            _explainable(build_model(kind, seed=0, X_ref=rows()))
        with pytest.raises(ValueError, match="no explanation"):
            CpuScorer(build_model(kind, seed=0, X_ref=rows())).explain(X)
    phi, bv = CpuScorer(mlp).explain(X)
    np.testing.assert_array_equal(phi, shapley_mlp_sampled(mlp, X, 64, 0)[0])
    phi_lr, bv_lr = CpuScorer(lr).explain(X)
    np.testing.assert_array_equal(phi_lr, shapley_lr(lr, X)[0])

    async def go():
        for m, want, b in ((mlp, phi, bv), (lr, phi_lr, bv_lr)):
            async with TestClient(TestServer(SeldonServer(CpuScorer(m)).app)) as cl:
                r = await cl.post("/explain", json=seldon.build_request(X))
                assert r.status == 200
                body = await r.json()
                assert body["data"]["names"] == list(FEATURE_NAMES)
                got = np.asarray(body["data"]["ndarray"])
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
                tags = body["meta"]["tags"]
                assert tags["base_value"] == pytest.approx(b)
                # base_value + sum phi is the log-odds of proba: of the W64 chain for the MLP, which the
                # suite holds within 1e-2 of the float32 model's proba; of the model itself for LR
                p = 1.0 / (1.0 + np.exp(-(tags["base_value"] + got.sum(1))))
                if m.kind == "mlp":
                    np.testing.assert_allclose(p, m.wire_proba(X), rtol=0, atol=1e-6)
                    np.testing.assert_allclose(p, tags["proba"], rtol=0, atol=1e-2)
                else:
                    np.testing.assert_allclose(tags["base_value"] + got.sum(1), _logit(tags["proba"]), rtol=0, atol=1e-4)
                r = await cl.post("/predict", json=seldon.build_request(X))
                assert r.status == 200
        for other in (build_model("mlp", seed=0, X_ref=rows()), build_model("lr", seed=0, X_ref=rows())):
            async with TestClient(TestServer(SeldonServer(CpuScorer(other)).app)) as cl:
                r = await cl.post("/explain", json=seldon.build_request(X))
                assert r.status == 400
                body = await r.json()
                assert body["status"]["status"] == "FAILURE" and "no explanation" in body["status"]["info"]
    _run(go())


def test_router_reasons_on_an_mlp_fraud_start():
    from ccfd_demo_summit_amd.process import ProcessEngine
    from ccfd_demo_summit_amd.router.router import Router
    from ccfd_demo_summit_amd.router.rules import RuleSet
    from ccfd_demo_summit_amd.serving import CpuScorer
    m = mlp_case()
    X = rows()[:40]
    proba = m.predict_proba(X)
    thr = float(np.sort(proba)[-3])                                       # 3 fraud rows
    phi, _ = shapley_mlp_sampled(m, X, 64, 0)
    eng = ProcessEngine(notification_timeout_s=60)
    router = Router(RuleSet.threshold(thr), eng, explainer=CpuScorer(m), reasons=3)
    out = router.on_scored(np.arange(40) + 500, np.arange(40), proba, X=X)
    assert out["fraud"] == 3
    seen = 0
    for i in np.nonzero(proba >= thr)[0]:
        why = eng.get(eng._by_tx[500 + int(i)]).variables["reasons"]
        assert why == top_reasons(phi[i], FEATURE_NAMES, 3) and all(r["phi"] > 0 for r in why)
        seen += len(why)
    assert seen > 0


# --------------------------------------------------------------------------------- docs
def test_explain_doc_example_runs():
    doc = Path(__file__).resolve().parents[1] / "docs" / "EXPLAIN.md"
    blocks = re.findall(r"```python\n(.*?)```", doc.read_text(), re.S)
    assert len(blocks) == 1
    ns = {}
    exec(blocks[0], ns)
    assert ns["phi"].shape == (4, 30) and ns["reasons"] is not None
    np.testing.assert_allclose(ns["phi"].sum(1) + ns["base_value"], ns["model"].wire_logits(ns["X"][:4]), atol=1e-12)
