"""Exact Shapley attributions of the oblivious GBDT, CPU side: the oracle's properties, the
GBX1 table, the cover key of saved models, the /explain route and the router's ``reasons``.

The builders at the top are shared with tests/test_explain_gpu.py."""
import asyncio

import numpy as np
import pytest

from ccfd_demo_summit_amd.contracts import seldon
from ccfd_demo_summit_amd.contracts.transaction import FEATURE_NAMES
from ccfd_demo_summit_amd.models import build_model
from ccfd_demo_summit_amd.models.explain import ExplainTable, base_value, shapley_oblivious, top_reasons
from ccfd_demo_summit_amd.models.gbdt import BinSpec, ObliviousGBDT


# ------------------------------------------------------------------------------- shared builders
def background(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 30)).astype(np.float32)


def random_case(T, D, seed, n_bg=300):
    """A random T x depth D ensemble with cover from ``n_bg`` background rows (deep trees keep
    empty leaves) and a non-zero base."""
    bg = background(n_bg, 100 + seed)
    m = ObliviousGBDT.random_init(T, D, seed=seed, X_ref=bg)
    m.base = -1.25
    return m.fit_cover(bg)


def toy_case():
    """4 x depth 4: tree 1 tests feature of level 0 again at level 2, tree 2 has a NaN threshold,
    and 60 background rows leave some of the 16 leaves of every tree empty."""
    bg = background(60, 7)
    m = ObliviousGBDT.random_init(4, 4, seed=3, X_ref=bg)
    m.feat[1, 2] = m.feat[1, 0]
    m.thr[2, 1] = np.nan
    m.base = 0.3
    m = m.fit_cover(bg)
    assert (m.cover == 0).any()
    return m


def edge_case():
    """3 x depth 4 against a bin table with 255 edges on feature 5: tree 0 tests feature 5 at
    every level, tree 1 has a NaN level and a repeated feature; rows reach bins 0 and 255.
    Returns (model, spec, X)."""
    bg = background(60, 11)
    m = ObliviousGBDT.random_init(3, 4, seed=5, X_ref=bg)
    edges5 = np.linspace(-2.0, 2.0, 255).astype(np.float32)
    m.feat[0, :] = 5
    m.thr[0, :] = edges5[[40, 200, 127, 254]]
    m.feat[1, 3] = m.feat[1, 1]
    m.thr[1, 2] = np.nan
    for t, d in zip(*np.nonzero(m.feat[1:] == 5)):          # other trees: keep feature 5 on the table
        m.thr[1 + t, d] = edges5[17]
    m.base = 0.5
    m = m.fit_cover(bg)
    own = m.bin_spec()
    spec = BinSpec([edges5 if j == 5 else own.edges[j] for j in range(30)])
    X = background(65, 12) * 1.5
    X[0, 5], X[1, 5], X[2, 5] = -9.0, 9.0, 2.0              # bins 0, 255 and 254 of feature 5
    rows = spec.encode(X)
    assert rows[0, 5] == 0 and rows[1, 5] == 255
    return m, spec, X


def unit(model):
    """u = 2^-24 * sum_t max_l |leaves[t, l]|: the tolerance unit of the attributions."""
    return 2.0 ** -24 * float(np.abs(model.leaves).max(1).astype(np.float64).sum())


def raw_f64(model, lx):
    return model.base + model.leaves[np.arange(model.n_trees)[None, :], lx].astype(np.float64).sum(1)


def table_shapley(tab: ExplainTable, rows: np.ndarray) -> np.ndarray:
    """The kernel's algorithm on the unpacked table, in float64: per tree and feature subset the
    restricted leaf sum, phi_j = sum_S c_j(S) v(S)."""
    T, D = tab.feat.shape
    phi = np.zeros((rows.shape[0], 30))
    for i, r in enumerate(rows):
        if r[31] != tab.stamp:
            phi[i] = np.nan
            continue
        for t in range(T):
            lx = sum(int(r[tab.feat[t, d]] > tab.k[t, d]) << d for d in range(D))
            m = int(tab.m[t])
            for S in range(1 << m):
                lmask = 0
                for j in range(m):
                    if (S >> j) & 1:
                        lmask |= int(tab.slot_mask[t, j])
                free = ~lmask & ((1 << D) - 1)
                v, sub = 0.0, free
                while True:
                    leaf = (lx & lmask) | sub
                    p = float(tab.leaves[t, leaf])
                    for d in range(D):
                        if (free >> d) & 1:
                            f = float(tab.frac[t, (2 << d) - 2 + (leaf & ((2 << d) - 1))])
                            p *= (0.0 if ((leaf ^ lx) >> d) & 1 else 1.0) if f < 0 else f
                    v += p
                    if sub == 0:
                        break
                    sub = (sub - 1) & free
                s = bin(S).count("1")
                for j in range(m):
                    c = tab.weights[m, s - 1] if (S >> j) & 1 else -tab.weights[m, s]
                    phi[i, tab.slot_feat[t, j]] += c * v
    return phi


# ------------------------------------------------------------------------------- the oracle
def test_oracle_local_accuracy_zeros_and_padding():
    m = toy_case()
    X = background(40, 21) * 2
    phi, bv = shapley_oblivious(m, X)
    assert phi.shape == (40, 30) and phi.dtype == np.float64
    assert abs(bv - base_value(m)) == 0
    np.testing.assert_allclose(bv + phi.sum(1), raw_f64(m, m.leaf_index(X)), rtol=0, atol=1e-13)
    unused = np.setdiff1d(np.arange(30), np.unique(m.feat))
    assert unused.size and (phi[:, unused] == 0.0).all()
    assert np.abs(phi[:, np.unique(m.feat)]).max() > 1e-3
    p2, bv2 = shapley_oblivious(m.padded(6, 6), X)
    assert abs(bv2 - bv) < 1e-13
    np.testing.assert_allclose(p2, phi, rtol=0, atol=1e-13)
    # G32 rows of the model's own table give the same leaves, hence the same attributions
    p3, _ = shapley_oblivious(m, m.bin_spec().encode(X))
    assert (p3 == phi).all()


def test_oracle_single_split_closed_form():
    """One depth-1 tree: phi = leaf(x) - cover-weighted mean, base_value = base + that mean."""
    m = ObliviousGBDT(np.array([[4]]), np.array([[0.5]], np.float32), np.array([[-1.0, 3.0]], np.float32), 0.25,
                      cover=np.array([[30.0, 10.0]], np.float32))
    X = np.zeros((2, 30), np.float32)
    X[1, 4] = 1.0
    phi, bv = shapley_oblivious(m, X)
    assert bv == pytest.approx(0.25 + 0.0)                   # (-1 * 30 + 3 * 10) / 40 = 0
    np.testing.assert_allclose(phi[:, 4], [-1.0, 3.0], atol=1e-15)


def test_model_without_cover_is_refused():
    m = ObliviousGBDT.random_init(2, 3, seed=1)
    for fn in (lambda: shapley_oblivious(m, np.zeros((1, 30), np.float32)), lambda: ExplainTable.pack(m)):
        with pytest.raises(ValueError, match="fit_cover"):
            fn()


def test_padded_cover_layout():
    m = toy_case()
    p = m.padded(6, 5)
    assert p.cover.shape == (6, 32)
    assert (p.cover[:4, :16] == m.cover).all() and (p.cover[:4, 16:] == 0).all()
    assert (p.cover[4:, 0] == 60).all() and (p.cover[4:, 1:] == 0).all()
    assert ObliviousGBDT.random_init(2, 3, seed=1).padded(3, 4).cover is None


# ------------------------------------------------------------------------------- the GBX1 table
def test_explain_table_round_trip():
    m, spec, X = edge_case()
    blob = ExplainTable.pack(m, spec)
    assert blob[:4] == b"GBX1" and len(blob) % 16 == 0 and len(blob) == ExplainTable.offsets(3, 4)[-1]
    tab = ExplainTable.unpack(blob)
    assert (tab.feat == m.feat).all() and (tab.k == spec.bin_index(m.feat, m.thr)).all()
    assert (tab.leaves == m.leaves).all() and tab.stamp == spec.stamp
    assert tab.base_value == pytest.approx(base_value(m), abs=1e-6)
    assert list(tab.m) == [1, 3, len(set(m.feat[2].tolist()))]
    assert tab.slot_mask[0, 0] == 0b1111 and tab.slot_feat[0, 0] == 5
    assert tab.k[1, 2] == 255                                 # the NaN level never fires
    for t in range(3):
        for d in range(4):
            assert tab.slot_feat[t, tab.lvl_slot[t, d]] == m.feat[t, d]
            # the two children of a node share its rows, or the node is empty
            f = tab.frac[t, (2 << d) - 2:(4 << d) - 2].reshape(2, 1 << d)
            empty = f[0] < 0
            assert (f[1][empty] < 0).all() and np.allclose((f[0] + f[1])[~empty], 1.0, atol=1e-6)
    assert tab.weights[3, :3].tolist() == pytest.approx([1 / 3, 1 / 6, 1 / 3])
    # the kernel's algorithm on the table is the oracle (up to the f32 rounding of the fractions)
    rows = spec.encode(X[:9])
    rows[4, 31] ^= 1                                          # a stale row
    got = table_shapley(tab, rows)
    want, _ = shapley_oblivious(m, rows, bins=spec)
    assert np.isnan(got[4]).all()
    good = np.arange(9) != 4
    np.testing.assert_allclose(got[good], want[good], rtol=0, atol=20 * unit(m))
    for T, D in ((1, 1), (2, 8), (5, 2)):                     # sizes that are no multiple of 16 B
        mm = random_case(T, D, seed=T + D)
        b = ExplainTable.pack(mm)
        assert len(b) % 16 == 0 and 0 <= len(b) - ExplainTable.offsets(T, D)[-1] < 16
        assert (ExplainTable.unpack(b).frac[:, -2:] == -1).all()   # the spare entries are marked empty
    toy = toy_case()
    with pytest.raises(ValueError, match="8-bit"):
        ExplainTable.pack(toy, toy.bin_spec(bits=5))


def test_cover_key_in_state_dict(tmp_path):
    m = toy_case()
    st = m.state_dict()
    assert st["gbdt.cover"].dtype == np.float32 and (st["gbdt.cover"] == m.cover).all()
    back = ObliviousGBDT.from_state_dict(st)
    assert (back.cover == m.cover).all()
    bare = ObliviousGBDT.random_init(2, 3, seed=1)
    assert "gbdt.cover" not in bare.state_dict() and ObliviousGBDT.from_state_dict(bare.state_dict()).cover is None
    from ccfd_demo_summit_amd.models import load_model, save_model
    save_model(m, str(tmp_path / "m.npz"))
    assert (load_model(str(tmp_path / "m.npz")).cover == m.cover).all()


def test_catboost_leaf_weights_become_cover():
    from ccfd_demo_summit_amd.models.gbdt_import import from_catboost_json, to_catboost_json
    m = toy_case()
    doc = to_catboost_json(m)
    assert from_catboost_json(doc).cover is None
    for t, tree in enumerate(doc["oblivious_trees"]):
        tree["leaf_weights"] = m.cover[t].tolist()
    assert (from_catboost_json(doc).cover == m.cover).all()


def test_trainer_fits_cover():
    from ccfd_demo_summit_amd.train.trainer import train_oblivious_gbdt
    rng = np.random.default_rng(0)
    X = rng.standard_normal((500, 30)).astype(np.float32)
    y = (X[:, 3] + 0.5 * X[:, 7] > 1.0).astype(np.float32)
    m, _ = train_oblivious_gbdt(X, y, n_trees=3, depth=3, n_bins=8, device="cpu")
    assert (m.cover == m.fit_cover(X).cover).all() and (m.cover.sum(1) == 500).all()
    phi, bv = shapley_oblivious(m, X[:5])
    np.testing.assert_allclose(bv + phi.sum(1), raw_f64(m, m.leaf_index(X[:5])), atol=1e-12)


# ------------------------------------------------------------------------------- serving
def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def test_explain_route_cpu_scorer_and_mlp_400():
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.serving import CpuScorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    m = toy_case()
    X = background(5, 31)
    want, bv = shapley_oblivious(m, X)

    async def go():
        srv = SeldonServer(CpuScorer(m), token="s3cret")
        async with TestClient(TestServer(srv.app)) as cl:
            h = {"Authorization": "Bearer s3cret"}
            for path in ("/api/v0.1/explain", "/api/v1.0/explain", "/explain"):
                r = await cl.post(path, json=seldon.build_request(X), headers=h)
                assert r.status == 200
                body = await r.json()
                assert body["data"]["names"] == list(FEATURE_NAMES)
                np.testing.assert_allclose(np.asarray(body["data"]["ndarray"]), want, rtol=0, atol=1e-12)
                tags = body["meta"]["tags"]
                assert set(tags) == {"base_value", "proba"} and tags["base_value"] == pytest.approx(bv)
                np.testing.assert_allclose(tags["proba"], m.predict_proba(X), rtol=1e-6)
            assert (await cl.post("/explain", json=seldon.build_request(X))).status == 401
            assert (await cl.post("/explain", data=b"{nope", headers=h)).status == 400
            assert (await cl.post("/explain", json={"data": {"ndarray": [[1, 2]]}}, headers=h)).status == 400
            r = await cl.post("/predict", json=seldon.build_request(X), headers=h)     # untouched
            assert r.status == 200 and (await r.json())["data"]["names"] == ["proba_0", "proba_1"]
        for other in (build_model("mlp", seed=0, X_ref=X), ObliviousGBDT.random_init(2, 3, seed=1)):
            srv = SeldonServer(CpuScorer(other))
            async with TestClient(TestServer(srv.app)) as cl:
                r = await cl.post("/explain", json=seldon.build_request(X))
                assert r.status == 400
                assert (await r.json())["status"]["status"] == "FAILURE"
    _run(go())


def test_client_explain_url():
    from ccfd_demo_summit_amd.serving.client import SeldonClient
    assert SeldonClient("h:8000").explain_url == "http://h:8000/api/v0.1/explain"
    assert SeldonClient("h:8000", endpoint="predict").explain_url == "http://h:8000/explain"
    assert SeldonClient("h:8000", endpoint="api/v1.0/predictions").explain_url == "http://h:8000/api/v1.0/explain"


# ------------------------------------------------------------------------------- router
def test_router_reasons_reach_the_process_instance():
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.process import ProcessEngine
    from ccfd_demo_summit_amd.process.kie_server import BASE, KieServer
    from ccfd_demo_summit_amd.router.router import Router
    from ccfd_demo_summit_amd.router.rules import RuleSet
    from ccfd_demo_summit_amd.serving import CpuScorer
    m = toy_case()
    X = background(30, 41) * 2
    proba = m.predict_proba(X)
    thr = float(np.sort(proba)[-4])                           # 4 fraud rows
    phi, _ = shapley_oblivious(m, X)

    class Counting(CpuScorer):
        calls = 0

        def explain(self, X):
            Counting.calls += 1
            return super().explain(X)

    eng = ProcessEngine(notification_timeout_s=60)
    router = Router(RuleSet.threshold(thr), eng, explainer=Counting(m), reasons=2)
    out = router.on_scored(np.arange(30) + 1000, np.arange(30), proba, X=X)
    assert out["fraud"] == 4 and Counting.calls == 1          # one batch
    fraud = np.nonzero(proba >= thr)[0]
    for i in fraud:
        inst = eng.get(eng._by_tx[1000 + int(i)])
        why = inst.variables["reasons"]
        assert why == top_reasons(phi[i], FEATURE_NAMES, 2) and len(why) <= 2
        assert all(w["phi"] > 0 for w in why) and why == sorted(why, key=lambda w: -w["phi"])
    assert any(eng.get(eng._by_tx[1000 + int(i)]).variables["reasons"] for i in fraud)

    async def view():
        async with TestClient(TestServer(KieServer(eng).app)) as cl:
            iid = eng._by_tx[1000 + int(fraud[0])]
            r = await cl.get(f"{BASE}/containers/ccd-fraud-kjar/processes/instances/{iid}")
            assert (await r.json())["variables"]["reasons"] == top_reasons(phi[fraud[0]], FEATURE_NAMES, 2)
    _run(view())

    # without an explainer, and on the engine hot path, nothing changes
    eng2 = ProcessEngine(notification_timeout_s=60)
    Router(RuleSet.threshold(thr), eng2).on_scored(np.arange(30) + 1000, np.arange(30), proba, X=X)
    assert all("reasons" not in i.variables for i in eng2.instances.values())
