"""The general-tree kernel (csrc/kernels/score_forest.hip) against the CPU oracle
``TreeEnsemble.predict_proba``: LDS-resident and global-memory node tables, every row-count
edge of the 64-row chunking, both links, strided rows, rules, the streaming engine in launch
mode with a hot swap, and the GPU scorer."""
import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import TreeEnsemble, build_model
from ccfd_demo_summit_amd.models.forest import LDS_NODE_BYTES, NODE_BYTES
from tests.helpers.forest_cases import _chain, _concat, proba_bound
from tests.helpers.forest_cases import check_counters_f32 as _check_counters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    return generate(70001, seed=11)


@pytest.fixture(scope="module")
def ensembles(data):
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier
    from ccfd_demo_summit_amd.models.sklearn_import import from_sklearn
    X, y = data[0][:4000], data[1][:4000]
    one_leaf = TreeEnsemble([0], [0.375], [0], [True], [0])
    e = {
        "t1": TreeEnsemble.random_init(1, 6, 0.2, 1, X),
        "t3": TreeEnsemble.random_init(3, 5, 0.2, 2, X),          # wave 3 has no tree
        "t5": TreeEnsemble.random_init(5, 7, 0.25, 3, X),
        "t21": TreeEnsemble.random_init(21, 6, 0.2, 9, X),        # 4-tree groups and single-tree tails per wave
        "leaf_only_among": _concat([TreeEnsemble.random_init(2, 4, 0.2, 4, X), one_leaf,
                                    TreeEnsemble.random_init(3, 4, 0.2, 5, X)]),
        "stumps": TreeEnsemble.random_init(9, 1, 0.0, 6, X),
        "chain24": _concat([_chain(24, X, 7), TreeEnsemble.random_init(2, 3, 0.2, 8, X)]),
        "lds_below": TreeEnsemble.random_init(64, 12, 0.295, 3, X),
        "lds_above": TreeEnsemble.random_init(64, 12, 0.3, 4, X),
        "rf_identity": from_sklearn(RandomForestClassifier(n_estimators=5, random_state=0).fit(X, y)),
        "gb_sigmoid": from_sklearn(GradientBoostingClassifier(n_estimators=10, max_depth=3, random_state=3).fit(X, y)),
    }
    assert e["stumps"].depth == 1 and e["chain24"].depth == 24 and e["leaf_only_among"].tree_depth[2] == 0
    assert 0.95 * LDS_NODE_BYTES < e["lds_below"].n_nodes * NODE_BYTES <= LDS_NODE_BYTES
    assert LDS_NODE_BYTES < e["lds_above"].n_nodes * NODE_BYTES < 1.05 * LDS_NODE_BYTES
    assert e["rf_identity"].link == "identity" and e["gb_sigmoid"].link == "sigmoid"
    return e


_oracle_cache = {}


def _oracle(name, m, X):
    key = (name, X.shape[0])
    if key not in _oracle_cache:
        _oracle_cache[key] = m.predict_proba(X)
    return _oracle_cache[key]


NAMES = ["t1", "t3", "t5", "t21", "leaf_only_among", "stumps", "chain24", "lds_below", "lds_above", "rf_identity",
         "gb_sigmoid"]
# every ensemble at 65 rows; every row-count edge on a small LDS-resident ensemble and on the
# global-memory path; and the sizes past one workgroup wave, where a workgroup walks several
# chunks with the next one prefetched: 256 x 4 chunks for a small table, 256 x 1 for a large one
CASES = [(k, 65) for k in NAMES] + [(k, n) for k in ("t5", "lds_above") for n in (1, 63, 64, 4097)] + \
        [("rf_identity", 4097), ("t5", 70001), ("lds_below", 20001)]


@pytest.mark.parametrize("name,n", CASES)
def test_forest_kernel_matches_oracle(gpu, data, ensembles, name, n):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_counters, score
    m = ensembles[name]
    X = data[0][:n]
    dm = DeviceModel(m, gpu)
    assert dm.row_format == "f32" and (dm.trees, dm.depth) == (m.n_trees, m.depth)
    cnt = new_counters(gpu)
    p, r = score(dm, torch.from_numpy(X).to(gpu), 0.5, counters=cnt)
    torch.cuda.synchronize()
    p, r = p.cpu().numpy(), r.cpu().numpy()
    err = np.abs(p.astype(np.float64) - _oracle(name, m, X)).max()
    print(f"{name} n={n}: nodes {m.n_nodes}, max |p - oracle| = {err:.3e}, bound {proba_bound(m):.3e}")
    assert err <= proba_bound(m)
    np.testing.assert_array_equal(r, (p >= 0.5).astype(np.uint8))
    _check_counters(cnt, p, r, X)


def test_forest_matches_oblivious_kernel(gpu, data):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, score
    X = data[0][:4097]
    g = build_model("gbdt", seed=3, X_ref=data[0][:5000], calibrate_rate=0.05)
    f = TreeEnsemble.from_oblivious(g)
    xt = torch.from_numpy(X).to(gpu)
    pg, rg = score(DeviceModel(g, gpu), xt, 0.5)
    pf, rf = score(DeviceModel(f, gpu), xt, 0.5)
    torch.cuda.synchronize()
    pg, rg, pf, rf = (t.cpu().numpy() for t in (pg, rg, pf, rf))
    b = proba_bound(f)
    assert np.abs(pf.astype(np.float64) - f.predict_proba(X)).max() <= b
    assert np.abs(pf.astype(np.float64) - pg).max() <= 2 * b
    clear = np.abs(pg - 0.5) > 2 * b
    assert clear.sum() > 4000 and 0 < rg.sum() < 4097
    np.testing.assert_array_equal(rf[clear], rg[clear])


def test_forest_strided_input(gpu, data, ensembles):
    """ld = 32 takes the generic (non-contiguous) loader."""
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_counters, score
    X = data[0][:1000]
    big = np.full((1000, 32), 7.0, np.float32)
    big[:, :30] = X
    xt = torch.from_numpy(big).to(gpu)[:, :30]
    assert xt.stride(0) == 32
    for name in ("t5", "lds_above"):
        m = ensembles[name]
        cnt = new_counters(gpu)
        p, r = score(DeviceModel(m, gpu), xt, 0.5, counters=cnt)
        torch.cuda.synchronize()
        p, r = p.cpu().numpy(), r.cpu().numpy()
        assert np.abs(p.astype(np.float64) - m.predict_proba(X)).max() <= proba_bound(m)
        _check_counters(cnt, p, r, X)


def test_forest_rules_epilogue(gpu, data, ensembles):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, DeviceRules, new_counters, score
    from ccfd_demo_summit_amd.router.rules import RuleSet
    X = data[0][:4097]
    m = ensembles["gb_sigmoid"]
    rs = RuleSet.parse("when amount > 200 and proba >= 0.001 then fraud\n"
                       "when V17 < -2.5 or abs(V14) > 4 then fraud\notherwise standard")
    assert rs.feature_vars()
    cnt = new_counters(gpu)
    p, r = score(DeviceModel(m, gpu), torch.from_numpy(X).to(gpu), 0.5, counters=cnt, rules=DeviceRules(rs, gpu))
    torch.cuda.synchronize()
    p, r = p.cpu().numpy(), r.cpu().numpy()
    assert np.abs(p.astype(np.float64) - m.predict_proba(X)).max() <= proba_bound(m)
    want = rs.evaluate(p, X=X)
    assert 0 < want.sum() < 4097
    np.testing.assert_array_equal(r, want)
    _check_counters(cnt, p, r, X)


def test_forest_refuses_other_row_formats(gpu, ensembles):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    with pytest.raises(ValueError, match="f32 rows"):
        DeviceModel(ensembles["t5"], gpu, wire=True)
    with pytest.raises(ValueError, match="f32 rows"):
        DeviceModel(ensembles["t5"], gpu, bins=True)


def test_forest_stream_engine_launch_mode_and_swap(gpu, data, ensembles):
    from ccfd_demo_summit_amd.engine import StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    X = data[0][:5000]
    a, b = ensembles["gb_sigmoid"], ensembles["lds_above"]
    assert (a.n_nodes, a.n_trees) != (b.n_nodes, b.n_trees)
    eng = StreamEngine(DeviceModel(a, gpu), batch=4096, depth=2, streams=1, input_mode="dma",
                       output_mode="zerocopy", threshold=0.5)
    try:
        p, r = eng.score(X)
        assert np.abs(p.astype(np.float64) - a.predict_proba(X)).max() <= proba_bound(a)
        np.testing.assert_array_equal(r, (p >= 0.5).astype(np.uint8))
        eng.swap_model(DeviceModel(b, gpu))
        p, r = eng.score(X)
        assert np.abs(p.astype(np.float64) - b.predict_proba(X)).max() <= proba_bound(b)
        np.testing.assert_array_equal(r, (p >= 0.5).astype(np.uint8))
        with pytest.raises(ValueError, match="same kind"):
            eng.swap_model(DeviceModel(build_model("lr", seed=1), gpu))
    finally:
        eng.close()


def test_forest_persistent_mode_is_refused(gpu, ensembles):
    """A host-side check at construction, before any launch."""
    from ccfd_demo_summit_amd.engine import StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    with pytest.raises(RuntimeError, match="forest"):
        StreamEngine(DeviceModel(ensembles["t5"], gpu), batch=1024, depth=2, streams=1, input_mode="zerocopy",
                     output_mode="zerocopy", exec_mode="persistent")


def test_forest_gpu_scorer_and_seldon_predict(gpu, data, tmp_path):
    """fitted RandomForest -> from_sklearn -> save -> load -> GPU scorer -> Seldon predict():
    the estimator's own probabilities come back."""
    import asyncio
    from aiohttp.test_utils import TestClient, TestServer
    from sklearn.ensemble import RandomForestClassifier
    from ccfd_demo_summit_amd.contracts import seldon
    from ccfd_demo_summit_amd.models import load_model, save_model
    from ccfd_demo_summit_amd.models.sklearn_import import from_sklearn
    from ccfd_demo_summit_amd.serving.scorers import GpuScorer, make_scorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    rf = RandomForestClassifier(n_estimators=5, random_state=0).fit(data[0][:4000], data[1][:4000])
    path = str(tmp_path / "rf.safetensors")
    save_model(from_sklearn(rf), path)
    m = load_model(path)
    X = data[0][4000:4300]
    want = rf.predict_proba(X)[:, 1]
    s = make_scorer(m, threshold=0.5, device="gpu")
    try:
        assert isinstance(s, GpuScorer)
        p, r = s.score(X)
        assert np.abs(p.astype(np.float64) - m.predict_proba(X)).max() <= proba_bound(m)
        assert np.abs(p.astype(np.float64) - want).max() <= 2 * proba_bound(m)
        np.testing.assert_array_equal(r, (p >= 0.5).astype(np.uint8))

        async def go():
            srv = SeldonServer(s, max_batch=256, max_delay_us=1000)
            async with TestClient(TestServer(srv.app)) as cl:
                q = await cl.post("/api/v0.1/predictions", json=seldon.build_request(X[:40]))
                assert q.status == 200
                body = await q.json()
                assert body["data"]["names"] == ["proba_0", "proba_1"]
                got = np.asarray(seldon.proba1_from_response(body), np.float64)
                assert np.abs(got - want[:40]).max() <= 2 * proba_bound(m)
        asyncio.new_event_loop().run_until_complete(go())
    finally:
        s.close()
