"""General tree ensembles on the host: TreeEnsemble (models/forest.py) against scikit-learn,
the FRS1 blob and safetensors round trips, the oblivious expansion, the XGBoost JSON
importer (hand-built documents; no XGBoost here) and the routing of the new kind."""
import json

import numpy as np
import pytest

from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import TreeEnsemble, build_model, load_model, save_model
from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
from ccfd_demo_summit_amd.models.sklearn_import import f32_floor, from_sklearn
from ccfd_demo_summit_amd.models.xgboost_import import from_xgboost_json


def proba_bound(m: TreeEnsemble) -> float:
    """fp32 leaf-rounding bound on a probability: every leaf (and the base) is rounded to
    float32 once, relative error 2^-24 each; T of them sum to at most
    T * 2^-23 * (|base| + sum_t max|leaf_t|) with slack 2 for the summation itself, and the
    sigmoid's slope is at most 1/4."""
    return 0.25 * m.n_trees * 2.0 ** -23 * (abs(m.base) + m.leaf_abs_max().sum()) + 1e-6


@pytest.fixture(scope="module")
def data():
    return generate(4000, seed=11)


@pytest.fixture(scope="module")
def estimators(data):
    from sklearn.ensemble import ExtraTreesClassifier, GradientBoostingClassifier, RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier
    X, y = data
    return {
        "rf": RandomForestClassifier(n_estimators=5, random_state=0).fit(X, y),
        "et": ExtraTreesClassifier(n_estimators=4, max_depth=10, random_state=1).fit(X, y),
        "dt": DecisionTreeClassifier(max_depth=8, random_state=2).fit(X, y),
        "gb": GradientBoostingClassifier(n_estimators=10, max_depth=3, random_state=3).fit(X, y),
    }


def _sk_trees(est):
    name = type(est).__name__
    if name == "DecisionTreeClassifier":
        return [est.tree_]
    if name == "GradientBoostingClassifier":
        return [e.tree_ for e in est.estimators_[:, 0]]
    return [e.tree_ for e in est.estimators_]


def _sk_leaf_values(est, X):
    """float32 of the value at ``tree_.apply(X)``, scaled as the importer documents."""
    trees = _sk_trees(est)
    out = np.empty((X.shape[0], len(trees)), np.float32)
    gb = type(est).__name__ == "GradientBoostingClassifier"
    for k, tr in enumerate(trees):
        at = tr.apply(X)
        if gb:
            v = est.learning_rate * tr.value[:, 0, 0]
        else:
            v = tr.value[:, 0, 1] / tr.value[:, 0, :].sum(1) / len(trees)
        out[:, k] = v[at].astype(np.float32)
    return out


def _adversarial_rows(est, X):
    """For every inner node: a base row with that feature at float32(t), its float32
    predecessor and its successor -- the rows a wrongly rounded threshold misroutes.  The base
    row is one that reaches the node (when the data has one), so the node's test decides."""
    rows = []
    rng = np.random.default_rng(0)
    for tr in _sk_trees(est):
        reach = tr.decision_path(X).tocsc()
        for node in np.flatnonzero(tr.children_left != -1):
            t = np.float32(tr.threshold[node])
            at = reach.indices[reach.indptr[node]:reach.indptr[node + 1]]
            base = X[at[0]] if at.size else X[rng.integers(0, X.shape[0])]
            for v in (t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))):
                r = base.copy()
                r[tr.feature[node]] = v
                rows.append(r)
    return np.asarray(rows, np.float32)


@pytest.mark.parametrize("name", ["rf", "et", "dt", "gb"])
def test_sklearn_leaf_selection_bit_exact(estimators, data, name):
    est = estimators[name]
    m = from_sklearn(est)
    assert m.kind == "forest" and m.n_trees == len(_sk_trees(est))
    assert m.link == ("sigmoid" if name == "gb" else "identity")
    for X in (data[0], _adversarial_rows(est, data[0])):
        got = m.leaf_values(X)
        want = _sk_leaf_values(est, X)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", ["rf", "et", "dt", "gb"])
def test_sklearn_predict_proba_within_fp32_bound(estimators, data, name):
    est = estimators[name]
    m = from_sklearn(est)
    X = np.concatenate([data[0], _adversarial_rows(est, data[0])])
    err = np.abs(m.predict_proba(X).astype(np.float64) - est.predict_proba(X)[:, 1]).max()
    print(f"{name}: max |proba - sklearn| = {err:.3e}, bound {proba_bound(m):.3e}")
    assert err <= proba_bound(m)


def test_round_to_nearest_thresholds_would_misroute(estimators):
    """The rounding rule matters on these very trees: some float64 thresholds round UP to
    float32, and f32_floor moves exactly those one step down."""
    t = np.concatenate([tr.threshold[tr.children_left != -1] for tr in _sk_trees(estimators["rf"])])
    near = t.astype(np.float32)
    down = f32_floor(t)
    assert (down.astype(np.float64) <= t).all()
    assert (np.nextafter(down, np.float32(np.inf)).astype(np.float64) > t).all()
    assert (near.astype(np.float64) > t).any() and (down[near.astype(np.float64) > t] < near[near.astype(np.float64) > t]).all()


def test_gb_init_variants(data):
    from sklearn.ensemble import GradientBoostingClassifier
    from sklearn.linear_model import LogisticRegression
    X, y = data[0][:1500], data[1][:1500]
    y = y.copy(); y[:30] = 1
    z = GradientBoostingClassifier(n_estimators=3, max_depth=2, init="zero", random_state=0).fit(X, y)
    m = from_sklearn(z)
    assert m.base == 0.0
    assert np.abs(m.predict_proba(X).astype(np.float64) - z.predict_proba(X)[:, 1]).max() <= proba_bound(m)
    other = GradientBoostingClassifier(n_estimators=2, max_depth=2, init=LogisticRegression(), random_state=0).fit(X, y)
    with pytest.raises(ValueError, match="init"):
        from_sklearn(other)


@pytest.mark.parametrize("trees,depth,nan", [(100, 6, False), (7, 8, True), (3, 1, False)])
def test_from_oblivious_selects_the_same_leaves(data, trees, depth, nan):
    X = data[0]
    g = build_model("gbdt", seed=4, X_ref=X, gbdt_trees=trees, gbdt_depth=depth)
    if nan:
        g.thr[2, 3] = np.nan
        g.thr[5, 0] = np.nan
    f = TreeEnsemble.from_oblivious(g)
    assert (f.n_trees, f.depth, f.n_nodes) == (trees, depth, trees * ((2 << depth) - 1))
    want = g.leaves[np.arange(trees)[None, :], g.leaf_index(X)]
    np.testing.assert_array_equal(f.leaf_values(X).view(np.uint32), want.view(np.uint32))
    assert np.abs(f.raw_score(X).astype(np.float64) - g.raw_score(X)).max() <= 4 * proba_bound(f)
    np.testing.assert_array_equal(f.raw_score(X), g.raw_score(X))      # same f64 sum of the same leaves


def test_nan_feature_goes_left():
    f = TreeEnsemble([3, 0, 0], [0.5, -1.0, 2.0], [1, 0, 0], [False, True, True], [0], 0.0, "identity")
    X = np.zeros((3, 30), np.float32)
    X[:, 3] = [np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1))]
    np.testing.assert_array_equal(f.leaf_values(X)[:, 0], np.float32([-1.0, -1.0, 2.0]))
    np.testing.assert_array_equal(f.predict_proba(X), np.float32([0.0, 0.0, 1.0]))    # identity link clips


def _same(a: TreeEnsemble, b: TreeEnsemble):
    for k in ("feat", "child", "leaf", "root", "tree_depth"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    np.testing.assert_array_equal(a.value.view(np.uint32), b.value.view(np.uint32))
    assert a.link == b.link


def test_pack_unpack_and_safetensors_round_trip(tmp_path, data, estimators):
    for m in (TreeEnsemble.random_init(9, 7, 0.3, 5, data[0]), from_sklearn(estimators["rf"]),
              from_sklearn(estimators["gb"])):
        blob = m.pack()
        assert blob[:4] == b"FRS1" and len(blob) % 16 == 0
        u = TreeEnsemble.unpack(blob)
        _same(m, u)
        assert np.float32(u.base) == np.float32(m.base)
        assert u.pack() == blob
        path = str(tmp_path / "m.safetensors")
        save_model(m, path)
        l = load_model(path)
        assert isinstance(l, TreeEnsemble) and l.base == m.base
        _same(m, l)
        assert l.pack() == blob
    with pytest.raises(ValueError, match="f32 rows"):
        m.pack(wire=True)
    with pytest.raises(ValueError, match="FRS1"):
        TreeEnsemble.unpack(b"GBT1" + blob[4:])


def test_blob_layout(data):
    m = TreeEnsemble([5, 0, 7, 0, 0], [0.25, 1.5, -3.0, 2.5, 3.5], [1, 0, 3, 0, 0], [0, 1, 0, 1, 1], [0], 0.75, "sigmoid")
    blob = m.pack()
    hdr = np.frombuffer(blob, np.int32, 6)
    assert hdr[1] == 1 and hdr[2] == 1 and hdr[3] == 2 and hdr[5] == 5
    assert np.frombuffer(blob, np.float32, 1, 16)[0] == np.float32(0.75)
    np.testing.assert_array_equal(np.frombuffer(blob, np.int32, 2, 64), [0, 2])
    node = np.frombuffer(blob, np.uint32, 10, 80).reshape(5, 2)
    np.testing.assert_array_equal(node[:, 0], [5 | 1 << 8, 32 | 1 << 8, 7 | 3 << 8, 32 | 3 << 8, 32 | 4 << 8])
    np.testing.assert_array_equal(node[:, 1].view(np.float32), np.float32([0.25, 1.5, -3.0, 2.5, 3.5]))
    assert m.pack()[4:8] != TreeEnsemble(m.feat, m.value, m.child, m.leaf, m.root, 0.75, "identity").pack()[4:8]


def test_random_init_reproducible(data):
    a = TreeEnsemble.random_init(12, 9, 0.25, 7, data[0])
    b = TreeEnsemble.random_init(12, 9, 0.25, 7, data[0])
    c = TreeEnsemble.random_init(12, 9, 0.25, 8, data[0])
    assert a.pack() == b.pack() and a.pack() != c.pack()
    assert a.n_trees == 12 and 1 <= a.depth <= 9
    assert len(set(a.tree_depth.tolist())) > 1 or a.n_nodes < 12 * ((2 << 9) - 1)      # unbalanced
    # thresholds come from the reference data: most splits actually partition it
    lv = a.leaf_node(data[0])
    assert np.mean([len(np.unique(lv[:, t])) > 1 for t in range(12)]) > 0.9


def _chain(n):
    """One tree of depth n: every right child splits again, every left child is a leaf.
    Node 0 is the root; inner node 2i has children (2i + 1, 2i + 2); values = node index."""
    feat = [1] + [0, 1] * (n - 1) + [0, 0]
    leaf = [False] + [True, False] * (n - 1) + [True, True]
    child = [1] + [0, 0] * (n - 1) + [0, 0]
    for i in range(n - 1):
        child[2 + 2 * i] = 3 + 2 * i
    return dict(feat=feat, value=np.arange(len(feat), dtype=np.float32), child=child, leaf=leaf, root=[0])


def test_validation_errors():
    ok = dict(feat=[3, 0, 0], value=[0.5, 1.0, 2.0], child=[1, 0, 0], leaf=[False, True, True], root=[0])
    TreeEnsemble(**ok)
    TreeEnsemble([0], [1.0], [0], [True], [0])                                        # single leaf, depth 0
    with pytest.raises(ValueError, match="feature index"):
        TreeEnsemble(**{**ok, "feat": [30, 0, 0]})
    with pytest.raises(ValueError, match="feature index"):
        TreeEnsemble(**{**ok, "feat": [-1, 0, 0]})
    with pytest.raises(ValueError, match="out of range"):
        TreeEnsemble(**{**ok, "child": [2, 0, 0]})                                     # right child = 3
    with pytest.raises(ValueError, match="forward"):
        TreeEnsemble(**{**ok, "child": [0, 0, 0]})
    with pytest.raises(ValueError, match="two parents"):                               # nodes 0 and 1 share children
        TreeEnsemble([1, 2, 0, 0], [0.0, 0.0, 1.0, 2.0], [1, 2, 0, 0], [False, False, True, True], [0])
    with pytest.raises(ValueError, match="two parents"):                               # a root that is a child
        TreeEnsemble(**{**ok, "root": [0, 1]})
    with pytest.raises(ValueError, match="link"):
        TreeEnsemble(**ok, link="probit")
    with pytest.raises(ValueError, match="depth exceeds 64"):
        TreeEnsemble(**_chain(65))


def test_depth_64_chain_is_legal():
    n = 64
    m = TreeEnsemble(**_chain(n))
    assert m.depth == 64 and m.n_nodes == 2 * n + 1
    X = np.full((2, 30), 1e9, np.float32)
    X[1, 1] = -1.0
    np.testing.assert_array_equal(m.leaf_node(X)[:, 0], [2 * n, 1])


# ---------------------------------------------------------------------------- XGBoost JSON
def _xgb_tree(left, right, feat, cond):
    return {"left_children": left, "right_children": right, "split_indices": feat, "split_conditions": cond,
            "split_type": [0] * len(left), "default_left": [0] * len(left), "categories": [],
            "tree_param": {"num_nodes": str(len(left))}}


def _xgb_doc(trees, base_score="5E-1", objective="binary:logistic", booster="gbtree", tree_info=None,
             num_class="0"):
    return {"learner": {"gradient_booster": {"name": booster, "model": {
                "trees": trees, "tree_info": tree_info if tree_info is not None else [0] * len(trees),
                "gbtree_model_param": {"num_trees": str(len(trees))}}},
            "learner_model_param": {"base_score": base_score, "num_class": num_class, "num_feature": "30"},
            "objective": {"name": objective}}, "version": [2, 0, 3]}


# XGBoost numbers nodes breadth-first but children need not be adjacent in general: tree B
# lists the right subtree's children before the left one's
_TA = _xgb_tree([1, -1, -1], [2, -1, -1], [4, 0, 0], [0.5, -0.25, 0.75])
_TB = _xgb_tree([1, 5, 3, -1, -1, -1, -1], [2, 6, 4, -1, -1, -1, -1], [29, 2, 7, 0, 0, 0, 0],
                [100.0, -1.0, 2.0, 0.1, 0.2, 0.3, 0.4])
_TLEAF = _xgb_tree([-1], [-1], [0], [0.125])


def _xgb_ref(trees, base, X):
    z = np.full(X.shape[0], base, np.float64)
    for tr in trees:
        for r in range(X.shape[0]):
            i = 0
            while tr["left_children"][i] != -1:
                t = np.float32(tr["split_conditions"][i])
                i = tr["left_children"][i] if X[r, tr["split_indices"][i]] < t else tr["right_children"][i]
            z[r] += np.float32(tr["split_conditions"][i])
    return z


@pytest.mark.parametrize("base_score,base", [("5E-1", 0.0), ("[2.5E-1]", np.log(0.25 / 0.75))])
def test_xgboost_json_two_and_three_trees(tmp_path, data, base_score, base):
    X = data[0][:300].copy()
    for trees in ([_TA, _TB], [_TA, _TLEAF, _TB]):
        doc = _xgb_doc(trees, base_score)
        m = from_xgboost_json(doc)
        assert m.kind == "forest" and m.link == "sigmoid" and m.n_trees == len(trees)
        assert m.base == pytest.approx(base, abs=1e-12)
        assert m.tree_depth.tolist() == [{3: 1, 7: 2, 1: 0}[len(t["left_children"])] for t in trees]
        ref = _xgb_ref(trees, base, X)
        assert np.abs(m.raw_score(X).astype(np.float64) - ref).max() <= 4 * proba_bound(m)
        # text and path forms
        text = json.dumps(doc)
        path = tmp_path / "m.json"
        path.write_text(text)
        for other in (from_xgboost_json(text), from_xgboost_json(str(path))):
            assert other.pack() == m.pack()


def test_xgboost_row_exactly_on_a_split():
    """XGBoost goes left on x < t: x == t goes right, its float32 predecessor left."""
    m = from_xgboost_json(_xgb_doc([_TA, _TLEAF]))
    t = np.float32(0.5)
    X = np.zeros((3, 30), np.float32)
    X[:, 4] = [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))]
    np.testing.assert_array_equal(m.leaf_values(X)[:, 0], np.float32([0.75, -0.25, 0.75]))
    np.testing.assert_array_equal(m.leaf_values(X)[:, 1], np.float32([0.125] * 3))


def test_xgboost_refusals():
    with pytest.raises(ValueError, match="output group"):
        from_xgboost_json(_xgb_doc([_TA, _TA], tree_info=[0, 1]))
    with pytest.raises(ValueError, match="output group"):
        from_xgboost_json(_xgb_doc([_TA], num_class="3"))
    with pytest.raises(ValueError, match="dart"):
        from_xgboost_json(_xgb_doc([_TA], booster="dart"))
    cat = dict(_TA, split_type=[1, 0, 0])
    with pytest.raises(ValueError, match="categorical"):
        from_xgboost_json(_xgb_doc([cat]))
    with pytest.raises(ValueError, match="feature index 30"):
        from_xgboost_json(_xgb_doc([_xgb_tree([1, -1, -1], [2, -1, -1], [30, 0, 0], [0.5, 1.0, 2.0])]))
    with pytest.raises(ValueError, match="binary:logistic"):
        from_xgboost_json(_xgb_doc([_TA], objective="reg:squarederror"))
    with pytest.raises(ValueError, match="learner"):
        from_xgboost_json({"oblivious_trees": []})
    with pytest.raises(ValueError, match="probability"):
        from_xgboost_json(_xgb_doc([_TA], base_score="0"))


def test_train_cli_imports_xgboost_json(tmp_path, capsys):
    from ccfd_demo_summit_amd.train.__main__ import main
    src, out = tmp_path / "xgb.json", tmp_path / "xgb.safetensors"
    src.write_text(json.dumps(_xgb_doc([_TA, _TLEAF, _TB])))
    assert main(["--from-xgboost", str(src), "--out", str(out)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == {"model": "forest", "imported": str(src), "out": str(out), "trees": 3, "depth": 2, "nodes": 11}
    m = load_model(str(out))
    assert m.kind == "forest" and m.pack() == from_xgboost_json(str(src)).pack()


# ---------------------------------------------------------------------------- refusals, routing
def test_from_sklearn_refusals(data):
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    X, y = data[0][:600], data[1][:600]
    y2 = y.copy(); y2[:20] = 1
    pipe = make_pipeline(StandardScaler(), RandomForestClassifier(n_estimators=2, max_depth=3, random_state=0)).fit(X, y2)
    with pytest.raises(ValueError, match="raw features"):
        from_sklearn(pipe)
    y3 = (np.arange(600) % 3).astype(np.int64)
    rf3 = RandomForestClassifier(n_estimators=2, max_depth=3, random_state=0).fit(X, y3)
    with pytest.raises(ValueError, match="3 classes"):
        from_sklearn(rf3)
    few = RandomForestClassifier(n_estimators=2, max_depth=3, random_state=0).fit(X[:, :10], y2)
    with pytest.raises(ValueError, match="10 features"):
        from_sklearn(few)


def test_row_format_and_scorer_routing(estimators, data):
    from ccfd_demo_summit_amd.parallel.dp import resolve_row_format
    from ccfd_demo_summit_amd.serving.scorers import CpuScorer, make_scorer
    assert resolve_row_format("forest", "auto") == "f32"
    assert resolve_row_format("forest", "f32") == "f32"
    for fmt in ("w64", "g32", "g20"):
        with pytest.raises(ValueError, match="forest"):
            resolve_row_format("forest", fmt)
    m = from_sklearn(estimators["rf"])
    s = make_scorer(m, threshold=0.5, device="cpu")
    assert isinstance(s, CpuScorer)
    p, r = s.score(data[0][:200])
    np.testing.assert_array_equal(p, m.predict_proba(data[0][:200]))
    np.testing.assert_array_equal(r, (p >= 0.5).astype(np.uint8))


def test_kind_registered():
    from ccfd_demo_summit_amd import models
    from ccfd_demo_summit_amd.models.forest import LDS_NODE_BYTES
    assert models.KINDS["forest"] is TreeEnsemble and "TreeEnsemble" in models.__all__
    assert LDS_NODE_BYTES >= 64 * 1024
    assert isinstance(TreeEnsemble.from_oblivious(ObliviousGBDT.random_init(2, 2, 0)), TreeEnsemble)
