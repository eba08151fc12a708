"""Exact Shapley attributions of general tree ensembles, CPU side: the cover of ``TreeEnsemble``
and its importers, the two oracles, the FRX1 table and the emulator of the kernel's algorithm on
it, the /explain route and the router's ``reasons``.

The builders at the top are shared with tests/test_explain_forest_gpu.py."""
import asyncio

import numpy as np
import pytest

from test_explain_cpu import background, edge_case, random_case, toy_case

from ccfd_demo_summit_amd.contracts import seldon
from ccfd_demo_summit_amd.contracts.transaction import FEATURE_NAMES
from ccfd_demo_summit_amd.models import build_model, load_model, save_model
from ccfd_demo_summit_amd.models.explain import shapley_oblivious, top_reasons
from ccfd_demo_summit_amd.models.explain_forest import (ForestExplainTable, forest_base_value, forest_paths,
                                                        shapley_forest, shapley_forest_enum, table_shapley_forest)
from ccfd_demo_summit_amd.models.forest import TreeEnsemble
from ccfd_demo_summit_amd.models.gbdt import BinSpec


# ------------------------------------------------------------------------------- shared builders
def concat(models, base=0.0, link="sigmoid"):
    """One ensemble of the trees of several, covers included."""
    off = np.cumsum([0] + [m.n_nodes for m in models])
    return TreeEnsemble(np.concatenate([m.feat for m in models]), np.concatenate([m.value for m in models]),
                        np.concatenate([m.child + o for m, o in zip(models, off)]),
                        np.concatenate([m.leaf for m in models]),
                        np.concatenate([m.root + o for m, o in zip(models, off)]), base, link,
                        cover=np.concatenate([m.cover for m in models]))


def single_leaf(value, rows):
    return TreeEnsemble([0], [value], [0], [True], [0], cover=[rows])


def chain(feats, thr, seed):
    """One tree that tests ``feats`` one after the other: left is a leaf, right goes on."""
    d = len(feats)
    rng = np.random.default_rng(seed)
    feat, value, child, leaf = (np.zeros(2 * d + 1, t) for t in (np.int32, np.float32, np.int32, bool))
    leaf[:] = True
    value[:] = rng.standard_normal(2 * d + 1) * 0.2
    for i, f in enumerate(feats):
        feat[2 * i], value[2 * i], child[2 * i], leaf[2 * i] = f, thr[i], 2 * i + 1, False
    return TreeEnsemble(feat, value, child, leaf, [0])


def random_forest_case(T, depth, seed, n_bg, p_leaf=0.2, base=-0.75, n_feats=30):
    """Random unbalanced trees over the first ``n_feats`` features with cover from ``n_bg``
    background rows (few rows leave empty nodes, which become gates) and a non-zero base."""
    bg = background(max(n_bg, 40), 500 + seed)
    m = TreeEnsemble.random_init(T, depth, p_leaf=p_leaf, seed=seed, X_ref=bg)
    m = TreeEnsemble(m.feat % n_feats, m.value, m.child, m.leaf, m.root, base)
    return m.fit_cover(bg[:n_bg])


def forest_unit(model):
    """u = 2^-24 * sum_t max |leaf_t|: the tolerance unit of the attributions."""
    return 2.0 ** -24 * float(model.leaf_abs_max().sum())


def forest_raw_f64(model, X):
    return model.base + model.leaf_values(X).astype(np.float64).sum(1)


def node_kinds(model):
    """(reachable empty inner nodes, non-empty inner nodes with a child of cover 0)."""
    inner = np.flatnonzero(~model.leaf & (model.node_tree >= 0))
    c = model.child[inner]
    tot = model.cover[c].astype(np.float64) + model.cover[c + 1]
    return inner[tot == 0], inner[(tot > 0) & ((model.cover[c] == 0) | (model.cover[c + 1] == 0))]


def player_features(model):
    return sorted({f for p in forest_paths(model)[0] for f in p.feats})


def gpu_cases():
    """name -> (ensemble, bin spec, X float32 [n,30]): the cases of tests/test_explain_forest_gpu.py."""
    out = {}

    def add(name, m, n=65, seed=0, spec=None):
        out[name] = (m, spec if spec is not None else m.bin_spec(), background(n, 700 + seed) * 1.5)

    bg = background(300, 901)
    add("stump", chain([4], [0.25], 1).fit_cover(bg), seed=1)
    sparse = random_forest_case(5, 8, seed=21, n_bg=40)                  # 40 rows: most deep nodes are empty
    assert node_kinds(sparse)[0].size > 20 and node_kinds(sparse)[1].size > 5
    add("sparse_d8", sparse, seed=2)
    for n in (1, 63, 64, 257):                                           # 65 rows: every other case
        add(f"rows_{n}", sparse, n=n, seed=10 + n)
    beside = concat([random_forest_case(2, 4, seed=22, n_bg=200), single_leaf(0.375, 200),
                     random_forest_case(1, 3, seed=23, n_bg=200)], base=0.5)
    add("single_leaf_beside", beside, seed=3)
    c16 = chain(list(range(3, 19)), np.full(16, -1.5, np.float32), 2).fit_cover(bg)
    assert (c16.cover[c16.leaf] > 0).all()                               # 16 players on the last path
    add("chain_16", c16, seed=4)
    odd = random_forest_case(7, 5, seed=24, n_bg=300)
    add("odd_7_trees", odd, seed=5)
    many = random_forest_case(13, 8, seed=25, n_bg=300, p_leaf=0.08)
    add("slices", many, seed=6)
    obl = random_case(100, 6, seed=606)
    add("oblivious_100x6", TreeEnsemble.from_oblivious(obl), seed=7, spec=obl.bin_spec())
    return out


# ------------------------------------------------------------------------------- the model layer
def test_cover_field_validation_and_fit_cover():
    bg = background(50, 1)
    m = TreeEnsemble.random_init(3, 4, seed=1, X_ref=bg)
    assert m.cover is None
    c = m.fit_cover(bg)
    assert c is not m and m.cover is None and c.cover.dtype == np.float32 and c.cover.shape == (m.n_nodes,)
    assert (c.cover[c.root] == 50).all()
    inner = np.flatnonzero(~c.leaf)
    assert (c.cover[c.child[inner]] + c.cover[c.child[inner] + 1] == c.cover[inner]).all()
    leaves = c.leaf_node(bg)
    assert (np.bincount(leaves.reshape(-1), minlength=c.n_nodes)[c.leaf] == c.cover[c.leaf]).all()
    args = (m.feat, m.value, m.child, m.leaf, m.root)
    for bad in (np.ones(m.n_nodes - 1), -np.ones(m.n_nodes), np.full(m.n_nodes, np.nan), np.full(m.n_nodes, np.inf)):
        with pytest.raises(ValueError, match="cover"):
            TreeEnsemble(*args, cover=bad)
    with pytest.raises(ValueError, match="30"):
        m.fit_cover(bg[:, :29])


def test_state_dict_round_trip_with_and_without_cover(tmp_path):
    bg = background(50, 2)
    bare = TreeEnsemble.random_init(3, 4, seed=2, X_ref=bg)
    m = bare.fit_cover(bg)
    st = m.state_dict()
    assert st["forest.cover"].dtype == np.float32 and (TreeEnsemble.from_state_dict(st).cover == m.cover).all()
    assert "forest.cover" not in bare.state_dict() and TreeEnsemble.from_state_dict(bare.state_dict()).cover is None
    save_model(m, str(tmp_path / "m.npz"))
    back = load_model(str(tmp_path / "m.npz"))
    assert (back.cover == m.cover).all() and (back.value == m.value).all()
    save_model(bare, str(tmp_path / "b.npz"))
    assert load_model(str(tmp_path / "b.npz")).cover is None
    # the kernels' scoring blobs do not change with cover
    assert m.pack() == bare.pack() and m.pack(bins=m.bin_spec()) == bare.pack(bins=bare.bin_spec())
    assert TreeEnsemble.unpack(m.pack()).cover is None


def test_from_oblivious_carries_cover():
    m = toy_case()
    te = TreeEnsemble.from_oblivious(m)
    assert te.cover is not None and (te.cover[te.root] == m.cover.sum(1)).all()
    assert (te.cover == te.fit_cover(background(60, 7)).cover).all()       # toy_case's own background
    from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
    assert TreeEnsemble.from_oblivious(ObliviousGBDT.random_init(2, 3, seed=1)).cover is None


def test_sklearn_cover_is_fit_cover():
    from sklearn.ensemble import GradientBoostingClassifier
    from sklearn.tree import DecisionTreeClassifier
    from ccfd_demo_summit_amd.models.sklearn_import import from_sklearn
    rng = np.random.default_rng(5)
    X = rng.standard_normal((400, 30)).astype(np.float32)
    y = (X[:, 3] + 0.5 * X[:, 7] * X[:, 1] + 0.3 * rng.standard_normal(400) > 0.8).astype(int)
    for est in (DecisionTreeClassifier(max_depth=6, random_state=0),
                GradientBoostingClassifier(n_estimators=5, max_depth=3, subsample=1.0, random_state=0)):
        m = from_sklearn(est.fit(X, y))
        assert m.cover is not None and m.cover.dtype == np.float32
        assert (m.cover == m.fit_cover(X).cover).all() and (m.cover[m.root] == 400).all()
        phi, bv = shapley_forest(m, X[:9])
        np.testing.assert_allclose(bv + phi.sum(1), forest_raw_f64(m, X[:9]), rtol=0, atol=1e-12)


def _xgb_doc(with_hessian=(True, True)):
    def tree(left, right, split, cond, hess, keep):
        t = {"left_children": left, "right_children": right, "split_indices": split, "split_conditions": cond}
        if keep:
            t["sum_hessian"] = hess
        return t
    # tree 0: node 0 -> (1, 2), node 2 -> (3, 4), stored with the children of 2 before node 2's sibling
    trees = [tree([1, -1, 3, -1, -1], [2, -1, 4, -1, -1], [2, 0, 5, 0, 0], [0.5, -0.1, 1.5, 0.2, 0.3],
                  [10.0, 4.0, 6.0, 1.5, 4.5], with_hessian[0]),
             tree([2, -1, -1], [1, -1, -1], [7, 0, 0], [0.0, 0.4, -0.4], [10.0, 7.0, 3.0], with_hessian[1])]
    return {"learner": {"objective": {"name": "binary:logistic"}, "learner_model_param": {"base_score": "5E-1"},
                        "gradient_booster": {"name": "gbtree", "model": {"trees": trees, "tree_info": [0, 0]}}}}


def test_xgboost_sum_hessian_becomes_cover():
    from ccfd_demo_summit_amd.models.xgboost_import import from_xgboost_json
    m = from_xgboost_json(_xgb_doc())
    # breadth-first per tree; tree 1 lists its right child first, so left = node 2 (hessian 3)
    assert m.cover.dtype == np.float32 and m.cover.tolist() == [10.0, 4.0, 6.0, 1.5, 4.5, 10.0, 3.0, 7.0]
    assert m.value[m.leaf].tolist() == pytest.approx([-0.1, 0.2, 0.3, -0.4, 0.4])
    assert from_xgboost_json(_xgb_doc((True, False))).cover is None
    assert from_xgboost_json(_xgb_doc((False, False))).cover is None
    doc = _xgb_doc()
    doc["learner"]["gradient_booster"]["model"]["trees"][0]["sum_hessian"].pop()
    with pytest.raises(ValueError, match="sum_hessian"):
        from_xgboost_json(doc)
    X = background(6, 3)
    phi, bv = shapley_forest(m, X)
    np.testing.assert_allclose(bv + phi.sum(1), forest_raw_f64(m, X), rtol=0, atol=1e-13)
    assert bv == pytest.approx(-0.1 * 0.4 + 0.6 * (0.2 * 0.25 + 0.3 * 0.75) + (-0.4 * 0.3 + 0.4 * 0.7))


# ------------------------------------------------------------------------------- the oracles
def test_enumeration_equals_the_path_oracle():
    X = background(40, 31) * 1.5
    empties = zero_shares = 0
    for seed in range(6):
        m = random_forest_case(3, 4, seed=seed, n_bg=10, p_leaf=0.1, n_feats=9)
        empty, zero = node_kinds(m)
        empties, zero_shares = empties + empty.size, zero_shares + zero.size
        tol = 1e-12 * float(m.leaf_abs_max().sum())
        want, bv = shapley_forest_enum(m, X)
        got, bv2 = shapley_forest(m, X)
        assert bv == bv2 == forest_base_value(m) and got.dtype == np.float64 and got.shape == (40, 30)
        assert np.abs(got - want).max() <= tol
        raw = forest_raw_f64(m, X)
        assert np.abs(bv + want.sum(1) - raw).max() <= tol and np.abs(bv + got.sum(1) - raw).max() <= tol
        assert np.abs(want).max() > 1e-3
        rows = m.bin_spec().encode(X)                          # binned rows take the same paths
        assert (shapley_forest(m, rows)[0] == got).all() and (shapley_forest_enum(m, rows)[0] == want).all()
    assert empties >= 7 and zero_shares >= 7
    wide = chain(list(range(13)), np.zeros(13, np.float32), 1).fit_cover(background(100, 5))
    with pytest.raises(ValueError, match="13 distinct"):
        shapley_forest_enum(wide, X)
    assert shapley_forest(wide, X)[0].shape == (40, 30)


def test_from_oblivious_equals_shapley_oblivious():
    X = background(30, 32) * 2
    m_edge, spec_edge, X_edge = edge_case()
    for m, rows, spec in ((random_case(5, 6, seed=9, n_bg=60), X, None), (toy_case().padded(6, 5), X, None),
                          (toy_case().padded(4, 5), X, None), (m_edge, X_edge, None),
                          (m_edge, spec_edge.encode(X_edge), spec_edge)):
        te = TreeEnsemble.from_oblivious(m)
        want, bv = shapley_oblivious(m, rows, bins=spec)
        got, bv2 = shapley_forest(te, rows, bins=spec)
        assert abs(bv - bv2) <= 1e-13 and np.abs(got - want).max() <= 1e-13
        unused = np.setdiff1d(np.arange(30), np.unique(m.feat))
        assert (got[:, unused] == 0.0).all()
    # a G20 spec decodes to the same bins
    m = random_case(3, 3, seed=4)
    te = TreeEnsemble.from_oblivious(m)
    s5 = te.bin_spec(bits=5)
    assert (shapley_forest(te, s5.encode(X), bins=s5)[0] == shapley_forest(te, X)[0]).all()


def test_unused_and_gated_features_get_exact_zero():
    # feature 9 is tested only below a node that no background row reaches
    feat = [2, 0, 9, 0, 0, 0, 0]
    value = [0.0, 1.0, 0.5, 2.0, -3.0, 4.0, -5.0]
    child = [1, 3, 5, 0, 0, 0, 0]
    leaf = [False, False, False, True, True, True, True]
    m = TreeEnsemble(feat, value, child, leaf, [0], 0.25, cover=[8, 8, 0, 3, 5, 0, 0])
    X = background(20, 33)
    X[:10, 2] = 1.0                                           # into the empty subtree
    for fn in (shapley_forest, shapley_forest_enum):
        phi, bv = fn(m, X)
        assert bv == 0.25 + (2.0 * 3 - 3.0 * 5) / 8
        assert (phi[:, [j for j in range(30) if j not in (0, 2)]] == 0.0).all()
        assert np.abs(phi[:10, 2]).min() > 0 and (phi[10:][X[10:, 2] <= 0, 2] == 0).all()
        np.testing.assert_allclose(bv + phi.sum(1), forest_raw_f64(m, X), rtol=0, atol=1e-14)
    assert player_features(m) == [0, 2]
    # an empty root has no constant base value
    empty_root = TreeEnsemble(feat, value, child, leaf, [0], cover=np.zeros(7))
    for fn in (shapley_forest, shapley_forest_enum, forest_base_value, ForestExplainTable.pack):
        with pytest.raises(ValueError, match="base value"):
            fn(empty_root, X) if fn in (shapley_forest, shapley_forest_enum) else fn(empty_root)
    with pytest.raises(ValueError, match="fit_cover"):
        shapley_forest(TreeEnsemble(feat, value, child, leaf, [0]), X)


def test_depth_zero_tree_moves_only_the_base_value():
    bg = background(100, 34)
    real = random_forest_case(2, 3, seed=3, n_bg=100)
    both = concat([real, single_leaf(0.625, 100)], base=real.base)
    X = background(10, 35)
    a, bva = shapley_forest(real, X)
    b, bvb = shapley_forest(both, X)
    assert (a == b).all() and bvb == pytest.approx(bva + 0.625, abs=1e-15)
    alone = single_leaf(-0.5, 3)
    phi, bv = shapley_forest(alone, X)
    assert (phi == 0).all() and bv == -0.5 and (shapley_forest_enum(alone, X)[0] == 0).all()
    tab = ForestExplainTable.unpack(ForestExplainTable.pack(alone, BinSpec([np.zeros(0, np.float32)] * 30)))
    assert tab.paths == 0 and tab.slices == 1 and tab.base_value == -0.5
    assert bg.shape == (100, 30)


def _triple(thr, dirs, cover_rows):
    """feature 6 tested three times on the way to the last leaf; ``dirs`` = directions of that path."""
    n = 7
    feat, value, child, leaf = np.full(n, 6), np.zeros(n, np.float32), np.zeros(n, np.int32), np.ones(n, bool)
    at = 0
    for i, (t, d) in enumerate(zip(thr, dirs)):
        feat[at], value[at], child[at], leaf[at] = 6, t, 2 * i + 1, False
        value[2 * i + 1 + (1 - d)] = 0.1 * (i + 1)            # the sibling leaf
        at = 2 * i + 1 + d
    value[at] = 1.0
    return TreeEnsemble(feat, value, child, leaf, [0]).fit_cover(cover_rows), at


def test_repeated_feature_merges_to_one_interval():
    bg = background(200, 36)
    m, last = _triple([-0.5, 0.75, 0.25], [1, 0, 1], bg)       # -0.5 < x, x <= 0.75, 0.25 < x
    spec = m.bin_spec()
    assert spec.edges[6].tolist() == [-0.5, 0.25, 0.75]
    tab = ForestExplainTable.unpack(ForestExplainTable.pack(m, spec))
    assert tab.paths == 4 and tab.width == 4 and (tab.m == 1).all() and (tab.feat[:, 0] == 6).all()
    p = int(np.flatnonzero(tab.leaf == 1.0)[0])
    assert (tab.lo[p, 0], tab.hi[p, 0]) == (1, 2)              # bin 2 only: 0.25 < x <= 0.75
    path = [q for q in forest_paths(m)[0] if q.leaf == 1.0][0]
    c = m.cover.astype(np.float64)
    assert path.z[0] == pytest.approx(c[last] / c[0]) and len(path.splits[0]) == 3
    # an interval no row satisfies: x > 0.75 and then x <= 0.25; the leaf still enters through its share
    m2, last2 = _triple([0.75, 0.25, -0.5], [1, 0, 1], bg)
    assert m2.cover[last2] == 0
    tab2 = ForestExplainTable.unpack(ForestExplainTable.pack(m2, m2.bin_spec()))
    p2 = int(np.flatnonzero(tab2.leaf == 1.0)[0])
    assert tab2.paths == 4 and tab2.lo[p2, 0] >= tab2.hi[p2, 0]
    X = background(50, 37)
    for mm in (m, m2):
        want, bv = shapley_forest_enum(mm, X)
        got, _ = shapley_forest(mm, X)
        assert np.abs(got - want).max() <= 1e-15 and (got[:, np.arange(30) != 6] == 0).all()
        rows = mm.bin_spec().encode(X)
        emu = table_shapley_forest(ForestExplainTable.unpack(ForestExplainTable.pack(mm)), rows, np.float64)
        assert np.abs(emu - want).max() <= 1e-7


def test_nan_thresholds_and_the_end_bins():
    edges5 = np.linspace(-2.0, 2.0, 255).astype(np.float32)
    bg = background(300, 38)
    m = chain([5, 8, 5, 11], [edges5[0], np.nan, edges5[254], 0.0], 3).fit_cover(bg)
    assert m.cover[4] == 0                                     # nothing goes right of the NaN split
    own = m.bin_spec()
    spec = BinSpec([edges5 if j == 5 else own.edges[j] for j in range(30)])
    X = background(40, 39) * 1.5
    X[0, 5], X[1, 5], X[2, 5], X[3, 8] = -9.0, 9.0, 2.0, np.nan
    rows = spec.encode(X)
    assert rows[0, 5] == 0 and rows[1, 5] == 255 and rows[2, 5] == 254
    want, bv = shapley_forest_enum(m, X)
    for r in (X, rows):
        got, bv2 = shapley_forest(m, r, bins=spec)
        assert bv2 == bv and np.abs(got - want).max() <= 1e-15
    # no row passes the NaN split: it is a null player, and feature 11 behind it is gated away
    assert (want[:, [8, 11]] == 0).all() and np.abs(want[:, 5]).min() > 0
    tab = ForestExplainTable.unpack(ForestExplainTable.pack(m, spec))
    assert tab.stamp == spec.stamp and tab.paths == 5 and sorted(len(g) for g in tab.gates) == [0, 0, 1, 2, 2]
    emu = table_shapley_forest(tab, rows, np.float64)
    assert np.abs(emu - want).max() <= 1e-7


# ------------------------------------------------------------------------------- the FRX1 table
def test_table_round_trip_and_emulator():
    m = random_forest_case(5, 6, seed=41, n_bg=30)
    assert node_kinds(m)[0].size > 3
    spec = m.bin_spec()
    blob = ForestExplainTable.pack(m, spec)
    assert blob[:4] == b"FRX1" and len(blob) % 16 == 0
    tab = ForestExplainTable.unpack(blob)
    assert 0 <= len(blob) - ForestExplainTable.offsets(tab.slices, int(np.frombuffer(blob, np.int32, 1, 28)[0]))[-1] < 16
    paths, bv = forest_paths(m)
    assert tab.base_value == pytest.approx(bv, abs=1e-6) and tab.stamp == spec.stamp
    with_players = [p for p in paths if p.feats]
    assert 0 < tab.paths <= len(with_players) and tab.width == 8 and tab.m.max() in (5, 6)
    assert any(tab.gates)
    # the q-point Gauss-Legendre rules on (0, 1): exact for the degree 2 q - 1 integrands of 2 q players
    assert tab.rules.shape == (8, 2, 8)
    for q in range(1, 9):
        t, w = tab.rules[q - 1]
        assert (t[q:] == 0).all() and (w[q:] == 0).all() and (t[:q] > 0).all() and (t[:q] < 1).all()
        for k in range(2 * q):
            assert (w * t ** k)[:q].sum() == pytest.approx(1 / (k + 1), abs=1e-15)
    # the runs of the waves are consecutive and cover every record
    assert tab.seg[:, :, 1].sum() == tab.paths and tab.seg[0, 0, 0] == 0
    assert (np.diff(tab.seg[:, :, 0].reshape(-1)) >= 0).all()
    # z is the float64 product rounded once
    kept = iter(p for p in with_players)
    for i in range(tab.paths):
        p = next(kept)
        while len(p.feats) != tab.m[i] or np.float32(p.leaf) != tab.leaf[i] or p.feats != tab.feat[i, :tab.m[i]].tolist():
            p = next(kept)                                    # dropped: its gates contradict each other
        assert (tab.z[i, :tab.m[i]] == np.array(p.z, np.float64).astype(np.float32)).all()
    X = background(33, 42) * 1.5
    rows = spec.encode(X)
    rows[4, 31] ^= 1                                          # a stale row
    want, _ = shapley_forest(m, rows, bins=spec)
    good = np.arange(33) != 4
    u = forest_unit(m)
    e64 = table_shapley_forest(tab, rows, np.float64)
    e32 = table_shapley_forest(tab, rows, np.float32)
    assert np.isnan(e64[4]).all() and np.isnan(e32[4]).all() and e32.dtype == np.float32
    assert np.abs(e64[good] - want[good]).max() <= 2 * u      # z rounded to f32: 2^-24 relative a path
    assert np.abs(e32[good] - want[good]).max() <= 8 * u
    unused = [j for j in range(30) if j not in player_features(m)]
    assert unused and (e32[good][:, unused] == 0).all()
    with pytest.raises(ValueError, match="8-bit"):
        ForestExplainTable.pack(m, m.bin_spec(bits=5))
    with pytest.raises(ValueError, match="FRX1"):
        ForestExplainTable.unpack(b"GBX1" + blob[4:])
    with pytest.raises(ValueError, match="truncated"):
        ForestExplainTable.unpack(blob[:-32])


def test_slices_are_fixed_at_pack_time():
    m = gpu_cases()["slices"][0]
    tab = ForestExplainTable.unpack(ForestExplainTable.pack(m))
    assert tab.slices >= 2 and tab.slices == -(-tab.paths // 512) and tab.seg.shape == (tab.slices, 4, 2)
    odd = gpu_cases()["odd_7_trees"][0]
    assert odd.n_trees == 7 and ForestExplainTable.unpack(ForestExplainTable.pack(odd)).paths % 4 != 0


def test_width_17_is_refused_by_the_table_only():
    bg = background(400, 43)
    feats = list(range(17))
    m = chain(feats, np.full(17, -1.8, np.float32), 4).fit_cover(bg)
    assert (m.cover[m.leaf] > 0).all()
    with pytest.raises(ValueError, match=r"tree 0.*17"):
        ForestExplainTable.pack(m)
    X = background(8, 44)
    phi, bv = shapley_forest(m, X)
    np.testing.assert_allclose(bv + phi.sum(1), forest_raw_f64(m, X), rtol=0, atol=1e-13)
    m16 = gpu_cases()["chain_16"][0]
    assert ForestExplainTable.unpack(ForestExplainTable.pack(m16)).width == 16


def test_abi_layout_of_the_launch_arguments(tmp_path):
    import ctypes as C
    import subprocess
    from ccfd_demo_summit_amd.ops._lib import ForestExplainArgs
    from ccfd_demo_summit_amd.ops.build import CSRC
    fields = [name for name, _ in ForestExplainArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccfd_abi.h"\nint main(){printf("%zu %d %d",'
                   'sizeof(ccfd_forest_explain_args),CCFD_FRX_RULE_BYTES,CCFD_FRX_MAX_SLICES);'
                   + "".join(f'printf(" %zu",offsetof(ccfd_forest_explain_args,{f}));' for f in fields) + "}\n")
    exe = tmp_path / "sz"
    r = subprocess.run(["gcc", str(src), "-I", str(CSRC / "include"), "-o", str(exe)], capture_output=True)
    if r.returncode != 0:
        pytest.skip("no C compiler")
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    from ccfd_demo_summit_amd.models import explain_forest as ef
    assert out[:3] == [C.sizeof(ForestExplainArgs), ef.RULE_BYTES, ef.MAX_SLICES] and out[0] == 72
    assert out[3:] == [getattr(ForestExplainArgs, f).offset for f in fields]


# ------------------------------------------------------------------------------- serving
def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def _sk_forest():
    from sklearn.ensemble import RandomForestClassifier
    from ccfd_demo_summit_amd.models.sklearn_import import from_sklearn
    rng = np.random.default_rng(6)
    X = rng.standard_normal((300, 30)).astype(np.float32)
    y = (X[:, 3] + 0.5 * X[:, 7] > 0.8).astype(int)
    return from_sklearn(RandomForestClassifier(n_estimators=4, max_depth=4, random_state=0).fit(X, y)), X


def test_explain_route_for_an_imported_forest():
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.serving import CpuScorer
    from ccfd_demo_summit_amd.serving.scorers import _explainable
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    m, Xtr = _sk_forest()
    X = Xtr[:5]
    want, bv = shapley_forest(m, X)
    np.testing.assert_allclose(bv + want.sum(1), forest_raw_f64(m, X), rtol=0, atol=1e-13)
    bare = TreeEnsemble(m.feat, m.value, m.child, m.leaf, m.root, m.base, m.link)

    async def go():
        async with TestClient(TestServer(SeldonServer(CpuScorer(m)).app)) as cl:
            r = await cl.post("/explain", json=seldon.build_request(X))
            assert r.status == 200
            body = await r.json()
            assert body["data"]["names"] == list(FEATURE_NAMES)
            np.testing.assert_allclose(np.asarray(body["data"]["ndarray"]), want, rtol=0, atol=1e-12)
            assert body["meta"]["tags"]["base_value"] == pytest.approx(bv)
        async with TestClient(TestServer(SeldonServer(CpuScorer(bare)).app)) as cl:
            r = await cl.post("/explain", json=seldon.build_request(X))
            assert r.status == 400 and "fit_cover" in (await r.json())["status"]["info"]
    _run(go())
    with pytest.raises(ValueError, match="fit_cover"):
        _explainable(bare)
    with pytest.raises(ValueError, match="no explanation"):
        _explainable(build_model("mlp", seed=0, X_ref=X))
    with pytest.raises(ValueError, match="no explanation"):
        _explainable(build_model("lr", seed=0, X_ref=X))


def test_api_doc_forest_block_runs():
    import re
    from pathlib import Path
    doc = (Path(__file__).resolve().parents[1] / "docs" / "API.md").read_text()
    blocks = [b for b in re.findall(r"```py\n(.*?)```", doc, re.S) if "shapley_forest" in b]
    assert len(blocks) == 1
    ns = {}
    exec(blocks[0], ns)
    assert ns["phi"].shape == (4, 30) and ns["forest"].cover is not None and isinstance(ns["why"], list)


def test_router_reasons_for_a_forest():
    from ccfd_demo_summit_amd.process import ProcessEngine
    from ccfd_demo_summit_amd.router.router import Router
    from ccfd_demo_summit_amd.router.rules import RuleSet
    from ccfd_demo_summit_amd.serving import CpuScorer
    m, Xtr = _sk_forest()
    X = Xtr[:40]
    proba = m.predict_proba(X)
    thr = float(np.sort(proba)[-4])
    phi, _ = shapley_forest(m, X)
    eng = ProcessEngine(notification_timeout_s=60)
    out = Router(RuleSet.threshold(thr), eng, explainer=CpuScorer(m), reasons=2).on_scored(
        np.arange(40) + 1000, np.arange(40), proba, X=X)
    fraud = np.nonzero(proba >= thr)[0]
    assert out["fraud"] == fraud.size >= 4
    for i in fraud:
        why = eng.get(eng._by_tx[1000 + int(i)]).variables["reasons"]
        assert why == top_reasons(phi[i], FEATURE_NAMES, 2)
    assert any(eng.get(eng._by_tx[1000 + int(i)]).variables["reasons"] for i in fraud)
