"""General tree ensembles on binned rows, on the host: ``TreeEnsemble.bin_spec``, the 'FRB1' blob
of ``pack(bins=)`` and the numpy oracle of the device walk, ``leaf_node_binned`` -- every
(row, tree) leaf of the binned walk is the leaf of the f32 walk, for 8-bit (G32) and 5-bit (G20)
bins, on rows built around every threshold."""
import numpy as np
import pytest

from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import TreeEnsemble, build_model
from ccfd_demo_summit_amd.models.gbdt import BinSpec
from ccfd_demo_summit_amd.models.sklearn_import import from_sklearn


@pytest.fixture(scope="module")
def data():
    return generate(4000, seed=11)


@pytest.fixture(scope="module")
def ensembles(data):
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier
    X, y = data
    g = build_model("gbdt", seed=3, X_ref=X, calibrate_rate=0.05)
    return {
        "t1_d1": TreeEnsemble.random_init(1, 1, 0.0, 1, X),
        "t7_d5": TreeEnsemble.random_init(7, 5, 0.2, 2, X),
        "t64_d12": TreeEnsemble.random_init(64, 12, 0.3, 3, X),
        "rf": from_sklearn(RandomForestClassifier(n_estimators=5, random_state=0).fit(X, y)),
        "gb": from_sklearn(GradientBoostingClassifier(n_estimators=10, max_depth=3, random_state=3).fit(X, y)),
        "oblivious": TreeEnsemble.from_oblivious(g),
        "oblivious_padded": TreeEnsemble.from_oblivious(g.padded(n_trees=g.n_trees + 2, depth=g.depth + 1)),
    }


def adversarial_rows(m: TreeEnsemble, X: np.ndarray) -> np.ndarray:
    """Synthetic rows, then for every inner node three rows that hold its threshold itself, the
    float just below and the float just above it in the node's feature, and rows of NaN, +inf
    and -inf."""
    rng = np.random.default_rng(5)
    inner = np.flatnonzero(~m.leaf)
    thr, feat = m.value[inner], m.feat[inner]
    keep = ~np.isnan(thr)
    thr, feat = thr[keep], feat[keep]
    edge = X[rng.integers(0, X.shape[0], 3 * thr.size)].copy()
    for j, v in enumerate((thr, np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf)))):
        edge[np.arange(thr.size) * 3 + j, feat] = v
    special = X[:6].copy()
    special[0, :] = np.nan
    special[1, :] = np.inf
    special[2, :] = -np.inf
    special[3, ::2] = np.nan
    special[4, 1::2] = np.inf
    special[5, ::3] = -np.inf
    return np.concatenate([X[:300], edge, special]).astype(np.float32)


def superset(spec: BinSpec, bits: int) -> BinSpec:
    """``spec`` with extra edges: two between / around the model's edges of every feature (one
    for 5-bit bins at most up to the 31-edge cap)."""
    out = []
    cap = 255 if bits == 8 else 31
    for e in spec.edges:
        extra = np.float32([-1e30, 1e30]) if e.size == 0 else \
            np.concatenate([np.float32([e[0] - 1.0, e[-1] + 1.0]), (e[:-1] + np.diff(e) / 2).astype(np.float32)])
        u = np.unique(np.concatenate([e, extra]))
        if u.size > cap:                       # drop added edges only, from the top
            added = np.setdiff1d(u, e)
            u = np.unique(np.concatenate([e, added[:cap - e.size]]))
        out.append(u)
    return BinSpec(out, bits=bits)


@pytest.mark.parametrize("bits", [8, 5])
@pytest.mark.parametrize("name", ["t1_d1", "t7_d5", "t64_d12", "rf", "gb", "oblivious", "oblivious_padded"])
def test_binned_walk_selects_the_f32_leaves(data, ensembles, name, bits):
    m = ensembles[name]
    X = adversarial_rows(m, data[0])
    want = m.leaf_node(X)
    spec = m.bin_spec(bits)
    assert spec.bits == bits and spec.row_format == ("g32" if bits == 8 else "g20")
    rows = spec.encode(X)
    assert rows.shape == (X.shape[0], 32 if bits == 8 else 20)
    np.testing.assert_array_equal(m.leaf_node_binned(rows, spec), want)
    if bits == 8:                              # the default table is the ensemble's own 8-bit one
        np.testing.assert_array_equal(m.leaf_node_binned(rows), want)
    big = superset(spec, bits)
    assert big.contains(spec) and big.stamp != spec.stamp
    assert sum(e.size for e in big.edges) > sum(e.size for e in spec.edges)
    np.testing.assert_array_equal(m.leaf_node_binned(big.encode(X), big), want)


def test_bin_spec_is_the_reachable_non_nan_thresholds():
    nan = np.float32(np.nan)
    #      0: f5 > 0.25 | 1: leaf | 2: f7 > NaN | 3: leaf | 4: leaf | 5: unreachable inner | 6, 7: its leaves
    m = TreeEnsemble([5, 0, 7, 0, 0, 9, 0, 0], [0.25, 1.5, nan, 2.5, 3.5, 8.0, 0.0, 0.0], [1, 0, 3, 0, 0, 6, 0, 0],
                     [0, 1, 0, 1, 1, 0, 1, 1], [0], 0.75, "identity")
    spec = m.bin_spec()
    assert [e.tolist() for e in spec.edges] == [[0.25] if j == 5 else [] for j in range(30)]
    blob = m.pack(bins=spec)
    node = np.frombuffer(blob, np.uint32, 16, 80).reshape(8, 2)
    np.testing.assert_array_equal(node[[0, 2, 5], 1], [0, 255, 255])     # k; NaN and unreachable never fire
    X = np.zeros((3, 30), np.float32)
    X[:, 5] = [0.25, np.nextafter(np.float32(0.25), np.float32(1)), nan]
    X[:, 7] = [1.0, 1.0, nan]
    np.testing.assert_array_equal(m.leaf_node_binned(spec.encode(X))[:, 0], [1, 3, 1])
    np.testing.assert_array_equal(m.leaf_node(X)[:, 0], [1, 3, 1])


@pytest.mark.parametrize("bits", [8, 5])
def test_frb1_blob_round_trip(data, ensembles, bits):
    for name in ("t7_d5", "rf", "gb", "oblivious_padded"):
        m = ensembles[name]
        spec = m.bin_spec(bits)
        f32, blob = m.pack(), m.pack(bins=spec)
        assert blob[:4] == b"FRB1" and len(blob) == len(f32)
        hdr, ref = np.frombuffer(blob, np.int32, 16), np.frombuffer(f32, np.int32, 16)
        np.testing.assert_array_equal(hdr[1:6], ref[1:6])               # flags, T, depth, base bits, n_nodes
        assert hdr[6] == spec.stamp and ref[6] == 0 and not hdr[7:].any()
        off = 64 + ((8 * m.n_trees + 15) & ~15)
        assert blob[64:off] == f32[64:off]                              # the tree section
        node = np.frombuffer(blob, np.uint32, 2 * m.n_nodes, off).reshape(-1, 2)
        want = np.frombuffer(f32, np.uint32, 2 * m.n_nodes, off).reshape(-1, 2)
        np.testing.assert_array_equal(node[:, 0], want[:, 0])           # the same w
        np.testing.assert_array_equal(node[m.leaf, 1], m.value[m.leaf].view(np.uint32))   # leaf values, bit for bit
        inner = np.flatnonzero(~m.leaf)
        k = node[inner, 1].astype(np.int64)
        nanthr = np.isnan(m.value[inner])
        assert (k[nanthr] == 255).all() and (name != "oblivious_padded" or nanthr.any())
        for i, ki in zip(inner[~nanthr], k[~nanthr]):
            assert spec.edges[m.feat[i]][ki] == m.value[i]
        # packed against a superset table: the same nodes, other indices, that table's stamp
        big = superset(spec, bits)
        blob2 = m.pack(bins=big)
        assert np.frombuffer(blob2, np.int32, 16)[6] == big.stamp
        k2 = np.frombuffer(blob2, np.uint32, 2 * m.n_nodes, off).reshape(-1, 2)[inner, 1]
        for i, ki in zip(inner[~nanthr], k2[~nanthr]):
            assert big.edges[m.feat[i]][ki] == m.value[i]
    with pytest.raises(ValueError, match="FRS1"):
        TreeEnsemble.unpack(blob)


def test_pack_refuses_a_threshold_outside_the_spec(data, ensembles):
    a, b = ensembles["t7_d5"], ensembles["rf"]
    with pytest.raises(ValueError, match="not a bin edge"):
        b.pack(bins=a.bin_spec())
    with pytest.raises(ValueError, match="not a bin edge"):
        b.leaf_node_binned(a.bin_spec().encode(data[0][:4]), a.bin_spec())
    with pytest.raises(ValueError, match="f32 rows"):
        a.pack(wire=True)


def test_too_many_thresholds_for_a_byte_or_five_bits(data):
    # N(0,1) thresholds: every split has its own; 40 depth-9 trees put far more than 255 on a feature
    wide = TreeEnsemble.random_init(40, 9, 0.0, 1)
    per_feat = [np.unique(wide.value[~wide.leaf & (wide.feat == j)]).size for j in range(30)]
    assert max(per_feat) > 255
    with pytest.raises(ValueError, match="split thresholds > 255"):
        wide.bin_spec()
    # between 32 and 255 on every feature: G32 rows, not G20
    mid = TreeEnsemble.random_init(8, 8, 0.0, 2)
    per_feat = [np.unique(mid.value[~mid.leaf & (mid.feat == j)]).size for j in range(30)]
    assert 31 < max(per_feat) <= 255
    spec = mid.bin_spec()
    assert not spec.fits_g20
    with pytest.raises(ValueError, match="split thresholds > 31"):
        mid.bin_spec(bits=5)
    X = adversarial_rows(mid, data[0])
    np.testing.assert_array_equal(mid.leaf_node_binned(spec.encode(X)), mid.leaf_node(X))
