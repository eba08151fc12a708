"""The fixtures of tests/helpers/gbdt_edges.py, checked on the numpy reference alone -- the gate
that keeps test_gbdt_edges_gpu.py from passing vacuously: on every fixture the GPU file uses,
a single wrong leaf moves the probability by at least 10 x the comparison tolerance, |z| <= 4,
at least 99 % of the rows are clear of the routing threshold, every split has a row on its
threshold and one on each side, and the binned rows choose the f32 rows' leaves."""
import numpy as np
import pytest

from ccfd_demo_summit_amd.contracts.metric_names import AMOUNT_BUCKETS
from ccfd_demo_summit_amd.contracts.transaction import AMOUNT_COL, amount_bucket, decode_g20_bins
from tests.helpers import gbdt_edges as ge


def _all_cases():
    for d in ge.DEPTHS:
        yield f"probe-d{d}", ge.probe_case(d)
        for t in ge.TREES:
            yield f"shape-{t}x{d}", ge.shape_case(t, d)
    yield "shape-2x1", ge.shape_case(2, 1)              # the shadow kernels' 4-float champion table
    yield "chunked-131x7", ge.chunked_case()


def _sweeps():
    for bits in (8, 5):
        for which in (0, 1):
            yield bits, which, ge.sweep_case(bits, which)


def test_tolerance_and_margin_are_the_documented_ones():
    assert ge.TOL == 1e-5 and ge.MARGIN >= 10 * ge.TOL and ge.ZMAX == 4.0 and ge.CLEAR_FRACTION == 0.99


def test_single_leaf_swaps_are_visible_and_z_is_bounded():
    for name, (m, X, ref) in _all_cases():
        z = ge.raw_reference(m, X)
        assert np.abs(z).max() <= ge.ZMAX, name
        assert ge.min_leaf_swap_delta(m, X) >= ge.MARGIN, name
        assert ge.clear_rows(ref, 0.5).mean() >= ge.CLEAR_FRACTION, name
        assert np.abs(ref - m.predict_proba(X)).max() < 2e-7, name      # the model's own f32 oracle agrees
    for bits, which, (spec, m, X, bins, ref) in _sweeps():
        assert np.abs(ge.raw_reference(m, X)).max() <= ge.ZMAX
        assert ge.min_leaf_swap_delta(m, X) >= ge.MARGIN
        assert ge.clear_rows(ref, 0.5).mean() >= ge.CLEAR_FRACTION
    for trees, depth in ge.SHADOW_SHAPES:
        for bits in (8, 5):
            A, B, spec, X, refA, refB = ge.shadow_case(trees, depth, bits)
            assert (A.n_trees, A.depth, B.n_trees, B.depth) == (trees, depth, trees, depth)
            assert not np.array_equal(A.thr, B.thr)
            for m, ref in ((A, refA), (B, refB)):
                assert np.abs(ge.raw_reference(m, X)).max() <= ge.ZMAX
                assert ge.min_leaf_swap_delta(m, X) >= ge.MARGIN
                assert ge.clear_rows(ref, 0.5).mean() >= ge.CLEAR_FRACTION
                np.testing.assert_array_equal(m.leaf_index_g32(spec.encode(X), spec), m.leaf_index(X))
            # the pair disagrees on some rows and agrees on others: every shadow counter is non-trivial
            fa, fb = refA >= 0.5, refB >= 0.5
            assert (fa & fb).any() and (fa != fb).any() and not fb.all()


def test_one_row_launches_are_clear_and_summation_orders_differ():
    for name, (m, X, ref) in _all_cases():
        assert ge.clear_rows(ref, 0.5)[ge.take(len(X), 1)].all(), name      # the n = 1 launch's row
        for n in ge.ROW_COUNTS:
            assert ge.clear_rows(ref, 0.5)[ge.take(len(X), n)].any(), name
    # v1 and v2 add the trees in different orders: on float32 arithmetic alone the 8-tree ensembles'
    # raw scores differ in the last bits on many rows, by far less than the tolerance, and so do
    # the probabilities rounded to float32
    for d in ge.ORDER_DEPTHS:
        m, X, _ = ge.shape_case(ge.ORDER_TREES, d)
        z1, z2 = ge.f32_sum_orders(m, X)
        p1, p2 = ((1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32) for z in (z1, z2))
        assert (z1 != z2).sum() >= 40 and (p1 != p2).sum() >= 20 and np.abs(z1 - z2).max() < 4e-6, d


def test_probe_tree_probability_identifies_the_leaf():
    for d in ge.DEPTHS:
        m = ge.probe_tree(d)
        assert m.n_trees == 1 and m.depth == d and m.base == 0.0
        lv = np.sort(m.leaves[0].astype(np.float64))
        np.testing.assert_allclose(lv, np.linspace(-4, 4, 1 << d), atol=1e-6)
        p = 1.0 / (1.0 + np.exp(-lv))
        assert np.diff(p).min() > (5.5e-4 if d == 8 else 1e-3)


def test_every_split_has_a_row_on_and_on_each_side_of_its_threshold():
    for name, (m, X, _) in _all_cases():
        zero = 0
        for t in range(m.n_trees):
            for d in range(m.depth):
                col = X[:, m.feat[t, d]]
                th = m.thr[t, d]
                assert (col == th).any(), name
                assert (col == np.nextafter(th, np.float32(-np.inf))).any(), name
                assert (col == np.nextafter(th, np.float32(np.inf))).any(), name
                if th == 0:
                    zero += 1
                    tiny = np.nextafter(np.float32(0), np.float32(1))
                    bits = col.view(np.uint32)
                    assert (bits == 0x80000000).any() and (bits == 0).any(), name          # -0.0 and +0.0
                    assert (col == tiny).any() and (col == -tiny).any(), name
        assert zero >= 1, name
        f = int(m.feat[0, 0])
        assert np.isnan(X[:, f]).any() and (X[:, f] == np.inf).any() and (X[:, f] == -np.inf).any(), name
        # the leaf on the threshold is the "not greater" one, the leaf one ulp above is the other
        idx = m.leaf_index(X)
        assert len(np.unique(idx[:, 0])) >= 2, name


def test_edge_rows_cover_every_amount_bound():
    _, X, _ = ge.shape_case(3, 2)
    amt = X[:, AMOUNT_COL]
    for b in AMOUNT_BUCKETS:
        b = np.float32(b)
        for v in (b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))):
            assert (amt == v).any()
    assert (amt == 0).any() and (amt < 0).any() and np.isnan(amt).any()
    assert (amt == np.inf).any() and (amt == -np.inf).any()
    assert set(np.unique(amount_bucket(amt)).tolist()) == set(range(14))
    assert (amount_bucket(amt[np.isnan(amt)]) == 0).all()
    # counters_problem accepts the reference's own counts and names a shifted histogram
    m, X, ref = ge.shape_case(3, 2)
    p = ref.astype(np.float32)
    r = (ref >= 0.5).astype(np.uint8)
    cnt = np.zeros(64, np.int64)
    cnt[0], cnt[1], cnt[2] = len(p), r.sum(), len(p) - r.sum()
    cnt[3] = int(np.round(ref * 1e6).sum())
    b = amount_bucket(amt).astype(np.int64)
    cnt[8:22] = np.bincount(b[r == 0], minlength=14)
    cnt[24:38] = np.bincount(b[r == 1], minlength=14)
    assert ge.counters_problem(cnt, p, r, X) is None
    cnt[8], cnt[21] = cnt[8] - 1, cnt[21] + 1
    assert "standard histogram" in ge.counters_problem(cnt, p, r, X)


@pytest.mark.parametrize("bits", [8, 5])
def test_binned_edge_rows_choose_the_f32_leaves(bits):
    for name, (m, X, _) in _all_cases():
        if name.startswith("chunked"):
            continue
        spec = m.bin_spec(bits)
        np.testing.assert_array_equal(m.leaf_index_g32(spec.encode(X), spec), m.leaf_index(X), err_msg=name)


def test_feature_sweep_rows_encode_to_their_bins_and_every_field_decides_a_leaf():
    for bits, which, (spec, m, X, bins, ref) in _sweeps():
        cap = 255 if bits == 8 else 31
        assert all(e.size == cap for e in spec.edges)
        enc = spec.encode(X)
        got = (decode_g20_bins(enc) if bits == 5 else enc)[:, :30]
        np.testing.assert_array_equal(got, bins)
        np.testing.assert_array_equal(m.leaf_index_g32(enc, spec), m.leaf_index(X))
        assert (bins == 0).all(1).any() and (bins == cap).all(1).any()
        idx = m.leaf_index(X)
        ks = ge.SWEEP_KS[bits][which]
        for f in range(30):
            assert (m.feat[f] == f).all()
            assert set(np.unique(idx[:, f]).tolist()) == {0, 1, 2, 3} - ({2} if ks[0] < ks[1] else {1})
            for k in ks:                                   # bins k and k + 1 under all-0 and all-high neighbours
                for nb in (0, cap):
                    others = np.delete(bins, f, 1)
                    for b in (k, k + 1):
                        assert ((bins[:, f] == b) & (others == nb).all(1)).any()


def test_take_slices_and_tiles():
    for n in ge.ROW_COUNTS:
        i = ge.take(300, n)
        assert len(i) == n and i.max() < 300
        if n >= 300:
            assert len(np.unique(i)) == 300
    assert ge.take(300, 1)[0] == ge.N_BASE
