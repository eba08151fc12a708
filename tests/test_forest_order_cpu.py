"""The float32 model of the general-tree kernels' summation order (tests/helpers/forest_cases.py
kernel_order_z), checked without a GPU: its group plan reaches every group size of both
layouts, and on the rows tests/test_forest_order_gpu.py scores the order is visible in the bits
-- a kernel that added the same leaves in another order would fail there."""
import numpy as np
import pytest

from ccfd_demo_summit_amd.data import generate
from tests.helpers import forest_cases as fc


@pytest.fixture(scope="module")
def rows():
    return generate(4000, seed=11)[0][:321]


@pytest.fixture(scope="module")
def ensembles(rows):
    return fc.order_ensembles(generate(4000, seed=11)[0])


def _sizes(plans):
    return [[len(g) for g in groups] for groups in plans]


def test_group_plan_covers_every_tree_once():
    for T in fc.ORDER_T + (8, 16, 64, 100):
        for layout in ("f32", "bins"):
            for resident in (True, False):
                plans = fc.group_plan(T, layout, resident)
                assert len(plans) == (4 if layout == "f32" else 1)
                flat = [t for groups in plans for g in groups for t in g]
                assert sorted(flat) == list(range(T))
                for w, groups in enumerate(plans):
                    trees = [t for g in groups for t in g]
                    assert trees == (list(range(w, T, 4)) if layout == "f32" else list(range(T)))
                    if not resident:
                        assert all(len(g) == 1 for g in groups)


def test_group_plan_reaches_every_group_size():
    f32 = {T: _sizes(fc.group_plan(T, "f32", True)) for T in fc.ORDER_T}
    bins = {T: _sizes(fc.group_plan(T, "bins", True)) for T in fc.ORDER_T}
    assert f32[3] == [[1], [1], [1], []]                        # a wave with no tree
    assert f32[60] == [[8, 4, 2, 1]] * 4
    assert f32[37] == [[8, 2], [8, 1], [8, 1], [8, 1]]
    assert f32[21] == [[4, 2], [4, 1], [4, 1], [4, 1]]
    assert {s for T in fc.ORDER_T for w in f32[T] for s in w} == {8, 4, 2, 1}
    assert bins[31] == [[16, 8, 4, 2, 1]]
    assert bins[37] == [[16, 16, 4, 1]]
    assert bins[60] == [[16, 16, 16, 8, 4]]
    assert {s for T in fc.ORDER_T for s in bins[T][0]} == {16, 8, 4, 2, 1}


def test_the_order_shows_in_the_bits(rows, ensembles):
    """Not vacuous: on these rows the two layouts give different float32 bits from each other,
    and from the plain tree-order sum, for at least one row of every ensemble with T >= 3.  (At
    T = 3 the f32 layout IS the plain sum -- one tree a wave, added after base in wave order --
    so there the binned layout alone differs from it.)"""
    for name, (m, resident) in ensembles.items():
        v = m.leaf_values(rows)
        zf = fc.kernel_order_z(m, v, "f32", resident)
        zb = fc.kernel_order_z(m, v, "bins", resident)
        zp = fc.plain_z(m, v)
        assert zf.dtype == zb.dtype == np.float32
        lo, hi = min(zf.min(), zb.min()), max(zf.max(), zb.max())
        assert 0.0 < lo and hi < 1.0                           # the identity link's clamp is exact
        exact = m.base + v.astype(np.float64).sum(1)
        assert np.abs(zf - exact).max() < 1e-5 and np.abs(zb - exact).max() < 1e-5
        d_fb, d_fp, d_bp = (int((a.view(np.uint32) != b.view(np.uint32)).sum()) for a, b in
                            ((zf, zb), (zf, zp), (zb, zp)))
        print(f"{name}: T={m.n_trees} rows differing f32/bins {d_fb}, f32/plain {d_fp}, bins/plain {d_bp}")
        if m.n_trees == 1:
            assert d_fb == d_fp == d_bp == 0
            continue
        assert d_fb > 0
        assert d_bp > 0
        if m.n_trees == 3:
            assert d_fp == 0
        else:
            assert d_fp > 0
