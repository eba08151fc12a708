"""Shadow (challenger) scoring of oblivious GBDTs on G32 / G20 rows: the launch kernel per row,
the launch-mode and persistent engines by role swap (B as A's shadow must count what B counts
as champion, to the bit), leaf tables in LDS and in global memory, stale rows, the runtime
toggle, promotion, the refusals, and a challenger trained against the live bin table."""
import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate
from tests.helpers.gbdt_pairs import make_pair

pytestmark = pytest.mark.gpu

BATCH = 8192
N_ENGINE = 2 * BATCH + 2 * 1300            # pump(2) + pump(2, batch_rows=1300): partial items
ID_BASE = 1000
FORMATS = ("g32", "g20")


@pytest.fixture(scope="module")
def X():
    return generate(70001, seed=11)[0]


def _pair(gpu, X, rows, **kw):
    """One champion / challenger pair on the device: models, blobs, the shared bin table, the
    first ``rows`` rows encoded on the device and the f32 oracles."""
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    A, B, spec = make_pair(X[:kw.pop("n_ref", 20000)], **kw)
    return {"A": A, "B": B, "spec": spec, "dmA": DeviceModel(A, gpu, bins=spec), "dmB": DeviceModel(B, gpu, bins=spec),
            "rows": torch.from_numpy(spec.encode(X[:rows])).to(gpu),
            "refA": A.predict_proba(X[:rows]), "refB": B.predict_proba(X[:rows])}


@pytest.fixture(scope="module")
def fx(gpu, X):
    """100 x 6 on G32 rows, 30 x 5 on G20 rows: computed once, never modified."""
    return {"g32": _pair(gpu, X, 70001), "g20": _pair(gpu, X, 70001, trees=30, depth=5, seeds=(5, 6), bits=5)}


def _totals(eng, gpu):
    """Sum of the two epoch buffers once everything submitted has completed."""
    side = torch.cuda.Stream(gpu)
    eng.flip_epoch(side)
    side.synchronize()
    return (eng.counters[0] + eng.counters[1]).cpu().numpy()


def _ids(flagged):
    return set((flagged["tx_id"].astype(np.int64) - ID_BASE).tolist())


def _make_log(X, spec):
    from ccfd_demo_summit_amd.engine import PartitionLog
    return PartitionLog.from_arrays(X[:N_ENGINE], ids=np.arange(N_ENGINE, dtype=np.uint64) + ID_BASE, bins=spec)


def _run_engine(gpu, log, champion, shadow, exec_mode):
    """pump(2) + pump(2, batch_rows=1300) over ``log``.  Returns (counter totals, flagged rows)."""
    from ccfd_demo_summit_amd.engine import StreamEngine
    eng = StreamEngine(champion, batch=BATCH, depth=4, streams=1, exec_mode=exec_mode, shadow=shadow)
    try:
        eng.add_log(0, log)
        a = eng.pump(2)
        b = eng.pump(2, batch_rows=1300)
        assert a.rows + b.rows == N_ENGINE
        ids = _ids(eng.drain_flagged())
        return _totals(eng, gpu), ids
    finally:
        eng.close()


@pytest.fixture(scope="module")
def logs(X, fx):
    out = {f: _make_log(X, fx[f]["spec"]) for f in FORMATS}
    yield out
    for log in out.values():
        log.free()


def _check_role_swap(gpu, log, p, exec_mode):
    c1, ids1 = _run_engine(gpu, log, p["dmA"], p["dmB"], exec_mode)
    c2, ids2 = _run_engine(gpu, log, p["dmB"], p["dmA"], exec_mode)
    c3, ids3 = _run_engine(gpu, log, p["dmA"], None, exec_mode)
    n = N_ENGINE
    assert c1[40] == c1[0] == n and c2[40] == c2[0] == n
    # B as A's shadow counts exactly what B counts as champion, and the other way round
    assert (c1[41], c1[43]) == (c2[1], c2[3])
    assert (c2[41], c2[43]) == (c1[1], c1[3])
    assert c1[42] == c2[42] and c1[44] == c2[44]
    assert c1[42] == len(ids1 & ids2)
    assert c1[1] == len(ids1) and c2[1] == len(ids2)
    assert 0 < c1[42] < min(c1[1], c2[1]) and c1[44] > 0            # every counter is non-trivial
    # the champion's own results do not change when a shadow rides along
    np.testing.assert_array_equal(c1[:38], c3[:38])
    assert ids1 == ids3
    assert not c3[38:].any() and not c1[38:40].any() and not c1[45:].any() and c1[4] == 0
    return ids1, ids2


# A launch takes one wave per 64-row chunk, 4 waves a workgroup, capped at 256 workgroups per
# CCFD_G32_WGS_PER_CU.  n = 70001 with one workgroup per CU is 1094 chunks on 1024 waves: 70
# waves take a second chunk through the prefetch, and the last chunk has 49 rows.
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097, 70001])
def test_launch_kernel_per_row(gpu, fx, monkeypatch, fmt, n):
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    if n == 70001:
        monkeypatch.setenv("CCFD_G32_WGS_PER_CU", "1")
    p = fx[fmt]
    x = p["rows"][:n]
    c0, c1 = new_counters(gpu), new_counters(gpu)
    pA, rA = score(p["dmA"], x, 0.5, counters=c0)
    pB, _ = score(p["dmB"], x, 0.5)
    out = score(p["dmA"], x, 0.5, counters=c1, shadow=p["dmB"])
    assert len(out) == 3
    torch.cuda.synchronize(gpu)
    pr, r, ps = (t.cpu().numpy() for t in out)
    np.testing.assert_array_equal(pr.view(np.uint32), pA.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(ps.view(np.uint32), pB.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(r, rA.cpu().numpy())
    da, db = np.abs(pr - p["refA"][:n]).max(), np.abs(ps - p["refB"][:n]).max()
    print(f"{fmt} n={n}: |p - A.predict_proba| max {da:.3g}, |ps - B.predict_proba| max {db:.3g}")
    assert da < 2e-5 and db < 2e-5
    c0, c1 = c0.cpu().numpy(), c1.cpu().numpy()
    np.testing.assert_array_equal(c1[:38], c0[:38])
    assert not c0[38:].any()
    fa, fb = pr >= 0.5, ps >= 0.5
    assert c1[40] == n
    assert c1[41] == fb.sum()
    assert c1[42] == (fa & fb).sum()
    p64, ps64 = pr.astype(np.float64), ps.astype(np.float64)
    assert abs(int(c1[43]) - np.round(ps64 * 1e6).sum()) <= n
    assert abs(int(c1[44]) - np.round(np.abs(p64 - ps64) * 1e6).sum()) <= n
    assert not c1[45:].any() and not c1[38:40].any()
    if n >= 4097:
        assert 0 < c1[42] < min(c1[1], c1[41])


@pytest.mark.parametrize("fmt", FORMATS)
def test_launch_kernel_identity(gpu, fx, fmt):
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    n = 4097
    p = fx[fmt]
    c = new_counters(gpu)
    sp = torch.full((n + 3,), -1.0, device=gpu)
    pr, r, ps = score(p["dmA"], p["rows"][:n], 0.5, counters=c, shadow=p["dmA"], shadow_proba=sp)
    torch.cuda.synchronize(gpu)
    assert ps.data_ptr() == sp.data_ptr()
    np.testing.assert_array_equal(ps[:n].cpu().numpy().view(np.uint32), pr.cpu().numpy().view(np.uint32))
    assert (sp[n:] == -1.0).all()                        # nothing written past row n
    c = c.cpu().numpy()
    assert c[1] > 0
    assert c[41] == c[42] == c[1] and c[43] == c[3] and c[44] == 0 and c[40] == n


@pytest.mark.parametrize("fmt", FORMATS)
def test_launch_engine_role_swap(gpu, fx, logs, fmt):
    _check_role_swap(gpu, logs[fmt], fx[fmt], "launch")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("item_rows", [256, 512, 1024])
def test_persistent_engine_role_swap(gpu, fx, logs, monkeypatch, fmt, item_rows):
    monkeypatch.setenv("CCFD_PERSIST_ITEM_ROWS", str(item_rows))
    _check_role_swap(gpu, logs[fmt], fx[fmt], "persistent")


# 150 x 6: two tables of 9600 floats exceed the 16384 the kernels stage, so in the persistent
# kernel the champion's leaves stay in LDS and the shadow's are gathered from global memory (a
# launch reads both from global memory: its champion rule stages up to 8192 floats).  700 x 6:
# both tables in global memory in either kernel.
@pytest.mark.parametrize("exec_mode", ["launch", "persistent"])
@pytest.mark.parametrize("trees", [150, 700])
def test_leaf_placement(gpu, X, exec_mode, trees):
    p = _pair(gpu, X, 64, trees=trees, n_ref=4000)
    log = _make_log(X, p["spec"])
    try:
        ids1, ids2 = _check_role_swap(gpu, log, p, exec_mode)
    finally:
        log.free()
    # routes against the f32 oracle (same leaves; the sums differ in order only)
    for ids, m in ((ids1, p["A"]), (ids2, p["B"])):
        ref = m.predict_proba(X[:N_ENGINE])
        got = np.zeros(N_ENGINE, bool)
        got[sorted(ids)] = True
        sure = np.abs(ref - 0.5) > 2e-5
        np.testing.assert_array_equal(got[sure], (ref >= 0.5)[sure])


@pytest.mark.parametrize("exec_mode", ["launch", "persistent"])
def test_stale_rows_are_not_counted(gpu, X, fx, exec_mode):
    """A log whose rows carry another table's stamp: the champion counts them as stale, the
    shadow counts nothing."""
    from ccfd_demo_summit_amd.engine import StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    p = fx["g32"]
    other = p["A"].bin_spec()
    assert other.stamp != p["spec"].stamp
    log = _make_log(X, p["spec"])
    log.feats.array.view(np.uint8).reshape(N_ENGINE, 32)[:] = other.encode(X[:N_ENGINE])
    eng = StreamEngine(p["dmA"], batch=BATCH, depth=4, streams=1, exec_mode=exec_mode, shadow=p["dmB"])
    try:
        eng.add_log(0, log)
        st = eng.pump(2)
        c = _totals(eng, gpu)
        assert st.rows == 2 * BATCH and c[0] == 2 * BATCH and c[4] == 2 * BATCH and c[1] == 0
        assert not c[40:45].any()
    finally:
        eng.close()
        log.free()
    if exec_mode == "launch":                             # per row: NaN for both models
        cnt = new_counters(gpu)
        x = torch.from_numpy(other.encode(X[:257])).to(gpu)
        pr, r, ps = score(p["dmA"], x, 0.5, counters=cnt, shadow=p["dmB"])
        torch.cuda.synchronize(gpu)
        assert torch.isnan(pr).all() and torch.isnan(ps).all() and not r.any()
        cnt = cnt.cpu().numpy()
        assert cnt[4] == 257 and not cnt[40:45].any()


def test_runtime_toggle_and_promote(gpu, fx, logs):
    from ccfd_demo_summit_amd.engine import StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import score
    p = fx["g32"]
    eng = StreamEngine(p["dmA"], batch=4096, depth=4, streams=1, exec_mode="persistent")
    try:
        eng.add_log(0, logs["g32"])
        eng.pump(1)
        assert _totals(eng, gpu)[40] == 0
        eng.set_shadow(p["dmB"])
        assert eng.shadow is p["dmB"]
        eng.pump(1)
        mid = _totals(eng, gpu)
        assert mid[40] == 4096 and mid[0] == 2 * 4096 and mid[41] > 0
        eng.set_shadow(None)
        eng.pump(1)
        end = _totals(eng, gpu)
        assert end[40] == 4096 and end[0] == 3 * 4096
        np.testing.assert_array_equal(end[41:45], mid[41:45])
        _, rA = score(p["dmA"], p["rows"][:3 * 4096], 0.5)
        torch.cuda.synchronize(gpu)
        assert end[1] == int(rA.sum().item()) > 0
        s = eng.shadow_counters(end)
        assert s["rows"] == 4096 and 0.0 < s["mean_proba"] < 1.0 and s["mean_abs_diff"] > 0.0
        # promotion: B's routes become the engine's, shadow scoring stops
        eng.set_shadow(p["dmB"])
        eng.promote_shadow()
        assert eng.dm is p["dmB"] and eng.shadow is None
        eng.pump(1)                                          # rows [12288, 16384)
        after = _totals(eng, gpu)
        _, rB = score(p["dmB"], p["rows"][3 * 4096:4 * 4096], 0.5)
        torch.cuda.synchronize(gpu)
        nB = int(rB.sum().item())
        assert nB > 0 and after[1] - end[1] == nB
        assert after[40] == end[40] and after[0] == 4 * 4096
    finally:
        eng.close()


def test_refusals(gpu, fx):
    from ccfd_demo_summit_amd.engine import StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    p = fx["g32"]
    dmA, dmB, A = p["dmA"], p["dmB"], p["A"]
    with pytest.raises(ValueError, match="routing rules"):
        StreamEngine(dmA, rules=object(), shadow=dmB)
    with pytest.raises(ValueError, match="pipelined"):
        StreamEngine(dmA, exec_mode="persistent", persist_items="pipelined", shadow=dmB)
    with pytest.raises(ValueError, match="'gbdt' models have no shadow kernel"):
        StreamEngine(DeviceModel(A, gpu), shadow=DeviceModel(p["B"], gpu))
    eng = StreamEngine(dmA, batch=4096, depth=4, streams=1, exec_mode="persistent")
    try:
        with pytest.raises(ValueError, match="shape mismatch"):
            eng.set_shadow(DeviceModel(A.padded(n_trees=101), gpu, bins=p["spec"]))
        with pytest.raises(ValueError, match="bin tables differ"):
            eng.set_shadow(DeviceModel(A, gpu, bins=True))
        with pytest.raises(ValueError, match="g32 rows and the shadow for g20"):
            eng.set_shadow(fx["g20"]["dmA"])
        assert eng.shadow is None and eng.progress()["submitted"] == 0
    finally:
        eng.close()


def test_padded_challenger_rides_as_shadow(gpu, X, fx):
    """A smaller ensemble brought to the champion's shape scores what it scores alone."""
    from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_counters, score
    p = fx["g32"]
    B = p["B"]
    small = ObliviousGBDT(B.feat[:40, :4], B.thr[:40, :4], B.leaves[:40, :16], B.base - 1.0)
    n = 4097
    c = new_counters(gpu)
    _, _, ps = score(p["dmA"], p["rows"][:n], 0.5, counters=c,
                     shadow=DeviceModel(small.padded(n_trees=100, depth=6), gpu, bins=p["spec"]))
    torch.cuda.synchronize(gpu)
    assert np.abs(ps.cpu().numpy() - small.predict_proba(X[:n])).max() < 2e-5
    assert c.cpu().numpy()[40] == n


def test_train_hip_against_the_live_bin_table(gpu, X, fx):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, check_shadow_pair
    from ccfd_demo_summit_amd.train.trainer import train_oblivious_gbdt
    p = fx["g32"]
    n = 20000
    y = (p["refB"][:n] > np.quantile(p["refB"][:n], 0.95)).astype(np.int64)
    model, info = train_oblivious_gbdt(X[:n], y, n_trees=4, depth=4, device=str(gpu), hist="hip", bin_spec=p["spec"])
    assert info["hist"] == "hip" and np.isfinite(model.thr).all()
    assert p["spec"].contains(model.bin_spec())
    check_shadow_pair(p["dmA"], DeviceModel(model.padded(n_trees=100, depth=6), gpu, bins=p["spec"]))
