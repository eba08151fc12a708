"""Every depth, odd tree counts and split edges of the oblivious-GBDT kernels (score_gbdt.hip
v1 / v2, score_gbdt_g32.hip, score_gbdt_g32_persist.hip, score_gbdt_shadow.hip) against the
float64 numpy reference, on the fixtures of tests/helpers/gbdt_edges.py: rows exactly on, one ulp
below and one ulp above every split threshold, NaN / inf / -0.0 / subnormal features, amounts on
every histogram bound, bin tables with the most edges a row format can carry.

Tolerance: the suite's 1e-5 on probabilities.  test_gbdt_edges_cpu.py proves on the reference
that on every fixture here a single wrong leaf moves the probability by >= 1e-4 and that >= 99 %
of the rows are more than 1e-5 from the routing threshold; routes are compared exactly on those.
Row counts 1, 64, 65, 513, 1025: a lane, a 64-row chunk, a chunk + 1 row, a second workgroup
at one and at two chunks per wave step."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.contracts.metric_names import AMOUNT_BUCKETS
from ccfd_demo_summit_amd.contracts.transaction import AMOUNT_COL, amount_bucket
from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import build_model
from tests.helpers import gbdt_edges as ge

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# variant -> (row format, environment read per launch, strided f32 view)
VARIANTS = {
    "f32-v1": ("f32", {}, False),
    "f32-v1-strided": ("f32", {}, True),
    "g32": ("g32", {}, False),
    "g32-r2": ("g32", {"CCFD_G32_R": "2"}, False),
    "g32-global-leaves": ("g32", {"CCFD_G32_GLOBAL_LEAVES": "1"}, False),
    "g32-one-wg-per-cu": ("g32", {"CCFD_G32_WGS_PER_CU": "1"}, False),
    "g20": ("g20", {}, False),
    "g20-global-leaves": ("g20", {"CCFD_G32_GLOBAL_LEAVES": "1"}, False),
}


def _device_model(gpu, model, fmt, spec=None):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    if fmt == "f32":
        return DeviceModel(model, gpu)
    return DeviceModel(model, gpu, bins=spec if spec is not None else (True if fmt == "g32" else "g20"))


def _device_rows(gpu, dm, X, strided=False):
    if dm.bins is not None:
        return torch.from_numpy(dm.bins.encode(X)).to(gpu)
    if not strided:
        return torch.from_numpy(np.array(X, np.float32)).to(gpu)
    big = np.zeros((X.shape[0], 32), np.float32)            # ld = 32: the generic (non-contiguous) loader
    big[:, :30] = X
    return torch.from_numpy(big).to(gpu)[:, :30]


def _score_and_judge(gpu, dm, X, ref, strided=False, threshold=0.5):
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    cnt = new_counters(gpu)
    p, r = score(dm, _device_rows(gpu, dm, X, strided), threshold, counters=cnt)
    torch.cuda.synchronize(gpu)
    return ge.judge(p.cpu().numpy(), r.cpu().numpy(), cnt.cpu().numpy(), ref, X, threshold)


def _run_variant(gpu, monkeypatch, case, variant):
    fmt, env, strided = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, X, ref = case
    assert ge.clear_rows(ref, 0.5).mean() >= ge.CLEAR_FRACTION
    dm = _device_model(gpu, m, fmt)
    for n in ge.ROW_COUNTS:
        i = ge.take(len(X), n)
        j = _score_and_judge(gpu, dm, X[i], ref[i], strided)
        print(f"{variant} {m.n_trees}x{m.depth} n={n}: {j}")
        ge.assert_judged(j, (variant, m.n_trees, m.depth, n))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("trees", ge.TREES)
@pytest.mark.parametrize("depth", ge.DEPTHS)
def test_every_depth_and_tree_count(gpu, monkeypatch, depth, trees, variant):
    """Depths 1..8 x 1, 3, 5, 8 trees (the trees-at-a-time blocks of 4 with 1, 3, 1 and 0 trees
    left over; depth 1 the only one whose leaf table is no multiple of a float4) through the f32
    v1 kernel, contiguous and strided, and the G32 / G20 launch kernel with one and two chunks
    per wave step, leaves in LDS and in global memory."""
    _run_variant(gpu, monkeypatch, ge.shape_case(trees, depth), variant)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("depth", ge.DEPTHS)
def test_probe_tree_leaf_identified_at_every_depth(gpu, monkeypatch, depth, variant):
    """One tree whose 2^depth leaves are linspace(-4, 4) shuffled: the probability names the leaf."""
    _run_variant(gpu, monkeypatch, ge.probe_case(depth), variant)


@pytest.mark.parametrize("strided", [False, True])
def test_f32_v1_leaf_chunks_not_resident(gpu, strided):
    """131 x depth 7: the leaf table exceeds the 16384 floats v1 keeps in LDS, so every 64-row
    chunk re-stages it in two pieces (128 trees, then the last 3)."""
    m, X, ref = ge.chunked_case()
    assert m.n_trees << m.depth > 16384 and m.n_trees % (16384 >> m.depth) != 0
    dm = _device_model(gpu, m, "f32")
    for n in (65, len(X)):
        i = ge.take(len(X), n)
        j = _score_and_judge(gpu, dm, X[i], ref[i], strided)
        print(f"chunked n={n} strided={strided}: {j}")
        ge.assert_judged(j, n)


@pytest.mark.parametrize("rows_per_step", ["1", "2"])
def test_f32_v2_kernel_every_depth_and_tree_count(gpu, rows_per_step):
    """score_gbdt.hip v2 (rows in registers), one and two chunks per wave step, depths 1..8 x
    1, 3, 5, 8 trees and the probe trees at the small row counts: CCFD_GBDT_KERNEL and CCFD_GBDT_R
    are read once per process, so a child process scores and this test judges every line it
    printed.  Nothing reports which kernel a launch took, and launch_gbdt falls back to v1 for
    rows that are not contiguous and 16-byte aligned, so the test also pins a difference the two
    kernels must show: v1 adds the trees as four per-wave partial sums, v2 one after the other
    (test_gbdt_edges_cpu.py shows on float32 arithmetic alone that the two orders give different
    sums on these rows), hence the child's probabilities of the 8-tree ensembles of depth >= 2
    cannot be bit-identical to the v1 launch of this process."""
    env = dict(os.environ, CCFD_GBDT_KERNEL="v2", CCFD_GBDT_R=rows_per_step)
    # child: interpreter + torch + HIP start-up (tens of seconds at worst), 40 fixtures (~1 s),
    # 200 launches of <= 1025 rows (milliseconds each)
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "gbdt_variant_probe.py")], env=env,
                       capture_output=True, text=True, timeout=150)
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert lines[0] == {"kernel": "v2", "R": rows_per_step}
    assert lines[-1] == {"done": len(ge.DEPTHS) * (len(ge.TREES) + 1) * len(ge.ROW_COUNTS)}
    cases = lines[1:-1]
    assert {(j["depth"], j["trees"], j["n"]) for j in cases} == \
        {(d, t, n) for d in ge.DEPTHS for t in (0,) + ge.TREES for n in ge.ROW_COUNTS}      # 0: the probe tree
    bad = [(j["depth"], j["trees"], j["n"], j["err"], j["route_mismatch"], j["counters"]) for j in cases
           if not (j["err"] < ge.TOL and j["route_mismatch"] == 0 and j["counters"] is None)]
    print("failing (depth, trees, n, max err, route mismatches, counters):", *bad, sep="\n")
    assert not bad, f"{len(bad)} of {len(cases)} launches, first {bad[:6]}"
    assert all(j["clear"] > 0 for j in cases)
    # this process takes v1 below 262144 rows
    assert os.environ.get("CCFD_GBDT_KERNEL") in (None, "v1")
    from ccfd_demo_summit_amd.ops.kernels import score
    n = ge.ROW_COUNTS[-1]
    same = []
    for depth in ge.ORDER_DEPTHS:
        m, X, _ = ge.shape_case(ge.ORDER_TREES, depth)
        dm = _device_model(gpu, m, "f32")
        p1, _ = score(dm, _device_rows(gpu, dm, X[ge.take(len(X), n)]), 0.5)
        torch.cuda.synchronize(gpu)
        crc2 = [j["crc"] for j in cases if (j["depth"], j["trees"], j["n"]) == (depth, ge.ORDER_TREES, n)]
        if crc2 == [zlib.crc32(p1.cpu().numpy().tobytes())]:
            same.append(depth)
    assert not same, f"depths {same}: the child's probabilities are v1's to the bit, v2 was not launched"


# --------------------------------------------------------------------------- persistent engines
BATCH = 4096
N_ENGINE = 2 * BATCH + 1234                  # two full micro-batches and a partial one
ID_BASE = 7


def _totals(eng, gpu):
    side = torch.cuda.Stream(gpu)
    eng.flip_epoch(side)
    side.synchronize()
    return (eng.counters[0] + eng.counters[1]).cpu().numpy()


def _pump_log(eng, log):
    eng.add_log(0, log)
    assert eng.pump(2).rows + eng.pump(1, batch_rows=N_ENGINE - 2 * BATCH).rows == N_ENGINE


def _check_persistent(gpu, model, spec, X, ref):
    """A persistent engine over ``X`` tiled to N_ENGINE rows: every row's proba and route from the
    kernel's own outputs (scored ring), flagged ids, counters and histograms; then eng.score()."""
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    i = ge.take(len(X), N_ENGINE)
    Xn, refn = X[i], ref[i]
    clear = ge.clear_rows(refn, 0.5)
    assert clear.mean() >= ge.CLEAR_FRACTION
    dm = DeviceModel(model, gpu, bins=spec)
    eng = StreamEngine(dm, batch=BATCH, depth=2, streams=1, exec_mode="persistent")
    log = PartitionLog.from_arrays(Xn, ids=np.arange(N_ENGINE, dtype=np.uint64) + ID_BASE, bins=dm.bins)
    try:
        eng.enable_scored(N_ENGINE)
        _pump_log(eng, log)
        rec = eng.drain_scored()
        ids = rec["tx_id"].astype(np.int64) - ID_BASE
        np.testing.assert_array_equal(np.sort(ids), np.arange(N_ENGINE))
        p = np.empty(N_ENGINE, np.float32)
        r = np.empty(N_ENGINE, np.uint8)
        p[ids], r[ids] = rec["proba"], rec["route"] != 0
        fl = eng.drain_flagged()
        got = np.zeros(N_ENGINE, bool)
        got[fl["tx_id"].astype(np.int64) - ID_BASE] = True
        np.testing.assert_array_equal(got, r.astype(bool))
        j = ge.judge(p, r, _totals(eng, gpu), refn, Xn)
        print(f"persistent {spec.row_format} {model.n_trees}x{model.depth}: {j}")
        ge.assert_judged(j)
        ps, _ = eng.score(X)
        assert np.abs(ps.astype(np.float64) - ref).max() < ge.TOL
    finally:
        eng.close()
        log.free()


@pytest.mark.parametrize("fmt,depth,trees,global_leaves", [
    ("g32", 1, 3, False), ("g32", 2, 5, False), ("g32", 5, 3, False), ("g32", 7, 5, False),
    ("g20", 1, 5, False), ("g20", 7, 3, False), ("g32", 5, 5, True)])
def test_persistent_engine_depths_and_odd_tree_counts(gpu, monkeypatch, fmt, depth, trees, global_leaves):
    if global_leaves:
        monkeypatch.setenv("CCFD_G32_GLOBAL_LEAVES", "1")
    m, X, ref = ge.shape_case(trees, depth)
    _check_persistent(gpu, m, m.bin_spec(8 if fmt == "g32" else 5), X, ref)


# --------------------------------------------------------------------------- shadow kernels
def _check_shadow_counters(c, n, pa, fa, pb):
    """CNT_SHADOW_* of ``n`` rows against the per-row outputs, as test_shadow_gbdt_gpu.py does: the
    counts exactly, the two sums within the half unit per row their rounding allows."""
    assert c[40] == n and not c[38:40].any() and not c[45:].any()
    fb = pb >= 0.5
    assert c[41] == fb.sum() and c[42] == (fa & fb).sum()
    assert abs(int(c[43]) - np.round(pb.astype(np.float64) * 1e6).sum()) <= n
    assert abs(int(c[44]) - np.round(np.abs(pa.astype(np.float64) - pb.astype(np.float64)) * 1e6).sum()) <= n


def _check_shadow_launch(gpu, A, B, spec, X, refA, refB, counts):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_counters, score
    dmA, dmB = DeviceModel(A, gpu, bins=spec), DeviceModel(B, gpu, bins=spec)
    for ref in (refA, refB):
        assert ge.clear_rows(ref, 0.5).mean() >= ge.CLEAR_FRACTION
    for n in counts:
        i = ge.take(len(X), n)
        c = new_counters(gpu)
        out = score(dmA, torch.from_numpy(spec.encode(X[i])).to(gpu), 0.5, counters=c, shadow=dmB)
        torch.cuda.synchronize(gpu)
        pa, r, pb = (t.cpu().numpy() for t in out)
        c = c.cpu().numpy()
        j = ge.judge(pa, r, c, refA[i], X[i])
        eb = float(np.abs(pb.astype(np.float64) - refB[i]).max())
        print(f"shadow {spec.row_format} {A.n_trees}x{A.depth} n={n}: {j}, challenger err {eb:.3g}")
        ge.assert_judged(j, n)
        assert eb < ge.TOL
        clear = ge.clear_rows(refB[i], 0.5)
        np.testing.assert_array_equal((pb >= 0.5)[clear], (refB[i] >= 0.5)[clear])
        _check_shadow_counters(c, n, pa, r.astype(bool), pb)


@pytest.mark.parametrize("fmt", ["g32", "g20"])
@pytest.mark.parametrize("trees,depth", ge.SHADOW_SHAPES)
def test_shadow_launch_small_and_deep_tables(gpu, trees, depth, fmt):
    """Depth 1 with 3 and 2 trees: the champion's leaf table is 6 / 4 floats and the challenger's
    starts behind it at the next float4; depth 7 with 5 trees."""
    _check_shadow_launch(gpu, *ge.shadow_case(trees, depth, 8 if fmt == "g32" else 5), ge.ROW_COUNTS)


def _persistent_rows(gpu, log, champion, shadow):
    """One persistent engine over ``log``: per-row (proba, route) from the scored ring in log
    order, and the counter totals."""
    from ccfd_demo_summit_amd.engine import StreamEngine
    eng = StreamEngine(champion, batch=BATCH, depth=2, streams=1, exec_mode="persistent", shadow=shadow)
    try:
        eng.enable_scored(N_ENGINE)
        _pump_log(eng, log)
        rec = eng.drain_scored()
        ids = rec["tx_id"].astype(np.int64) - ID_BASE
        np.testing.assert_array_equal(np.sort(ids), np.arange(N_ENGINE))
        p = np.empty(N_ENGINE, np.float32)
        r = np.empty(N_ENGINE, np.uint8)
        p[ids], r[ids] = rec["proba"], rec["route"] != 0
        return p, r, _totals(eng, gpu)
    finally:
        eng.close()


@pytest.mark.parametrize("trees,depth,fmt", [(3, 1, "g32"), (2, 1, "g32"), (5, 7, "g32"), (2, 1, "g20")])
def test_shadow_persistent_small_and_deep_tables(gpu, trees, depth, fmt):
    """The persistent kernel writes no per-row challenger output, so the challenger's rows come
    from a role swap: B scored as champion over the same log, judged per row against its
    reference; what B counts as A's shadow must then be exactly what those rows give."""
    from ccfd_demo_summit_amd.engine import PartitionLog
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    A, B, spec, X, refA, refB = ge.shadow_case(trees, depth, 8 if fmt == "g32" else 5)
    i = ge.take(len(X), N_ENGINE)
    Xn = X[i]
    dmA, dmB = DeviceModel(A, gpu, bins=spec), DeviceModel(B, gpu, bins=spec)
    log = PartitionLog.from_arrays(Xn, ids=np.arange(N_ENGINE, dtype=np.uint64) + ID_BASE, bins=spec)
    try:
        pa, fa, c1 = _persistent_rows(gpu, log, dmA, dmB)
        pb, fb, c2 = _persistent_rows(gpu, log, dmB, None)
    finally:
        log.free()
    ge.assert_judged(ge.judge(pa, fa, c1, refA[i], Xn), "champion")
    ge.assert_judged(ge.judge(pb, fb, c2, refB[i], Xn), "challenger as champion")
    np.testing.assert_array_equal(fb.astype(bool), pb >= 0.5)
    assert not c2[38:].any()
    assert (c1[41], c1[43]) == (c2[1], c2[3])             # B as A's shadow counts what B counts alone
    _check_shadow_counters(c1, N_ENGINE, pa, fa.astype(bool), pb)


# --------------------------------------------------------------------------- full bin tables
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("variant", ["g32", "g32-r2", "g20"])
def test_feature_sweep_launch(gpu, monkeypatch, variant, which):
    """255 (31) edges on every feature, tree f splitting feature f at both ends or in the middle
    of its table: every byte / 5-bit field decides a leaf, with bin 0 and the highest bin next
    to it."""
    fmt, env, _ = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec, m, X, _, ref = ge.sweep_case(8 if fmt == "g32" else 5, which)
    dm = _device_model(gpu, m, fmt, spec)
    for n in (len(X), 1025):
        i = ge.take(len(X), n)
        j = _score_and_judge(gpu, dm, X[i], ref[i])
        print(f"sweep {variant} ks={ge.SWEEP_KS[spec.bits][which]} n={n}: {j}")
        ge.assert_judged(j, n)


@pytest.mark.parametrize("bits", [8, 5])
def test_feature_sweep_persistent(gpu, bits):
    spec, m, X, _, ref = ge.sweep_case(bits, 0)
    _check_persistent(gpu, m, spec, X, ref)


@pytest.mark.parametrize("bits", [8, 5])
def test_feature_sweep_as_shadow_challenger(gpu, bits):
    spec, B, X, _, refB = ge.sweep_case(bits, 0)
    _, A, XA, _, refA = ge.sweep_case(bits, 1)
    np.testing.assert_array_equal(X, XA)
    _check_shadow_launch(gpu, A, B, spec, X, refA, refB, (len(X), 1025))


# --------------------------------------------------------------------------- routing thresholds
@pytest.mark.parametrize("fmt", ["f32", "g32", "g20"])
def test_threshold_route_away_from_one_half(gpu, fmt):
    """The kernels sum in a fixed order, so a second launch reproduces p to the bit: with the
    threshold set to a row's own probability the route is exactly p >= p[i], row i included;
    0.0 routes every fresh row to fraud and 1.0 none."""
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    m, X, _ = ge.shape_case(5, 4)
    dm = _device_model(gpu, m, fmt)
    rows = _device_rows(gpu, dm, X)
    stale = None
    if fmt != "f32":
        stale = 3
        enc = dm.bins.encode(X)
        if fmt == "g32":
            enc[stale, 31] = (enc[stale, 31] % 255) + 1
        else:
            enc[stale, 19] = (enc[stale, 19] & 0x03) | (((dm.bins.stamp % 63) + 1) << 2)
        rows = torch.from_numpy(enc).to(gpu)
    fresh = np.ones(len(X), bool)
    if stale is not None:
        fresh[stale] = False
    p0, _ = score(dm, rows, 0.5)
    torch.cuda.synchronize(gpu)
    p0 = p0.cpu().numpy()
    assert np.isnan(p0[~fresh]).all() and not np.isnan(p0[fresh]).any()
    order = np.argsort(np.where(fresh, p0, np.inf))
    i = int(order[fresh.sum() // 2])                       # the median row
    for thr, want in ((float(p0[i]), fresh & (p0 >= p0[i])), (0.0, fresh), (1.0, np.zeros(len(X), bool))):
        cnt = new_counters(gpu)
        p, r = score(dm, rows, thr, counters=cnt)
        torch.cuda.synchronize(gpu)
        p, r = p.cpu().numpy(), r.cpu().numpy()
        np.testing.assert_array_equal(p.view(np.uint32)[fresh], p0.view(np.uint32)[fresh])
        np.testing.assert_array_equal(r.astype(bool), want)
        assert ge.counters_problem(cnt.cpu().numpy(), p, r, X, stale=int((~fresh).sum())) is None
    assert want.sum() == 0 and not (p0 == 1.0).any()
    mid = fresh & (p0 >= p0[i])
    assert mid[i] and 0 < mid.sum() < fresh.sum()


# --------------------------------------------------------------------------- the other histogram paths
@pytest.fixture(scope="module")
def amount_rows():
    """generate() rows whose amounts are the finite histogram bounds and their float neighbours."""
    X, _ = generate(4096, seed=61)
    f32 = np.float32
    amounts = [f32(0.0)]
    for b in AMOUNT_BUCKETS:
        amounts += [np.nextafter(f32(b), f32(-np.inf)), f32(b), np.nextafter(f32(b), f32(np.inf))]
    Xa = X[:len(amounts)].copy()
    Xa[:, AMOUNT_COL] = amounts
    assert set(amount_bucket(Xa[:, AMOUNT_COL]).tolist()) == set(range(14))
    return X, Xa


@pytest.mark.parametrize("n,start", [(16, 0), (17, 16), (65, 0)])
@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("kind", ["lr", "mlp"])
def test_amount_bounds_through_lr_and_mlp_histograms(gpu, amount_rows, kind, wire, n, start):
    """The LR / MLP epilogues (per-lane bound counters, fraud rows per row) with amounts exactly on
    and next to every bound: both histograms exact on f32 and W64 rows."""
    from ccfd_demo_summit_amd.contracts import encode_wire
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_counters, score
    Xref, Xa = amount_rows
    X = Xa[(np.arange(n) + start) % len(Xa)]
    m = build_model(kind, seed=1, X_ref=Xref, calibrate_rate=0.3)
    dm = DeviceModel(m, gpu, wire=wire)
    x = torch.from_numpy(encode_wire(X) if wire else X).to(gpu)
    cnt = new_counters(gpu)
    p, r = score(dm, x, 0.5, counters=cnt)
    torch.cuda.synchronize(gpu)
    p, r = p.cpu().numpy(), r.cpu().numpy()
    np.testing.assert_array_equal(r, (p >= 0.5).astype(np.uint8))
    if n == 65:
        assert 0 < r.sum() < n                            # both histograms are populated
    assert ge.counters_problem(cnt.cpu().numpy(), p, r, X) is None
