"""Shadow (challenger) scoring on the GPU: the fused launch kernel per row, the persistent and
the launch-mode engine by role swap (B as A's shadow must count what B counts as champion, to
the bit), the runtime toggle, promotion and the refusals."""
import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import build_model

pytestmark = pytest.mark.gpu

N_ENGINE = 3 * 4096 + 2 * 1000           # pump(3) + pump(2, batch_rows=1000)
ID_BASE = 1000


@pytest.fixture(scope="module")
def fx(gpu):
    """Rows, the two models (A: champion, B: challenger), their device blobs, the W64 rows on
    the device and the CPU wire oracles -- computed once, never modified."""
    from ccfd_demo_summit_amd.contracts import encode_wire
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    X, _ = generate(70001, seed=11)
    mA = build_model("mlp", seed=3, X_ref=X[:20000], calibrate_rate=0.01)
    mB = build_model("mlp", seed=4, X_ref=X[:20000], calibrate_rate=0.03)
    return {"X": X, "mA": mA, "mB": mB, "dmA": DeviceModel(mA, gpu, wire=True), "dmB": DeviceModel(mB, gpu, wire=True),
            "xw": torch.from_numpy(encode_wire(X)).to(gpu), "refA": mA.wire_proba(X), "refB": mB.wire_proba(X)}


def _totals(eng, gpu):
    """Sum of the two epoch buffers once everything submitted has completed."""
    side = torch.cuda.Stream(gpu)
    eng.flip_epoch(side)
    side.synchronize()
    return (eng.counters[0] + eng.counters[1]).cpu().numpy()


def _ids(flagged):
    return set((flagged["tx_id"].astype(np.int64) - ID_BASE).tolist())


def _run_engine(gpu, fx, champion, shadow, exec_mode):
    """pump(3) + pump(2, batch_rows=1000) over the fixture rows: n = 14288, with partial items
    and a partial last tile.  Returns (counter totals, flagged row indices)."""
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    X = fx["X"]
    eng = StreamEngine(champion, batch=4096, depth=4, streams=1, exec_mode=exec_mode, shadow=shadow)
    log = PartitionLog.from_arrays(X, ids=np.arange(X.shape[0], dtype=np.uint64) + ID_BASE, wire=True)
    try:
        eng.add_log(0, log)
        a = eng.pump(3)
        b = eng.pump(2, batch_rows=1000)
        assert a.rows + b.rows == N_ENGINE
        ids = _ids(eng.drain_flagged())
        return _totals(eng, gpu), ids
    finally:
        eng.close()
        log.free()


@pytest.fixture(scope="module")
def plain_a(gpu, fx):
    """Champion A, never a shadow: the reference for the champion's own counters and flags."""
    return {mode: _run_engine(gpu, fx, fx["dmA"], None, mode) for mode in ("persistent", "launch")}


def _check_role_swap(gpu, fx, plain, exec_mode):
    c1, ids1 = _run_engine(gpu, fx, fx["dmA"], fx["dmB"], exec_mode)
    c2, ids2 = _run_engine(gpu, fx, fx["dmB"], fx["dmA"], exec_mode)
    c3, ids3 = plain
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
    assert not c3[38:].any()


# The launch grid is ceil(tiles / 8) workgroups of 4 waves (one tile pair a wave), capped at 256;
# a wave starts at tile 4 * block + wave, strides by 4 * grid, and its steady-state loop takes
# two tiles a turn while tile < tiles - stride.  n = 70001 is 4376 tiles on the capped grid of
# 256, stride 1024: every wave owns 4 or 5 tiles, so its loop turns at tile t0 and t0 + 2048
# (both < 3352) -- exactly twice -- and the 280 waves with a fifth tile also take the tail, one of
# them the 1-row last tile.  n = 261 is 17 tiles on 3 workgroups (stride 12): five waves with one
# pair (the last one's second tile has 5 rows), seven with a lone tail tile.  4097: 33 workgroups.
@pytest.mark.parametrize("n", [1, 16, 17, 65, 261, 4097, 70001])
def test_launch_kernel_per_row(gpu, fx, n):
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    xw = fx["xw"][:n]
    c0, c1 = new_counters(gpu), new_counters(gpu)
    pA, rA = score(fx["dmA"], xw, 0.5, counters=c0)
    pB, _ = score(fx["dmB"], xw, 0.5)
    out = score(fx["dmA"], xw, 0.5, counters=c1, shadow=fx["dmB"])
    assert len(out) == 3
    torch.cuda.synchronize(gpu)
    p, r, ps = (t.cpu().numpy() for t in out)
    np.testing.assert_array_equal(p.view(np.uint32), pA.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(ps.view(np.uint32), pB.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(r, rA.cpu().numpy())
    da, db = np.abs(p - fx["refA"][:n]).max(), np.abs(ps - fx["refB"][:n]).max()
    print(f"n={n}: |p - A.wire_proba| max {da:.3g}, |ps - B.wire_proba| max {db:.3g}")
    assert da < 2e-4 and db < 2e-4
    c0, c1 = c0.cpu().numpy(), c1.cpu().numpy()
    np.testing.assert_array_equal(c1[:38], c0[:38])
    assert not c0[38:].any()
    fa, fb = p >= 0.5, ps >= 0.5
    assert c1[40] == n
    assert c1[41] == fb.sum()
    assert c1[42] == (fa & fb).sum()
    p64, ps64 = p.astype(np.float64), ps.astype(np.float64)
    assert abs(int(c1[43]) - np.round(ps64 * 1e6).sum()) <= n
    assert abs(int(c1[44]) - np.round(np.abs(p64 - ps64) * 1e6).sum()) <= n
    assert not c1[45:].any() and not c1[38:40].any()


def test_launch_kernel_identity(gpu, fx):
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    n = 4097
    c = new_counters(gpu)
    sp = torch.full((n + 3,), -1.0, device=gpu)
    p, r, ps = score(fx["dmA"], fx["xw"][:n], 0.5, counters=c, shadow=fx["dmA"], shadow_proba=sp)
    torch.cuda.synchronize(gpu)
    assert ps.data_ptr() == sp.data_ptr()
    np.testing.assert_array_equal(ps[:n].cpu().numpy().view(np.uint32), p.cpu().numpy().view(np.uint32))
    assert (sp[n:] == -1.0).all()                        # nothing written past row n
    c = c.cpu().numpy()
    assert c[1] > 0
    assert c[41] == c[42] == c[1] and c[43] == c[3] and c[44] == 0 and c[40] == n


def test_no_shadow_leaves_slots_zero(gpu, fx):
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    c = new_counters(gpu)
    out = score(fx["dmA"], fx["xw"][:4097], 0.5, counters=c)
    torch.cuda.synchronize(gpu)
    assert isinstance(out, tuple) and len(out) == 2
    c = c.cpu().numpy()
    assert c[0] == 4097 and not c[38:].any()
    with pytest.raises(ValueError):
        score(fx["dmA"], fx["xw"][:16], 0.5, shadow_proba=torch.empty(16, device=gpu))


@pytest.mark.parametrize("item_rows", [128, 256, 512])
def test_persistent_engine_role_swap(gpu, fx, plain_a, monkeypatch, item_rows):
    monkeypatch.setenv("CCFD_PERSIST_ITEM_ROWS", str(item_rows))
    _check_role_swap(gpu, fx, plain_a["persistent"], "persistent")


def test_launch_engine_role_swap_and_score_sync(gpu, fx, plain_a):
    from ccfd_demo_summit_amd.engine import StreamEngine
    _check_role_swap(gpu, fx, plain_a["launch"], "launch")
    eng = StreamEngine(fx["dmA"], batch=4096, depth=4, streams=1, exec_mode="launch", coalesce=8, shadow=fx["dmB"])
    try:
        p, r = eng.score(fx["X"][:5000])
        assert np.abs(p - fx["refA"][:5000]).max() < 2e-4
        np.testing.assert_array_equal(r, (p >= 0.5).astype(np.uint8))
        c = _totals(eng, gpu)
        assert c[0] == c[40] == 5000 and c[1] == r.sum() and c[41] > 0
    finally:
        eng.close()


def test_runtime_toggle_and_promote(gpu, fx, plain_a):
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import score
    X = fx["X"]
    eng = StreamEngine(fx["dmA"], batch=4096, depth=4, streams=1, exec_mode="persistent")
    log = PartitionLog.from_arrays(X, ids=np.arange(X.shape[0], dtype=np.uint64) + ID_BASE, wire=True)
    try:
        eng.add_log(0, log)
        eng.pump(1)
        assert _totals(eng, gpu)[40] == 0
        eng.set_shadow(fx["dmB"])
        assert eng.shadow is fx["dmB"]
        eng.pump(2)
        mid = _totals(eng, gpu)
        assert mid[40] == 2 * 4096 and mid[0] == 3 * 4096
        eng.set_shadow(None)
        eng.pump(2, batch_rows=1000)
        end = _totals(eng, gpu)
        assert end[40] == 2 * 4096 and end[0] == N_ENGINE
        np.testing.assert_array_equal(end[41:45], mid[41:45])
        # same rows in the same order as the engine that never had a shadow
        c3, ids3 = plain_a["persistent"]
        assert _ids(eng.drain_flagged()) == ids3
        np.testing.assert_array_equal(end[:38], c3[:38])
        s = eng.shadow_counters(end)
        assert s["rows"] == 2 * 4096 and 0.0 < s["mean_proba"] < 1.0 and s["mean_abs_diff"] > 0.0
        # promotion: B becomes the champion, shadow scoring stops
        eng.set_shadow(fx["dmB"])
        eng.promote_shadow()
        assert eng.dm is fx["dmB"] and eng.shadow is None
        eng.pump(1)                                          # rows [14288, 18384)
        after = _totals(eng, gpu)
        _, rB = score(fx["dmB"], fx["xw"][N_ENGINE:N_ENGINE + 4096], 0.5)
        torch.cuda.synchronize(gpu)
        nB = int(rB.sum().item())
        assert nB > 0 and after[1] - end[1] == nB
        assert after[40] == end[40] and after[0] == N_ENGINE + 4096
    finally:
        eng.close()
        log.free()


def test_refusals(gpu, fx, monkeypatch):
    from ccfd_demo_summit_amd.engine import StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    dmA, dmB = fx["dmA"], fx["dmB"]
    f32B = DeviceModel(fx["mB"], gpu)

    def fake(kind):              # refused before anything reads the blob
        return DeviceModel.from_blob(kind, torch.zeros(64, dtype=torch.uint8, device=gpu), trees=1, depth=1)

    with pytest.raises(ValueError, match="champion MLP is packed for f32"):
        StreamEngine(DeviceModel(fx["mA"], gpu), shadow=dmB)
    for kind in ("lr", "gbdt", "forest"):
        with pytest.raises(ValueError, match=f"'{kind}' models have no shadow kernel"):
            StreamEngine(fake(kind), shadow=fake(kind))
    with pytest.raises(ValueError, match="routing rules"):
        StreamEngine(dmA, rules=object(), shadow=dmB)
    with pytest.raises(ValueError, match="pipelined"):
        StreamEngine(dmA, exec_mode="persistent", persist_items="pipelined", shadow=dmB)

    eng = StreamEngine(dmA, batch=4096, depth=4, streams=1, exec_mode="persistent")
    try:
        with pytest.raises(ValueError, match="shadow MLP is packed for f32"):
            eng.set_shadow(f32B)
        with pytest.raises(ValueError, match="kind mismatch"):
            eng.set_shadow(fake("lr"))
        assert eng.shadow is None and eng.progress()["submitted"] == 0
    finally:
        eng.close()

    # the environment's pipelined items are known to the native engine only: it refuses
    monkeypatch.setenv("CCFD_PERSIST_PIPE", "1")
    with pytest.raises(RuntimeError, match="pipelined persistent items"):
        StreamEngine(dmA, batch=4096, depth=4, streams=1, exec_mode="persistent", shadow=dmB)
    monkeypatch.delenv("CCFD_PERSIST_PIPE")
    monkeypatch.setenv("CCFD_PERSIST_ITEM_ROWS", "64")
    eng = StreamEngine(dmA, batch=4096, depth=4, streams=1, exec_mode="persistent")
    try:
        with pytest.raises(RuntimeError, match="items of 64 rows"):
            eng.set_shadow(dmB)
        assert eng.shadow is None and eng.progress()["submitted"] == 0
    finally:
        eng.close()


def test_engine_service_publishes_shadow_counters(gpu, fx):
    """The rank loop with a shadow: rings fed from a broker, persistent kernel, X2 reduction,
    Prometheus series.  The shadow is a second copy of the champion's weights, so its counters
    must repeat the champion's exactly."""
    import time

    from prometheus_client import CollectorRegistry, generate_latest

    from ccfd_demo_summit_amd.ingest import InProcBroker, ProducerConfig, TransactionProducer
    from ccfd_demo_summit_amd.launch.engine_service import EngineService, EngineServiceConfig
    from ccfd_demo_summit_amd.metrics import MetricsHub
    from ccfd_demo_summit_amd.metrics.exporter import GpuEngineCollector
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    from ccfd_demo_summit_amd.parallel import DistContext
    from ccfd_demo_summit_amd.process import ProcessEngine
    from ccfd_demo_summit_amd.router import Router, RuleSet
    broker = InProcBroker(default_partitions=2)
    broker.create_topic("odh-demo", 2)
    total = 20_000
    TransactionProducer(broker, ProducerConfig(fmt="txb1", batch=2500, seed=5)).produce(total)
    hub = MetricsHub()
    router = Router(RuleSet.threshold(0.5), ProcessEngine(notification_timeout_s=60), hub.router)
    svc = EngineService(DistContext(0, 1, 0, gpu, "none"), fx["dmA"], broker, router,
                        EngineServiceConfig(batch=4096, depth=4, streams=2, ring_rows=16384, flush_us=200,
                                            reduce_period_ms=1.0, shadow_model="copy-of-a.safetensors"),
                        shadow=DeviceModel(fx["mA"], gpu, wire=True)).start()
    try:
        assert svc.exec_mode == "persistent" and svc.engine.shadow is not None
        t0 = time.time()
        while svc.rows_scored < total and time.time() - t0 < 30:
            svc.step()
        svc.reducer.wait()
        assert svc.rows_scored == total
        svc.flush_epochs()
        c, _ = svc.reducer.snapshot()
        assert c[0] == c[40] == total and c[1] > 0
        assert c[41] == c[42] == c[1] and c[43] == c[3] and c[44] == 0
        reg = CollectorRegistry()
        reg.register(GpuEngineCollector(svc.metrics_source, rank_label="0"))
        text = generate_latest(reg).decode()
        assert f'ccfd_gpu_shadow_rows_total{{rank="0"}} {float(total)}' in text
        assert f'ccfd_gpu_shadow_both_fraud_total{{rank="0"}} {float(c[1])}' in text
    finally:
        svc.stop()
