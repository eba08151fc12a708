"""csrc/kernels/drift_hist.hip against the numpy oracle (models/drift.py bin_counts): integer
counts, so every comparison is for equality.  Then DriftMonitor, GpuScorer.set_drift behind the
REST routes, and EngineService(drift=) over the in-process broker."""
import asyncio
import time

import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models.drift import DriftReference, DriftReport, bin_counts
from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 257, 5000)


@pytest.fixture(scope="module")
def fx(gpu):
    X, _ = generate(40_000, seed=7)
    model = ObliviousGBDT.random_init(100, 6, 0, X)
    out = {"X": X, "model": model}
    for fmt, bits in (("g32", 8), ("g20", 5)):
        bins = model.bin_spec(bits=bits)
        host = np.ascontiguousarray(bins.encode(X[:5000]))
        out[fmt] = {"bins": bins, "host": host, "dev": torch.from_numpy(host).to(gpu),
                    "want": {n: bin_counts(host[:n], bins.stamp) for n in SIZES}}
    return out


def same(got, want) -> bool:
    counts, tail = got
    assert counts.dtype == torch.uint64 and tail.dtype == torch.uint64
    return torch.equal(counts.cpu(), torch.from_numpy(want[0])) and torch.equal(tail.cpu(), torch.from_numpy(want[1]))


@pytest.mark.parametrize("max_workgroups", [1, 512])
@pytest.mark.parametrize("fmt", ["g32", "g20"])
def test_drift_histogram_equals_the_oracle(fx, fmt, max_workgroups):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram
    f = fx[fmt]
    for n in SIZES:
        rows = f["dev"][:n]
        assert same(drift_histogram(rows, f["bins"].stamp, max_workgroups=max_workgroups), f["want"][n]), n


def test_g20_rows_at_an_odd_row_are_four_byte_aligned_only(fx):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram
    f = fx["g20"]
    rows = f["dev"][1:1 + 257]
    assert rows.is_contiguous() and rows.data_ptr() % 16 == 4
    assert same(drift_histogram(rows, f["bins"].stamp), bin_counts(f["host"][1:258], f["bins"].stamp))


@pytest.mark.parametrize("fmt", ["g32", "g20"])
def test_worst_contention_identical_rows(fx, fmt):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram
    f = fx[fmt]
    host = np.repeat(f["host"][:1], 4096, axis=0)
    counts, tail = drift_histogram(torch.from_numpy(host).to(f["dev"].device), f["bins"].stamp)
    assert same((counts, tail), bin_counts(host, f["bins"].stamp))
    c = counts.cpu().numpy()
    assert ((c != 0).sum(1) == 1).all() and (c.max(1) == 4096).all() and tail.cpu().tolist() == [4096, 0]


@pytest.mark.parametrize("fmt", ["g32", "g20"])
def test_accumulates_mixes_stamps_and_skips_empty(fx, fmt):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram, new_drift_counts
    f = fx[fmt]
    stamp = f["bins"].stamp
    rows = f["dev"][:5000]
    counts, tail = new_drift_counts(rows.device)
    for _ in range(2):
        out = drift_histogram(rows, stamp, counts, tail)
        assert out[0] is counts and out[1] is tail
    want = f["want"][5000]
    assert same((counts, tail), (2 * want[0], 2 * want[1]))
    # n = 0 leaves the outputs untouched
    drift_histogram(rows[:0], stamp, counts, tail)
    assert same((counts, tail), (2 * want[0], 2 * want[1]))
    # two stamps in one batch: the other table's rows count in tail[1] only
    other = ObliviousGBDT.random_init(100, 6, 1, fx["X"]).bin_spec(bits=f["bins"].bits)
    assert other.stamp != stamp
    mixed = f["host"][:3000].copy()
    mixed[500:1234] = other.encode(fx["X"][500:1234])
    got = drift_histogram(torch.from_numpy(mixed).to(rows.device), stamp)
    oracle = bin_counts(mixed, stamp)
    assert oracle[1].tolist() == [3000 - 734, 734] and same(got, oracle)


def test_refusals_happen_before_any_launch(fx):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram, new_drift_counts
    f32, f20 = fx["g32"], fx["g20"]
    dev = f32["dev"].device
    counts, tail = new_drift_counts(dev)
    raw = torch.zeros(64 * 32 + 16, dtype=torch.uint8, device=dev)
    view = raw[8:8 + 64 * 32].view(64, 32)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError, match="G32 rows must be 16-byte aligned"):
        drift_histogram(view, f32["bins"].stamp, counts, tail)
    with pytest.raises(RuntimeError, match="G32 stamp outside 1..255"):
        drift_histogram(f32["dev"][:64], 0, counts, tail)
    with pytest.raises(RuntimeError, match="G32 stamp outside 1..255"):
        drift_histogram(f32["dev"][:64], 256, counts, tail)
    with pytest.raises(RuntimeError, match="G20 stamp outside 1..63"):
        drift_histogram(f20["dev"][:64], 64, counts, tail)
    with pytest.raises(RuntimeError, match="max_workgroups < 1"):
        drift_histogram(f20["dev"][:64], 5, counts, tail, max_workgroups=0)
    with pytest.raises(ValueError, match="uint64"):
        drift_histogram(f20["dev"][:64], 5, counts.view(torch.int64), tail)
    with pytest.raises(ValueError, match="rows must be"):
        drift_histogram(f32["dev"][:64, :31], 5)
    torch.cuda.synchronize()
    assert int(counts.view(torch.int64).sum()) == 0 and int(tail.view(torch.int64).sum()) == 0


def test_drift_monitor_host_and_device_paths_agree_with_the_oracle(fx, gpu):
    from ccfd_demo_summit_amd.ops.kernels import DriftMonitor
    bins = fx["g20"]["bins"]
    ref = DriftReference.fit(fx["X"][0::2], bins)
    with pytest.raises(ValueError, match="g20 rows"):
        DriftMonitor(ref, gpu).observe(fx["g32"]["dev"][:64])
    live = fx["X"][1::2].copy()
    live[:, 14] += fx["X"][:, 14].std()
    host = np.ascontiguousarray(bins.encode(np.concatenate([live] * 11)[:210_000]))
    counts, tail = bin_counts(host, bins.stamp)
    want = DriftReport.compare(ref, counts, tail)
    a, b = DriftMonitor(ref, gpu), DriftMonitor(ref, gpu)
    dev = torch.from_numpy(host).to(gpu)
    for i in range(3):                       # 70 000 rows: a split chunk, and both buffers reused
        a.observe_host(host[70_000 * i:70_000 * (i + 1)])
        b.observe(dev[70_000 * i:70_000 * (i + 1)])
    for mon in (a, b):
        rep = mon.report()
        assert rep.rows == 210_000 and rep.stale == 0
        assert np.array_equal(rep.psi, want.psi) and rep.status == want.status
        assert torch.equal(mon.counts.cpu(), torch.from_numpy(counts))
    assert want.status[14] == "drift" and want.drifting == 1
    rep = a.report(reset=True)
    assert rep.rows == 210_000
    rep = a.report()
    assert rep.rows == 0 and rep.status == ["insufficient"] * 31
    assert int(a.counts.view(torch.int64).sum()) == 0 and int(a.tail.view(torch.int64).sum()) == 0
    a.observe_host(host[:12_000])            # the next window
    assert a.report().rows == 12_000
    a.close()
    b.close()


def test_gpu_scorer_drift_route_equals_the_oracle(fx, gpu):
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.contracts import seldon
    from ccfd_demo_summit_amd.serving import GpuScorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    bins = fx["g32"]["bins"]
    ref = DriftReference.fit(fx["X"][0::2], bins)
    live = fx["X"][1::2][:3000]
    want = DriftReport.compare(ref, *bin_counts(bins.encode(live), bins.stamp), min_rows=1000)
    scorer = GpuScorer(fx["model"])

    async def go():
        srv = SeldonServer(scorer)
        async with TestClient(TestServer(srv.app)) as cl:
            assert (await cl.get("/drift")).status == 400
            scorer.set_drift(ref, min_rows=1000)
            for lo in range(0, 3000, 1000):
                r = await cl.post("/api/v0.1/predictions", json=seldon.build_request(live[lo:lo + 1000]))
                assert r.status == 200
            js = await (await cl.get("/api/v1.0/drift")).json()
            assert js["rows"] == 3000 and js["stale"] == 0
            assert js["psi"] == want.psi.tolist() and js["status"] == want.status
            r = await cl.post("/drift", json={"reset": True})
            assert (await r.json())["rows"] == 3000
            assert (await (await cl.get("/drift")).json())["rows"] == 0
    try:
        asyncio.new_event_loop().run_until_complete(go())
    finally:
        scorer.set_drift(None)
        scorer.close()


def test_engine_service_taps_every_ingested_row(fx, gpu):
    from prometheus_client import CollectorRegistry, generate_latest

    from ccfd_demo_summit_amd.contracts.transaction import TxBatch
    from ccfd_demo_summit_amd.ingest import InProcBroker, ProducerConfig, TransactionProducer
    from ccfd_demo_summit_amd.launch.engine_service import EngineService, EngineServiceConfig
    from ccfd_demo_summit_amd.metrics import MetricsHub
    from ccfd_demo_summit_amd.metrics.exporter import GpuEngineCollector
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, DriftMonitor
    from ccfd_demo_summit_amd.parallel import DistContext
    from ccfd_demo_summit_amd.process import ProcessEngine
    from ccfd_demo_summit_amd.router import Router, RuleSet
    bins = fx["g20"]["bins"]
    ref = DriftReference.fit(fx["X"][0::2], bins)
    broker = InProcBroker(default_partitions=2)
    broker.create_topic("odh-demo", 2)
    total = 5 * 4096
    TransactionProducer(broker, ProducerConfig(fmt="txb1", batch=4096, seed=5)).produce(total)
    produced = np.concatenate([TxBatch.decode(r.value).features for p in range(2)
                               for r in broker.fetch("odh-demo", p, 0, 1000)])
    assert len(produced) == total
    want = DriftReport.compare(ref, *bin_counts(bins.encode(produced), bins.stamp))
    hub = MetricsHub()
    router = Router(RuleSet.threshold(0.5), ProcessEngine(notification_timeout_s=60), hub.router)
    dm = DeviceModel(fx["model"], gpu, bins=bins)
    ctx = DistContext(0, 1, 0, gpu, "none")
    cfg = EngineServiceConfig(batch=4096, depth=4, streams=2, ring_rows=16384, flush_us=200, reduce_period_ms=1.0,
                              exec_mode="launch")
    with pytest.raises(ValueError, match="persistent"):
        EngineService(ctx, dm, broker, router, EngineServiceConfig(batch=4096, exec_mode="persistent"),
                      drift=DriftMonitor(ref, gpu))
    svc = EngineService(ctx, dm, broker, router, cfg, drift=DriftMonitor(ref, gpu)).start()
    try:
        assert svc.exec_mode == "launch" and svc.native is None
        t0 = time.time()
        while svc.rows_scored < total and time.time() - t0 < 30:
            svc.step()
        svc.reducer.wait()
        assert svc.rows_scored == total
        svc.flush_epochs()
        _, _, extra = svc.metrics_source()
        assert extra["ccfd_gpu_drift_rows_total"] == total and extra["ccfd_gpu_drift_stale_rows_total"] == 0
        psi = np.array([extra["drift_psi"]["feature"][n] for n in want.names])
        assert np.array_equal(psi, want.psi)
        assert extra["drift_features_drifting"] == want.drifting
        reg = CollectorRegistry()
        reg.register(GpuEngineCollector(svc.metrics_source, rank_label="0"))
        text = generate_latest(reg).decode()
        assert f"ccfd_gpu_drift_rows_total {float(total)}" in text and 'ccfd_gpu_drift_psi{feature="V14"}' in text
    finally:
        svc.stop()
