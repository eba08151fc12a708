"""csrc/kernels/drift_wire.hip against the numpy oracle (models/drift.py wire_bin_counts): integer
counts, so every comparison is for equality.  Then DriftMonitor with a W64 reference,
GpuScorer(mlp).set_drift behind the REST routes, and EngineService(drift=) on W64 rows."""
import asyncio
import time

import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.contracts.transaction import AMOUNT_COL, TIME_COL, encode_wire
from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models.drift import DriftReference, DriftReport, wire_bin_counts, wire_bins, wire_bins_fit

pytestmark = pytest.mark.gpu

# around a 16-row tile, a wave, a workgroup and the 1 024-rows-per-workgroup grid rule
SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 257, 1025, 5000)
EDGES = np.array([-1.0, 0.0, 0.5, 2.0], np.float32)     # every value a bf16


@pytest.fixture(scope="module")
def fx(gpu):
    X, _ = generate(40_000, seed=7)
    bins = wire_bins_fit(X[0::2])
    host = encode_wire(X[:5000])
    return {"X": X, "bins": bins, "host": host, "dev": torch.from_numpy(host).to(gpu),
            "want": {n: wire_bin_counts(host[:n], bins) for n in SIZES}}


def same(got, want) -> bool:
    counts, tail = got
    assert counts.dtype == torch.uint64 and tail.dtype == torch.uint64
    return torch.equal(counts.cpu(), torch.from_numpy(want[0])) and torch.equal(tail.cpu(), torch.from_numpy(want[1]))


def edge_case_rows():
    """W64 rows poked bit by bit (every other feature 0.25): on an edge, one step above it on the
    bf16 / f32 grid, NaN, +-inf, +-0 and the smallest denormals, in a bf16 column and in the two
    f32 ones."""
    cases = []
    for j in (3, TIME_COL, AMOUNT_COL):
        wide = j in (TIME_COL, AMOUNT_COL)
        sh = 0 if wide else 16
        on = int(np.float32(0.5).view(np.uint32)) >> sh
        up = int(np.nextafter(np.float32(0.5), np.float32(np.inf)).view(np.uint32)) if wide else on + 1
        cases += [(j, b) for b in (on, up, 0x7FC00000 >> sh, 0xFFC00000 >> sh, 0x7F800000 >> sh, 0xFF800000 >> sh,
                                   0x80000000 >> sh, 0, 1, (0x80000000 >> sh) + 1)]
    rows = encode_wire(np.full((len(cases), 30), 0.25, np.float32))
    for r, (j, bits) in enumerate(cases):
        if j in (TIME_COL, AMOUNT_COL):
            rows[r].view(np.uint32)[14 if j == TIME_COL else 15] = bits
        else:
            rows[r].view(np.uint16)[j - 1] = bits
    return rows


@pytest.mark.parametrize("max_workgroups", [1, 512])
def test_drift_histogram_wire_equals_the_oracle(fx, max_workgroups):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram_wire
    for n in SIZES:
        got = drift_histogram_wire(fx["dev"][:n], fx["bins"], max_workgroups=max_workgroups)
        assert same(got, fx["want"][n]), n


def test_edge_values_land_where_the_oracle_puts_them(fx, gpu):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram_wire
    cases = edge_case_rows()
    host = np.ascontiguousarray(np.tile(cases, (257 // len(cases) + 1, 1))[:257])
    table = [EDGES] * 30
    want = wire_bin_counts(host, table)
    # the oracle itself, on the cases a kernel gets wrong: on-edge / next-above, NaN, -0, denormals
    one = wire_bin_counts(cases[:10], table)[0][3]
    assert one[:5].tolist() == [3, 3, 2, 1, 1]
    assert same(drift_histogram_wire(torch.from_numpy(host).to(gpu), table), want)


def test_ragged_tables_never_count_the_padding(fx, gpu):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram_wire
    full = fx["bins"].edges
    edges = [e.copy() for e in full]
    edges[0] = full[0][:0]                       # Time: no edge, everything in cell 0
    edges[1] = full[1][15:16]
    edges[2] = full[2][10:21:10]
    edges[28] = full[28][:30]
    edges[29] = full[29][:0]                     # Amount: no edge
    bins = wire_bins(edges)
    host = fx["host"].copy()
    host[:8].view(np.float32).reshape(8, 16)[:, 14:] = np.inf          # +inf against an all-padding column
    want = wire_bin_counts(host, bins)
    got = drift_histogram_wire(torch.from_numpy(host).to(gpu), bins)
    assert same(got, want)
    c = got[0].cpu().numpy()
    for j in range(30):
        assert c[j, edges[j].size + 1:].sum() == 0 and c[j].sum() == 5000
    assert c[0, 0] == 5000 and c[29, 0] == 5000


def test_worst_contention_identical_rows(fx, gpu):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram_wire
    host = np.repeat(fx["host"][:1], 4096, axis=0)
    counts, tail = drift_histogram_wire(torch.from_numpy(host).to(gpu), fx["bins"])
    assert same((counts, tail), wire_bin_counts(host, fx["bins"]))
    c = counts.cpu().numpy()
    assert ((c != 0).sum(1) == 1).all() and (c.max(1) == 4096).all() and tail.cpu().tolist() == [4096, 0]


def test_accumulates_skips_empty_and_ignores_the_grid(fx):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram_wire, drift_wire_table, new_drift_counts
    rows = fx["dev"][:5000]
    table = drift_wire_table(fx["bins"], rows.device)
    assert drift_wire_table(fx["bins"], rows.device) is table              # uploaded once per table
    counts, tail = new_drift_counts(rows.device)
    for _ in range(2):
        out = drift_histogram_wire(rows, table, counts, tail)
        assert out[0] is counts and out[1] is tail
    want = fx["want"][5000]
    assert same((counts, tail), (2 * want[0], 2 * want[1]))
    drift_histogram_wire(rows[:0], table, counts, tail)                    # n = 0 leaves the outputs untouched
    assert same((counts, tail), (2 * want[0], 2 * want[1]))
    for mw in (2, 3, 2048):
        assert same(drift_histogram_wire(rows, fx["bins"], max_workgroups=mw), want), mw


def test_alignment_and_argument_refusals(fx):
    from ccfd_demo_summit_amd.ops.kernels import drift_histogram, drift_histogram_wire, new_drift_counts
    dev = fx["dev"].device
    raw = torch.zeros(257 * 64 + 64, dtype=torch.uint8, device=dev)
    view = raw[16:16 + 257 * 64].view(257, 64)
    view.copy_(fx["dev"][:257])
    assert view.is_contiguous() and view.data_ptr() % 64 == 16
    assert same(drift_histogram_wire(view, fx["bins"]), fx["want"][257])
    counts, tail = new_drift_counts(dev)
    off4 = raw[4:4 + 64 * 64].view(64, 64)
    assert off4.is_contiguous() and off4.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="W64 rows must be 16-byte aligned"):
        drift_histogram_wire(off4, fx["bins"], counts, tail)
    with pytest.raises(RuntimeError, match="max_workgroups < 1"):
        drift_histogram_wire(fx["dev"][:64], fx["bins"], counts, tail, max_workgroups=0)
    with pytest.raises(RuntimeError, match="max_workgroups < 1"):
        drift_histogram_wire(fx["dev"][:64], fx["bins"], counts, tail, max_workgroups=-3)
    with pytest.raises(ValueError, match="uint64"):
        drift_histogram_wire(fx["dev"][:64], fx["bins"], counts.view(torch.int64), tail)
    with pytest.raises(ValueError, match="rows must be"):
        drift_histogram_wire(fx["dev"][:64, :32], fx["bins"])
    with pytest.raises(ValueError, match="edge table"):
        drift_histogram_wire(fx["dev"][:64], torch.zeros(30, 31, device=dev), counts, tail)
    with pytest.raises(ValueError, match="rows must be"):                  # the binned entry point keeps its widths
        drift_histogram(fx["dev"][:64], 5)
    torch.cuda.synchronize()
    assert int(counts.view(torch.int64).sum()) == 0 and int(tail.view(torch.int64).sum()) == 0


def test_null_and_negative_arguments_are_refused_by_the_library(fx):
    import ctypes as C

    from ccfd_demo_summit_amd.ops._lib import DriftWireArgs, lib
    from ccfd_demo_summit_amd.ops.kernels import drift_wire_table, new_drift_counts
    dev = fx["dev"].device
    counts, tail = new_drift_counts(dev)
    table = drift_wire_table(fx["bins"], dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch(**kw):
        a = DriftWireArgs()
        a.rows, a.edges, a.counts, a.tail = fx["dev"].data_ptr(), table.data_ptr(), counts.data_ptr(), tail.data_ptr()
        a.n, a.max_workgroups = 64, 512
        for k, v in kw.items():
            setattr(a, k, v)
        return lib().ccfd_drift_wire_launch(C.byref(a), stream)
    for kw in ({"rows": None}, {"edges": None}, {"counts": None}, {"tail": None}):
        assert launch(**kw) == -1
    assert lib().ccfd_drift_wire_launch(None, stream) == -1
    assert launch(n=-1) == -2
    assert launch(edges=table.data_ptr() + 2) == -3 and launch(counts=counts.data_ptr() + 4) == -3
    assert launch(rows=None, n=0) == 0                                      # nothing to read: no launch
    torch.cuda.synchronize()
    assert int(counts.view(torch.int64).sum()) == 0 and int(tail.view(torch.int64).sum()) == 0


def test_drift_monitor_with_a_w64_reference(fx, gpu):
    from ccfd_demo_summit_amd.ops.kernels import DriftMonitor
    ref = DriftReference.fit_wire(fx["X"][0::2], bins=fx["bins"])
    live = fx["X"][1::2].copy()
    live[:, 14] += fx["X"][:, 14].std()
    host = encode_wire(np.concatenate([live] * 5)[:3 * 4096 + 70_000])
    counts, tail = wire_bin_counts(host, ref.edges)
    want = DriftReport.compare(ref, counts, tail)
    a, b = DriftMonitor(ref, gpu), DriftMonitor(ref, gpu)
    assert a.fmt == "w64" and a.row_bytes == 64
    with pytest.raises(ValueError, match="w64 rows"):
        a.observe_host(np.zeros((64, 20), np.uint8))
    dev = torch.from_numpy(host).to(gpu)
    side = torch.cuda.Stream(gpu)
    for i in range(3):
        a.observe_host(host[4096 * i:4096 * (i + 1)])
    a.observe_host(host[3 * 4096:])                   # 70 000 rows: crosses a staging buffer
    b.observe(dev[:40_000])
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        b.observe(dev[40_000:])
    for mon in (a, b):
        rep = mon.report()
        assert rep.rows == len(host) and rep.stale == 0
        assert np.array_equal(rep.psi, want.psi) and rep.status == want.status
        assert torch.equal(mon.counts.cpu(), torch.from_numpy(counts))
    assert want.status[14] == "drift" and want.drifting == 1
    assert a.report(reset=True).rows == len(host)
    rep = a.report()
    assert rep.rows == 0 and rep.status == ["insufficient"] * 31
    a.observe_host(host[:12_000])                     # the next window starts from zero
    assert a.report().rows == 12_000
    a.close()
    b.close()


def test_gpu_scorer_mlp_drift_route_equals_the_oracle(fx, gpu):
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.contracts import seldon
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.serving import GpuScorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    ref = DriftReference.fit_wire(fx["X"][0::2], bins=fx["bins"])
    live = fx["X"][1::2][:3000]
    want = DriftReport.compare(ref, *wire_bin_counts(encode_wire(live), ref.edges), min_rows=1000)
    scorer = GpuScorer(build_model("mlp", seed=0))
    plain = scorer.score(live)

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
        got = scorer.score(live)                                           # the monitor changes no score
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
        gb = ObliviousGBDT.random_init(20, 4, 0, fx["X"])
        with pytest.raises(ValueError, match="no drift detector"):
            scorer.set_drift(DriftReference.fit(fx["X"][:2000], gb.bin_spec(bits=5)))
    finally:
        scorer.set_drift(None)
        scorer.close()


def test_engine_service_taps_every_ingested_w64_row(fx, gpu):
    from prometheus_client import CollectorRegistry, generate_latest

    from ccfd_demo_summit_amd.contracts.transaction import TxBatch
    from ccfd_demo_summit_amd.ingest import InProcBroker, ProducerConfig, TransactionProducer
    from ccfd_demo_summit_amd.launch.engine_service import EngineService, EngineServiceConfig
    from ccfd_demo_summit_amd.metrics import MetricsHub
    from ccfd_demo_summit_amd.metrics.exporter import GpuEngineCollector
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, DriftMonitor
    from ccfd_demo_summit_amd.parallel import DistContext
    from ccfd_demo_summit_amd.process import ProcessEngine
    from ccfd_demo_summit_amd.router import Router, RuleSet
    ref = DriftReference.fit_wire(fx["X"][0::2], bins=fx["bins"])
    broker = InProcBroker(default_partitions=2)
    broker.create_topic("odh-demo", 2)
    total = 5 * 4096
    TransactionProducer(broker, ProducerConfig(fmt="txb1", batch=4096, seed=5)).produce(total)
    produced = np.concatenate([TxBatch.decode(r.value).features for p in range(2)
                               for r in broker.fetch("odh-demo", p, 0, 1000)])
    assert len(produced) == total
    want = DriftReport.compare(ref, *wire_bin_counts(encode_wire(produced), ref.edges))
    hub = MetricsHub()
    router = Router(RuleSet.threshold(0.5), ProcessEngine(notification_timeout_s=60), hub.router)
    dm = DeviceModel(build_model("mlp", seed=0), gpu, wire=True)
    assert dm.row_format == "w64"
    ctx = DistContext(0, 1, 0, gpu, "none")
    cfg = EngineServiceConfig(batch=4096, depth=4, streams=2, ring_rows=16384, flush_us=200, reduce_period_ms=1.0,
                              exec_mode="launch")
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
