"""csrc/kernels/outlier_ae.hip against models/outlier.py: bit-exact on the integer model, exact
bookkeeping on real-valued models, the two numerics gates of the wire oracle, edge rows, refusals,
then OutlierMonitor, GpuScorer.set_outlier behind the REST routes and EngineService(outlier=)."""
import asyncio
import ctypes as C
import time

import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.contracts.transaction import WIRE_PERM, encode_wire
from ccfd_demo_summit_amd.models.outlier import (OUTLIER_SLOTS, SLOT_FLAGGED, SLOT_HIST, SLOT_INVALID, SLOT_ROWS,
                                                 SLOT_TOP, OutlierReport, combine_scores, recount)
from tests.helpers import outlier_cases as oc

pytestmark = pytest.mark.gpu

GRIDS = (1, None)            # max_workgroups: one workgroup strides over everything, and the default


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_counts(t):
    return t.view(torch.int64).cpu().numpy().view(np.uint64)


def run(dm, rows, n=None, mw=None, counts=None, threshold=None):
    from ccfd_demo_summit_amd.ops.kernels import OUTLIER_MAX_WORKGROUPS, outlier_scores
    rows = rows if n is None else rows[:n]
    resid = torch.full((rows.shape[0], 32), 7.0, dtype=torch.float32, device=rows.device)
    score = outlier_scores(dm, rows, None, resid, counts, threshold, OUTLIER_MAX_WORKGROUPS if mw is None else mw)
    return score.cpu().numpy(), resid.cpu().numpy()


@pytest.fixture(scope="module")
def ints(gpu):
    from ccfd_demo_summit_amd.ops.kernels import DeviceOutlierModel
    host = oc.integer_rows()
    out = {"host": host, "dev": torch.from_numpy(host).to(gpu), "models": {}}
    for L in oc.INT_LATENTS:
        m = oc.integer_model(L)
        out["models"][L] = (m, DeviceOutlierModel(m, gpu), m.wire_residuals(host), m.wire_scores(host))
    return out


@pytest.fixture(scope="module")
def real(gpu):
    """The numerics cases: model, device model, oracle residuals / scores and both bounds, computed once."""
    from ccfd_demo_summit_amd.ops.kernels import DeviceOutlierModel
    X, host = oc.numeric_rows()
    out = {"X": X, "host": host, "dev": torch.from_numpy(host).to(gpu), "cases": {}}
    for L, la in oc.NUMERIC_CASES:
        m = oc.numeric_model(X, L, la)
        want = m.wire_residuals(host)
        score = combine_scores(want)
        m.threshold = float(np.quantile(score.astype(np.float64), 0.99))
        out["cases"][(L, la)] = dict(model=m, dm=DeviceOutlierModel(m, gpu), resid=want, score=score,
                                     bound=m.residual_bounds(host), sbound=m.residual_bounds(host, stable=True),
                                     stable=m.stable_rows(host), score_bound=m.score_bounds(host))
    return out


# ------------------------------------------------------------------ 1. integer model, exact
@pytest.mark.parametrize("latent", oc.INT_LATENTS)
@pytest.mark.parametrize("mw", GRIDS)
def test_integer_model_equals_the_oracle_bit_for_bit(ints, latent, mw):
    m, dm, want_r, want_s = ints["models"][latent]
    for n in oc.SIZES:
        score, resid = run(dm, ints["dev"], n, mw)
        assert np.array_equal(bits(resid), bits(want_r[:n])), (latent, n)
        assert np.array_equal(bits(score), bits(want_s[:n])), (latent, n)
    assert np.abs(want_r).max() > 4 and len(np.unique(want_s)) > 100       # the fixture is no constant


# ------------------------------------------------------------------ 2. bookkeeping, exact
@pytest.mark.parametrize("case", oc.NUMERIC_CASES[:2])
def test_scores_counts_and_rows_are_exact_functions_of_the_residuals(real, case):
    from ccfd_demo_summit_amd.ops.kernels import new_outlier_counts, outlier_scores
    c = real["cases"][case]
    dm, thr = c["dm"], c["model"].threshold
    dev = real["dev"]
    want_counts = {}
    for mw in GRIDS:
        for n in oc.SIZES:
            counts = new_outlier_counts(dev.device)
            score, resid = run(dm, dev, n, mw, counts)
            assert np.array_equal(bits(score), bits(combine_scores(resid))), n
            assert not resid[:, 30:].any()
            got = host_counts(counts)
            assert np.array_equal(got, recount(score, resid, thr)), n
            assert np.array_equal(got, want_counts.setdefault(n, got)), n            # whatever the grid
    full_s, full_r = run(dm, dev)
    full = recount(full_s, full_r, thr)
    assert full[SLOT_FLAGGED] > 10 and full[SLOT_ROWS] == 5000 and full[SLOT_TOP:].sum() == full[SLOT_FLAGGED]
    # accumulates over two launches, n = 0 leaves the counts alone, an explicit threshold is used
    counts = new_outlier_counts(dev.device)
    for _ in range(2):
        outlier_scores(dm, dev, counts=counts)
    outlier_scores(dm, dev[:0], counts=counts)
    assert np.array_equal(host_counts(counts), 2 * full)
    counts = new_outlier_counts(dev.device)
    low = float(np.median(full_s))
    outlier_scores(dm, dev, counts=counts, threshold=low)
    assert np.array_equal(host_counts(counts), recount(full_s, full_r, low))
    # a row alone, or at any position of any batch, gets identical bits
    for i in (0, 1, 15, 16, 31, 33, 100, 4999):
        s1, r1 = run(dm, dev[i:i + 1])
        assert bits(s1)[0] == bits(full_s)[i] and np.array_equal(bits(r1)[0], bits(full_r)[i])
    perm = np.random.default_rng(0).permutation(5000)[:777]
    s2, r2 = run(dm, torch.from_numpy(real["host"][perm]).to(dev.device))
    assert np.array_equal(bits(s2), bits(full_s[perm])) and np.array_equal(bits(r2), bits(full_r[perm]))


def test_top_feature_takes_the_lowest_position_on_a_tie(ints):
    """Integer residuals tie often: the kernel's top-feature cells equal the host recount's
    (argmax of the squares, first position) on thousands of flagged rows."""
    from ccfd_demo_summit_amd.ops.kernels import new_outlier_counts
    m, dm, want_r, want_s = ints["models"][16]
    thr = float(np.median(want_s))
    counts = new_outlier_counts(ints["dev"].device)
    score, resid = run(dm, ints["dev"], counts=counts, threshold=thr)
    sq = want_r[:, :30] ** 2
    ties = int(((sq == sq.max(1, keepdims=True)).sum(1) > 1).sum())
    assert ties > 100
    got = host_counts(counts)
    assert np.array_equal(got, recount(want_s, want_r, thr)) and got[SLOT_FLAGGED] > 1000


# ------------------------------------------------------------------ 3. numerics
@pytest.mark.parametrize("case", oc.NUMERIC_CASES)
def test_residuals_are_within_the_bounds_of_the_wire_oracle(real, case):
    """Measured on an MI355X (max error, max error / bound): docs/OUTLIER.md."""
    c = real["cases"][case]
    score, resid = run(c["dm"], real["dev"])
    err = np.abs(resid.astype(np.float64) - c["resid"].astype(np.float64))
    st = c["stable"]
    every = (err / c["bound"])[:, :30].max()
    stable = (err[st] / c["sbound"][st])[:, :30].max()
    print(f"outlier numerics latent={case[0]} log_amount={case[1]}: every row max err {err.max():.3e} "
          f"ratio {every:.3e}; stable rows {int(st.sum())} max err {err[st].max():.3e} ratio {stable:.3e}")
    assert st.sum() >= 250                                      # the condition: 5 % of the rows
    assert (err <= c["bound"]).all()
    assert (err[st] <= c["sbound"][st]).all()
    # flagged set at the oracle's 0.99 quantile, except rows within their own score bound of it
    thr = c["model"].threshold
    near = np.abs(c["score"].astype(np.float64) - thr) <= c["score_bound"]
    assert np.array_equal((score > np.float32(thr))[~near], (c["score"] > np.float32(thr))[~near])
    assert near.sum() < 2500 and (c["score"] > np.float32(thr)).sum() == 50
    assert (np.abs(score.astype(np.float64) - c["score"]) <= c["score_bound"]).all()


# ------------------------------------------------------------------ 4. edge rows
def test_non_finite_rows_score_nan_and_touch_no_neighbour(real, gpu):
    from ccfd_demo_summit_amd.ops.kernels import new_outlier_counts
    c = real["cases"][(8, True)]
    m, dm = c["model"], c["dm"]
    edge, bad = oc.edge_case_rows()
    host = real["host"][:64].copy()
    at = np.array([0, 3, 15, 16, 17, 31, 32, 33, 40, 41, 42, 43, 47, 48, 49, 50, 51, 55, 60, 61, 62, 63, 5, 7])
    clean_s, clean_r = run(dm, torch.from_numpy(host).to(gpu))
    host[at] = edge
    counts = new_outlier_counts(gpu)
    score, resid = run(dm, torch.from_numpy(host).to(gpu), counts=counts)
    nonfinite = np.zeros(64, bool)
    nonfinite[at] = bad
    assert np.isnan(score[nonfinite]).all() and np.isnan(resid[nonfinite]).all()
    assert np.isfinite(score[~nonfinite]).all() and np.isfinite(resid[~nonfinite]).all()
    untouched = np.setdiff1d(np.arange(64), at)
    assert np.array_equal(bits(score[untouched]), bits(clean_s[untouched]))
    assert np.array_equal(bits(resid[untouched]), bits(clean_r[untouched]))
    # +-0 and denormal rows: finite, and within the every-row bound of the oracle
    want = m.wire_residuals(host)
    assert np.array_equal(np.isnan(want).all(1), nonfinite) and np.array_equal(np.isnan(want).any(1), nonfinite)
    ok = ~nonfinite
    assert (np.abs(resid[ok].astype(np.float64) - want[ok]) <= m.residual_bounds(host)[ok]).all()
    got = host_counts(counts)
    assert got[SLOT_INVALID] == nonfinite.sum() == 12 and got[SLOT_ROWS] == 64
    assert got[SLOT_HIST:SLOT_HIST + 32].sum() == 64 - 12
    assert np.array_equal(got, recount(score, resid, m.threshold))
    assert got[SLOT_FLAGGED] == int((score > np.float32(m.threshold)).sum())        # NaN is not flagged


# ------------------------------------------------------------------ 5. refusals
def test_alignment_and_argument_refusals(real):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_outlier_counts, outlier_scores
    c = real["cases"][(8, True)]
    dm, dev = c["dm"], real["dev"]
    full_s, _ = run(dm, dev, 257)
    raw = torch.zeros(257 * 64 + 64, dtype=torch.uint8, device=dev.device)
    view = raw[16:16 + 257 * 64].view(257, 64)
    view.copy_(dev[:257])
    assert view.is_contiguous() and view.data_ptr() % 64 == 16
    assert np.array_equal(bits(outlier_scores(dm, view)), bits(full_s))
    counts = new_outlier_counts(dev.device)
    out = torch.full((64,), 5.0, device=dev.device)
    resid = torch.full((64, 32), 5.0, device=dev.device)
    off4 = raw[4:4 + 64 * 64].view(64, 64)
    assert off4.is_contiguous() and off4.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="W64 rows must be 16-byte aligned"):
        outlier_scores(dm, off4, out, resid, counts)
    for mw in (0, -3):
        with pytest.raises(RuntimeError, match="max_workgroups < 1"):
            outlier_scores(dm, dev[:64], out, resid, counts, max_workgroups=mw)
    with pytest.raises(ValueError, match="uint64"):
        outlier_scores(dm, dev[:64], out, resid, counts.view(torch.int64))
    with pytest.raises(ValueError, match="rows must be"):
        outlier_scores(dm, dev[:64, :32], out)
    with pytest.raises(ValueError, match="rows must be"):
        outlier_scores(dm, dev[:64].view(torch.int8), out)
    with pytest.raises(ValueError, match="out must be"):
        outlier_scores(dm, dev[:64], out[:63])
    with pytest.raises(ValueError, match="out must be"):
        outlier_scores(dm, dev[:64], out.double())
    with pytest.raises(ValueError, match="resid_out must be"):
        outlier_scores(dm, dev[:64], out, resid[:, :30])
    with pytest.raises(ValueError, match="DeviceOutlierModel"):
        outlier_scores(c["model"], dev[:64], out)
    with pytest.raises(ValueError, match="no device kernel"):
        DeviceModel(c["model"], dev.device)                                  # it is no fraud scorer
    torch.cuda.synchronize()
    assert int(counts.view(torch.int64).sum()) == 0 and bool((out == 5).all()) and bool((resid == 5).all())


def test_null_negative_misaligned_and_truncated_are_refused_by_the_library(real):
    from ccfd_demo_summit_amd.ops._lib import OutlierArgs, lib
    from ccfd_demo_summit_amd.ops.kernels import new_outlier_counts
    c = real["cases"][(8, True)]
    dm, dev = c["dm"], real["dev"]
    counts = new_outlier_counts(dev.device)
    out = torch.full((64,), 5.0, device=dev.device)
    resid = torch.full((64, 32), 5.0, device=dev.device)
    stream = C.c_void_p(torch.cuda.current_stream(dev.device).cuda_stream)

    def launch(**kw):
        a = OutlierArgs()
        a.rows, a.blob, a.score, a.resid_out, a.counts = (dev.data_ptr(), dm.blob.data_ptr(), out.data_ptr(),
                                                          resid.data_ptr(), counts.data_ptr())
        a.n, a.blob_bytes, a.latent, a.magic, a.max_workgroups = 64, dm.blob.numel(), dm.latent, dm.magic, 512
        for k, v in kw.items():
            setattr(a, k, v)
        return lib().ccfd_outlier_ae_launch(C.byref(a), stream)
    for kw in ({"rows": None}, {"blob": None}, {"score": None}):
        assert launch(**kw) == -1
    assert lib().ccfd_outlier_ae_launch(None, stream) == -1
    assert launch(n=-1) == -2 and launch(max_workgroups=0) == -2
    assert launch(rows=dev.data_ptr() + 4) == -3 and launch(blob=dm.blob.data_ptr() + 8) == -3
    assert launch(score=out.data_ptr() + 2) == -3 and launch(resid_out=resid.data_ptr() + 4) == -3
    assert launch(counts=counts.data_ptr() + 4) == -3
    assert launch(blob_bytes=dm.blob.numel() - 16) == -4                       # a truncated blob
    assert launch(magic=0x3150_4C4D) == -4 and launch(latent=0) == -4 and launch(latent=33) == -4
    assert launch(rows=None, n=0) == 0                                         # nothing to read: no launch
    torch.cuda.synchronize()
    assert int(counts.view(torch.int64).sum()) == 0 and bool((out == 5).all()) and bool((resid == 5).all())


# ------------------------------------------------------------------ 6. monitor
def test_outlier_monitor_equals_the_recount_of_outlier_scores(real, gpu):
    from ccfd_demo_summit_amd.ops.kernels import OutlierMonitor
    c = real["cases"][(8, True)]
    m, dm = c["model"], c["dm"]
    host = np.concatenate([real["host"]] * 17)[:3 * 4096 + 70_000]
    dev = torch.from_numpy(host).to(gpu)
    score, resid = run(dm, dev)
    want = recount(score, resid, m.threshold)
    a, b = OutlierMonitor(m, gpu), OutlierMonitor(dm, gpu, max_workgroups=64)
    with pytest.raises(ValueError, match="W64 rows"):
        a.observe_host(np.zeros((64, 20), np.uint8))
    side = torch.cuda.Stream(gpu)
    for i in range(3):
        a.observe_host(host[4096 * i:4096 * (i + 1)])
    a.observe_host(host[3 * 4096:])                   # 70 000 rows: crosses a staging buffer
    got = b.observe(dev[:40_000])
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        b.observe(dev[40_000:])
    assert np.array_equal(bits(got), bits(score[:40_000]))
    for mon in (a, b):
        rep = mon.report()
        assert isinstance(rep, OutlierReport) and rep.rows == len(host) and rep.invalid == 0
        assert np.array_equal(host_counts(mon.counts), want)
        assert rep.outliers == want[SLOT_FLAGGED] > 0 and rep.threshold == pytest.approx(m.threshold)
        assert np.array_equal(rep.histogram, want[SLOT_HIST:SLOT_HIST + 32].astype(np.int64))
        assert np.array_equal(rep.top_feature, want[SLOT_TOP:].astype(np.int64))
    assert a.report(reset=True).rows == len(host)
    assert a.report().rows == 0 and a.report().outliers == 0
    a.observe_host(host[:12_000])                     # the next window starts from zero
    assert a.report().rows == 12_000
    a.close()
    b.close()
    assert a._stage == [] and b._stage == []


# ------------------------------------------------------------------ 7. serving
def test_gpu_scorer_outlier_routes_equal_outlier_scores(real, gpu):
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.contracts import seldon
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.serving import GpuScorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    c = real["cases"][(8, True)]
    m, dm = c["model"], c["dm"]
    live = real["X"][:3000]
    want_s, want_r = run(dm, real["dev"], 3000)
    want_sq = np.empty((3000, 30), np.float32)
    want_sq[:, WIRE_PERM] = want_r[:, :30] * want_r[:, :30]
    scorer = GpuScorer(build_model("mlp", seed=0))
    plain = scorer.score(live)

    async def go():
        async with TestClient(TestServer(SeldonServer(scorer).app)) as cl:
            assert (await cl.get("/outlier")).status == 400
            assert (await cl.post("/api/v1.0/outlier", json=seldon.build_request(live[:10]))).status == 400
            scorer.set_outlier(m)
            r = await cl.post("/outlier", json=seldon.build_request(live[:500]))
            assert r.status == 200
            score, flag, thr, tops = seldon.parse_outlier_response(await r.json())
            assert np.array_equal(bits(score), bits(want_s[:500])) and thr == pytest.approx(m.threshold)
            assert np.array_equal(flag, want_s[:500] > np.float32(m.threshold))
            from ccfd_demo_summit_amd.contracts.transaction import FEATURE_NAMES
            assert [t[0]["name"] for t in tops] == [FEATURE_NAMES[j] for j in np.argmax(want_sq[:500], axis=1)]
            assert (await (await cl.post("/outlier", json={"reset": True})).json())["rows"] == 500
            for lo in range(0, 3000, 1000):
                r = await cl.post("/api/v0.1/predictions", json=seldon.build_request(live[lo:lo + 1000]))
                assert r.status == 200
            js = await (await cl.get("/api/v1.0/outlier")).json()
            want = OutlierReport.from_counts(recount(want_s, want_r, m.threshold), m.threshold).to_json()
            assert js["rows"] == 3000 and js == want
    try:
        asyncio.new_event_loop().run_until_complete(go())
        s, f, sq = scorer.outlier(live, count=False)
        assert np.array_equal(bits(s), bits(want_s)) and np.array_equal(bits(sq), bits(want_sq))
        got = scorer.score(live)                                           # the detector changes no fraud score
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        with pytest.raises(ValueError, match="kind 'ae'"):
            scorer.set_outlier(build_model("mlp", seed=0))
    finally:
        scorer.set_outlier(None)
        scorer.close()


# ------------------------------------------------------------------ 8. engine
def test_engine_service_taps_every_ingested_row_for_outlier_and_drift(real, gpu):
    from prometheus_client import CollectorRegistry, generate_latest

    from ccfd_demo_summit_amd.contracts.transaction import FEATURE_NAMES, TxBatch
    from ccfd_demo_summit_amd.ingest import InProcBroker, ProducerConfig, TransactionProducer
    from ccfd_demo_summit_amd.launch.engine_service import EngineService, EngineServiceConfig
    from ccfd_demo_summit_amd.metrics import MetricsHub
    from ccfd_demo_summit_amd.metrics.exporter import GpuEngineCollector
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.models.drift import DriftReference, DriftReport, wire_bin_counts
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, DriftMonitor, OutlierMonitor
    from ccfd_demo_summit_amd.parallel import DistContext
    from ccfd_demo_summit_amd.process import ProcessEngine
    from ccfd_demo_summit_amd.router import Router, RuleSet
    c = real["cases"][(8, True)]
    m, dm_out = c["model"], c["dm"]
    ref = DriftReference.fit_wire(real["X"])
    broker = InProcBroker(default_partitions=2)
    broker.create_topic("odh-demo", 2)
    total = 5 * 4096
    TransactionProducer(broker, ProducerConfig(fmt="txb1", batch=4096, seed=5)).produce(total)
    produced = np.concatenate([TxBatch.decode(r.value).features for p in range(2)
                               for r in broker.fetch("odh-demo", p, 0, 1000)])
    assert len(produced) == total
    host = encode_wire(produced)
    want_s, want_r = run(dm_out, torch.from_numpy(host).to(gpu))
    want = recount(want_s, want_r, m.threshold)
    want_drift = DriftReport.compare(ref, *wire_bin_counts(host, ref.edges))
    hub = MetricsHub()
    router = Router(RuleSet.threshold(0.5), ProcessEngine(notification_timeout_s=60), hub.router)
    dm = DeviceModel(build_model("mlp", seed=0), gpu, wire=True)
    ctx = DistContext(0, 1, 0, gpu, "none")
    cfg = EngineServiceConfig(batch=4096, depth=4, streams=2, ring_rows=16384, flush_us=200, reduce_period_ms=1.0,
                              exec_mode="launch")
    svc = EngineService(ctx, dm, broker, router, cfg, drift=DriftMonitor(ref, gpu),
                        outlier=OutlierMonitor(m, gpu)).start()
    try:
        assert svc.exec_mode == "launch" and svc.native is None
        t0 = time.time()
        while svc.rows_scored < total and time.time() - t0 < 30:
            svc.step()
        svc.reducer.wait()
        assert svc.rows_scored == total
        svc.flush_epochs()
        _, _, extra = svc.metrics_source()
        assert extra["ccfd_gpu_outlier_rows_total"] == total == want[SLOT_ROWS]
        assert extra["ccfd_gpu_outlier_flagged_total"] == want[SLOT_FLAGGED] > 0
        assert extra["ccfd_gpu_outlier_invalid_rows_total"] == 0
        tops = extra["outlier_top_feature_total"]["feature"]
        assert [tops[n] for n in FEATURE_NAMES] == want[SLOT_TOP:].tolist()
        assert extra["outlier_score_bucket"]["le"]["+Inf"] == total
        assert extra["outlier_rate"] == want[SLOT_FLAGGED] / total
        # drift beside it, from the same tap
        assert extra["ccfd_gpu_drift_rows_total"] == total
        psi = np.array([extra["drift_psi"]["feature"][n] for n in want_drift.names])
        assert np.array_equal(psi, want_drift.psi)
        reg = CollectorRegistry()
        reg.register(GpuEngineCollector(svc.metrics_source, rank_label="0"))
        text = generate_latest(reg).decode()
        assert f"ccfd_gpu_outlier_rows_total {float(total)}" in text
        assert f"ccfd_gpu_outlier_flagged_total {float(want[SLOT_FLAGGED])}" in text
        assert 'ccfd_gpu_outlier_top_feature_total{feature="V14"}' in text and "ccfd_gpu_outlier_rate " in text
        assert 'ccfd_gpu_outlier_score_bucket{le="+Inf"}' in text and "ccfd_gpu_drift_rows_total" in text
    finally:
        svc.stop()
