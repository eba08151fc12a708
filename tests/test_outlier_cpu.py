"""models/outlier.py without a GPU: the lane-by-lane emulation of the packed blob against the wire
oracle, round trips, score cells, threshold, report arithmetic, the REST routes through CpuScorer,
the trainer CLI, the metric series, the tap refusals and the preconditions of the GPU fixtures."""
import asyncio
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from ccfd_demo_summit_amd.contracts.transaction import FEATURE_NAMES, WIRE_PERM, decode_wire, encode_wire
from ccfd_demo_summit_amd.models import KINDS, load_model, save_model
from ccfd_demo_summit_amd.models.common import Normalizer
from ccfd_demo_summit_amd.models.mlp import MLPModel
from ccfd_demo_summit_amd.models.outlier import (BLOB_BYTES, OUTLIER_SLOTS, SLOT_FLAGGED, SLOT_HIST, SLOT_INVALID,
                                                 SLOT_ROWS, SLOT_TOP, OutlierAE, OutlierReport, combine_scores,
                                                 emulate_packed_kernel, recount, score_cell, unpack, wire_deviation)
from tests.helpers import outlier_cases as oc

GOLDEN = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def data():
    X, rows = oc.numeric_rows()
    return X, rows


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("log_amount", [True, False])
@pytest.mark.parametrize("latent", [1, 8, 16, 17, 32])
def test_emulated_blob_equals_the_wire_oracle(data, latent, log_amount):
    X, rows = data
    m = oc.numeric_model(X, latent, log_amount)
    edge, bad = oc.edge_case_rows()
    rows = np.concatenate([rows[:23], edge])                   # 47 rows: three tiles, the last one ragged
    score, resid = emulate_packed_kernel(m.pack(), rows)
    want = m.wire_residuals(rows)
    fin = np.isfinite(want).all(1)
    assert np.array_equal(~fin[23:], bad) and fin[:23].all()
    assert np.isnan(resid[~fin]).all() and np.isnan(score[~fin]).all()
    # both accumulate in float64 and round once: equal up to the order of the float64 sums
    assert np.allclose(resid[fin], want[fin], rtol=1e-6, atol=1e-6)
    assert np.array_equal(bits(score[fin]), bits(combine_scores(resid)[fin]))
    assert not resid[fin][:, 30:].any()


@pytest.mark.parametrize("latent", oc.INT_LATENTS)
def test_integer_fixture_is_exact_and_the_emulator_matches_bit_for_bit(latent):
    """The GPU test's precondition: every pre-rounding activation an integer of magnitude <= 256."""
    m = oc.integer_model(latent)
    rows = oc.integer_rows()
    f = m._wire_forward(rows)
    for k in ("a1", "a2", "a3", "res"):
        assert np.array_equal(f[k], np.round(f[k])) and np.abs(f[k]).max() <= 256, k
    assert (m.score_bounds(rows[:1]) >= 0).all()
    score, resid = emulate_packed_kernel(m.pack(), rows[:70])
    assert np.array_equal(bits(resid), bits(m.wire_residuals(rows[:70])))
    assert np.array_equal(bits(score), bits(m.wire_scores(rows[:70])))
    # asymmetric enough: transposing a weight matrix's use or dropping the k-permutation changes the result
    want = m.wire_residuals(rows[:70])
    # k columns 4..7 and 16..19 are the ones pi exchanges
    for name in ("W2", "W4") + (("W3",) if latent > 16 else ()):
        W = {k: getattr(m, k).copy() for k in ("W1", "W2", "W3", "W4")}
        hi = min(20, W[name].shape[1])
        W[name][:, list(range(4, 4 + hi - 16)) + list(range(16, hi))] = \
            W[name][:, list(range(16, hi)) + list(range(4, 4 + hi - 16))]
        swapped = OutlierAE(W["W1"], m.b1, W["W2"], m.b2, W["W3"], m.b3, W["W4"], m.b4, m.norm)
        assert not np.array_equal(swapped.wire_residuals(rows[:70]), want), name
    swapped = OutlierAE(m.W1, m.b1, m.W2, m.b2, m.W3, m.b3, m.W4[::-1].copy(), m.b4, m.norm)      # output rows
    assert not np.array_equal(swapped.wire_residuals(rows[:70]), want)


def test_wire_path_reuses_the_mlp_operands_and_layer_one(data):
    X, rows = data
    norm = Normalizer.fit(X)
    mlp = MLPModel.random_init(3, norm)
    ae = OutlierAE.random_init(8, 3, norm)
    x, finite = ae.wire_inputs(rows[:100])
    assert finite.all() and np.array_equal(x, mlp.wire_inputs(X[:100]))
    assert mlp._wire_w1().shape == (128, 32)
    # the model and what the kernel computes agree to bf16 accuracy (the docstring's figures)
    dev = wire_deviation(ae, X[:2000])
    assert dev["median_rel"] < 1e-3 and dev["max_rel"] < 5e-2
    r = ae.residuals(decode_wire(rows[:50]))
    w = ae.wire_residuals(rows[:50])
    assert np.abs(r[:, WIRE_PERM] - w[:, :30]).max() < 0.05


def test_pack_unpack_and_save_load_round_trip(data, tmp_path):
    X, _ = data
    m = oc.numeric_model(X, 17, True)
    m.threshold = 1.75
    blob = m.pack()
    assert len(blob) == BLOB_BYTES == 21312 and blob[:4] == b"AEW1"
    u = unpack(blob)
    W1p, W2, b2, W3, b3, W4, b4, Th, Tl = m._wire_mats()
    assert u.latent == 17 and u.threshold == 1.75 and u.flags & 1
    for got, want in ((u.W1p, W1p), (u.W2, W2), (u.W3, W3), (u.W4, W4), (u.nTh, -Th), (u.nTl, -Tl), (u.b2, b2),
                      (u.b3, b3), (u.b4, b4)):
        assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(u.mu[:30], m.norm.mu[WIRE_PERM]) and not u.W2[17:].any() and not u.W3[:, 17:].any()
    with pytest.raises(ValueError, match="AEW1"):
        unpack(blob[:-16])
    assert KINDS["ae"] is OutlierAE
    save_model(m, str(tmp_path / "ae.safetensors"))
    back = load_model(str(tmp_path / "ae.safetensors"))
    assert isinstance(back, OutlierAE) and back.latent == 17 and back.threshold == 1.75
    assert back.pack() == blob and all(k.startswith(("ae.", "norm.")) for k in m.state_dict())
    with pytest.raises(ValueError, match="latent"):
        OutlierAE.random_init(33)
    from ccfd_demo_summit_amd.serving.scorers import make_scorer
    with pytest.raises(ValueError, match="no fraud scorer"):
        make_scorer(m, device="cpu")


def test_score_cell_at_the_exponent_edges():
    f = np.float32
    below = np.nextafter(f(2.0 ** -15), f(0))
    cases = [(0.0, 0), (1e-30, 0), (below, 0), (2.0 ** -15, 1), (np.nextafter(f(2.0 ** -14), f(0)), 1), (2.0 ** -14, 2),
             (0.999, 15), (1.0, 16), (1.999, 16), (2.0, 17), (2.0 ** 14, 30), (np.nextafter(f(2.0 ** 15), f(0)), 30),
             (2.0 ** 15, 31), (3e38, 31), (np.float32(1e-45), 0)]
    got = score_cell(np.array([c[0] for c in cases], np.float32))
    assert got.tolist() == [c[1] for c in cases]
    assert score_cell(np.float32(1.0)) == 16


def test_fit_threshold_is_the_quantile_of_the_wire_scores(data):
    X, rows = data
    m = oc.numeric_model(X, 8, True)
    assert m.threshold == float("inf")
    s = m.wire_scores(rows)
    thr = m.fit_threshold(X, 0.99)
    assert thr == m.threshold == float(np.float32(np.quantile(s.astype(np.float64), 0.99)))
    assert int((s > np.float32(thr)).sum()) == 50
    m.fit_threshold(X)
    assert int((s > np.float32(m.threshold)).sum()) == 5
    bad = X.copy()
    bad[:7, 5] = np.nan                                          # non-finite rows take no part
    assert np.isfinite(m.fit_threshold(bad, 0.5))
    with pytest.raises(ValueError, match="quantile"):
        m.fit_threshold(X, 0.0)


def test_report_arithmetic_and_recount(data):
    X, rows = data
    m = oc.numeric_model(X, 8, False)
    rows = rows[:1000].copy()
    rows[:3].view(np.float32).reshape(3, 16)[:, 15] = np.nan     # three invalid rows
    res = m.wire_residuals(rows)
    s = combine_scores(res)
    thr = float(np.nanquantile(s, 0.9))
    c = recount(s, res, thr)
    assert c.shape == (OUTLIER_SLOTS,) and c[SLOT_ROWS] == 1000 and c[SLOT_INVALID] == 3
    assert c[SLOT_FLAGGED] == int((s > np.float32(thr)).sum()) == c[SLOT_TOP:].sum() == 100
    assert c[SLOT_HIST:SLOT_HIST + 32].sum() == 997
    rep = OutlierReport.from_counts(c, thr)
    assert (rep.rows, rep.outliers, rep.invalid) == (1000, 100, 3) and rep.outlier_rate == pytest.approx(100 / 997)
    sq = res[:, :30] ** 2
    flagged = np.flatnonzero(s > np.float32(thr))
    top = np.bincount(WIRE_PERM[np.argmax(sq[flagged], axis=1)], minlength=30)
    assert np.array_equal(rep.top_feature, top)
    js = rep.to_json()
    assert json.loads(json.dumps(js)) == js and js["names"] == list(FEATURE_NAMES) and len(js["histogram"]) == 32
    assert js["worst"][0]["name"] == FEATURE_NAMES[int(np.argmax(top))] and js["threshold"] == thr
    assert OutlierReport.from_counts(np.zeros(OUTLIER_SLOTS, np.uint64)).outlier_rate == 0.0


def test_rest_routes_through_the_cpu_scorer(data):
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.contracts import seldon
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.serving import CpuScorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    X, rows = data
    m = oc.numeric_model(X, 8, True)
    m.fit_threshold(X, 0.99)
    live = X[:300].copy()
    live[7, 3] = np.nan
    want_s, want_sq = m.wire_sq_err(encode_wire(live))
    scorer = CpuScorer(build_model("mlp", seed=0))
    plain = scorer.score(X[:300])

    async def go():
        async with TestClient(TestServer(SeldonServer(scorer).app)) as cl:
            for path in ("/outlier", "/api/v0.1/outlier", "/api/v1.0/outlier"):
                assert (await cl.get(path)).status == 400
                assert (await cl.post(path, json=seldon.build_request(live))).status == 400
            scorer.set_outlier(m)
            r = await cl.post("/api/v1.0/outlier", json=seldon.build_request(np.nan_to_num(live)))
            assert r.status == 200
            body = json.loads((await r.text()).replace("NaN", "null"))
            score, flag, thr, tops = seldon.parse_outlier_response(body)
            clean_s, clean_sq = m.wire_sq_err(encode_wire(np.nan_to_num(live)))
            assert np.array_equal(score, clean_s) and thr == m.threshold
            assert np.array_equal(flag, clean_s > np.float32(m.threshold))
            assert tops[0][0]["name"] == FEATURE_NAMES[int(np.argmax(clean_sq[0]))] and len(tops[0]) == 3
            assert (await cl.post("/outlier", json={"data": {"ndarray": [[1.0, 2.0]]}})).status == 400
            for lo in range(0, 300, 100):
                assert (await cl.post("/api/v0.1/predictions", json=seldon.build_request(X[lo:lo + 100]))).status == 200
            js = await (await cl.get("/api/v0.1/outlier")).json()
            assert js["rows"] == 600 and js["invalid"] == 0 and js["threshold"] == m.threshold
            r = await cl.post("/outlier", json={"reset": True})
            assert (await r.json())["rows"] == 600
            assert (await (await cl.get("/outlier")).json())["rows"] == 0
    asyncio.new_event_loop().run_until_complete(go())
    # the codec with a non-finite row: null score, never an outlier
    s, f, sq = scorer.outlier(live)
    assert np.array_equal(bits(s), bits(want_s)) and np.isnan(s[7]) and not f[7] and np.array_equal(bits(sq), bits(want_sq))
    body = json.dumps(seldon.build_outlier_response(s, f, sq, m.threshold))
    assert "NaN" not in body and json.loads(body)["data"]["ndarray"][7] == [None, 0]
    assert scorer.outlier_report().invalid == 1
    got = scorer.score(X[:300])                                  # the detector changes no fraud score
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    scorer.set_outlier(None)
    with pytest.raises(ValueError, match="no outlier model"):
        scorer.outlier(live)
    with pytest.raises(ValueError, match="kind 'ae'"):
        scorer.set_outlier(build_model("mlp", seed=0))


def test_train_cli_writes_a_detector_that_separates_a_far_cluster(tmp_path):
    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.train.__main__ import main
    out, ae_out = tmp_path / "lr.safetensors", tmp_path / "ae.safetensors"
    rc = main(["--model", "lr", "--rows", "4000", "--epochs", "30", "--batch", "256", "--device", "cpu", "--fraud-rate",
               "0.02", "--out", str(out), "--outlier-out", str(ae_out), "--outlier-latent", "6",
               "--outlier-quantile", "0.99"])
    assert rc == 0 and load_model(str(out)).kind == "lr"
    ae = load_model(str(ae_out))
    assert ae.kind == "ae" and ae.latent == 6 and np.isfinite(ae.threshold)
    X, _ = generate(2000, seed=99, fraud_rate=0.0)
    far = X[:200].copy()
    far[:, 1:29] += 6.0 * X[:, 1:29].std(0)                      # the planted cluster: six sigma off in every V
    s_in = ae.wire_scores(encode_wire(X))
    s_far = ae.wire_scores(encode_wire(far))
    assert s_far.min() > s_in.max() and (s_far > ae.threshold).all()
    assert (s_in > ae.threshold).mean() < 0.05


def _exposition(extra):
    from prometheus_client import CollectorRegistry, generate_latest

    from ccfd_demo_summit_amd.metrics.exporter import GpuEngineCollector
    c = np.zeros(64, np.int64)                                   # tests/test_shadow_cpu.py::_counters
    c[0], c[1], c[2], c[3], c[4] = 14288, 122, 14166, 7_100_000_000, 0
    c[8:22] = np.arange(14) * 7 + 3
    c[24:38] = np.arange(14)
    lat = np.zeros(256, np.int64)
    lat[60:64] = [5, 9, 3, 1]
    reg = CollectorRegistry()
    reg.register(GpuEngineCollector(lambda: (c, lat, extra), rank_label="0"))
    return generate_latest(reg).decode()


def test_exposition_is_unchanged_without_a_monitor_and_carries_the_series_with_one():
    from ccfd_demo_summit_amd.launch.engine_service import outlier_series
    base_extra = {"tx_per_second": 8.5e8, "handoff_dead_letter_total": 2}
    base = _exposition(dict(base_extra))
    assert "outlier" not in base and base == (GOLDEN / "shadow_exposition_baseline.txt").read_text()
    hist = np.zeros(32, np.int64)
    hist[[14, 15, 16, 20]] = [100, 700, 190, 7]
    top = np.zeros(30, np.int64)
    top[[0, 14, 29]] = [1, 4, 2]
    rep = OutlierReport(1000, 7, 3, hist, top, 4.0)
    text = _exposition({**base_extra, **outlier_series(rep)})
    for line in ("ccfd_gpu_outlier_rows_total 1000.0", "ccfd_gpu_outlier_flagged_total 7.0",
                 "ccfd_gpu_outlier_invalid_rows_total 3.0", 'ccfd_gpu_outlier_score_bucket{le="0.5"} 100.0',
                 'ccfd_gpu_outlier_score_bucket{le="2.0"} 990.0', 'ccfd_gpu_outlier_score_bucket{le="+Inf"} 997.0',
                 'ccfd_gpu_outlier_top_feature_total{feature="V14"} 4.0',
                 'ccfd_gpu_outlier_top_feature_total{feature="Amount"} 2.0'):
        assert line in text, line
    assert f"ccfd_gpu_outlier_rate {7 / 997}" in text
    assert "".join(l for l in text.splitlines(keepends=True) if "outlier" not in l) == base


def test_check_outlier_tap_refusals():
    from ccfd_demo_summit_amd.launch.engine_service import check_drift_tap, check_outlier_tap
    mon = object()
    w64 = SimpleNamespace(row_format="w64")
    check_outlier_tap(mon, w64, "launch", False)
    with pytest.raises(ValueError, match="native Kafka consumer"):
        check_outlier_tap(mon, w64, "launch", True)
    for fmt in ("f32", "g32", "g20"):
        with pytest.raises(ValueError, match=f"rows are {fmt}"):
            check_outlier_tap(mon, SimpleNamespace(row_format=fmt), "launch", False)
    with pytest.raises(ValueError, match="exec_mode is 'persistent'"):
        check_outlier_tap(mon, w64, "persistent", False)
    with pytest.raises(ValueError, match="drift monitor: the native Kafka consumer"):      # as it was
        check_drift_tap(mon, w64, "launch", True)


@pytest.mark.parametrize("case", oc.NUMERIC_CASES + [(16, True)])
def test_numeric_fixture_has_a_stable_subset_and_sane_bounds(data, case):
    """The condition of the GPU numerics test: at least 5 % of the 5000 rows are stable, and there
    the bound is the last layer's accumulation term, orders below the residuals."""
    X, rows = data
    m = oc.numeric_model(X, *case)
    st = m.stable_rows(rows)
    assert st.sum() >= 250, st.sum()
    every, stable = m.residual_bounds(rows), m.residual_bounds(rows, stable=True)
    res = m.wire_residuals(rows)
    assert (stable <= every).all() and not every[:, 30:].any()
    assert 1e-6 < stable[:, :30].max() < 1e-3 and np.sqrt((res[:, :30] ** 2).mean()) > 0.3
    edge, bad = oc.edge_case_rows()
    assert np.array_equal(m.stable_rows(edge) | bad, ~bad) or not m.stable_rows(edge)[bad].any()
