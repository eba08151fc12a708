"""CPU side of feature-drift detection (docs/DRIFT.md): the bin-count oracle, PSI, the
reference file, the report, the CpuScorer / SeldonServer surface and the ring tap."""
import asyncio
import ctypes as C

import numpy as np
import pytest

from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.contracts import seldon
from ccfd_demo_summit_amd.contracts.transaction import FEATURE_NAMES, decode_g20_bins
from ccfd_demo_summit_amd.models.drift import (COLUMN_NAMES, N_CELLS, N_COLS, DriftReference, DriftReport, bin_counts,
                                               n_bins_of, psi)
from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT

SHIFTED = 14       # feature index of V14: the 100 x 6 ensemble below has 20 edges on it (>= 4 asserted)


@pytest.fixture(scope="module")
def fx():
    """40 000 synthetic rows against the table of a random 100 x 6 ensemble.  The halves are
    the even and the odd rows: synthetic Time grows with the row index, so a first half /
    second half split is a real drift of Time (PSI ~14) and not a no-drift case."""
    X, _ = generate(40_000, seed=7)
    model = ObliviousGBDT.random_init(100, 6, 0, X)
    return {"X": X, "model": model, "g32": model.bin_spec(), "g20": model.bin_spec(bits=5),
            "ref_half": X[0::2], "live_half": X[1::2]}


def test_bin_counts_g32_equals_a_loop(fx):
    rows = fx["g32"].encode(fx["X"][:700])
    stamp = fx["g32"].stamp
    want = np.zeros((N_COLS, N_CELLS), np.uint64)
    for r in rows:
        for j in range(N_COLS):
            want[j, r[j]] += 1
    counts, tail = bin_counts(rows, stamp)
    assert counts.dtype == np.uint64 and counts.shape == (31, 256)
    assert np.array_equal(counts, want) and tail.tolist() == [700, 0]
    assert (counts.sum(1) == 700).all()


def test_bin_counts_g20_equals_decoded_rows(fx):
    rows = fx["g20"].encode(fx["X"][:3000])
    assert rows.shape[1] == 20
    c20, t20 = bin_counts(rows, fx["g20"].stamp)
    c32, t32 = bin_counts(decode_g20_bins(rows), fx["g20"].stamp)
    assert np.array_equal(c20, c32) and np.array_equal(t20, t32)
    assert c20[:, 32:].sum() == 0 and t20.tolist() == [3000, 0]


def test_stale_rows_land_in_tail_only(fx):
    rows = fx["g32"].encode(fx["X"][:500]).copy()
    stamp = fx["g32"].stamp
    rows[100:180, 31] = stamp % 255 + 1                       # another table's stamp
    counts, tail = bin_counts(rows, stamp)
    keep = np.r_[0:100, 180:500]
    want, _ = bin_counts(rows[keep], stamp)
    assert tail.tolist() == [420, 80] and np.array_equal(counts, want)
    with pytest.raises(ValueError):
        bin_counts(rows[:, :31], stamp)


def test_psi_properties():
    rng = np.random.default_rng(0)
    nb = np.full(N_COLS, 9, np.int32)
    nb[3] = 1
    a = np.zeros((N_COLS, N_CELLS), np.uint64)
    b = np.zeros((N_COLS, N_CELLS), np.uint64)
    for j in range(N_COLS):
        a[j, :nb[j]] = rng.multinomial(5000, np.ones(nb[j]) / nb[j])
        b[j, :nb[j]] = rng.multinomial(7000, np.ones(nb[j]) / nb[j])
    same, beyond = psi(a, 5000, a, 5000, nb)
    assert same.dtype == np.float64 and same.shape == (31,) and (same == 0.0).all() and not beyond.any()
    ab, _ = psi(a, 5000, b, 7000, nb)
    ba, _ = psi(b, 7000, a, 5000, nb)
    assert ab[3] == 0.0 and (np.delete(ab, 3) > 0).all()        # K == 1: exactly 0
    assert np.allclose(ab, ba, rtol=1e-12, atol=0)              # symmetric under the swap
    # the definition, column 0, written out
    K = 9
    p = (a[0, :K].astype(np.float64) + 0.5) / (5000 + 0.5 * K)
    q = (b[0, :K].astype(np.float64) + 0.5) / (7000 + 0.5 * K)
    assert ab[0] == pytest.approx(float(((q - p) * np.log(q / p)).sum()), rel=1e-12)
    # cells >= K are reported, not scored
    c = b.copy()
    c[5, 9] = 11
    c[5, 200] = 2
    got, beyond = psi(a, 5000, c, 7000, nb)
    assert beyond[5] == 13 and beyond.sum() == 13 and got[5] == ab[5]


def test_no_false_alarm_and_true_alarm(fx):
    for bins in (fx["g32"], fx["g20"]):
        assert bins.edges[SHIFTED].size >= 4
        ref = DriftReference.fit(fx["ref_half"], bins)
        assert ref.rows == 20_000
        rep = DriftReport.compare(ref, *bin_counts(bins.encode(fx["live_half"]), bins.stamp))
        assert rep.rows == 20_000 and rep.stale == 0 and not rep.beyond_table.any()
        assert rep.status == ["stable"] * 31, rep.worst(3)
        assert rep.names == COLUMN_NAMES and rep.names[:30] == tuple(FEATURE_NAMES) and rep.names[30] == "AmountBucket"
        live = fx["live_half"].copy()
        live[:, SHIFTED] += fx["X"][:, SHIFTED].std()
        rep = DriftReport.compare(ref, *bin_counts(bins.encode(live), bins.stamp))
        assert rep.status[SHIFTED] == "drift"
        assert [s for j, s in enumerate(rep.status) if 1 <= j <= 28 and j != SHIFTED] == ["stable"] * 27
        assert rep.worst(1)[0][0] == "V14" and rep.drifting == 1
        js = rep.to_json()
        assert js["status"][SHIFTED] == "drift" and js["worst"][0]["name"] == "V14" and js["rows"] == 20_000


def test_report_bands_and_min_rows(fx):
    ref = DriftReference.fit(fx["ref_half"], fx["g32"])
    live = fx["live_half"][::2][:9_999]                      # strided: the whole range of Time
    counts, tail = bin_counts(fx["g32"].encode(live), fx["g32"].stamp)
    rep = DriftReport.compare(ref, counts, tail)
    assert np.isnan(rep.psi).all() and rep.status == ["insufficient"] * 31 and rep.worst(3) == []
    assert rep.to_json()["psi"] == [None] * 31
    rep = DriftReport.compare(ref, counts, tail, min_rows=5_000)
    assert np.isfinite(rep.psi).all() and set(rep.status) == {"stable"}
    rep = DriftReport(np.r_[0.05, 0.1, 0.2, 0.25, np.zeros(27)], 20_000, 0, np.zeros(31, np.uint64))
    assert rep.status[:4] == ["stable", "moderate", "moderate", "drift"]
    rep = DriftReport(np.r_[0.05, 0.1, np.zeros(29)], 20_000, 0, np.zeros(31, np.uint64), bands=(0.01, 0.08))
    assert rep.status[:3] == ["moderate", "drift", "stable"]


def test_reference_round_trip_and_compatible(fx, tmp_path):
    for bins in (fx["g32"], fx["g20"]):
        ref = DriftReference.fit(fx["X"][:5000], bins)
        assert ref.bits == bins.bits and ref.stamp == bins.stamp and ref.rows == 5000
        assert ref.n_bins.dtype == np.int32 and ref.n_bins[30] == 14
        assert ref.n_bins[:30].tolist() == [e.size + 1 for e in bins.edges]
        path = str(tmp_path / f"ref{bins.bits}.safetensors")
        ref.save(path)
        back = DriftReference.load(path)
        assert (back.bits, back.stamp, back.rows) == (ref.bits, ref.stamp, ref.rows)
        assert back.counts.dtype == np.uint64 and np.array_equal(back.counts, ref.counts)
        assert np.array_equal(back.n_bins, ref.n_bins)
        assert back.compatible(bins)
    ref = DriftReference.fit(fx["X"][:5000], fx["g32"])
    assert not ref.compatible(fx["g20"]) and not ref.compatible(None)
    other = ObliviousGBDT.random_init(100, 6, 1, fx["X"]).bin_spec()
    assert other.stamp != fx["g32"].stamp and not ref.compatible(other)
    same = DriftReference.from_counts(fx["g32"], ref.counts, ref.rows)
    assert np.array_equal(same.n_bins, n_bins_of(fx["g32"])) and same.compatible(fx["g32"])


def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def test_cpu_scorer_and_drift_routes(fx):
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.serving import CpuScorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    model, bins = fx["model"], fx["g20"]
    ref = DriftReference.fit(fx["ref_half"], bins)
    with pytest.raises(ValueError, match="no drift detector"):
        CpuScorer(build_model("mlp", seed=0)).set_drift(ref)
    with pytest.raises(ValueError, match="not counted against"):
        CpuScorer(ObliviousGBDT.random_init(100, 6, 1, fx["X"])).set_drift(ref)
    live = fx["live_half"][:1200]
    want = DriftReport.compare(ref, *bin_counts(bins.encode(live), bins.stamp), min_rows=1000)

    async def go():
        scorer = CpuScorer(model)
        srv = SeldonServer(scorer, token="s3cret")
        h = {"Authorization": "Bearer s3cret"}
        async with TestClient(TestServer(srv.app)) as cl:
            assert (await cl.get("/drift")).status == 401
            r = await cl.get("/drift", headers=h)                      # no reference yet
            assert r.status == 400 and (await r.json())["status"]["status"] == "FAILURE"
            scorer.set_drift(ref, min_rows=1000)
            for lo in range(0, 1200, 400):
                r = await cl.post("/api/v0.1/predictions", json=seldon.build_request(live[lo:lo + 400]), headers=h)
                assert r.status == 200
            for path in ("/api/v0.1/drift", "/api/v1.0/drift", "/drift"):
                r = await cl.get(path, headers=h)
                assert r.status == 200
                js = await r.json()
                assert js["rows"] == 1200 and js["stale"] == 0 and js["names"] == list(COLUMN_NAMES)
                assert js["psi"] == want.psi.tolist() and js["status"] == want.status
                assert [w["name"] for w in js["worst"]] == [w[0] for w in want.worst(3)]
            r = await cl.post("/drift", json={"reset": True}, headers=h)
            assert r.status == 200 and (await r.json())["rows"] == 1200
            js = await (await cl.get("/drift", headers=h)).json()
            assert js["rows"] == 0 and js["status"] == ["insufficient"] * 31 and js["psi"] == [None] * 31
    _run(go())


class FakeLog:
    """The fields of a PartitionLog that ring_write touches, in ordinary memory."""

    def __init__(self, n, bins):
        self.bins, self.row_bytes, self.row_format = bins, 20, "g20"
        self.feats = type("A", (), {})()
        self.feats.array = np.zeros((n, 5), np.float32)
        self.ids = type("A", (), {"array": np.zeros(n, np.uint64)})()
        self.customer = type("A", (), {"array": np.zeros(n, np.uint32)})()

    def write_rows(self, r, X):
        self.feats.array.view(np.uint8).reshape(-1, 20)[r:r + len(X)] = self.bins.encode(X)


class FakeRing:
    """Stands in for libccfd_hip's ring calls: hands out at most `grant` contiguous slots of a
    ring of `n`, wrapping, and logs every call."""

    def __init__(self, n, grant, events):
        self.n, self.grant, self.head, self.events = n, grant, 0, events

    def ccfd_engine_ring_acquire(self, h, part, want, row_ref):
        k = min(want, self.grant, self.n - self.head % self.n)
        row_ref._obj.value = self.head % self.n
        return k

    def ccfd_engine_ring_commit(self, h, part, k):
        self.events.append(("commit", int(k)))
        self.head += k


def test_ring_write_tap_sees_committed_rows_before_the_commit(fx, monkeypatch):
    from ccfd_demo_summit_amd.engine import stream_engine as se
    events = []
    fake = FakeRing(96, 40, events)
    monkeypatch.setattr(se, "lib", lambda: fake)
    eng = object.__new__(se.StreamEngine)
    eng.h = 1
    eng.logs = {0: FakeLog(96, fx["g20"])}
    X = fx["X"][:250]
    seen = []

    def tap(view):
        assert view.dtype == np.uint8 and view.shape[1] == 20
        events.append(("tap", len(view)))
        seen.append(view.copy())
    assert eng.ring_write(0, X, np.arange(250, dtype=np.uint64), tap=tap) == 250
    assert np.array_equal(np.concatenate(seen), fx["g20"].encode(X))       # exactly the rows, in order
    kinds = [e[0] for e in events]
    assert kinds == ["tap", "commit"] * (len(events) // 2) and len(events) > 6   # each tap before its commit
    assert [e[1] for e in events[0::2]] == [e[1] for e in events[1::2]]
    assert sum(e[1] for e in events[1::2]) == 250
    n_events = len(events)
    assert eng.ring_write(0, X[:10]) == 10 and len(events) == n_events + 1   # no tap: commits only
    eng.h = None


def test_engine_service_drift_refusals(fx):
    from ccfd_demo_summit_amd.launch.engine_service import check_drift_tap

    class Dm:
        def __init__(self, fmt, bins):
            self.row_format, self.bins = fmt, bins

    class Mon:
        def __init__(self, ref):
            self.reference = ref
    mon = Mon(DriftReference.fit(fx["X"][:2000], fx["g20"]))
    check_drift_tap(mon, Dm("g20", fx["g20"]), "launch", False)
    with pytest.raises(ValueError, match="native Kafka consumer"):
        check_drift_tap(mon, Dm("g20", fx["g20"]), "launch", True)
    with pytest.raises(ValueError, match="not binned"):
        check_drift_tap(mon, Dm("w64", None), "launch", False)
    with pytest.raises(ValueError, match="persistent"):
        check_drift_tap(mon, Dm("g20", fx["g20"]), "persistent", False)
    with pytest.raises(ValueError, match="not counted against"):
        check_drift_tap(mon, Dm("g32", fx["g32"]), "launch", False)


def test_drift_series_in_the_exposition():
    from prometheus_client import CollectorRegistry, generate_latest
    from ccfd_demo_summit_amd.contracts import metric_names as M
    from ccfd_demo_summit_amd.metrics.exporter import GpuEngineCollector
    extra = {M.GPU_DRIFT_ROWS + "_total": 12345, M.GPU_DRIFT_STALE_ROWS + "_total": 2,
             "drift_psi": {"feature": {"V14": 0.5, "Time": 0.0}}, "drift_features_drifting": 1}
    reg = CollectorRegistry()
    reg.register(GpuEngineCollector(lambda: (np.zeros(64, np.int64), np.zeros(256, np.int64), extra)))
    text = generate_latest(reg).decode()
    assert "ccfd_gpu_drift_rows_total 12345.0" in text and "ccfd_gpu_drift_stale_rows_total 2.0" in text
    assert 'ccfd_gpu_drift_psi{feature="V14"} 0.5' in text and "ccfd_gpu_drift_features_drifting 1.0" in text
    assert M.GPU_DRIFT_PSI == "ccfd_gpu_drift_psi"


def test_train_cli_writes_a_reference(tmp_path):
    from ccfd_demo_summit_amd.models import load_model
    from ccfd_demo_summit_amd.train.__main__ import main
    out, ref_path = str(tmp_path / "m.safetensors"), str(tmp_path / "ref.safetensors")
    assert main(["--model", "gbdt", "--rows", "6000", "--trees", "4", "--depth", "3", "--device", "cpu", "--out", out,
                 "--drift-reference-out", ref_path]) == 0
    ref, model = DriftReference.load(ref_path), load_model(out)
    assert ref.bits == 5 and ref.rows == 4800 and ref.compatible(model.bin_spec(bits=5))
    assert main(["--model", "gbdt", "--rows", "6000", "--trees", "4", "--depth", "3", "--device", "cpu", "--out", out,
                 "--drift-reference-out", ref_path, "--bits", "8"]) == 0
    assert DriftReference.load(ref_path).bits == 8
