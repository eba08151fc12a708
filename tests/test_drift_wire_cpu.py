"""CPU side of drift detection on W64 rows (docs/DRIFT.md "W64 rows"): the quantile fit, the
wire_bin_counts oracle on hand-checkable rows, PSI end to end, the W64 reference file, the
CpuScorer / SeldonServer surface for MLP and LR, the engine tap's refusals, the ring tap over a
64-byte log, the ABI mirror and the training CLI."""
import asyncio
import ctypes as C
import subprocess

import numpy as np
import pytest

from ccfd_demo_summit_amd.contracts import seldon
from ccfd_demo_summit_amd.contracts.transaction import AMOUNT_COL, TIME_COL, amount_bucket, decode_wire, encode_wire
from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models.drift import (COLUMN_NAMES, N_CELLS, N_COLS, DriftReference, DriftReport,
                                               wire_bin_counts, wire_bins, wire_bins_fit, wire_edge_table)
from ccfd_demo_summit_amd.models.gbdt import BinSpec, ObliviousGBDT

SHIFTED = 14                                   # feature index of V14
EDGES = np.array([-1.0, 0.0, 0.5, 2.0], np.float32)     # every value a bf16


@pytest.fixture(scope="module")
def fx():
    X, _ = generate(40_000, seed=7)
    ref_half, live_half = X[0::2], X[1::2]
    return {"X": X, "ref_half": ref_half, "live_half": live_half, "bins": wire_bins_fit(ref_half)}


def edge_case_rows():
    """W64 rows poked bit by bit, every feature 0.25 (cell 2 of EDGES) unless named, and the
    cell each named value must land in.  Returns (rows u8 [k,64], [(row, feature, cell)])."""
    cases = []                                  # (feature j, raw bits, cell)
    for j in (3, TIME_COL, AMOUNT_COL):         # a bf16 column and the two f32 ones
        wide = j in (TIME_COL, AMOUNT_COL)
        one_up = np.nextafter(np.float32(0.5), np.float32(np.inf)).view(np.uint32) if wide else np.uint32(0x3F01)
        on = np.float32(0.5).view(np.uint32) if wide else np.uint32(0x3F00)
        sh = 0 if wide else 16
        cases += [(j, int(on), 2), (j, int(one_up), 3),                       # on the edge is not above it
                  (j, 0x7FC00000 >> sh, 0), (j, 0xFFC00000 >> sh, 0),          # NaN of either sign
                  (j, 0x7F800000 >> sh, 4), (j, 0xFF800000 >> sh, 0),          # +inf, -inf
                  (j, 0x80000000 >> sh, 1), (j, 0, 1),                         # -0.0 == 0.0: not above the edge 0.0
                  (j, 1, 2), ((j, 0x80000001, 1) if wide else (j, 0x8001, 1))]  # smallest denormals: not flushed
    rows = encode_wire(np.full((len(cases), 30), 0.25, np.float32))
    want = []
    for r, (j, bits, cell) in enumerate(cases):
        if j == TIME_COL:
            rows[r].view(np.uint32)[14] = bits
        elif j == AMOUNT_COL:
            rows[r].view(np.uint32)[15] = bits
        else:
            rows[r].view(np.uint16)[j - 1] = bits
        want.append((r, j, cell))
    return rows, want


def test_quantile_fit_gives_31_edges_everywhere(fx):
    bins = fx["bins"]
    assert isinstance(bins, BinSpec) and bins.bits == 5 and len(bins.edges) == 30
    for e in bins.edges:
        assert e.dtype == np.float32 and e.size == 31 and np.isfinite(e).all() and (np.diff(e) > 0).all()
    # the edges are quantiles of the rows as the model sees them: half the V14 column lies below the middle edge
    seen = decode_wire(encode_wire(fx["ref_half"]))[:, SHIFTED]
    assert abs(float((seen <= bins.edges[SHIFTED][15]).mean()) - 0.5) < 0.01
    X = fx["ref_half"].copy()
    X[:, 5] = 3.0
    X[:, 9] = np.nan
    got = wire_bins_fit(X, cells=8)
    assert got.edges[5].size <= 1 and got.edges[9].size == 0 and max(e.size for e in got.edges) == 7
    for cells in (1, 33):
        with pytest.raises(ValueError, match="cells"):
            wire_bins_fit(X, cells=cells)


def test_wire_table_refusals():
    ok = [EDGES] * 30
    assert wire_bins(ok).bits == 5
    t = wire_edge_table(ok)
    assert t.shape == (30, 32) and t.dtype == np.float32 and np.array_equal(t[:, :4], np.tile(EDGES, (30, 1)))
    assert np.isposinf(t[:, 4:]).all()
    for bad in (np.arange(32, dtype=np.float32), np.array([0.0, np.nan], np.float32), np.array([1.0, 0.5], np.float32),
                np.array([0.5, 0.5], np.float32), np.array([0.0, np.inf], np.float32)):
        with pytest.raises(ValueError):
            wire_bins(ok[:7] + [bad] + ok[8:])
    with pytest.raises(ValueError):
        wire_bins(ok[:29])
    with pytest.raises(ValueError, match="rows must be"):
        wire_bin_counts(np.zeros((4, 32), np.uint8), ok)


def test_oracle_on_hand_checked_rows():
    rows, want = edge_case_rows()
    n = len(rows)
    counts, tail = wire_bin_counts(rows, [EDGES] * 30)
    assert counts.dtype == np.uint64 and counts.shape == (N_COLS, N_CELLS) and tail.dtype == np.uint64
    assert tail.tolist() == [n, 0] and (counts.sum(1) == n).all()
    expect = np.zeros((N_COLS, N_CELLS), np.uint64)
    expect[:30, 2] = n                                   # 0.25 everywhere ...
    for r, j, cell in want:                              # ... but the poked value
        expect[j, 2] -= 1
        expect[j, cell] += 1
    expect[30] = np.bincount(amount_bucket(decode_wire(rows)[:, AMOUNT_COL]), minlength=N_CELLS)
    assert np.array_equal(counts, expect)
    # one row at a time, so each case stands alone
    for r, j, cell in want:
        c, _ = wire_bin_counts(rows[r:r + 1], [EDGES] * 30)
        assert c[j, cell] == 1 and c[j].sum() == 1, (r, j, cell)


def test_oracle_equals_a_loop_and_the_amount_column(fx):
    rows = encode_wire(fx["X"][:600])
    x = decode_wire(rows)
    want = np.zeros((N_COLS, N_CELLS), np.uint64)
    for r in range(600):
        for j in range(30):
            want[j, int(sum(1 for e in fx["bins"].edges[j] if e < x[r, j]))] += 1
    want[30] = np.bincount(amount_bucket(x[:, AMOUNT_COL]), minlength=N_CELLS)
    counts, tail = wire_bin_counts(rows, fx["bins"])
    assert np.array_equal(counts, want) and tail.tolist() == [600, 0]
    assert counts[:, 32:].sum() == 0


def test_no_false_alarm_and_true_alarm(fx):
    ref = DriftReference.fit_wire(fx["ref_half"])
    assert ref.rows == 20_000 and ref.bits == 16 and ref.row_bytes == 64 and ref.is_wire
    assert ref.stamp == fx["bins"].stamp and ref.n_bins.tolist() == [32] * 30 + [14]
    rep = DriftReport.compare(ref, *wire_bin_counts(encode_wire(fx["live_half"]), ref.edges))
    assert rep.rows == 20_000 and rep.stale == 0 and not rep.beyond_table.any()
    assert rep.status == ["stable"] * 31, rep.worst(3)
    assert rep.names == COLUMN_NAMES and rep.names[30] == "AmountBucket"
    live = fx["live_half"].copy()
    live[:, SHIFTED] += fx["X"][:, SHIFTED].std()
    rep = DriftReport.compare(ref, *wire_bin_counts(encode_wire(live), ref.edges))
    assert rep.status[SHIFTED] == "drift" and rep.drifting == 1 and rep.worst(1)[0][0] == "V14"
    assert [s for j, s in enumerate(rep.status) if j != SHIFTED] == ["stable"] * 30
    # first half / second half: synthetic Time grows with the row index, a real drift of Time
    first = DriftReference.fit_wire(fx["X"][:20_000])
    rep = DriftReport.compare(first, *wire_bin_counts(encode_wire(fx["X"][20_000:]), first.edges))
    assert rep.status[TIME_COL] == "drift"


def test_reference_round_trip_and_old_files(fx, tmp_path):
    ref = DriftReference.fit_wire(fx["X"][:5000], cells=16)
    assert ref.n_bins[:30].max() == 16 and ref.rows == 5000
    path = str(tmp_path / "w64.safetensors")
    ref.save(path)
    back = DriftReference.load(path)
    assert (back.bits, back.stamp, back.rows, back.row_bytes) == (16, ref.stamp, 5000, 64)
    assert np.array_equal(back.counts, ref.counts) and np.array_equal(back.n_bins, ref.n_bins)
    assert len(back.edges) == 30 and all(np.array_equal(a, b) and a.dtype == np.float32
                                          for a, b in zip(back.edges, ref.edges))
    assert back.bins.stamp == ref.stamp
    given = DriftReference.fit_wire(fx["X"][:5000], bins=ref.bins)
    assert np.array_equal(given.counts, ref.counts) and given.stamp == ref.stamp
    # a binned reference: the five-argument constructor, and a file laid out as version 1 writes it
    model = ObliviousGBDT.random_init(100, 6, 0, fx["X"])
    from safetensors.numpy import save_file
    for bits in (5, 8):
        bins = model.bin_spec(bits=bits)
        old = DriftReference.fit(fx["X"][:3000], bins)
        five = DriftReference(old.bits, old.stamp, old.n_bins, old.counts, old.rows)
        assert five.edges is None and not five.is_wire and five.compatible(bins)
        p = str(tmp_path / f"old{bits}.safetensors")
        save_file({"n_bins": old.n_bins, "counts": old.counts}, p,
                  metadata={"kind": "drift_reference", "version": "1", "bits": str(bits), "stamp": str(old.stamp),
                            "rows": "3000"})
        got = DriftReference.load(p)
        assert got.bits == bits and got.edges is None and got.compatible(bins) and np.array_equal(got.counts, old.counts)
        assert not ref.compatible(bins)                   # a W64 reference belongs to no model's table
        with pytest.raises(ValueError, match="edges"):
            DriftReference(bits, old.stamp, old.n_bins, old.counts, old.rows, ref.edges)
    assert not ref.compatible(ref.bins) and not ref.compatible(None)
    with pytest.raises(ValueError, match="edges"):
        DriftReference(16, ref.stamp, ref.n_bins, ref.counts, ref.rows)


def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


@pytest.mark.parametrize("kind", ["mlp", "lr"])
def test_cpu_scorer_and_drift_routes(fx, kind):
    from aiohttp.test_utils import TestClient, TestServer
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.serving import CpuScorer
    from ccfd_demo_summit_amd.serving.seldon_server import SeldonServer
    ref = DriftReference.fit_wire(fx["ref_half"], bins=fx["bins"])
    gbdt = ObliviousGBDT.random_init(100, 6, 0, fx["X"])
    binned = DriftReference.fit(fx["ref_half"][:2000], gbdt.bin_spec(bits=5))
    model = build_model(kind, seed=0)
    with pytest.raises(ValueError, match="no drift detector"):
        CpuScorer(model).set_drift(binned)
    with pytest.raises(ValueError, match="W64 rows.*'gbdt' does not score"):
        CpuScorer(gbdt).set_drift(ref)
    live = fx["live_half"][:1200]
    want = DriftReport.compare(ref, *wire_bin_counts(encode_wire(live), ref.edges), min_rows=1000)
    plain = CpuScorer(model).score(live)

    async def go():
        scorer = CpuScorer(model)
        srv = SeldonServer(scorer)
        async with TestClient(TestServer(srv.app)) as cl:
            assert (await cl.get("/drift")).status == 400
            scorer.set_drift(ref, min_rows=1000)
            for lo in range(0, 1200, 400):
                r = await cl.post("/api/v0.1/predictions", json=seldon.build_request(live[lo:lo + 400]))
                assert r.status == 200
            for path in ("/api/v0.1/drift", "/api/v1.0/drift", "/drift"):
                js = await (await cl.get(path)).json()
                assert js["rows"] == 1200 and js["stale"] == 0 and js["names"] == list(COLUMN_NAMES)
                assert js["psi"] == want.psi.tolist() and js["status"] == want.status
                assert [w["name"] for w in js["worst"]] == [w[0] for w in want.worst(3)]
            r = await cl.post("/drift", json={"reset": True})
            assert r.status == 200 and (await r.json())["rows"] == 1200
            js = await (await cl.get("/drift")).json()
            assert js["rows"] == 0 and js["status"] == ["insufficient"] * 31
        got = scorer.score(live)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])    # counting changes no score
        assert scorer.drift().rows == 1200
    _run(go())


def test_engine_tap_refusals(fx):
    from ccfd_demo_summit_amd.launch.engine_service import check_drift_tap

    class Dm:
        def __init__(self, fmt, bins):
            self.row_format, self.bins = fmt, bins

    class Mon:
        def __init__(self, ref):
            self.reference = ref
    g20 = ObliviousGBDT.random_init(100, 6, 0, fx["X"]).bin_spec(bits=5)
    wire = Mon(DriftReference.fit_wire(fx["X"][:2000], bins=fx["bins"]))
    binned = Mon(DriftReference.fit(fx["X"][:2000], g20))
    check_drift_tap(wire, Dm("w64", None), "launch", False)
    check_drift_tap(binned, Dm("g20", g20), "launch", False)
    with pytest.raises(ValueError, match="native Kafka consumer"):
        check_drift_tap(wire, Dm("w64", None), "launch", True)
    with pytest.raises(ValueError, match="persistent"):
        check_drift_tap(wire, Dm("w64", None), "persistent", False)
    with pytest.raises(ValueError, match="not binned"):
        check_drift_tap(binned, Dm("w64", None), "launch", False)
    for fmt in ("g20", "g32"):
        with pytest.raises(ValueError, match=f"reference is for W64 rows.*engine's rows are {fmt}"):
            check_drift_tap(wire, Dm(fmt, g20), "launch", False)
    with pytest.raises(ValueError, match="W64 reference needs W64 rows"):
        check_drift_tap(wire, Dm("f32", None), "launch", False)


class FakeLog:
    """The fields of a W64 PartitionLog that ring_write touches, in ordinary memory."""

    def __init__(self, n):
        self.row_bytes, self.row_format = 64, "w64"
        self.feats = type("A", (), {})()
        self.feats.array = np.zeros((n, 16), np.float32)
        self.ids = type("A", (), {"array": np.zeros(n, np.uint64)})()
        self.customer = type("A", (), {"array": np.zeros(n, np.uint32)})()

    def write_rows(self, r, X):
        self.feats.array.view(np.uint8).reshape(-1, 64)[r:r + len(X)] = encode_wire(X)


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


def test_ring_write_tap_sees_w64_rows_before_the_commit(fx, monkeypatch):
    from ccfd_demo_summit_amd.engine import stream_engine as se
    events = []
    fake = FakeRing(96, 40, events)
    monkeypatch.setattr(se, "lib", lambda: fake)
    eng = object.__new__(se.StreamEngine)
    eng.h = 1
    eng.logs = {0: FakeLog(96)}
    X = fx["X"][:250]
    counts, tail = np.zeros((N_COLS, N_CELLS), np.uint64), np.zeros(2, np.uint64)
    seen = []

    def tap(view):
        assert view.dtype == np.uint8 and view.shape[1] == 64
        events.append(("tap", len(view)))
        seen.append(view.copy())
        c, t = wire_bin_counts(view, fx["bins"])
        counts.__iadd__(c)
        tail.__iadd__(t)
    assert eng.ring_write(0, X, np.arange(250, dtype=np.uint64), tap=tap) == 250
    assert np.array_equal(np.concatenate(seen), encode_wire(X))            # exactly the rows, in order
    kinds = [e[0] for e in events]
    assert kinds == ["tap", "commit"] * (len(events) // 2) and len(events) > 6   # each tap before its commit
    assert [e[1] for e in events[0::2]] == [e[1] for e in events[1::2]]
    assert sum(e[1] for e in events[1::2]) == 250
    want = wire_bin_counts(encode_wire(X), fx["bins"])
    assert np.array_equal(counts, want[0]) and np.array_equal(tail, want[1])
    eng.h = None


def test_abi_layout_of_the_wire_args(tmp_path):
    from ccfd_demo_summit_amd.ops import _lib
    from ccfd_demo_summit_amd.ops.build import CSRC
    fields = ["rows", "edges", "counts", "tail", "n", "max_workgroups", "pad"]
    items = ["sizeof(ccfd_drift_wire_args)"] + [f"offsetof(ccfd_drift_wire_args,{f})" for f in fields]
    items += ["CCFD_DRIFT_WIRE_EDGES", "CCFD_DRIFT_COLS", "CCFD_DRIFT_CELLS", "CCFD_WIRE_ROW_BYTES"]
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ccfd_abi.h"\nint main(){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    r = subprocess.run(["g++", str(src), "-I", str(CSRC / "include"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.DriftWireArgs)] + [getattr(_lib.DriftWireArgs, f).offset for f in fields]
    want += [_lib.DRIFT_WIRE_EDGES, _lib.DRIFT_COLS, _lib.DRIFT_CELLS, 64]
    assert out == want and out[0] == 48
    assert wire_edge_table([EDGES] * 30).shape == (_lib.DRIFT_COLS - 1, _lib.DRIFT_WIRE_EDGES)


def test_train_cli_writes_w64_references(tmp_path):
    from ccfd_demo_summit_amd.train.__main__ import main
    out, ref_path = str(tmp_path / "m.safetensors"), str(tmp_path / "ref.safetensors")
    for kind in ("mlp", "lr"):
        assert main(["--model", kind, "--rows", "6000", "--epochs", "1", "--device", "cpu", "--out", out,
                     "--drift-reference-out", ref_path]) == 0
        ref = DriftReference.load(ref_path)
        assert ref.bits == 16 and ref.rows == 4800 and ref.row_bytes == 64 and ref.n_bins[30] == 14
        assert 8 < ref.n_bins[:30].max() <= 32 and (ref.counts.sum(1) == 4800).all()
    assert main(["--model", "mlp", "--rows", "6000", "--epochs", "1", "--device", "cpu", "--out", out,
                 "--drift-reference-out", ref_path, "--drift-cells", "8"]) == 0
    assert DriftReference.load(ref_path).n_bins[:30].max() <= 8
    with pytest.raises(SystemExit, match="drift-cells"):
        main(["--model", "mlp", "--rows", "6000", "--device", "cpu", "--out", out, "--drift-reference-out", ref_path,
              "--drift-cells", "33"])
    with pytest.raises(SystemExit, match="--bits is for --model gbdt"):
        main(["--model", "lr", "--rows", "6000", "--device", "cpu", "--out", out, "--drift-reference-out", ref_path,
              "--bits", "5"])
    assert main(["--model", "gbdt", "--rows", "6000", "--trees", "4", "--depth", "3", "--device", "cpu", "--out", out,
                 "--drift-reference-out", ref_path]) == 0
    ref = DriftReference.load(ref_path)
    assert ref.bits == 5 and ref.rows == 4800 and ref.edges is None
