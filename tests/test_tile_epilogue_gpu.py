"""What the MLP / LR kernels do with a scored 16-row tile (tile_core.h): outputs, route,
counters, BOTH amount histograms per bucket and the flag list -- on the claimed and pipelined
persistent kernels and on plain and coalesced launches, f32 and W64 rows, with row amounts ON
the histogram's bucket bounds (each bound, one float32 ulp below and above it, and 0)."""
import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.contracts.metric_names import AMOUNT_BUCKETS
from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import build_model

pytestmark = pytest.mark.gpu

BOUNDS = np.asarray(AMOUNT_BUCKETS, np.float32)
EDGE_AMOUNTS = np.concatenate([[np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(np.inf))]
                               for b in BOUNDS] + [[np.float32(0)]]).astype(np.float32)
N_PERSIST = 2 * 4096 + 999          # 2 full batches, then a partial item and a partial 16-row tile
LAUNCH_SIZES = [1, 15, 17, 65, 1025]


@pytest.fixture(scope="module")
def setup(gpu):
    """Rows whose amounts cycle through EDGE_AMOUNTS, both models, and each model's oracle on
    f32 and on W64 rows -- computed once, read-only."""
    from ccfd_demo_summit_amd.contracts import decode_wire, encode_wire
    X, _ = generate(N_PERSIST + 41, seed=23)
    X[:, 29] = EDGE_AMOUNTS[np.arange(X.shape[0]) % len(EDGE_AMOUNTS)]
    Xd = decode_wire(encode_wire(X))
    models = {"mlp": build_model("mlp", seed=4, X_ref=X, calibrate_rate=0.05),
              "lr": build_model("lr", seed=5, X_ref=X, calibrate_rate=0.05)}
    ref = {("mlp", False): models["mlp"].predict_proba(X, emulate_bf16=True),
           ("mlp", True): models["mlp"].wire_proba(X),
           ("lr", False): models["lr"].predict_proba(X),
           ("lr", True): models["lr"].predict_proba(Xd)}
    for v in ref.values():
        v.setflags(write=False)
    X.setflags(write=False)
    return X, models, ref


def _check(c, amount, ref, fraud, flagged_rows, what):
    """Counters `c` of rows with amounts `amount` and oracle proba `ref`; `fraud`: the device's
    own route per row; `flagged_rows`: the flag list as row indices (None: not read)."""
    n = len(amount)
    nf = int(fraud.sum())
    want = float(np.round(ref.astype(np.float64) * 1e6).sum())
    print(f"{what}: n={n} fraud={nf} psum={int(c[3])} oracle={want:.0f} bound={2e-4 * n * 1e6 / 100:.0f}")
    if flagged_rows is not None:
        assert len(np.unique(flagged_rows)) == len(flagged_rows)          # no row flagged twice
        np.testing.assert_array_equal(np.sort(flagged_rows), np.flatnonzero(fraud))
    assert c[0] == n and c[1] == nf and c[2] == n - nf
    bk = np.searchsorted(BOUNDS, amount, side="left")
    np.testing.assert_array_equal(c[8:22], np.bincount(bk[~fraud], minlength=14))
    np.testing.assert_array_equal(c[24:38], np.bincount(bk[fraud], minlength=14))
    assert abs(int(c[3]) - want) < 2e-4 * n * 1e6 / 100


def _engine_case(gpu, setup, kind, wire, n_rows, pumps, **kw):
    """One engine over the first `n_rows` rows: pump, then the epoch's counters against the
    scored-record ring (device proba / route per row) and the flag list."""
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    X, models, ref = setup
    eng = StreamEngine(DeviceModel(models[kind], gpu, wire=wire), input_mode="zerocopy", **kw)
    eng.enable_scored(n_rows + 64)
    log = PartitionLog.from_arrays(X[:n_rows], ids=np.arange(n_rows, dtype=np.uint64) + 1000, wire=wire)
    eng.add_log(0, log)
    rows = sum(eng.pump(k, batch_rows=b, drain=True).rows for k, b in pumps)
    assert rows == n_rows
    flagged = eng.drain_flagged()
    rec = eng.drain_scored()
    side = torch.cuda.Stream(gpu)
    c = eng.flip_epoch(side)
    side.synchronize()
    c = c.cpu().numpy()
    eng.close()
    log.free()
    ids = (rec["tx_id"] - 1000).astype(np.int64)
    np.testing.assert_array_equal(np.sort(ids), np.arange(n_rows))           # every row scored once
    fraud = np.zeros(n_rows, bool)
    fraud[ids] = rec["route"] != 0
    _check(c, X[:n_rows, 29], ref[(kind, wire)][:n_rows], fraud, (flagged["tx_id"] - 1000).astype(np.int64),
           f"{kind} wire={wire} {kw}")


@pytest.mark.parametrize("kind,wire,item_rows,pipe", [
    (k, w, r, False) for k in ("mlp", "lr") for w in (True, False) for r in (64, 256)
] + [("mlp", True, 64, True), ("mlp", True, 128, True)])
def test_persistent_tile_epilogue_bucket_bounds(gpu, setup, monkeypatch, kind, wire, item_rows, pipe):
    monkeypatch.setenv("CCFD_PERSIST_ITEM_ROWS", str(item_rows))
    if pipe:
        monkeypatch.setenv("CCFD_PERSIST_PIPE", "1")
    else:
        monkeypatch.delenv("CCFD_PERSIST_PIPE", raising=False)
    _engine_case(gpu, setup, kind, wire, N_PERSIST, [(2, 4096), (1, 999)],
                 batch=4096, depth=3, streams=1, exec_mode="persistent")


@pytest.mark.parametrize("kind", ["mlp", "lr"])
@pytest.mark.parametrize("wire", [True, False])
@pytest.mark.parametrize("n", LAUNCH_SIZES)
def test_plain_launch_tile_epilogue_bucket_bounds(gpu, setup, kind, wire, n):
    from ccfd_demo_summit_amd.contracts import encode_wire
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_counters, score
    X, models, ref = setup
    s = 7 * n % len(EDGE_AMOUNTS)                     # another phase of the amount cycle per size
    rows = X[s:s + n]
    cnt = new_counters(gpu)
    x = torch.from_numpy(encode_wire(rows) if wire else np.ascontiguousarray(rows)).to(gpu)
    p, r = score(DeviceModel(models[kind], gpu, wire=wire), x, 0.5, counters=cnt)
    torch.cuda.synchronize(gpu)
    p, r = p.cpu().numpy(), r.cpu().numpy()
    c = cnt.cpu().numpy()
    _check(c, rows[:, 29], ref[(kind, wire)][s:s + n], r != 0, None, f"{kind} wire={wire} plain n={n}")
    # the proba sum is the sum of the kernel's own per-row outputs, rounded per row
    assert abs(int(c[3]) - int(np.round(p.astype(np.float64) * 1e6).sum())) <= n


@pytest.mark.parametrize("kind", ["mlp", "lr"])
@pytest.mark.parametrize("wire", [True, False])
@pytest.mark.parametrize("n", LAUNCH_SIZES)
def test_coalesced_launch_tile_epilogue_bucket_bounds(gpu, setup, kind, wire, n):
    """Four micro-batches of n rows in one coalesced launch."""
    _engine_case(gpu, setup, kind, wire, 4 * n, [(4, n)], batch=n, depth=4, streams=1,
                 exec_mode="launch", coalesce=4)
