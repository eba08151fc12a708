"""What the MLP / LR kernels do with a scored 16-row tile (tile_core.h): outputs, route,
counters, BOTH amount histograms per bucket and the flag list -- on the claimed and pipelined
persistent kernels and on plain and coalesced launches, f32 and W64 rows, with row amounts ON
the histogram's bucket bounds (each bound, one float32 ulp below and above it, and 0)."""
import numpy as np
import pytest
import torch

from tests.helpers import tile_cases
from tests.helpers.tile_cases import EDGE_AMOUNTS, N_PERSIST
from tests.helpers.tile_cases import check as _check
from tests.helpers.tile_cases import engine_case as _engine_case

pytestmark = pytest.mark.gpu

LAUNCH_SIZES = [1, 15, 17, 65, 1025]


@pytest.fixture(scope="module")
def setup(gpu):
    """Rows whose amounts cycle through EDGE_AMOUNTS, both models, and each model's oracle on
    f32 and on W64 rows -- computed once, read-only (tests/helpers/tile_cases.py)."""
    return tile_cases.build_setup()


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
