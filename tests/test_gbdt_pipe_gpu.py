"""Pipelined static items of the persistent binned-GBDT scorer (persist_items="pipelined":
csrc/kernels/score_gbdt_g32_persist.hip persist_gbdt_pipe_kernel) on G32 and G20 rows, at the
smallest shapes that run the kernel's own logic: four 512-row items a micro-batch over three
workers (a worker's consecutive items fall in different micro-batches and ring slots, both
halves of the two-stage loop run), then 1300-row micro-batches (1300 = 2 x 512 + 276: one
partial item and one item with no rows).  Checks are those of
test_gbdt_g32_gpu.py::test_g32_persistent_item_modes_exact."""
import numpy as np
import pytest
import torch

from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models import build_model

pytestmark = pytest.mark.gpu

B = 2048
N = 3 * B + 2 * 1300


@pytest.fixture(scope="module")
def case():
    X, _ = generate(N + 500, seed=61)
    m = build_model("gbdt", seed=16, X_ref=X, calibrate_rate=0.05)
    assert m.bin_spec().fits_g20, "test ensemble must fit 5-bit bins"
    return X, m, m.predict_proba(X[:N])


def _pump(gpu, dm, X, rules=None):
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    eng = StreamEngine(dm, batch=B, depth=3, streams=1, exec_mode="persistent", persist_items="pipelined",
                       persist_grid=4, rules=rules)
    log = PartitionLog.from_arrays(X, ids=np.arange(X.shape[0], dtype=np.uint64) + 7, bins=dm.bins)
    eng.add_log(0, log)
    assert eng.pump(3).rows + eng.pump(2, batch_rows=1300).rows == N
    fl = eng.drain_flagged()
    got = np.zeros(N, bool)
    got[(fl["tx_id"] - 7).astype(np.int64)] = True
    side = torch.cuda.Stream(gpu)
    c = eng.flip_epoch(side)
    side.synchronize()
    eng.close()
    log.free()
    return got, c.cpu().numpy()


@pytest.mark.parametrize("fmt", ["g32", "g20"])
def test_pipelined_items_exact(gpu, case, fmt):
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    X, m, pr = case
    dm = DeviceModel(m, gpu, bins=True if fmt == "g32" else "g20")
    assert dm.row_format == fmt
    got, c = _pump(gpu, dm, X)
    np.testing.assert_array_equal(got, pr >= 0.5)
    assert c[0] == N and c[1] == (pr >= 0.5).sum() and c[4] == 0
    assert abs(int(c[3]) - float(np.round(pr.astype(np.float64) * 1e6).sum())) <= N
    assert int(c[8:22].sum() + c[24:38].sum()) == N


def test_pipelined_items_with_proba_rules(gpu, case):
    """The kernel's kR instantiation: a probability-only rule set routes every row like
    RuleSet.evaluate (rows within fp32 summation order of a rule's edge excepted)."""
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, DeviceRules
    from ccfd_demo_summit_amd.router.rules import RuleSet
    X, m, pr = case
    rs = RuleSet.parse("when proba >= 0.8 then fraud\nwhen proba < 0.001 then fraud\notherwise standard")
    got, c = _pump(gpu, DeviceModel(m, gpu, bins=True), X, rules=DeviceRules(rs, gpu))
    want = rs.evaluate(pr).astype(bool)
    clear = (np.abs(pr - 0.8) > 1e-5) & (np.abs(pr - 0.001) > 1e-6)
    np.testing.assert_array_equal(got[clear], want[clear])
    assert c[0] == N and c[1] == got.sum() and c[4] == 0
    assert int(c[8:22].sum() + c[24:38].sum()) == N
