"""bench.py end to end on one MI355X: the JSON contract the driver parses, a sustained
timed region, exact row accounting, per-rank attribution and precision evidence."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _run(args, env=None, timeout=240):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_json_contract(gpu):
    r = _run(["--full", "--steps", "5", "--warmup", "2", "--min-timed-s", "0.3", "--log-rows", str(1 << 20),
              "--precision-rows", str(1 << 18)])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["dtype"] == "bf16"
    assert d["timed_region_s"] >= 0.3
    assert d["rows_scored"] == d["rows_expected"]
    assert abs(d["value"] * d["timed_region_s"] - d["rows_scored"]) / d["rows_scored"] < 1e-3
    assert d["backend"] in ("none", "nccl") and not d["rehearsal"]
    assert len(d["per_rank"]) == 1 and d["per_rank"][0]["rows"] == d["rows_scored"]
    assert d["per_rank"][0]["h2d_zerocopy_GBps"] > 1
    pr = d["precision_vs_fp32"]
    assert pr["rows"] == 1 << 18 and pr["max_abs_dp"] < 1e-2 and pr["route_flips_outside_1e-2_band"] == 0
    assert d["f32_wire_tx_s"] > 0


def test_bench_plain_run_is_lean_and_dumps_its_outputs(gpu, tmp_path):
    """Without --full the line keeps its headline fields and leaves the side measurements null;
    --dump-outputs writes the last timed step's hand-off, consistent with the route array."""
    import numpy as np
    r = _run(["--steps", "3", "--warmup", "1", "--min-timed-s", "0.2", "--log-rows", str(1 << 18),
              "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["unit"] == "tx/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert abs(d["ms_per_step"] * 3 - d["timed_region_s"] * 1e3) < 0.01 * d["timed_region_s"] * 1e3
    assert d["rows_scored"] == d["rows_expected"] and d["flagged_handed_off"] == d["fraud_routed"]
    for k in ("precision_vs_fp32", "f32_wire_tx_s", "host_encode", "p50_latency_us_unloaded",
              "h2d_zerocopy_ceiling_tx_s_rank0", "host_dram_ceiling_tx_s"):
        assert d[k] is None, k
    # every step replays the whole log (twice over), whatever the calibration chose
    assert d["config"]["batches_per_step"] >= 2 * (1 << 18) // 4096
    out = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(out) == {"route", "flagged_tx_id", "flagged_partition", "flagged_customer",
                        "flagged_proba", "flagged_amount"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert out["route"].shape == (1 << 18,) and set(np.unique(out["route"])) <= {0.0, 1.0}
    n = len(out["flagged_tx_id"])
    assert 0 < n == int(out["route"].sum()) and np.all(np.diff(out["flagged_tx_id"]) > 0)
    assert np.all(out["flagged_proba"] >= 0.5) and np.all(out["flagged_proba"] <= 1.0)


def test_bench_refuses_gpu_count_mismatch(gpu):
    # an explicit WORLD_SIZE that disagrees with --gpus is refused, never re-launched
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"],
             env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr, r.stderr[-2000:]
    import torch
    if torch.cuda.device_count() < 2:
        # --gpus 2 self-spawns two ranks (launch/local_ranks.py); on a one-GPU box the second
        # rank refuses with a clear message and the parent exits non-zero
        r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"])
        assert r.returncode != 0 and "visible GPU" in r.stderr, r.stderr[-2000:]
