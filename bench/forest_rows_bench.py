#!/usr/bin/env python3
"""Row formats of a general-tree ensemble through the streaming engine, one MI355X.

``StreamEngine`` in launch mode, batch 65536, rows read zero-copy from a pinned partition log:
the same forest (the 100 x depth-6 ensemble expanded into general trees, the one
profiles/forest/ uses) on f32 rows (120 B), G32 rows (32 B) and G20 rows (20 B).  What bounds
the f32 case is the PCIe link (4.6e8 rows/s for 120-byte rows, profiles/r1/roofline.json); the
binned rows move that ceiling to 1.73e9 and 2.87e9 rows/s.

    python bench/forest_rows_bench.py [--passes 2] [--batches 400] [--out profiles/forest/binned_rows.jsonl]

Every (pass, format) step is a fresh child process under its own time limit, formats
alternating within a pass; the first step that fails ends the run.  Raw JSON lines are appended
to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FORMATS = ("f32", "g32", "g20")
LINK_ROWS_PER_S = {"f32": 4.6e8, "g32": 1.73e9, "g20": 2.87e9}     # PCIe ceiling per row format


def step(args) -> dict:
    import numpy as np
    import torch
    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.models import TreeEnsemble, build_model
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel

    dev = torch.device("cuda", 0)
    X, _ = generate(args.log_rows, seed=3)
    m = TreeEnsemble.from_oblivious(build_model("gbdt", seed=0, X_ref=X[:100_000], calibrate_rate=0.01))
    dm = DeviceModel(m, dev, bins=None if args.step == "f32" else args.step)
    log = PartitionLog.from_arrays(X, ids=np.arange(args.log_rows, dtype=np.uint64), bins=dm.bins)
    eng = StreamEngine(dm, batch=args.batch, depth=args.depth, streams=2, input_mode="zerocopy",
                       output_mode="zerocopy", exec_mode="launch")
    try:
        eng.add_log(0, log)
        eng.pump(32, drain=True)                       # warm-up: code objects, the blob header, the log's pages
        eng.drain_flagged()
        eng.reset_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = eng.pump(args.batches, drain=True)
        dt = time.perf_counter() - t0
        flagged = len(eng.drain_flagged())
    finally:
        eng.close()
        log.free()
    rate = st.rows / dt
    return {"case": "forest_from_oblivious_100x6", "rows_format": args.step, "row_bytes": log.row_bytes,
            "mode": f"engine launch, zero-copy rows, batch {args.batch}, depth {args.depth}", "pass": args.rep,
            "trees": m.n_trees, "nodes": m.n_nodes, "rows": int(st.rows), "wall_s": round(dt, 4),
            "rows_per_s": round(rate, 1), "frac_of_link_ceiling": round(rate / LINK_ROWS_PER_S[args.step], 3),
            "p50_us": st.p50_us, "dev_exec_mean_us": st.dev_exec_mean_us, "flagged": flagged}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--batches", type=int, default=400)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--log-rows", type=int, default=1 << 21)
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds a (pass, format) step may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "forest" / "binned_rows.jsonl"))
    ap.add_argument("--step", choices=FORMATS, default=None, help="(child) run this one step and print its line")
    ap.add_argument("--rep", type=int, default=0)
    args = ap.parse_args()
    if args.step is not None:
        print(json.dumps(step(args)), flush=True)
        return 0
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for rep in range(args.passes):
        for fmt in FORMATS:
            cmd = [sys.executable, __file__, "--step", fmt, "--rep", str(rep), "--batches", str(args.batches),
                   "--batch", str(args.batch), "--depth", str(args.depth), "--log-rows", str(args.log_rows)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"step {fmt} pass {rep}: no result within {args.step_timeout:.0f} s; stopping", file=sys.stderr)
                return 124
            if r.returncode != 0:
                print(f"step {fmt} pass {rep} failed (rc={r.returncode}); stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return r.returncode if r.returncode > 0 else 1
            line = r.stdout.strip().splitlines()[-1]
            json.loads(line)
            print(line, flush=True)
            with out.open("a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
