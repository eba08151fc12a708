"""Exact Shapley attributions of the 100 x depth 6 oblivious GBDT: the HIP kernel
(csrc/kernels/explain_gbdt.hip) against the float64 oracle (models/explain.py).

    python bench/explain_bench.py [--trees 100 --depth 6]

Measures rows/s of the kernel alone at n = 4096 and n = 65536 G32 rows (median of event-timed
launches), the oracle's CPU time on 256 rows, and max |phi_gpu - phi_f64| on those rows (also
in units u = 2^-24 * sum_t max_l |leaves[t, l]|).  Prints one JSON line and writes it to
profiles/explain/bench.json.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
OUT_DIR = ROOT / "profiles" / "explain"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--oracle-rows", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=str(OUT_DIR / "bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models.explain import shapley_oblivious
    from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
    from ccfd_demo_summit_amd.ops.kernels import DeviceExplainer, explain_gbdt

    dev = torch.device("cuda")
    X, _ = generate(max(a.sizes), seed=1)
    X = np.asarray(X, np.float32)
    bg, _ = generate(50_000, seed=2)
    model = ObliviousGBDT.random_init(a.trees, a.depth, seed=0, X_ref=bg).fit_cover(bg)
    ex = DeviceExplainer(model, device=dev)
    rows_all = torch.from_numpy(ex.bins.encode(X)).to(dev)
    u = 2.0 ** -24 * float(np.abs(model.leaves).max(1).astype(np.float64).sum())

    res = {"bench": "explain_gbdt", "device": torch.cuda.get_device_name(0),
           "config": {"trees": a.trees, "depth": a.depth, "empty_leaves": int((model.cover == 0).sum())},
           "kernel": []}
    for n in a.sizes:
        rows = rows_all[:n].contiguous()
        out = explain_gbdt(ex, rows)                      # warm-up, and the buffer of the timed runs
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            explain_gbdt(ex, rows, out=out)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        med = float(np.median(ts))
        res["kernel"].append({"n": n, "ms_median": round(med * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4),
                              "rows_per_s": round(n / med, 1)})

    k = a.oracle_rows
    t0 = time.perf_counter()
    want, _bv = shapley_oblivious(model, X[:k])
    res["oracle_cpu_s"] = round(time.perf_counter() - t0, 4)
    res["oracle_rows"] = k
    res["oracle_rows_per_s"] = round(k / res["oracle_cpu_s"], 1)
    got = explain_gbdt(ex, rows_all[:k].contiguous()).cpu().numpy().astype(np.float64)
    res["max_abs_dphi"] = float(np.abs(got - want).max())
    res["max_abs_dphi_u"] = round(res["max_abs_dphi"] / u, 4)
    res["flagged_rows_per_s_config4"] = 5.0e6             # ~2.7e9 tx/s at a 0.17 % fraud rate
    print(json.dumps(res), flush=True)
    try:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res) + "\n")
    except OSError as e:
        print(f"could not write {a.out}: {e}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
