"""Sampled Shapley attributions of the MLP on W64 rows: the HIP kernel
(csrc/kernels/explain_mlp.hip) against the oracles of models/explain_mlp.py.

    python bench/explain_mlp_bench.py [--perms 64]

Measures rows/s of the kernel alone at n = 64, 4096 and 65536 W64 rows (median of event-timed
launches) with the MFMA FLOP/s it issues, the CPU oracle's rows/s, max |phi_gpu - phi_oracle|, and
the convergence of the estimator for P in {16, 64, 256} against ``shapley_mlp_exact`` on rows that
differ from the baseline in 10 positions (kernel attributions; max and median error, share of rows
whose top-3 positive reasons are the exact ones).  Prints one JSON line and writes it to
profiles/explain/mlp_bench.json.  Nothing here gates a test.
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

# one mlp_logit_w64_x2 call: 2 tiles x (8 + 16 + 2) MFMAs of 16 x 16 x 32, 2 FLOP a multiply-add
FLOP_PER_PERM = 2 * 26 * 2 * 16 * 16 * 32
PEAK_BF16_FLOPS = 2.5e15              # MI355X dense bf16
FLAGGED_ROWS_PER_S_CONFIG2 = 1.5e6    # 8.9e8 tx/s at a 0.17 % fraud rate


def top3(phi_row):
    import numpy as np
    order = np.argsort(-phi_row, kind="stable")[:3]
    return tuple(int(j) for j in order if phi_row[j] > 0)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--perms", type=int, default=64)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 4096, 65536])
    ap.add_argument("--oracle-rows", type=int, default=64)
    ap.add_argument("--convergence-rows", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=str(OUT_DIR / "mlp_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from ccfd_demo_summit_amd.contracts.transaction import N_FEATURES, encode_wire
    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.models.explain_mlp import shapley_mlp_exact, shapley_mlp_sampled
    from ccfd_demo_summit_amd.ops.kernels import DeviceMlpExplainer, explain_mlp

    dev = torch.device("cuda")
    X, _ = generate(max(a.sizes), seed=1)
    X = np.asarray(X, np.float32)
    bg, _ = generate(50_000, seed=2)
    model = build_model("mlp", seed=0, X_ref=bg, calibrate_rate=0.0017).fit_baseline(bg, "median")
    ex = DeviceMlpExplainer(model, perms=a.perms, seed=0, device=dev)
    rows_all = torch.from_numpy(encode_wire(X)).to(dev)

    res = {"bench": "explain_mlp", "device": torch.cuda.get_device_name(0),
           "config": {"perms": a.perms, "seed": 0, "baseline": "median of 50000 rows"}, "kernel": []}
    for n in a.sizes:
        rows = rows_all[:n].contiguous()
        out = explain_mlp(ex, rows)                       # warm-up, and the buffer of the timed runs
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            explain_mlp(ex, rows, out=out)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        med = float(np.median(ts))
        flops = n * a.perms * FLOP_PER_PERM / med
        res["kernel"].append({"n": n, "ms_median": round(med * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4),
                              "rows_per_s": round(n / med, 1), "mfma_flops": round(flops, 1),
                              "share_of_bf16_peak": round(flops / PEAK_BF16_FLOPS, 4),
                              "vs_flagged_rows_config2": round(n / med / FLAGGED_ROWS_PER_S_CONFIG2, 3)})

    k = a.oracle_rows
    t0 = time.perf_counter()
    want, _bv = shapley_mlp_sampled(model, X[:k], a.perms, 0)
    res["oracle_cpu_s"] = round(time.perf_counter() - t0, 4)
    res["oracle_rows"] = k
    res["oracle_rows_per_s"] = round(k / res["oracle_cpu_s"], 1)
    got = explain_mlp(ex, rows_all[:k].contiguous()).cpu().numpy().astype(np.float64)
    res["max_abs_dphi"] = float(np.abs(got - want).max())
    res["max_abs_phi"] = float(np.abs(want).max())
    res["flagged_rows_per_s_config2"] = FLAGGED_ROWS_PER_S_CONFIG2

    # convergence: rows that differ from the baseline in 10 features, against enumeration
    rng = np.random.default_rng(7)
    Xc = np.tile(model.baseline, (a.convergence_rows, 1))
    for r in Xc:
        f = rng.choice(N_FEATURES, 10, replace=False)
        r[f] = X[rng.integers(len(X)), f]
    exact = np.stack([shapley_mlp_exact(model, x) for x in Xc])
    rows_c = torch.from_numpy(encode_wire(Xc)).to(dev)
    res["convergence"] = []
    for P in (16, 64, 256):
        exp = DeviceMlpExplainer(model, perms=P, seed=0, device=dev)
        phi = explain_mlp(exp, rows_c).cpu().numpy().astype(np.float64)
        err = np.abs(phi - exact)
        same = np.mean([top3(phi[i]) == top3(exact[i]) for i in range(len(Xc))])
        res["convergence"].append({"perms": P, "rows": len(Xc), "max_abs_err": float(err.max()),
                                   "median_abs_err": float(np.median(err[exact != 0])),
                                   "median_abs_phi": float(np.median(np.abs(exact[exact != 0]))),
                                   "top3_equal_share": round(float(same), 4)})
    print(json.dumps(res), flush=True)
    try:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res) + "\n")
    except OSError as e:
        print(f"could not write {a.out}: {e}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
