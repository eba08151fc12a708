"""The autoencoder outlier kernel (csrc/kernels/outlier_ae.hip) on one GPU.

    python bench/outlier_bench.py

On HBM-resident W64 rows of the synthetic data (65 536 and 2 M rows) with a He-init 30-64-8-64-30
autoencoder: `outlier_scores` (scores and counts, no residual output) as the median of --iters
launches timed with device events after a warm-up, and -- in the same process, on the same rows,
alternating with it -- a torch composite of the same network (decode W64 on the device, normalise,
a bf16 linear chain, mean squared residual) and `drift_histogram_wire` (for scale: the other
monitor of W64 rows).  Then `OutlierMonitor.observe_host` in 4096-row chunks: copy into pinned
staging plus launch, one thread, next to the in-process ingest rate.  A run without a GPU fails.
Prints one JSON line and writes it to profiles/outlier/bench.json.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
OUT_DIR = ROOT / "profiles" / "outlier"
INGEST_TX_S = (1.1e7, 1.19e7)        # the in-process ingest rate the README gives


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[65_536, 2_000_000])
    ap.add_argument("--latent", type=int, default=8)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-seconds", type=float, default=1.0, help="least duration of the observe_host measurement")
    ap.add_argument("--out", default=str(OUT_DIR / "bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from ccfd_demo_summit_amd.contracts.transaction import WIRE_PERM, encode_wire
    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models.common import Normalizer
    from ccfd_demo_summit_amd.models.drift import wire_bins_fit
    from ccfd_demo_summit_amd.models.outlier import OutlierAE, recount
    from ccfd_demo_summit_amd.ops.kernels import (OUTLIER_MAX_WORKGROUPS, DeviceOutlierModel, OutlierMonitor,
                                                  drift_histogram_wire, drift_wire_table, new_drift_counts,
                                                  new_outlier_counts, outlier_scores)
    if not torch.cuda.is_available():
        print("outlier_bench needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda")
    n_max = max(a.rows)
    X, _ = generate(n_max, seed=1)
    model = OutlierAE.random_init(a.latent, seed=0, norm=Normalizer.fit(X[:50_000]))
    model.fit_threshold(X[:50_000], 0.999)
    host = encode_wire(X)
    rows_all = torch.from_numpy(host).to(dev)
    dm = DeviceOutlierModel(model, dev)
    table = drift_wire_table(wire_bins_fit(X[:200_000], cells=32), dev)

    # the torch composite: the same network from stock operators on the device
    mu = torch.from_numpy(model.norm.mu[WIRE_PERM]).to(dev)
    isg = torch.from_numpy(model.norm.inv_sigma[WIRE_PERM]).to(dev)
    Ws = [torch.from_numpy(np.ascontiguousarray(w)).to(dev).bfloat16()
          for w in (model.W1[:, WIRE_PERM], model.W2, model.W3, model.W4[WIRE_PERM])]
    bs = [torch.from_numpy(np.ascontiguousarray(b)).to(dev).bfloat16()
          for b in (model.b1, model.b2, model.b3, model.b4[WIRE_PERM])]
    log_amount = model.norm.log_amount

    def composite(rows: torch.Tensor) -> torch.Tensor:
        v = rows.view(torch.bfloat16)[:, :28].float()
        f = rows.view(torch.float32)[:, 14:]
        am = torch.log1p(f[:, 1].clamp_min(0)) if log_amount else f[:, 1]
        xn = (torch.cat([v, f[:, :1], am[:, None]], dim=1) - mu) * isg
        h = xn.bfloat16()
        for k in range(3):
            h = torch.relu(torch.nn.functional.linear(h, Ws[k], bs[k]))
        r = torch.nn.functional.linear(h, Ws[3], bs[3]).float() - xn
        return (r * r).mean(dim=1)

    def event_time(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def stats(ts, n):
        ts = np.sort(np.asarray(ts))
        med = float(np.median(ts))
        return {"median_ms": round(med * 1e3, 4), "min_ms": round(float(ts[0]) * 1e3, 4),
                "p90_ms": round(float(ts[int(0.9 * (len(ts) - 1))]) * 1e3, 4), "rows_per_s": round(n / med, 0),
                "row_GBps": round(n * 64 / med / 1e9, 1)}

    res = {"bench": "outlier_ae", "device": torch.cuda.get_device_name(0), "latent": a.latent, "iters": a.iters,
           "max_workgroups": OUTLIER_MAX_WORKGROUPS, "kernel": {}}
    # before anything is timed: the kernel's counts equal the recount of its own outputs, and the
    # composite agrees with it to bf16 accuracy
    k = min(n_max, 65_536)
    resid = torch.empty((k, 32), dtype=torch.float32, device=dev)
    counts = new_outlier_counts(dev)
    score = outlier_scores(dm, rows_all[:k], None, resid, counts)
    got = counts.view(torch.int64).cpu().numpy().view(np.uint64)
    if not np.array_equal(got, recount(score.cpu().numpy(), resid.cpu().numpy(), model.threshold)):
        print("outlier_scores counts differ from the recount of its own scores", file=sys.stderr)
        return 3
    rel = ((composite(rows_all[:k]) - score).abs() / score.abs().clamp_min(1e-6)).median().item()
    res["composite_median_rel_diff"] = round(rel, 5)
    if not rel < 0.05:
        print(f"the torch composite is {rel} (median, relative) off the kernel", file=sys.stderr)
        return 3

    for n in a.rows:
        rows = rows_all[:n]
        out = torch.empty(n, dtype=torch.float32, device=dev)
        oc = new_outlier_counts(dev)
        dc, dt_ = new_drift_counts(dev)
        fns = {"outlier_ae_w64": lambda: outlier_scores(dm, rows, out, None, oc),
               "torch_composite_w64": lambda: composite(rows),
               "drift_wire_w64": lambda: drift_histogram_wire(rows, table, dc, dt_)}
        ts = {name: [] for name in fns}
        for i in range(a.warmup + a.iters):              # alternating: the three share whatever else runs
            for name, fn in fns.items():
                dt = event_time(fn)
                if i >= a.warmup:
                    ts[name].append(dt)
        r = {name: stats(v, n) for name, v in ts.items()}
        r["ae_vs_torch_composite"] = round(r["torch_composite_w64"]["median_ms"] / r["outlier_ae_w64"]["median_ms"], 3)
        r["ae_vs_drift_wire"] = round(r["outlier_ae_w64"]["median_ms"] / r["drift_wire_w64"]["median_ms"], 3)
        res["kernel"][str(n)] = r

    # observe_host: one thread copies 64-byte rows into pinned staging and launches over them
    mon = OutlierMonitor(dm, dev)
    chunk = 4096
    for lo in range(0, min(64 * chunk, (n_max // chunk) * chunk), chunk):               # warm-up
        mon.observe_host(host[lo:lo + chunk])
    mon.report(reset=True)
    n, passes = 0, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.host_seconds:     # whole passes over the rows, back to back
        for lo in range(0, (n_max // chunk) * chunk, chunk):
            mon.observe_host(host[lo:lo + chunk])
            n += chunk
        passes += 1
    rows_seen = mon.report(reset=True).rows              # synchronises the monitor's stream
    dt = time.perf_counter() - t0
    mon.close()
    if rows_seen != n:
        print(f"observe_host counted {rows_seen} of {n} rows", file=sys.stderr)
        return 3
    res["observe_host_w64"] = {"4096": {"rows": n, "passes": passes, "seconds": round(dt, 4),
                                        "rows_per_s": round(n / dt, 0), "us_per_call": round(dt / (n // chunk) * 1e6, 2)}}
    res["ingest_tx_per_s"] = list(INGEST_TX_S)
    res["observe_host_4096_vs_ingest"] = round(n / dt / INGEST_TX_S[1], 2)

    print(json.dumps(res), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
