"""The W64 drift kernel (csrc/kernels/drift_wire.hip) on one GPU.

    python bench/drift_wire_bench.py --rows 2000000

On HBM-resident W64 rows of the synthetic data against their own 32-cell quantile table:
`drift_histogram_wire` as the median of --iters launches timed with device events after a
warm-up, rows/s and row-bytes/s against the measured HBM read rate, and -- in the same process,
on the same data, alternating with it -- `drift_histogram` on G20 rows (for scale: it counts
bins that are already there) and a torch composite that produces the same counts on the device
(bf16 -> float, `torch.bucketize(right=False)` per column, offset, `bincount`), the only way to
get these counts without the kernel.  Then `DriftMonitor.observe_host` on 64-byte rows: copy
into pinned staging plus launch, one thread.  A run without a GPU fails.  Prints one JSON line
and writes it to profiles/drift/wire_bench.json.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
OUT_DIR = ROOT / "profiles" / "drift"
INGEST_TX_S = (1.1e7, 1.19e7)        # the in-process ingest rate the README gives


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-workgroups", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--host-seconds", type=float, default=1.0, help="least duration of each observe_host measurement")
    ap.add_argument("--out", default=str(OUT_DIR / "wire_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from ccfd_demo_summit_amd.contracts.metric_names import AMOUNT_BUCKETS
    from ccfd_demo_summit_amd.contracts.transaction import encode_wire
    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models.drift import DriftReference, bin_counts, wire_bin_counts, wire_bins_fit
    from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
    from ccfd_demo_summit_amd.ops._lib import lib
    from ccfd_demo_summit_amd.ops.kernels import (DRIFT_WIRE_MAX_WORKGROUPS, DriftMonitor, drift_histogram,
                                                  drift_histogram_wire, drift_wire_table, new_drift_counts)
    if not torch.cuda.is_available():
        print("drift_wire_bench needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda")
    X, _ = generate(a.rows, seed=1)
    bins = wire_bins_fit(X, cells=32)
    g20 = ObliviousGBDT.random_init(100, 6, 0, X[:50_000]).bin_spec(bits=5)
    host = encode_wire(X)
    host20 = np.ascontiguousarray(g20.encode(X))
    rows, rows20 = torch.from_numpy(host).to(dev), torch.from_numpy(host20).to(dev)
    table = drift_wire_table(bins, dev)

    # HBM read roofline: a 1 GiB buffer (4x the 256 MiB Infinity Cache) read by a plain kernel
    L = lib()
    L.ccfd_bw_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.ccfd_bw_probe.restype = C.c_double
    nbytes = 1 << 30
    src = torch.ones(nbytes // 4, dtype=torch.float32, device=dev)
    scratch = torch.empty(4096, dtype=torch.float32, device=dev)
    hbm = L.ccfd_bw_probe(C.c_void_p(src.data_ptr()), nbytes, 2, 10, C.c_void_p(scratch.data_ptr()))
    del src

    # the torch composite: the same [31][32] cells from stock operators (no NaN in these rows:
    # bucketize puts NaN past the last edge, where the definition puts it in cell 0)
    edges_dev = [torch.from_numpy(e).to(dev) for e in bins.edges]
    bounds_dev = torch.tensor(AMOUNT_BUCKETS, dtype=torch.float32, device=dev)

    def composite() -> torch.Tensor:
        v = rows.view(torch.bfloat16)[:, :28].float().t().contiguous()        # [28, n]: contiguous columns
        f = rows.view(torch.float32)[:, 14:].t().contiguous()                  # Time, Amount
        cols = [f[0]] + [v[k] for k in range(28)] + [f[1]]
        idx = [torch.bucketize(c, e, right=False) + 32 * j for j, (c, e) in enumerate(zip(cols, edges_dev))]
        idx.append(torch.bucketize(f[1], bounds_dev, right=False) + 32 * 30)
        return torch.bincount(torch.cat(idx), minlength=31 * 32)

    def event_time(fn) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def stats(ts, row_bytes):
        ts = np.sort(np.asarray(ts))
        med = float(np.median(ts))
        gbps = a.rows * row_bytes / med / 1e9
        return {"median_ms": round(med * 1e3, 4), "min_ms": round(float(ts[0]) * 1e3, 4),
                "p90_ms": round(float(ts[int(0.9 * (len(ts) - 1))]) * 1e3, 4), "rows_per_s": round(a.rows / med, 0),
                "row_GBps": round(gbps, 1), "of_hbm_read": round(gbps / hbm, 4) if hbm > 0 else None}

    res = {"bench": "drift_wire", "device": torch.cuda.get_device_name(0), "rows": a.rows, "iters": a.iters,
           "cells": 32, "edges": [int(e.size) for e in bins.edges], "hbm_read_GBps": round(hbm, 1), "kernel": {}}
    # the counts agree before anything is timed: the kernel and the composite with the oracle
    want, want_tail = wire_bin_counts(host, bins)
    c, t = drift_histogram_wire(rows, table)
    if not (np.array_equal(c.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), want_tail)):
        print("drift_histogram_wire counts differ from the oracle", file=sys.stderr)
        return 3
    if not np.array_equal(composite().cpu().numpy().reshape(31, 32).astype(np.uint64), want[:, :32]):
        print("the torch composite's counts differ from the oracle", file=sys.stderr)
        return 3
    c, t = drift_histogram(rows20, g20.stamp)
    if not np.array_equal(c.cpu().numpy(), bin_counts(host20, g20.stamp)[0]):
        print("drift_histogram (G20) counts differ from the oracle", file=sys.stderr)
        return 3

    counts, tail = new_drift_counts(dev)
    for mw in a.max_workgroups:
        fns = {"drift_wire_w64": lambda: drift_histogram_wire(rows, table, counts, tail, mw),
               "drift_g20": lambda: drift_histogram(rows20, g20.stamp, counts, tail, mw),
               "torch_composite_w64": composite}
        ts = {k: [] for k in fns}
        for i in range(a.warmup + a.iters):              # alternating: the three share whatever else runs
            for k, fn in fns.items():
                dt = event_time(fn)
                if i >= a.warmup:
                    ts[k].append(dt)
        rb = {"drift_wire_w64": 64, "drift_g20": 20, "torch_composite_w64": 64}
        res["kernel"][str(mw)] = {k: stats(v, rb[k]) for k, v in ts.items()}
    best = min(res["kernel"], key=lambda k: res["kernel"][k]["drift_wire_w64"]["median_ms"])
    res["default_max_workgroups"] = DRIFT_WIRE_MAX_WORKGROUPS
    d = res["kernel"].get(str(DRIFT_WIRE_MAX_WORKGROUPS), res["kernel"][best])
    res["wire_vs_torch_composite"] = round(d["torch_composite_w64"]["median_ms"] / d["drift_wire_w64"]["median_ms"], 3)
    res["wire_vs_g20"] = round(d["drift_wire_w64"]["median_ms"] / d["drift_g20"]["median_ms"], 3)
    res["best_max_workgroups"] = int(best)

    # observe_host: one thread copies 64-byte rows into pinned staging and launches over them
    ref = DriftReference.fit_wire(X[:20_000], bins=bins)
    mon = DriftMonitor(ref, dev)
    chunk = 4096
    for lo in range(0, 64 * chunk, chunk):               # warm-up
        mon.observe_host(host[lo:lo + chunk])
    mon.report(reset=True)
    per = {}
    for chunk in (4096, 65536):
        n, passes = 0, 0
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.host_seconds:     # whole passes over the rows, back to back
            for lo in range(0, (a.rows // chunk) * chunk, chunk):
                mon.observe_host(host[lo:lo + chunk])
                n += chunk
            passes += 1
        rows_seen = mon.report(reset=True).rows          # synchronises the monitor's stream
        dt = time.perf_counter() - t0
        if rows_seen != n:
            print(f"observe_host counted {rows_seen} of {n} rows", file=sys.stderr)
            return 3
        per[str(chunk)] = {"rows": n, "passes": passes, "seconds": round(dt, 4), "rows_per_s": round(n / dt, 0),
                           "us_per_call": round(dt / (n // chunk) * 1e6, 2)}
    mon.close()
    res["observe_host_w64"] = per
    res["ingest_tx_per_s"] = list(INGEST_TX_S)
    res["observe_host_4096_vs_ingest"] = round(per["4096"]["rows_per_s"] / INGEST_TX_S[1], 2)

    print(json.dumps(res), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
