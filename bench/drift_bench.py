"""The drift bin-count kernel (csrc/kernels/drift_hist.hip) on one GPU.

    python bench/drift_bench.py --rows 2000000

On HBM-resident G32 and G20 rows of the synthetic data against the table of a 100 x 6 ensemble:
`drift_histogram` as the median of --iters launches timed with device events after a warm-up,
rows/s and row-bytes/s against the measured HBM read rate, and -- in the same process, on the
same G32 rows, alternating with it -- `gbdt_histogram(level 0, grad = hess = 1, n_bins = 32)`,
the only way to get these counts without the kernel.  Then `DriftMonitor.observe_host` on
20-byte rows: copy into pinned staging plus launch, one thread.  A run without a GPU fails.
Prints one JSON line and writes it to profiles/drift/bench.json.
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-workgroups", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--host-seconds", type=float, default=1.0, help="least duration of each observe_host measurement")
    ap.add_argument("--out", default=str(OUT_DIR / "bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models.drift import DriftReference, bin_counts
    from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
    from ccfd_demo_summit_amd.ops._lib import lib
    from ccfd_demo_summit_amd.ops.kernels import DriftMonitor, drift_histogram, gbdt_histogram, new_drift_counts
    if not torch.cuda.is_available():
        print("drift_bench needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda")
    X, _ = generate(a.rows, seed=1)
    model = ObliviousGBDT.random_init(100, 6, 0, X[:50_000])
    bins = {"g32": model.bin_spec(), "g20": model.bin_spec(bits=5)}
    host = {f: np.ascontiguousarray(b.encode(X)) for f, b in bins.items()}
    rows = {f: torch.from_numpy(h).to(dev) for f, h in host.items()}

    # HBM read roofline: a 1 GiB buffer (4x the 256 MiB Infinity Cache) read by a plain kernel
    L = lib()
    L.ccfd_bw_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.ccfd_bw_probe.restype = C.c_double
    nbytes = 1 << 30
    src = torch.ones(nbytes // 4, dtype=torch.float32, device=dev)
    scratch = torch.empty(4096, dtype=torch.float32, device=dev)
    hbm = L.ccfd_bw_probe(C.c_void_p(src.data_ptr()), nbytes, 2, 10, C.c_void_p(scratch.data_ptr()))
    del src

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

    res = {"bench": "drift", "device": torch.cuda.get_device_name(0), "rows": a.rows, "iters": a.iters,
           "hbm_read_GBps": round(hbm, 1), "kernel": {}}
    counts, tail = new_drift_counts(dev)
    grad = torch.ones(a.rows, dtype=torch.float32, device=dev)
    out = gbdt_histogram(rows["g32"], grad, grad, 32)
    # the counts agree before anything is timed: the new kernel with the oracle, the old one with both
    for f in bins:
        c, t = drift_histogram(rows[f], bins[f].stamp)
        wc, wt = bin_counts(host[f], bins[f].stamp)
        if not (np.array_equal(c.cpu().numpy(), wc) and np.array_equal(t.cpu().numpy(), wt)):
            print(f"{f}: counts differ from the oracle", file=sys.stderr)
            return 3
    G = out[0][0].cpu().numpy()
    if not np.array_equal(G.astype(np.uint64), bin_counts(host["g32"], bins["g32"].stamp)[0][:30, :32]):
        print("gbdt_histogram counts differ from the oracle", file=sys.stderr)
        return 3

    for mw in a.max_workgroups:
        fns = {"drift_g32": lambda: drift_histogram(rows["g32"], bins["g32"].stamp, counts, tail, mw),
               "drift_g20": lambda: drift_histogram(rows["g20"], bins["g20"].stamp, counts, tail, mw),
               "gbdt_histogram_g32": lambda: gbdt_histogram(rows["g32"], grad, grad, 32, out=out)}
        ts = {k: [] for k in fns}
        for i in range(a.warmup + a.iters):              # alternating: the three share whatever else runs
            for k, fn in fns.items():
                t = event_time(fn)
                if i >= a.warmup:
                    ts[k].append(t)
        rb = {"drift_g32": 32, "drift_g20": 20, "gbdt_histogram_g32": 32}
        res["kernel"][str(mw)] = {k: stats(v, rb[k]) for k, v in ts.items()}
    best = min(res["kernel"], key=lambda k: res["kernel"][k]["drift_g32"]["median_ms"])
    res["default_max_workgroups"] = 512
    d = res["kernel"]["512" if "512" in res["kernel"] else best]
    res["g32_vs_gbdt_histogram"] = round(d["gbdt_histogram_g32"]["median_ms"] / d["drift_g32"]["median_ms"], 3)
    res["best_max_workgroups_g32"] = int(best)

    # observe_host: one thread copies 20-byte rows into pinned staging and launches over them
    ref = DriftReference.from_counts(bins["g20"], np.zeros((31, 256), np.uint64), 0)
    mon = DriftMonitor(ref, dev)
    chunk = 4096
    for lo in range(0, 64 * chunk, chunk):               # warm-up
        mon.observe_host(host["g20"][lo:lo + chunk])
    mon.report(reset=True)
    per = {}
    for chunk in (4096, 65536):
        n, passes = 0, 0
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.host_seconds:     # whole passes over the rows, back to back
            for lo in range(0, (a.rows // chunk) * chunk, chunk):
                mon.observe_host(host["g20"][lo:lo + chunk])
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
    res["observe_host_g20"] = per

    print(json.dumps(res), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
