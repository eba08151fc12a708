"""Oblivious-GBDT training on one GPU: torch scatter_add histograms vs the HIP histogram kernel
over G32 rows (train_oblivious_gbdt hist="torch" / "hip").

    python bench/train_gbdt_bench.py --rows 2000000 --trees 20 --depth 6 --bins 32

One worker process trains torch, hip, torch, hip on the same rows and borders (the second pair
runs with warm caches / allocator and is the one compared), then times the histogram kernel
alone at every level against the measured HBM read rate.  The driver starts no GPU work
itself: it reads the worker's progress line by line and ends it when a step outlives its own
time limit (--step-timeout).  Prints one JSON line and writes it to
profiles/train_gbdt/bench.json.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import queue
import subprocess
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
OUT_DIR = ROOT / "profiles" / "train_gbdt"
STEPS = ("setup", "torch_1", "hip_1", "torch_2", "hip_2", "levels")


def _emit(step: str, payload: dict) -> None:
    print("STEP " + json.dumps({"step": step, **payload}, default=float), flush=True)


def worker(a) -> int:
    import numpy as np
    import torch

    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.ops._lib import lib
    from ccfd_demo_summit_amd.ops.kernels import gbdt_histogram
    from ccfd_demo_summit_amd.train import evaluate, train_oblivious_gbdt
    from ccfd_demo_summit_amd.train.trainer import _encode_training_rows, _quantile_borders

    dev = torch.device("cuda")
    X, y = generate(a.rows, seed=1, fraud_rate=0.0172)
    Xv, yv = generate(50_000, seed=2, fraud_rate=0.0172)
    X = np.asarray(X, np.float32)
    borders = _quantile_borders(X, a.bins)
    # HBM read roofline: a 1 GiB buffer (4x the 256 MiB Infinity Cache) read by a plain kernel
    L = lib()
    L.ccfd_bw_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.ccfd_bw_probe.restype = C.c_double
    nbytes = 1 << 30
    src = torch.ones(nbytes // 4, dtype=torch.float32, device=dev)
    scratch = torch.empty(4096, dtype=torch.float32, device=dev)
    hbm = L.ccfd_bw_probe(C.c_void_p(src.data_ptr()), nbytes, 2, 10, C.c_void_p(scratch.data_ptr()))
    del src
    _emit("setup", {"hbm_read_GBps": round(hbm, 1), "device": torch.cuda.get_device_name(0)})

    models = {}
    for step in STEPS[1:5]:
        backend = step.split("_")[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, info = train_oblivious_gbdt(X, y, n_trees=a.trees, depth=a.depth, n_bins=a.bins, device="cuda",
                                       borders=borders, hist=backend)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert info["hist"] == backend
        models[backend] = m
        _emit(step, {"backend": backend, "seconds": round(dt, 4), "s_per_tree": round(dt / a.trees, 5),
                     "boost_s_per_tree": round(info["seconds_boost"] / a.trees, 5),
                     "train_logloss": round(info["train_logloss"], 6),
                     "roc_auc": round(evaluate(m, Xv, yv)["roc_auc"], 5)})

    # the histogram kernel alone, level by level, under the hip model's first tree
    rows = torch.from_numpy(_encode_training_rows(X, borders)).to(dev)
    yt = torch.from_numpy(np.asarray(y, np.float32)).to(dev)
    p = torch.full((a.rows,), float(np.clip(y.mean(), 1e-6, 1 - 1e-6)), device=dev)
    grad, hess = p - yt, (p * (1 - p)).clamp_min(1e-6)
    m = models["hip"]
    splits = [(int(f), int(np.searchsorted(borders[f], t, side="left"))) for f, t in zip(m.feat[0], m.thr[0])]
    bt = rows[:, :30].long()
    fidx = torch.arange(30, device=dev)
    levels = []
    for d in range(a.depth):
        def timed(fn, iters):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3)
            return float(np.median(ts))
        out = gbdt_histogram(rows, grad, hess, a.bins, splits[:d])
        t_hip = timed(lambda: gbdt_histogram(rows, grad, hess, a.bins, splits[:d], out=out), 20)
        leaf = torch.zeros(a.rows, dtype=torch.long, device=dev)
        for k, (f, b) in enumerate(splits[:d]):
            leaf |= (bt[:, f] > b).long() << k
        n_cells = (1 << d) * 30 * a.bins

        def scatter():
            key = ((leaf[:, None] * 30 + fidx[None, :]) * a.bins + bt).reshape(-1)
            torch.zeros(n_cells, device=dev).scatter_add_(0, key, grad[:, None].expand(a.rows, 30).reshape(-1))
            torch.zeros(n_cells, device=dev).scatter_add_(0, key, hess[:, None].expand(a.rows, 30).reshape(-1))
        t_torch = timed(scatter, 3)
        row_gbps = a.rows * 32 / t_hip / 1e9
        levels.append({"level": d, "hip_ms": round(t_hip * 1e3, 4), "torch_scatter_ms": round(t_torch * 1e3, 4),
                       "row_GBps": round(row_gbps, 1), "of_hbm_read": round(row_gbps / hbm, 4) if hbm > 0 else None})
    _emit("levels", {"levels": levels})
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds each step may take")
    ap.add_argument("--out", default=str(OUT_DIR / "bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)

    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--rows", str(a.rows), "--trees", str(a.trees),
           "--depth", str(a.depth), "--bins", str(a.bins)]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, cwd=str(ROOT))
    lines: "queue.Queue" = queue.Queue()

    def pump():
        for line in proc.stdout:
            lines.put(line)
        lines.put(None)
    threading.Thread(target=pump, daemon=True).start()

    steps, failed = {}, None
    for step in STEPS:
        deadline = time.monotonic() + a.step_timeout
        while step not in steps and failed is None:
            try:
                line = lines.get(timeout=max(0.0, deadline - time.monotonic()))
            except queue.Empty:
                failed = f"{step}: no result within {a.step_timeout:.0f} s"
                break
            if line is None:
                failed = f"{step}: worker ended (exit code {proc.wait()})"
            elif line.startswith("STEP "):
                rec = json.loads(line[5:])
                steps[rec.pop("step")] = rec
        if failed is not None:
            break
    if failed is not None:
        proc.kill()          # nothing more is started on the GPU after a step ran out of time or died
    rc = proc.wait()

    res = {"bench": "train_gbdt", "config": {"rows": a.rows, "trees": a.trees, "depth": a.depth, "bins": a.bins},
           **steps.pop("setup", {}), "runs": steps}
    if "levels" in steps:
        res["levels"] = steps.pop("levels")["levels"]
    if "torch_2" in steps and "hip_2" in steps:
        res["torch_s_per_tree"] = steps["torch_2"]["s_per_tree"]
        res["hip_s_per_tree"] = steps["hip_2"]["s_per_tree"]
        res["speedup"] = round(res["torch_s_per_tree"] / res["hip_s_per_tree"], 2)
        res["boost_speedup"] = round(steps["torch_2"]["boost_s_per_tree"] / steps["hip_2"]["boost_s_per_tree"], 2)
        res["roc_auc"] = {"torch": steps["torch_2"]["roc_auc"], "hip": steps["hip_2"]["roc_auc"]}
    if failed is not None:
        res["error"] = failed
    print(json.dumps(res), flush=True)
    try:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res) + "\n")
    except OSError as e:
        print(f"could not write {a.out}: {e}", file=sys.stderr)
    return 0 if failed is None and rc == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
