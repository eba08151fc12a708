"""What a shadow (challenger) MLP costs the streaming engine: shadow off / on legs, alternated
in one process on one engine per exec mode, with bench.py config 2's engine settings (MLP on W64
rows, micro-batch 4096, depth 12, zero-copy in both directions, flagged ring drained by a
collector thread).

    python bench/shadow_ab.py --out profiles/shadow [--seconds 4] [--rounds 2]

Writes one JSON line per leg (tx/s, p50 / p99 micro-batch latency) and a summary line per exec
mode (on/off ratio next to the spread between the off legs) to <out>/shadow_ab.jsonl.
Every engine toggles the shadow at runtime (set_shadow).  Launch mode is measured twice: with
coalesce 8, where the shadow-off legs put 8 micro-batches into a launch and the shadow-on legs
one (a shadow is not coalesced), and with coalesce 1, where both legs launch per micro-batch.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def leg(eng, seconds: float, batches_per_step: int):
    """One timed leg on a drained engine: pump without draining for ``seconds``, then drain."""
    from ccfd_demo_summit_amd.engine import FlaggedDrainer
    flagged = [0]

    def sink(recs):
        flagged[0] += len(recs)

    eng.reset_stats()
    rows = 0
    with FlaggedDrainer(eng, sink):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            rows += eng.pump(batches_per_step, drain=False, on_flagged=sink).rows
        st = eng.pump(0, drain=True, on_flagged=sink)
        wall = time.perf_counter() - t0
        rows += st.rows
    return {"rows": rows, "wall_s": round(wall, 4), "tx_per_s": rows / wall, "p50_us": st.p50_us,
            "p99_us": st.p99_us, "flagged": flagged[0]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/shadow")
    ap.add_argument("--seconds", type=float, default=4.0, help="length of one leg")
    ap.add_argument("--rounds", type=int, default=2, help="off/on pairs per exec mode")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--log-rows", type=int, default=1 << 21)
    ap.add_argument("--batches-per-step", type=int, default=256)
    ap.add_argument("--modes", default="persistent:8,launch:8,launch:1", help="exec_mode:coalesce, comma-separated")
    a = ap.parse_args(argv)

    import torch

    from ccfd_demo_summit_amd.data import FRAUD_RATE, generate
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    dev = torch.device("cuda", 0)
    Xr, _ = generate(100_000, seed=17)
    champion = DeviceModel(build_model("mlp", seed=0, X_ref=Xr, calibrate_rate=FRAUD_RATE), dev, wire=True)
    shadow = DeviceModel(build_model("mlp", seed=1, X_ref=Xr, calibrate_rate=FRAUD_RATE), dev, wire=True)
    parts = 2
    logs = []
    for p in range(parts):
        log = PartitionLog(a.log_rows // parts, wire=True)
        Xp, _ = generate(log.n, seed=7919 + p)
        log.write_rows(0, Xp)
        log.ids.array[:] = np.arange(log.n, dtype=np.uint64) + np.uint64(p) * np.uint64(1 << 40)
        log.customer.array[:] = 0
        logs.append(log)

    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "shadow_ab.jsonl")
    with open(path, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for spec in a.modes.split(","):
            mode, co = spec.split(":")
            eng = StreamEngine(champion, batch=a.batch, depth=a.depth, streams=a.streams, input_mode="zerocopy",
                               output_mode="zerocopy", device=dev.index, exec_mode=mode, coalesce=int(co),
                               flag_capacity=1 << 23)
            for p, log in enumerate(logs):
                eng.add_log(p, log)
            leg(eng, 1.0, a.batches_per_step)                     # warm-up, not reported
            res = {"off": [], "on": []}
            for r in range(a.rounds):
                for which in ("off", "on"):
                    eng.set_shadow(shadow if which == "on" else None)
                    out = leg(eng, a.seconds, a.batches_per_step)
                    res[which].append(out)
                    emit(dict(out, kind="leg", exec_mode=mode, shadow=which, round=r, batch=a.batch, depth=a.depth,
                              coalesce=0 if mode != "launch" else 1 if which == "on" else int(co)))
            c = (eng.counters[0] + eng.counters[1]).cpu().numpy()
            sc = StreamEngine.shadow_counters(c)
            sc.pop("disagree")           # slot 1 also counts the champion's fraud rows of the off legs
            eng.set_shadow(None)
            eng.close()
            off = [x["tx_per_s"] for x in res["off"]]
            on = [x["tx_per_s"] for x in res["on"]]
            emit({"kind": "summary", "exec_mode": mode, "coalesce": int(co) if mode == "launch" else 0,
                  "off_tx_per_s": off, "on_tx_per_s": on,
                  "on_off_ratio": float(np.mean(on) / np.mean(off)),
                  "off_spread": float((max(off) - min(off)) / np.mean(off)),
                  "off_p50_us": [x["p50_us"] for x in res["off"]], "on_p50_us": [x["p50_us"] for x in res["on"]],
                  "off_p99_us": [x["p99_us"] for x in res["off"]], "on_p99_us": [x["p99_us"] for x in res["on"]],
                  "shadow": sc})
    for log in logs:
        log.free()
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
