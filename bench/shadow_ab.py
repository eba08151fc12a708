"""What a shadow (challenger) model costs the streaming engine: shadow off / on legs, alternated
in one process on one engine per exec mode, with bench.py config 2's engine settings (MLP on W64
rows, micro-batch 4096, depth 12, zero-copy in both directions, flagged ring drained by a
collector thread) -- or, with ``--model gbdt``, config 4's (oblivious GBDT 100 x 6 on G20 / G32
rows, micro-batch 65536, depth 4 on G20 / 3 on G32).

    python bench/shadow_ab.py --out profiles/shadow [--seconds 4] [--rounds 2]
    python bench/shadow_ab.py --model gbdt [--wire g20|g32] --out profiles/shadow_gbdt

The GBDT challenger is "a retrained ensemble inside the live bin table": the champion's splits
with leaves of its own, packed against the champion's table -- what a hot swap without
re-encoding the logs allows, and on the GPU the same work as any ensemble of that shape.

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
    ap.add_argument("--model", default="mlp", choices=["mlp", "gbdt"])
    ap.add_argument("--wire", default="g20", choices=["g20", "g32"], help="--model gbdt: binned row format")
    ap.add_argument("--trees", type=int, default=100, help="--model gbdt: trees of both ensembles")
    ap.add_argument("--tree-depth", type=int, default=6, help="--model gbdt: depth of both ensembles")
    ap.add_argument("--out", default=None, help="default: profiles/shadow (mlp), profiles/shadow_gbdt (gbdt)")
    ap.add_argument("--seconds", type=float, default=4.0, help="length of one leg")
    ap.add_argument("--rounds", type=int, default=2, help="off/on pairs per exec mode")
    ap.add_argument("--batch", type=int, default=None, help="default: 4096 (mlp), 65536 (gbdt)")
    ap.add_argument("--depth", type=int, default=None, help="default: 12 (mlp), 4 (gbdt on G20), 3 (gbdt on G32)")
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--log-rows", type=int, default=1 << 21)
    ap.add_argument("--batches-per-step", type=int, default=256)
    ap.add_argument("--modes", default=None, help="exec_mode:coalesce, comma-separated (default: "
                    "persistent:8,launch:8,launch:1 for mlp; persistent:1,launch:1 for gbdt, which is never coalesced)")
    a = ap.parse_args(argv)
    gbdt = a.model == "gbdt"
    a.out = a.out or ("profiles/shadow_gbdt" if gbdt else "profiles/shadow")
    a.batch = a.batch or (65536 if gbdt else 4096)
    a.depth = a.depth or ((4 if a.wire == "g20" else 3) if gbdt else 12)
    a.modes = a.modes or ("persistent:1,launch:1" if gbdt else "persistent:8,launch:8,launch:1")

    import torch

    from ccfd_demo_summit_amd.data import FRAUD_RATE, generate
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    dev = torch.device("cuda", 0)
    Xr, _ = generate(100_000, seed=17)
    bins = None
    if gbdt:
        from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
        mA = build_model("gbdt", seed=0, X_ref=Xr, calibrate_rate=FRAUD_RATE, gbdt_trees=a.trees,
                         gbdt_depth=a.tree_depth)
        bins = mA.bin_spec(bits=5 if a.wire == "g20" else 8)
        mB = ObliviousGBDT(mA.feat, mA.thr, build_model("gbdt", seed=1, gbdt_trees=a.trees, gbdt_depth=a.tree_depth).leaves, 0.0)
        mB.calibrate_bias(Xr, FRAUD_RATE)
        champion, shadow = DeviceModel(mA, dev, bins=bins), DeviceModel(mB, dev, bins=bins)
    else:
        champion = DeviceModel(build_model("mlp", seed=0, X_ref=Xr, calibrate_rate=FRAUD_RATE), dev, wire=True)
        shadow = DeviceModel(build_model("mlp", seed=1, X_ref=Xr, calibrate_rate=FRAUD_RATE), dev, wire=True)
    parts = 2
    logs = []
    for p in range(parts):
        log = PartitionLog(max(a.log_rows // parts, 4 * a.batch), wire=not gbdt, bins=bins)
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
                    emit(dict(out, kind="leg", model=a.model, rows_format=champion.row_format, exec_mode=mode,
                              shadow=which, round=r, batch=a.batch, depth=a.depth,
                              **({"trees": a.trees, "tree_depth": a.tree_depth} if gbdt else {}),
                              coalesce=0 if mode != "launch" else 1 if which == "on" else int(co)))
            c = (eng.counters[0] + eng.counters[1]).cpu().numpy()
            sc = StreamEngine.shadow_counters(c)
            sc.pop("disagree")           # slot 1 also counts the champion's fraud rows of the off legs
            eng.set_shadow(None)
            eng.close()
            off = [x["tx_per_s"] for x in res["off"]]
            on = [x["tx_per_s"] for x in res["on"]]
            emit({"kind": "summary", "model": a.model, "rows_format": champion.row_format, "exec_mode": mode, "coalesce": int(co) if mode == "launch" else 0,
                  **({"trees": a.trees, "tree_depth": a.tree_depth} if gbdt else {}),
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
