"""Training job -- the batch analogue of the reference's JupyterHub + Spark workbench
(deploy/frauddetection_cr.yaml:7-53): train a fraud model on
``creditcard.csv`` (or synthetic rows of that shape), evaluate it on a held-out split and
save it as a versioned safetensors file that a running engine hot-swaps (``launch engine
--watch-model``).  Data-parallel under torchrun: DDP for LR/MLP, all-reduced histograms for
the GBDT (train/trainer.py); rank 0 evaluates and writes.

    python -m ccfd_demo_summit_amd.train --model mlp --out model.safetensors
    torchrun --nproc-per-node 2 -m ccfd_demo_summit_amd.train --model gbdt --csv creditcard.csv --out m.st
    python -m ccfd_demo_summit_amd.train --from-catboost model.json --out m.st   # import, no training
    python -m ccfd_demo_summit_amd.train --from-xgboost model.json --out m.st    # general trees, no training
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np


def _serve_metrics(port: int):
    """TrainMetrics on :port/metrics in a daemon thread (stdlib HTTP server)."""
    import threading
    from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

    from ..metrics.exporter import CONTENT_TYPE, TrainMetrics
    tm = TrainMetrics()

    class H(BaseHTTPRequestHandler):
        def do_GET(self):
            body = tm.expose()
            self.send_response(200)
            self.send_header("Content-Type", CONTENT_TYPE)
            self.send_header("Content-Length", str(len(body)))
            self.end_headers()
            self.wfile.write(body)

        def log_message(self, *a):
            pass
    srv = ThreadingHTTPServer(("0.0.0.0", port), H)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    return tm


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="mlp", choices=["lr", "mlp", "gbdt"])
    ap.add_argument("--csv", default=None, help="creditcard.csv (Time, V1..V28, Amount, Class)")
    ap.add_argument("--rows", type=int, default=400_000, help="synthetic rows when no --csv")
    ap.add_argument("--fraud-rate", type=float, default=0.0017)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--device", default="auto")
    ap.add_argument("--holdout", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--version", default="1")
    ap.add_argument("--out", required=True)
    ap.add_argument("--max-borders", type=int, default=31,
                    help="GBDT: split candidates per feature (<= 31 keeps every trained ensemble on the "
                         "20-byte G20 row format; <= 255 for G32)")
    ap.add_argument("--hist", default="torch", choices=["torch", "hip", "auto"],
                    help="GBDT: histogram backend -- torch scatter_add (default), the HIP histogram kernel over "
                         "G32 rows (CUDA device, <= 64 bins), or auto (hip when it can)")
    ap.add_argument("--bin-spec-from", default=None, metavar="MODEL.safetensors",
                    help="GBDT: take the split candidates from this GBDT's bin table (its bin_spec()), so the "
                         "trained ensemble packs against the table the live G32 / G20 logs were encoded with "
                         "(a challenger for `launch engine --shadow-model`); replaces --max-borders")
    ap.add_argument("--drift-reference-out", default=None, metavar="REF.safetensors",
                    help="also write the drift reference of the training rows (models/drift.py; `launch "
                         "seldon|engine --drift-reference`): against the trained model's bin table for a GBDT, "
                         "as W64 rows against their own quantile table (--drift-cells) for an MLP / LR")
    ap.add_argument("--bits", type=int, default=None, choices=[5, 8],
                    help="GBDT --drift-reference-out: bin width of the rows the reference is for (5 = G20, "
                         "8 = G32); default 5 when the table fits G20 rows, else 8")
    ap.add_argument("--drift-cells", type=int, default=32, metavar="N",
                    help="MLP / LR --drift-reference-out: quantile cells per feature of the W64 reference, 2..32")
    ap.add_argument("--explain-baseline", default=None, choices=["median", "mean"],
                    help="MLP / LR: store the per-feature median or mean of the training rows as the model's "
                         "baseline (fit_baseline), the row its Shapley explanations start from (docs/EXPLAIN.md); "
                         "off by default")
    ap.add_argument("--outlier-out", default=None, metavar="AE.safetensors",
                    help="also train the outlier autoencoder (models/outlier.py; `launch seldon|engine|demo "
                         "--outlier-model`) on the legitimate rows of the same training split, beside any --model, "
                         "and fit its threshold on the training rows")
    ap.add_argument("--outlier-latent", type=int, default=8, help="--outlier-out: latent width, 1..32")
    ap.add_argument("--outlier-quantile", type=float, default=0.999,
                    help="--outlier-out: the threshold is this quantile of the training rows' scores")
    ap.add_argument("--metrics-port", type=int, default=0,
                    help="serve the trainer's /metrics (the SparkMetrics dashboard series) on this port "
                         "(+ rank) while training; 0 = off")
    ap.add_argument("--from-catboost", default=None,
                    help="import an oblivious CatBoost JSON model (models/gbdt_import.py) instead of training")
    ap.add_argument("--from-xgboost", default=None,
                    help="import an XGBoost JSON model (binary:logistic gbtree, models/xgboost_import.py) as a "
                         "general tree ensemble instead of training")
    a = ap.parse_args(argv)
    if a.from_xgboost:
        from ..models import save_model
        from ..models.xgboost_import import from_xgboost_json
        m = from_xgboost_json(a.from_xgboost)
        save_model(m, a.out, version=a.version)
        print(json.dumps({"model": "forest", "imported": a.from_xgboost, "out": a.out, "trees": m.n_trees,
                          "depth": m.depth, "nodes": m.n_nodes}), flush=True)
        return 0
    if a.from_catboost:
        from ..models import save_model
        from ..models.gbdt_import import from_catboost_json
        m = from_catboost_json(a.from_catboost)
        save_model(m, a.out, version=a.version)
        print(json.dumps({"model": "gbdt", "imported": a.from_catboost, "out": a.out, "trees": m.n_trees,
                          "depth": m.depth}), flush=True)
        return 0

    import torch
    import torch.distributed as dist
    from ..data import generate
    from ..models import save_model
    from .trainer import TrainConfig, evaluate, train_logistic, train_mlp, train_oblivious_gbdt

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    tm = None
    if a.metrics_port:
        tm = _serve_metrics(a.metrics_port + int(os.environ.get("LOCAL_RANK", "0")))
        tm.workers.set(world)
    if world > 1 and not dist.is_initialized():
        use_gpu = a.device != "cpu" and torch.cuda.is_available()
        if use_gpu:
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl" if use_gpu else "gloo")
    if a.csv:
        from ..data.csv_source import read_creditcard_csv
        X, y = read_creditcard_csv(a.csv)
        if y is None:
            raise SystemExit(f"{a.csv}: no Class column to train on")
    else:
        X, y = generate(a.rows, seed=a.seed, fraud_rate=a.fraud_rate)
    rng = np.random.default_rng(a.seed)
    idx = rng.permutation(len(X))
    n_test = int(len(X) * a.holdout)
    te, tr = idx[:n_test], idx[n_test:]
    dev = a.device
    if world > 1 and dev == "auto" and torch.cuda.is_available():
        dev = f"cuda:{torch.cuda.current_device()}"
    if a.bin_spec_from and a.model != "gbdt":
        raise SystemExit("--bin-spec-from is for --model gbdt")
    if a.drift_reference_out and a.model not in ("gbdt", "mlp", "lr"):
        raise SystemExit("--drift-reference-out is for --model gbdt|mlp|lr")
    if a.bits is not None and a.model != "gbdt":
        raise SystemExit("--bits is for --model gbdt (an MLP / LR reference is for W64 rows: --drift-cells)")
    if not 2 <= a.drift_cells <= 32:
        raise SystemExit("--drift-cells is 2..32")
    if not 1 <= a.outlier_latent <= 32:
        raise SystemExit("--outlier-latent is 1..32")
    if not 0.0 < a.outlier_quantile <= 1.0:
        raise SystemExit("--outlier-quantile is in (0, 1]")
    if a.explain_baseline and a.model == "gbdt":
        raise SystemExit("--explain-baseline is for --model mlp|lr (a GBDT is explained through its cover)")
    if a.model == "gbdt":
        spec = None
        if a.bin_spec_from:
            from ..models import load_model
            live = load_model(a.bin_spec_from)
            if live.kind != "gbdt":
                raise SystemExit(f"--bin-spec-from {a.bin_spec_from}: a {live.kind!r} model has no bin table")
            spec = live.bin_spec()
        model, info = train_oblivious_gbdt(X[tr], y[tr], n_trees=a.trees, depth=a.depth, device=dev,
                                           n_bins=a.max_borders + 1, hist=a.hist, bin_spec=spec)
    else:
        cfg = TrainConfig(epochs=a.epochs, batch=a.batch, device=dev, seed=a.seed, metrics=tm)
        model, info = (train_mlp if a.model == "mlp" else train_logistic)(X[tr], y[tr], cfg)
        if a.explain_baseline:
            model = model.fit_baseline(X[tr], a.explain_baseline)
    ae = ae_info = None
    if a.outlier_out:
        from .trainer import train_autoencoder
        ae, ae_info = train_autoencoder(X[tr], y[tr], TrainConfig(epochs=a.epochs, batch=a.batch, device=dev,
                                                                  seed=a.seed), latent=a.outlier_latent)
    if rank == 0:
        metrics = evaluate(model, X[te], y[te]) if n_test and 0 < y[te].sum() < n_test else {}
        save_model(model, a.out, version=a.version)
        out = {"model": a.model, "out": a.out, "world": world, "train": info, "holdout": metrics}
        if a.drift_reference_out:
            from ..models.drift import DriftReference
            if a.model == "gbdt":
                bits = a.bits or (5 if model.bin_spec().fits_g20 else 8)
                ref = DriftReference.fit(X[tr], model.bin_spec(bits=bits))
            else:
                ref = DriftReference.fit_wire(X[tr], cells=a.drift_cells)
            ref.save(a.drift_reference_out)
            out["drift_reference"] = {"out": a.drift_reference_out, "bits": ref.bits, "stamp": ref.stamp,
                                      "rows": ref.rows}
        if ae is not None:
            ae.fit_threshold(X[tr], a.outlier_quantile)
            save_model(ae, a.outlier_out, version=a.version)
            if n_test and 0 < y[te].sum() < n_test:
                from sklearn.metrics import roc_auc_score
                ae_info["test_roc_auc"] = float(roc_auc_score(y[te], ae.scores(X[te])))
            out["outlier"] = {"out": a.outlier_out, "latent": ae.latent, "threshold": ae.threshold,
                              "quantile": a.outlier_quantile, "train": ae_info}
        print(json.dumps(out, default=float), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
