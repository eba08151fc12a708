"""Fraud-model workbench: the interactive model-development loop of the reference's
JupyterHub + Spark workbench (deploy/frauddetection_cr.yaml:7-53),
as a script to run, or to paste into a notebook cell by cell (the ``# %%`` markers).

1. load ``creditcard.csv`` (Time, V1..V28, Amount, Class), or synthetic rows of its shape;
2. train the three model families the engine serves (LR, MLP, oblivious GBDT);
3. compare them on a held-out split (ROC-AUC, PR-AUC);
4. check that the GBDT's exact 32-byte G32 wire picks the f32 model's leaves;
5. save versioned safetensors files a running engine hot-swaps (``launch engine --watch-model``);
6. print the top reasons (exact per-feature Shapley values) of the highest-scoring rows, for the
   trained GBDT and for a scikit-learn forest imported with its cover;
7. with an MI355X visible, score through the HIP kernels and compare with the CPU models.

    python examples/model_workbench.py [--csv creditcard.csv] [--rows 200000] [--out models_out]

Multi-GPU training is the batch job: ``torchrun --nproc-per-node N -m ccfd_demo_summit_amd.train``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csv", default="")
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--hist", default="torch", choices=["torch", "hip", "auto"],
                    help="GBDT histogram backend (train_oblivious_gbdt hist=)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--device", default="auto", help="auto | cpu | cuda:N")
    ap.add_argument("--out", default="models_out")
    a = ap.parse_args(argv)

    # %% data
    import numpy as np
    import torch

    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models import load_model, save_model
    from ccfd_demo_summit_amd.train.trainer import (TrainConfig, evaluate, train_logistic, train_mlp,
                                                    train_oblivious_gbdt)
    if a.csv:
        from ccfd_demo_summit_amd.data.csv_source import read_creditcard_csv
        X, y = read_creditcard_csv(a.csv)
        if y is None:
            raise SystemExit(f"{a.csv}: no Class column")
    else:
        X, y = generate(a.rows, seed=0, fraud_rate=0.0017)
    idx = np.random.default_rng(0).permutation(len(X))
    n_test = len(X) // 5
    Xte, yte, Xtr, ytr = X[idx[:n_test]], y[idx[:n_test]], X[idx[n_test:]], y[idx[n_test:]]
    device = a.device if a.device != "auto" else ("cuda:0" if torch.cuda.is_available() else "cpu")
    print(f"{len(X)} rows, {int(y.sum())} fraud ({y.mean():.4%}), training on {device}")

    # %% train the three model families
    cfg = TrainConfig(epochs=a.epochs, batch=a.batch, device=device)
    models = {"lr": train_logistic(Xtr, ytr, cfg)[0], "mlp": train_mlp(Xtr, ytr, cfg)[0],
              "gbdt": train_oblivious_gbdt(Xtr, ytr, n_trees=a.trees, depth=6, device=device,
                                           hist=a.hist)[0]}
    report = {"rows": int(len(X)), "device": device, "models": {}}
    for name, m in models.items():
        r = evaluate(m, Xte, yte)
        report["models"][name] = r
        print(f"{name:5s} ROC-AUC {r['roc_auc']:.4f}  PR-AUC {r['pr_auc']:.4f}")

    # %% G32: one u8 bin per feature against the ensemble's own split thresholds
    gb = models["gbdt"]
    spec = gb.bin_spec()
    rows = spec.encode(Xte)
    same = bool(np.array_equal(gb.leaf_index(Xte), gb.leaf_index_g32(rows, spec)))
    report["g32"] = {"rows": int(len(rows)), "leaves_equal": same, "stamp": int(spec.stamp),
                     "edges": int(spec.offsets[-1])}
    print(f"G32: {len(rows)} rows, leaves identical to f32: {same}, {int(spec.offsets[-1])} edges, stamp {spec.stamp}")
    if not same:
        raise SystemExit("G32 leaves differ from the f32 model's")

    # %% save versioned models for the engine's hot swap
    os.makedirs(a.out, exist_ok=True)
    for name, m in models.items():
        path = os.path.join(a.out, f"{name}.safetensors")
        save_model(m, path, version="1")
        back = load_model(path)
        assert np.allclose(back.predict_proba(Xte[:1000]), m.predict_proba(Xte[:1000]), atol=1e-6)
        print("saved", path)

    # %% why were the highest-scoring rows flagged?  (exact Shapley values, docs/EXPLAIN.md)
    from ccfd_demo_summit_amd.contracts.transaction import FEATURE_NAMES
    from ccfd_demo_summit_amd.models.explain import shapley_oblivious, top_reasons
    top = np.argsort(-gb.predict_proba(Xte))[:3]
    on_gpu = torch.cuda.is_available() and device.startswith("cuda")
    if on_gpu:
        from ccfd_demo_summit_amd.ops.kernels import DeviceExplainer
        phi, base_value = DeviceExplainer(gb, bins=spec, device=torch.device(device)).explain(Xte[top])
    else:
        phi, base_value = shapley_oblivious(gb, Xte[top])
    report["reasons"] = {"base_value": float(base_value), "backend": "hip" if on_gpu else "cpu", "rows": []}
    for i, row in zip(top, phi):
        why = top_reasons(row, FEATURE_NAMES, 3)
        report["reasons"]["rows"].append({"row": int(i), "raw_score": float(base_value + row.sum()), "reasons": why})
        print(f"row {int(i)}: log-odds {base_value + row.sum():+.3f} = base {base_value:+.3f} "
              + " ".join(f"{w['feature']} {w['phi']:+.3f}" for w in why) + " ...")

    # %% the same question to a model brought from elsewhere: a scikit-learn forest, imported with its cover
    try:
        from sklearn.ensemble import RandomForestClassifier
    except ImportError:
        RandomForestClassifier = None
    if RandomForestClassifier is not None:
        from ccfd_demo_summit_amd.models.explain_forest import shapley_forest
        from ccfd_demo_summit_amd.models.sklearn_import import from_sklearn
        k = min(len(Xtr), 20_000)
        forest = from_sklearn(RandomForestClassifier(n_estimators=8, max_depth=6, random_state=0).fit(Xtr[:k], ytr[:k]))
        ftop = np.argsort(-forest.predict_proba(Xte))[:3]
        if on_gpu:
            fphi, fbase = DeviceExplainer(forest, device=torch.device(device)).explain(Xte[ftop])
        else:
            fphi, fbase = shapley_forest(forest, Xte[ftop])
        report["forest_reasons"] = {"base_value": float(fbase), "backend": "hip" if on_gpu else "cpu", "rows": []}
        for i, row in zip(ftop, fphi):
            why = top_reasons(row, FEATURE_NAMES, 3)
            report["forest_reasons"]["rows"].append({"row": int(i), "raw_score": float(fbase + row.sum()), "reasons": why})
            print(f"forest row {int(i)}: class fraction {fbase + row.sum():.3f} = base {fbase:.3f} "
                  + " ".join(f"{w['feature']} {w['phi']:+.3f}" for w in why) + " ...")

    # %% does the holdout still look like the training rows?  (PSI per feature, docs/DRIFT.md)
    from ccfd_demo_summit_amd.models.drift import DriftReference, DriftReport, bin_counts
    ref = DriftReference.fit(Xtr, spec)
    drift = DriftReport.compare(ref, *bin_counts(rows, spec.stamp))
    report["drift"] = {"rows": drift.rows, "worst": [{"feature": n, "psi": v, "status": s} for n, v, s in drift.worst(3)]}
    print("drift train -> holdout, worst PSI: " + ", ".join(f"{n} {v:.4f} ({s})" for n, v, s in drift.worst(3)))
    # the MLP / LR see W64 rows and have no table: the reference brings 32 quantile cells a feature
    from ccfd_demo_summit_amd.contracts.transaction import encode_wire
    from ccfd_demo_summit_amd.models.drift import wire_bin_counts
    wref = DriftReference.fit_wire(Xtr)
    wdrift = DriftReport.compare(wref, *wire_bin_counts(encode_wire(Xte), wref.edges))
    report["drift_w64"] = {"rows": wdrift.rows,
                           "worst": [{"feature": n, "psi": v, "status": s} for n, v, s in wdrift.worst(3)]}
    print("drift train -> holdout on W64 rows (MLP / LR), worst PSI: "
          + ", ".join(f"{n} {v:.4f} ({s})" for n, v, s in wdrift.worst(3)))

    # %% score through the MI355X kernels
    if torch.cuda.is_available() and device.startswith("cuda"):
        from ccfd_demo_summit_amd.engine import StreamEngine
        from ccfd_demo_summit_amd.ops.kernels import DeviceModel
        report["gpu"] = {}
        n = min(len(Xte), 100_000)
        for name, m in models.items():
            eng = StreamEngine(DeviceModel(m, torch.device(device), bins=(name == "gbdt")), batch=4096, depth=4)
            try:
                p, route = eng.score(Xte[:n])
            finally:
                eng.close()
            err = float(np.abs(p - m.predict_proba(Xte[:n])).max())
            report["gpu"][name] = {"max_abs_dp": err, "fraud_routed": int(route.sum())}
            print(f"{name:5s} GPU max |dp| {err:.2e}, {int(route.sum())} rows routed to the fraud process")
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
