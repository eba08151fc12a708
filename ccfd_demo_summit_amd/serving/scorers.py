"""Scoring back-ends behind predict() and the compat (JSON-topic) router path.

* ``CpuScorer``  -- NumPy model on the host; config 1 (LR, batch=1) and the CPU oracle.
* ``GpuScorer``  -- the fused HIP kernels through a native StreamEngine slot set
                    (pageable host input is staged by DMA; results come back pinned).

Both return ``(proba_1 float32[n], route uint8[n])`` with route = proba >= threshold.
``explain(X)`` (an oblivious GBDT or a general tree ensemble, with cover, or an MLP / LR with a
baseline; anything else raises ``ValueError``) returns ``(phi float32/64 [n,30], base_value)``, the
Shapley attributions of docs/EXPLAIN.md: exact for the trees and LR, sampled for the MLP.
``set_drift(reference)`` makes every later ``score(X)`` batch also count its rows into a drift
window -- binned against the model's table for an oblivious GBDT with a binned reference, as W64
rows against the reference's own quantile table for an MLP / LR with a W64 reference; any other
pairing raises ``ValueError`` -- and ``drift()`` reports it (docs/DRIFT.md).
``set_outlier(model)`` sets a ``models.outlier.OutlierAE`` beside the fraud model: ``outlier(X)`` returns
``(scores float32 [n], is_outlier bool [n], sq_err float32 [n,30])`` of the rows as W64, every later
``score(X)`` batch is also counted into an outlier window, and ``outlier_report()`` reports it
(docs/OUTLIER.md).  The fraud scores do not change.
"""
from __future__ import annotations

import threading
from typing import Tuple

import numpy as np

from ..contracts.transaction import encode_wire


class CpuScorer:
    device = "cpu"

    def __init__(self, model, threshold: float = 0.5):
        self.model = model
        self.threshold = float(threshold)
        self._drift = None           # (reference, bins or None for W64, counts, tail) after set_drift
        self._drift_min_rows = 10_000
        self._drift_lock = threading.Lock()
        self._outlier = None         # (OutlierAE, counts uint64 [66]) after set_outlier

    def score(self, X: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        X = np.asarray(X, np.float32)
        p = self.model.predict_proba(X).astype(np.float32)
        if self._outlier is not None:
            self.outlier(X.reshape(-1, X.shape[-1]))
        if self._drift is not None:
            from ..models.drift import bin_counts, wire_bin_counts
            with self._drift_lock:
                ref, bins, counts, tail = self._drift
                rows = X.reshape(-1, X.shape[-1])
                c, t = wire_bin_counts(encode_wire(rows), ref.edges) if bins is None else \
                    bin_counts(bins.encode(rows), ref.stamp)
                counts += c
                tail += t
        return p, (p >= self.threshold).astype(np.uint8)

    def set_drift(self, reference, min_rows: int = 10_000) -> None:
        """Count every later ``score`` batch against ``reference`` (``None`` turns it off)."""
        with self._drift_lock:
            if reference is None:
                self._drift = None
                return
            bins = _drift_bins(self.model, reference)
            self._drift_min_rows = int(min_rows)
            self._drift = (reference, bins, np.zeros((31, 256), np.uint64), np.zeros(2, np.uint64))

    def drift(self, reset: bool = False):
        """``models.drift.DriftReport`` of the rows scored since ``set_drift`` / the last reset."""
        from ..models.drift import DriftReport
        with self._drift_lock:
            if self._drift is None:
                raise ValueError("no drift reference set (set_drift)")
            ref, _, counts, tail = self._drift
            rep = DriftReport.compare(ref, counts.copy(), tail.copy(), min_rows=self._drift_min_rows)
            if reset:
                counts[:] = 0
                tail[:] = 0
        return rep

    def set_outlier(self, model) -> None:
        """Score every later batch with the numpy wire oracle of ``model`` too (``None`` turns it off)."""
        with self._drift_lock:
            self._outlier = None if model is None else (_outlier_model(model), np.zeros(_OUT_SLOTS, np.uint64))

    def outlier(self, X: np.ndarray, count: bool = True):
        """``(scores [n], is_outlier [n], sq_err [n,30] canonical)`` of ``OutlierAE.wire_sq_err``."""
        from ..models.outlier import recount
        with self._drift_lock:
            if self._outlier is None:
                raise ValueError("no outlier model set (set_outlier)")
            model, counts = self._outlier
            rows = encode_wire(np.asarray(X, np.float32).reshape(-1, 30))
            res = model.wire_residuals(rows)
            score, sq = model.wire_sq_err(rows)
            if count:
                counts += recount(score, res, model.threshold)
            with np.errstate(invalid="ignore"):
                return score, score > np.float32(model.threshold), sq

    def outlier_report(self, reset: bool = False):
        """``models.outlier.OutlierReport`` of the rows seen since ``set_outlier`` / the last reset."""
        from ..models.outlier import OutlierReport
        with self._drift_lock:
            if self._outlier is None:
                raise ValueError("no outlier model set (set_outlier)")
            model, counts = self._outlier
            rep = OutlierReport.from_counts(counts.copy(), model.threshold)
            if reset:
                counts[:] = 0
        return rep

    def explain(self, X: np.ndarray) -> Tuple[np.ndarray, float]:
        _explainable(self.model)
        if self.model.kind == "mlp":
            from ..models.explain_mlp import shapley_mlp_sampled
            return shapley_mlp_sampled(self.model, np.asarray(X, np.float32), EXPLAIN_PERMS, EXPLAIN_SEED)
        if self.model.kind == "lr":
            from ..models.explain_mlp import shapley_lr
            return shapley_lr(self.model, np.asarray(X, np.float32))
        if self.model.kind == "forest":
            from ..models.explain_forest import shapley_forest
            return shapley_forest(self.model, np.asarray(X, np.float32))
        from ..models.explain import shapley_oblivious
        return shapley_oblivious(self.model, np.asarray(X, np.float32))


EXPLAIN_PERMS, EXPLAIN_SEED = 64, 0      # the MLP's sampled permutations (docs/EXPLAIN.md)
_OUT_SLOTS = 66                          # models.outlier.OUTLIER_SLOTS


def _outlier_model(model):
    if getattr(model, "kind", None) != "ae":
        raise ValueError(f"the outlier detector is an OutlierAE (kind 'ae'), not kind {getattr(model, 'kind', None)!r}")
    return model


def _explainable(model) -> None:
    kind = getattr(model, "kind", None)
    if kind in ("mlp", "lr"):
        if getattr(model, "baseline", None) is None:
            raise ValueError(f"model kind {kind!r} has no explanation without a baseline row "
                             "(call fit_baseline(X) first, or train with --explain-baseline)")
        return
    if kind not in ("gbdt", "forest"):
        raise ValueError(f"model kind {kind!r} has no explanation "
                         "(Shapley values exist for the tree models, and for MLP / LR with a baseline)")
    if kind == "forest" and getattr(model, "cover", None) is None:
        raise ValueError("the ensemble has no cover (background weight of every node): call fit_cover(X) first, "
                         "or import a model that carries one")


def _drift_bins(model, reference):
    """The model's own bin table at a binned reference's width, refused unless the reference was
    counted against it; ``None`` for a W64 reference on an MLP / LR, whose rows are counted as
    W64 against the reference's own table."""
    kind = getattr(model, "kind", None)
    if getattr(reference, "is_wire", False):
        if kind not in ("mlp", "lr"):
            raise ValueError(f"drift reference is for W64 rows (quantile bins of the raw values), which model kind "
                             f"{kind!r} does not score; fit a binned reference against its table (DriftReference.fit)")
        return None
    if kind != "gbdt":
        raise ValueError(f"model kind {kind!r} has no drift detector for a binned reference "
                         "(bin counts exist for the oblivious GBDT's split table only; an MLP / LR takes a "
                         "W64 reference, DriftReference.fit_wire)")
    bins = model.bin_spec(bits=reference.bits)
    if not reference.compatible(bins):
        raise ValueError(f"drift reference (stamp {reference.stamp}, {reference.bits}-bit) was not counted against "
                         f"this model's bin table (stamp {bins.stamp})")
    return bins


class GpuScorer:
    device = "gpu"

    def __init__(self, model, threshold: float = 0.5, max_batch: int = 4096, depth: int = 2,
                 device_index: int = 0):
        import torch
        from ..engine import StreamEngine
        from ..ops.kernels import DeviceModel
        self.threshold = float(threshold)
        self.model = model
        self._device_index = device_index
        self._explainer = None
        self._drift = None           # (DriftMonitor, bins or None for W64) after set_drift
        self._outlier = None         # (OutlierAE, OutlierMonitor) after set_outlier
        self.dm = DeviceModel(model, torch.device("cuda", device_index))
        self.engine = StreamEngine(self.dm, batch=max_batch, depth=depth, streams=1,
                                   input_mode="dma", output_mode="zerocopy", threshold=threshold,
                                   device=device_index)
        self._lock = threading.Lock()

    def score(self, X: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        with self._lock:
            if self._drift is not None:
                import torch
                mon, bins = self._drift
                X = np.asarray(X, np.float32)
                rows = X.reshape(-1, X.shape[-1])
                rows = np.ascontiguousarray(encode_wire(rows) if bins is None else bins.encode(rows))
                mon.observe(torch.from_numpy(rows).to(mon.device))
            if self._outlier is not None:
                import torch
                mon = self._outlier[1]
                rows = np.asarray(X, np.float32)
                mon.observe(torch.from_numpy(encode_wire(rows.reshape(-1, rows.shape[-1]))).to(mon.device))
            return self.engine.score(X)

    def set_outlier(self, model) -> None:
        """Score every later ``score`` batch with csrc/kernels/outlier_ae.hip too, into an outlier
        window, and serve ``outlier(X)`` (``None`` turns it off).  The fraud scores do not change."""
        with self._lock:
            if self._outlier is not None:
                self._outlier[1].close()
                self._outlier = None
            if model is None:
                return
            import torch
            from ..ops.kernels import OutlierMonitor
            self._outlier = (_outlier_model(model), OutlierMonitor(model, torch.device("cuda", self._device_index)))

    def outlier(self, X: np.ndarray, count: bool = True):
        """``(scores float32 [n], is_outlier bool [n], sq_err float32 [n,30] canonical)`` of the rows
        as W64, from ``ops.kernels.outlier_scores``; ``count`` adds them to the window."""
        import torch
        from ..contracts.transaction import WIRE_PERM
        from ..ops.kernels import outlier_scores
        with self._lock:
            if self._outlier is None:
                raise ValueError("no outlier model set (set_outlier)")
            model, mon = self._outlier
            rows = torch.from_numpy(encode_wire(np.asarray(X, np.float32).reshape(-1, 30))).to(mon.device)
            resid = torch.empty((rows.shape[0], 32), dtype=torch.float32, device=mon.device)
            score = outlier_scores(mon.dev_model, rows, None, resid, mon.counts if count else None)
            score, resid = score.cpu().numpy(), resid.cpu().numpy()
        sq = np.empty((score.shape[0], 30), np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            sq[:, WIRE_PERM] = resid[:, :30] * resid[:, :30]
            return score, score > np.float32(model.threshold), sq

    def outlier_report(self, reset: bool = False):
        with self._lock:
            if self._outlier is None:
                raise ValueError("no outlier model set (set_outlier)")
            return self._outlier[1].report(reset=reset)

    def set_drift(self, reference, min_rows: int = 10_000) -> None:
        """Count every later ``score`` batch against ``reference`` with
        csrc/kernels/drift_hist.hip, or drift_wire.hip for a W64 reference (``None`` turns it off)."""
        with self._lock:
            if self._drift is not None:
                self._drift[0].close()
                self._drift = None
            if reference is None:
                return
            import torch
            from ..ops.kernels import DriftMonitor
            bins = _drift_bins(self.model, reference)
            self._drift = (DriftMonitor(reference, torch.device("cuda", self._device_index), min_rows=min_rows), bins)

    def drift(self, reset: bool = False):
        with self._lock:
            if self._drift is None:
                raise ValueError("no drift reference set (set_drift)")
            return self._drift[0].report(reset=reset)

    def explain(self, X: np.ndarray) -> Tuple[np.ndarray, float]:
        """csrc/kernels/explain_gbdt.hip (oblivious GBDT) or explain_forest.hip (general trees) on
        the rows binned against the model's own table; csrc/kernels/explain_mlp.hip (MLP with a
        baseline) on the rows as W64; the closed form on the host for LR."""
        _explainable(self.model)
        if self.model.kind == "lr":
            from ..models.explain_mlp import shapley_lr
            return shapley_lr(self.model, np.asarray(X, np.float32))
        with self._lock:
            if self._explainer is None:
                import torch
                from ..ops.kernels import DeviceExplainer, DeviceMlpExplainer
                dev = torch.device("cuda", self._device_index)
                self._explainer = (DeviceMlpExplainer(self.model, EXPLAIN_PERMS, EXPLAIN_SEED, device=dev)
                                   if self.model.kind == "mlp" else DeviceExplainer(self.model, device=dev))
            return self._explainer.explain(X)

    def close(self):
        self.set_drift(None)
        self.set_outlier(None)
        self.engine.close()


def make_scorer(model, threshold: float = 0.5, device: str = "auto", **kw):
    if getattr(model, "kind", None) == "ae":
        raise ValueError("an outlier autoencoder (kind 'ae') is no fraud scorer: set it beside one with set_outlier")
    if device in ("auto", "gpu"):
        try:
            import torch
            if torch.cuda.is_available() and getattr(model, "kind", None) in ("lr", "mlp", "gbdt", "forest"):
                return GpuScorer(model, threshold, **kw)
        except Exception:
            if device == "gpu":
                raise
        if device == "gpu":
            raise RuntimeError("GPU scorer requested but no GPU is available")
    return CpuScorer(model, threshold)
