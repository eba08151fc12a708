"""Feature-drift detection on binned rows (CPU side: definition, numpy oracle, PSI, report).

A G32 / G20 row is the transaction binned against the model's own split table
(``models.gbdt.BinSpec``, ``bin = #edges < x``), so a per-feature histogram of its bytes is
the feature distribution at exactly the resolution the model can see: a shift inside one bin
cannot change any score.  ``csrc/kernels/drift_hist.hip`` counts those histograms on the GPU
(``ops.kernels.drift_histogram`` / ``DriftMonitor``); ``bin_counts`` here is its oracle.

The statistic is the Population Stability Index per column with additive smoothing
(docs/DRIFT.md).  Column 30 is the amount bucket, which every table has.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

from ..contracts.metric_names import AMOUNT_BUCKETS
from ..contracts.transaction import FEATURE_NAMES, G20_ROW_BYTES, G32_ROW_BYTES, N_FEATURES, decode_g20_bins

N_COLS = N_FEATURES + 1                  # 30 features + the amount bucket (ccfd_abi.h CCFD_DRIFT_COLS)
N_CELLS = 256                            # ccfd_abi.h CCFD_DRIFT_CELLS
N_BUCKETS = len(AMOUNT_BUCKETS) + 1      # 14
COLUMN_NAMES: Tuple[str, ...] = tuple(FEATURE_NAMES) + ("AmountBucket",)
PSI_BANDS = (0.1, 0.25)                  # the conventional bands: < 0.1 stable, < 0.25 moderate, else drift
MIN_ROWS = 10_000


def bin_counts(rows: np.ndarray, stamp: int) -> Tuple[np.ndarray, np.ndarray]:
    """numpy oracle of the drift kernel: uint8 ``[n,32]`` G32 or ``[n,20]`` G20 rows ->
    ``(counts uint64 [31,256], tail uint64 [2])``.  Rows whose stamp equals ``stamp`` add one to
    ``counts[j, bin_j]`` (j < 30), to ``counts[30, amount bucket]`` and to ``tail[0]``; every
    other row adds one to ``tail[1]`` only."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] not in (G32_ROW_BYTES, G20_ROW_BYTES):
        raise ValueError("rows must be uint8 [n,32] (G32) or [n,20] (G20)")
    g = decode_g20_bins(rows) if rows.shape[1] == G20_ROW_BYTES else rows
    ok = g[:, 31] == int(stamp)
    live = g[ok]
    counts = np.zeros((N_COLS, N_CELLS), np.uint64)
    for j in range(N_COLS):
        counts[j] = np.bincount(live[:, j], minlength=N_CELLS).astype(np.uint64)
    tail = np.array([int(ok.sum()), int((~ok).sum())], np.uint64)
    return counts, tail


def n_bins_of(bins) -> np.ndarray:
    """int32 [31]: cells a column of ``bins`` can reach (edges + 1; 14 amount buckets)."""
    return np.array([e.size + 1 for e in bins.edges] + [N_BUCKETS], np.int32)


def psi(ref_counts: np.ndarray, ref_rows: int, live_counts: np.ndarray, live_rows: int, n_bins: Sequence[int],
        alpha: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """Population Stability Index per column, float64 ``[31]``, and ``beyond_table`` uint64
    ``[31]``.  With ``K = n_bins[j]``: ``p_b = (ref_b + alpha) / (N_ref + alpha K)``, ``q_b``
    likewise for live, ``PSI_j = sum_{b<K} (q_b - p_b) ln(q_b / p_b)``.  A column with
    ``K == 1`` gives exactly 0.  Live counts in cells ``>= K`` (rows binned against a larger
    table: a caller error) are not part of the index; they are summed into ``beyond_table``."""
    ref = np.asarray(ref_counts).astype(np.float64)
    live = np.asarray(live_counts).astype(np.float64)
    out = np.zeros(N_COLS, np.float64)
    beyond = np.zeros(N_COLS, np.uint64)
    for j in range(N_COLS):
        K = int(n_bins[j])
        beyond[j] = int(np.asarray(live_counts)[j, K:].sum())
        if K <= 1:
            continue
        p = (ref[j, :K] + alpha) / (float(ref_rows) + alpha * K)
        q = (live[j, :K] + alpha) / (float(live_rows) + alpha * K)
        out[j] = float(np.sum((q - p) * np.log(q / p)))
    return out, beyond


@dataclass
class DriftReference:
    """The training-time bin distribution a live window is compared against."""
    bits: int                    # 8: G32 rows, 5: G20 rows
    stamp: int                   # the bin table's stamp (BinSpec.stamp)
    n_bins: np.ndarray           # int32 [31]
    counts: np.ndarray           # uint64 [31,256]
    rows: int

    def __post_init__(self):
        if self.bits not in (8, 5):
            raise ValueError("bits is 8 (G32 rows) or 5 (G20 rows)")
        self.n_bins = np.ascontiguousarray(self.n_bins, np.int32).reshape(N_COLS)
        self.counts = np.ascontiguousarray(self.counts, np.uint64).reshape(N_COLS, N_CELLS)
        self.stamp, self.rows = int(self.stamp), int(self.rows)

    @property
    def row_bytes(self) -> int:
        return G32_ROW_BYTES if self.bits == 8 else G20_ROW_BYTES

    @classmethod
    def fit(cls, X: np.ndarray, bins) -> "DriftReference":
        """Encode float32 ``X [n,30]`` against ``bins`` and count on the host."""
        counts, tail = bin_counts(bins.encode(np.ascontiguousarray(X, np.float32)), bins.stamp)
        return cls.from_counts(bins, counts, int(tail[0]))

    @classmethod
    def from_counts(cls, bins, counts: np.ndarray, rows: int) -> "DriftReference":
        return cls(bins.bits, bins.stamp, n_bins_of(bins), np.array(counts, np.uint64), int(rows))

    def compatible(self, bins) -> bool:
        """``bins`` is the table this reference was counted against, as far as the reference
        can tell: same width, stamp and cells per column."""
        return bins is not None and bins.bits == self.bits and bins.stamp == self.stamp and \
            np.array_equal(n_bins_of(bins), self.n_bins)

    def save(self, path: str) -> None:
        from safetensors.numpy import save_file
        save_file({"n_bins": self.n_bins, "counts": self.counts}, path,
                  metadata={"kind": "drift_reference", "version": "1", "bits": str(self.bits),
                            "stamp": str(self.stamp), "rows": str(self.rows)})

    @classmethod
    def load(cls, path: str) -> "DriftReference":
        from safetensors import safe_open
        with safe_open(path, framework="numpy") as f:
            meta = f.metadata() or {}
            if meta.get("kind") != "drift_reference":
                raise ValueError(f"{path}: not a drift reference (kind {meta.get('kind')!r})")
            return cls(int(meta["bits"]), int(meta["stamp"]), f.get_tensor("n_bins"), f.get_tensor("counts"),
                       int(meta["rows"]))


@dataclass
class DriftReport:
    """PSI of one live window against a reference.  ``status[j]`` is ``"stable"`` below
    ``bands[0]``, ``"moderate"`` below ``bands[1]``, else ``"drift"``; with fewer than
    ``min_rows`` live rows ``psi`` is NaN and every status is ``"insufficient"`` (the no-drift
    expectation of PSI is about ``(K - 1)(1 / N_live + 1 / N_ref)``)."""
    psi: np.ndarray
    rows: int
    stale: int
    beyond_table: np.ndarray
    bands: Tuple[float, float] = PSI_BANDS
    min_rows: int = MIN_ROWS
    names: Tuple[str, ...] = COLUMN_NAMES
    status: List[str] = field(default_factory=list)

    def __post_init__(self):
        self.psi = np.asarray(self.psi, np.float64).reshape(N_COLS)
        if self.rows < self.min_rows:
            self.psi = np.full(N_COLS, np.nan)
            self.status = ["insufficient"] * N_COLS
        else:
            lo, hi = self.bands
            self.status = ["stable" if v < lo else "moderate" if v < hi else "drift" for v in self.psi.tolist()]

    @classmethod
    def compare(cls, ref: DriftReference, counts: np.ndarray, tail: np.ndarray, bands=PSI_BANDS,
                min_rows: int = MIN_ROWS, alpha: float = 0.5) -> "DriftReport":
        p, beyond = psi(ref.counts, ref.rows, counts, int(tail[0]), ref.n_bins, alpha)
        return cls(p, int(tail[0]), int(tail[1]), beyond, tuple(bands), int(min_rows))

    @property
    def drifting(self) -> int:
        return sum(s == "drift" for s in self.status)

    def worst(self, k: int = 3) -> List[Tuple[str, float, str]]:
        """The ``k`` columns of largest PSI as ``(name, psi, status)``, largest first."""
        if self.rows < self.min_rows:
            return []
        order = np.argsort(-self.psi, kind="stable")[:k]
        return [(self.names[j], float(self.psi[j]), self.status[j]) for j in order.tolist()]

    def to_json(self, k: int = 3) -> dict:
        nan = self.rows < self.min_rows
        return {"names": list(self.names), "psi": [None if nan else float(v) for v in self.psi.tolist()],
                "status": list(self.status), "rows": self.rows, "stale": self.stale,
                "beyond_table": [int(v) for v in self.beyond_table.tolist()],
                "worst": [{"name": n, "psi": v, "status": s} for n, v, s in self.worst(k)]}
