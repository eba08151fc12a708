"""Feature-drift detection on binned and W64 rows (CPU side: definition, numpy oracles, PSI, report).

A G32 / G20 row is the transaction binned against the model's own split table
(``models.gbdt.BinSpec``, ``bin = #edges < x``), so a per-feature histogram of its bytes is
the feature distribution at exactly the resolution the model can see: a shift inside one bin
cannot change any score.  ``csrc/kernels/drift_hist.hip`` counts those histograms on the GPU
(``ops.kernels.drift_histogram`` / ``DriftMonitor``); ``bin_counts`` here is its oracle.

A W64 row (the MLP / LR path) carries values, not bins, and those models have no table of their
own, so the reference brings one: per-feature quantile edges of the training rows
(``wire_bins_fit``), at most 31 a feature.  ``csrc/kernels/drift_wire.hip`` bins and counts on the
GPU (``ops.kernels.drift_histogram_wire``); ``wire_bin_counts`` is its oracle.

The statistic is the Population Stability Index per column with additive smoothing
(docs/DRIFT.md).  Column 30 is the amount bucket, which every table has.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..contracts.metric_names import AMOUNT_BUCKETS
from ..contracts.transaction import (AMOUNT_COL, FEATURE_NAMES, G20_ROW_BYTES, G32_ROW_BYTES, N_FEATURES, WIRE_ROW_BYTES,
                                     amount_bucket, decode_g20_bins, decode_wire, encode_wire)

N_COLS = N_FEATURES + 1                  # 30 features + the amount bucket (ccfd_abi.h CCFD_DRIFT_COLS)
N_CELLS = 256                            # ccfd_abi.h CCFD_DRIFT_CELLS
N_BUCKETS = len(AMOUNT_BUCKETS) + 1      # 14
COLUMN_NAMES: Tuple[str, ...] = tuple(FEATURE_NAMES) + ("AmountBucket",)
PSI_BANDS = (0.1, 0.25)                  # the conventional bands: < 0.1 stable, < 0.25 moderate, else drift
MIN_ROWS = 10_000
WIRE_BITS = 16                           # DriftReference.bits of a W64 reference (bf16 values; 5 / 8 are bin widths)
WIRE_CELLS = 32                          # cells of a W64 column: <= 31 edges (ccfd_abi.h CCFD_DRIFT_WIRE_EDGES)


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


def wire_bins(edges):
    """``edges`` (a ``BinSpec`` or 30 edge arrays in canonical feature order) as the validated
    wire bin table: a 5-bit ``BinSpec`` -- float32, ascending, distinct, at most 31 a feature --
    whose edges are also finite.  ``ValueError`` otherwise."""
    from .gbdt import BinSpec
    bins = edges if isinstance(edges, BinSpec) else BinSpec([np.asarray(e, np.float32) for e in edges], bits=5)
    if bins.bits != 5:
        bins = bins.with_bits(5)
    for j, e in enumerate(bins.edges):
        if not np.isfinite(e).all():
            raise ValueError(f"feature {j}: wire bin edges must be finite")
    return bins


def wire_bins_fit(X: np.ndarray, cells: int = WIRE_CELLS):
    """Quantile bin table of float32 ``X [n,30]`` for W64 rows: per feature the ``k / cells``
    quantiles (k = 1..cells-1) of the rows after the W64 round trip, so the edges live at the
    resolution the model sees; cast to float32, non-finite values dropped, duplicates merged.  A
    constant feature gets at most one edge."""
    cells = int(cells)
    if not 2 <= cells <= WIRE_CELLS:
        raise ValueError(f"cells must be 2..{WIRE_CELLS}")
    Xw = decode_wire(encode_wire(np.ascontiguousarray(X, np.float32).reshape(-1, N_FEATURES)))
    q = np.arange(1, cells, dtype=np.float64) / cells
    edges = []
    for j in range(N_FEATURES):
        col = Xw[:, j]
        col = col[~np.isnan(col)]
        e = np.quantile(col, q).astype(np.float32) if col.size else np.zeros(0, np.float32)
        edges.append(np.unique(e[np.isfinite(e)]))
    return wire_bins(edges)


def wire_edge_table(bins) -> np.ndarray:
    """float32 ``[30,32]``: each feature's edges followed by ``+inf`` (the device table of
    drift_wire.hip; a ``+inf`` edge is below no value, so the padding never counts)."""
    bins = wire_bins(bins)
    t = np.full((N_FEATURES, WIRE_CELLS), np.inf, np.float32)
    for j, e in enumerate(bins.edges):
        t[j, :e.size] = e
    return t


def wire_bin_counts(rows: np.ndarray, edges) -> Tuple[np.ndarray, np.ndarray]:
    """numpy oracle of the W64 drift kernel: uint8 ``[n,64]`` rows and a wire bin table ->
    ``(counts uint64 [31,256], tail uint64 [2])``.  With ``x = decode_wire(rows)``:
    ``counts[j, #{edges_j < x_j}] += 1`` (IEEE float32 compare: NaN -> cell 0, ``+inf`` -> the last
    cell, a value equal to an edge is not above it, ``-0.0 == 0.0``, denormals kept),
    ``counts[30, amount_bucket(Amount)] += 1``, ``tail = [n, 0]``: W64 rows carry no stamp."""
    rows = np.asarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] != WIRE_ROW_BYTES:
        raise ValueError("rows must be uint8 [n,64] (W64)")
    bins = wire_bins(edges)
    x = decode_wire(rows)
    counts = np.zeros((N_COLS, N_CELLS), np.uint64)
    for j in range(N_FEATURES):
        b = np.searchsorted(bins.edges[j], x[:, j], side="left")          # #edges < x
        b[np.isnan(x[:, j])] = 0
        counts[j] = np.bincount(b, minlength=N_CELLS).astype(np.uint64)
    counts[N_FEATURES] = np.bincount(amount_bucket(x[:, AMOUNT_COL]), minlength=N_CELLS).astype(np.uint64)
    return counts, np.array([rows.shape[0], 0], np.uint64)


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
    bits: int                    # 8: G32 rows, 5: G20 rows, 16: W64 rows (then ``edges`` is the table)
    stamp: int                   # the bin table's stamp (BinSpec.stamp); W64 rows do not carry it
    n_bins: np.ndarray           # int32 [31]
    counts: np.ndarray           # uint64 [31,256]
    rows: int
    edges: Optional[List[np.ndarray]] = None   # W64 only: the wire bin table (30 float32 arrays)

    def __post_init__(self):
        if self.bits not in (8, 5, WIRE_BITS):
            raise ValueError("bits is 8 (G32 rows), 5 (G20 rows) or 16 (W64 rows)")
        self.n_bins = np.ascontiguousarray(self.n_bins, np.int32).reshape(N_COLS)
        self.counts = np.ascontiguousarray(self.counts, np.uint64).reshape(N_COLS, N_CELLS)
        self.stamp, self.rows = int(self.stamp), int(self.rows)
        if self.is_wire:
            if self.edges is None:
                raise ValueError("a W64 drift reference carries its bin edges")
            bins = wire_bins(self.edges)
            self.edges = bins.edges
            if not np.array_equal(n_bins_of(bins), self.n_bins):
                raise ValueError("n_bins does not match the edges")
        elif self.edges is not None:
            raise ValueError("only a W64 drift reference (bits=16) carries edges; binned rows use the model's table")

    @property
    def is_wire(self) -> bool:
        return self.bits == WIRE_BITS

    @property
    def row_bytes(self) -> int:
        return WIRE_ROW_BYTES if self.is_wire else G32_ROW_BYTES if self.bits == 8 else G20_ROW_BYTES

    @property
    def bins(self):
        """The wire bin table of a W64 reference (a 5-bit ``BinSpec``)."""
        if not self.is_wire:
            raise ValueError("a binned drift reference does not carry its table; take the model's bin_spec()")
        return wire_bins(self.edges)

    @classmethod
    def fit_wire(cls, X: np.ndarray, bins=None, cells: int = WIRE_CELLS) -> "DriftReference":
        """The W64 reference of float32 ``X [n,30]``: fit the quantile table when none is given,
        then count ``encode_wire(X)`` on the host."""
        X = np.ascontiguousarray(X, np.float32).reshape(-1, N_FEATURES)
        bins = wire_bins_fit(X, cells) if bins is None else wire_bins(bins)
        counts, tail = wire_bin_counts(encode_wire(X), bins)
        return cls(WIRE_BITS, bins.stamp, n_bins_of(bins), counts, int(tail[0]), bins.edges)

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
        can tell: same width, stamp and cells per column.  Never true of a W64 reference: its
        rows are not encoded against any model's table."""
        return bins is not None and bins.bits == self.bits and bins.stamp == self.stamp and \
            np.array_equal(n_bins_of(bins), self.n_bins)

    def save(self, path: str) -> None:
        from safetensors.numpy import save_file
        tensors = {"n_bins": self.n_bins, "counts": self.counts}
        if self.is_wire:        # the table as BinSpec.to_bytes lays it out: offsets i32 [31], edges f32
            bins = self.bins
            tensors.update(edge_offsets=bins.offsets, edges=np.concatenate(bins.edges + [np.zeros(0, np.float32)]))
        save_file(tensors, path,
                  metadata={"kind": "drift_reference", "version": "2" if self.is_wire else "1", "bits": str(self.bits),
                            "stamp": str(self.stamp), "rows": str(self.rows)})

    @classmethod
    def load(cls, path: str) -> "DriftReference":
        from safetensors import safe_open
        with safe_open(path, framework="numpy") as f:
            meta = f.metadata() or {}
            if meta.get("kind") != "drift_reference":
                raise ValueError(f"{path}: not a drift reference (kind {meta.get('kind')!r})")
            edges = None
            if int(meta["bits"]) == WIRE_BITS:
                off, flat = f.get_tensor("edge_offsets"), f.get_tensor("edges")
                edges = [flat[off[j]:off[j + 1]].copy() for j in range(N_FEATURES)]
            return cls(int(meta["bits"]), int(meta["stamp"]), f.get_tensor("n_bins"), f.get_tensor("counts"),
                       int(meta["rows"]), edges)


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
