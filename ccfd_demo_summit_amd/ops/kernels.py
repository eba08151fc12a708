"""Python API over the fused HIP scoring kernels (csrc/kernels/*.hip).

All functions take torch tensors on the GPU and enqueue on the current torch stream.
There is deliberately NO silent fallback: on a machine with a GPU these ops either run
the gfx950 code object or raise (the CPU oracles live in ``models/*.py``).
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import (ARG_WIRE_G20, ARG_WIRE_G32, ARG_WIRE_W64, BIN_FORMATS, DRIFT_CELLS, DRIFT_COLS, DRIFT_WIRE_EDGES,
                   GBDT_MAX_SPLITS, MODEL_IDS, N_COUNTER_SLOTS, DriftHistArgs, DriftWireArgs, ForestExplainArgs,
                   GbdtExplainArgs, GbdtHistArgs, GbdtUpdateArgs, MlpExplainArgs, OUT_BLOB_BYTES, OUT_FLAG_THRESHOLD,
                   OUTLIER_SLOTS, OutlierArgs, ScoreArgs, ShadowArgs, check, lib)

N_FEATURES = 30
ROW_BYTES = {"f32": 4 * N_FEATURES, "w64": 64, "g32": 32, "g20": 20}
WIRE_FLAGS = {"f32": 0, "w64": ARG_WIRE_W64, "g32": ARG_WIRE_G32, "g20": ARG_WIRE_G32 | ARG_WIRE_G20}


class DeviceModel:
    """A packed model resident in HBM (the blob is broadcast once over RCCL in DP runs)."""

    def __init__(self, model, device: torch.device | str | int = "cuda", wire: bool = False, bins=None):
        """``wire=True``: blob packed for W64 wire rows (MLP / LR; see contracts/transaction.py).
        ``bins``: GBDT on binned rows -- ``True`` for the model's own G32 bin table, ``"g20"``
        for the same table on 20-byte G20 rows (<= 31 thresholds a feature), or a
        ``models.gbdt.BinSpec`` containing its thresholds (e.g. the live logs' spec; its
        ``bits`` select G32 or G20).  A ``TreeEnsemble`` (kind "forest") scores f32 rows by
        default and binned rows when asked by name: ``bins="g32"``, ``bins="g20"`` or a
        ``BinSpec``; ``bins=True`` is refused for it."""
        self.kind = model.kind
        if self.kind not in MODEL_IDS:
            raise ValueError(f"no device kernel for model kind {self.kind!r}")
        if wire and self.kind not in ("mlp", "lr"):
            raise ValueError("W64 wire rows are supported by the MLP and LR kernels" if self.kind != "forest" else
                             "general trees (forest) score f32 rows, or G32 / G20 rows (bins=): no wire=")
        if bins is not None and bins is not False and self.kind not in ("gbdt", "forest"):
            raise ValueError("G32 rows (bins=) are for the GBDT and general-tree kernels")
        if bins is True and self.kind == "forest":
            raise ValueError("general trees (forest) score f32 rows unless a binned format is named: "
                             "bins=\"g32\", bins=\"g20\" or bins=<BinSpec>, not bins=True")
        self.wire = bool(wire)
        if bins is True or bins == "g32":
            bins = model.bin_spec()
        elif isinstance(bins, str) and bins == "g20":
            bins = model.bin_spec(bits=5)
        self.bins = bins if bins is not False else None
        if self.bins is not None:
            packed = model.pack(bins=self.bins)
        else:
            packed = model.pack(wire=True) if wire else model.pack()
        self.blob = torch.from_numpy(np.frombuffer(packed, np.uint8).copy()).to(device)
        self.trees = getattr(model, "n_trees", 0)
        self.depth = getattr(model, "depth", 0)
        self._uploaded()

    def _uploaded(self) -> None:
        # the forest launch caches blob headers by address; this allocation may be a recycled one
        if self.kind == "forest":
            lib().ccfd_forest_blob_changed(C.c_void_p(self.blob.data_ptr()))

    @classmethod
    def from_blob(cls, kind: str, blob: torch.Tensor, trees: int = 0, depth: int = 0,
                  wire: bool = False, bins=None) -> "DeviceModel":
        self = cls.__new__(cls)
        self.kind, self.blob, self.trees, self.depth, self.wire = kind, blob, trees, depth, bool(wire)
        self.bins = bins
        self._uploaded()
        return self

    @property
    def model_id(self) -> int:
        return MODEL_IDS[self.kind]

    @property
    def row_format(self) -> str:
        """Row layout the blob expects: "f32" (30 x f32), "w64", "g32" or "g20"."""
        bins = getattr(self, "bins", None)
        return bins.row_format if bins is not None else "w64" if self.wire else "f32"


class DeviceRules:
    """A compiled routing rule set resident in HBM (``RuleSet.device_program``); pass it to
    ``score(..., rules=)`` / ``StreamEngine(rules=)`` and the kernels' epilogue routes by the
    rules instead of ``proba >= threshold``."""

    def __init__(self, ruleset, device: torch.device | str | int = "cuda"):
        self.ruleset = ruleset
        prog = np.frombuffer(ruleset.device_program(), np.uint8)
        self.prog = torch.from_numpy(prog.copy()).to(device)

    @property
    def ptr(self) -> int:
        return self.prog.data_ptr()


def new_counters(device="cuda") -> torch.Tensor:
    return torch.zeros(N_COUNTER_SLOTS, dtype=torch.int64, device=device)


def check_shadow_pair(dm: DeviceModel, shadow: DeviceModel, rules=None, persist_items: int = 0) -> None:
    """Refuse (``ValueError`` naming the combination) every champion / shadow pair the shadow
    kernels do not cover.  Covered: two MLPs packed for W64 rows (``DeviceModel(..., wire=True)``),
    or two oblivious GBDTs of the same ``(trees, depth)`` packed against the same G32 / G20 bin
    table (``DeviceModel(model, bins=spec)``; ``ObliviousGBDT.padded`` brings a smaller
    challenger to the champion's shape).  Either pair is routed by ``proba >= threshold`` (no
    ``rules``), and a persistent engine must use claimed items (``persist_items`` 0 / 1, not the
    pipelined 2).  Pure host check: no launch, no GPU."""
    from ..models.mlp import WIRE_BLOB_BYTES
    if dm.kind != shadow.kind:
        raise ValueError(f"shadow model: kind mismatch, champion is {dm.kind!r} and shadow is {shadow.kind!r} "
                         "(a shadow is a candidate for swap_model: same kind and shape)")
    if dm.kind == "gbdt" and (dm.row_format in BIN_FORMATS or shadow.row_format in BIN_FORMATS):
        from ..engine.stream_engine import same_bins
        if dm.row_format != shadow.row_format:
            raise ValueError(f"shadow model: the champion GBDT is packed for {dm.row_format} rows and the shadow "
                             f"for {shadow.row_format} rows; both must be packed for the same binned format")
        if not same_bins(dm.bins, shadow.bins):
            raise ValueError(f"shadow model: the champion's and the shadow's {dm.row_format} bin tables differ "
                             f"(stamps {dm.bins.stamp} and {shadow.bins.stamp}); pack the shadow against the "
                             "champion's table (DeviceModel(model, bins=champion.bins))")
        if (dm.trees, dm.depth) != (shadow.trees, shadow.depth):
            raise ValueError(f"shadow model: shape mismatch, the champion is {dm.trees} trees x depth {dm.depth} and "
                             f"the shadow is {shadow.trees} trees x depth {shadow.depth} "
                             "(ObliviousGBDT.padded brings a smaller ensemble to the champion's shape)")
    elif dm.kind != "mlp":
        raise ValueError(f"shadow model: {dm.kind!r} models have no shadow kernel (MLP on W64 rows, or "
                         "oblivious GBDT on G32 / G20 rows: DeviceModel(model, bins=...))")
    else:
        for role, m in (("champion", dm), ("shadow", shadow)):
            if m.row_format != "w64":
                raise ValueError(f"shadow model: the {role} MLP is packed for {m.row_format} rows; "
                                 "both blobs must be packed for W64 rows (DeviceModel(..., wire=True))")
            if m.blob.numel() * m.blob.element_size() != WIRE_BLOB_BYTES:
                raise ValueError(f"shadow model: the {role} blob is not a {WIRE_BLOB_BYTES}-byte W64 MLP blob")
    if rules is not None:
        raise ValueError("shadow model: routing rules present; a shadow routes by proba >= threshold only")
    if int(persist_items) == 2:
        raise ValueError("shadow model: pipelined persistent items (persist_items=2 / \"pipelined\") have no "
                         "shadow kernel; use claimed items")


def score(dm: DeviceModel, x: torch.Tensor, threshold: float = 0.5,
          proba: Optional[torch.Tensor] = None, route: Optional[torch.Tensor] = None,
          counters: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
          flags: int = 0, rules: Optional[DeviceRules] = None, shadow: Optional[DeviceModel] = None,
          shadow_proba: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
    """Fused score of x [n,30] (float32, CUDA) -- or, for a ``wire`` model, W64 rows
    ([n,64] uint8 or [n,16] float32 view), for a ``bins`` model G32 / G20 rows ([n,32] / [n,20] u8) --
    returns (proba_1 [n] f32, route [n] u8).
    ``flags``: extra ``CCFD_ARG_*`` bits (ablation switches for profiling).
    ``shadow``: a challenger scored on the same rows in the same pass -- an MLP (W64 blob, like
    ``dm``), or an oblivious GBDT of ``dm``'s shape packed against ``dm``'s G32 / G20 bin table;
    returns (proba_1, route, shadow proba_1 [n] f32) and adds the ``CNT_SHADOW_*`` counters
    (``check_shadow_pair`` lists what is refused)."""
    if shadow is not None:
        check_shadow_pair(dm, shadow, rules=rules)
    elif shadow_proba is not None:
        raise ValueError("shadow_proba= without shadow=")
    fmt = dm.row_format
    wire = fmt != "f32"
    if wire:
        rb = ROW_BYTES[fmt]
        if not x.is_cuda or x.dim() != 2 or x.element_size() * x.shape[1] != rb or not x.is_contiguous():
            raise ValueError(f"{fmt} model: x must be contiguous CUDA {fmt.upper()} rows ([n,{rb}] u8)")
        if fmt in BIN_FORMATS and rules is not None and rules.ruleset.feature_vars():
            raise ValueError("G32 / G20 rows carry bins, not feature values: routing rules may only use proba_1")
    elif not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != N_FEATURES:
        raise ValueError("x must be a CUDA float32 tensor of shape [n, 30]")
    if x.stride(1) != 1:
        x = x.contiguous()
    n = x.shape[0]
    if proba is None:
        proba = torch.empty(n, dtype=torch.float32, device=x.device)
    if route is None:
        route = torch.empty(n, dtype=torch.uint8, device=x.device)
    a = ScoreArgs()
    a.x = x.data_ptr()
    a.ld = ROW_BYTES[fmt] // 4 if wire else x.stride(0)
    a.flags = WIRE_FLAGS[fmt] | int(flags)
    a.n = n
    a.model = dm.model_id
    a.blob = dm.blob.data_ptr()
    a.threshold = float(threshold)
    a.gbdt_trees = dm.trees
    a.gbdt_depth = dm.depth
    a.proba = proba.data_ptr()
    a.route = route.data_ptr()
    a.counters = counters.data_ptr() if counters is not None else None
    a.rules = rules.ptr if rules is not None else None
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    if shadow is not None:
        if shadow_proba is None:
            shadow_proba = torch.empty(n, dtype=torch.float32, device=x.device)
        elif not shadow_proba.is_cuda or shadow_proba.dtype != torch.float32 or shadow_proba.numel() < n or \
                not shadow_proba.is_contiguous():
            raise ValueError("shadow_proba must be a contiguous CUDA float32 tensor of at least n elements")
        sa = ShadowArgs()
        sa.base = a
        sa.shadow_blob = shadow.blob.data_ptr()
        sa.shadow_proba = shadow_proba.data_ptr()
        check(lib().ccfd_score_launch_shadow(C.byref(sa), C.c_void_p(s.cuda_stream)), "ccfd_score_launch_shadow")
        return proba, route, shadow_proba
    check(lib().ccfd_score_launch(C.byref(a), C.c_void_p(s.cuda_stream)), "ccfd_score_launch")
    return proba, route


# ---------------------------------------------------------------------------- GBDT training
def _g32_rows(rows: torch.Tensor) -> int:
    if not rows.is_cuda or rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != ROW_BYTES["g32"] or \
            not rows.is_contiguous():
        raise ValueError("rows must be contiguous CUDA G32 rows ([n,32] u8)")
    return rows.shape[0]


def _f32_vec(t: torch.Tensor, n: int, name: str, like: torch.Tensor) -> None:
    if not t.is_cuda or t.device != like.device or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n or \
            not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous CUDA float32 tensor of shape [{n}] on the rows' device")


def _set_splits(a, splits) -> int:
    splits = [(int(f), int(b)) for f, b in splits]
    if len(splits) > GBDT_MAX_SPLITS:
        raise ValueError(f"at most {GBDT_MAX_SPLITS} splits (got {len(splits)})")
    for k, (f, b) in enumerate(splits):
        a.split_feat[k], a.split_bin[k] = f, b
    return len(splits)


def gbdt_histogram(rows: torch.Tensor, grad: torch.Tensor, hess: torch.Tensor, n_bins: int, splits=(),
                   out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                   stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One level's gradient / hessian histograms of an oblivious tree over G32 rows
    (csrc/kernels/train_hist.hip): with ``d = len(splits)`` pairs ``(feature, bin)`` chosen so far,
    ``leaf(i) = sum_k (rows[i, feature_k] > bin_k) << k`` and
    ``G[leaf(i), f, rows[i, f]] += grad[i]`` for every row and feature (``H`` with ``hess``).
    Returns ``(G, H)``, float32 ``[2^d, 30, n_bins]``, overwritten (``out=`` reuses two such
    tensors).  Supported: d <= 7, 2 <= n_bins <= 64, n >= 1; anything else is refused by the
    library (``RuntimeError`` with its message).  Bytes 30 / 31 of a row are ignored; a bin byte
    >= n_bins is skipped.  The sums are f32 in no fixed order, so the last bits can differ from
    run to run (as with ``scatter_add_``)."""
    n = _g32_rows(rows)
    _f32_vec(grad, n, "grad", rows)
    _f32_vec(hess, n, "hess", rows)
    a = GbdtHistArgs()
    d = _set_splits(a, splits)
    shape = (1 << d, N_FEATURES, int(n_bins))
    if out is None:
        out = (torch.empty(shape, dtype=torch.float32, device=rows.device),
               torch.empty(shape, dtype=torch.float32, device=rows.device))
    G, H = out
    for name, t in (("G", G), ("H", H)):
        if not t.is_cuda or t.device != rows.device or t.dtype != torch.float32 or tuple(t.shape) != shape or \
                not t.is_contiguous():
            raise ValueError(f"out {name} must be a contiguous CUDA float32 tensor of shape {list(shape)}")
    a.rows, a.grad, a.hess = rows.data_ptr(), grad.data_ptr(), hess.data_ptr()
    a.G, a.H = G.data_ptr(), H.data_ptr()
    a.n, a.n_bins, a.level = n, int(n_bins), d
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    check(lib().ccfd_gbdt_hist_launch(C.byref(a), C.c_void_p(s.cuda_stream)), "ccfd_gbdt_hist_launch")
    return G, H


def gbdt_apply_tree(rows: torch.Tensor, raw: torch.Tensor, leaf_val: torch.Tensor, splits,
                    y: Optional[torch.Tensor] = None, grad: Optional[torch.Tensor] = None,
                    hess: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """Close a tree of ``depth = len(splits)`` (1..8): ``raw[i] += leaf_val[leaf(i)]`` in place,
    with ``leaf(i)`` as in ``gbdt_histogram``.  With labels ``y`` it also writes the next tree's
    logloss gradients ``grad = sigmoid(raw) - y`` and ``hess = max(p (1 - p), 1e-6)`` (allocated
    unless given) and returns ``(raw, grad, hess)``; without ``y`` it returns ``(raw, None, None)``."""
    n = _g32_rows(rows)
    _f32_vec(raw, n, "raw", rows)
    a = GbdtUpdateArgs()
    depth = _set_splits(a, splits)
    _f32_vec(leaf_val, 1 << depth, "leaf_val", rows)
    if y is None:
        if grad is not None or hess is not None:
            raise ValueError("grad= / hess= need y=")
    else:
        _f32_vec(y, n, "y", rows)
        grad = torch.empty_like(raw) if grad is None else grad
        hess = torch.empty_like(raw) if hess is None else hess
        _f32_vec(grad, n, "grad", rows)
        _f32_vec(hess, n, "hess", rows)
        a.y, a.grad, a.hess = y.data_ptr(), grad.data_ptr(), hess.data_ptr()
    a.rows, a.leaf_val, a.raw = rows.data_ptr(), leaf_val.data_ptr(), raw.data_ptr()
    a.n, a.depth = n, depth
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    check(lib().ccfd_gbdt_update_launch(C.byref(a), C.c_void_p(s.cuda_stream)), "ccfd_gbdt_update_launch")
    return raw, grad, hess


# ---------------------------------------------------------------------------- explanations
class DeviceExplainer:
    """The explain table of a tree model with cover resident in HBM: the 'GBX1' table of an
    oblivious GBDT (``ObliviousGBDT.fit_cover``) for ``explain_gbdt``, or the 'FRX1' path table of
    a general ensemble (kind "forest"; ``TreeEnsemble.fit_cover`` or an importer's cover) for
    ``explain_forest``, together with the workspace that kernel's small batches need.  ``bins``:
    the 8-bit ``BinSpec`` the G32 rows were encoded with (default: the model's own table).
    ``base_value + phi.sum(1)`` is the raw score."""

    def __init__(self, model, bins=None, device: torch.device | str | int = "cuda"):
        self.kind = getattr(model, "kind", None)
        if self.kind not in ("gbdt", "forest"):
            raise ValueError(f"no explain kernel for model kind {self.kind!r} (oblivious GBDT and general tree "
                             "ensembles only)")
        self.bins = bins if bins is not None else model.bin_spec()
        if self.kind == "gbdt":
            from ..models.explain import ExplainTable, base_value
            packed = ExplainTable.pack(model, self.bins)
            self.base_value = base_value(model)
        else:
            from ..models.explain_forest import ForestExplainTable, forest_base_value
            packed = ForestExplainTable.pack(model, self.bins)
            self.base_value = forest_base_value(model)
            self.paths, self.width = (int(v) for v in np.frombuffer(packed, np.int32, 2, 8))
            self.slices, self.rec_words = (int(v) for v in np.frombuffer(packed, np.int32, 2, 24))
            self._workspace = {}         # stream handle -> float32 tensor of partial sums
        self.blob = torch.from_numpy(np.frombuffer(packed, np.uint8).copy()).to(device)
        self.trees, self.depth = model.n_trees, model.depth
        self.device = self.blob.device

    def workspace(self, n: int, stream: torch.cuda.Stream) -> Optional[torch.Tensor]:
        """The partial-sum buffer ``explain_forest`` needs for ``n`` rows on ``stream`` (``None``
        when the launch needs none).  One buffer a stream, grown on demand and kept."""
        need = int(lib().ccfd_forest_explain_workspace_bytes(int(n), self.slices))
        if need == 0:
            return None
        ws = self._workspace.get(stream.cuda_stream)
        if ws is None or ws.numel() * 4 < need:
            ws = torch.empty(need // 4, dtype=torch.float32, device=self.device)
            self._workspace[stream.cuda_stream] = ws
        ws.record_stream(stream)
        return ws

    def explain(self, X: np.ndarray) -> Tuple[np.ndarray, float]:
        """float32 [n,30] host rows -> (phi float32 [n,30] numpy, base_value)."""
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2 or X.shape[1] != N_FEATURES:
            raise ValueError("X must be float32 [n, 30]")
        rows = torch.from_numpy(np.ascontiguousarray(self.bins.encode(X))).to(self.device)
        fn = explain_gbdt if self.kind == "gbdt" else explain_forest
        return fn(self, rows).cpu().numpy(), self.base_value


def _explain_out(ex: DeviceExplainer, kind: str, rows: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    if getattr(ex, "kind", None) != kind:
        raise ValueError(f"the explainer holds a {getattr(ex, 'kind', None)!r} table: use "
                         f"explain_{'gbdt' if kind == 'forest' else 'forest'} (or DeviceExplainer.explain)")
    n = _g32_rows(rows)
    if rows.device != ex.blob.device:
        raise ValueError("rows must be on the explainer's device")
    shape = (n, N_FEATURES)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rows.device)
    elif not out.is_cuda or out.device != rows.device or out.dtype != torch.float32 or tuple(out.shape) != shape or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous CUDA float32 tensor of shape {list(shape)} on the rows' device")
    return out


def explain_gbdt(ex: DeviceExplainer, rows: torch.Tensor, out: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Exact per-feature Shapley values (margin space) of G32 ``rows`` ([n,32] u8, CUDA) under
    ``ex``'s model (csrc/kernels/explain_gbdt.hip; definition in docs/EXPLAIN.md): returns
    ``phi`` float32 ``[n, 30]`` (``out=`` reuses such a tensor).  A row whose stamp differs from
    the table's gets NaN in all 30 entries; a feature no tree tests gets exactly 0.  The
    summation order is fixed: two runs give identical bits."""
    out = _explain_out(ex, "gbdt", rows, out)
    a = GbdtExplainArgs()
    a.rows, a.blob, a.phi = rows.data_ptr(), ex.blob.data_ptr(), out.data_ptr()
    a.n, a.blob_bytes, a.trees, a.depth = rows.shape[0], ex.blob.numel(), ex.trees, ex.depth
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    check(lib().ccfd_gbdt_explain_launch(C.byref(a), C.c_void_p(s.cuda_stream)), "ccfd_gbdt_explain_launch")
    return out


def explain_forest(ex: DeviceExplainer, rows: torch.Tensor, out: Optional[torch.Tensor] = None,
                   stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """``explain_gbdt``'s contract for a general tree ensemble (csrc/kernels/explain_forest.hip):
    exact per-feature Shapley values of the raw score of G32 ``rows`` ([n,32] u8, CUDA) under
    ``ex``'s ensemble, ``phi`` float32 ``[n, 30]`` (``out=`` reuses such a tensor).  A row whose
    stamp differs from the table's gets NaN in all 30 entries; a feature that no split with
    cover tests gets exactly 0.  Every sum has a fixed order that depends on neither ``n`` nor
    the other rows: a row explained alone gets the bits it gets in a batch.  Small batches
    under a large table use ``ex.workspace`` on the launch's stream."""
    out = _explain_out(ex, "forest", rows, out)
    n = rows.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    ws = ex.workspace(n, s)
    a = ForestExplainArgs()
    a.rows, a.blob, a.phi = rows.data_ptr(), ex.blob.data_ptr(), out.data_ptr()
    a.workspace, a.workspace_bytes = (ws.data_ptr(), ws.numel() * 4) if ws is not None else (None, 0)
    a.n, a.blob_bytes = n, ex.blob.numel()
    a.paths, a.width, a.slices, a.rec_words = ex.paths, ex.width, ex.slices, ex.rec_words
    check(lib().ccfd_forest_explain_launch(C.byref(a), C.c_void_p(s.cuda_stream)), "ccfd_forest_explain_launch")
    return out


class DeviceMlpExplainer:
    """The W64 wire blob of an MLP with a baseline (``MLPModel.fit_baseline``) and the 'MLX1'
    table of ``perms`` sampled permutations (``models.explain_mlp.MlpExplainTable``) resident in
    HBM, for ``explain_mlp``.  ``base_value`` is the baseline's wire logit;
    ``base_value + phi.sum(1)`` is the row's logit for every ``perms``."""

    kind = "mlp"

    def __init__(self, model, perms: int = 64, seed: int = 0, device: torch.device | str | int = "cuda"):
        if getattr(model, "kind", None) != "mlp":
            raise ValueError(f"no sampled-Shapley kernel for model kind {getattr(model, 'kind', None)!r} (MLP only; "
                             "LR has the closed form models.explain_mlp.shapley_lr)")
        from ..models.explain_mlp import MlpExplainTable, mlp_base_value
        packed = MlpExplainTable.pack(model, perms, seed)          # refuses a model without baseline
        self.perms, self.seed = int(perms), int(seed)
        self.base_value = mlp_base_value(model)
        self.table_head = tuple(int(v) for v in np.frombuffer(packed, np.uint32, 2, 0))
        self.table = torch.from_numpy(np.frombuffer(packed, np.uint8).copy()).to(device)
        self.blob = torch.from_numpy(np.frombuffer(model.pack(wire=True), np.uint8).copy()).to(self.table.device)
        self.device = self.table.device

    def explain(self, X: np.ndarray) -> Tuple[np.ndarray, float]:
        """float32 [n,30] host rows -> (phi float32 [n,30] numpy, base_value)."""
        from ..contracts.transaction import encode_wire
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2 or X.shape[1] != N_FEATURES:
            raise ValueError("X must be float32 [n, 30]")
        rows = torch.from_numpy(encode_wire(X)).to(self.device)
        return explain_mlp(self, rows).cpu().numpy(), self.base_value


MLP_EXPLAIN_WORKGROUPS = 2048       # default upper bound on explain_mlp's grid (4 rows a workgroup at a time)


def explain_mlp(ex: DeviceMlpExplainer, rows: torch.Tensor, out: Optional[torch.Tensor] = None,
                z_out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                max_workgroups: int = MLP_EXPLAIN_WORKGROUPS) -> torch.Tensor:
    """Sampled Shapley values (logit space) of W64 ``rows`` ([n,64] u8, CUDA) under ``ex``'s MLP,
    baseline and permutations (csrc/kernels/explain_mlp.hip; definition in docs/EXPLAIN.md):
    returns ``phi`` float32 ``[n, 30]`` in canonical feature order (``out=`` reuses such a tensor).
    ``z_out``: a float32 ``[n, perms, 32]`` tensor that receives every coalition row's logit.
    A position whose bits equal the baseline's gets exactly 0.  The sum over permutations has a
    fixed order: two runs, any ``max_workgroups`` (the upper bound on the grid) and any batch
    around a row give that row identical bits."""
    if not isinstance(ex, DeviceMlpExplainer):
        raise ValueError("explain_mlp needs a DeviceMlpExplainer (tree models: DeviceExplainer and explain_gbdt / "
                         "explain_forest)")
    rb = ROW_BYTES["w64"]
    if not rows.is_cuda or rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != rb or \
            not rows.is_contiguous():
        raise ValueError(f"rows must be contiguous CUDA W64 rows ([n,{rb}] u8)")
    if rows.device != ex.device:
        raise ValueError("rows must be on the explainer's device")
    n = rows.shape[0]
    shape = (n, N_FEATURES)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rows.device)
    elif not out.is_cuda or out.device != rows.device or out.dtype != torch.float32 or tuple(out.shape) != shape or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous CUDA float32 tensor of shape {list(shape)} on the rows' device")
    zshape = (n, ex.perms, 32)
    if z_out is not None and (not z_out.is_cuda or z_out.device != rows.device or z_out.dtype != torch.float32 or
                              tuple(z_out.shape) != zshape or not z_out.is_contiguous()):
        raise ValueError(f"z_out must be a contiguous CUDA float32 tensor of shape {list(zshape)} on the rows' device")
    a = MlpExplainArgs()
    a.rows, a.blob, a.table, a.phi = rows.data_ptr(), ex.blob.data_ptr(), ex.table.data_ptr(), out.data_ptr()
    a.z_out = z_out.data_ptr() if z_out is not None else None
    a.n, a.table_bytes, a.blob_bytes = n, ex.table.numel(), ex.blob.numel()
    a.perms, a.max_workgroups = ex.perms, int(max_workgroups)
    a.table_head[0], a.table_head[1] = ex.table_head
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    check(lib().ccfd_mlp_explain_launch(C.byref(a), C.c_void_p(s.cuda_stream)), "ccfd_mlp_explain_launch")
    return out


# ---------------------------------------------------------------------------- feature drift
_DRIFT_FMT = {ROW_BYTES["g32"]: "g32", ROW_BYTES["g20"]: "g20"}
DRIFT_STAGE_ROWS = 65536        # rows of one pinned staging buffer of DriftMonitor.observe_host


def new_drift_counts(device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """Zeroed ``(counts uint64 [31,256], tail uint64 [2])`` for ``drift_histogram``."""
    return (torch.zeros((DRIFT_COLS, DRIFT_CELLS), dtype=torch.int64, device=device).view(torch.uint64),
            torch.zeros(2, dtype=torch.int64, device=device).view(torch.uint64))


def _drift_launch(ptr: int, n: int, fmt: str, stamp: int, counts: torch.Tensor, tail: torch.Tensor,
                  max_workgroups: int, stream: torch.cuda.Stream) -> None:
    a = DriftHistArgs()
    a.rows, a.counts, a.tail = ptr, counts.data_ptr(), tail.data_ptr()
    a.n, a.wire, a.stamp, a.max_workgroups = int(n), WIRE_FLAGS[fmt], int(stamp), int(max_workgroups)
    check(lib().ccfd_drift_hist_launch(C.byref(a), C.c_void_p(stream.cuda_stream)), "ccfd_drift_hist_launch")


def drift_histogram(rows: torch.Tensor, stamp: int, counts: Optional[torch.Tensor] = None,
                    tail: Optional[torch.Tensor] = None, max_workgroups: int = 512,
                    stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-feature bin counts of binned rows (csrc/kernels/drift_hist.hip; oracle
    ``models.drift.bin_counts``).  ``rows``: contiguous CUDA uint8 ``[n,32]`` (G32) or ``[n,20]``
    (G20); the format follows from the width.  For every row whose stamp equals ``stamp``:
    ``counts[j, bin_j] += 1`` for j < 30, ``counts[30, amount bucket] += 1`` and ``tail[0] += 1``;
    a row with another stamp adds 1 to ``tail[1]`` and nothing else.  G20 rows only touch cells
    0..31 of a column.  Returns ``(counts uint64 [31,256], tail uint64 [2])``.  Missing outputs are
    allocated zeroed; given ones are ACCUMULATED into (the launch never zeroes), so a window is
    whatever was summed since the caller last zeroed them.  Integer sums: exact, identical from
    run to run and for every ``max_workgroups`` (the upper bound on the grid).  ``n == 0``
    launches nothing; a stamp outside 1..255 (G20: 1..63), G32 rows off a 16-byte boundary or
    G20 rows off a 4-byte one are refused by the library (``RuntimeError`` with its message)."""
    if not rows.is_cuda or rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] not in _DRIFT_FMT or \
            not rows.is_contiguous():
        raise ValueError("rows must be contiguous CUDA G32 / G20 rows ([n,32] or [n,20] u8)")
    if counts is None or tail is None:
        fresh = new_drift_counts(rows.device)
        counts = fresh[0] if counts is None else counts
        tail = fresh[1] if tail is None else tail
    for name, t, shape in (("counts", counts, (DRIFT_COLS, DRIFT_CELLS)), ("tail", tail, (2,))):
        if not t.is_cuda or t.device != rows.device or t.dtype != torch.uint64 or tuple(t.shape) != shape or \
                not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous CUDA uint64 tensor of shape {list(shape)} on the rows' device")
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    _drift_launch(rows.data_ptr(), rows.shape[0], _DRIFT_FMT[rows.shape[1]], stamp, counts, tail, max_workgroups, s)
    return counts, tail


DRIFT_WIRE_MAX_WORKGROUPS = 1024    # measured: 0.095 ms on 2 M rows against 0.123 ms at 512 (docs/DRIFT.md)
_wire_tables: dict = {}         # (edge table bytes, device index) -> float32 [30,32] on that device


def drift_wire_table(bins, device) -> torch.Tensor:
    """The ``+inf``-padded float32 ``[30,32]`` edge table of ``bins`` (a wire bin table:
    ``models.drift.wire_bins``) on ``device``, uploaded once per table and device."""
    from ..models.drift import wire_edge_table
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    host = wire_edge_table(bins)
    key = (host.tobytes(), device.index)
    t = _wire_tables.get(key)
    if t is None:
        if len(_wire_tables) >= 16:              # a process holds a handful of tables at most
            _wire_tables.clear()
        t = torch.from_numpy(host).to(device)
        torch.cuda.current_stream(device).synchronize()      # usable from any stream from here on
        _wire_tables[key] = t
    return t


def _drift_wire_launch(ptr: int, n: int, table: torch.Tensor, counts: torch.Tensor, tail: torch.Tensor,
                       max_workgroups: int, stream: torch.cuda.Stream) -> None:
    a = DriftWireArgs()
    a.rows, a.edges, a.counts, a.tail = ptr, table.data_ptr(), counts.data_ptr(), tail.data_ptr()
    a.n, a.max_workgroups = int(n), int(max_workgroups)
    check(lib().ccfd_drift_wire_launch(C.byref(a), C.c_void_p(stream.cuda_stream)), "ccfd_drift_wire_launch")


def drift_histogram_wire(rows: torch.Tensor, bins, counts: Optional[torch.Tensor] = None,
                         tail: Optional[torch.Tensor] = None, max_workgroups: int = DRIFT_WIRE_MAX_WORKGROUPS,
                         stream: Optional[torch.cuda.Stream] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-feature quantile-bin counts of W64 rows (csrc/kernels/drift_wire.hip; oracle
    ``models.drift.wire_bin_counts``).  ``rows``: contiguous CUDA uint8 ``[n,64]``; ``bins``: the wire
    bin table (a ``BinSpec`` of at most 31 finite edges a feature, e.g. ``wire_bins_fit`` or
    ``DriftReference.bins``), or its device table from ``drift_wire_table``.  For every row
    ``counts[j, #{edges_j < x_j}] += 1`` for j < 30 (IEEE float32 compare on the decoded value),
    ``counts[30, amount bucket] += 1`` and ``tail[0] += 1``; ``tail[1]`` stays as it is (W64 rows
    carry no stamp).  Outputs, accumulation, exactness and ``max_workgroups`` as
    ``drift_histogram``, but the default grid bound is 1024: the binning wants more waves a CU.  Rows off a 16-byte boundary are refused by the library."""
    if not rows.is_cuda or rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != ROW_BYTES["w64"] or \
            not rows.is_contiguous():
        raise ValueError("rows must be contiguous CUDA W64 rows ([n,64] u8)")
    table = bins if isinstance(bins, torch.Tensor) else drift_wire_table(bins, rows.device)
    if table.device != rows.device or table.dtype != torch.float32 or tuple(table.shape) != (DRIFT_COLS - 1, DRIFT_WIRE_EDGES) \
            or not table.is_contiguous():
        raise ValueError("the edge table must be a contiguous float32 [30,32] tensor on the rows' device")
    if counts is None or tail is None:
        fresh = new_drift_counts(rows.device)
        counts = fresh[0] if counts is None else counts
        tail = fresh[1] if tail is None else tail
    for name, t, shape in (("counts", counts, (DRIFT_COLS, DRIFT_CELLS)), ("tail", tail, (2,))):
        if not t.is_cuda or t.device != rows.device or t.dtype != torch.uint64 or tuple(t.shape) != shape or \
                not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous CUDA uint64 tensor of shape {list(shape)} on the rows' device")
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    _drift_wire_launch(rows.data_ptr(), rows.shape[0], table, counts, tail, max_workgroups, s)
    return counts, tail


class DriftMonitor:
    """A tumbling window of bin counts on the GPU, compared against a ``models.drift.DriftReference``
    (G32 / G20 rows of a binned reference, or W64 rows of a ``fit_wire`` one, whose padded edge
    table the monitor holds on its device).

    ``observe(rows)`` counts CUDA rows on the caller's current stream; ``observe_host(rows)``
    copies a host ``uint8 [k, row_bytes]`` view into one of two pinned staging buffers and counts
    it from there on the monitor's own stream (the kernel reads the pinned memory directly, as
    the engines read their logs), so the caller's memory is free again when it returns.
    ``report()`` reads the counts back and computes PSI on the host.  Thread-safe (one lock)."""

    def __init__(self, reference, device: torch.device | str | int = "cuda", max_workgroups: Optional[int] = None,
                 min_rows: int = 10_000, bands=(0.1, 0.25)):
        """``max_workgroups``: the launches' grid bound; ``None`` is each kernel's default (512 for
        binned rows, 1024 for W64 rows)."""
        from ..engine.stream_engine import PinnedArray
        self.reference = reference
        wire = getattr(reference, "is_wire", False)
        self.fmt = "w64" if wire else "g32" if reference.bits == 8 else "g20"
        self.row_bytes = ROW_BYTES[self.fmt]
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if max_workgroups is None:
            max_workgroups = DRIFT_WIRE_MAX_WORKGROUPS if wire else 512
        self.max_workgroups, self.min_rows, self.bands = int(max_workgroups), int(min_rows), tuple(bands)
        self.counts, self.tail = new_drift_counts(self.device)
        self._table = drift_wire_table(reference.bins, self.device) if wire else None    # W64: the padded edges
        with torch.cuda.device(self.device):
            self._stream = torch.cuda.Stream(self.device)
            self._stage = [PinnedArray((DRIFT_STAGE_ROWS, self.row_bytes), np.uint8) for _ in range(2)]
            self._stage_ptr = [int(lib().ccfd_host_device_ptr(C.c_void_p(p.ptr))) for p in self._stage]
        self._busy: list = [None, None]          # event of the last launch that read each buffer
        self._next = 0
        self._streams = {}                       # streams observe() launched on since the last report
        self._lock = threading.Lock()
        torch.cuda.current_stream(self.device).synchronize()     # the zeroed outputs, before any side-stream launch

    def _check(self, width: int) -> None:
        if width != self.row_bytes:
            raise ValueError(f"drift reference is for {self.fmt} rows ({self.row_bytes} B, bits={self.reference.bits}); "
                             f"got rows of {width} B")

    def observe(self, rows: torch.Tensor) -> None:
        if rows.dim() != 2:
            raise ValueError("rows must be [n, row_bytes] u8")
        self._check(rows.shape[1])
        with self._lock:
            s = torch.cuda.current_stream(self.device)
            if self._table is not None:
                drift_histogram_wire(rows, self._table, self.counts, self.tail, self.max_workgroups, s)
            else:
                drift_histogram(rows, self.reference.stamp, self.counts, self.tail, self.max_workgroups, s)
            self._streams[s.cuda_stream] = s

    def observe_host(self, rows: np.ndarray) -> None:
        rows = np.asarray(rows)
        if rows.dtype != np.uint8 or rows.ndim != 2:
            raise ValueError("rows must be a host uint8 [k, row_bytes] array")
        self._check(rows.shape[1])
        with self._lock, torch.cuda.device(self.device):     # torch's current device is per thread
            for lo in range(0, rows.shape[0], DRIFT_STAGE_ROWS):
                chunk = rows[lo:lo + DRIFT_STAGE_ROWS]
                b = self._next
                self._next ^= 1
                if self._busy[b] is not None:
                    self._busy[b].synchronize()          # the launch that read this buffer last
                k = chunk.shape[0]
                self._stage[b].array[:k] = chunk
                if self._table is not None:
                    _drift_wire_launch(self._stage_ptr[b], k, self._table, self.counts, self.tail,
                                       self.max_workgroups, self._stream)
                else:
                    _drift_launch(self._stage_ptr[b], k, self.fmt, self.reference.stamp, self.counts, self.tail,
                                  self.max_workgroups, self._stream)
                ev = torch.cuda.Event()
                ev.record(self._stream)
                self._busy[b] = ev

    def report(self, reset: bool = False):
        """``DriftReport`` of the window so far; ``reset=True`` starts the next one."""
        from ..models.drift import DriftReport
        with self._lock:
            self._stream.synchronize()
            for s in self._streams.values():
                s.synchronize()
            self._streams.clear()
            with torch.cuda.device(self.device):
                counts = self.counts.view(torch.int64).cpu().numpy().view(np.uint64)
                tail = self.tail.view(torch.int64).cpu().numpy().view(np.uint64)
                if reset:
                    self.counts.view(torch.int64).zero_()
                    self.tail.view(torch.int64).zero_()
                    torch.cuda.current_stream(self.device).synchronize()
        return DriftReport.compare(self.reference, counts, tail, self.bands, self.min_rows)

    def close(self) -> None:
        with self._lock:
            self._stream.synchronize()
            for p in self._stage:
                p.free()
            self._stage = []


# ---------------------------------------------------------------------------- outlier scores
OUTLIER_MAX_WORKGROUPS = 1024       # the launches' default grid bound (4 waves, 128 rows a workgroup and stride)


class DeviceOutlierModel:
    """A ``models.outlier.OutlierAE`` packed (``'AEW1'`` blob) and resident in HBM."""

    def __init__(self, model, device: torch.device | str | int = "cuda"):
        if getattr(model, "kind", None) != "ae":
            raise ValueError(f"the outlier kernel takes an OutlierAE (kind 'ae'), not kind {getattr(model, 'kind', None)!r}")
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        packed = model.pack()
        self.latent = int(model.latent)
        self.threshold = float(model.threshold)
        self.magic = int(np.frombuffer(packed, np.int32, 1)[0])
        self.blob = torch.from_numpy(np.frombuffer(packed, np.uint8).copy()).to(self.device)
        torch.cuda.current_stream(self.device).synchronize()      # usable from any stream from here on


def new_outlier_counts(device="cuda") -> torch.Tensor:
    """Zeroed ``counts uint64 [66]`` for ``outlier_scores`` (slots: ``models.outlier.SLOT_*``)."""
    return torch.zeros(OUTLIER_SLOTS, dtype=torch.int64, device=device).view(torch.uint64)


def _outlier_launch(dev_model: DeviceOutlierModel, ptr: int, n: int, score_ptr: int, resid_ptr: Optional[int],
                    counts_ptr: Optional[int], threshold: Optional[float], max_workgroups: int,
                    stream: torch.cuda.Stream) -> None:
    a = OutlierArgs()
    a.rows, a.blob, a.score, a.resid_out, a.counts = ptr, dev_model.blob.data_ptr(), score_ptr, resid_ptr, counts_ptr
    a.n, a.blob_bytes, a.latent, a.magic = int(n), dev_model.blob.numel(), dev_model.latent, dev_model.magic
    a.max_workgroups = int(max_workgroups)
    if threshold is not None:
        a.flags, a.threshold = OUT_FLAG_THRESHOLD, float(threshold)
    check(lib().ccfd_outlier_ae_launch(C.byref(a), C.c_void_p(stream.cuda_stream)), "ccfd_outlier_ae_launch")


def outlier_scores(dev_model: DeviceOutlierModel, rows: torch.Tensor, out: Optional[torch.Tensor] = None,
                   resid_out: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                   threshold: Optional[float] = None, max_workgroups: int = OUTLIER_MAX_WORKGROUPS,
                   stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Autoencoder reconstruction-error scores of W64 rows (csrc/kernels/outlier_ae.hip; oracle
    ``models.outlier.OutlierAE.wire_scores``).  ``rows``: contiguous CUDA uint8 ``[n,64]``.  Returns
    ``out``: float32 ``[n]`` (allocated when missing).  ``resid_out``: optional float32 ``[n,32]``, the
    residuals in wire order (positions 30 / 31 are 0).  ``counts``: optional uint64 ``[66]``
    (``new_outlier_counts``), ACCUMULATED into: rows, rows with ``score > threshold``, rows with a
    non-finite score, the 32 ``score_cell`` cells of the finite scores and, for every flagged row,
    the feature of its largest squared residual.  ``threshold``: ``None`` is the model's.  A row
    with a non-finite feature scores NaN.  Integer counts: exact and the same for every
    ``max_workgroups`` (the upper bound on the grid); a row's score does not depend on the batch
    around it.  ``n == 0`` launches nothing; rows off a 16-byte boundary are refused by the library."""
    if not isinstance(dev_model, DeviceOutlierModel):
        raise ValueError("dev_model must be a DeviceOutlierModel")
    if not rows.is_cuda or rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != ROW_BYTES["w64"] or \
            not rows.is_contiguous():
        raise ValueError("rows must be contiguous CUDA W64 rows ([n,64] u8)")
    if rows.device != dev_model.device:
        raise ValueError("rows must be on the outlier model's device")
    n = rows.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=rows.device)
    for name, t, dtype, shape in (("out", out, torch.float32, (n,)), ("resid_out", resid_out, torch.float32, (n, 32)),
                                  ("counts", counts, torch.uint64, (OUTLIER_SLOTS,))):
        if t is None:
            continue
        if not t.is_cuda or t.device != rows.device or t.dtype != dtype or tuple(t.shape) != shape or \
                not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous CUDA {str(dtype).split('.')[-1]} tensor of shape "
                             f"{list(shape)} on the rows' device")
    s = stream if stream is not None else torch.cuda.current_stream(rows.device)
    _outlier_launch(dev_model, rows.data_ptr(), n, out.data_ptr(), resid_out.data_ptr() if resid_out is not None else None,
                    counts.data_ptr() if counts is not None else None, threshold, max_workgroups, s)
    return out


class OutlierMonitor:
    """A tumbling window of outlier counts of W64 rows on the GPU, built like ``DriftMonitor``.

    ``observe(rows)`` scores CUDA rows on the caller's current stream; ``observe_host(rows)`` copies
    a host ``uint8 [k,64]`` view into one of two pinned staging buffers and scores it from there on
    the monitor's own stream (the kernel reads the pinned memory directly), so the caller's memory
    is free again when it returns.  No score travels to the host: the kernel writes them to a
    device scratch buffer and only the counts come back, at ``report()`` time.  Thread-safe (one lock)."""

    def __init__(self, model, device: torch.device | str | int = "cuda", max_workgroups: Optional[int] = None):
        from ..engine.stream_engine import PinnedArray
        self.model = model
        self.dev_model = model if isinstance(model, DeviceOutlierModel) else DeviceOutlierModel(model, device)
        self.device = self.dev_model.device
        self.threshold = self.dev_model.threshold
        self.row_bytes = ROW_BYTES["w64"]
        self.max_workgroups = int(OUTLIER_MAX_WORKGROUPS if max_workgroups is None else max_workgroups)
        self.counts = new_outlier_counts(self.device)
        with torch.cuda.device(self.device):
            self._stream = torch.cuda.Stream(self.device)
            self._stage = [PinnedArray((DRIFT_STAGE_ROWS, self.row_bytes), np.uint8) for _ in range(2)]
            self._stage_ptr = [int(lib().ccfd_host_device_ptr(C.c_void_p(p.ptr))) for p in self._stage]
            self._scratch = torch.empty(DRIFT_STAGE_ROWS, dtype=torch.float32, device=self.device)   # own stream only
        self._busy: list = [None, None]          # event of the last launch that read each buffer
        self._next = 0
        self._streams = {}                       # streams observe() launched on since the last report
        self._lock = threading.Lock()
        torch.cuda.current_stream(self.device).synchronize()     # the zeroed counts, before any side-stream launch

    def observe(self, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Score CUDA rows on the current stream and count them; returns the scores."""
        with self._lock:
            s = torch.cuda.current_stream(self.device)
            out = outlier_scores(self.dev_model, rows, out, None, self.counts, None, self.max_workgroups, s)
            self._streams[s.cuda_stream] = s
        return out

    def observe_host(self, rows: np.ndarray) -> None:
        rows = np.asarray(rows)
        if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] != self.row_bytes:
            raise ValueError("rows must be a host uint8 [k,64] array of W64 rows")
        with self._lock, torch.cuda.device(self.device):     # torch's current device is per thread
            for lo in range(0, rows.shape[0], DRIFT_STAGE_ROWS):
                chunk = rows[lo:lo + DRIFT_STAGE_ROWS]
                b = self._next
                self._next ^= 1
                if self._busy[b] is not None:
                    self._busy[b].synchronize()          # the launch that read this buffer last
                k = chunk.shape[0]
                self._stage[b].array[:k] = chunk
                _outlier_launch(self.dev_model, self._stage_ptr[b], k, self._scratch.data_ptr(), None,
                                self.counts.data_ptr(), None, self.max_workgroups, self._stream)
                ev = torch.cuda.Event()
                ev.record(self._stream)
                self._busy[b] = ev

    def report(self, reset: bool = False):
        """``models.outlier.OutlierReport`` of the window so far; ``reset=True`` starts the next one."""
        from ..models.outlier import OutlierReport
        with self._lock:
            self._stream.synchronize()
            for s in self._streams.values():
                s.synchronize()
            self._streams.clear()
            with torch.cuda.device(self.device):
                counts = self.counts.view(torch.int64).cpu().numpy().view(np.uint64)
                if reset:
                    self.counts.view(torch.int64).zero_()
                    torch.cuda.current_stream(self.device).synchronize()
        return OutlierReport.from_counts(counts, self.threshold)

    def close(self) -> None:
        with self._lock:
            self._stream.synchronize()
            for p in self._stage:
                p.free()
            self._stage = []
