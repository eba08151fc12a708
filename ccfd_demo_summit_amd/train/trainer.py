"""Model training (replaces the JupyterHub/Spark workbench of the reference,
deploy/frauddetection_cr.yaml:7-53).

* ``train_logistic`` / ``train_mlp``: PyTorch-ROCm training on the GPU (bf16 autocast for
  the MLP, class-imbalance weighting), optionally data-parallel with DDP over RCCL when
  launched under torchrun.  The result is exported into the same ``LogisticModel`` /
  ``MLPModel`` containers the HIP kernels consume, so a trained model is packed and
  hot-swapped exactly like a random-init one.
* ``train_oblivious_gbdt``: gradient-boosted oblivious trees (logloss, second-order
  leaves, quantile-binned splits) with histograms built by ``scatter_add`` on the GPU, or
  (``hist="hip"``) by the HIP histogram kernel over G32 rows (csrc/kernels/train_hist.hip).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ..models.common import Normalizer
from ..models.gbdt import ObliviousGBDT
from ..models.lr import LogisticModel
from ..models.mlp import H1, H2, MLPModel


@dataclass
class TrainConfig:
    epochs: int = 3
    batch: int = 8192
    lr: float = 3e-3
    weight_decay: float = 1e-4
    pos_weight: Optional[float] = None     # default: sqrt(neg/pos)
    seed: int = 0
    device: str = "auto"
    bf16: bool = True
    metrics: Optional[object] = None       # metrics.exporter.TrainMetrics (Training dashboard)
    graph: bool = True                     # single GPU: replay the whole step as one HIP graph
    log_every: int = 50                    # graph mode: loss read back every N steps


def _device(name: str) -> torch.device:
    if name == "auto":
        return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(name)


def _ddp_ctx():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _fit(net: nn.Module, Xn: np.ndarray, y: np.ndarray, cfg: TrainConfig, use_bf16: bool) -> Dict[str, float]:
    dev = _device(cfg.device)
    torch.manual_seed(cfg.seed)
    rank, world = _ddp_ctx()
    net = net.to(dev)
    model = net
    if world > 1:
        from torch.nn.parallel import DistributedDataParallel as DDP
        model = DDP(net, device_ids=[dev.index] if dev.type == "cuda" else None)
    Xt = torch.from_numpy(np.ascontiguousarray(Xn)).to(dev)
    yt = torch.from_numpy(y.astype(np.float32)).to(dev)
    pos = float(y.sum())
    pw = cfg.pos_weight if cfg.pos_weight is not None else math.sqrt(max(1.0, (len(y) - pos) / max(pos, 1.0)))
    loss_fn = nn.BCEWithLogitsLoss(pos_weight=torch.tensor(pw, device=dev))
    opt = torch.optim.AdamW(model.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    g = torch.Generator(device="cpu").manual_seed(cfg.seed)
    n = Xt.shape[0]
    shard = torch.arange(rank, n, world)
    steps = 0
    last = float("nan")
    tm = cfg.metrics
    name = "mlp" if isinstance(net, nn.Sequential) else "lr"
    if tm is not None:
        tm.workers.set(world)
    import time as _time
    t_start = _time.perf_counter()
    if cfg.graph and dev.type == "cuda" and world == 1 and len(shard) >= cfg.batch:
        return _fit_graph(model, Xt, yt, loss_fn, opt, shard, g, cfg, use_bf16, pw, name, tm, t_start)
    for _ in range(cfg.epochs):
        perm = shard[torch.randperm(len(shard), generator=g)].to(dev)
        for s in range(0, len(perm), cfg.batch):
            idx = perm[s:s + cfg.batch]
            with torch.autocast(device_type=dev.type, dtype=torch.bfloat16, enabled=use_bf16 and dev.type == "cuda"):
                logit = model(Xt[idx]).squeeze(-1)
            loss = loss_fn(logit.float(), yt[idx])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            steps += 1
            last = float(loss.detach())
            if tm is not None:
                tm.loss.labels(name).set(last)
                tm.steps.labels(name).inc()
                tm.samples_per_s.labels(name).set(steps * cfg.batch / max(1e-9, _time.perf_counter() - t_start))
                if dev.type == "cuda":
                    tm.mem_bytes.set(torch.cuda.memory_allocated(dev))
    return {"steps": steps, "final_loss": last, "pos_weight": pw}


def _fit_graph(model, Xt, yt, loss_fn, opt, shard, g, cfg: TrainConfig, use_bf16: bool, pw: float, name: str,
               tm, t_start) -> Dict[str, float]:
    """The training step (gather -> forward -> BCE -> backward -> AdamW) captured once as a
    HIP graph (``torch.cuda.CUDAGraph`` is hipGraph on ROCm) and replayed per step.  A
    12K-parameter MLP step is ~40 tiny kernels, i.e. launch-bound; a replay is one launch,
    plus one index copy into the static batch-index buffer.  Batches are full ``cfg.batch``
    rows (the tail of an epoch that does not fill one is skipped), the optimizer state lives
    in capturable tensors, and the loss is read back only every ``cfg.log_every`` steps."""
    import time as _time
    dev = Xt.device
    B = cfg.batch
    for group in opt.param_groups:         # optimizer step must run inside the graph
        group["capturable"] = True
    idx = torch.zeros(B, dtype=torch.int64, device=dev)
    xb = torch.empty(B, Xt.shape[1], dtype=Xt.dtype, device=dev)
    yb = torch.empty(B, dtype=yt.dtype, device=dev)

    def step():
        torch.index_select(Xt, 0, idx, out=xb)
        torch.index_select(yt, 0, idx, out=yb)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=use_bf16, cache_enabled=False):
            logit = model(xb).squeeze(-1)
        loss = loss_fn(logit.float(), yb)
        loss.backward()
        opt.step()
        return loss

    batches = []
    for _ in range(cfg.epochs):
        perm = shard[torch.randperm(len(shard), generator=g)].to(dev)
        batches += [perm[s:s + B] for s in range(0, len(perm) - B + 1, B)]
    # warm-up (real steps on the first batches) on a side stream, as capture requires
    warm = min(3, len(batches))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for k in range(warm):
            idx.copy_(batches[k])
            opt.zero_grad(set_to_none=False)
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=False)        # grads stay allocated: the graph accumulates into them
    with torch.cuda.graph(graph):
        for p in model.parameters():
            p.grad.zero_()
        static_loss = step()
    last = float("nan")
    steps = logged = warm
    for k in range(warm, len(batches)):
        idx.copy_(batches[k], non_blocking=True)
        graph.replay()
        steps += 1
        if tm is not None and (steps % cfg.log_every == 0 or k == len(batches) - 1):
            last = float(static_loss.detach())
            tm.loss.labels(name).set(last)
            tm.steps.labels(name).inc(steps - logged)
            logged = steps
            tm.samples_per_s.labels(name).set(steps * B / max(1e-9, _time.perf_counter() - t_start))
            tm.mem_bytes.set(torch.cuda.memory_allocated(dev))
    torch.cuda.synchronize(dev)
    last = float(static_loss.detach()) if len(batches) > warm else last
    return {"steps": steps, "final_loss": last, "pos_weight": pw, "graph": True,
            "seconds": _time.perf_counter() - t_start}


def train_logistic(X: np.ndarray, y: np.ndarray, cfg: TrainConfig = TrainConfig()) -> Tuple[LogisticModel, Dict]:
    norm = Normalizer.fit(X)
    net = nn.Linear(X.shape[1], 1)
    with torch.no_grad():                 # convex problem: deterministic zero start
        net.weight.zero_()
        net.bias.zero_()
    info = _fit(net, norm(X), y, cfg, use_bf16=False)
    w = net.weight.detach().float().cpu().numpy()[0]
    b = float(net.bias.detach().float().cpu().numpy()[0])
    return LogisticModel(w.astype(np.float32), b, norm), info


def train_mlp(X: np.ndarray, y: np.ndarray, cfg: TrainConfig = TrainConfig()) -> Tuple[MLPModel, Dict]:
    norm = Normalizer.fit(X)
    torch.manual_seed(cfg.seed)           # reproducible init
    net = nn.Sequential(nn.Linear(X.shape[1], H1), nn.ReLU(), nn.Linear(H1, H2), nn.ReLU(), nn.Linear(H2, 1))
    info = _fit(net, norm(X), y, cfg, use_bf16=cfg.bf16)
    p = [t.detach().float().cpu().numpy() for t in net.parameters()]
    m = MLPModel(p[0], p[1], p[2], p[3], p[4][0], float(p[5][0]), norm)
    return m, info


def train_autoencoder(X: np.ndarray, y: np.ndarray, cfg: TrainConfig = TrainConfig(), latent: int = 8,
                      holdout: float = 0.1):
    """The outlier autoencoder 30 -> 64 -> latent -> 64 -> 30 (models/outlier.py): MSE on the
    normalised features of the legitimate (``y == 0``) rows, AdamW, same device / DDP plumbing as
    ``train_mlp``.  The last ``holdout`` share of the rows (both classes) is kept out of training;
    the metrics carry the ROC-AUC of the fp32 score against ``y`` there (NaN when it holds one
    class only).  Returns ``(OutlierAE, metrics)``; the threshold is left to ``fit_threshold``."""
    from ..models.outlier import HID, OutlierAE
    X = np.asarray(X, np.float32)
    y = np.asarray(y)
    n_hold = int(len(X) * holdout)
    Xtr, ytr = (X[:-n_hold], y[:-n_hold]) if n_hold else (X, y)
    norm = Normalizer.fit(Xtr[ytr == 0])
    dev = _device(cfg.device)
    torch.manual_seed(cfg.seed)           # reproducible init
    rank, world = _ddp_ctx()
    net = nn.Sequential(nn.Linear(X.shape[1], HID), nn.ReLU(), nn.Linear(HID, latent), nn.ReLU(),
                        nn.Linear(latent, HID), nn.ReLU(), nn.Linear(HID, X.shape[1])).to(dev)
    model = net
    if world > 1:
        from torch.nn.parallel import DistributedDataParallel as DDP
        model = DDP(net, device_ids=[dev.index] if dev.type == "cuda" else None)
    Xt = torch.from_numpy(np.ascontiguousarray(norm(Xtr[ytr == 0]))).to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=cfg.lr, weight_decay=cfg.weight_decay)
    g = torch.Generator(device="cpu").manual_seed(cfg.seed)
    shard = torch.arange(rank, Xt.shape[0], world)
    steps, last = 0, float("nan")
    for _ in range(cfg.epochs):
        perm = shard[torch.randperm(len(shard), generator=g)].to(dev)
        for s in range(0, len(perm), cfg.batch):
            xb = Xt[perm[s:s + cfg.batch]]
            loss = nn.functional.mse_loss(model(xb), xb)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            steps += 1
        last = float(loss.detach()) if steps else last
        if cfg.metrics is not None and steps:
            cfg.metrics.loss.labels("ae").set(last)
    p = [t.detach().float().cpu().numpy() for t in net.parameters()]
    m = OutlierAE(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], norm)
    info = {"steps": steps, "final_loss": last, "latent": int(latent), "rows": int(Xt.shape[0]), "holdout_roc_auc": float("nan")}
    if n_hold and 0 < int(y[-n_hold:].sum()) < n_hold:
        from sklearn.metrics import roc_auc_score
        info["holdout_roc_auc"] = float(roc_auc_score(y[-n_hold:], m.scores(X[-n_hold:])))
    return m, info


# ---------------------------------------------------------------------------- GBDT
def _quantile_borders(X: np.ndarray, n_bins: int) -> np.ndarray:
    qs = np.linspace(0, 1, n_bins + 1)[1:-1]
    return np.quantile(X, qs, axis=0).T.astype(np.float32)        # [F, n_bins-1]


HIP_HIST_MAX_BINS = 64      # csrc/include/ccfd_abi.h CCFD_GBDT_HIST_MAX_BINS
HIP_HIST_MAX_DEPTH = 8      # CCFD_GBDT_MAX_SPLITS (the last histogram level is depth - 1 <= 7)
HIST_BACKENDS = ("torch", "hip", "auto")


def _hip_hist_refusal(dev: torch.device, n_bins: int, depth: int, n_features: int) -> Optional[str]:
    """Why the HIP histogram path cannot train this shape (None: it can)."""
    if n_bins > HIP_HIST_MAX_BINS:
        return f"n_bins = {n_bins} exceeds its limit of {HIP_HIST_MAX_BINS} bins per feature"
    if n_bins < 2:
        return f"n_bins = {n_bins}: it needs at least 2 bins per feature"
    if not 1 <= depth <= HIP_HIST_MAX_DEPTH:
        return f"depth = {depth} is outside its range 1..{HIP_HIST_MAX_DEPTH}"
    if n_features != 30:
        return f"{n_features} features: G32 rows hold exactly 30"
    if dev.type != "cuda":
        return f"device {str(dev)!r}: it needs a CUDA device"
    return None


def _encode_training_rows(X: np.ndarray, borders: np.ndarray, counts: Optional[np.ndarray] = None) -> np.ndarray:
    """X [n, 30] f32 -> G32 rows [n, 32] u8 against ``borders`` [30, B-1] as a bin table
    (native encoder, csrc/engine/ingest.cpp): byte j = #borders_j < x_j, the trainer's
    ``searchsorted(..., "left")``, except that NaN goes to bin 0.  ``counts`` [30]: only the
    first ``counts[j]`` borders of feature j are edges (a ragged table, ``bin_spec=``)."""
    import os
    from ..ops._lib import lib
    X = np.ascontiguousarray(X, np.float32)
    n, F = X.shape
    if counts is None:
        flat = np.ascontiguousarray(borders, np.float32).reshape(-1)
        offsets = (np.arange(F + 1, dtype=np.int32) * np.int32(borders.shape[1])).astype(np.int32)
    else:
        flat = np.concatenate([borders[f, :counts[f]] for f in range(F)] + [np.zeros(1, np.float32)]).astype(np.float32)
        offsets = np.zeros(F + 1, np.int32)
        np.cumsum(counts, out=offsets[1:])
    rows = np.empty((n, 32), np.uint8)
    threads = max(1, min(16, os.cpu_count() or 1, (n + 65535) // 65536))
    if lib().ccfd_encode_bins_mt(X.ctypes.data, n, F, flat.ctypes.data, offsets.ctypes.data, 1, 0,
                                 rows.ctypes.data, None, threads) != n:
        raise RuntimeError("ccfd_encode_bins_mt failed")
    return rows


def _boost_hip(rows: torch.Tensor, yt: torch.Tensor, raw: torch.Tensor, borders: np.ndarray, feat: np.ndarray,
               thr: np.ndarray, leaves: np.ndarray, l2: float, learning_rate: float, allreduce,
               padded: Optional[torch.Tensor] = None) -> None:
    """The boosting loop of ``train_oblivious_gbdt(hist="hip")``: fills feat / thr / leaves and
    advances ``raw`` in place.  Per level one histogram launch over the G32 ``rows``, then the
    all-reduce and the gain scan of the torch path; per tree one update launch.  ``padded``
    [F, B-1] bool: candidates that are padding of a ragged border matrix (never chosen)."""
    from ..ops.kernels import gbdt_apply_tree, gbdt_histogram
    n_trees, depth = feat.shape
    B = borders.shape[1] + 1
    prob = torch.sigmoid(raw)
    grad = prob - yt
    hess = (prob * (1 - prob)).clamp_min(1e-6)
    for t in range(n_trees):
        splits = []
        for d in range(depth):
            G, H = gbdt_histogram(rows, grad, hess, B, splits)         # [2^d, F, B], overwritten
            G, H = allreduce(G), allreduce(H)
            Gl = G.cumsum(-1)[..., :-1]                                # split after bin b: left = bins <= b
            Hl = H.cumsum(-1)[..., :-1]
            Gt = G.sum(-1, keepdim=True)
            Ht = H.sum(-1, keepdim=True)
            Gr, Hr = Gt - Gl, Ht - Hl
            gain = (Gl ** 2 / (Hl + l2) + Gr ** 2 / (Hr + l2) - Gt ** 2 / (Ht + l2)).sum(0)   # [F, B-1]
            if padded is not None:
                gain = gain.masked_fill(padded, float("-inf"))
            best = int(torch.argmax(gain))
            f, b = divmod(best, B - 1)
            feat[t, d] = f
            thr[t, d] = borders[f, b]
            splits.append((f, b))
        # the last split sends leaf l's rows left (stay l) or right (l + 2^(depth-1)): its partial
        # sums ARE the 2^depth leaf totals, already all-reduced
        Gs = torch.cat([G[:, f, :b + 1].sum(-1), G[:, f, b + 1:].sum(-1)])
        Hs = torch.cat([H[:, f, :b + 1].sum(-1), H[:, f, b + 1:].sum(-1)])
        vals = (-learning_rate * Gs / (Hs + l2)).contiguous()
        leaves[t] = vals.cpu().numpy()
        gbdt_apply_tree(rows, raw, vals, splits, y=yt, grad=grad, hess=hess)


def _leaf_counts(X: np.ndarray, feat: np.ndarray, thr: np.ndarray, dev) -> torch.Tensor:
    """``ObliviousGBDT.fit_cover`` on the training device: rows of X per (tree, leaf), float64
    [T, 2^D] (a sum the ranks all-reduce)."""
    T, D = feat.shape
    ft = torch.from_numpy(feat.astype(np.int64)).to(dev)
    tt = torch.from_numpy(np.ascontiguousarray(thr, np.float32)).to(dev)
    shift = torch.arange(D, device=dev)
    tree_off = torch.arange(T, device=dev) << D
    count = torch.zeros(T << D, dtype=torch.float64, device=dev)
    step = max(1, (1 << 22) // (T * D))                               # ~4 M compares at a time
    for s in range(0, X.shape[0], step):
        Xc = torch.from_numpy(np.ascontiguousarray(X[s:s + step], np.float32)).to(dev)
        idx = ((Xc[:, ft] > tt).long() << shift).sum(-1) + tree_off    # [rows, T]
        count += torch.bincount(idx.reshape(-1), minlength=T << D)
    return count.view(T, 1 << D)


def train_oblivious_gbdt(X: np.ndarray, y: np.ndarray, n_trees: int = 100, depth: int = 6,
                         learning_rate: float = 0.1, n_bins: int = 32, l2: float = 1.0,
                         device: str = "auto", borders: Optional[np.ndarray] = None,
                         hist: str = "torch", bin_spec=None) -> Tuple[ObliviousGBDT, Dict]:
    """Level-wise oblivious boosting on logloss.  At each level one (feature, border) is
    chosen for ALL current leaves (maximum summed second-order gain).

    Data-parallel when torch.distributed is initialised (the reference's 2-executor Spark
    training, deploy/frauddetection_cr.yaml:27,34-35): like the DDP trainers every rank
    passes the same X and works on its shard (rows rank::world); the borders come from
    rank 0 (broadcast), and the per-level gradient/hessian histograms,
    the leaf sums and the base-rate statistics are all-reduced (SUM), so every rank grows
    the same trees -- the ones a single process would grow on the union of the shards, up to
    float summation order.  ``borders`` [F, n_bins-1]: use these split candidates instead of
    quantiles of X.  ``bin_spec`` (a ``models.gbdt.BinSpec``, e.g. the table the live partition
    logs were encoded with): the split candidates of feature f are exactly ``bin_spec.edges[f]``,
    so ``bin_spec.contains(model.bin_spec())`` holds and ``DeviceModel(model, bins=bin_spec)``
    always packs -- a challenger for live G32 / G20 logs is trained without re-encoding them.
    The table may be ragged (``B = max_f len(edges_f) + 1`` bins; the border matrix is padded
    with ``+inf`` and a padded candidate is never chosen); ``ValueError`` if it is given together
    with ``borders`` or if no feature has an edge.

    ``hist`` picks how the histograms are built; ``info["hist"]`` reports the path used.

    * ``"torch"`` (default): an int64 bin matrix and two ``scatter_add_`` per level.
    * ``"hip"``: X is encoded once into G32 rows (32 B a row, the borders as the bin table),
      each level is one launch of the LDS-privatised histogram kernel
      (``ops.kernels.gbdt_histogram``, csrc/kernels/train_hist.hip), the leaf sums are read off
      the last level's histogram, and one update launch per tree (``ops.kernels.gbdt_apply_tree``)
      advances the raw scores and writes the next gradients / hessians.  No per-row leaf array
      and no int64 matrix exist on the device.  The all-reduce of G / H and the gain scan are
      the torch path's.  It needs a CUDA device, ``n_bins <= 64`` and ``depth <= 8``; otherwise
      ``ValueError`` names the limit.
    * ``"auto"``: ``"hip"`` when those conditions hold, else ``"torch"``.

    Both paths sum in f32 in no fixed order (float atomics), so histograms -- and with them a
    near-tied split choice -- can differ in the last bits between the paths and from run to
    run.  They bin identically except for NaN: the G32 encoder sends NaN to bin 0, which is
    how the scorers treat it (``x > thr`` is false), while the torch path's ``searchsorted``
    sends it to the last bin."""
    if hist not in HIST_BACKENDS:
        raise ValueError(f"hist must be one of {HIST_BACKENDS}, got {hist!r}")
    dev = _device(device)
    rank, world = _ddp_ctx()

    def allreduce(t: torch.Tensor) -> torch.Tensor:
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(t)
        return t

    X = np.asarray(X, np.float32)
    counts = None
    if bin_spec is not None:
        if borders is not None:
            raise ValueError("bin_spec= and borders= both name the split candidates: give one of them")
        counts = np.array([e.size for e in bin_spec.edges], np.int32)
        if len(counts) != X.shape[1]:
            raise ValueError(f"bin_spec has {len(counts)} features, X has {X.shape[1]}")
        if counts.max(initial=0) == 0:
            raise ValueError("bin_spec has no edge on any feature: there is no split candidate")
        borders = np.full((len(counts), int(counts.max())), np.inf, np.float32)
        for f, e in enumerate(bin_spec.edges):
            borders[f, :e.size] = e
    use_hip = False
    if hist != "torch":
        why = _hip_hist_refusal(dev, n_bins if borders is None else np.shape(borders)[1] + 1, depth, X.shape[1])
        if why is not None and hist == "hip":
            raise ValueError(f"hist='hip': {why}")
        use_hip = why is None
    if borders is None:
        borders = _quantile_borders(X, n_bins)                      # [F, B-1]
    if world > 1:
        X, y = X[rank::world], np.asarray(y)[rank::world]
    n, F = X.shape
    borders = np.ascontiguousarray(borders, np.float32)
    n_bins = borders.shape[1] + 1
    if world > 1:                                                   # rank 0's split candidates
        import torch.distributed as dist
        bt0 = torch.from_numpy(borders).to(dev)
        dist.broadcast(bt0, 0)
        borders = bt0.cpu().numpy()
    # bin index of every value: number of borders strictly below it -> x > border[b] iff bin > b
    if use_hip:
        rows = torch.from_numpy(_encode_training_rows(X, borders, counts)).to(dev)      # [n, 32] u8
    else:
        bins = np.empty((n, F), np.int64)
        for f in range(F):                                          # a ragged table: the real edges only
            bins[:, f] = np.searchsorted(borders[f] if counts is None else borders[f, :counts[f]], X[:, f], side="left")
        bt = torch.from_numpy(bins).to(dev)
    # padding of a ragged border matrix: gain -inf before the argmax
    padded = None if counts is None else \
        (torch.arange(n_bins - 1, device=dev)[None, :] >= torch.from_numpy(counts).to(dev)[:, None])
    yt = torch.from_numpy(y.astype(np.float32)).to(dev)
    stats = allreduce(torch.tensor([float(y.sum()), float(n)], dtype=torch.float64, device=dev))
    p0 = float(np.clip(float(stats[0]) / max(float(stats[1]), 1.0), 1e-6, 1 - 1e-6))
    base = math.log(p0 / (1 - p0))
    raw = torch.full((n,), base, device=dev)
    feat = np.zeros((n_trees, depth), np.int32)
    thr = np.zeros((n_trees, depth), np.float32)
    leaves = np.zeros((n_trees, 1 << depth), np.float32)
    B = n_bins
    fidx = torch.arange(F, device=dev)
    import time as _time
    t_boost = _time.perf_counter()
    if use_hip:
        _boost_hip(rows, yt, raw, borders, feat, thr, leaves, l2, learning_rate, allreduce, padded)
    for t in range(0 if use_hip else n_trees):                         # hist="torch"
        prob = torch.sigmoid(raw)
        grad = prob - yt
        hess = (prob * (1 - prob)).clamp_min(1e-6)
        leaf = torch.zeros(n, dtype=torch.long, device=dev)
        for d in range(depth):
            L = 1 << d
            key = (leaf[:, None] * F + fidx[None, :]) * B + bt          # [n, F]
            G = torch.zeros(L * F * B, device=dev).scatter_add_(0, key.reshape(-1), grad[:, None].expand(n, F).reshape(-1))
            H = torch.zeros(L * F * B, device=dev).scatter_add_(0, key.reshape(-1), hess[:, None].expand(n, F).reshape(-1))
            G = allreduce(G).view(L, F, B)
            H = allreduce(H).view(L, F, B)
            Gl = G.cumsum(-1)[..., :-1]                                # split after bin b: left = bins <= b
            Hl = H.cumsum(-1)[..., :-1]
            Gt = G.sum(-1, keepdim=True)
            Ht = H.sum(-1, keepdim=True)
            Gr, Hr = Gt - Gl, Ht - Hl
            gain = (Gl ** 2 / (Hl + l2) + Gr ** 2 / (Hr + l2) - Gt ** 2 / (Ht + l2)).sum(0)   # [F, B-1]
            if padded is not None:
                gain = gain.masked_fill(padded, float("-inf"))
            best = int(torch.argmax(gain))
            f, b = divmod(best, B - 1)
            feat[t, d] = f
            thr[t, d] = borders[f, b]
            leaf = leaf | ((bt[:, f] > b).long() << d)
        Gs = allreduce(torch.zeros(1 << depth, device=dev).scatter_add_(0, leaf, grad))
        Hs = allreduce(torch.zeros(1 << depth, device=dev).scatter_add_(0, leaf, hess))
        vals = -learning_rate * Gs / (Hs + l2)
        leaves[t] = vals.cpu().numpy()
        raw = raw + vals[leaf]
    model = ObliviousGBDT(feat, thr, leaves, float(base))
    # background of the Shapley attributions (models/explain.py): the training rows per leaf,
    # summed over the ranks' shards
    model.cover = allreduce(_leaf_counts(X, feat, thr, dev)).cpu().numpy().astype(np.float32)
    with torch.no_grad():
        ll_sum = torch.nn.functional.binary_cross_entropy_with_logits(raw, yt, reduction="sum").double()
        ll = float(allreduce(ll_sum.reshape(1))[0]) / max(float(stats[1]), 1.0)
    return model, {"train_logloss": ll, "trees": n_trees, "depth": depth, "world": world,
                   "hist": "hip" if use_hip else "torch",
                   "seconds_boost": _time.perf_counter() - t_boost}       # the tree loop, binning excluded


def evaluate(model, X: np.ndarray, y: np.ndarray) -> Dict[str, float]:
    from sklearn.metrics import average_precision_score, roc_auc_score
    p = model.predict_proba(X)
    return {"roc_auc": float(roc_auc_score(y, p)), "pr_auc": float(average_precision_score(y, p))}
