"""Autoencoder outlier detector 30 -> 64 -> L -> 64 -> 30 on W64 rows (``kind = "ae"``).

The third monitoring component a Seldon deployment puts beside a model, next to ``explain`` and
``drift``: the per-row reconstruction error of an autoencoder trained on legitimate traffic.  A
row the network cannot reconstruct "looks like nothing in the training data".  It is no fraud
scorer (``make_scorer`` refuses it); ``GpuScorer.set_outlier`` / ``OutlierMonitor`` run it beside one.

Two definitions, as ``MLPModel`` has ``logits`` and ``wire_logits``
-------------------------------------------------------------------
The model (fp32): ``residuals(X) = dec(enc(norm(X))) - norm(X)`` with ReLU after layers 1, 2, 3
and a linear layer 4; ``scores(X) = mean(r ** 2, axis=1)``.

What the kernel computes (csrc/kernels/outlier_ae.hip; oracle ``wire_residuals`` / ``wire_scores``),
all in W64 wire order (position p holds canonical feature WIRE_PERM[p]):

  x [32]   the MLP wire operand (``models.mlp.wire_operands``): raw bf16 V1..V28, bf16 of the
           normalised Time and Amount, constant 1 in K columns 30 / 31
  h1 = bf16(relu(W1p x))            W1p = ``models.mlp.wire_layer1``: V-normalisation folded into
                                    the columns, b1 as a bf16 hi/lo pair in columns 30 / 31
  z  = bf16(relu(b2 + W2 h1))       latent zero-padded to 32; weights bf16, biases fp32
  h3 = bf16(relu(b3 + W3 z))
  r  = b4 - T_hi x - T_lo x + W4 h3     fp32 accumulation in exactly this order: accumulator
                                    initialised with b4, then the T_hi, T_lo MFMAs, then the two
                                    K-steps of W4 (k order pi, below)

The target ``T x`` comes out of the matrix unit in the accumulator layout, so nothing is
transposed: for a V position p, ``t_p = x_p * isg_p - mu_p * isg_p`` with ``isg_p`` as a bf16
hi + lo pair (T_hi[p,p], T_lo[p,p]: within 2^-16 relative of the fp32 normalised value) and the
constant as a bf16 hi/lo pair in T_hi[p,30], T_hi[p,31] against the constant-1 inputs; for Time
and Amount T_hi[p,p] = 1, i.e. the target is the operand, the row as the model sees it.  Rows
30 / 31 of W4, b4 and T are zero: residual positions 30 and 31 are exactly 0.

Score: lane group g of the kernel owns positions 4g+j and 16+4g+j (j = 0..3).  Its partial is
``q_g = ((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7`` over the float32 squares
``s = r * r`` (no fused multiply-add) of positions 4g, 4g+1, 4g+2, 4g+3, 16+4g, .., 16+4g+3, and
``score = ((q_0 + q_1) + (q_2 + q_3)) * float32(1 / 30)`` (``combine_scores``).

Non-finite inputs: a row with any non-finite feature scores NaN and all 32 residual positions
are NaN (``0 * NaN`` in the target matrix carries it to every position of that row, and the
matrix unit keeps the columns, i.e. the rows of the batch, apart).  Time / Amount are checked
on the raw value, because the ``log1p(max(a, 0))`` clamp would otherwise hide a NaN or -inf Amount.

Deviation of ``wire_scores`` from ``scores`` (a property of this definition, not of the kernel),
measured on ``generate(20000, seed=7)`` rows with a He-init network and a fitted normaliser:
``wire_deviation`` gives a median relative deviation of 1.3e-4, 8e-4 at the 99th percentile and
5e-3 at most (latents 8 to 32, ``log_amount`` on and off).  The bf16 activations dominate; the
bf16 V columns of the W64 row itself are the same in both (``scores`` of the decoded rows).

Blob ``'AEW1'`` (``pack`` / ``unpack``), ``BLOB_BYTES`` = 21312, all 16-byte aligned; fragment
maps as in models/mlp.py: lane l holds A[l&15][8(l>>4)+j]; an accumulator pair (tiles 2s, 2s+1)
becomes K-step s of the next layer in k order ``pi(s,g,j) = 32s + 4g + (j&3) + 16(j>>2)``:
  [0,64)         header: 'AEW1', flags u32 (FLAG_LOG_AMOUNT | FLAG_WIRE), L i32, threshold f32
  [64,320)       mu[32], isg[32] f32, W64 order
  [320,4416)     W1f [4 t][64 l][8 j]        bf16  W1p[16t+(l&15)][8(l>>4)+j]
  [4416,8512)    W2f [2 u][2 s][64][8]       bf16  W2pad[16u+(l&15)][pi(s,l>>4,j)]
  [8512,12608)   W3f [4 t][64][8]            bf16  W3pad[16t+(l&15)][pi(0,l>>4,j)]
  [12608,16704)  W4f [2 u][2 s][64][8]       bf16  W4w[16u+(l&15)][pi(s,l>>4,j)]  (rows in wire order)
  [16704,18752)  THf [2 u][64][8]            bf16  -T_hi[16u+(l&15)][8(l>>4)+j]
  [18752,20800)  TLf [2 u][64][8]            bf16  -T_lo[...]
  [20800,20928)  b2q [2 u][4 g][4 r]  f32    b2pad[16u+4g+r]   (accumulator-init quads)
  [20928,21184)  b3q [4 t][4 g][4 r]  f32    b3[16t+4g+r]
  [21184,21312)  b4q [2 u][4 g][4 r]  f32    b4w[16u+4g+r]
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from ..contracts.transaction import (AMOUNT_COL, FEATURE_NAMES, N_FEATURES, TIME_COL, WIRE_PERM, WIRE_ROW_BYTES,
                                     decode_wire, encode_wire)
from .common import FLAG_WIRE, HEADER_BYTES, KPAD, Normalizer, bf16_bits, bf16_round, header
from .mlp import WIRE_N_BF16, _pi, wire_layer1, wire_operands

HID = 64
LPAD = 32                      # the latent is zero-padded to one K-step
MAGIC = b"AEW1"
OFF_NORM = HEADER_BYTES
OFF_W1 = OFF_NORM + 256
OFF_W2 = OFF_W1 + 4 * 64 * 16
OFF_W3 = OFF_W2 + 4 * 64 * 16
OFF_W4 = OFF_W3 + 4 * 64 * 16
OFF_TH = OFF_W4 + 4 * 64 * 16
OFF_TL = OFF_TH + 2 * 64 * 16
OFF_B2 = OFF_TL + 2 * 64 * 16
OFF_B3 = OFF_B2 + 2 * 64
OFF_B4 = OFF_B3 + 4 * 64
BLOB_BYTES = OFF_B4 + 2 * 64
assert BLOB_BYTES == 21312 and BLOB_BYTES % 16 == 0

# counts uint64 [OUTLIER_SLOTS] of the kernel (ccfd_abi.h CCFD_OUT_*)
SLOT_ROWS, SLOT_FLAGGED, SLOT_INVALID, SLOT_HIST, SLOT_TOP, OUTLIER_SLOTS = 0, 1, 2, 4, 36, 66
N_CELLS = 32
INV30 = np.float32(1.0 / 30.0)
ACC_C = 2.0                    # residual_bounds: any faithfully rounded fp32 add in any order


def score_cell(score) -> np.ndarray:
    """Histogram cell 0..31 of a float32 score from its exponent bits:
    ``clamp(((bits >> 23) & 255) - 111, 0, 31)``: cell 0 is everything below 2^-15, cell k holds
    [2^(k-16), 2^(k-15)), cell 31 everything from 2^15 up.  Integer work on the bits, so host and
    device agree by construction."""
    b = np.ascontiguousarray(score, np.float32).view(np.uint32).astype(np.int64)
    return np.clip(((b >> 23) & 255) - 111, 0, 31).astype(np.int64).reshape(np.shape(score))


def combine_scores(resid: np.ndarray) -> np.ndarray:
    """float32 ``[n]`` scores of float32 wire-order residuals ``[n,32]`` in the kernel's
    summation order (module docstring).  Bit-exact against the kernel on its own ``resid_out``."""
    r = np.ascontiguousarray(resid, np.float32).reshape(-1, KPAD)
    with np.errstate(over="ignore", invalid="ignore"):
        s = r * r
        q = []
        for g in range(4):
            pos = [4 * g + j for j in range(4)] + [16 + 4 * g + j for j in range(4)]
            acc = s[:, pos[0]]
            for p in pos[1:]:
                acc = (acc + s[:, p]).astype(np.float32)
            q.append(acc)
        return (((q[0] + q[1]).astype(np.float32) + (q[2] + q[3]).astype(np.float32)).astype(np.float32)
                * INV30).astype(np.float32)


def top_positions(resid: np.ndarray) -> np.ndarray:
    """Wire position 0..29 of the largest squared float32 residual of each row, lowest position
    on a tie (the kernel's rule for an outlier row's ``top_feature`` cell)."""
    r = np.ascontiguousarray(resid, np.float32).reshape(-1, KPAD)[:, :N_FEATURES]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.argmax(r * r, axis=1)


def recount(score: np.ndarray, resid: np.ndarray, threshold: float) -> np.ndarray:
    """The kernel's ``counts uint64 [OUTLIER_SLOTS]`` recomputed on the host from float32 scores
    and wire-order residuals: rows, flagged (``score > threshold``; NaN is not), invalid
    (non-finite score), the 32 ``score_cell`` cells of finite scores, and for every flagged row
    the canonical feature of its ``top_positions``."""
    score = np.ascontiguousarray(score, np.float32).reshape(-1)
    c = np.zeros(OUTLIER_SLOTS, np.uint64)
    fin = np.isfinite(score)
    with np.errstate(invalid="ignore"):
        flagged = score > np.float32(threshold)
    c[SLOT_ROWS] = score.size
    c[SLOT_FLAGGED] = int(flagged.sum())
    c[SLOT_INVALID] = int((~fin).sum())
    c[SLOT_HIST:SLOT_HIST + N_CELLS] = np.bincount(score_cell(score[fin]), minlength=N_CELLS).astype(np.uint64)
    top = WIRE_PERM[top_positions(resid)[flagged]]
    c[SLOT_TOP:SLOT_TOP + N_FEATURES] = np.bincount(top, minlength=N_FEATURES).astype(np.uint64)
    return c


@dataclass
class OutlierReport:
    """One window of ``OutlierMonitor`` counts."""
    rows: int
    outliers: int
    invalid: int
    histogram: np.ndarray                 # int64 [32]: score_cell of the finite scores
    top_feature: np.ndarray               # int64 [30], canonical order: outlier rows by worst feature
    threshold: float = float("nan")
    names: Tuple[str, ...] = FEATURE_NAMES

    def __post_init__(self):
        self.rows, self.outliers, self.invalid = int(self.rows), int(self.outliers), int(self.invalid)
        self.histogram = np.asarray(self.histogram, np.int64).reshape(N_CELLS)
        self.top_feature = np.asarray(self.top_feature, np.int64).reshape(N_FEATURES)

    @classmethod
    def from_counts(cls, counts: np.ndarray, threshold: float = float("nan")) -> "OutlierReport":
        c = np.asarray(counts, np.uint64).reshape(OUTLIER_SLOTS).astype(np.int64)
        return cls(c[SLOT_ROWS], c[SLOT_FLAGGED], c[SLOT_INVALID], c[SLOT_HIST:SLOT_HIST + N_CELLS],
                   c[SLOT_TOP:SLOT_TOP + N_FEATURES], float(threshold))

    @property
    def outlier_rate(self) -> float:
        """Outliers over the rows with a finite score (0 when there are none)."""
        valid = self.rows - self.invalid
        return self.outliers / valid if valid > 0 else 0.0

    def worst(self, k: int = 3) -> List[Tuple[str, int]]:
        order = np.argsort(-self.top_feature, kind="stable")[:k]
        return [(self.names[j], int(self.top_feature[j])) for j in order.tolist() if self.top_feature[j] > 0]

    def to_json(self, k: int = 3) -> dict:
        thr = self.threshold
        return {"rows": self.rows, "outliers": self.outliers, "invalid": self.invalid,
                "outlier_rate": self.outlier_rate, "threshold": None if thr != thr else thr,
                "histogram": [int(v) for v in self.histogram.tolist()],
                "cell_upper_bounds": [float(2.0 ** (k_ - 15)) for k_ in range(N_CELLS - 1)] + [None],
                "names": list(self.names), "top_feature": [int(v) for v in self.top_feature.tolist()],
                "worst": [{"name": n, "rows": v} for n, v in self.worst(k)]}


def _rows_w64(rows) -> np.ndarray:
    rows = np.ascontiguousarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] != WIRE_ROW_BYTES:
        raise ValueError("rows must be W64 rows (uint8 [n,64])")
    return rows


def _bf16_ulp(a: np.ndarray) -> np.ndarray:
    """Spacing of bf16 at |a| (float64), 0 at 0."""
    a = np.abs(np.asarray(a, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, np.exp2(np.maximum(e, -126.0) - 7.0), 0.0)


def _round_margin(a: np.ndarray) -> np.ndarray:
    """Distance of a pre-rounding activation (float64) from where ``bf16(relu(.))`` changes its
    value: the ReLU kink for a <= 0, else the nearer of the kink and the RNE midpoint of the two
    bf16 neighbours."""
    a = np.asarray(a, np.float64)
    pos = np.maximum(a, 0.0)
    ulp = _bf16_ulp(pos)
    lo = np.where(ulp > 0, np.floor(pos / np.where(ulp > 0, ulp, 1.0)) * ulp, 0.0)
    return np.where(a > 0, np.minimum(np.abs(pos - (lo + 0.5 * ulp)), a), -a)


@dataclass
class OutlierAE:
    W1: np.ndarray   # [64, 30]
    b1: np.ndarray   # [64]
    W2: np.ndarray   # [L, 64]
    b2: np.ndarray   # [L]
    W3: np.ndarray   # [64, L]
    b3: np.ndarray   # [64]
    W4: np.ndarray   # [30, 64]
    b4: np.ndarray   # [30]
    norm: Normalizer = field(default_factory=Normalizer.identity)
    threshold: float = float("inf")
    kind: str = "ae"

    def __post_init__(self):
        f = lambda a: np.ascontiguousarray(a, np.float32)
        self.W1, self.b1, self.W2, self.b2 = f(self.W1), f(self.b1), f(self.W2), f(self.b2)
        self.W3, self.b3, self.W4, self.b4 = f(self.W3), f(self.b3), f(self.W4), f(self.b4)
        L = self.W2.shape[0]
        if not 1 <= L <= LPAD:
            raise ValueError(f"latent width must be 1..{LPAD}, not {L}")
        shapes = ((self.W1, (HID, N_FEATURES)), (self.b1, (HID,)), (self.W2, (L, HID)), (self.b2, (L,)),
                  (self.W3, (HID, L)), (self.b3, (HID,)), (self.W4, (N_FEATURES, HID)), (self.b4, (N_FEATURES,)))
        for a, s in shapes:
            if a.shape != s:
                raise ValueError(f"autoencoder parameter of shape {a.shape}, expected {s}")
        self.threshold = float(self.threshold)

    @property
    def latent(self) -> int:
        return self.W2.shape[0]

    @property
    def n_params(self) -> int:
        return sum(a.size for a in (self.W1, self.b1, self.W2, self.b2, self.W3, self.b3, self.W4, self.b4))

    @classmethod
    def random_init(cls, latent: int = 8, seed: int = 0, norm: Optional[Normalizer] = None) -> "OutlierAE":
        """He-uniform init, as ``MLPModel.random_init``."""
        rng = np.random.default_rng(seed)

        def lin(fan_out, fan_in):
            bound = 1.0 / np.sqrt(fan_in)
            return (rng.uniform(-bound, bound, (fan_out, fan_in)).astype(np.float32),
                    rng.uniform(-bound, bound, fan_out).astype(np.float32))
        W1, b1 = lin(HID, N_FEATURES)
        W2, b2 = lin(latent, HID)
        W3, b3 = lin(HID, latent)
        W4, b4 = lin(N_FEATURES, HID)
        return cls(W1, b1, W2, b2, W3, b3, W4, b4, norm or Normalizer.identity())

    # ---------------------------------------------------------------- the model (fp32)
    def residuals(self, X: np.ndarray) -> np.ndarray:
        """``dec(enc(norm(X))) - norm(X)``: float32 [n,30], canonical order."""
        Xn = self.norm(np.asarray(X, np.float32)).astype(np.float64)
        h = np.maximum(Xn @ self.W1.T.astype(np.float64) + self.b1, 0.0)
        h = np.maximum(h @ self.W2.T.astype(np.float64) + self.b2, 0.0)
        h = np.maximum(h @ self.W3.T.astype(np.float64) + self.b3, 0.0)
        return (h @ self.W4.T.astype(np.float64) + self.b4 - Xn).astype(np.float32)

    def scores(self, X: np.ndarray) -> np.ndarray:
        r = self.residuals(X).astype(np.float64)
        return (r * r).mean(axis=1).astype(np.float32)

    # ---------------------------------------------------------------- what the kernel computes
    def _wire_mats(self):
        """bf16-rounded float64 matrices of the wire path, wire order, padded:
        ``(W1p [64,32], W2 [32,64], b2 [32], W3 [64,32], b3 [64], W4 [32,64], b4 [32], T_hi [32,32], T_lo [32,32])``."""
        L = self.latent
        W1p = bf16_round(wire_layer1(self.W1, self.b1, self.norm)).astype(np.float64)
        W2 = np.zeros((LPAD, HID)); W2[:L] = bf16_round(self.W2)
        b2 = np.zeros(LPAD); b2[:L] = self.b2
        W3 = np.zeros((HID, LPAD)); W3[:, :L] = bf16_round(self.W3)
        W4 = np.zeros((KPAD, HID)); W4[:N_FEATURES] = bf16_round(self.W4[WIRE_PERM])
        b4 = np.zeros(KPAD); b4[:N_FEATURES] = self.b4[WIRE_PERM]
        mu = self.norm.mu[WIRE_PERM].astype(np.float64)
        isg = self.norm.inv_sigma[WIRE_PERM].astype(np.float64)
        Th, Tl = np.zeros((KPAD, KPAD)), np.zeros((KPAD, KPAD))
        v = np.arange(WIRE_N_BF16)
        hi = bf16_round(isg[v].astype(np.float32)).astype(np.float64)
        Th[v, v] = hi
        Tl[v, v] = bf16_round((isg[v] - hi).astype(np.float32))
        c = -mu[v] * isg[v]
        chi = bf16_round(c.astype(np.float32)).astype(np.float64)
        Th[v, N_FEATURES] = chi
        Th[v, N_FEATURES + 1] = bf16_round((c - chi).astype(np.float32))
        Th[WIRE_N_BF16, WIRE_N_BF16] = 1.0
        Th[WIRE_N_BF16 + 1, WIRE_N_BF16 + 1] = 1.0
        return W1p, W2, b2, W3, self.b3.astype(np.float64), W4, b4, Th, Tl

    def wire_inputs(self, rows_w64) -> Tuple[np.ndarray, np.ndarray]:
        """``(x float32 [n,32], finite bool [n])``: the kernel's layer-1 operand of W64 rows
        (``models.mlp.wire_operands``, zero for a row with a non-finite feature) and which rows
        are finite."""
        Xd = decode_wire(_rows_w64(rows_w64))
        finite = np.isfinite(Xd).all(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            x = wire_operands(self.norm, np.where(finite[:, None], Xd, np.float32(0)))
        x[~finite] = 0
        return x, finite

    def _wire_forward(self, rows_w64):
        """Pre-rounding activations (float64) and rounded ones of the wire path."""
        x32, finite = self.wire_inputs(rows_w64)
        W1p, W2, b2, W3, b3, W4, b4, Th, Tl = self._wire_mats()
        x = x32.astype(np.float64)
        r = lambda a: bf16_round(np.maximum(a, 0.0).astype(np.float32)).astype(np.float64)
        a1 = x @ W1p.T
        h1 = r(a1)
        a2 = h1 @ W2.T + b2
        z = r(a2)
        a3 = z @ W3.T + b3
        h3 = r(a3)
        res = b4 - x @ Th.T - x @ Tl.T + h3 @ W4.T
        return dict(x=x, finite=finite, a1=a1, h1=h1, a2=a2, z=z, a3=a3, h3=h3, res=res)

    def wire_residuals(self, rows_w64) -> np.ndarray:
        """Numerics oracle of the kernel's ``resid_out``: float32 [n,32], wire order (bf16 operands
        and activations, fp64 accumulation rounded once to fp32; module docstring)."""
        f = self._wire_forward(rows_w64)
        res = f["res"].astype(np.float32)
        res[~f["finite"]] = np.nan
        return res

    def wire_scores(self, rows_w64) -> np.ndarray:
        return combine_scores(self.wire_residuals(rows_w64))

    def wire_sq_err(self, rows_w64) -> Tuple[np.ndarray, np.ndarray]:
        """``(scores [n], squared residuals [n,30] in canonical order)`` of the wire oracle."""
        res = self.wire_residuals(rows_w64)
        sq = np.empty((res.shape[0], N_FEATURES), np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            sq[:, WIRE_PERM] = res[:, :N_FEATURES] * res[:, :N_FEATURES]
        return combine_scores(res), sq

    def fit_threshold(self, X: np.ndarray, quantile: float = 0.999) -> float:
        """Set ``threshold`` to that quantile of ``wire_scores`` of the finite rows of float32 ``X [n,30]``."""
        if not 0.0 < quantile <= 1.0:
            raise ValueError("quantile must be in (0, 1]")
        s = self.wire_scores(encode_wire(np.asarray(X, np.float32)))
        s = s[np.isfinite(s)]
        if s.size == 0:
            raise ValueError("no finite rows to fit the outlier threshold on")
        self.threshold = float(np.float32(np.quantile(s.astype(np.float64), quantile)))
        return self.threshold

    # ---------------------------------------------------------------- bounds for the GPU tests
    def _operand_slack(self, rows_w64) -> np.ndarray:
        """float64 [n,2]: bound on |kernel pre-rounding Time / Amount operand - ours|.  The kernel
        forms ``fma(t, isg, -mu*isg)`` and ``fma(log2(1 + clamp(a)), isg*ln2, -mu*isg)`` with the
        hardware log2 (1 ulp); ``wire_operands`` forms ``(t - mu) * isg`` with ``log1p``.  Each side
        is a few float32 roundings of terms no larger than |t*isg| + |mu*isg|: 8 * 2^-24 of that sum
        covers the roundings of both (two in ours, the product and the constant and the fma in the
        kernel's, one more for 1 + a and two ulp for the log)."""
        Xd = decode_wire(_rows_w64(rows_w64)).astype(np.float64)
        Xd = np.where(np.isfinite(Xd), Xd, 0.0)
        mu, isg = self.norm.mu.astype(np.float64), self.norm.inv_sigma.astype(np.float64)
        t = Xd[:, TIME_COL]
        a = Xd[:, AMOUNT_COL]
        if self.norm.log_amount:
            a = np.log1p(np.maximum(a, 0.0)) + 1.0      # + 1: the absolute error of log(1 + a) from rounding 1 + a
        u = 8.0 * 2.0 ** -24
        return np.stack([u * (np.abs(t * isg[TIME_COL]) + np.abs(mu[TIME_COL] * isg[TIME_COL])),
                         u * (np.abs(a * isg[AMOUNT_COL]) + np.abs(mu[AMOUNT_COL] * isg[AMOUNT_COL]))], axis=1)

    def _acc_terms(self, f):
        """Per-layer fp32 accumulation terms ``c (K + 2) 2^-24 sum |w| |h|`` (bias included)."""
        W1p, W2, b2, W3, b3, W4, b4, Th, Tl = self._wire_mats()
        u = ACC_C * 2.0 ** -24
        ax = np.abs(f["x"])
        e1 = u * (KPAD + 2) * (ax @ np.abs(W1p).T)
        e2 = u * (HID + 2) * (f["h1"] @ np.abs(W2).T + np.abs(b2))
        e3 = u * (LPAD + 2) * (f["z"] @ np.abs(W3).T + np.abs(b3))
        e4 = u * (HID + 2 * KPAD + 2) * (f["h3"] @ np.abs(W4).T + ax @ (np.abs(Th) + np.abs(Tl)).T + np.abs(b4))
        return e1, e2, e3, e4

    def residual_bounds(self, rows_w64, stable: bool = False) -> np.ndarray:
        """float64 [n,32]: first-order worst case of |kernel residual - ``wire_residuals``|.

        Every row: the computed Time / Amount operands may land one bf16 ulp away, every rounded
        activation too (``|bf16(a') - bf16(a)| <= |a' - a| + 2^-7 (|a| + |a' - a|)``), propagated
        through ``|W|``, plus the accumulation term ``c (K + 2) 2^-24 sum|w||h|`` of every dot
        product (``ACC_C = 2``: any faithfully rounded fp32 add in any order) and the oracle's own
        final float32 rounding.  ``stable=True``: the bound for ``stable_rows``, where the kernel
        has the oracle's activations: the last layer's accumulation term alone."""
        f = self._wire_forward(rows_w64)
        W1p, W2, b2, W3, b3, W4, b4, Th, Tl = self._wire_mats()
        e1, e2, e3, e4 = self._acc_terms(f)
        own = 2.0 ** -24 * np.abs(f["res"])
        if stable:
            return e4 + own
        rel = 2.0 ** -7
        dx = np.zeros_like(f["x"])
        slack = self._operand_slack(rows_w64)
        for k in range(2):
            xk = np.abs(f["x"][:, WIRE_N_BF16 + k])
            dx[:, WIRE_N_BF16 + k] = slack[:, k] + rel * (xk + slack[:, k]) + 2.0 ** -133
        d1 = dx @ np.abs(W1p).T + e1
        dh1 = d1 + rel * (f["h1"] + d1)
        d2 = dh1 @ np.abs(W2).T + e2
        dz = d2 + rel * (f["z"] + d2)
        d3 = dz @ np.abs(W3).T + e3
        dh3 = d3 + rel * (f["h3"] + d3)
        return dh3 @ np.abs(W4).T + dx @ (np.abs(Th) + np.abs(Tl)).T + e4 + own

    def score_bounds(self, rows_w64) -> np.ndarray:
        """float64 [n]: bound on |kernel score - ``wire_scores``| from ``residual_bounds``
        (``2|r| d + d^2`` a position, and 40 float32 roundings of the sum)."""
        f = self._wire_forward(rows_w64)
        d = self.residual_bounds(rows_w64)
        r = np.abs(f["res"])
        s = (r * r).sum(axis=1) / 30.0
        return (2.0 * r * d + d * d).sum(axis=1) / 30.0 + 40.0 * 2.0 ** -24 * s

    def stable_rows(self, rows_w64) -> np.ndarray:
        """bool [n]: finite rows where no pre-rounding activation of layers 1-3 lies within its own
        accumulation term of a bf16 rounding boundary or of the ReLU kink, and neither computed
        operand (Time, Amount) lies within ``_operand_slack`` of a bf16 rounding boundary: there a
        kernel that adds in fp32 within ``ACC_C`` roundings has exactly the oracle's activations.
        An activation whose accumulation term is 0 (zero padding) is exact on both sides."""
        rows_w64 = _rows_w64(rows_w64)
        f = self._wire_forward(rows_w64)
        e1, e2, e3, _ = self._acc_terms(f)
        ok = f["finite"].copy()
        for a, e in ((f["a1"], e1), (f["a2"], e2), (f["a3"], e3)):
            ok &= ((_round_margin(a) > e) | (e == 0)).all(axis=1)
        # the operands before their bf16 rounding, as wire_operands forms them
        Xd = decode_wire(rows_w64)
        Xd = np.where(np.isfinite(Xd), Xd, np.float32(0))
        t = Xd[:, TIME_COL].astype(np.float32)
        a = Xd[:, AMOUNT_COL].astype(np.float32)
        if self.norm.log_amount:
            a = np.log1p(np.maximum(a, 0.0)).astype(np.float32)
        mu, isg = self.norm.mu, self.norm.inv_sigma
        pre = np.stack([(t - mu[TIME_COL]) * isg[TIME_COL], (a - mu[AMOUNT_COL]) * isg[AMOUNT_COL]], axis=1)
        pre = np.abs(pre.astype(np.float64))
        ulp = _bf16_ulp(pre)
        lo = np.where(ulp > 0, np.floor(pre / np.where(ulp > 0, ulp, 1.0)) * ulp, 0.0)
        margin = np.abs(pre - (lo + 0.5 * ulp))
        slack = self._operand_slack(rows_w64)
        ok &= ((margin > slack) | (pre == 0)).all(axis=1)
        return ok

    # ---------------------------------------------------------------- packing
    def pack(self) -> bytes:
        """The ``'AEW1'`` blob (module docstring)."""
        W1p, W2, b2, W3, b3, W4, b4, Th, Tl = self._wire_mats()
        lanes = np.arange(64)
        c, g = lanes & 15, lanes >> 4
        j = np.arange(8)
        knat = 8 * g[:, None] + j[None, :]                                                    # [64][8]
        kpi = np.array([[[_pi(s, gg, jj) for jj in range(8)] for gg in g] for s in range(2)])   # [2 s][64][8]

        def nat(M, tiles):          # [t][l][j] = M[16t + (l&15)][8(l>>4)+j]
            return M[(16 * np.arange(tiles)[:, None, None] + c[None, :, None]), knat[None, :, :]]

        def perm(M, tiles, steps):  # [u][s][l][j] = M[16u + (l&15)][pi(s, l>>4, j)]
            rows = 16 * np.arange(tiles)[:, None, None, None] + c[None, None, :, None]
            return M[rows, kpi[None, :steps, :, :]]

        gi, ri = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
        quads = lambda b, tiles: np.stack([b[16 * t + 4 * gi + ri] for t in range(tiles)]).astype(np.float32)
        blob = (header(MAGIC, self.norm.flags | FLAG_WIRE, int(self.latent), float(self.threshold))
                + self.norm.packed(True)
                + bf16_bits(nat(W1p, 4)).tobytes() + bf16_bits(perm(W2, 2, 2)).tobytes()
                + bf16_bits(perm(W3, 4, 1)).tobytes() + bf16_bits(perm(W4, 2, 2)).tobytes()
                + bf16_bits(nat(-Th, 2)).tobytes() + bf16_bits(nat(-Tl, 2)).tobytes()
                + quads(b2, 2).tobytes() + quads(b3, 4).tobytes() + quads(b4, 2).tobytes())
        assert len(blob) == BLOB_BYTES, len(blob)
        return blob

    # ---------------------------------------------------------------- state io
    def state_dict(self) -> dict:
        st = {"ae.W1": self.W1, "ae.b1": self.b1, "ae.W2": self.W2, "ae.b2": self.b2, "ae.W3": self.W3,
              "ae.b3": self.b3, "ae.W4": self.W4, "ae.b4": self.b4,
              "ae.threshold": np.array([self.threshold], np.float32)}
        st.update(self.norm.state())
        return st

    @classmethod
    def from_state_dict(cls, st: dict) -> "OutlierAE":
        g = lambda k: np.asarray(st[k], np.float32)
        return cls(g("ae.W1"), g("ae.b1"), g("ae.W2"), g("ae.b2"), g("ae.W3"), g("ae.b3"), g("ae.W4"), g("ae.b4"),
                   Normalizer.from_state(st), float(g("ae.threshold").reshape(-1)[0]))


@dataclass
class PackedAE:
    """What ``unpack`` reads back from a blob: the header, the normaliser (wire order) and the
    matrices the fragments hold (bf16-exact float32, wire order, padded; T as stored: negated)."""
    latent: int
    threshold: float
    flags: int
    mu: np.ndarray
    isg: np.ndarray
    W1p: np.ndarray
    W2: np.ndarray
    W3: np.ndarray
    W4: np.ndarray
    nTh: np.ndarray
    nTl: np.ndarray
    b2: np.ndarray
    b3: np.ndarray
    b4: np.ndarray


def _fragments(blob: bytes):
    b = memoryview(blob)
    if len(blob) != BLOB_BYTES or bytes(b[:4]) != MAGIC:
        raise ValueError("not an 'AEW1' outlier blob")
    flags, L = struct.unpack_from("<Ii", b, 4)
    thr = struct.unpack_from("<f", b, 12)[0]
    if not 1 <= L <= LPAD or not flags & FLAG_WIRE:
        raise ValueError("'AEW1' blob with a bad latent width or without the wire flag")

    def bf(off, shape):
        n = int(np.prod(shape))
        return (np.frombuffer(b, np.uint16, n, off).astype(np.uint32) << 16).view(np.float32).reshape(shape)
    fr = dict(W1f=bf(OFF_W1, (4, 64, 8)), W2f=bf(OFF_W2, (2, 2, 64, 8)), W3f=bf(OFF_W3, (4, 64, 8)),
              W4f=bf(OFF_W4, (2, 2, 64, 8)), THf=bf(OFF_TH, (2, 64, 8)), TLf=bf(OFF_TL, (2, 64, 8)),
              b2q=np.frombuffer(b, np.float32, 32, OFF_B2).reshape(2, 4, 4),
              b3q=np.frombuffer(b, np.float32, 64, OFF_B3).reshape(4, 4, 4),
              b4q=np.frombuffer(b, np.float32, 32, OFF_B4).reshape(2, 4, 4),
              mu=np.frombuffer(b, np.float32, 32, OFF_NORM), isg=np.frombuffer(b, np.float32, 32, OFF_NORM + 128))
    return flags, L, thr, fr


def unpack(blob: bytes) -> PackedAE:
    """Invert ``OutlierAE.pack``: undo the fragment maps and the ``pi`` permutation."""
    flags, L, thr, fr = _fragments(blob)
    lanes = np.arange(64)
    c, g = lanes & 15, lanes >> 4

    def un_nat(F, tiles):
        M = np.zeros((16 * tiles, KPAD), np.float32)
        for t in range(tiles):
            for l in range(64):
                M[16 * t + c[l], 8 * g[l]: 8 * g[l] + 8] = F[t, l]
        return M

    def un_perm(F, tiles, steps):
        M = np.zeros((16 * tiles, 32 * steps), np.float32)
        F = F.reshape(tiles, steps, 64, 8)
        for u in range(tiles):
            for s in range(steps):
                for l in range(64):
                    for jj in range(8):
                        M[16 * u + c[l], _pi(s, g[l], jj)] = F[u, s, l, jj]
        return M
    unq = lambda q: np.concatenate([q[t].reshape(-1) for t in range(q.shape[0])])      # [t][g][r] -> 16t+4g+r
    return PackedAE(L, thr, flags, fr["mu"].copy(), fr["isg"].copy(), un_nat(fr["W1f"], 4), un_perm(fr["W2f"], 2, 2),
                    un_perm(fr["W3f"], 4, 1), un_perm(fr["W4f"], 2, 2), un_nat(fr["THf"], 2), un_nat(fr["TLf"], 2),
                    unq(fr["b2q"]), unq(fr["b3q"]), unq(fr["b4q"]))


def emulate_packed_kernel(blob: bytes, rows_w64) -> Tuple[np.ndarray, np.ndarray]:
    """Lane-by-lane NumPy emulation of outlier_ae.hip on the packed blob: ``(score [n],
    resid [n,32])``.  It walks the kernel's fragment maps per 16-row tile -- operand chunk of lane
    (c, g), accumulator pairs re-used as the next B operand, bias quads, the lane's 8 squares and
    the two cross-group adds -- so a packing or permutation bug shows without a GPU."""
    flags, L, thr, fr = _fragments(blob)
    rows_w64 = _rows_w64(rows_w64)
    n = rows_w64.shape[0]
    norm = Normalizer(np.zeros(N_FEATURES, np.float32), np.ones(N_FEATURES, np.float32), bool(flags & 1))
    norm.mu[WIRE_PERM] = fr["mu"][:N_FEATURES]
    norm.inv_sigma[WIRE_PERM] = fr["isg"][:N_FEATURES]
    Xd = decode_wire(rows_w64)
    finite = np.isfinite(Xd).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        xop = wire_operands(norm, np.where(finite[:, None], Xd, np.float32(0)))
    lanes = np.arange(64)
    c, g = lanes & 15, lanes >> 4
    kk = 8 * g[:, None] + np.arange(8)[None, :]
    rr = 4 * g[:, None] + np.arange(4)[None, :]

    def mfma(A, B, C):
        Am = np.zeros((16, 32)); Bm = np.zeros((32, 16))
        Am[c[:, None], kk] = A
        Bm[kk, c[:, None]] = B
        return C.astype(np.float64) + (Am @ Bm)[rr, c[:, None]]

    def pair(a0, a1):           # bf16(relu) of an accumulator pair as the next B fragment
        return bf16_round(np.maximum(np.concatenate([a0, a1], axis=1), 0.0).astype(np.float32))
    score = np.empty(n, np.float32)
    resid = np.empty((n, KPAD), np.float32)
    zero = np.zeros((64, 4))
    for t0 in range(0, n, 16):
        row = t0 + c
        valid = row < n
        xb = np.zeros((64, 8), np.float32)
        xb[valid] = xop[row[valid][:, None], kk[valid]]
        nanrow = np.zeros(64, bool)
        nanrow[valid] = ~finite[row[valid]]
        a1 = [mfma(fr["W1f"][t], xb, zero) for t in range(4)]
        h1 = [pair(a1[0], a1[1]), pair(a1[2], a1[3])]
        a2 = []
        for u in range(2):
            acc = fr["b2q"][u][g]
            for s in range(2):
                acc = mfma(fr["W2f"][u, s], h1[s], acc)
            a2.append(acc)
        z = pair(a2[0], a2[1])
        a3 = [mfma(fr["W3f"][t], z, fr["b3q"][t][g]) for t in range(4)]
        h3 = [pair(a3[0], a3[1]), pair(a3[2], a3[3])]
        res = []
        for u in range(2):
            acc = fr["b4q"][u][g]
            acc = mfma(fr["THf"][u], xb, acc)
            acc = mfma(fr["TLf"][u], xb, acc)
            for s in range(2):
                acc = mfma(fr["W4f"][u, s], h3[s], acc)
            acc = acc.astype(np.float32)
            acc[nanrow] = np.nan
            res.append(acc)
        with np.errstate(over="ignore", invalid="ignore"):
            sq = np.concatenate([res[0] * res[0], res[1] * res[1]], axis=1)
            q = sq[:, 0]
            for k in range(1, 8):
                q = (q + sq[:, k]).astype(np.float32)
            q = (q + q[lanes ^ 16]).astype(np.float32)
            q = (q + q[lanes ^ 32]).astype(np.float32)
            sc = (q * INV30).astype(np.float32)
        for l in range(64):
            if valid[l]:
                score[row[l]] = sc[l]
                for u in range(2):
                    resid[row[l], 16 * u + 4 * g[l]: 16 * u + 4 * g[l] + 4] = res[u][l]
    return score, resid


def wire_deviation(model: OutlierAE, X: np.ndarray) -> dict:
    """Deviation of ``wire_scores`` from ``scores`` on float32 rows ``X`` (``scores`` of the decoded
    W64 rows, so the row format itself is not counted): median and maximum relative deviation."""
    rows = encode_wire(np.asarray(X, np.float32))
    a = model.scores(decode_wire(rows)).astype(np.float64)
    b = model.wire_scores(rows).astype(np.float64)
    rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-30)
    return {"rows": int(rows.shape[0]), "median_rel": float(np.median(rel)), "max_rel": float(rel.max()),
            "p99_rel": float(np.quantile(rel, 0.99))}
