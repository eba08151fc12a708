"""Exact per-feature Shapley values of an oblivious GBDT (path-dependent TreeSHAP), in margin
(log-odds) space.  docs/EXPLAIN.md holds the definition; this module is its CPU oracle and
the packer of the 'GBX1' blob that csrc/kernels/explain_gbdt.hip reads.

For one tree, a row with leaf ``lx`` and a set ``S`` of features

    v(S) = sum_l leaves[l] * prod_{d<D} g_d(l)

with ``g_d(l) = [bit_d(l) == bit_d(lx)]`` when ``feat[d]`` is in ``S`` and otherwise the share
``cover(prefix of l through level d) / cover(prefix of l through level d-1)`` of the background
rows -- or, at a node no background row reaches, again ``[bit_d(l) == bit_d(lx)]`` (follow the
row).  ``phi_j`` is the Shapley value of feature ``j`` in the game ``v`` over the tree's distinct
features, summed over trees; ``base_value + sum_j phi_j == raw_score(x)``.

GBX1 blob (sections back to back, every one 8-byte aligned; padded to 16 B at the end):
  [0,64)   header 'GBX1', flags, T (i32), D (i32), base_value (f32), bin stamp (i32)
  weights  f64 [9][8]        w[m][s] = s! (m-s-1)! / m!  (0 where s >= m)
  meta     i32 [T][48]       feat[8], split bin k[8], level->slot[8], slot->feature[8],
                             slot->level mask[8], m, 7 x 0
  leaves   f32 [T][2^D]
  frac     f32 [T][2^(D+1)]  level d, prefix p (d+1 bits) at (2 << d) - 2 + p; -1 for both
                             children of a node without background rows, and for the 2
                             spare entries at the end (the kernel's "level fixed by S")
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from math import factorial
from typing import Optional, Tuple

import numpy as np

from ..contracts.transaction import N_FEATURES
from .common import HEADER_BYTES, header, pad16
from .gbdt import MAX_DEPTH, BinSpec, ObliviousGBDT

META_WORDS = 48
EMPTY = -1.0            # fraction of a child whose parent holds no background row


def _need_cover(model: ObliviousGBDT) -> np.ndarray:
    if getattr(model, "cover", None) is None:
        raise ValueError("the model has no cover (background leaf counts): call fit_cover(X) first")
    return model.cover.astype(np.float64)


def shapley_weights() -> np.ndarray:
    """w[m][s] = s! (m-s-1)! / m! for 0 <= s < m <= 8, float64 [9, 8]."""
    w = np.zeros((MAX_DEPTH + 1, MAX_DEPTH), np.float64)
    for m in range(1, MAX_DEPTH + 1):
        for s in range(m):
            w[m, s] = factorial(s) * factorial(m - s - 1) / factorial(m)
    return w


def tree_slots(feat_row: np.ndarray):
    """Distinct features of one tree in order of first use: (level -> slot, slot -> feature)."""
    slot_feat = []
    lvl_slot = []
    for f in feat_row:
        f = int(f)
        if f not in slot_feat:
            slot_feat.append(f)
        lvl_slot.append(slot_feat.index(f))
    return lvl_slot, slot_feat


def cover_fractions(cover_t: np.ndarray, depth: int) -> np.ndarray:
    """float64 [2^(D+1)]: share of its parent's background rows that each node holds (layout
    of the blob's ``frac`` section), ``EMPTY`` under a parent that holds none."""
    out = np.zeros(2 << depth, np.float64)
    leaf = np.arange(1 << depth)
    parent = np.array([cover_t.sum()])
    for d in range(depth):
        node = np.bincount(leaf & ((2 << d) - 1), weights=cover_t, minlength=2 << d)
        par = parent[np.arange(2 << d) & ((1 << d) - 1)]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[(2 << d) - 2:(4 << d) - 2] = np.where(par > 0, node / par, EMPTY)
        parent = node
    return out


def base_value(model: ObliviousGBDT) -> float:
    cover = _need_cover(model)
    tot = cover.sum(1)
    if not (tot > 0).all():
        raise ValueError("every tree needs at least one background row in its cover")
    return float(model.base) + float(((model.leaves.astype(np.float64) * cover).sum(1) / tot).sum())


def _leaf_indices(model: ObliviousGBDT, X: np.ndarray, bins: Optional[BinSpec]) -> np.ndarray:
    X = np.asarray(X)
    if X.dtype == np.uint8:
        spec = bins if bins is not None else model.bin_spec()
        if X.ndim != 2 or X.shape[1] != (32 if spec.bits == 8 else 20):
            raise ValueError(f"binned rows must be u8 [n,{32 if spec.bits == 8 else 20}]")
        return model.leaf_index_g32(X, spec)
    if X.ndim != 2 or X.shape[1] != N_FEATURES:
        raise ValueError("rows must be float32 [n,30] features or u8 G32 / G20 rows")
    return model.leaf_index(X)


def shapley_oblivious(model: ObliviousGBDT, X: np.ndarray, bins: Optional[BinSpec] = None,
                      dtype=np.float64) -> Tuple[np.ndarray, float]:
    """(phi [n,30], base_value) by enumeration of every feature subset of every tree, straight
    from the definition.  ``X``: float32 [n,30] features, or u8 G32 / G20 rows of ``bins`` (the
    model's own table by default).  ``dtype`` is the arithmetic of the value function and of
    the Shapley sum (the fractions are formed in float64 and rounded once, as in the blob)."""
    cover = _need_cover(model)
    bv = base_value(model)
    lx_all = _leaf_indices(model, X, bins)                   # [n, T]
    n, (T, D) = lx_all.shape[0], model.feat.shape
    L = np.arange(1 << D)
    w = shapley_weights().astype(dtype)
    phi = np.zeros((n, N_FEATURES), dtype)
    for t in range(T):
        lvl_slot, slot_feat = tree_slots(model.feat[t])
        m = len(slot_feat)
        frac = cover_fractions(cover[t], D)
        leaves = model.leaves[t].astype(dtype)
        lx = lx_all[:, t]
        follow, share = [], []
        for d in range(D):
            f = frac[(2 << d) - 2 + (L & ((2 << d) - 1))]                       # [2^D]
            same = (((L[None, :] ^ lx[:, None]) >> d) & 1) == 0                 # [n, 2^D]
            follow.append(same.astype(dtype))
            share.append(np.where(f[None, :] < 0, same, f[None, :]).astype(dtype))
        v = np.empty((1 << m, n), dtype)
        for S in range(1 << m):
            g = np.ones((n, 1 << D), dtype)
            for d in range(D):
                g = g * (follow[d] if (S >> lvl_slot[d]) & 1 else share[d])
            v[S] = (g * leaves[None, :]).sum(1, dtype=dtype)
        for j in range(m):
            acc = np.zeros(n, dtype)
            for S in range(1 << m):
                if (S >> j) & 1:
                    continue
                acc = acc + w[m, bin(S).count("1")] * (v[S | (1 << j)] - v[S])
            phi[:, slot_feat[j]] += acc
    return phi, bv


@dataclass
class ExplainTable:
    """The unpacked content of a GBX1 blob."""
    feat: np.ndarray         # i32 [T, D]
    k: np.ndarray            # i32 [T, D] split bins
    lvl_slot: np.ndarray     # i32 [T, D]
    slot_feat: np.ndarray    # i32 [T, 8] (first m valid)
    slot_mask: np.ndarray    # i32 [T, 8] levels of each slot as a bit mask
    m: np.ndarray            # i32 [T]
    leaves: np.ndarray       # f32 [T, 2^D]
    frac: np.ndarray         # f32 [T, 2^(D+1)]
    weights: np.ndarray      # f64 [9, 8]
    base_value: float
    stamp: int

    @staticmethod
    def offsets(T: int, D: int):
        off_w = HEADER_BYTES
        off_meta = off_w + 8 * (MAX_DEPTH + 1) * MAX_DEPTH
        off_leaf = off_meta + 4 * META_WORDS * T
        off_frac = off_leaf + 4 * (T << D)
        return off_w, off_meta, off_leaf, off_frac, off_frac + 4 * (T << (D + 1))

    @classmethod
    def pack(cls, model: ObliviousGBDT, bins: Optional[BinSpec] = None) -> bytes:
        cover = _need_cover(model)
        spec = bins if bins is not None else model.bin_spec()
        if spec.bits != 8:
            raise ValueError("the explain kernel reads G32 rows: pack against an 8-bit BinSpec")
        T, D = model.feat.shape
        k = spec.bin_index(model.feat, model.thr)
        meta = np.zeros((T, META_WORDS), np.int32)
        frac = np.zeros((T, 2 << D), np.float32)
        for t in range(T):
            lvl_slot, slot_feat = tree_slots(model.feat[t])
            meta[t, 0:D] = model.feat[t]
            meta[t, 8:8 + D] = k[t]
            meta[t, 16:16 + D] = lvl_slot
            meta[t, 24:24 + len(slot_feat)] = slot_feat
            for d, s in enumerate(lvl_slot):
                meta[t, 32 + s] |= 1 << d
            meta[t, 40] = len(slot_feat)
            frac[t] = cover_fractions(cover[t], D).astype(np.float32)
            frac[t, -2:] = EMPTY
        blob = header(b"GBX1", 0, T, D, float(np.float32(base_value(model))), int(spec.stamp))
        blob += shapley_weights().tobytes() + meta.tobytes() + model.leaves.tobytes() + frac.tobytes()
        assert len(blob) == cls.offsets(T, D)[-1]
        return pad16(blob)

    @classmethod
    def unpack(cls, blob: bytes) -> "ExplainTable":
        if blob[:4] != b"GBX1":
            raise ValueError("not a GBX1 blob")
        T, D = struct.unpack_from("<ii", blob, 8)
        bv, stamp = struct.unpack_from("<fi", blob, 16)
        ow, om, ol, of, end = cls.offsets(T, D)
        if len(blob) < end:
            raise ValueError("truncated GBX1 blob")
        meta = np.frombuffer(blob, np.int32, T * META_WORDS, om).reshape(T, META_WORDS)
        return cls(feat=meta[:, 0:D].copy(), k=meta[:, 8:8 + D].copy(), lvl_slot=meta[:, 16:16 + D].copy(),
                   slot_feat=meta[:, 24:32].copy(), slot_mask=meta[:, 32:40].copy(), m=meta[:, 40].copy(),
                   leaves=np.frombuffer(blob, np.float32, T << D, ol).reshape(T, 1 << D).copy(),
                   frac=np.frombuffer(blob, np.float32, T << (D + 1), of).reshape(T, 2 << D).copy(),
                   weights=np.frombuffer(blob, np.float64, (MAX_DEPTH + 1) * MAX_DEPTH, ow)
                   .reshape(MAX_DEPTH + 1, MAX_DEPTH).copy(),
                   base_value=float(bv), stamp=int(stamp))


def top_reasons(phi_row: np.ndarray, names, k: int = 3):
    """The ``k`` largest positive attributions of one row: [{"feature": name, "phi": float}]."""
    order = np.argsort(-np.asarray(phi_row, np.float64), kind="stable")[:max(0, int(k))]
    return [{"feature": names[int(j)], "phi": float(phi_row[j])} for j in order if phi_row[j] > 0]
