"""Sampled Shapley values of the MLP (and the closed form for LR) against one baseline row, in
logit (log-odds) space, on W64 rows.  docs/EXPLAIN.md holds the definition; this module is its
CPU oracle and the packer of the 'MLX1' table that csrc/kernels/explain_mlp.hip reads.

A *position* is a wire position 0..29 of a W64 row (``contracts.transaction.WIRE_PERM``):
0..27 the bf16 V-columns, 28 Time (f32 word 14), 29 Amount (f32 word 15).  The value function
``v(S)`` is the MLP's wire logit of the row that carries ``x``'s bits on the positions in ``S``
and the baseline's bits elsewhere.  With ``P`` permutations of the positions, in antithetic
pairs (permutation ``2i+1`` is permutation ``2i`` reversed),

    phi_j = (1/P) sum_p [ v(S_pj + {j}) - v(S_pj) ],   S_pj = the positions before j in p.

Every permutation's sum telescopes to ``v(all) - v(none)``, so ``base_value + sum_j phi_j`` is
the row's logit for every ``P``; a position whose bits equal the baseline's never changes a
coalition row and gets exactly 0; a row that differs in two positions gets its exact Shapley
values (a pair holds both orders once).

MLX1 table (``MlpExplainTable.pack``), ``128 + 160 P`` bytes:
  [0,64)     header 'MLX1', P (i32), seed (u64), flags (u32; bit 0: antithetic pairs)
  [64,128)   the baseline as one W64 row
  masks      u32 [P][32]   bit i of masks[p][s]: position i is among the first s of permutation p
                           (slot 0 is the empty set, slots 30 and 31 are both the full set)
  inv        u8  [P][32]   inv[p][j] = place of position j in permutation p (30 for j = 30, 31)
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from math import factorial
from typing import Optional, Sequence, Tuple

import numpy as np

from ..contracts.transaction import N_FEATURES, WIRE_PERM, WIRE_ROW_BYTES, decode_wire, encode_wire
from .common import HEADER_BYTES

MAX_PERMS = 256            # ccfd_abi.h CCFD_MLX_MAX_PERMS
SLOTS = 32                 # coalition rows a permutation: two 16-row MFMA tiles
MAGIC = b"MLX1"
FLAG_ANTITHETIC = 1
EXACT_MAX_POSITIONS = 12

# the uint16 fields of a W64 row that make up each position
_FIELDS = [(i,) for i in range(28)] + [(28, 29), (30, 31)]


def _need_baseline(model) -> np.ndarray:
    b = getattr(model, "baseline", None)
    if b is None:
        raise ValueError(f"the {getattr(model, 'kind', None)!r} model has no baseline (the row its Shapley values "
                         "start from): call fit_baseline(X) first")
    b = np.asarray(b, np.float32)
    if b.shape != (N_FEATURES,):
        raise ValueError("baseline must be float32 [30]")
    return b


def _check_perms(P: int, limit: Optional[int] = None) -> int:
    P = int(P)
    if P < 2 or P % 2:
        raise ValueError(f"P must be even and >= 2 (antithetic pairs), not {P}")
    if limit is not None and P > limit:
        raise ValueError(f"P must be <= {limit} for a packed table, not {P}")
    return P


def permutation_table(P: int, seed: int = 0) -> np.ndarray:
    """uint8 [P, 30]: ``P / 2`` permutations of the 30 positions drawn from
    ``numpy.random.Generator(PCG64(seed))``, each followed by its reverse."""
    P = _check_perms(P)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    out = np.empty((P, N_FEATURES), np.uint8)
    for i in range(P // 2):
        out[2 * i] = rng.permutation(N_FEATURES)
        out[2 * i + 1] = out[2 * i, ::-1]
    return out


def mlp_base_value(model) -> float:
    """``v(none)``: the wire logit of the baseline row."""
    return float(model.wire_logits(_need_baseline(model)[None, :])[0])


@dataclass
class MlpExplainTable:
    """The unpacked content of an MLX1 table."""
    perms: np.ndarray        # u8 [P, 30]
    masks: np.ndarray        # u32 [P, 32]
    inv: np.ndarray          # u8 [P, 32]
    baseline_w64: np.ndarray  # u8 [64]
    seed: int
    flags: int = FLAG_ANTITHETIC

    @property
    def P(self) -> int:
        return int(self.masks.shape[0])

    @staticmethod
    def nbytes(P: int) -> int:
        return 2 * HEADER_BYTES + (4 + 1) * SLOTS * int(P)

    @classmethod
    def build(cls, model, P: int = 64, seed: int = 0) -> "MlpExplainTable":
        """The table of ``permutation_table(P, seed)`` (any even ``P``; only ``pack`` is limited)."""
        base = encode_wire(_need_baseline(model)[None, :])[0]
        perms = permutation_table(P, seed)
        return cls(perms, *cls._masks_inv(perms), baseline_w64=base, seed=int(seed))

    @staticmethod
    def _masks_inv(perms: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        P = perms.shape[0]
        bits = np.uint32(1) << perms.astype(np.uint32)                       # [P, 30]
        masks = np.zeros((P, SLOTS), np.uint32)
        masks[:, 1:N_FEATURES + 1] = np.bitwise_or.accumulate(bits, axis=1)
        masks[:, N_FEATURES + 1:] = masks[:, N_FEATURES:N_FEATURES + 1]
        inv = np.full((P, SLOTS), N_FEATURES, np.uint8)
        inv[np.arange(P)[:, None], perms] = np.arange(N_FEATURES, dtype=np.uint8)[None, :]
        return masks, inv

    def to_bytes(self) -> bytes:
        head = MAGIC + struct.pack("<iQI", self.P, self.seed, self.flags)
        blob = head + b"\0" * (HEADER_BYTES - len(head)) + self.baseline_w64.tobytes() + \
            self.masks.astype("<u4").tobytes() + self.inv.tobytes()
        assert len(blob) == self.nbytes(self.P) and len(blob) % 16 == 0
        return blob

    @classmethod
    def pack(cls, model, P: int = 64, seed: int = 0) -> bytes:
        _check_perms(P, MAX_PERMS)
        return cls.build(model, P, seed).to_bytes()

    @classmethod
    def unpack(cls, blob: bytes) -> "MlpExplainTable":
        if len(blob) < 2 * HEADER_BYTES or blob[:4] != MAGIC:
            raise ValueError("not an MLX1 table")
        P, seed, flags = struct.unpack_from("<iQI", blob, 4)
        if P < 2 or P % 2 or len(blob) != cls.nbytes(P):
            raise ValueError("damaged MLX1 table: P and the length disagree")
        masks = np.frombuffer(blob, "<u4", P * SLOTS, 2 * HEADER_BYTES).reshape(P, SLOTS).astype(np.uint32)
        inv = np.frombuffer(blob, np.uint8, P * SLOTS, 2 * HEADER_BYTES + 4 * SLOTS * P).reshape(P, SLOTS).copy()
        perms = np.argsort(inv[:, :N_FEATURES], axis=1, kind="stable").astype(np.uint8)
        base = np.frombuffer(blob, np.uint8, WIRE_ROW_BYTES, HEADER_BYTES).copy()
        return cls(perms, masks, inv, base, int(seed), int(flags))


_POS_OF_FIELD = np.array([i for i, fs in enumerate(_FIELDS) for _ in fs], np.uint32)      # u16 field -> position


def _masked_rows(r16: np.ndarray, b16: np.ndarray, masks: np.ndarray) -> np.ndarray:
    """uint16 [..., 32]: the fields of position i from ``r16`` where bit i of ``masks`` is set,
    else from ``b16`` (``r16`` broadcasts against ``masks[..., None]``)."""
    take = ((masks[..., None] >> _POS_OF_FIELD) & 1).astype(bool)
    return np.where(take, r16, b16).astype(np.uint16)


def coalition_rows(table: MlpExplainTable, rows_w64: np.ndarray) -> np.ndarray:
    """uint8 [n, P, 32, 64]: every slot's masked W64 row, built by the mask words: the fields of
    position i come from the row where bit i of ``masks[p][s]`` is set, else from the baseline."""
    rows = np.ascontiguousarray(rows_w64, np.uint8).reshape(-1, WIRE_ROW_BYTES)
    b16 = np.ascontiguousarray(table.baseline_w64).view(np.uint16)
    out = _masked_rows(rows.view(np.uint16)[:, None, None, :], b16, table.masks[None])
    return np.ascontiguousarray(out).view(np.uint8).reshape(rows.shape[0], table.P, SLOTS, WIRE_ROW_BYTES)


def _differing_mask(r16: np.ndarray, b16: np.ndarray) -> np.ndarray:
    """uint32 [n]: bit i set where position i of the row and of the baseline differ in any bit."""
    ne = (r16 != b16).astype(np.uint32)                                      # [n, 32]
    out = np.zeros(r16.shape[0], np.uint32)
    for f in range(32):
        out |= ne[:, f] << _POS_OF_FIELD[f]
    return out


def coalition_logits(model, table: MlpExplainTable, rows_w64: np.ndarray) -> np.ndarray:
    """float32 [n, P, 32]: ``MLPModel.wire_logits`` of every slot's masked row.  A slot's row
    depends only on the mask bits of the positions where the row differs from the baseline, so
    each distinct (row, effective mask) is built and scored once: slots with equal bits get equal
    logits, whatever the matrix library does with the batch around them."""
    rows = np.ascontiguousarray(rows_w64, np.uint8).reshape(-1, WIRE_ROW_BYTES)
    r16 = rows.view(np.uint16)
    b16 = np.ascontiguousarray(table.baseline_w64).view(np.uint16)
    eff = table.masks[None] & _differing_mask(r16, b16)[:, None, None]       # [n, P, 32]
    key = (np.arange(rows.shape[0], dtype=np.uint64)[:, None, None] << np.uint64(32)) | eff.astype(np.uint64)
    uniq, back = np.unique(key.ravel(), return_inverse=True)
    which = (uniq >> np.uint64(32)).astype(np.int64)
    u16 = _masked_rows(r16[which], b16, (uniq & np.uint64(0xffffffff)).astype(np.uint32))
    z = model.wire_logits(decode_wire(np.ascontiguousarray(u16).view(np.uint8)))
    return z[back.ravel()].reshape(eff.shape)


def recombine(z: np.ndarray, table: MlpExplainTable, dtype=np.float64) -> np.ndarray:
    """phi [n, 30] (canonical feature order) from coalition logits ``z`` [n, P, 32], in the
    kernel's order: ``d[p][k] = z[p][k+1] - z[p][k]``, ``phi_j += d[p][inv[p][j]]`` over ``p``
    ascending, then one division by ``P``; all in ``dtype``."""
    z = np.asarray(z).astype(dtype)
    n, P = z.shape[0], table.P
    d = z[:, :, 1:] - z[:, :, :-1]                                           # [n, P, 31]
    acc = np.zeros((n, N_FEATURES), dtype)
    for p in range(P):
        acc = acc + d[:, p, table.inv[p, :N_FEATURES]]
    acc = (acc / dtype(P)).astype(dtype)
    phi = np.empty_like(acc)
    phi[:, WIRE_PERM] = acc
    return phi


def _shapley_table(model, table: MlpExplainTable, rows_w64: np.ndarray, dtype) -> Tuple[np.ndarray, np.ndarray]:
    z = coalition_logits(model, table, rows_w64)
    return recombine(z, table, dtype), z


def shapley_mlp_table(model, table_bytes: bytes, rows_w64: np.ndarray, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """The emulator of csrc/kernels/explain_mlp.hip on the CPU: ``(phi [n,30], z float32
    [n,P,32])`` from the packed table and W64 row bytes.  Every slot's row is built by the mask
    words and scored by ``MLPModel.wire_logits``; ``dtype`` is the arithmetic of the differences
    and of the sum over permutations (float32 is the kernel's)."""
    return _shapley_table(model, MlpExplainTable.unpack(table_bytes), rows_w64, dtype)


def shapley_mlp_sampled(model, X: np.ndarray, P: int = 64, seed: int = 0) -> Tuple[np.ndarray, float]:
    """``(phi float64 [n,30], base_value)`` of float32 ``[n,30]`` rows: the same estimator in
    float64 (any even ``P``, also above the packed table's limit)."""
    X = np.asarray(X, np.float32)
    if X.ndim != 2 or X.shape[1] != N_FEATURES:
        raise ValueError("X must be float32 [n, 30]")
    table = MlpExplainTable.build(model, P, seed)
    phi, _ = _shapley_table(model, table, encode_wire(X), np.float64)
    return phi, mlp_base_value(model)


def _wire_logits_of_rows(model, w64: np.ndarray) -> np.ndarray:
    """``wire_logits`` of W64 rows [k, 64], one evaluation per distinct row."""
    flat = np.ascontiguousarray(w64, np.uint8).reshape(-1, WIRE_ROW_BYTES)
    keys = flat.view(np.dtype((np.void, WIRE_ROW_BYTES))).ravel()
    _, first, back = np.unique(keys, return_index=True, return_inverse=True)
    return model.wire_logits(decode_wire(flat[first]))[back.ravel()]


def differing_positions(model, x: np.ndarray) -> np.ndarray:
    """The wire positions where the W64 bits of ``x`` and of the baseline differ."""
    a = encode_wire(np.asarray(x, np.float32).reshape(1, N_FEATURES))[0].view(np.uint16)
    b = encode_wire(_need_baseline(model)[None, :])[0].view(np.uint16)
    return np.array([i for i, fs in enumerate(_FIELDS) if any(a[f] != b[f] for f in fs)], np.int64)


def shapley_mlp_exact(model, x: np.ndarray, positions: Optional[Sequence[int]] = None) -> np.ndarray:
    """Exact baseline Shapley values of one row, float64 [30] (canonical order), by enumeration
    of every subset of ``positions`` (default: the positions where ``x`` differs from the
    baseline; at most 12).  The other positions keep the baseline's bits and get 0."""
    pos = differing_positions(model, x) if positions is None else np.asarray(positions, np.int64)
    m = len(pos)
    if m > EXACT_MAX_POSITIONS:
        raise ValueError(f"{m} positions differ from the baseline: enumeration stops at {EXACT_MAX_POSITIONS}")
    a16 = encode_wire(np.asarray(x, np.float32).reshape(1, N_FEATURES))[0].view(np.uint16)
    b16 = encode_wire(_need_baseline(model)[None, :])[0].view(np.uint16)
    rows = np.tile(b16, (1 << m, 1))
    for k, i in enumerate(pos):
        on = ((np.arange(1 << m) >> k) & 1).astype(bool)
        for f in _FIELDS[int(i)]:
            rows[on, f] = a16[f]
    v = _wire_logits_of_rows(model, rows.view(np.uint8)).astype(np.float64)
    size = np.array([bin(s).count("1") for s in range(1 << m)])
    w = np.array([factorial(s) * factorial(m - s - 1) / factorial(m) for s in range(m)]) if m else np.zeros(0)
    acc = np.zeros(N_FEATURES, np.float64)
    S = np.arange(1 << m)
    for k, i in enumerate(pos):
        out = S[((S >> k) & 1) == 0]
        acc[int(i)] = (w[size[out]] * (v[out | (1 << k)] - v[out])).sum()
    phi = np.empty_like(acc)
    phi[WIRE_PERM] = acc
    return phi


def shapley_lr(model, X: np.ndarray) -> Tuple[np.ndarray, float]:
    """Exact Shapley values of the logistic model against its baseline, the closed form
    ``phi_j = w_j (n(x_j) - n(b_j))`` with ``n`` the normaliser (log1p of Amount included):
    ``(phi float64 [n,30], base_value = logit(baseline))``."""
    b = _need_baseline(model)
    X = np.asarray(X, np.float32)
    if X.ndim != 2 or X.shape[1] != N_FEATURES:
        raise ValueError("X must be float32 [n, 30]")
    nx = model.norm(X).astype(np.float64)
    nb = model.norm(b[None, :]).astype(np.float64)
    phi = model.w.astype(np.float64)[None, :] * (nx - nb)
    return phi, float(nb[0] @ model.w.astype(np.float64) + model.b)
