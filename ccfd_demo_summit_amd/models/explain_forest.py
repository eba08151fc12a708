"""Exact per-feature Shapley values of a general tree ensemble (``TreeEnsemble`` with ``cover``):
path-dependent TreeSHAP of ``raw_score``, the definition of docs/EXPLAIN.md.  This module holds
the two CPU oracles, the packer of the 'FRX1' blob that csrc/kernels/explain_forest.hip reads,
and a CPU emulator of that kernel's algorithm on the unpacked blob.

Only children's covers enter a split: the share of child ``c`` of inner node ``n`` is
``cover[c] / (cover[left] + cover[right])`` and ``n`` is *empty* when that sum is 0.  For one
tree, a row ``x`` and a feature set ``S``, ``v_S(n)`` is the leaf value at a leaf,
``v_S(child x goes to)`` if ``feat[n]`` is in ``S`` or ``n`` is empty (follow the row), and
otherwise ``sum_c share(c) v_S(c)``.  ``phi_j`` is the Shapley value of ``j`` in the game
``S -> v_S(root)`` summed over trees; ``base_value = base + sum_t v_0(root_t)``; ``base_value +
sum_j phi_j == raw_score(x)``.  ``v_0`` has to be a constant: a tree in which an empty inner node
is reached with a non-zero product of shares (its root, or a node whose own cover disagrees
with its children's) is refused with ``ValueError``.

Path form (``shapley_forest``, the kernel).  On one root-to-leaf path the splits at non-empty
nodes are merged per feature into one *player* ``i``: the row satisfies it (``o_i = 1``) iff
every one of those splits sends it along the path, ``z_i`` is the product of their shares.
The splits at empty nodes are the path's *gate*: the path counts only for a row that passes
all of them; gates are no players.  With A the satisfied players, B the others and m players

    phi[f_e] += leaf * gate * (o_e - z_e) * prod_{i in B, i != e} z_i * sum_k q_k k! (m-k-1)! / m!

where ``q`` are the coefficients of ``prod_{i in A, i != e} (z_i + y)``.  Nothing divides by a
``z`` (a share may be exactly 0): ``(z_e + y)`` leaves the monic product by synthetic division
from the top, ``q_{a-1} = c_a, q_{k-1} = c_k - z_e q_k``.  That is the float64 oracle.

Integral form (the kernel and its emulator ``table_shapley_forest``).  In float32 the division
loses the small end coefficients under the rounding of the large middle ones (a 16-player chain
with shares near 1: 9 u for one attribution and 80 u for local accuracy, u as in the tests), so
the kernel uses ``k! (m-k-1)! / m! = int_0^1 t^k (1-t)^(m-k-1) dt``, which turns the sum into

    phi[f_e] += leaf * gate * (o_e - z_e) * int_0^1 prod_{i != e} (o_i t + z_i (1 - t)) dt

The integrand is a polynomial of degree m - 1 in t, so the Gauss-Legendre rule of ceil(m / 2)
nodes is exact; every factor lies in [0, 1], every term is >= 0, and the product
without ``e`` is a prefix times a suffix: no division and no cancellation (3.4 u and 3.7 u on
that chain).  A spare slot of a record narrower than W is the null player ``o = z = 1``.

FRX1 blob (sections back to back, each a multiple of 8 bytes; padded to 16 B at the end):
  [0,64)   header 'FRX1', flags, P paths (i32), W (i32), base_value (f32), bin stamp (i32),
           S slices (i32), R words of the record section (i32)
           W is the width bucket of the blob: the smallest of 4 / 8 / 12 / 16 that holds the
           widest path
  rules    f64 [8][2][8]     rules[q-1]: the q-point Gauss-Legendre rule on (0, 1), nodes t_j,
                             then their weights (sum 1), 0 past q; a record of m players
                             uses q = ceil(m / 2)
  seg      i32 [S][4][2]     per slice and wave of a workgroup: {first word of its run of
                             records, number of records}; the runs are consecutive
  rec      u32 [R]           one record per leaf that a row can reach and that has a player:
             f32 leaf value
             u32 m | gates << 8
             m x {u32 feature | (lo + 1) << 8 | hi << 20, f32 z}    satisfied iff lo < bin <= hi
             gates x u32 feature | (lo + 1) << 8 | hi << 20         passed iff lo < bin <= hi
           a record has an even number of words (one 0 word after an odd number of gates)
``z`` is formed in float64 and rounded once.  Leaves without a player (single-leaf trees, paths
of gates only) move ``base_value`` alone and have no record; a path whose gates contradict
each other can be reached by no row and is dropped.  The slices are fixed here, at pack time:
the kernel adds the partial sums of the waves of a slice, and then the slices, in this order,
whatever the batch.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from itertools import combinations
from math import factorial
from typing import List, Optional, Tuple

import numpy as np

from ..contracts.transaction import N_FEATURES
from .common import HEADER_BYTES, header, pad16
from .forest import TreeEnsemble
from .gbdt import BinSpec

MAX_WIDTH = 16                  # players of one path the kernel holds in registers
WIDTHS = (4, 8, 12, 16)         # the kernel's instantiations
MAX_ENUM_FEATURES = 12
WAVES = 4                       # waves of a workgroup (csrc/kernels/explain_forest.hip)
SLICE_PATHS = 512               # paths of a slice, until MAX_SLICES is reached
MAX_SLICES = 16
RULE_BYTES = 8 * (MAX_WIDTH // 2) * 2 * (MAX_WIDTH // 2)


def _need_cover(model: TreeEnsemble) -> np.ndarray:
    if getattr(model, "kind", None) != "forest":
        raise ValueError("shapley_forest explains a TreeEnsemble (kind 'forest')")
    if getattr(model, "cover", None) is None:
        raise ValueError("the ensemble has no cover (background weight of every node): call fit_cover(X) first, "
                         "or import a model that carries one")
    return model.cover.astype(np.float64)


def forest_quadrature() -> np.ndarray:
    """float64 [8, 2, 8]: ``[q - 1]`` holds the nodes on (0, 1) and the weights of the q-point
    Gauss-Legendre rule (exact for polynomials of degree < 2 q), zero-padded."""
    out = np.zeros((MAX_WIDTH // 2, 2, MAX_WIDTH // 2), np.float64)
    for q in range(1, MAX_WIDTH // 2 + 1):
        x, w = np.polynomial.legendre.leggauss(q)
        out[q - 1, 0, :q] = (x + 1.0) / 2.0
        out[q - 1, 1, :q] = w / 2.0
    return out


def _weights_row(m: int) -> np.ndarray:
    return np.array([factorial(k) * factorial(m - k - 1) / factorial(m) for k in range(m)], np.float64)


# ------------------------------------------------------------------------------- the paths
@dataclass
class _Path:
    tree: int
    leaf: float                       # value of the leaf
    feats: List[int]                  # one entry per player, in order of first use
    splits: List[List[Tuple[int, int]]]   # per player: (node, direction taken: 1 = right)
    z: List[float]                    # per player: product of the shares, float64
    gates: List[Tuple[int, int]]      # (node, direction taken) of the empty nodes


def _tree_paths(model: TreeEnsemble, cover: np.ndarray, t: int) -> Tuple[List[_Path], float]:
    """(the root-to-leaf paths of tree ``t``, v_0(root))."""
    out: List[_Path] = []
    v0 = 0.0
    stack = [(int(model.root[t]), [], [], [], [], 1.0)]
    while stack:
        n, feats, splits, z, gates, weight = stack.pop()
        if model.leaf[n]:
            out.append(_Path(t, float(model.value[n]), feats, splits, z, gates))
            v0 += float(model.value[n]) * weight
            continue
        c = int(model.child[n])
        tot = cover[c] + cover[c + 1]
        if tot == 0 and weight != 0:
            raise ValueError(f"tree {t}: no background row reaches the children of node {n}, which the background "
                             "itself reaches (an empty root, or a cover that disagrees with its children's): "
                             "the tree has no constant base value")
        for d in (1, 0):                              # right pushed first: left paths come out first
            if tot == 0:
                stack.append((c + d, feats, splits, z, gates + [(n, d)], 0.0))
                continue
            share = cover[c + d] / tot
            f = int(model.feat[n])
            if f in feats:
                i = feats.index(f)
                sp = [s + [(n, d)] if j == i else s for j, s in enumerate(splits)]
                zz = [v * share if j == i else v for j, v in enumerate(z)]
                stack.append((c + d, feats, sp, zz, gates, weight * share))
            else:
                stack.append((c + d, feats + [f], splits + [[(n, d)]], z + [share], gates, weight * share))
    return out, v0


def forest_paths(model: TreeEnsemble):
    """(every root-to-leaf path of the ensemble, tree by tree and left to right; base_value)."""
    cover = _need_cover(model)
    paths: List[_Path] = []
    bv = float(model.base)
    for t in range(model.n_trees):
        p, v0 = _tree_paths(model, cover, t)
        paths += p
        bv += v0
    return paths, bv


def forest_base_value(model: TreeEnsemble) -> float:
    return forest_paths(model)[1]


def _went_right(model: TreeEnsemble, X: np.ndarray, bins: Optional[BinSpec]) -> np.ndarray:
    """bool [n, n_nodes]: the row passes the test of the node (``x[feat] > thr`` / ``bin > k``)."""
    X = np.asarray(X)
    if X.dtype == np.uint8:
        spec = bins if bins is not None else model.bin_spec()
        if X.ndim != 2 or X.shape[1] != (32 if spec.bits == 8 else 20):
            raise ValueError(f"binned rows must be u8 [n,{32 if spec.bits == 8 else 20}]")
        if spec.bits == 5:
            from ..contracts.transaction import decode_g20_bins
            b = decode_g20_bins(X).astype(np.int32)
        else:
            b = X[:, :N_FEATURES].astype(np.int32)
        return b[:, model.feat] > _split_bins(model, spec)[None, :]
    if X.ndim != 2 or X.shape[1] != N_FEATURES:
        raise ValueError("rows must be float32 [n,30] features or u8 G32 / G20 rows")
    X = X.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return X[:, model.feat] > model.value[None, :]


def _split_bins(model: TreeEnsemble, spec: BinSpec) -> np.ndarray:
    """The bin index k of every reachable inner node's threshold (255 for NaN, which never fires)."""
    k = np.full(model.n_nodes, 255, np.int32)
    i = model._split_nodes()
    k[i] = spec.bin_index(model.feat[i], model.value[i])
    return k


# ------------------------------------------------------------------------------- the oracles
def shapley_forest_enum(model: TreeEnsemble, X: np.ndarray, bins: Optional[BinSpec] = None) -> Tuple[np.ndarray, float]:
    """(phi float64 [n,30], base_value) straight from the definition: every subset of every tree's
    distinct features.  Ground truth for small trees: more than 12 distinct features in a tree
    are refused."""
    cover = _need_cover(model)
    bv = forest_base_value(model)
    right = _went_right(model, X, bins)
    n = right.shape[0]
    phi = np.zeros((n, N_FEATURES), np.float64)
    for t in range(model.n_trees):
        nodes = np.flatnonzero((model.node_tree == t) & ~model.leaf)
        feats = sorted(set(model.feat[nodes].tolist()))
        m = len(feats)
        if m > MAX_ENUM_FEATURES:
            raise ValueError(f"tree {t} tests {m} distinct features: enumeration is for at most {MAX_ENUM_FEATURES}")

        def value(node, S):
            if model.leaf[node]:
                return np.full(n, float(model.value[node]))
            c = int(model.child[node])
            tot = cover[c] + cover[c + 1]
            lo, hi = value(c, S), value(c + 1, S)
            if tot == 0 or int(model.feat[node]) in S:
                return np.where(right[:, node], hi, lo)
            return (cover[c] / tot) * lo + (cover[c + 1] / tot) * hi

        v = {}
        for size in range(m + 1):
            for S in combinations(feats, size):
                v[frozenset(S)] = value(int(model.root[t]), frozenset(S))
        for j in feats:
            rest = [f for f in feats if f != j]
            for size in range(m):
                w = factorial(size) * factorial(m - size - 1) / factorial(m)
                for S in combinations(rest, size):
                    S = frozenset(S)
                    phi[:, j] += w * (v[S | {j}] - v[S])
    return phi, bv


def shapley_forest(model: TreeEnsemble, X: np.ndarray, bins: Optional[BinSpec] = None,
                   dtype=np.float64) -> Tuple[np.ndarray, float]:
    """(phi [n,30], base_value) by the path form of the module docstring, in polynomial time for
    any depth the model allows.  ``X``: float32 [n,30] features, or u8 G32 / G20 rows of ``bins``
    (the model's own table by default).  ``dtype`` is the arithmetic of the polynomials and the
    sums (``z`` is formed in float64 and rounded once, as in the blob)."""
    paths, bv = forest_paths(model)
    right = _went_right(model, X, bins)
    n = right.shape[0]
    phi = np.zeros((n, N_FEATURES), dtype)
    one, zero = dtype(1), dtype(0)
    for p in paths:
        m = len(p.feats)
        if m == 0:
            continue
        gate = np.ones(n, bool)
        for node, d in p.gates:
            gate &= right[:, node] == bool(d)
        if not gate.any():
            continue
        sat = np.ones((n, m), bool)
        for i, sp in enumerate(p.splits):
            for node, d in sp:
                sat[:, i] &= right[:, node] == bool(d)
        z = np.array(p.z, np.float64).astype(dtype)
        w = _weights_row(m).astype(dtype)
        lead = (dtype(p.leaf) * gate.astype(dtype)).astype(dtype)
        # c[:, k]: coefficient of y^k of prod_{i in A} (z_i + y); out: prod_{i in B} z_i without i
        c = np.zeros((n, m + 1), dtype)
        c[:, 0] = one
        for i in range(m):
            grown = z[i] * c
            grown[:, 1:] += c[:, :-1]
            c = np.where(sat[:, i:i + 1], grown, c)
        for e in range(m):
            others = np.ones(n, dtype)
            for i in range(m):
                if i != e:
                    others = np.where(sat[:, i], others, others * z[i])
            q = np.zeros((n, m), dtype)                # the division, for the rows that satisfy e
            top = np.zeros(n, dtype)
            for k in range(m, 0, -1):
                top = c[:, k] - z[e] * top
                q[:, k - 1] = top
            q = np.where(sat[:, e:e + 1], q, c[:, :m])
            s = np.zeros(n, dtype)
            for k in range(m):
                s = s + q[:, k] * w[k]
            phi[:, p.feats[e]] += lead * (np.where(sat[:, e], one, zero) - z[e]) * others * s
    return phi, bv


# ------------------------------------------------------------------------------- the FRX1 table
def _interval(model: TreeEnsemble, k: np.ndarray, splits) -> Tuple[int, int]:
    """The bin interval ``lo < bin <= hi`` of rows that every split sends along the path."""
    lo, hi = -1, 255
    for node, d in splits:
        if d:
            lo = max(lo, int(k[node]))
        else:
            hi = min(hi, int(k[node]))
    return lo, hi


def _word(feat: int, lo: int, hi: int) -> int:
    return int(feat) | (lo + 1) << 8 | hi << 20


def _unword(w: int) -> Tuple[int, int, int]:
    return w & 31, ((w >> 8) & 0x1ff) - 1, (w >> 20) & 0xff


@dataclass
class ForestExplainTable:
    """The unpacked content of an FRX1 blob: per record its leaf value, players and gates."""
    leaf: np.ndarray                 # f32 [P]
    m: np.ndarray                    # i32 [P]
    feat: np.ndarray                 # i32 [P, W] (first m valid)
    lo: np.ndarray                   # i32 [P, W]
    hi: np.ndarray                   # i32 [P, W]
    z: np.ndarray                    # f32 [P, W]
    gates: List[List[Tuple[int, int, int]]]    # per record: (feature, lo, hi)
    seg: np.ndarray                  # i32 [S, 4, 2]
    rules: np.ndarray                # f64 [8, 2, 8] quadrature nodes and weights of the q-point rules
    width: int
    base_value: float
    stamp: int

    @property
    def paths(self) -> int:
        return int(self.leaf.size)

    @property
    def slices(self) -> int:
        return int(self.seg.shape[0])

    @staticmethod
    def offsets(S: int, R: int):
        off_w = HEADER_BYTES
        off_seg = off_w + RULE_BYTES
        off_rec = off_seg + 4 * 2 * WAVES * S
        return off_w, off_seg, off_rec, off_rec + 4 * R

    @classmethod
    def pack(cls, model: TreeEnsemble, bins: Optional[BinSpec] = None) -> bytes:
        paths, bv = forest_paths(model)
        spec = bins if bins is not None else model.bin_spec()
        if spec.bits != 8:
            raise ValueError("the explain kernel reads G32 rows: pack against an 8-bit BinSpec")
        k = _split_bins(model, spec)
        recs: List[np.ndarray] = []
        width = 1
        for p in paths:
            m = len(p.feats)
            if m == 0:
                continue
            if m > MAX_WIDTH:
                raise ValueError(f"tree {p.tree}: a path tests {m} distinct features; the explain kernel holds "
                                 f"{MAX_WIDTH} (shapley_forest explains such a model on the CPU)")
            merged = {}
            for node, d in p.gates:
                merged.setdefault(int(model.feat[node]), []).append((node, d))
            gates = [(f,) + _interval(model, k, sp) for f, sp in merged.items()]
            if any(lo >= hi for _, lo, hi in gates):
                continue                                  # no row passes this path's gates
            r = np.zeros(2 + 2 * m + len(gates) + (len(gates) & 1), np.uint32)
            r[0] = np.array([p.leaf], np.float32).view(np.uint32)[0]
            r[1] = m | len(gates) << 8
            for i in range(m):
                r[2 + 2 * i] = _word(p.feats[i], *_interval(model, k, p.splits[i]))
            r[3:3 + 2 * m:2] = np.array(p.z, np.float64).astype(np.float32).view(np.uint32)
            for g, (f, lo, hi) in enumerate(gates):
                r[2 + 2 * m + g] = _word(f, lo, hi)
            recs.append(r)
            width = max(width, m)
        P = len(recs)
        W = next(w for w in WIDTHS if w >= width)
        S = max(1, min(MAX_SLICES, -(-P // SLICE_PATHS)))
        first = np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.int64)
        seg = np.zeros((S, WAVES, 2), np.int32)
        for g in range(S * WAVES):
            a, b = P * g // (S * WAVES), P * (g + 1) // (S * WAVES)
            seg[g // WAVES, g % WAVES] = (first[a], b - a)
        rec = np.concatenate(recs) if recs else np.zeros(0, np.uint32)
        if rec.size >= 1 << 31:
            raise ValueError("the path table exceeds 2^31 words")
        blob = header(b"FRX1", 0, P, W, float(np.float32(bv)), int(spec.stamp), S, int(rec.size))
        blob += forest_quadrature().tobytes() + seg.tobytes() + rec.tobytes()
        assert len(blob) == cls.offsets(S, rec.size)[-1]
        return pad16(blob)

    @classmethod
    def unpack(cls, blob: bytes) -> "ForestExplainTable":
        if blob[:4] != b"FRX1":
            raise ValueError("not an FRX1 blob")
        P, W = struct.unpack_from("<ii", blob, 8)
        bv, stamp, S, R = struct.unpack_from("<fiii", blob, 16)
        ow, oseg, orec, end = cls.offsets(S, R)
        if len(blob) < end:
            raise ValueError("truncated FRX1 blob")
        seg = np.frombuffer(blob, np.int32, 2 * WAVES * S, oseg).reshape(S, WAVES, 2).copy()
        rec = np.frombuffer(blob, np.uint32, R, orec)
        leaf = np.zeros(P, np.float32)
        m = np.zeros(P, np.int32)
        feat, lo, hi = (np.zeros((P, W), np.int32) for _ in range(3))
        z = np.zeros((P, W), np.float32)
        gates = []
        at = 0
        for p in range(P):
            leaf[p] = rec[at:at + 1].view(np.float32)[0]
            m[p], ng = int(rec[at + 1]) & 0xff, int(rec[at + 1]) >> 8 & 0xff
            if m[p] > W:
                raise ValueError("FRX1 blob: a record is wider than the blob's width")
            for i in range(m[p]):
                feat[p, i], lo[p, i], hi[p, i] = _unword(int(rec[at + 2 + 2 * i]))
            z[p, :m[p]] = rec[at + 3:at + 3 + 2 * m[p]:2].view(np.float32)
            gates.append([_unword(int(w)) for w in rec[at + 2 + 2 * m[p]:at + 2 + 2 * m[p] + ng]])
            at += 2 + 2 * int(m[p]) + ng + (ng & 1)
        if at != R:
            raise ValueError("FRX1 blob: the records do not fill the record section")
        return cls(leaf, m, feat, lo, hi, z, gates, seg,
                   np.frombuffer(blob, np.float64, RULE_BYTES // 8, ow).reshape(MAX_WIDTH // 2, 2, MAX_WIDTH // 2).copy(),
                   int(W), float(bv), int(stamp))


def table_shapley_forest(tab: ForestExplainTable, rows: np.ndarray, dtype=np.float32) -> np.ndarray:
    """The kernel's algorithm on the unpacked table, in ``dtype`` arithmetic: phi [n,30] of G32
    ``rows``.  Every record is widened to the blob's W players (a spare player is the null player
    o = z = 1); at every node of the rule of ceil(m / 2) points the product of the other players'
    factors is a running prefix times a stored suffix; sums follow the kernel's order: records
    of a wave's run, then the 4 waves of a slice, then the slices.  A row whose stamp differs
    from the table's gets NaN."""
    rows = np.asarray(rows, np.uint8)
    n = rows.shape[0]
    b = rows[:, :N_FEATURES].astype(np.int32)
    rules = tab.rules.astype(dtype)
    total = np.zeros((n, N_FEATURES), dtype)
    first = {}
    at = 0
    for p in range(tab.paths):
        first[at] = p
        at += 2 + 2 * int(tab.m[p]) + len(tab.gates[p]) + (len(tab.gates[p]) & 1)
    for s in range(tab.slices):
        part = []
        for wv in range(WAVES):
            phi = np.zeros((n, N_FEATURES), dtype)
            if tab.seg[s, wv, 1]:
                p0 = first[int(tab.seg[s, wv, 0])]
                for p in range(p0, p0 + int(tab.seg[s, wv, 1])):
                    _emulate_record(tab, p, b, phi, rules, dtype)
            part.append(phi)
        acc = part[0]
        for wv in range(1, WAVES):
            acc = acc + part[wv]
        total = total + acc
    total[rows[:, 31] != tab.stamp] = np.nan
    return total


def _emulate_record(tab, p, b, phi, rules, dtype):
    n, m = b.shape[0], int(tab.m[p])
    nq = (m + 1) // 2                                   # nodes that integrate degree m - 1 exactly
    rule = rules[nq - 1]
    one, zero = dtype(1), dtype(0)
    lead = np.full(n, dtype(tab.leaf[p]), dtype)
    for f, lo, hi in tab.gates[p]:
        lead = np.where((b[:, f] > lo) & (b[:, f] <= hi), lead, zero)
    z = [dtype(tab.z[p, i]) for i in range(m)]
    sat = [(b[:, tab.feat[p, i]] > tab.lo[p, i]) & (b[:, tab.feat[p, i]] <= tab.hi[p, i]) for i in range(m)]
    acc = [np.zeros(n, dtype) for _ in range(m)]
    for j in range(nq):
        t, om = rule[0, j], rule[1, j]
        u = one - t
        f = [np.where(sat[i], z[i] * u + t, z[i] * u).astype(dtype) for i in range(m)]
        suf = [None] * m
        suf[m - 1] = np.full(n, one, dtype)
        for i in range(m - 1, 0, -1):
            suf[i - 1] = suf[i] * f[i]
        pre = np.full(n, one, dtype)
        for e in range(m):
            acc[e] = om * (pre * suf[e]) + acc[e]
            pre = pre * f[e]
    for e in range(m):
        phi[:, tab.feat[p, e]] += (lead * (np.where(sat[e], one, zero) - z[e])) * acc[e]
