"""General (non-oblivious) binary decision-tree ensembles: random forests, extra trees,
scikit-learn / XGBoost boosted trees (importers: models/sklearn_import.py,
models/xgboost_import.py; device kernels: csrc/kernels/score_forest.hip for f32 rows,
csrc/kernels/score_forest_bins.hip for G32 / G20 rows).

Every inner node has its own test: a row goes RIGHT iff ``x[feat] > thr`` as a float32
compare -- the predicate of the oblivious kernels, so NaN goes left (transactions are dense
floats; missing-value routing is out of scope).  Nodes live ensemble-wide in one array and
the two children of a node are adjacent: left = ``child``, right = ``child + 1``.  A leaf
carries one float32 value.  Each tree has a root node index and a depth (longest
root-to-leaf path; a single-leaf tree has depth 0).

``z = base + sum_t leaf_t(x)``; ``proba = sigmoid(z)`` for ``link == "sigmoid"`` (boosted
trees), ``clip(z, 0, 1)`` for ``link == "identity"`` (forests that average class fractions:
their leaves are pre-scaled by 1/T).  Features are RAW (trees are scale invariant).

Blob for the kernel (16-B aligned sections):
  [0,64)  header 'FRS1', flags (bit 0 = sigmoid link), T (i32), max_depth (i32), base (f32),
          n_nodes (i32)
  tree    i32  [T][2]       {root node index, depth}
  node    [n_nodes] x 8 B   {u32 w, f32 v}
            w bits 0..4  = feature, bit 5 = leaf flag, bits 8..31 = index of the left child
            v            = threshold of an inner node, value of a leaf
          a leaf's child field is its own index, so one step of the walk is
          ``next = leaf ? cur : child + (x[feat] > v)`` and a finished row stays put.

Binned rows (G32 / G20, contracts/transaction.py; device kernel: csrc/kernels/score_forest_bins.hip)
work for any tree: with a ``BinSpec`` whose edges contain the ensemble's thresholds, ``x > edges[k]``
<=> ``bin > k`` for every float (NaN -> bin 0 -> left).  The 'FRB1' blob is the FRS1 blob with the
spec's stamp in the header word at byte 24 and, for an inner node, ``v`` = the bin index k of its
threshold as u32 (255 for a NaN threshold, which never fires); leaves keep their f32 value.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..contracts.transaction import N_FEATURES
from .common import HEADER_BYTES, header, pad16, sigmoid
from .gbdt import MAX_BINS, BinSpec, ObliviousGBDT

MAX_DEPTH = 64
MAX_NODES = 1 << 24              # the blob's child field is 24 bits
# Node-table bytes the kernel keeps in LDS (csrc/kernels/score_forest.hip kNodeLdsBytes);
# larger tables are walked from global memory (L2).
LDS_NODE_BYTES = 144 * 1024
NODE_BYTES = 8
LINKS = ("sigmoid", "identity")


@dataclass
class TreeEnsemble:
    feat: np.ndarray      # int32 [n_nodes]   feature of an inner node (0 for a leaf)
    value: np.ndarray     # float32 [n_nodes] threshold of an inner node, value of a leaf
    child: np.ndarray     # int32 [n_nodes]   left child (right = child + 1); a leaf: its own index
    leaf: np.ndarray      # bool [n_nodes]
    root: np.ndarray      # int32 [T]
    base: float = 0.0
    link: str = "sigmoid"
    kind: str = "forest"
    cover: Optional[np.ndarray] = None    # float32 [n_nodes] background weight of every node (explanations)

    def __post_init__(self):
        self.feat = np.ascontiguousarray(self.feat, np.int32).reshape(-1)
        self.value = np.ascontiguousarray(self.value, np.float32).reshape(-1)
        self.child = np.ascontiguousarray(self.child, np.int32).reshape(-1)
        self.leaf = np.ascontiguousarray(self.leaf, bool).reshape(-1)
        self.root = np.ascontiguousarray(self.root, np.int32).reshape(-1)
        self.base = float(self.base)
        n = self.feat.size
        if self.link not in LINKS:
            raise ValueError(f"link must be one of {LINKS}")
        if not (self.value.size == self.child.size == self.leaf.size == n):
            raise ValueError("inconsistent node arrays")
        if self.root.size < 1 or n < 1:
            raise ValueError("an ensemble needs at least one tree")
        if n >= MAX_NODES:
            raise ValueError(f"{n} nodes: the node table holds fewer than 2^24")
        if self.feat.min() < 0 or self.feat.max() >= N_FEATURES:
            raise ValueError("feature index out of range")
        if self.root.min() < 0 or self.root.max() >= n:
            raise ValueError("root index out of range")
        idx = np.arange(n, dtype=np.int32)
        inner = ~self.leaf
        ci = self.child[inner]
        if ci.size and (ci.min() < 0 or ci.max() + 1 >= n):
            raise ValueError("child index out of range")
        if (ci <= idx[inner]).any():
            raise ValueError("child indices must point forward (child > node)")
        self.child = np.where(self.leaf, idx, self.child).astype(np.int32)
        self.feat = np.where(self.leaf, 0, self.feat).astype(np.int32)
        parents = np.zeros(n, np.int64)
        np.add.at(parents, ci, 1)
        np.add.at(parents, ci + 1, 1)
        np.add.at(parents, self.root, 1)
        if (parents > 1).any():
            raise ValueError("a node is reachable from two parents (or a root is shared / is a child)")
        # level-by-level expansion from the roots: per-tree depth
        depth = np.zeros(self.root.size, np.int32)
        owner = np.full(n, -1, np.int32)              # tree of every reachable node
        node, tree, level = self.root.copy(), np.arange(self.root.size), 0
        while True:
            owner[node] = tree
            keep = inner[node]
            node, tree = node[keep], tree[keep]
            if not node.size:
                break
            level += 1
            if level > MAX_DEPTH:
                raise ValueError(f"tree depth exceeds {MAX_DEPTH}")
            depth[tree] = level
            c = self.child[node]
            node, tree = np.concatenate([c, c + 1]), np.concatenate([tree, tree])
        self.tree_depth = depth
        self.node_tree = owner
        if self.cover is not None:
            self.cover = np.ascontiguousarray(self.cover, np.float32).reshape(-1)
            if self.cover.size != n:
                raise ValueError(f"cover has {self.cover.size} entries for {n} nodes")
            if not np.isfinite(self.cover).all() or (self.cover < 0).any():
                raise ValueError("cover must be finite and >= 0")

    # ------------------------------------------------------------------ shape
    @property
    def n_trees(self) -> int:
        return int(self.root.size)

    @property
    def depth(self) -> int:
        return int(self.tree_depth.max())

    @property
    def n_nodes(self) -> int:
        return int(self.feat.size)

    def leaf_abs_max(self) -> np.ndarray:
        """max |leaf value| per tree -- float64 [T] (the scale of float32 summation error)."""
        out = np.zeros(self.n_trees, np.float64)
        sel = self.leaf & (self.node_tree >= 0)
        np.maximum.at(out, self.node_tree[sel], np.abs(self.value[sel].astype(np.float64)))
        return out

    # ------------------------------------------------------------------ scoring (CPU oracle)
    def leaf_node(self, X: np.ndarray) -> np.ndarray:
        """Index of the leaf every (row, tree) ends in -- [n, T]."""
        X = np.asarray(X, np.float32)
        cur = np.broadcast_to(self.root[None, :], (X.shape[0], self.n_trees)).astype(np.int64)
        rows = np.arange(X.shape[0])[:, None]
        for _ in range(self.depth):
            right = X[rows, self.feat[cur]] > self.value[cur]      # f32 compare; NaN -> left
            cur = np.where(self.leaf[cur], cur, self.child[cur] + right)
        return cur

    def leaf_values(self, X: np.ndarray) -> np.ndarray:
        """The selected leaf value per tree -- float32 [n, T]."""
        return self.value[self.leaf_node(X)]

    def raw_score(self, X: np.ndarray) -> np.ndarray:
        return (self.base + self.leaf_values(X).astype(np.float64).sum(1)).astype(np.float32)

    def predict_proba(self, X: np.ndarray) -> np.ndarray:
        z = self.raw_score(X)
        return sigmoid(z) if self.link == "sigmoid" else np.clip(z, 0.0, 1.0).astype(np.float32)

    def fit_cover(self, X: np.ndarray) -> "TreeEnsemble":
        """A copy whose ``cover`` counts the rows of ``X`` (float32 [n,30]) at every node: the
        background of the Shapley attributions (models/explain_forest.py).  Counted in int64."""
        X = np.asarray(X, np.float32)
        if X.ndim != 2 or X.shape[1] != N_FEATURES:
            raise ValueError("background rows must be float32 [n, 30]")
        count = np.zeros(self.n_nodes, np.int64)
        cur = np.broadcast_to(self.root[None, :], (X.shape[0], self.n_trees)).astype(np.int64)
        rows = np.arange(X.shape[0])[:, None]
        count += np.bincount(cur.reshape(-1), minlength=self.n_nodes)
        for _ in range(self.depth):
            inner = ~self.leaf[cur]
            right = X[rows, self.feat[cur]] > self.value[cur]
            cur = np.where(inner, self.child[cur] + right, cur)
            count += np.bincount(cur[inner], minlength=self.n_nodes)
        return TreeEnsemble(self.feat, self.value, self.child, self.leaf, self.root, self.base, self.link,
                            cover=count.astype(np.float32))

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_oblivious(cls, m: ObliviousGBDT) -> "TreeEnsemble":
        """Each oblivious tree expanded into a complete general tree with identical outputs
        (level l of the tree tests split l; NaN thresholds carry over: ``x > NaN`` is false).  The
        cover of the oblivious model, if it has one, carries over: a node's is the sum of its leaves'."""
        T, D = m.n_trees, m.depth
        per = (2 << D) - 1
        L = 1 << D
        # node at level l, position p (its path bits, first step = most significant)
        lvl = np.concatenate([np.full(1 << l, l) for l in range(D + 1)])
        pos = np.concatenate([np.arange(1 << l) for l in range(D + 1)])
        is_leaf = lvl == D
        # the oblivious leaf index has the bit of level d at position d: bit-reverse the path
        rev = np.zeros(L, np.int64)
        for d in range(D):
            rev |= ((np.arange(L) >> d) & 1) << (D - 1 - d)
        feat = np.zeros((T, per), np.int32)
        value = np.zeros((T, per), np.float32)
        child = np.zeros((T, per), np.int32)
        li = np.minimum(lvl, D - 1)
        feat[:, ~is_leaf] = m.feat[:, li[~is_leaf]]
        value[:, ~is_leaf] = m.thr[:, li[~is_leaf]]
        value[:, is_leaf] = m.leaves[:, rev[pos[is_leaf]]]
        off = np.arange(T, dtype=np.int64)[:, None] * per
        child[:] = (off + ((2 << lvl) - 1 + 2 * pos)[None, :]).astype(np.int32)
        cover = None
        if getattr(m, "cover", None) is not None:
            # leaf cover in path order, then every level is the pairwise sum of the one below
            levels = [np.asarray(m.cover, np.float64)[:, rev]]
            for _ in range(D):
                levels.append(levels[-1][:, 0::2] + levels[-1][:, 1::2])
            cover = np.concatenate(levels[::-1], axis=1).astype(np.float32).reshape(-1)
        return cls(feat.reshape(-1), value.reshape(-1), child.reshape(-1), np.tile(is_leaf, T),
                   (off[:, 0]).astype(np.int32), float(m.base), "sigmoid", cover=cover)

    @classmethod
    def random_init(cls, n_trees: int = 16, max_depth: int = 8, p_leaf: float = 0.2, seed: int = 0,
                    X_ref: Optional[np.ndarray] = None, link: str = "sigmoid") -> "TreeEnsemble":
        """Random, unbalanced trees: below the root a node becomes a leaf with probability
        ``p_leaf`` (always at ``max_depth``); thresholds are feature quantiles of ``X_ref``
        (or N(0,1)) so that splits partition the data.  Reproducible by ``seed``."""
        rng = np.random.default_rng(seed)
        qs = None
        if X_ref is not None:
            qs = np.quantile(np.asarray(X_ref, np.float32), np.linspace(0.05, 0.95, 19), axis=0).astype(np.float32)
        feat, value, child, leaf, root = [], [], [], [], []

        def new_node():
            feat.append(0); value.append(0.0); child.append(0); leaf.append(True)
            return len(feat) - 1

        for _ in range(n_trees):
            r = new_node()
            root.append(r)
            frontier = [(r, 0)]
            while frontier:
                nxt = []
                for i, d in frontier:
                    if d == max_depth or (d > 0 and rng.random() < p_leaf):
                        value[i] = float(rng.standard_normal() * 0.1)
                        continue
                    f = int(rng.integers(0, N_FEATURES))
                    feat[i] = f
                    value[i] = float(qs[rng.integers(0, qs.shape[0]), f]) if qs is not None else float(rng.standard_normal())
                    leaf[i] = False
                    a = new_node()
                    new_node()
                    child[i] = a
                    nxt += [(a, d + 1), (a + 1, d + 1)]
                frontier = nxt
        return cls(np.array(feat), np.array(value, np.float32), np.array(child), np.array(leaf), np.array(root),
                   0.0, link)

    # ------------------------------------------------------------------ device blob
    def _split_nodes(self) -> np.ndarray:
        """Indices of the inner nodes a walk can reach (nodes no root leads to are never tested)."""
        return np.flatnonzero(~self.leaf & (self.node_tree >= 0))

    def bin_spec(self, bits: int = 8) -> BinSpec:
        """The smallest bin table of this ensemble -- the distinct non-NaN thresholds of its
        reachable inner nodes, per feature -- for G32 rows (``bits=8``; ValueError past 255
        thresholds a feature: such a forest keeps f32 rows) or G20 rows (``bits=5``; past 31)."""
        i = self._split_nodes()
        spec = BinSpec.from_thresholds(self.feat[i], self.value[i])
        return spec if bits == 8 else spec.with_bits(bits)

    def leaf_node_binned(self, rows: np.ndarray, bins: Optional[BinSpec] = None) -> np.ndarray:
        """``leaf_node`` from binned rows (u8 [n,32] G32 rows, or [n,20] G20 rows of a 5-bit
        spec; ``BinSpec.encode``) -- the device walk's form of every step, ``bin[feat] > k`` with
        k the threshold's edge index -- [n, T]."""
        spec = bins if bins is not None else self.bin_spec()
        k = np.zeros(self.n_nodes, np.int32)
        i = self._split_nodes()
        k[i] = spec.bin_index(self.feat[i], self.value[i])               # NaN thresholds: 255
        if spec.bits == 5:
            from ..contracts.transaction import decode_g20_bins
            b = decode_g20_bins(rows).astype(np.int32)
        else:
            b = np.asarray(rows, np.uint8)[:, :N_FEATURES].astype(np.int32)
        cur = np.broadcast_to(self.root[None, :], (b.shape[0], self.n_trees)).astype(np.int64)
        r = np.arange(b.shape[0])[:, None]
        for _ in range(self.depth):
            right = b[r, self.feat[cur]] > k[cur]
            cur = np.where(self.leaf[cur], cur, self.child[cur] + right)
        return cur

    def pack(self, wire: bool = False, bins: Optional[BinSpec] = None) -> bytes:
        """FRS1 blob for f32 rows, or (``bins``) the FRB1 blob for G32 / G20 rows of that spec;
        a threshold that is not one of its edges raises ``BinSpec``'s ValueError.  General trees
        have no W64 kernel."""
        if wire:
            raise ValueError("general trees score f32 rows, or G32 / G20 rows (bins=): no W64 wire rows")
        w = (self.feat.astype(np.uint32) | (self.leaf.astype(np.uint32) << 5) | (self.child.astype(np.uint32) << 8))
        node = np.empty((self.n_nodes, 2), np.uint32)
        node[:, 0] = w
        node[:, 1] = self.value.view(np.uint32)
        tree = np.stack([self.root, self.tree_depth], 1).astype(np.int32)
        flags = 1 if self.link == "sigmoid" else 0
        if bins is None:
            blob = header(b"FRS1", flags, self.n_trees, self.depth, float(self.base), self.n_nodes)
        else:
            inner = np.flatnonzero(~self.leaf)
            reach = self.node_tree[inner] >= 0
            k = np.full(inner.size, MAX_BINS, np.int32)                  # unreachable: never fires
            k[reach] = bins.bin_index(self.feat[inner[reach]], self.value[inner[reach]])
            node[inner, 1] = k.astype(np.uint32)
            blob = header(b"FRB1", flags, self.n_trees, self.depth, float(self.base), self.n_nodes, int(bins.stamp))
        return blob + pad16(tree.tobytes()) + pad16(node.tobytes())

    @classmethod
    def unpack(cls, blob: bytes) -> "TreeEnsemble":
        if blob[:4] != b"FRS1":
            raise ValueError("not an FRS1 blob")
        flags, T, _depth = struct.unpack_from("<Iii", blob, 4)
        base = struct.unpack_from("<f", blob, 16)[0]
        n = struct.unpack_from("<i", blob, 20)[0]
        off_node = HEADER_BYTES + ((8 * T + 15) & ~15)
        tree = np.frombuffer(blob, np.int32, 2 * T, HEADER_BYTES).reshape(T, 2)
        node = np.frombuffer(blob, np.uint32, 2 * n, off_node).reshape(n, 2)
        w = node[:, 0]
        m = cls((w & 31).astype(np.int32), node[:, 1].copy().view(np.float32), (w >> 8).astype(np.int32),
                (w >> 5 & 1).astype(bool), tree[:, 0].copy(), float(base), "sigmoid" if flags & 1 else "identity")
        if not np.array_equal(m.tree_depth, tree[:, 1]):
            raise ValueError("FRS1 blob: stored tree depths do not match the node table")
        return m

    def state_dict(self) -> dict:
        st = {"forest.feat": self.feat, "forest.value": self.value, "forest.child": self.child,
              "forest.leaf": self.leaf.astype(np.uint8), "forest.root": self.root,
              "forest.base": np.array([self.base], np.float64),
              "forest.link": np.array([LINKS.index(self.link)], np.int32)}
        if self.cover is not None:
            st["forest.cover"] = self.cover
        return st

    @classmethod
    def from_state_dict(cls, st: dict) -> "TreeEnsemble":
        return cls(st["forest.feat"], st["forest.value"], st["forest.child"], np.asarray(st["forest.leaf"]) != 0,
                   st["forest.root"], float(np.asarray(st["forest.base"]).reshape(-1)[0]),
                   LINKS[int(np.asarray(st["forest.link"]).reshape(-1)[0])],
                   cover=st["forest.cover"] if "forest.cover" in st else None)
