"""Edge fixtures for the oblivious-GBDT kernels (test_gbdt_edges_cpu.py proves their
properties on the numpy reference alone, test_gbdt_edges_gpu.py and gbdt_variant_probe.py
run them through the kernels).  Pure numpy.

Every ensemble here is built so that a wrong leaf is VISIBLE at the suite's 1e-5 tolerance on
probabilities: within a tree the leaves are a shuffled ``linspace`` (all distinct), and the scale
is chosen so that ``|z| <= 4`` on the fixture's rows, where the sigmoid still has a slope of
0.0177 -- swapping any single leaf for its nearest neighbour moves the probability by at least
``MARGIN = 10 x TOL``."""
import functools

import numpy as np

from ccfd_demo_summit_amd.contracts.metric_names import AMOUNT_BUCKETS
from ccfd_demo_summit_amd.contracts.transaction import AMOUNT_COL, N_FEATURES, amount_bucket
from ccfd_demo_summit_amd.data import generate
from ccfd_demo_summit_amd.models.gbdt import G20_MAX_EDGES, MAX_BINS, BinSpec, ObliviousGBDT

TOL = 1e-5                      # the project's tolerance on GBDT probabilities
MARGIN = 10 * TOL               # smallest probability change of a single swapped leaf
ZMAX = 4.0
CLEAR_FRACTION = 0.99           # rows whose reference is more than TOL from the threshold
DEPTHS = tuple(range(1, 9))
TREES = (1, 3, 5, 8)
ROW_COUNTS = (1, 64, 65, 513, 1025)     # a lane, a chunk, a chunk + 1, a 2nd workgroup at R = 1 / R = 2
SHADOW_SHAPES = ((3, 1), (2, 1), (5, 7))    # (trees, depth): 6- and 4-float champion tables, and a deep one
ORDER_TREES = 8                 # ensembles on which the f32 kernels' summation orders are told apart ...
ORDER_DEPTHS = DEPTHS[1:]       # ... (at depth 1 every leaf is +-a and both orders are exact)
N_BASE = 4                      # generate() rows the edge rows are copies of
_Z_FILL = ZMAX - 0.15           # half range of z the leaves are scaled to ...
_Z_SHIFT = 0.05                 # ... around this offset, so that no sum of +-leaves is exactly 0


@functools.lru_cache(maxsize=None)
def _ref_rows():
    return generate(2000, seed=7)[0]


def _random_splits(trees, depth, rng):
    """Random features, thresholds at random quantiles of generate(2000); split (0, 0) is forced
    to exactly 0.0 (the -0.0 / subnormal rows of edge_rows compare against it)."""
    X = _ref_rows()
    feat = rng.integers(0, N_FEATURES, (trees, depth), dtype=np.int32)
    q = rng.uniform(0.05, 0.95, (trees, depth))
    thr = np.empty((trees, depth), np.float32)
    for t in range(trees):
        for d in range(depth):
            thr[t, d] = np.quantile(X[:, feat[t, d]], q[t, d])
    thr[0, 0] = 0.0
    return feat, thr


def _shuffled_leaves(trees, depth, rng, a=1.0):
    lin = np.linspace(-a, a, 1 << depth)
    return np.stack([rng.permutation(lin) for _ in range(trees)])


def _balanced_leaves(feat, thr, X, rng, tries=16):
    """Unit leaves like _shuffled_leaves, each tree's shuffle the one of ``tries`` random ones that
    keeps the range of the running sum over the rows ``X`` smallest: a narrow range of z leaves
    room for a large leaf scale, i.e. a large gap between neighbouring leaves."""
    T, D = feat.shape
    lin = np.linspace(-1.0, 1.0, 1 << D)
    idx = ObliviousGBDT(feat, thr, np.zeros((T, 1 << D), np.float32), 0.0).leaf_index(X)
    z = np.zeros(X.shape[0])
    out = np.empty((T, 1 << D))
    for t in range(T):
        best = None
        for _ in range(tries):
            perm = rng.permutation(lin)
            cand = z + perm[idx[:, t]]
            width = cand.max() - cand.min()
            if best is None or width < best[0]:
                best = (width, perm, cand)
        out[t], z = best[1], best[2]
    return out


def raw_reference(model, X):
    """float64 sum of the leaves ``model.leaf_index`` selects (+ base)."""
    idx = model.leaf_index(X)
    vals = model.leaves[np.arange(model.n_trees)[None, :], idx].astype(np.float64)
    return float(model.base) + vals.sum(1)


def reference(model, X):
    """float64 probabilities of ``X`` under ``model``."""
    return 1.0 / (1.0 + np.exp(-raw_reference(model, X)))


def _scaled(feat, thr, unit, X):
    """The ensemble with leaves ``a * unit`` and the base that put z of the rows ``X`` into
    [_Z_SHIFT - _Z_FILL, _Z_SHIFT + _Z_FILL]."""
    z = raw_reference(ObliviousGBDT(feat, thr, unit.astype(np.float32), 0.0), X)
    lo, hi = float(z.min()), float(z.max())
    a = _Z_FILL / max((hi - lo) / 2, 1e-9)
    base = float(np.float32(_Z_SHIFT - a * (hi + lo) / 2))
    return ObliviousGBDT(feat, thr, (a * unit).astype(np.float32), base)


def probe_tree(depth, seed=0):
    """One tree, leaves a shuffled linspace(-4, 4, 2^depth), base 0: a row's probability
    identifies its leaf."""
    rng = np.random.default_rng(1000 + 16 * seed + depth)
    feat, thr = _random_splits(1, depth, rng)
    return ObliviousGBDT(feat, thr, _shuffled_leaves(1, depth, rng, ZMAX).astype(np.float32), 0.0)


def shape_ensemble(trees, depth, seed=0):
    """``trees`` x ``depth`` with random splits; per tree the leaves are a shuffled
    linspace(-a, a, 2^depth), with a and the base scaled to the ensemble's own edge_rows."""
    rng = np.random.default_rng(2000 + 1000 * seed + 16 * trees + depth)
    feat, thr = _random_splits(trees, depth, rng)
    X = _edge_matrix(feat, thr, seed)
    return _scaled(feat, thr, _balanced_leaves(feat, thr, X, rng), X)


def _edge_matrix(feat, thr, seed=0):
    base = generate(64, seed=300 + seed)[0][:N_BASE]
    f32 = np.float32
    rows = [r.copy() for r in base]
    state = {"i": 0}

    def add(f, values):
        src = base[state["i"] % N_BASE]
        state["i"] += 1
        for v in values:
            r = src.copy()
            r[f] = v
            rows.append(r)

    T, D = feat.shape
    for t in range(T):
        for d in range(D):
            th = f32(thr[t, d])
            if np.isnan(th):
                continue
            add(int(feat[t, d]), (th, np.nextafter(th, f32(-np.inf)), np.nextafter(th, f32(np.inf))))
    for f in list(dict.fromkeys(int(v) for v in feat.ravel()))[:6]:
        add(f, (f32(np.nan), f32(np.inf), f32(-np.inf)))
    tiny = np.nextafter(f32(0), f32(1))                    # smallest positive subnormal
    for t, d in zip(*np.nonzero(thr == 0)):
        add(int(feat[t, d]), (f32(-0.0), f32(0.0), tiny, -tiny))
    amounts = []
    for b in AMOUNT_BUCKETS:
        b = f32(b)
        amounts += [b, np.nextafter(b, f32(-np.inf)), np.nextafter(b, f32(np.inf))]
    amounts += [f32(0.0), f32(-3.5), f32(np.inf), f32(-np.inf), f32(np.nan)]
    for v in amounts:
        add(AMOUNT_COL, (v,))
    return np.ascontiguousarray(np.stack(rows), np.float32)


def edge_rows(model, seed=0):
    """(X float32 [m, 30], reference float64 [m]): a few generate() rows; for every split a copy
    with the split feature exactly on, one ulp below and one ulp above the threshold; NaN and
    +-inf in split features; -0.0, +0.0 and the smallest subnormals against every threshold that
    is exactly 0; and amounts on, below and above every histogram bound, 0, negative, +-inf, NaN."""
    X = _edge_matrix(model.feat, model.thr, seed)
    return X, reference(model, X)


def min_leaf_swap_delta(model, X):
    """Smallest |change of the probability| over all rows of ``X`` and all trees when the tree's
    chosen leaf is replaced by the leaf nearest in value (= by any other leaf)."""
    z = raw_reference(model, X)
    p = 1.0 / (1.0 + np.exp(-z))
    idx = model.leaf_index(X)
    best = np.inf
    for t in range(model.n_trees):
        lv = model.leaves[t].astype(np.float64)
        srt = np.sort(lv)
        pos = np.searchsorted(srt, lv[idx[:, t]])
        for nb in (pos - 1, pos + 1):
            ok = (nb >= 0) & (nb < srt.size)
            alt = z[ok] - lv[idx[ok, t]] + srt[nb[ok]]
            if alt.size:
                best = min(best, float(np.abs(1.0 / (1.0 + np.exp(-alt)) - p[ok]).min()))
    return best


def f32_sum_orders(model, X):
    """float32 z of ``X`` in the two orders the f32 kernels add the trees: (v1) four partial sums
    over trees w, w + 4, ... added to the base one after the other, (v2) base + the trees added one
    after the other."""
    idx = model.leaf_index(X)
    vals = model.leaves[np.arange(model.n_trees)[None, :], idx]          # float32 [n, T]
    base = np.float32(model.base)
    part = np.zeros((4, X.shape[0]), np.float32)
    acc = np.zeros(X.shape[0], np.float32)
    for t in range(model.n_trees):
        part[t % 4] = part[t % 4] + vals[:, t]
        acc = acc + vals[:, t]
    return (((base + part[0]) + part[1]) + part[2]) + part[3], base + acc


def clear_rows(ref, threshold):
    """Rows whose reference probability is more than TOL away from ``threshold``."""
    return np.abs(np.asarray(ref, np.float64) - float(threshold)) > TOL


def take(m, n):
    """Indices of ``n`` rows out of ``m``: a slice past the base rows when n < m, else the rows
    tiled (every row at least once)."""
    return (np.arange(n) + (N_BASE if n < m else 0)) % m


@functools.lru_cache(maxsize=None)
def shape_case(trees, depth):
    """(model, X, reference) of shape_ensemble(trees, depth) on its edge rows: computed once,
    never modified."""
    m = shape_ensemble(trees, depth)
    X, ref = edge_rows(m)
    X.setflags(write=False)
    ref.setflags(write=False)
    return m, X, ref


@functools.lru_cache(maxsize=None)
def probe_case(depth):
    m = probe_tree(depth)
    X, ref = edge_rows(m)
    X.setflags(write=False)
    ref.setflags(write=False)
    return m, X, ref


@functools.lru_cache(maxsize=None)
def chunked_case():
    """131 x depth 7 = 16768 leaves > the 16384 the f32 v1 kernel keeps in LDS: 128 trees in the
    first leaf chunk, 3 in the second."""
    m = shape_ensemble(131, 7)
    X, ref = edge_rows(m)
    X.setflags(write=False)
    ref.setflags(write=False)
    return m, X, ref


@functools.lru_cache(maxsize=None)
def shadow_case(trees, depth, bits):
    """(A, B, spec, X, refA, refB): champion and challenger of one shape with different splits,
    the union bin table, and the edge rows of both ensembles -- each scaled to all of them."""
    models, mats = [], []
    for seed in (0, 1):
        rng = np.random.default_rng(3000 + 1000 * seed + 16 * trees + depth)
        feat, thr = _random_splits(trees, depth, rng)
        models.append((feat, thr, rng))
        mats.append(_edge_matrix(feat, thr, seed))
    X = np.concatenate(mats)
    A, B = (_scaled(feat, thr, _balanced_leaves(feat, thr, X, rng), X) for feat, thr, rng in models)
    sa, sb = A.bin_spec(), B.bin_spec()
    spec = BinSpec([np.union1d(x, y).astype(np.float32) for x, y in zip(sa.edges, sb.edges)], bits=bits)
    refA, refB = reference(A, X), reference(B, X)
    for a in (X, refA, refB):
        a.setflags(write=False)
    return A, B, spec, X, refA, refB


# --------------------------------------------------------------------------- full bin tables
SWEEP_KS = {8: ((0, 254), (127, 128)), 5: ((0, 30), (15, 16))}


@functools.lru_cache(maxsize=None)
def full_table_spec(bits):
    """A BinSpec with the most edges a row format can index on EVERY feature (255 / 31)."""
    cap = MAX_BINS if bits == 8 else G20_MAX_EDGES
    return BinSpec([np.linspace(-3.0 + 0.01 * j, 3.0 + 0.02 * j, cap).astype(np.float32) for j in range(N_FEATURES)],
                   bits=bits)


def _sweep_bins(cap, ks):
    zero = np.zeros(N_FEATURES, np.int64)
    high = np.full(N_FEATURES, cap, np.int64)
    alt = np.where(np.arange(N_FEATURES) % 2 == 0, 0, cap)
    rows = [zero, high, alt, cap - alt]
    for pattern in (zero, high, alt):
        for k in ks:
            for f in range(N_FEATURES):
                for b in (k, k + 1):
                    r = pattern.copy()
                    r[f] = b
                    rows.append(r)
    return np.stack(rows)


def feature_sweep(spec, ks, seed=0):
    """(model, X, bins, reference): 30 trees of depth 2, tree f testing feature f against edges
    ks[0] and ks[1] of ``spec``; rows with every feature in bin 0, in the highest bin, alternating
    0 / highest, and -- one feature at a time over those patterns -- in bins k and k + 1 for every
    k of the bit width's SWEEP_KS (the same rows for either pair, so the two ensembles can ride as
    champion and challenger).  ``bins`` [m, 30] is what the rows must encode to; a feature in bin
    b sits exactly on edge b (one past the last edge for the highest bin)."""
    cap = MAX_BINS if spec.bits == 8 else G20_MAX_EDGES
    assert all(e.size == cap for e in spec.edges) and len(ks) == 2
    rng = np.random.default_rng(4000 + seed + 64 * spec.bits + ks[0] + 7 * ks[1])
    feat = np.repeat(np.arange(N_FEATURES, dtype=np.int32)[:, None], 2, 1)
    thr = np.stack([np.array([e[ks[0]], e[ks[1]]], np.float32) for e in spec.edges])
    assert tuple(ks) in SWEEP_KS[spec.bits]
    bins = _sweep_bins(cap, [k for pair in SWEEP_KS[spec.bits] for k in pair])
    X = np.empty(bins.shape, np.float32)
    for f, e in enumerate(spec.edges):
        ext = np.append(e, np.float32(e[-1] + 1.0)).astype(np.float32)
        X[:, f] = ext[bins[:, f]]
    m = _scaled(feat, thr, _balanced_leaves(feat, thr, X, rng), X)
    return m, X, bins, reference(m, X)


@functools.lru_cache(maxsize=None)
def sweep_case(bits, which):
    spec = full_table_spec(bits)
    m, X, bins, ref = feature_sweep(spec, SWEEP_KS[bits][which])
    for a in (X, bins, ref):
        a.setflags(write=False)
    return spec, m, X, bins, ref


# --------------------------------------------------------------------------- result checks
def counters_problem(cnt, p, route, X, stale=0):
    """None, or what is wrong with a launch's counters (numpy int array): rows, fraud /
    standard, the proba sum within half a unit per row, and both amount histograms exactly --
    the suite's _check_counters with a NaN amount in bucket 0, as the kernels and the row
    encoders count it."""
    n = len(p)
    route = np.asarray(route)
    if int(cnt[0]) != n:
        return f"incoming {int(cnt[0])} != {n}"
    if int(cnt[1]) != int(route.sum()) or int(cnt[2]) != n - int(route.sum()):
        return f"fraud / standard {int(cnt[1])} / {int(cnt[2])} != {int(route.sum())} / {n - int(route.sum())}"
    fresh = ~np.isnan(p)
    if abs(int(cnt[3]) - int(np.round(p[fresh].astype(np.float64) * 1e6).sum())) > n:
        return f"proba sum {int(cnt[3])}"
    if int(cnt[4]) != stale:
        return f"stale {int(cnt[4])} != {stale}"
    b = amount_bucket(X[:, AMOUNT_COL]).astype(np.int64)
    # a stale row (NaN proba) is standard-routed but enters neither histogram
    if not np.array_equal(cnt[8:22], np.bincount(b[(route == 0) & fresh], minlength=14)):
        return f"standard histogram {cnt[8:22].tolist()}"
    if not np.array_equal(cnt[24:38], np.bincount(b[route == 1], minlength=14)):
        return f"fraud histogram {cnt[24:38].tolist()}"
    return None


def judge(p, route, cnt, ref, X, threshold=0.5):
    """One launch against the reference: {"err": max |p - ref|, "route_mismatch": rows clear of
    the threshold routed unlike ``ref >= threshold``, "clear": their fraction, "counters": None
    or the problem}."""
    clear = clear_rows(ref, threshold)
    want = ref >= threshold
    return {"err": float(np.abs(p.astype(np.float64) - ref).max()),
            "route_mismatch": int((route.astype(bool) != want)[clear].sum()),
            "clear": float(clear.mean()),
            "counters": counters_problem(cnt, p, route, X)}


def assert_judged(j, what=""):
    assert j["clear"] > 0, (what, j)                       # the route check is not vacuous, even at n = 1
    assert j["err"] < TOL, (what, j)
    assert j["route_mismatch"] == 0, (what, j)
    assert j["counters"] is None, (what, j)
