"""The case catalogue of the device rule interpreter (csrc/kernels/rules.h, compiled by
router/rules.py RuleSet.device_program), shared by test_rule_programs_cpu.py,
test_rule_programs_gpu.py, rules_variant_probe.py and test_rules_device.py:

* ``rows``: 273 fixture rows (17 full 16-row tiles and 1 row; 4 full 64-row chunks and 17 rows)
  as an f32 kernel and as a W64 kernel sees them; rows 0..7 share one V5 and one V6 value, so
  ``==``, ``>=`` and ``<=`` against that value have rows exactly on the edge.  No NaN, inf or
  hostile amount is in the rows: non-finite values arise inside the rule arithmetic only;
* ``models``: the CPU models (calibrate_rate 0.2, so that probabilities spread); every constant
  a program compares ``proba`` with is a quantile of the CPU model's predict_proba, never of a
  device output;
* ``feature_catalogue`` / ``proba_catalogue``: the programs (one per feature, packed 48-op
  sweeps, one program per stack depth 5..8, every opcode as a deciding operation, IEEE corners,
  an exact log1p rule, random rule sets);
* ``Interp``: a small postfix interpreter of its own with switchable faults (``MUTANTS``), by
  which test_rule_programs_cpu.py proves that the catalogue notices a subtly wrong interpreter;
* ``launch_problems``: the checks of one launch.  The verdict is ``RuleSet.evaluate`` on the
  kernel's own probabilities and the rows as the kernel saw them (the rules are under test,
  not the model), compared for equality: both sides are round-to-nearest float32.

Importing this module needs numpy only; torch and the native library are imported by the
functions that launch."""
import functools

import numpy as np

from ccfd_demo_summit_amd.contracts.metric_names import AMOUNT_BUCKETS
from ccfd_demo_summit_amd.router import rules as R
from ccfd_demo_summit_amd.router.rules import RuleError, RuleSet, run_device_program

N_ROWS = 273
ROW_COUNTS = (1, 17, 273)
VIEWS = ("f32", "w64")
C5, C6 = 0.375, -1.25                    # bf16-exact: the same edge value on f32 and on W64 rows
EDGE_ROWS = 8
FEATURES = ("Time",) + tuple(f"V{i}" for i in range(1, 29)) + ("amount",)
BOUNDS = np.asarray(AMOUNT_BUCKETS, np.float32)
N_V2 = 262144 + 64 + 9                   # v2's row threshold, one more 64-row chunk and 9 rows


def _lit(v) -> str:
    """A float32 as a literal that parses back to exactly that float32."""
    return repr(float(np.float32(v)))


# --------------------------------------------------------------------------- rows, models
def _with_edges(X):
    X = np.array(X, np.float32)
    X[:EDGE_ROWS, 5] = C5
    X[:EDGE_ROWS, 6] = C6
    return X


def _views(X):
    from ccfd_demo_summit_amd.contracts import decode_wire, encode_wire
    out = {"f32": X, "w64": decode_wire(encode_wire(X))}
    assert np.isfinite(X).all() and (X[:, 29] >= 0).all() and (X[:, 29] < 1e6).all()
    for v in out.values():
        assert (v[:EDGE_ROWS, 5] == np.float32(C5)).all() and (v[:EDGE_ROWS, 6] == np.float32(C6)).all()
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rows():
    """{"f32": X, "w64": decode_wire(encode_wire(X))}: the 273 rows as each kernel sees them."""
    from ccfd_demo_summit_amd.data import generate
    return _views(_with_edges(generate(N_ROWS, seed=41)[0]))


@functools.lru_cache(maxsize=None)
def big_rows():
    """N_V2 rows for the rows-in-registers GBDT kernel (f32 rows only)."""
    from ccfd_demo_summit_amd.data import generate
    X = _with_edges(generate(N_V2, seed=41)[0])
    X.setflags(write=False)
    return X


N_ENGINE = 3 * 256 + 41                  # three full micro-batches of 256 rows and a partial one


@functools.lru_cache(maxsize=None)
def engine_rows():
    """N_ENGINE rows in both views for the streaming engines (the catalogue's constants stay those of
    the 273 rows; the tests assert that both routes still occur)."""
    from ccfd_demo_summit_amd.data import generate
    return _views(_with_edges(generate(N_ENGINE, seed=41)[0]))


@functools.lru_cache(maxsize=None)
def models():
    """CPU models by name.  "gbdt" (60 x depth 6) and "gbdt_d3" keep their leaves in LDS on binned
    rows, "gbdt_gl" (40 x depth 8 = 10240 leaves, past the launch kernel's 8192) gathers them
    from global memory; all three and "forest" have few enough thresholds for G20 rows."""
    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models import TreeEnsemble, build_model
    ref = generate(5000, seed=3)[0]
    m = {"mlp": build_model("mlp", seed=2, X_ref=ref, calibrate_rate=0.2),
         "lr": build_model("lr", seed=3, X_ref=ref, calibrate_rate=0.2),
         "gbdt": build_model("gbdt", seed=4, X_ref=ref, calibrate_rate=0.2, gbdt_trees=60, gbdt_depth=6),
         "gbdt_d3": build_model("gbdt", seed=5, X_ref=ref, calibrate_rate=0.2, gbdt_trees=60, gbdt_depth=3),
         "gbdt_gl": build_model("gbdt", seed=6, X_ref=ref, calibrate_rate=0.2, gbdt_trees=40, gbdt_depth=8),
         "forest": TreeEnsemble.random_init(8, 5, 0.2, 7, ref)}
    assert (m["gbdt"].n_trees << 6) <= 8192 < (m["gbdt_gl"].n_trees << 8)
    for k in ("gbdt", "gbdt_d3", "gbdt_gl", "forest"):
        assert m[k].bin_spec().fits_g20, k
    return m


@functools.lru_cache(maxsize=None)
def cpu_proba(kind, view="f32"):
    """The CPU model's probabilities of the 273 rows: the source of every proba constant."""
    p = np.asarray(models()[kind].predict_proba(rows()[view]), np.float32)
    p.setflags(write=False)
    return p


def _quantiles(p, fracs):
    """float32 quantiles of p that are pairwise distinct and leave rows on both sides."""
    q = [np.float32(np.quantile(p.astype(np.float64), f)) for f in fracs]
    assert len(set(q)) == len(q) and (p > max(q)).any() and (p < min(q)).any(), "degenerate probabilities"
    return q


def _value(expr, X, p):
    """An expression's float32 value per row, to place a constant; never part of a verdict."""
    env = {n: X[:, j] for j, n in enumerate(FEATURES)} if X is not None else {}
    env.update(proba=p, abs=np.abs, min=np.fmin, max=np.fmax)
    with np.errstate(all="ignore"):
        return np.asarray(eval(expr, {"__builtins__": {}}, env), np.float32)     # noqa: S307 (own text)


def _median(v):
    return np.sort(np.asarray(v, np.float32))[len(v) // 2]


# --------------------------------------------------------------------------- random rule sets
RAND_LEAVES = ["proba", "amount", "Time", "V1", "V4", "V10", "V12", "V14", "V17", "V28", "FRAUD_THRESHOLD"]


def rand_expr(rng, depth=0, log1p=True):
    funcs = ["abs", "log1p", "min", "max"] if log1p else ["abs", "min", "max"]
    r = rng.random()
    if depth > 2 or r < 0.3:
        return rng.choice(RAND_LEAVES) if rng.random() < 0.7 else f"{rng.normal() * 3:.4g}"
    if r < 0.45:
        return (f"({rand_expr(rng, depth + 1, log1p)} {rng.choice(['+', '-', '*', '/'])} "
                f"{rand_expr(rng, depth + 1, log1p)})")
    if r < 0.55:
        f = rng.choice(funcs)
        if f in ("min", "max"):
            return f"{f}({rand_expr(rng, depth + 1, log1p)}, {rand_expr(rng, depth + 1, log1p)})"
        return f"{f}({rand_expr(rng, depth + 1, log1p)})"
    if r < 0.65:
        return f"-{rand_expr(rng, depth + 1, log1p)}"
    return (f"{rand_expr(rng, depth + 1, log1p)} {rng.choice(['<', '<=', '>', '>=', '==', '!='])} "
            f"{rand_expr(rng, depth + 1, log1p)}")


def rand_rule(rng, log1p=True):
    parts = [rand_expr(rng, 0, log1p) for _ in range(int(rng.integers(1, 3)))]
    cond = f" {rng.choice(['and', 'or'])} ".join(f"({p}) > 0" if rng.random() < 0.3 else p for p in parts)
    if rng.random() < 0.2:
        cond = f"not ({cond})"
    if rng.random() < 0.15:
        cond = f"-1 < {rng.choice(['V1', 'V2', 'proba'])} < 0.5"
    return cond


N_RANDOM = 40


def _random_sets(p, X):
    """The first N_RANDOM rule sets of a fixed seed (no log1p: libm and the device may differ by
    an ulp) that compile for the device and give both routes on (p, X)."""
    rng = np.random.default_rng(20)
    out = {}
    for _ in range(2000):
        lines = [f"when {rand_rule(rng, log1p=False)} then {rng.choice(['fraud', 'standard'])}"
                 for _ in range(int(rng.integers(1, 4)))]
        lines.append(f"otherwise {rng.choice(['fraud', 'standard'])}")
        rs = RuleSet.parse("\n".join(lines), {"FRAUD_THRESHOLD": 0.5})
        try:
            rs.device_program()
        except RuleError:
            continue
        if 0 < rs.evaluate(p, X=X).sum() < len(p):
            out[f"random{len(out)}"] = rs
            if len(out) == N_RANDOM:
                return out
    raise AssertionError("fewer than N_RANDOM usable random rule sets")


# --------------------------------------------------------------------------- the programs
def _one(cond, route="fraud", default="standard"):
    return f"when {cond} then {route}\notherwise {default}"


SLOT_EXPR = {8: "V1 + (V2 * (V3 - (V4 + (V5 * (V6 - (V7 / V8))))))",
             7: "V2 * (V3 - (V4 + (V5 * (V6 - (V7 / V8)))))",
             6: "V3 - (V4 + (V5 * (V6 - (V7 / V8))))",
             5: "V4 + (V5 * (V6 - (V7 / V8)))"}
SLOT_EXPR_P = {8: "proba + (0.5 * (proba - (0.25 + (proba * (0.75 - (proba / 3))))))",
               7: "0.5 * (proba - (0.25 + (proba * (0.75 - (proba / 3)))))",
               6: "proba - (0.25 + (proba * (0.75 - (proba / 3))))",
               5: "0.25 + (proba * (0.75 - (proba / 3)))"}


def _sweep_vars():
    """36 variables in three groups of 12: all 30 features and proba, then five again."""
    v = list(FEATURES) + ["proba"] + ["V9", "V18", "Time", "amount", "V27"]
    return [v[0:12], v[12:24], v[24:36]]


def _sweep(names, thr):
    """12 rules x 4 ops = MAX_OPS; routes alternate, the default is fraud, so every rule -- the
    last one too -- decides rows and the first match must win."""
    lines = [f"when {n} > {_lit(thr[n])} then {'fraud' if k % 2 == 0 else 'standard'}" for k, n in enumerate(names)]
    return "\n".join(lines + ["otherwise fraud"])


def _texts_feature(X, p):
    """name -> rule text of the feature programs on rows X with CPU probabilities p."""
    t = {}
    col = {n: X[:, j] for j, n in enumerate(FEATURES)}
    col["proba"] = p
    for n in list(FEATURES) + ["proba"]:
        t[f"feature_{n}"] = _one(f"{n} > {_lit(_median(col[n]))}")
    q85 = {n: np.float32(np.quantile(col[n].astype(np.float64), 0.85)) for n in col}
    for k, names in enumerate(_sweep_vars()):
        t[f"sweep{k}"] = _sweep(names, q85)
    t["slots8"] = _one(f"{SLOT_EXPR[8]} > 0.25")
    for d in (7, 6, 5):
        t[f"slots{d}"] = _one(f"{SLOT_EXPR[d]} > {_lit(_median(_value(SLOT_EXPR[d], X, p)))}")
    m = {n: _lit(_median(col[n])) for n in col}
    ops = {
        "min_le_max_neg": _one("min(V1, V2) <= max(V3, -V4)"),
        "not_eq_or_ne": _one(f"not (V5 == {C5}) or V6 != {C6}"),
        "eq_edge": _one(f"V5 == {C5}"),
        "ne_edge": _one(f"V6 != {C6}"),
        "abs_sub_ge": _one("abs(V7) - abs(V8) >= 0"),
        "ge_edge": _one(f"V5 >= {C5}"),
        "gt_edge": _one(f"V5 > {C5}"),
        "le_edge": _one(f"V6 <= {C6}"),
        "lt_edge": _one(f"V6 < {C6}"),
        "ge_feature": _one("V11 >= V13"),
        "le_neg_feature": _one("V15 <= -V16"),
        "not_arith": f"when V10 > {m['V10']} then standard\nwhen not (V9 - V9) then fraud\notherwise standard",
        "not_and": _one(f"not (V18 > {m['V18']} and V19 > {m['V19']})"),
        "chained": _one(f"-0.5 < V11 < 0.5"),
        "unary_plus": _one("+V13 > -(+V15)"),
        "sub_decides": _one(f"V20 - V21 > {_lit(_median(_value('V20 - V21', X, p)))}"),
        "mul_decides": _one(f"V22 * V23 > {_lit(_median(_value('V22 * V23', X, p)))}"),
        "div_decides": _one(f"V24 / V25 > {_lit(_median(_value('V24 / V25', X, p)))}"),
        "add_decides": _one(f"(V10 + V12) / 2 < {_lit(_median(_value('(V10 + V12) / 2', X, p)))}"),
        # an arithmetic opcode as the last operation before END: its value is the condition
        "bare_add": _one("(V23 > 0) + (V24 > 0)"),
        "bare_sub": _one("(V21 > 0) - (V22 > 0)"),
        "bare_mul": _one("(V19 > 0) * (V20 > 0)"),
        "bare_div": _one("(V25 > 0) / (V26 > 0)", default="standard"),      # 0/0 = NaN and 1/0 = inf match
        "bare_neg": _one("-(V27 > 0)"),
        "bare_abs": _one(f"abs((V28 > 0) - (Time > {m['Time']}))"),
        "bare_min": _one("min(V3 > 0, V4 > 0)"),
        "bare_max": _one("max(V7 > 0, V8 > 0)"),
        "bare_log1p": _one("log1p(V26 > 0)"),              # log1p(1) != 0 and log1p(0) == 0 whatever the ulp
        "and_or": _one(f"V14 > 0 and V17 > 0 or amount > {m['amount']} and proba > {m['proba']}"),
        "default_fraud": _one(f"V12 > {m['V12']}", route="standard", default="fraud"),
    }
    t.update(ops)
    ieee = {
        "ieee_div_zero": _one("V1 / (V2 - V2) > 0"),                         # +-inf
        "ieee_nan_matches": f"when V3 > {m['V3']} then standard\nwhen (V3 / 0) - (V3 / 0) then fraud\n"
                            "otherwise standard",                             # inf - inf = NaN != 0
        "ieee_overflow": f"when amount * 3e38 * 3e38 > 1e38 and V4 > {m['V4']} then fraud\notherwise standard",
        "ieee_denormal_gt": _one("V1 * 1e-38 * 1e-5 > 0"),
        "ieee_denormal_ne": f"when V2 * 1e-38 * 1e-5 != 0 and V2 > {m['V2']} then fraud\notherwise standard",
        "ieee_mix": "when V1 / (V2 - V2) > 0 and V3 > 0 then fraud\n"
                    "when amount * 3e38 * 3e38 > 1e38 and V4 > 0 then standard\n"
                    "when V6 * 1e-38 * 1e-5 > 0 then fraud\n"
                    "when (V7 / 0) - (V7 / 0) then standard\n"
                    "otherwise fraud",
    }
    t.update(ieee)
    t["log1p_exact"] = _one(f"log1p(max(amount, 0)) > {_lit(_log1p_constant(X[:, 29]))}")
    return t


def _log1p_constant(amount):
    """The midpoint of the widest gap between adjacent float64 log1p values of the middle half
    of the rows' amounts; every row is more than 16 float32 ulp from it, so that a last-bit
    difference between libm and the device log1pf cannot move a row across: no row is excused."""
    v = np.sort(np.log1p(np.maximum(amount.astype(np.float64), 0)))
    mid = v[len(v) // 4: 3 * len(v) // 4]
    i = int(np.argmax(np.diff(mid)))
    c = np.float32((mid[i] + mid[i + 1]) / 2)
    assert (np.abs(v - np.float64(c)) > 16 * np.spacing(c)).all()
    return c


def _texts_proba(p):
    """name -> rule text of the proba-only programs (all that binned rows can route by): twins
    of the opcode, slot, length and IEEE programs."""
    q = dict(zip((5, 10, 15, 20, 25, 30, 40, 50, 60, 70, 75, 80, 85, 90, 95),
                 (_lit(v) for v in _quantiles(p, [f / 100 for f in (5, 10, 15, 20, 25, 30, 40, 50, 60, 70, 75, 80,
                                                                   85, 90, 95)]))))
    t = {"feature_proba": _one(f"proba > {q[50]}")}
    order = (95, 90, 85, 80, 70, 60)
    lines = [f"when proba > {q[f]} then {'fraud' if k % 2 == 0 else 'standard'}" for k, f in enumerate(order)]
    lines += [f"when proba < {q[f]} then {'fraud' if k % 2 == 0 else 'standard'}"
              for k, f in enumerate((5, 10, 15, 20, 30, 40))]
    t["sweep_p"] = "\n".join(lines + ["otherwise fraud"])                    # 12 x 4 = MAX_OPS
    for d in (8, 7, 6, 5):
        t[f"slots{d}_p"] = _one(f"{SLOT_EXPR_P[d]} > {_lit(_median(_value(SLOT_EXPR_P[d], None, p)))}")
    t.update({
        "min_le_max_neg_p": _one(f"min(proba, 1 - proba) <= max({q[25]}, -proba)"),
        "eq_p": _one(f"(proba > {q[50]}) == (proba > {q[25]})"),
        "ne_p": _one(f"(proba > {q[75]}) != (proba > {q[40]})"),
        "not_or_p": _one(f"not (proba > {q[30]}) or proba > {q[70]}"),
        "abs_sub_ge_p": _one(f"abs(proba - {q[50]}) - abs(proba - {q[75]}) >= 0"),
        # against a probability the CPU model gives a row: that row is on the edge
        "ge_p": _one(f"proba >= {_lit(np.sort(p)[int(0.6 * len(p))])}"),
        "le_p": _one(f"proba <= {_lit(np.sort(p)[int(0.4 * len(p))])}"),
        "lt_p": _one(f"proba < {q[40]}"),
        "ge_neg_p": _one(f"-proba >= -{q[30]}"),
        "not_arith_p": f"when proba > {q[50]} then standard\nwhen not (proba - proba) then fraud\notherwise standard",
        "chained_p": _one(f"{q[25]} < proba < {q[75]}"),
        "unary_plus_p": _one(f"+proba > +{q[60]}"),
        "mul_div_p": _one(f"proba * proba / (1 - proba) > {_lit(_median(_value('proba * proba / (1 - proba)', None, p)))}"),
        "bare_sub_p": _one(f"(proba > {q[25]}) - (proba > {q[75]})"),
        "bare_mul_p": _one(f"(proba > {q[25]}) * (proba < {q[75]})"),
        "bare_div_p": _one(f"(proba > {q[60]}) / (proba > {q[30]})"),
        "bare_add_p": _one(f"(proba > {q[80]}) + (proba < {q[20]})"),
        "bare_neg_p": _one(f"-(proba > {q[50]})"),
        "bare_abs_p": _one(f"abs((proba > {q[40]}) - 1)"),
        "bare_min_p": _one(f"min(proba > {q[20]}, proba < {q[60]})"),
        "bare_max_p": _one(f"max(proba > {q[80]}, proba < {q[40]})"),
        "bare_log1p_p": _one(f"log1p(proba > {q[50]})"),
        "and_or_p": _one(f"proba > {q[20]} and proba < {q[40]} or proba > {q[80]}"),
        "default_fraud_p": _one(f"proba > {q[50]}", route="standard", default="fraud"),
        "ieee_mix_p": f"when proba / (proba - proba) > 0 and proba > {q[75]} then fraud\n"
                      f"when proba * 3e38 * 3e38 > 1e38 and proba > {q[50]} then standard\n"
                      f"when (proba - 1) * 1e-38 * 1e-5 < 0 and proba > {q[25]} then fraud\n"
                      "when (proba / 0) - (proba / 0) then standard\n"
                      "otherwise fraud",
        "ieee_denormal_p": f"when proba * 1e-38 * 1e-5 != 0 and proba > {q[50]} then fraud\notherwise standard",
    })
    return t


def _parse(texts):
    return {k: RuleSet.parse(v) for k, v in texts.items()}


@functools.lru_cache(maxsize=None)
def feature_catalogue(kind, view):
    """name -> RuleSet: the feature programs for a model kind on a row view ("f32" / "w64")."""
    X, p = rows()[view], cpu_proba(kind, view)
    out = _parse(_texts_feature(X, p))
    out.update(_random_sets(p, X))
    return out


@functools.lru_cache(maxsize=None)
def proba_catalogue(kind):
    """name -> RuleSet: the proba-only programs for a model kind (binned rows)."""
    out = _parse(_texts_proba(cpu_proba(kind)))
    assert not any(rs.feature_vars() for rs in out.values())
    return out


SWEEPS = ("sweep0", "sweep1", "sweep2")
ENGINE_PROGRAMS = SWEEPS + ("slots8", "ieee_mix")
ENGINE_PROGRAMS_P = ("sweep_p", "slots8_p", "ieee_mix_p")
V2_BIG_PROGRAMS = SWEEPS + ("slots8",)
STALE_PROGRAM = "default_fraud_p"


# --------------------------------------------------------------------------- program facts
ARITH = (R.OP_ADD, R.OP_SUB, R.OP_MUL, R.OP_DIV, R.OP_NEG, R.OP_ABS, R.OP_LOG1P, R.OP_MIN, R.OP_MAX)
COMPARE = (R.OP_GT, R.OP_GE, R.OP_LT, R.OP_LE, R.OP_EQ, R.OP_NE)
ALL_OPCODES = ARITH + COMPARE + (R.OP_AND, R.OP_OR, R.OP_NOT)


def program_ops(prog):
    head = np.frombuffer(prog, np.int32, 4)
    return head, np.frombuffer(prog, R.PROG_DTYPE, R.MAX_OPS, 16)[:int(head[0])].tolist()


def program_facts(prog):
    """(n_ops, stack depth reached, feature indices read, deciding opcodes).  A rule's deciding
    operations: the one before its END; when that is a comparison, also the arithmetic operation
    that produced the comparison's left or right operand directly."""
    head, ops = program_ops(prog)
    sp = top = 0
    feats, deciding = set(), set()
    for i, (op, arg, _) in enumerate(ops):
        if op in (R.OP_VAR, R.OP_CONST):
            sp += 1
            if op == R.OP_VAR and arg:
                feats.add(arg - 1)
        elif op == R.OP_END:
            sp -= 1
            deciding.add(ops[i - 1][0])
            if ops[i - 1][0] in COMPARE:
                k = i - 2
                if ops[k][0] in ARITH:
                    deciding.add(ops[k][0])                     # the right operand
                if ops[k][0] in (R.OP_VAR, R.OP_CONST) and ops[k - 1][0] in ARITH:
                    deciding.add(ops[k - 1][0])                 # the left operand, before a leaf
        elif op not in (R.OP_NEG, R.OP_ABS, R.OP_LOG1P, R.OP_NOT):
            sp -= 1
        top = max(top, sp)
    assert top == head[3] and sp == 0
    return len(ops), top, feats, deciding - {R.OP_VAR, R.OP_CONST}


# --------------------------------------------------------------------------- mutable interpreter
_SWAPPABLE = {"SUB": R.OP_SUB, "DIV": R.OP_DIV, "LT": R.OP_LT, "GT": R.OP_GT, "LE": R.OP_LE, "GE": R.OP_GE}
MUTANTS = ([f"pop_slot{k}" for k in (4, 5, 6, 7)] + [f"push_slot{k}" for k in (4, 5, 6, 7)] +
           [f"swap_{n}" for n in _SWAPPABLE] +
           ["ge_as_gt", "le_as_lt", "eq_as_ne", "min_as_max", "and_as_or", "not_as_truth", "neg_dropped",
            "abs_dropped", "last_match_wins", "default_flipped", "truncated_47", "feature_plus_1",
            "feature_minus_1", "w64_time_amount_exchanged", "f32_group3_from_group2", "mul_flushes_denormals"])
VIEW_MUTANTS = {"w64_time_amount_exchanged": "w64", "f32_group3_from_group2": "f32"}

_TINY = np.float32(np.finfo(np.float32).tiny)
_ONE, _ZERO = np.float32(1), np.float32(0)


class Interp:
    """A postfix interpreter of ccfd_rule_prog with the structure of csrc/kernels/rules.h (eight
    stack slots addressed by a uniform stack pointer; feature j gathered from a lane group and a
    slot) and the semantics of run_device_program, vectorised over the rows.  ``mutant`` (one
    of MUTANTS, or None) switches one fault on.  Its own code: no product code is changed."""

    def __init__(self, view, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.view, self.m = view, mutant

    # the stack -------------------------------------------------------------------------
    def _push(self, v):
        k = self.sp
        if self.m == f"push_slot{k}":
            k -= 1
        self.slots[k] = v
        self.sp += 1

    def _pop(self):
        self.sp -= 1
        k = self.sp
        if self.m == f"pop_slot{k}":
            k -= 1
        return self.slots[k]

    # the gather ------------------------------------------------------------------------
    def _feature(self, X, j):
        if self.m == "feature_plus_1":
            j = (j + 1) % 30
        elif self.m == "feature_minus_1":
            j = (j - 1) % 30
        if self.view == "w64":
            # wire order V1..V28, Time, Amount: 8 features a lane group
            pos = 28 if j == 0 else 29 if j == 29 else j - 1
            if self.m == "w64_time_amount_exchanged" and pos >= 28:
                pos = 57 - pos
            wire = np.concatenate([X[:, 1:29], X[:, 0:1], X[:, 29:30]], axis=1)
            return wire[:, pos]
        group, slot = j >> 3, j & 7
        if self.m == "f32_group3_from_group2" and group == 3:
            group = 2
        return X[:, group * 8 + slot]

    # the program -----------------------------------------------------------------------
    def run(self, prog, proba, X):
        head, ops = program_ops(prog)
        proba = np.asarray(proba, np.float32).reshape(-1)
        X = np.asarray(X, np.float32)
        n = len(proba)
        self.slots, self.sp = [np.zeros(n, np.float32) for _ in range(8)], 0
        default = int(head[1]) != 0
        if self.m == "default_flipped":
            default = not default
        if self.m == "truncated_47":
            ops = ops[:47]
        decided = np.zeros(n, bool)
        fraud = np.full(n, default)
        m = self.m
        with np.errstate(all="ignore"):
            for op, arg, imm in ops:
                if op == R.OP_VAR:
                    self._push(proba if arg == 0 else self._feature(X, arg - 1))
                elif op == R.OP_CONST:
                    self._push(np.full(n, np.float32(imm)))
                elif op == R.OP_END:
                    cond = self._pop() != 0
                    take = cond if m == "last_match_wins" else cond & ~decided
                    fraud = np.where(take, arg != 0, fraud)
                    decided |= cond
                elif op in (R.OP_NEG, R.OP_ABS, R.OP_LOG1P, R.OP_NOT):
                    a = self._pop()
                    if op == R.OP_NEG:
                        r = a if m == "neg_dropped" else -a
                    elif op == R.OP_ABS:
                        r = a if m == "abs_dropped" else np.abs(a)
                    elif op == R.OP_LOG1P:
                        r = np.log1p(a)
                    else:
                        r = np.where((a != 0) if m == "not_as_truth" else (a == 0), _ONE, _ZERO)
                    self._push(np.asarray(r, np.float32))
                else:
                    b = self._pop()
                    a = self._pop()
                    if m is not None and m.startswith("swap_") and _SWAPPABLE[m[5:]] == op:
                        a, b = b, a
                    if m == "ge_as_gt" and op == R.OP_GE:
                        op = R.OP_GT
                    elif m == "le_as_lt" and op == R.OP_LE:
                        op = R.OP_LT
                    elif m == "eq_as_ne" and op == R.OP_EQ:
                        op = R.OP_NE
                    elif m == "min_as_max" and op == R.OP_MIN:
                        op = R.OP_MAX
                    elif m == "and_as_or" and op == R.OP_AND:
                        op = R.OP_OR
                    if op == R.OP_ADD:
                        r = a + b
                    elif op == R.OP_SUB:
                        r = a - b
                    elif op == R.OP_MUL:
                        r = a * b
                        if m == "mul_flushes_denormals":
                            r = np.where(np.abs(r) < _TINY, np.copysign(_ZERO, r), r)
                    elif op == R.OP_DIV:
                        r = a / b
                    elif op == R.OP_MIN:
                        r = np.fmin(a, b)
                    elif op == R.OP_MAX:
                        r = np.fmax(a, b)
                    else:
                        r = {R.OP_GT: lambda: a > b, R.OP_GE: lambda: a >= b, R.OP_LT: lambda: a < b,
                             R.OP_LE: lambda: a <= b, R.OP_EQ: lambda: a == b, R.OP_NE: lambda: a != b,
                             R.OP_AND: lambda: (a != 0) & (b != 0), R.OP_OR: lambda: (a != 0) | (b != 0)}[op]()
                        r = np.where(r, _ONE, _ZERO)
                    self._push(np.asarray(r, np.float32))
        assert self.sp == 0 or m == "truncated_47"
        return fraud.astype(np.uint8)


# --------------------------------------------------------------------------- judging a launch
def want_routes(rs, p, X_seen):
    """The verdict: RuleSet.evaluate on the kernel's own probabilities; the host emulator of the
    device program must agree with it first (a precondition, not the check)."""
    want = rs.evaluate(p, X=X_seen)
    np.testing.assert_array_equal(run_device_program(rs.device_program(), p, X_seen), want)
    return want


def launch_problems(rs, p, r, c, X_seen, amount, flagged=None, stale=None):
    """The failures of one launch (a list of strings; empty: passed).  p, r: the kernel's
    probability and route per row; c: its counters; X_seen: the rows as the kernel saw them
    (None for binned rows); amount: the rows' amounts; flagged: the flag list as row indices
    (None: the path has none); stale: a bool mask of rows whose stamp is another table's."""
    n = len(p)
    bad = []
    fresh = np.ones(n, bool) if stale is None else ~stale
    want = np.zeros(n, np.uint8)
    want[fresh] = want_routes(rs, p[fresh], None if X_seen is None else X_seen[fresh])
    diff = np.flatnonzero(np.asarray(r) != want)
    if diff.size:
        bad.append(f"{diff.size} routes differ from evaluate, first rows {diff[:8].tolist()}")
    if stale is not None:
        if not np.isnan(p[stale]).all() or np.isnan(p[fresh]).any():
            bad.append("NaN probabilities are not exactly the stale rows")
        if int(c[4]) != int(stale.sum()):
            bad.append(f"stale counter {int(c[4])}, stale rows {int(stale.sum())}")
    fraud = np.asarray(r) != 0
    nf = int(fraud.sum())
    if [int(c[0]), int(c[1]), int(c[2])] != [n, nf, n - nf]:
        bad.append(f"counters {[int(c[0]), int(c[1]), int(c[2])]} for {n} rows, {nf} fraud")
    bk = np.searchsorted(BOUNDS, np.asarray(amount, np.float32), side="left")
    # a stale row is counted as incoming, stale and standard, and enters neither amount histogram
    if not np.array_equal(c[8:22], np.bincount(bk[~fraud & fresh], minlength=14)):
        bad.append(f"standard amount histogram {np.asarray(c[8:22]).tolist()}")
    if not np.array_equal(c[24:38], np.bincount(bk[fraud], minlength=14)):
        bad.append("fraud amount histogram")
    if flagged is not None:
        flagged = np.asarray(flagged, np.int64)
        if len(np.unique(flagged)) != len(flagged) or not np.array_equal(np.sort(flagged), np.flatnonzero(fraud)):
            bad.append(f"flag list of {len(flagged)} rows is not the {nf} fraud rows, each once")
    return bad
