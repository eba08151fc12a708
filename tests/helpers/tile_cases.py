"""Shared cases of the MLP / LR tile kernels (score_mlp.hip, score_lr.hip, wire_body.h):

* the bucket-bound fixture of test_tile_epilogue_gpu.py (rows, both models, each model's oracle,
  ``check`` and ``engine_case``);
* a block of hostile rows that is never compared with a tolerance (``hostile_rows``);
* ``plan``: a CPU model of the launch arithmetic, used ONLY to choose row counts -- it decides
  inputs and never a verdict (test_mlp_variants_cpu.py proves what the chosen counts reach);
* the env-knob configurations of test_mlp_variants_gpu.py, the list of cases each of them scores
  and ``Runner``, which the child process (mlp_variant_probe.py) runs under the knobs and the
  parent without them; ``judge`` turns a case's figures into a verdict (the parent's).

Importing this module needs numpy only; torch and the native library are imported by the
functions that launch."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from ccfd_demo_summit_amd.contracts.metric_names import AMOUNT_BUCKETS

# --------------------------------------------------------------------------- bucket-bound rows
BOUNDS = np.asarray(AMOUNT_BUCKETS, np.float32)
EDGE_AMOUNTS = np.concatenate([[np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(np.inf))]
                               for b in BOUNDS] + [[np.float32(0)]]).astype(np.float32)
N_PERSIST = 2 * 4096 + 999          # 2 full batches, then a partial item and a partial 16-row tile


@functools.lru_cache(maxsize=None)
def build_setup():
    """Rows whose amounts cycle through EDGE_AMOUNTS, both models, and each model's oracle on
    f32 and on W64 rows -- computed once, read-only."""
    from ccfd_demo_summit_amd.contracts import decode_wire, encode_wire
    from ccfd_demo_summit_amd.data import generate
    from ccfd_demo_summit_amd.models import build_model
    X, _ = generate(N_PERSIST + 41, seed=23)
    X[:, 29] = EDGE_AMOUNTS[np.arange(X.shape[0]) % len(EDGE_AMOUNTS)]
    Xd = decode_wire(encode_wire(X))
    models = {"mlp": build_model("mlp", seed=4, X_ref=X, calibrate_rate=0.05),
              "lr": build_model("lr", seed=5, X_ref=X, calibrate_rate=0.05)}
    ref = {("mlp", False): models["mlp"].predict_proba(X, emulate_bf16=True),
           ("mlp", True): models["mlp"].wire_proba(X),
           ("lr", False): models["lr"].predict_proba(X),
           ("lr", True): models["lr"].predict_proba(Xd)}
    for v in ref.values():
        v.setflags(write=False)
    X.setflags(write=False)
    return X, models, ref


@functools.lru_cache(maxsize=None)
def extras():
    """What the variant cases need beside build_setup(): the rows as a W64 kernel sees them (the
    features RuleSet.evaluate gets for W64 launches) and the fp32 MLP oracle."""
    from ccfd_demo_summit_amd.contracts import decode_wire, encode_wire
    X, models, _ = build_setup()
    Xd = decode_wire(encode_wire(X))
    p32 = models["mlp"].predict_proba(X)
    Xd.setflags(write=False)
    p32.setflags(write=False)
    return Xd, p32


def check(c, amount, ref, fraud, flagged_rows, what):
    """Counters `c` of rows with amounts `amount` and oracle proba `ref`; `fraud`: the device's
    own route per row; `flagged_rows`: the flag list as row indices (None: not read)."""
    n = len(amount)
    nf = int(fraud.sum())
    want = float(np.round(ref.astype(np.float64) * 1e6).sum())
    print(f"{what}: n={n} fraud={nf} psum={int(c[3])} oracle={want:.0f} bound={2e-4 * n * 1e6 / 100:.0f}")
    if flagged_rows is not None:
        assert len(np.unique(flagged_rows)) == len(flagged_rows)          # no row flagged twice
        np.testing.assert_array_equal(np.sort(flagged_rows), np.flatnonzero(fraud))
    assert c[0] == n and c[1] == nf and c[2] == n - nf
    bk = np.searchsorted(BOUNDS, amount, side="left")
    np.testing.assert_array_equal(c[8:22], np.bincount(bk[~fraud], minlength=14))
    np.testing.assert_array_equal(c[24:38], np.bincount(bk[fraud], minlength=14))
    assert abs(int(c[3]) - want) < 2e-4 * n * 1e6 / 100


def engine_case(gpu, setup, kind, wire, n_rows, pumps, **kw):
    """One engine over the first `n_rows` rows: pump, then the epoch's counters against the
    scored-record ring (device proba / route per row) and the flag list.  Returns the device's
    (proba, route != 0) by row."""
    import torch
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    X, models, ref = setup
    eng = StreamEngine(DeviceModel(models[kind], gpu, wire=wire), input_mode="zerocopy", **kw)
    eng.enable_scored(n_rows + 64)
    log = PartitionLog.from_arrays(X[:n_rows], ids=np.arange(n_rows, dtype=np.uint64) + 1000, wire=wire)
    eng.add_log(0, log)
    rows = sum(eng.pump(k, batch_rows=b, drain=True).rows for k, b in pumps)
    assert rows == n_rows
    flagged = eng.drain_flagged()
    rec = eng.drain_scored()
    side = torch.cuda.Stream(gpu)
    c = eng.flip_epoch(side)
    side.synchronize()
    c = c.cpu().numpy()
    eng.close()
    log.free()
    ids = (rec["tx_id"] - 1000).astype(np.int64)
    np.testing.assert_array_equal(np.sort(ids), np.arange(n_rows))           # every row scored once
    fraud = np.zeros(n_rows, bool)
    fraud[ids] = rec["route"] != 0
    proba = np.zeros(n_rows, np.float32)
    proba[ids] = rec["proba"]
    check(c, X[:n_rows, 29], ref[(kind, wire)][:n_rows], fraud, (flagged["tx_id"] - 1000).astype(np.int64),
          f"{kind} wire={wire} {kw}")
    return proba, fraud


# --------------------------------------------------------------------------- hostile rows
HOSTILE_AMOUNTS = np.asarray([-5, 1e-3, 1e7, 3e38], np.float32)
HOSTILE_TIMES = np.asarray([0, 1e6], np.float32)
HOSTILE_ROWS = 4128                     # >= the largest row count row_counts() can choose


@functools.lru_cache(maxsize=None)
def hostile_rows():
    """Fixture rows with every pair of a HOSTILE_AMOUNTS amount and a HOSTILE_TIMES time.  No
    numerics oracle is established on them (not for the default kernels either): they are judged
    only by 0 <= p <= 1 and finite, route == (p >= threshold), the exact amount bucket, the
    counters, and identity to the default variant."""
    X = build_setup()[0]
    H = X[:HOSTILE_ROWS].copy()
    i = np.arange(len(H))
    H[:, 29] = HOSTILE_AMOUNTS[i % 4]
    H[:, 0] = HOSTILE_TIMES[(i // 4) % 2]
    H.setflags(write=False)
    return H


# --------------------------------------------------------------------------- knobs, configurations
KNOBS = ("CCFD_MLP_WAVES", "CCFD_MLP_PF", "CCFD_MLP_REGW", "CCFD_MLP_TPW", "CCFD_MLP_WEIGHTS",
         "CCFD_LR_WAVES", "CCFD_LR_PF", "CCFD_LR_OCC")
KINDS = ("mlp", "lr")
FORMATS = ("f32", "f32s", "w64")        # contiguous f32 rows, f32 rows with ld = 32, W64 rows
TILE = 16
BIG_N = 65589                           # 4100 tiles: past every grid cap of configuration 1


def _config(waves, pf, regw, tpw, weights, lr_waves, lr_pf, lr_occ, big=False):
    env = dict(zip(KNOBS, (str(v) for v in (waves, pf, regw, tpw, weights, lr_waves, lr_pf, lr_occ))))
    return {"env": env, "big": big}


# One child process each.  The MLP columns and CCFD_MLP_TPW pair every waves-per-workgroup value
# with a prefetch depth it can fill (a wave gets at most TPW tiles unless the grid is capped, so
# a tail of PF-1 tiles needs TPW >= PF-1 and a steady round TPW >= PF); the LR columns are the
# full 3 x 3 of CCFD_LR_WAVES x CCFD_LR_PF, PF 2 on the TPW 1 / 2 rows, 4 on the TPW 4 rows, 8 on
# the TPW 8 rows, for the same reason.  Configurations 1 and 2 also score BIG_N rows: in 1 the
# grid caps of all four row paths are exceeded (grid-stride loop), in 2 the register-weight
# kernel's 2048-workgroup cap.
CONFIGS = {
    1: _config(1, 1, 0, 1, "global", 4, 2, 4, big=True),
    2: _config(1, 2, 1, 1, "lds", 8, 2, 8, big=True),
    3: _config(2, 2, 0, 2, "lds", 16, 2, 4),
    4: _config(4, 4, 0, 4, "global", 4, 4, 8),      # quad epilogue on the LDS scorer; coalesced PF=4
    5: _config(16, 4, 0, 8, "lds", 8, 8, 4),        # 16-wave groups
    6: _config(8, 1, 0, 8, "lds", 16, 8, 8),        # scalar loop; coalesced PF=1
    7: _config(2, 4, 1, 4, "global", 8, 4, 4),
    8: _config(4, 2, 1, 4, "lds", 16, 4, 4),
    9: _config(8, 2, 1, 8, "lds", 4, 8, 8),         # reg<8,2>
}


# --------------------------------------------------------------------------- launch arithmetic
Plan = namedtuple("Plan", "kernel waves pf grid ntiles tiles rounds tail partial")
Plan.__doc__ = """What a launch of n rows does, restated from launch_mlp_t / launch_w / launch_wire,
launch_lr_t / launch_lr_w, the coalesced launches and the ring of wire_stream_body:
kernel   "mlp_wire_reg", "mlp_wire", "lr_wire" (W64 rows) or "mlp_f32", "lr_f32"
waves    waves per workgroup
pf       effective tiles in flight per wave (W64), 1 on f32 rows (the one-tile prefetch)
grid     workgroups after the cap (of one sub-batch for a coalesced launch)
ntiles   16-row tiles of the launch
tiles    per wave (grid * waves of them): tiles it scores
rounds   per wave: steady rounds of pf tiles (W64 rows; 0 on f32 rows)
tail     per wave: tiles left to the tail loop (W64 rows; 0 on f32 rows)
partial  where the partial last tile is scored: "steady", "tail", "loop" (f32 rows), None if n % 16 == 0"""


def _int_knob(env, name, allowed, default):
    """atoi of the variable when it is one of `allowed`, else `default` (as the launch code reads it)."""
    try:
        v = int(env.get(name, ""))
    except ValueError:
        return default
    return v if v in allowed else default


def plan(kind, fmt, env, n, coalesced=False):
    """The Plan of `n` rows of format `fmt` scored by model `kind` under the knobs `env` (a dict
    of the variables that are set); coalesced: `n` is the sub-batch of a coalesced launch."""
    wire = fmt == "w64"
    ntiles = (n + TILE - 1) // TILE
    tpw = _int_knob(env, "CCFD_MLP_TPW", (1, 2, 4, 8), 8)            # also sizes the LR grids
    forced_waves = _int_knob(env, "CCFD_MLP_WAVES", (1, 2, 4, 8, 16), 0)
    forced_pf = _int_knob(env, "CCFD_MLP_PF", (1, 2, 4), 0)
    regw = "CCFD_MLP_REGW" not in env or _int_knob(env, "CCFD_MLP_REGW", (0,), 1) != 0
    if coalesced:
        kw = 4
        grid = (n + TILE * kw * tpw - 1) // (TILE * kw * tpw)         # no cap
        if not wire:
            kernel, pf = kind + "_f32", 1
        elif kind == "mlp":
            kernel, pf = "mlp_wire", forced_pf or 2                   # LDS weights only
        else:
            kernel, pf = "lr_wire", 4                                 # <4, 4> only
    elif not wire:
        # launch_mlp_t / launch_lr_t: 1 and 2 as asked, everything else (4, 8, 16, unset) is 4
        kw = forced_waves if forced_waves in (1, 2) else 4
        cap = 256 * 16 // kw if kind == "mlp" else 2048
        grid = min(max((ntiles + kw * tpw - 1) // (kw * tpw), 1), cap)
        kernel, pf = kind + "_f32", 1
    elif kind == "mlp":
        kw = (forced_waves or 4) if "CCFD_MLP_WAVES" in env else 8
        grid = min(max((ntiles + kw * tpw - 1) // (kw * tpw), 1), 256 * 16 // kw)
        if kw <= 8 and regw:                                          # 16 waves never take register weights
            grid = min(grid, 256 * 8 // kw)
            kernel, pf = "mlp_wire_reg", 4 if forced_pf in (0, 4) else 2      # a forced 1 means 2
        else:
            kernel, pf = "mlp_wire", forced_pf or 2
    else:
        kw = _int_knob(env, "CCFD_LR_WAVES", (4, 8, 16), 16)
        occ = _int_knob(env, "CCFD_LR_OCC", (4, 8), 4)
        grid = min(max((ntiles + kw * tpw - 1) // (kw * tpw), 1), 256 * 4 * occ // kw)
        kernel, pf = "lr_wire", _int_knob(env, "CCFD_LR_PF", (2, 4, 8), 4)
    tstride = grid * kw
    v = np.arange(tstride)
    tiles = np.maximum(0, (ntiles - v + tstride - 1) // tstride)
    if wire:
        full_end = ntiles - (pf - 1) * tstride
        rounds = np.where(v < full_end, (full_end - v + pf * tstride - 1) // (pf * tstride), 0)
        tail = tiles - rounds * pf
    else:
        rounds = tail = np.zeros(tstride, np.int64)
    partial = None
    if n % TILE:
        last = ntiles - 1
        partial = "loop" if not wire else "steady" if last // tstride < rounds[last % tstride] * pf else "tail"
    return Plan(kernel, kw, pf, grid, ntiles, tiles, rounds, tail, partial)


_CANDIDATES = tuple(16 * k + 9 for k in range(257))          # a partial last tile of 9 rows


def _first(pred):
    return next((n for n in _CANDIDATES if pred(n)), None)


def row_counts(env, kind, fmt):
    """Row counts of the plain launches of one (model, row format) under `env`: 1, 64 (no partial
    tile), 9 (a one-tile wave; the partial tile in the tail) and the first n = 16k + 9 <= 4105 at
    which plan() shows each of: a tail of every length 1 .. pf-1, a steady round that holds the
    partial last tile, a steady round followed by a tail, two steady rounds in one wave (W64
    rows); a wave with two tiles (f32 rows).  What no n <= 4105 reaches is
    left to BIG_N (test_mlp_variants_cpu.py says which those are)."""
    out = {1, 9, 64}
    pf = plan(kind, fmt, env, 9).pf
    if fmt == "w64":
        for length in range(1, pf):
            out.add(_first(lambda n: (plan(kind, fmt, env, n).tail == length).any()))
        out.add(_first(lambda n: plan(kind, fmt, env, n).partial == "steady"))
        # the slots a steady round refills are consumed only by what follows it
        out.add(_first(lambda n: (lambda p: ((p.rounds >= 1) & (p.tail >= 1)).any())(plan(kind, fmt, env, n))))
        out.add(_first(lambda n: plan(kind, fmt, env, n).rounds.max() >= 2))
    else:
        out.add(_first(lambda n: plan(kind, fmt, env, n).tiles.max() >= 2))
    return sorted(n for n in out if n is not None)


def engine_rows(env, kind, fmt, mode="engine4"):
    """Rows of one micro-batch of the engine launches: the first n = 16k + 9 at which a wave of
    the coalesced sub-batch has a steady round (TPW >= the coalesced PF), else 137.  The all-fraud
    launch ("engine1_all") instead takes the first n at which a wave of the single launch scores
    five tiles, where TPW allows one: more than 64 flagged rows in one wave, so the wave's flag
    stage (FlagStage, 128 entries) is flushed in mid-launch and filled again."""
    if fmt != "w64":
        return 137
    n = _first(lambda n: plan(kind, fmt, env, n, coalesced=True).rounds.max() >= 1) or 137
    if mode == "engine1_all":
        return _first(lambda n: plan(kind, fmt, env, n).tiles.max() >= 5) or n
    return n


def take(n, total):
    """Row indices of an n-row case: n consecutive fixture rows (cyclic), another phase of the
    amount cycle per size."""
    return (7 * n % len(EDGE_AMOUNTS) + np.arange(n)) % total


THRESHOLD = {"plain": 0.5, "rules": 0.5, "all": 0.0, "none": 2.0, "hostile": 0.5}
ENGINE_MODES = {"engine1": dict(coalesce=1), "engine4": dict(coalesce=4), "engine1_all": dict(coalesce=1, threshold=0.0)}
RULES3 = """
when amount > 200 and proba >= 0.2 then fraud
when V17 < -2.5 or abs(V14) > 4 then fraud
otherwise standard
"""                                     # the rule set RULES3 of test_rules_gpu.py


def cases(cfg):
    """Every case one configuration scores, in order: (kind, fmt, n, mode)."""
    env = cfg["env"]
    out = []
    for kind in KINDS:
        for fmt in FORMATS:
            ns = row_counts(env, kind, fmt)
            out += [(kind, fmt, n, mode) for n in ns for mode in ("plain", "rules", "all", "none")]
            out.append((kind, fmt, ns[-1], "hostile"))
            if cfg["big"]:
                out.append((kind, fmt, BIG_N, "plain"))
            if fmt != "f32s":                       # the engine's f32 rows are contiguous
                out += [(kind, fmt, engine_rows(env, kind, fmt, mode), mode) for mode in ENGINE_MODES]
    return out


def default_cases():
    """The cases of every configuration, once each: what the parent scores without the knobs."""
    seen = {}
    for cfg in CONFIGS.values():
        for case in cases(cfg):
            seen.setdefault(case_key(case), case)
    return seen


def case_key(case):
    """Cases with one key score the same rows with the same routing, so their probability and
    route bytes must be identical: an engine launch is compared with the plain launch of its rows."""
    kind, fmt, n, mode = case
    if mode in ENGINE_MODES:
        thr = ENGINE_MODES[mode].get("threshold", 0.5)
        return (kind, fmt, n * ENGINE_MODES[mode]["coalesce"], "first", thr)
    return (kind, fmt, n, mode, THRESHOLD[mode])


# --------------------------------------------------------------------------- running a case
def _why(e):
    """The failed assertion of check / engine_case as text: its source line and its message."""
    import traceback
    tb = traceback.extract_tb(e.__traceback__)[-1]
    return f"{tb.name}: {tb.line}: {' '.join(str(e).split())[:300]}"


class Runner:
    """Scores cases on one device: device models, rule program and uploaded rows are made once."""

    def __init__(self, dev):
        from ccfd_demo_summit_amd.ops.kernels import DeviceModel, DeviceRules
        from ccfd_demo_summit_amd.router.rules import RuleSet
        self.dev = dev
        self.setup = build_setup()
        self.ruleset = RuleSet.parse(RULES3)
        self.rules = DeviceRules(self.ruleset, dev)
        self.dm = {(k, w): DeviceModel(self.setup[1][k], dev, wire=w) for k in KINDS for w in (False, True)}
        self._rows = {}

    def _device_rows(self, src, idx_key, rows, fmt):
        import torch
        from ccfd_demo_summit_amd.contracts import encode_wire
        key = (src, idx_key, fmt)
        if key not in self._rows:
            if fmt == "w64":
                t = torch.from_numpy(encode_wire(rows)).to(self.dev)
            elif fmt == "f32":
                t = torch.from_numpy(np.array(rows, np.float32)).to(self.dev)
            else:                                   # leading dimension 32: launch_mlp_t's strided kernel
                t = torch.zeros(len(rows), 32, dtype=torch.float32, device=self.dev)[:, :30]
                t.copy_(torch.from_numpy(np.array(rows, np.float32)))
                assert t.stride(0) == 32
            if len(self._rows) > 64:                # bounded: a configuration has ~40 row sets
                self._rows.clear()
            self._rows[key] = t
        return self._rows[key]

    def launch(self, kind, fmt, src, idx_key, rows, thr, rules):
        import torch
        from ccfd_demo_summit_amd.ops.kernels import new_counters, score
        cnt = new_counters(self.dev)
        x = self._device_rows(src, idx_key, rows, fmt)
        p, r = score(self.dm[(kind, fmt == "w64")], x, thr, counters=cnt, rules=self.rules if rules else None)
        torch.cuda.synchronize(self.dev)            # raises on a HIP error: nothing runs after it
        return p.cpu().numpy(), r.cpu().numpy(), cnt.cpu().numpy()

    def run(self, case, default=False):
        """Scores `case` and returns its figures as a JSON-able dict; judging is the caller's.
        default: the plain launch an engine case is compared with (case_key) instead of the engine."""
        kind, fmt, n, mode = case
        X, _, ref = self.setup
        wire = fmt == "w64"
        j = {"kind": kind, "fmt": fmt, "n": n, "mode": mode}
        if mode in ENGINE_MODES:
            kw = ENGINE_MODES[mode]
            k = kw["coalesce"]
            if default:
                p, r, _ = self.launch(kind, fmt, "X", ("first", n * k), X[:n * k], kw.get("threshold", 0.5), False)
                fraud = r != 0
            else:
                try:
                    p, fraud = engine_case(self.dev, self.setup, kind, wire, n * k, [(k, n)], batch=n, depth=4,
                                           streams=1, exec_mode="launch", **kw)
                except AssertionError as e:
                    j["check"] = _why(e)
                    return j
            j.update(check=None, err=float(np.abs(p.astype(np.float64) - ref[(kind, wire)][:n * k]).max()),
                     fraud=int(fraud.sum()), crc_p=zlib.crc32(p.tobytes()),
                     crc_r=zlib.crc32(fraud.astype(np.uint8).tobytes()))
            return j
        thr = THRESHOLD[mode]
        if mode == "hostile":
            H = hostile_rows()
            rows = H[:n]
            p, r, c = self.launch(kind, fmt, "H", n, rows, thr, False)
            bk = np.searchsorted(BOUNDS, rows[:, 29], side="left")
            fraud = r != 0
            j.update(in_range=bool(np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()),
                     route_bad=int((fraud != (p >= np.float32(thr))).sum()),
                     hist_bad=int((c[8:22] != np.bincount(bk[~fraud], minlength=14)).sum()
                                  + (c[24:38] != np.bincount(bk[fraud], minlength=14)).sum()),
                     counters=[int(c[0]), int(c[1]), int(c[2])], fraud=int(fraud.sum()),
                     psum_own=abs(int(c[3]) - int(np.round(p.astype(np.float64) * 1e6).sum())),
                     crc_p=zlib.crc32(p.tobytes()), crc_r=zlib.crc32(r.tobytes()))
            return j
        idx = take(n, len(X))
        rows = X[idx]
        p, r, c = self.launch(kind, fmt, "X", n, rows, thr, mode == "rules")
        fraud = r != 0
        if mode == "rules":
            want = self.ruleset.evaluate(p, X=extras()[0][idx] if wire else rows)
        else:
            want = p >= np.float32(thr)
        try:
            check(c, rows[:, 29], ref[(kind, wire)][idx], fraud, None, f"{kind} {fmt} {mode} n={n}")
            j["check"] = None
        except AssertionError as e:
            j["check"] = _why(e)
        j.update(err=float(np.abs(p.astype(np.float64) - ref[(kind, wire)][idx]).max()),
                 route_bad=int((fraud != (np.asarray(want) != 0)).sum()), fraud=int(fraud.sum()),
                 psum_own=abs(int(c[3]) - int(np.round(p.astype(np.float64) * 1e6).sum())),
                 crc_p=zlib.crc32(p.tobytes()), crc_r=zlib.crc32(r.tobytes()))
        if kind == "mlp" and not wire:
            j["err32"] = float(np.abs(p.astype(np.float64) - extras()[1][idx]).max())
        return j


# tolerances the suite already uses for these paths (test_kernels_gpu.py)
TOL = {("mlp", True): 2e-4, ("mlp", False): 2e-3, ("lr", True): 1e-5, ("lr", False): 1e-5}
TOL_MLP_FP32 = 1e-2


def judge(j):
    """The failures of one case's figures against the oracle (a list of strings, empty: passed)."""
    bad = []
    wire = j["fmt"] == "w64"
    if j["mode"] == "hostile":
        n = j["n"]
        if not j["in_range"]:
            bad.append("proba outside [0, 1] or not finite")
        if j["route_bad"]:
            bad.append(f"route != (p >= thr) on {j['route_bad']} rows")
        if j["hist_bad"]:
            bad.append(f"{j['hist_bad']} histogram buckets differ")
        if j["counters"] != [n, j["fraud"], n - j["fraud"]]:
            bad.append(f"counters {j['counters']}")
        if j["psum_own"] > n:
            bad.append(f"proba sum off by {j['psum_own']}")
        return bad
    if j["check"] is not None:
        bad.append(j["check"])
    if "err" not in j:                  # an engine case that failed before its outputs were read
        return bad
    if not j["err"] < TOL[(j["kind"], wire)]:
        bad.append(f"max err {j['err']:.3g}")
    if "err32" in j and not j["err32"] < TOL_MLP_FP32:
        bad.append(f"max err against fp32 {j['err32']:.3g}")
    if j["mode"] in ENGINE_MODES:
        return bad
    if j["route_bad"]:
        bad.append(f"{j['route_bad']} routes differ from the host's")
    if j["psum_own"] > j["n"]:
        bad.append(f"proba sum off by {j['psum_own']}")
    if j["mode"] == "all" and j["fraud"] != j["n"] or j["mode"] == "none" and j["fraud"] != 0:
        bad.append(f"{j['fraud']} fraud rows at threshold {THRESHOLD[j['mode']]}")
    return bad
