"""The device rule interpreter (csrc/kernels/rules.h rule_route) on every opcode, stack slot,
feature gather and row path, with the catalogue of tests/helpers/rule_cases.py
(test_rule_programs_cpu.py proves what the catalogue notices).

Every route is compared for equality with ``RuleSet.evaluate`` on the kernel's own probability
output and the rows as the kernel saw them (the rules are under test, not the model): both
sides are round-to-nearest float32, so there is no tolerance and no excused row anywhere in
this file.  Every launch is also checked for its counters, both amount histograms and, where
the path has one, its flag list (rule_cases.launch_problems).

Paths: the plain launches of MLP / LR (f32 contiguous, f32 with leading dimension 32, W64), the
oblivious GBDT v1 and the general forest (f32 contiguous and strided), the binned kernels
(G32 / G20; leaves in LDS and in global memory; score_forest_bins), the rows-in-registers GBDT
kernel v2 (by size, and forced with R = 2 and R = 1 in child processes), the streaming engines
(persistent and coalesced launches), and stale binned rows under a default-fraud program."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from tests.helpers import rule_cases as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class Ctx:
    """Device models, uploaded rows and rule programs of the module, each made once."""

    def __init__(self, dev):
        self.dev = dev
        self._dm, self._rows, self._rules = {}, {}, {}
        self.results = {}

    def model(self, kind, fmt):
        from ccfd_demo_summit_amd.ops.kernels import DeviceModel
        key = (kind, "f32" if fmt == "f32s" else fmt)
        if key not in self._dm:
            m = rc.models()[kind]
            if fmt in ("g32", "g20"):
                bins = fmt if kind == "forest" else (True if fmt == "g32" else "g20")
                self._dm[key] = DeviceModel(m, self.dev, bins=bins)
            else:
                self._dm[key] = DeviceModel(m, self.dev, wire=fmt == "w64")
            assert self._dm[key].row_format == key[1]
        return self._dm[key]

    def upload(self, X, dm, fmt):
        from ccfd_demo_summit_amd.contracts import encode_wire
        if fmt == "w64":
            return torch.from_numpy(encode_wire(X)).to(self.dev)
        if fmt in ("g32", "g20"):
            return torch.from_numpy(dm.bins.encode(X)).to(self.dev)
        if fmt == "f32":
            return torch.from_numpy(np.array(X, np.float32)).to(self.dev)
        t = torch.zeros(len(X), 32, dtype=torch.float32, device=self.dev)[:, :30]     # leading dimension 32
        t.copy_(torch.from_numpy(np.array(X, np.float32)))
        assert t.stride(0) == 32
        return t

    def rows(self, kind, fmt, n):
        key = (kind if fmt in ("g32", "g20") else None, fmt, n)
        if key not in self._rows:
            self._rows[key] = self.upload(rc.rows()["f32"][:n], self.model(kind, fmt), fmt)
        return self._rows[key]

    def rules(self, tag, name, rs):
        from ccfd_demo_summit_amd.ops.kernels import DeviceRules
        key = (tag, name)
        if key not in self._rules:
            self._rules[key] = DeviceRules(rs, self.dev)
        return self._rules[key]


@pytest.fixture(scope="module")
def ctx(gpu):
    return Ctx(gpu)


def _launch(ctx, dm, x, dr):
    from ccfd_demo_summit_amd.ops.kernels import new_counters, score
    cnt = new_counters(ctx.dev)
    p, r = score(dm, x, 0.5, counters=cnt, rules=dr)
    torch.cuda.synchronize(ctx.dev)
    return p.cpu().numpy(), r.cpu().numpy(), cnt.cpu().numpy()


def _assert_none_failed(failed, what):
    for name, bad in failed.items():
        print(what, name, bad)
    assert not failed, f"{what}: {len(failed)} programs fail, first {list(failed.items())[:3]}"


# --------------------------------------------------------------------------- plain launches
FEATURE_PATHS = [(k, f) for k in ("mlp", "lr") for f in ("f32", "f32s", "w64")] + \
                [(k, f) for k in ("gbdt", "forest") for f in ("f32", "f32s")]
PROBA_PATHS = [(k, f) for k in ("gbdt", "gbdt_gl", "forest") for f in ("g32", "g20")]


@pytest.mark.parametrize("n", rc.ROW_COUNTS)
@pytest.mark.parametrize("kind,fmt", FEATURE_PATHS)
def test_feature_catalogue_on_plain_launches(ctx, kind, fmt, n):
    """score_mlp / score_lr (contiguous and strided f32 rows), wire_body (W64 rows), score_gbdt v1
    and score_forest (contiguous and strided): every feature program at 1 row, one tile and a
    row, and 17 tiles / 4 chunks with their tails."""
    view = "w64" if fmt == "w64" else "f32"
    dm, x = ctx.model(kind, fmt), ctx.rows(kind, fmt, n)
    seen = rc.rows()[view][:n]
    failed = {}
    for name, rs in rc.feature_catalogue(kind, view).items():
        p, r, c = _launch(ctx, dm, x, ctx.rules((kind, view), name, rs))
        bad = rc.launch_problems(rs, p, r, c, seen, seen[:, 29])
        if bad:
            failed[name] = bad
    _assert_none_failed(failed, f"{kind} {fmt} n={n}")


@pytest.mark.parametrize("n", rc.ROW_COUNTS)
@pytest.mark.parametrize("kind,fmt", PROBA_PATHS)
def test_proba_catalogue_on_binned_launches(ctx, kind, fmt, n):
    """score_gbdt_g32 on G32 and G20 rows with the leaves in LDS ("gbdt") and in global memory
    ("gbdt_gl": the kGL switch), and score_forest_bins on both formats: every proba-only program."""
    dm, x = ctx.model(kind, fmt), ctx.rows(kind, fmt, n)
    amount = rc.rows()["f32"][:n, 29]
    failed = {}
    for name, rs in rc.proba_catalogue(kind).items():
        p, r, c = _launch(ctx, dm, x, ctx.rules((kind, "proba"), name, rs))
        bad = rc.launch_problems(rs, p, r, c, None, amount)
        if int(c[4]):
            bad.append(f"{int(c[4])} rows counted stale")
        if bad:
            failed[name] = bad
    _assert_none_failed(failed, f"{kind} {fmt} n={n}")


# --------------------------------------------------------------------------- GBDT v2
def test_v2_kernel_by_size_routes_sweeps_and_deepest_stack(ctx):
    """score_gbdt_v2_kernel<D, 2, true> as the launch picks it from 262144 contiguous rows on:
    262144 + 64 + 9 rows (an odd number of two-chunk wave steps, 9 rows in the last chunk), the
    three packed sweeps (every feature through the register arrays x0[j] / x1[j] at a runtime j)
    and the depth-8 slot program.  Nothing on the GPU tells which kernel a launch took; rows that
    are not contiguous fall back to v1, which adds the trees as four per-wave partial sums where
    v2 adds them one after the other, so the CRC of the contiguous launch's probabilities must
    differ from the strided (v1) launch's of the same rows."""
    X = rc.big_rows()
    dm = ctx.model("gbdt", "f32")
    x = ctx.upload(X, dm, "f32")
    cat = rc.feature_catalogue("gbdt", "f32")
    failed, crc = {}, set()
    for name in rc.V2_BIG_PROGRAMS:
        rs = cat[name]
        p, r, c = _launch(ctx, dm, x, ctx.rules(("gbdt", "f32"), name, rs))
        assert 0 < r.sum() < len(r), name
        bad = rc.launch_problems(rs, p, r, c, X, X[:, 29])
        if bad:
            failed[name] = bad
        crc.add(zlib.crc32(p.tobytes()))
    _assert_none_failed(failed, "v2 by size")
    assert len(crc) == 1                                       # the program does not touch the probability
    p1, _, _ = _launch(ctx, dm, ctx.upload(X, dm, "f32s"), None)
    assert zlib.crc32(p1.tobytes()) not in crc, "bit-identical to the v1 launch: v2 was not launched"


@pytest.mark.parametrize("rows_per_step", ["2", "1"])
def test_forced_v2_kernel_routes_the_feature_catalogue(ctx, rows_per_step):
    """score_gbdt_v2_kernel<D, R, true> with R = 2 and R = 1, depths 3 and 6, the full feature
    catalogue at 1, 65 and 273 rows.  CCFD_GBDT_KERNEL and CCFD_GBDT_R are read once per process,
    so a child process (rules_variant_probe.py) scores and this test judges every line it
    printed.  Nothing on the GPU tells which kernel a launch took: as in
    test_gbdt_edges_gpu.py::test_f32_v2_kernel_every_depth_and_tree_count, the CRC of the
    child's probabilities is compared with this process's v1 launch of the same rows, which sums
    the 60 trees in another order, and must differ."""
    from tests.helpers import rules_variant_probe as probe
    env = dict(os.environ, CCFD_GBDT_KERNEL="v2", CCFD_GBDT_R=rows_per_step)
    # child: interpreter + torch + HIP start-up (tens of seconds at worst), the catalogues (~2 s),
    # ~700 launches of <= 273 rows (about a millisecond each)
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "rules_variant_probe.py")], env=env,
                       capture_output=True, text=True, timeout=150)
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert lines[0] == {"kernel": "v2", "R": rows_per_step}
    cases = lines[1:-1]
    want = {(k, n, name) for k in probe.MODELS for n in probe.ROW_COUNTS for name in rc.feature_catalogue(k, "f32")}
    assert lines[-1] == {"done": len(want)}
    assert {(j["model"], j["n"], j["program"]) for j in cases} == want
    bad = [(j["model"], j["n"], j["program"], j["problems"]) for j in cases if j["problems"]]
    print("failing (model, n, program, problems):", *bad, sep="\n")
    assert not bad, f"{len(bad)} of {len(cases)} launches, first {bad[:4]}"
    assert os.environ.get("CCFD_GBDT_KERNEL") in (None, "v1")      # this process takes v1 at 273 rows
    for kind in probe.MODELS:
        p1, _, _ = _launch(ctx, ctx.model(kind, "f32"), ctx.rows(kind, "f32", 273), None)
        crc = {j["crc"] for j in cases if (j["model"], j["n"]) == (kind, 273)}
        assert len(crc) == 1
        assert zlib.crc32(p1.tobytes()) not in crc, f"{kind}: the child's probabilities are v1's to the bit"


# --------------------------------------------------------------------------- engines
def _counters(eng, gpu):
    side = torch.cuda.Stream(gpu)
    c = eng.flip_epoch(side)
    side.synchronize()
    return c.cpu().numpy()


def _engine_program(gpu, dm, rs, X, seen, log_kw, **kw):
    """One engine routed by `rs`: a log of the rows pumped as three full micro-batches and a
    partial one (counters, histograms, flag list), then eng.score() for every row's probability
    and route.  The kernel is deterministic, so the pump and score() give a row the same route."""
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceRules
    n = len(X)
    eng = StreamEngine(dm, batch=256, depth=4, streams=1, input_mode="zerocopy", rules=DeviceRules(rs, gpu), **kw)
    log = PartitionLog.from_arrays(X, ids=np.arange(n, dtype=np.uint64), **log_kw)
    try:
        eng.add_log(0, log)
        assert eng.pump(3).rows + eng.pump(1, batch_rows=n - 3 * 256).rows == n
        flagged = eng.drain_flagged()["tx_id"].astype(np.int64)
        c = _counters(eng, gpu)
        p, r = eng.score(X)
    finally:
        eng.close()
        log.free()
    assert 0 < r.sum() < n
    return rc.launch_problems(rs, p, r, c, seen, X[:, 29], flagged=flagged)


ENGINE_PATHS = {
    "persistent-mlp-f32": ("mlp", "f32", dict(exec_mode="persistent"), {}),
    "persistent-mlp-w64-claimed": ("mlp", "w64", dict(exec_mode="persistent", persist_items="claimed"), {}),
    "persistent-mlp-w64-pipe": ("mlp", "w64", dict(exec_mode="persistent"), {"CCFD_PERSIST_PIPE": "1"}),
    "persistent-lr-w64": ("lr", "w64", dict(exec_mode="persistent"), {}),
    "launch-coalesce4-mlp-f32": ("mlp", "f32", dict(exec_mode="launch", coalesce=4), {}),
    "launch-coalesce4-mlp-w64": ("mlp", "w64", dict(exec_mode="launch", coalesce=4), {}),
}


@pytest.mark.parametrize("path", list(ENGINE_PATHS))
def test_engines_route_sweeps_deepest_stack_and_ieee(ctx, monkeypatch, path):
    """score_persist in both forms (claimed and pipelined items), the persistent f32 kernel, the
    persistent LR kernel and the coalesced launches: the three packed sweeps, the depth-8 slot
    program and the IEEE program."""
    kind, fmt, kw, env = ENGINE_PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, seen = rc.engine_rows()["f32"], rc.engine_rows()[fmt]
    cat = rc.feature_catalogue(kind, fmt)
    failed = {}
    for name in rc.ENGINE_PROGRAMS:
        bad = _engine_program(ctx.dev, ctx.model(kind, fmt), cat[name], X, seen, dict(wire=fmt == "w64"), **kw)
        if bad:
            failed[name] = bad
    _assert_none_failed(failed, path)


@pytest.mark.parametrize("fmt,items,global_leaves", [("g32", "auto", False), ("g20", "claimed", False),
                                                      ("g20", "pipelined", False), ("g32", "claimed", True)])
def test_persistent_binned_gbdt_routes_proba_programs(ctx, monkeypatch, fmt, items, global_leaves):
    """score_gbdt_g32_persist in both forms (claimed and pipelined items) on G32 and G20 rows, and
    the claimed form with its leaves gathered from global memory (kGL): the proba-only twins of
    the sweep, the depth-8 slot program and the IEEE program."""
    if global_leaves:
        monkeypatch.setenv("CCFD_G32_GLOBAL_LEAVES", "1")
    dm = ctx.model("gbdt", fmt)
    X = rc.engine_rows()["f32"]
    cat = rc.proba_catalogue("gbdt")
    failed = {}
    for name in rc.ENGINE_PROGRAMS_P:
        bad = _engine_program(ctx.dev, dm, cat[name], X, None, dict(bins=dm.bins), exec_mode="persistent",
                              persist_items=items)
        if bad:
            failed[name] = bad
    _assert_none_failed(failed, f"persistent gbdt {fmt} {items}")


# --------------------------------------------------------------------------- stale binned rows
def _restamp(enc, rows, stamp):
    """Rows re-encoded under another bin table's stamp (G32: byte 31; G20: bits 154..159)."""
    if enc.shape[1] == 32:
        enc[rows, 31] = (stamp % 255) + 1
    else:
        enc[rows, 19] = (enc[rows, 19] & 0x03) | (((stamp % 63) + 1) << 2)


def _stale_launch(ctx, kind, fmt):
    """The problems of one plain launch of the 273 rows with 83 of them stale."""
    key = ("stale", kind, fmt)
    if key not in ctx.results:
        dm = ctx.model(kind, fmt)
        X = rc.rows()["f32"]
        rs = rc.proba_catalogue(kind)[rc.STALE_PROGRAM]
        assert rs.default != 0 and not rs.feature_vars()
        stale = np.zeros(len(X), bool)
        stale[60:70] = stale[200:273] = True                   # across a chunk boundary; the partial last chunk
        enc = dm.bins.encode(X)
        _restamp(enc, stale, dm.bins.stamp)
        p, r, c = _launch(ctx, dm, torch.from_numpy(enc).to(ctx.dev), ctx.rules((kind, "proba"), rc.STALE_PROGRAM, rs))
        assert not r[stale].any() and 0 < r[~stale].sum() < (~stale).sum()
        ctx.results[key] = rc.launch_problems(rs, p, r, c, None, X[:, 29], stale=stale)
        print(kind, fmt, "standard histogram", c[8:22].tolist(), "fraud histogram", c[24:38].tolist(), ctx.results[key])
    return ctx.results[key]


def _stale_engine(ctx, fmt):
    """The same through score_gbdt_g32_persist: a log whose rows 500..539 (across the item and
    micro-batch boundary at 512) carry another table's stamp; per-row outputs from the scored ring."""
    key = ("stale-engine", fmt)
    if key in ctx.results:
        return ctx.results[key]
    from ccfd_demo_summit_amd.engine import PartitionLog, StreamEngine
    from ccfd_demo_summit_amd.ops.kernels import DeviceRules
    dm = ctx.model("gbdt", fmt)
    X = rc.engine_rows()["f32"]
    n = len(X)
    rs = rc.proba_catalogue("gbdt")[rc.STALE_PROGRAM]
    stale = np.zeros(n, bool)
    stale[500:540] = True
    eng = StreamEngine(dm, batch=256, depth=4, streams=1, input_mode="zerocopy", exec_mode="persistent",
                       rules=DeviceRules(rs, ctx.dev))
    log = PartitionLog.from_arrays(X, ids=np.arange(n, dtype=np.uint64), bins=dm.bins)
    try:
        raw = log.feats.array.view(np.uint8).reshape(n, -1)
        assert raw.shape[1] == (32 if fmt == "g32" else 20)
        _restamp(raw, stale, dm.bins.stamp)
        eng.enable_scored(n + 64)
        eng.add_log(0, log)
        assert eng.pump(3).rows + eng.pump(1, batch_rows=n - 3 * 256).rows == n
        flagged = eng.drain_flagged()["tx_id"].astype(np.int64)
        rec = eng.drain_scored()
        c = _counters(eng, ctx.dev)
    finally:
        eng.close()
        log.free()
    ids = rec["tx_id"].astype(np.int64)
    np.testing.assert_array_equal(np.sort(ids), np.arange(n))             # every row scored once
    p = np.empty(n, np.float32)
    r = np.empty(n, np.uint8)
    p[ids], r[ids] = rec["proba"], rec["route"] != 0
    assert not r[stale].any() and 0 < r[~stale].sum() < (~stale).sum()
    ctx.results[key] = rc.launch_problems(rs, p, r, c, None, X[:, 29], flagged=flagged, stale=stale)
    print("engine", fmt, "standard histogram", c[8:22].tolist(), "fraud histogram", c[24:38].tolist(), ctx.results[key])
    return ctx.results[key]


STALE_CASES = [("gbdt", "g32"), ("gbdt", "g20"), ("forest", "g32"), ("forest", "g20"), ("engine", "g32"), ("engine", "g20")]


def _stale_problems(ctx, kind, fmt):
    return _stale_engine(ctx, fmt) if kind == "engine" else _stale_launch(ctx, kind, fmt)


@pytest.mark.parametrize("kind,fmt", STALE_CASES)
def test_stale_rows_stay_standard_under_a_default_fraud_program(ctx, kind, fmt):
    """g32_core.h routes ``valid && fresh && rule_route(...)``: under a proba-only program whose
    default is fraud, through score_gbdt_g32, score_forest_bins and the persistent G32 / G20 engine,
    every stale row still has route 0 and a NaN probability, is counted in the stale counter and
    in neither the fraud counter, an amount histogram nor the flag list; the fresh rows route
    like evaluate.  (The epilogue used to add a stale row to the standard histogram under the
    bucket byte of a row it otherwise does not trust: 83 of the 273 rows here, 40 of the
    engines' 809.)"""
    bad = _stale_problems(ctx, kind, fmt)
    assert not bad, bad
