"""The inputs of test_mlp_variants_gpu.py, proved on the CPU: tile_cases.plan() restates the MLP /
LR launch arithmetic (launch_mlp_t, launch_w, launch_wire, launch_lr_t, launch_lr_w, the coalesced
launches and the prefetch ring of wire_stream_body), and the row counts chosen with it reach, in
every configuration and row format, every loop of the kernels that configuration selects.  plan()
chooses inputs only; no GPU verdict depends on it."""
import os

import numpy as np
import pytest

from tests.helpers import tile_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(c, k, f) for c in tc.CONFIGS for k in tc.KINDS for f in tc.FORMATS]


def _documented_values():
    """{knob: values} from the kernel table of docs/TUNING.md."""
    out = {}
    for line in open(os.path.join(ROOT, "docs", "TUNING.md"), encoding="utf-8"):
        cells = [c.strip() for c in line.split("|")]
        if len(cells) > 4 and cells[1].strip("`") in tc.KNOBS:
            out[cells[1].strip("`")] = [v.strip(" `") for v in cells[3].split(",")]
    return out


def test_every_documented_knob_value_is_in_some_configuration():
    doc = _documented_values()
    assert set(doc) == set(tc.KNOBS)
    assert doc == {"CCFD_MLP_WAVES": ["1", "2", "4", "8", "16"], "CCFD_MLP_PF": ["1", "2", "4"],
                   "CCFD_MLP_REGW": ["0", "1"], "CCFD_MLP_TPW": ["1", "2", "4", "8"],
                   "CCFD_MLP_WEIGHTS": ["lds", "global"], "CCFD_LR_WAVES": ["4", "8", "16"],
                   "CCFD_LR_PF": ["2", "4", "8"], "CCFD_LR_OCC": ["4", "8"]}
    assert len(tc.CONFIGS) <= 10                         # one child process each
    for knob, values in doc.items():
        used = {cfg["env"][knob] for cfg in tc.CONFIGS.values()}
        assert used == set(values), knob
    # the LR columns are the full CCFD_LR_WAVES x CCFD_LR_PF square
    assert len({(c["env"]["CCFD_LR_WAVES"], c["env"]["CCFD_LR_PF"]) for c in tc.CONFIGS.values()}) == 9


def _simulate(p, n):
    """wire_stream_body's ring, wave by wave, as written: (rounds, tail) per wave and where the
    partial last tile was scored."""
    ntiles = (n + 15) // 16
    tstride = p.grid * p.waves
    full_end = ntiles - (p.pf - 1) * tstride
    rounds, tail, where = [], [], None
    for v in range(tstride):
        tile, r, t = v, 0, 0
        while tile < full_end:
            for _ in range(p.pf):
                if tile == ntiles - 1 and n % 16:
                    where = "steady"
                assert tile < ntiles                     # a steady round's tiles all exist
                tile += tstride
            r += 1
        for _ in range(p.pf):
            if tile < ntiles:
                if tile == ntiles - 1 and n % 16:
                    where = "tail"
                t += 1
                tile += tstride
        assert tile >= ntiles                            # nothing is left behind
        rounds.append(r)
        tail.append(t)
    return rounds, tail, where


@pytest.mark.parametrize("cfg", list(tc.CONFIGS))
def test_plan_equals_the_ring_walked_tile_by_tile(cfg):
    env = tc.CONFIGS[cfg]["env"]
    for kind in tc.KINDS:
        for n in (1, 9, 16, 137, 393, 777, 1801, 4105, 20009):
            for coalesced in (False, True):
                p = tc.plan(kind, "w64", env, n, coalesced=coalesced)
                rounds, tail, where = _simulate(p, n)
                assert list(p.rounds) == rounds and list(p.tail) == tail and p.partial == where, (kind, n, coalesced)
                assert (p.tail < p.pf).all() and p.tiles.sum() == p.ntiles
                f = tc.plan(kind, "f32", env, n, coalesced=coalesced)
                assert f.tiles.sum() == f.ntiles and f.pf == 1


def test_plan_restates_the_launch_rules():
    def env(**kw):
        return {"CCFD_" + k: str(v) for k, v in kw.items()}
    # defaults: register weights, 8 waves, four tiles in flight; LR 16 waves, four tiles
    p = tc.plan("mlp", "w64", {}, 4096)
    assert (p.kernel, p.waves, p.pf, p.grid) == ("mlp_wire_reg", 8, 4, 4)
    p = tc.plan("lr", "w64", {}, 4096)
    assert (p.kernel, p.waves, p.pf, p.grid) == ("lr_wire", 16, 4, 2)
    assert tc.plan("mlp", "f32", {}, 4096).waves == 4 and tc.plan("lr", "f32s", {}, 4096).waves == 4
    # coalesced: LDS weights, two tiles in flight; LR <4, 4> whatever CCFD_LR_* say
    p = tc.plan("mlp", "w64", {}, 4096, coalesced=True)
    assert (p.kernel, p.waves, p.pf, p.grid) == ("mlp_wire", 4, 2, 8)
    p = tc.plan("lr", "w64", env(LR_WAVES=8, LR_PF=8), 4096, coalesced=True)
    assert (p.waves, p.pf) == (4, 4)
    # a forced CCFD_MLP_PF=1 means 2 on the register-weight kernel, 1 on the LDS-weight one
    assert tc.plan("mlp", "w64", env(MLP_PF=1), 4096).pf == 2
    assert tc.plan("mlp", "w64", env(MLP_PF=1, MLP_REGW=0), 4096).pf == 1
    # 16 waves never take register weights, and mean 4 on f32 rows (8 too)
    p = tc.plan("mlp", "w64", env(MLP_WAVES=16, MLP_REGW=1), 4096)
    assert (p.kernel, p.waves, p.pf) == ("mlp_wire", 16, 2)
    for w in (4, 8, 16):
        assert tc.plan("mlp", "f32", env(MLP_WAVES=w), 4096).waves == 4
        assert tc.plan("lr", "f32", env(MLP_WAVES=w), 4096).waves == 4
    assert tc.plan("lr", "f32", env(MLP_WAVES=2), 4096).waves == 2          # LR f32 rows follow CCFD_MLP_WAVES
    # CCFD_MLP_TPW sizes the LR grids too
    assert [tc.plan("lr", "w64", env(MLP_TPW=t), 65536).grid for t in (1, 2, 4, 8)] == [256, 128, 64, 32]
    assert [tc.plan("lr", "f32", env(MLP_TPW=t), 65536).grid for t in (1, 2, 4, 8)] == [1024, 512, 256, 128]
    # the caps: 256*16/kW, 256*8/kW with register weights, 2048 (LR f32), 256*4*OCC/kW (LR W64)
    big = 1 << 22
    assert tc.plan("mlp", "w64", env(MLP_WAVES=4), big).grid == 512
    assert tc.plan("mlp", "w64", env(MLP_WAVES=4, MLP_REGW=0), big).grid == 1024
    assert tc.plan("mlp", "f32", env(MLP_WAVES=1), big).grid == 4096
    assert tc.plan("lr", "f32", env(MLP_WAVES=1), big).grid == 2048
    assert tc.plan("lr", "w64", env(LR_WAVES=8, LR_OCC=8), big).grid == 1024
    assert tc.plan("lr", "w64", env(LR_WAVES=8), big).grid == 512
    # a value the launch code does not accept is the default
    assert tc.plan("lr", "w64", env(LR_WAVES=2, LR_PF=1, MLP_TPW=3), 4096)[:4] == tc.plan("lr", "w64", {}, 4096)[:4]


@pytest.mark.parametrize("knobs,tails,steady", [
    (dict(MLP_WAVES=8, MLP_PF=4, MLP_REGW=0, MLP_TPW=8), [1, 137, 265], 393),
    (dict(MLP_WAVES=4, MLP_PF=4, MLP_REGW=0, MLP_TPW=4), [1, 73, 137], 201),
    (dict(MLP_WAVES=16, MLP_PF=4, MLP_TPW=8), [1, 265, 521], 777),
    (dict(MLP_WAVES=2, MLP_PF=2, MLP_REGW=0, MLP_TPW=2), [1], 41),
    (dict(LR_WAVES=4, LR_PF=8, MLP_TPW=8), [1, 73, 137, 201, 265, 329, 393], 457),
])
def test_first_row_counts_of_each_tail_and_of_the_steady_round(knobs, tails, steady):
    """At grid 1: the first n = 16k + 9 (and n = 1) whose plan has a tail of 1, 2, .. tiles, and
    the first with a steady round that ends in the partial tile."""
    env = {"CCFD_" + k: str(v) for k, v in knobs.items()}
    kind = "lr" if "LR_PF" in knobs else "mlp"
    for length, n in enumerate(tails, 1):
        p = tc.plan(kind, "w64", env, n)
        assert p.grid == 1 and p.tail.max() == length and p.rounds.max() == 0
        if n > 1:
            assert tc.plan(kind, "w64", env, n - 16).tail.max() == length - 1
    p = tc.plan(kind, "w64", env, steady)
    assert p.grid == 1 and p.rounds.max() == 1 and p.partial == "steady"
    assert tc.plan(kind, "w64", env, steady - 16).rounds.max() == 0


@pytest.mark.parametrize("cfg,kind,fmt", CASES)
def test_row_counts_reach_every_loop_of_the_selected_kernel(cfg, kind, fmt):
    env = tc.CONFIGS[cfg]["env"]
    tpw = int(env["CCFD_MLP_TPW"])
    ns = tc.row_counts(env, kind, fmt) + ([tc.BIG_N] if tc.CONFIGS[cfg]["big"] else [])
    assert ns == sorted(set(ns)) and len(ns) <= 14 and max(tc.row_counts(env, kind, fmt)) <= tc.HOSTILE_ROWS
    plans = [tc.plan(kind, fmt, env, n) for n in ns]
    pf = plans[0].pf
    assert any(p.partial is not None for p in plans) and any(p.partial is None for p in plans)
    if fmt == "w64":
        # (b) a tail of every length
        assert set(range(1, pf)) <= {int(t) for p in plans for t in p.tail}
        assert pf == 1 or any(p.partial == "tail" for p in plans)        # one tile in flight: no tail loop
        if tpw >= pf:
            # (a) a full steady round, (c) the partial last tile inside one
            assert any(p.rounds.max() >= 1 for p in plans)
            assert any(p.partial == "steady" for p in plans)
        # what a steady round refills is consumed: by a tail, by a second round
        if tpw > pf > 1:
            assert any(((p.rounds >= 1) & (p.tail >= 1)).any() for p in plans)
        if tpw >= 2 * pf:
            assert any(p.rounds.max() >= 2 for p in plans)
        # (d) a coalesced sub-batch in which a wave has a steady round
        sub = tc.plan(kind, fmt, env, tc.engine_rows(env, kind, fmt), coalesced=True)
        if tpw >= sub.pf:
            assert sub.tiles.max() >= sub.pf and sub.rounds.max() >= 1
        # the all-fraud engine launch: a wave with more than 64 flagged rows (a flush in mid-launch)
        if tpw >= 5:
            assert tc.plan(kind, fmt, env, tc.engine_rows(env, kind, fmt, "engine1_all")).tiles.max() >= 5
    else:
        # (e) a wave with one tile, a wave with two (the prefetch branch goes both ways)
        assert any((p.tiles == 1).any() for p in plans)
        assert any(p.tiles.max() >= 2 for p in plans)
        assert all(p.pf == 1 and p.waves == min(int(env["CCFD_MLP_WAVES"]), 4) for p in plans)


def test_big_case_exceeds_the_grid_caps():
    """Configuration 1: all four row paths run past their grid cap at BIG_N (the grid-stride loop,
    and the only steady rounds of the LR ring at TPW 1); configuration 2: the register-weight
    kernel past its 2048 workgroups, every wave with a steady round."""
    env = tc.CONFIGS[1]["env"]
    want = {("mlp", "f32"): 4096, ("mlp", "f32s"): 4096, ("mlp", "w64"): 4096,
            ("lr", "f32"): 2048, ("lr", "f32s"): 2048, ("lr", "w64"): 1024}
    for (kind, fmt), cap in want.items():
        p = tc.plan(kind, fmt, env, tc.BIG_N)
        assert p.ntiles == 4100 > p.grid * p.waves and p.grid == cap and p.tiles.max() >= 2 and p.partial
    assert tc.plan("lr", "w64", env, tc.BIG_N).rounds.max() == 1
    p = tc.plan("mlp", "w64", tc.CONFIGS[2]["env"], tc.BIG_N)
    assert (p.kernel, p.pf, p.grid) == ("mlp_wire_reg", 2, 2048) and p.rounds.min() >= 1
    assert [c for c in tc.CONFIGS if tc.CONFIGS[c]["big"]] == [1, 2]


def test_configurations_select_every_branch_of_the_ring():
    """Over the nine configurations the single W64 launches select: the scalar steady loop (MLP
    PF 1, LR PF 2 and 8), the pair loop (register weights at PF 2, LDS weights at PF 2), the quad
    epilogue on register weights, on LDS weights and on the LR scorer, 1-, 2-, 4-, 8- and 16-wave
    groups; the f32 launches both weight sources; the coalesced launches PF 1, 2 and 4."""
    single = {(p.kernel, p.waves, p.pf) for c in tc.CONFIGS.values() for k in tc.KINDS
              for p in [tc.plan(k, "w64", c["env"], 4096)]}
    assert {(k, pf) for k, _, pf in single} == {("mlp_wire", 1), ("mlp_wire", 2), ("mlp_wire", 4),
                                               ("mlp_wire_reg", 2), ("mlp_wire_reg", 4),
                                               ("lr_wire", 2), ("lr_wire", 4), ("lr_wire", 8)}
    assert ("mlp_wire_reg", 8, 2) in single
    assert {w for k, w, _ in single if k.startswith("mlp")} == {1, 2, 4, 8, 16}
    assert {tc.plan("mlp", "w64", c["env"], 4096, coalesced=True).pf for c in tc.CONFIGS.values()} == {1, 2, 4}
    assert {tc.plan("mlp", "f32", c["env"], 4096).waves for c in tc.CONFIGS.values()} == {1, 2, 4}


def test_case_lists():
    """At most a few hundred launches a child, every case of every configuration has a default twin, and
    hostile rows hold every amount x time pair and no NaN."""
    keys = tc.default_cases()
    for cfg in tc.CONFIGS.values():
        cs = tc.cases(cfg)
        assert len(cs) == len(set(cs)) and 50 < len(cs) < 400
        assert all(tc.case_key(c) in keys for c in cs)
        assert sum(c[2] == tc.BIG_N for c in cs) == (6 if cfg["big"] else 0)
        assert {c[3] for c in cs} == {"plain", "rules", "all", "none", "hostile"} | set(tc.ENGINE_MODES)
    # the rule set is test_rules_gpu.py's RULES3, word for word
    assert 'RULES3 = """' + tc.RULES3 + '"""' in open(os.path.join(ROOT, "tests", "test_rules_gpu.py")).read()
    H = tc.hostile_rows()
    assert np.isfinite(H).all() and len(H) == tc.HOSTILE_ROWS
    assert {(a, t) for a, t in zip(H[:8, 29].tolist(), H[:8, 0].tolist())} == \
        {(float(a), float(t)) for a in tc.HOSTILE_AMOUNTS for t in tc.HOSTILE_TIMES}
