"""Every env-selected MLP / LR launch variant against the oracle and against the default variant.

CCFD_MLP_WAVES / _PF / _REGW / _TPW / _WEIGHTS and CCFD_LR_WAVES / _PF / _OCC (docs/TUNING.md)
select among about fifty instantiations of score_mlp.hip and score_lr.hip and are read once per
process, so each configuration of tile_cases.CONFIGS is scored by a child process
(helpers/mlp_variant_probe.py) that has the knobs in its environment; this test judges every line
the child printed.  The row counts come from tile_cases.plan() (test_mlp_variants_cpu.py proves
that they reach every loop of the selected kernels); no verdict does.

Per case: the oracle at the suite's tolerances (W64 MLP 2e-4 of wire_proba, f32 MLP 2e-3 of the
bf16-emulating model and 1e-2 of fp32, LR 1e-5), routes equal to the host's (threshold or
RuleSet.evaluate), everything tile_cases.check asserts (counters, both histograms per bucket, the
proba sum; on engine launches the flag list as a set without duplicates), and identity: the CRC-32
of the probability bytes and of the route bytes equals that of this process's default-variant
launch on the same rows.  A row's probability cannot depend on a knob: its tile and column are
row / 16 and row % 16 under every tiling, an MFMA output column depends on its own input column
only, and every variant of a row format runs one operation sequence (mlp_tile; mlp_tile_w64 =
logit2 + mlp_proba_of_logit; lr_proba; LrWireScorer::logit + proba).  Because the variants are
bit-identical nothing in the outputs tells which kernel a launch took; the test checks the
environment the child echoes, and the selection code is covered only in the sense that it runs."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests.helpers import tile_cases as tc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_CHILD_FAILED = []                  # configurations whose child ended non-zero or timed out: no child after one


@pytest.fixture(scope="module")
def defaults(gpu):
    """The figures of every case of every configuration under the default variant (this process
    has none of the knobs), by tile_cases.case_key -- computed once, read-only."""
    assert not [k for k in tc.KNOBS if k in os.environ], "this process must select the default kernels"
    run = tc.Runner(gpu)
    return {key: run.run(case, default=True) for key, case in tc.default_cases().items()}


def test_default_variant_passes_every_case(defaults):
    """What the variants are compared with is itself right on these rows."""
    bad = [(key, tc.judge(j)) for key, j in defaults.items() if tc.judge(j)]
    assert not bad, f"{len(bad)} of {len(defaults)} default launches, first {bad[:6]}"


@pytest.mark.parametrize("cfg", list(tc.CONFIGS))
def test_variant_equals_oracle_and_default(gpu, defaults, cfg):
    if _CHILD_FAILED:
        pytest.skip(f"the child of configuration {_CHILD_FAILED[0]} ended with an error: nothing more is started")
    knobs = tc.CONFIGS[cfg]["env"]
    want = tc.cases(tc.CONFIGS[cfg])
    # child: interpreter + torch + HIP start-up (tens of seconds at worst), the fixture (~1 s),
    # at most 160 launches of <= 1801 rows and 6 of 65589 (milliseconds each), 18 small engines
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "mlp_variant_probe.py"), str(cfg)],
                           env=dict(os.environ, **knobs), capture_output=True, text=True, timeout=150)
    except subprocess.TimeoutExpired:
        _CHILD_FAILED.append(cfg)
        raise
    print(f"configuration {cfg} {knobs}: child took {time.perf_counter() - t0:.1f} s")
    print(r.stdout[-3000:], r.stderr[-4000:])
    if r.returncode != 0:
        _CHILD_FAILED.append(cfg)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert lines[0] == knobs
    assert lines[-1] == {"done": len(want)}
    got = lines[1:-1]
    assert [(j["kind"], j["fmt"], j["n"], j["mode"]) for j in got] == want
    bad = []
    for case, j in zip(want, got):
        why = tc.judge(j)
        d = defaults[tc.case_key(case)]
        if "crc_p" in j:
            if j["crc_p"] != d["crc_p"]:
                why.append("probabilities differ from the default variant's")
            if j["crc_r"] != d["crc_r"]:
                why.append("routes differ from the default variant's")
        if why:
            bad.append((case, why, {k: j.get(k) for k in ("err", "err32", "fraud")}, {"default err": d.get("err")}))
    print("failing cases:", *bad, sep="\n")
    assert not bad, f"{len(bad)} of {len(got)} cases, first {bad[:4]}"
