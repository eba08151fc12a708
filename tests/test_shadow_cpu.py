"""Shadow (challenger) scoring, host side: ABI mirrors, the pair check, the counter summary,
the Prometheus series and the launch setting.  The kernels are covered by test_shadow_gpu.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).parent / "golden"


def test_abi_struct_sizes_and_slots(tmp_path):
    from ccfd_demo_summit_amd.ops import _lib
    from ccfd_demo_summit_amd.ops.build import CSRC
    assert [_lib.CNT_SHADOW_ROWS, _lib.CNT_SHADOW_FRAUD, _lib.CNT_SHADOW_BOTH, _lib.CNT_SHADOW_PROBA_E6,
            _lib.CNT_SHADOW_ABSDIFF_E6] == [40, 41, 42, 43, 44]
    # the existing kernels' argument block leads the new one unchanged
    assert _lib.ShadowArgs.base.offset == 0 and _lib.ShadowArgs.shadow_blob.offset == C.sizeof(_lib.ScoreArgs)
    assert _lib.PersistShadowArgs.shadow_blob.offset == C.sizeof(_lib.PersistArgs)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ccfd_abi.h"\nint main(){printf("%zu %zu %zu %d %d %d %d %d",'
                   'sizeof(ccfd_shadow_args),sizeof(ccfd_persist_shadow_args),sizeof(ccfd_persist_args),'
                   'CCFD_CNT_SHADOW_ROWS,CCFD_CNT_SHADOW_FRAUD,CCFD_CNT_SHADOW_BOTH,'
                   'CCFD_CNT_SHADOW_PROBA_E6,CCFD_CNT_SHADOW_ABSDIFF_E6);}\n')
    exe = tmp_path / "sz"
    r = subprocess.run(["gcc", str(src), "-I", str(CSRC / "include"), "-o", str(exe)], capture_output=True)
    if r.returncode != 0:
        pytest.skip("no C compiler")
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert out[:3] == [C.sizeof(_lib.ShadowArgs), C.sizeof(_lib.PersistShadowArgs), C.sizeof(_lib.PersistArgs)]
    assert out[3:] == [40, 41, 42, 43, 44]


def _dm(kind, wire=False, nbytes=None):
    from ccfd_demo_summit_amd.models.mlp import BLOB_BYTES, WIRE_BLOB_BYTES
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel
    if nbytes is None:
        nbytes = WIRE_BLOB_BYTES if wire else BLOB_BYTES
    return DeviceModel.from_blob(kind, torch.zeros(nbytes, dtype=torch.uint8), trees=4 if kind != "mlp" else 0,
                                 depth=3 if kind != "mlp" else 0, wire=wire)


def test_check_shadow_pair():
    from ccfd_demo_summit_amd.ops.kernels import check_shadow_pair
    a, b = _dm("mlp", wire=True), _dm("mlp", wire=True)
    check_shadow_pair(a, b)
    check_shadow_pair(a, b, rules=None, persist_items=1)
    msgs = []

    def refused(*args, **kw):
        with pytest.raises(ValueError) as e:
            check_shadow_pair(*args, **kw)
        msgs.append(str(e.value))
        return str(e.value)

    assert "champion MLP is packed for f32" in refused(_dm("mlp"), b)
    assert "shadow MLP is packed for f32" in refused(a, _dm("mlp"))
    for kind in ("lr", "gbdt", "forest"):
        m = refused(_dm(kind, wire=kind == "lr"), _dm(kind, wire=kind == "lr"))
        assert repr(kind) in m and "no shadow kernel" in m
    m = refused(_dm("lr", wire=True), b)
    assert "kind mismatch" in m and "'lr'" in m and "'mlp'" in m
    assert "kind mismatch" in refused(a, _dm("gbdt"))
    assert "routing rules" in refused(a, b, rules=object())
    assert "pipelined" in refused(a, b, persist_items=2)
    assert "27968-byte" in refused(a, _dm("mlp", wire=True, nbytes=25920))
    assert len(set(msgs)) == len(msgs)           # every combination has its own message


def test_shadow_counters():
    from ccfd_demo_summit_amd.engine import StreamEngine
    c = np.zeros(64, np.int64)
    c[0], c[1], c[2], c[3] = 1000, 30, 970, 123_000_000
    z = StreamEngine.shadow_counters(c)
    assert z == {"rows": 0, "fraud": 0, "both": 0, "disagree": 0, "mean_proba": 0.0, "mean_abs_diff": 0.0}
    c[40:45] = [1000, 50, 20, 250_000_000, 40_000_000]
    s = StreamEngine.shadow_counters(torch.from_numpy(c))
    assert (s["rows"], s["fraud"], s["both"], s["disagree"]) == (1000, 50, 20, 30 + 50 - 2 * 20)
    assert s["mean_proba"] == pytest.approx(0.25) and s["mean_abs_diff"] == pytest.approx(0.04)


def _exposition(cnt):
    from prometheus_client import CollectorRegistry, generate_latest

    from ccfd_demo_summit_amd.metrics.exporter import GpuEngineCollector
    lat = np.zeros(256, np.int64)
    lat[60:64] = [5, 9, 3, 1]
    reg = CollectorRegistry()
    reg.register(GpuEngineCollector(lambda: (cnt, lat, {"tx_per_second": 8.5e8, "handoff_dead_letter_total": 2}),
                                    rank_label="0"))
    return generate_latest(reg).decode()


def _counters():
    c = np.zeros(64, np.int64)
    c[0], c[1], c[2], c[3], c[4] = 14288, 122, 14166, 7_100_000_000, 0
    c[8:22] = np.arange(14) * 7 + 3
    c[24:38] = np.arange(14)
    return c


def test_exporter_shadow_series_only_with_a_shadow():
    c = _counters()
    base = _exposition(c)
    assert "shadow" not in base
    # recorded from the collector as it was before the shadow series existed, same inputs:
    # without a shadow the exposition is what it was, byte for byte
    assert base == (GOLDEN / "shadow_exposition_baseline.txt").read_text()
    c[40:45] = [14288, 557, 9, 7_200_000_000, 90_000_000]
    text = _exposition(c)
    want = {"ccfd_gpu_shadow_rows_total": 14288.0, "ccfd_gpu_shadow_fraud_total": 557.0,
            "ccfd_gpu_shadow_both_fraud_total": 9.0, "ccfd_gpu_shadow_proba_sum": 7200.0,
            "ccfd_gpu_shadow_abs_diff_sum": 90.0}
    got = {}
    rest = []
    for line in text.splitlines(keepends=True):
        if "ccfd_gpu_shadow_" in line:
            if not line.startswith("#"):
                name, value = line.split("{")[0], float(line.rsplit(" ", 1)[1])
                assert 'rank="0"' in line
                got[name] = value
        else:
            rest.append(line)
    assert got == pytest.approx(want) and set(got) == set(want)
    assert "".join(rest) == base                 # nothing else moved


def test_cli_and_config_reach_engine_settings(monkeypatch):
    from ccfd_demo_summit_amd.config import load_config
    from ccfd_demo_summit_amd.launch.__main__ import engine_service_settings, parse_args
    monkeypatch.delenv("CCFD_SHADOW_MODEL", raising=False)
    a = parse_args(["engine", "--shadow-model", "cand.safetensors", "--watch-model", "live.safetensors"])
    assert a.shadow_model == "cand.safetensors"
    s = engine_service_settings(a, load_config(None))
    assert (s.shadow_model, s.model_watch) == ("cand.safetensors", "live.safetensors")
    none = engine_service_settings(parse_args(["engine"]), load_config(None))
    assert none.shadow_model is None
    monkeypatch.setenv("CCFD_SHADOW_MODEL", "env.safetensors")
    cfg = load_config(None)
    assert cfg.engine.shadow_model == "env.safetensors"
    assert engine_service_settings(parse_args(["engine"]), cfg).shadow_model == "env.safetensors"
    assert engine_service_settings(a, cfg).shadow_model == "cand.safetensors"      # the flag wins
