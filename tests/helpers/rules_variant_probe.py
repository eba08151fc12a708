"""Child process of test_rule_programs_gpu.py::test_forced_v2_kernel_routes_the_feature_catalogue.

The f32 GBDT launch reads CCFD_GBDT_KERNEL and CCFD_GBDT_R once per process, so the rows-in-
registers kernel (score_gbdt.hip v2) below 262144 rows, and its R = 1 form at any size, can only
be reached from a fresh process that has them in its environment (the parent sets them).  Scores
the full feature catalogue of tests/helpers/rule_cases.py with the depth-3 and the depth-6
ensemble at 1, 65 and 273 rows and prints one JSON line per launch: the failed checks of
rule_cases.launch_problems and the CRC-32 of the launch's probabilities (nothing tells which
kernel a launch took, so the parent compares it with its own v1 launch).  A launch starts only
after the previous one synchronised without a HIP error (an exception ends the process with a
non-zero status).  Judging is the parent's."""
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

MODELS = ("gbdt_d3", "gbdt")                    # depth 3 and depth 6
ROW_COUNTS = (1, 65, 273)


def main():
    import torch
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, DeviceRules, new_counters, score
    from tests.helpers import rule_cases as rc
    dev = torch.device("cuda", 0)
    print(json.dumps({"kernel": os.environ.get("CCFD_GBDT_KERNEL"), "R": os.environ.get("CCFD_GBDT_R")}), flush=True)
    X = rc.rows()["f32"]
    cases = 0
    for kind in MODELS:
        dm = DeviceModel(rc.models()[kind], dev)
        for n in ROW_COUNTS:
            x = torch.from_numpy(X[:n].copy()).to(dev)
            for name, rs in rc.feature_catalogue(kind, "f32").items():
                dr = DeviceRules(rs, dev)
                cnt = new_counters(dev)
                p, r = score(dm, x, 0.5, counters=cnt, rules=dr)
                torch.cuda.synchronize(dev)             # raises on a HIP error: nothing runs after it
                p = p.cpu().numpy()
                bad = rc.launch_problems(rs, p, r.cpu().numpy(), cnt.cpu().numpy(), X[:n], X[:n, 29])
                print(json.dumps({"model": kind, "n": n, "program": name, "problems": bad,
                                  "crc": zlib.crc32(p.tobytes())}), flush=True)
                cases += 1
    print(json.dumps({"done": cases}), flush=True)


if __name__ == "__main__":
    main()
