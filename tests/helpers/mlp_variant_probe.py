"""Child process of test_mlp_variants_gpu.py.

The MLP / LR launch code reads CCFD_MLP_WAVES, CCFD_MLP_PF, CCFD_MLP_REGW, CCFD_MLP_TPW,
CCFD_MLP_WEIGHTS, CCFD_LR_WAVES, CCFD_LR_PF and CCFD_LR_OCC once per process, so every kernel
instantiation but the defaults can only be reached from a fresh process that has them in its
environment (the parent sets them).  argv[1] names the configuration of tile_cases.CONFIGS; the
process echoes the eight knobs as it sees them, scores every case of tile_cases.cases() -- plain,
rule-routed, all-fraud and no-fraud launches on contiguous f32, strided f32 and W64 rows, the
hostile rows, and engine launches with coalesce 1 and 4 -- and prints one JSON line of figures
per case, then {"done": N}.  A case starts only after the previous one synchronised without a
HIP error (an exception ends the process with a non-zero status).  Nothing tells which kernel a
launch took: "crc_p" / "crc_r" are the CRC-32 of the case's probability and route bytes, which
the parent compares with its own default-variant launch.  Judging is the parent's."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    import torch
    from tests.helpers import tile_cases as tc
    cfg = tc.CONFIGS[int(sys.argv[1])]
    print(json.dumps({k: os.environ.get(k) for k in tc.KNOBS}), flush=True)
    dev = torch.device("cuda", 0)
    run = tc.Runner(dev)
    done = 0
    for case in tc.cases(cfg):
        j = run.run(case)
        torch.cuda.synchronize(dev)                         # raises on a HIP error: nothing runs after it
        sys.stdout.flush()                                  # check()'s own lines stay in order
        print(json.dumps(j), flush=True)
        done += 1
    print(json.dumps({"done": done}), flush=True)


if __name__ == "__main__":
    main()
