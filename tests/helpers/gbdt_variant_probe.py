"""Child process of test_gbdt_edges_gpu.py::test_f32_v2_kernel_every_depth_and_tree_count.

The f32 GBDT launch reads CCFD_GBDT_KERNEL and CCFD_GBDT_R once per process, so the rows-in-
registers kernel (score_gbdt.hip v2) below 262144 rows, and its R = 1 form at any size, can only be
reached from a fresh process that has them in its environment (the parent sets them).  Scores
depths 1..8 x trees {1, 3, 5, 8}, and each depth's probe tree (reported as 0 trees), on the
ensemble's edge rows at every row count and prints one JSON line per launch; a case starts only
after the previous one synchronised without a HIP error (an exception ends the process with a
non-zero status).  "crc" is the CRC-32 of the launch's probabilities: nothing tells which kernel
a launch took, so the parent compares it with its own v1 launch (the two kernels add the trees
in different orders).  Judging is the parent's."""
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    import torch
    from ccfd_demo_summit_amd.ops.kernels import DeviceModel, new_counters, score
    from tests.helpers import gbdt_edges as ge
    dev = torch.device("cuda", 0)
    print(json.dumps({"kernel": os.environ.get("CCFD_GBDT_KERNEL"), "R": os.environ.get("CCFD_GBDT_R")}), flush=True)
    cases = 0
    for depth in ge.DEPTHS:
        for trees in (0,) + ge.TREES:                       # 0: the one-tree probe of that depth
            m, X, ref = ge.shape_case(trees, depth) if trees else ge.probe_case(depth)
            dm = DeviceModel(m, dev)
            for n in ge.ROW_COUNTS:
                i = ge.take(len(X), n)
                cnt = new_counters(dev)
                p, r = score(dm, torch.from_numpy(X[i]).to(dev), 0.5, counters=cnt)
                torch.cuda.synchronize(dev)                 # raises on a HIP error: nothing runs after it
                p = p.cpu().numpy()
                j = ge.judge(p, r.cpu().numpy(), cnt.cpu().numpy(), ref[i], X[i])
                j.update(depth=depth, trees=trees, n=n, crc=zlib.crc32(p.tobytes()))
                print(json.dumps(j), flush=True)
                cases += 1
    print(json.dumps({"done": cases}), flush=True)


if __name__ == "__main__":
    main()
