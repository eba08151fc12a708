"""Champion / challenger GBDT pairs for the shadow tests (test_shadow_gbdt_cpu.py,
test_shadow_gbdt_gpu.py): two ensembles of one shape that share a bin table and disagree on
some rows but not on all."""
import numpy as np


def union_spec(a, b, bits=8):
    """Per-feature union of two ensembles' split thresholds as one BinSpec."""
    from ccfd_demo_summit_amd.models.gbdt import BinSpec
    sa, sb = a.bin_spec(), b.bin_spec()
    return BinSpec([np.union1d(x, y).astype(np.float32) for x, y in zip(sa.edges, sb.edges)], bits=bits)


def make_pair(X_ref, trees=100, depth=6, seeds=(3, 4), rates=(0.01, 0.03), bits=8):
    """A = build_model("gbdt", seed=seeds[0]) calibrated to rates[0]; B = A's first half of the
    trees + the second half of the seeds[1] random ensemble, calibrated to rates[1] -- so the
    two score alike but not equally.  Returns (A, B, spec) with spec the union bin table."""
    from ccfd_demo_summit_amd.models import build_model
    from ccfd_demo_summit_amd.models.gbdt import ObliviousGBDT
    A = build_model("gbdt", seed=seeds[0], X_ref=X_ref, calibrate_rate=rates[0], gbdt_trees=trees, gbdt_depth=depth)
    R = build_model("gbdt", seed=seeds[1], X_ref=X_ref, gbdt_trees=trees, gbdt_depth=depth)
    h = trees // 2
    B = ObliviousGBDT(np.concatenate([A.feat[:h], R.feat[h:]]), np.concatenate([A.thr[:h], R.thr[h:]]),
                      np.concatenate([A.leaves[:h], R.leaves[h:]]), 0.0)
    B.calibrate_bias(X_ref, rates[1])
    return A, B, union_spec(A, B, bits=bits)
