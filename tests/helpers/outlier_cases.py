"""Fixtures shared by tests/test_outlier_cpu.py and tests/test_outlier_gpu.py: the integer
autoencoder whose wire path is exact, the real-valued cases of the numerics test, and the edge rows."""
import numpy as np

from ccfd_demo_summit_amd.contracts.transaction import AMOUNT_COL, TIME_COL, encode_wire
from ccfd_demo_summit_amd.models.common import Normalizer
from ccfd_demo_summit_amd.models.outlier import OutlierAE

SIZES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 1025, 5000)
INT_LATENTS = (1, 16, 17, 32)
NUMERIC_CASES = [(8, True), (8, False), (32, True), (32, False)]      # (latent, log_amount)


def _sparse(rng, rows, cols, nnz):
    """{-1, 0, 1} matrix with ``nnz`` non-zeros a row at random columns and random signs: no two
    rows or columns alike, so a swapped row / column or a wrong k-permutation changes the result
    (layer 2 is the densest: even a latent of one unit then sees the k columns ``pi`` exchanges)."""
    W = np.zeros((rows, cols), np.float32)
    for r in range(rows):
        idx = rng.choice(cols, size=min(nnz, cols), replace=False)
        W[r, idx] = rng.choice([-1.0, 1.0], size=idx.size)
    return W


def integer_model(latent: int, seed: int = 0) -> OutlierAE:
    """Identity normaliser, ``log_amount`` off, weights and biases in {-1, 0, 1}: on small-integer
    rows every pre-rounding activation is an integer of magnitude <= 256, so bf16 rounding is the
    identity and fp32 sums are exact in any order."""
    rng = np.random.default_rng(1000 + 31 * latent + seed)
    ints = lambda k: rng.integers(-1, 2, k).astype(np.float32)
    return OutlierAE(_sparse(rng, 64, 30, 4), ints(64), _sparse(rng, latent, 64, 12), ints(latent),
                     _sparse(rng, 64, latent, 3), ints(64), _sparse(rng, 30, 64, 3), ints(30),
                     Normalizer.identity(), threshold=float(40 + latent))


def integer_rows(n: int = 5000, seed: int = 3) -> np.ndarray:
    """W64 rows of integers in [-2, 2] (Time and Amount in [0, 4])."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-2, 3, (n, 30)).astype(np.float32)
    X[:, TIME_COL] = rng.integers(0, 5, n)
    X[:, AMOUNT_COL] = rng.integers(0, 5, n)
    return encode_wire(X)


def numeric_model(X: np.ndarray, latent: int, log_amount: bool) -> OutlierAE:
    """He-init autoencoder with the normaliser fitted on ``X``."""
    return OutlierAE.random_init(latent, seed=latent, norm=Normalizer.fit(X, log_amount=log_amount))


def numeric_rows():
    """``generate(20000, seed=7)[:5000]``: the float rows and their W64 encoding."""
    from ccfd_demo_summit_amd.data import generate
    X = generate(20000, seed=7)[0][:5000]
    return X, encode_wire(X)


def edge_case_rows():
    """W64 rows poked bit by bit as tests/test_drift_wire_gpu.py::edge_case_rows does (every other
    feature 0.25): NaN, +-inf, +-0 and the smallest denormals, in a bf16 column and in the two f32
    ones.  Returns ``(rows, nonfinite bool [k])``."""
    cases = []
    for j in (3, TIME_COL, AMOUNT_COL):
        sh = 0 if j in (TIME_COL, AMOUNT_COL) else 16
        cases += [(j, b, k < 4) for k, b in enumerate((0x7FC00000 >> sh, 0xFFC00000 >> sh, 0x7F800000 >> sh,
                                                        0xFF800000 >> sh, 0x80000000 >> sh, 0, 1,
                                                        (0x80000000 >> sh) + 1))]
    rows = encode_wire(np.full((len(cases), 30), 0.25, np.float32))
    for r, (j, bits, _) in enumerate(cases):
        if j in (TIME_COL, AMOUNT_COL):
            rows[r].view(np.uint32)[14 if j == TIME_COL else 15] = bits
        else:
            rows[r].view(np.uint16)[j - 1] = bits
    return rows, np.array([c[2] for c in cases])
