"""Test data and reference expressions shared by tests/test_pca_cpu.py and tests/test_gpu_pca.py (no test in here)."""
import numpy as np

SHAPES = ((32, 250), (96, 1000), (384, 4104), (1024, 2056))     # where the properties in planted_int's docstring were checked


def planted_int(F, n, seed):
    """Integer-valued [F][n] float64 data with a planted spectrum:
        clip(rint(1.5 sqrt(F) U diag(0.7^i, i < 8) W + 0.3 noise + integer column offsets in -2..2), -8, 8)
    U orthonormal F x 8, W standard normal 8 x n.  Every value is an integer of magnitude <= 8, so every product is <= 64 and
    any fp32 summation order over n <= 262144 voxels is exact (64 n < 2^24): a Gram matrix computed with fp32 accumulation must
    equal the integer result bit for bit.  At SHAPES: under 1 % of the values are clipped and the relative gaps of the top 6
    eigenvalues of the covariance are at least 0.39 (tests/test_pca_cpu.py checks both)."""
    return np.clip(np.rint(raw_planted(F, n, seed)), -8, 8)


def raw_planted(F, n, seed):
    """planted_int before rounding and clipping: for the clipped-fraction check."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((F, 8)))
    W = rng.standard_normal((8, n))
    return 1.5 * np.sqrt(F) * (U * 0.7 ** np.arange(8)) @ W + 0.3 * rng.standard_normal((F, n)) + rng.integers(-2, 3, size=(F, 1))


def ulp_fp16(y):
    """Spacing of fp16 at |y| (2^-24 in the subnormal range), elementwise, float64."""
    e = np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def project_bound(comp, x, offset, y):
    """Per-output error bound of vittf_feature_project against the fp64 value y = comp @ x - offset:
        0.5 ulp_fp16(y)                                             the single rounding of the result
      + (F + 8) 2^-24 (sum_f |v_kf x_fv| + |offset_k|)              worst-case fp32 accumulation in any order, plus the 2^-22 of
                                                                    the fp16 hi + lo split of the components
      + 2^-25 sum_f |x_fv|                                          a lo half below the fp16 subnormal spacing
    comp [k][F], x [F][n], offset [k], all float64."""
    F = x.shape[0]
    return (0.5 * ulp_fp16(y) + (F + 8) * 2.0 ** -24 * (np.abs(comp) @ np.abs(x) + np.abs(offset)[:, None])
            + 2.0 ** -25 * np.abs(x).sum(0)[None, :])
