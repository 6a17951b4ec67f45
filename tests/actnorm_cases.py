"""Inputs of the ActNorm fixtures (tests/golden/make_golden_actnorm.py) and of the tests that read them: integer-hash arithmetic, so that
the generator and a test on any machine and any numpy version build the same fp32 values.  The large case is rebuilt from here
instead of stored (the fixture keeps a per-channel checksum of it)."""
import numpy as np

#: name -> (shape, per-channel offset scale, smallest per-channel std)
CASES = {
    "actnorm_B6_C5_7x3": ((6, 5, 7, 3), 1.0, 0.5),                       # HW odd: the dword form
    "actnorm_B4_C12_8x8": ((4, 12, 8, 8), 1.0, 0.5),                     # the 16-byte form
    "actnorm_B64_C12_16x16_cancel": ((64, 12, 16, 16), 1000.0, 0.01),    # offsets up to 1000, std down to 0.01: the cancellation case
    "actnorm_B3_C4_1x1": ((3, 4, 1, 1), 1.0, 0.5),
}
#: the case whose activation-sized arrays are not stored whole: images kept in the fixture
BIG = "actnorm_B64_C12_16x16_cancel"
BIG_IMAGES = (0, 63)


def uniform(n, salt):
    """n values in [-0.5, 0.5), exact in float64: a multiplicative hash of the index."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B1)
    h = (i * np.uint64(2654435761) + (i >> np.uint64(7)) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    return h.astype(np.float64) / 4294967296.0 - 0.5


def inputs(name):
    """x, gy [B,C,H,W] and gl [B] as fp32 arrays: x has per-channel means offset * linspace(-1, 1, C) and standard deviations from
    min_std to 2 (geometric), each channel the sum of three uniforms (bell-shaped, bounded)."""
    shape, offset, min_std = CASES[name]
    B, C, H, W = shape
    n = B * C * H * W
    u = (uniform(n, 1) + uniform(n, 2) + uniform(n, 3)) * 2.0            # variance 3/12 * 4 = 1
    mean = offset * (np.linspace(-1.0, 1.0, C) if C > 1 else np.zeros(1))
    std = np.geomspace(min_std, 2.0, C)
    x = (u.reshape(shape) * std.reshape(1, C, 1, 1) + mean.reshape(1, C, 1, 1)).astype(np.float32)
    gy = (uniform(n, 4) * 3.0).reshape(shape).astype(np.float32)
    gl = (uniform(B, 5) * 3.0).astype(np.float32)
    return x, gy, gl
