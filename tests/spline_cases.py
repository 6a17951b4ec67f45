"""Cases of the rational-quadratic spline shared by tests/golden/make_golden_spline.py, tests/test_spline_host.py and
tests/test_gpu_spline.py: the recorded configurations, the knots in numpy float64 (independent of the layer's lines), the inputs
with their planted elements, and -- stated by hand from the launch rule, not read from the library -- what every GPU case launches.

The launch rule of every spline call (include/finc.h FINC_PIXEL_SPLINE): blocks = ceil(C * HW / 256) blocks of positions are the
outer units; a block's items are its 256 lanes times the B images; Q = min(B, ceil(2048 / blocks)) parts share them, a lane of part q
walks the images q, q + Q, ...; trips = ceil(B / Q); dwords whatever the alignment."""
import numpy as np

#: name -> (shape, n_bins, tail_bound, individual_weights): shared and individual weights, K = 5 and 8, tail_bound 10 and 3
CONFIGS = {
    "shared_k5_t10": ((3, 4, 6, 6), 5, 10.0, False),
    "indiv_k5_t10": ((3, 2, 4, 6), 5, 10.0, True),
    "shared_k8_t3": ((2, 3, 5, 5), 8, 3.0, False),
    "indiv_k8_t3": ((3, 2, 4, 6), 8, 3.0, True),
}
GOLDEN = "spline_reference.npz"
MIN_BIN, MIN_DERIVATIVE = 1e-3, 1e-3


def knots64(uw, uh, ud, tail_bound):
    """(cumwidths, cumheights, derivatives), each [P, K + 1] float64, from the unnormalised parameters reshaped to [P, K] / [P, K - 1]:
    rational_quadratic.py:97-115 with the padded end derivatives of :38-46."""
    uw, uh, ud = (np.asarray(a, dtype=np.float64).reshape(-1, np.shape(a)[-1]) for a in (uw, uh, ud))
    K = uw.shape[-1]

    def cumulative(u):
        e = np.exp(u - u.max(axis=-1, keepdims=True))
        part = MIN_BIN + (1 - MIN_BIN * K) * e / e.sum(axis=-1, keepdims=True)
        cum = 2 * tail_bound * np.cumsum(part, axis=-1) - tail_bound
        ends = np.full((len(cum), 1), tail_bound)
        return np.concatenate([-ends, cum[:, :-1], ends], axis=-1)

    padded = np.pad(ud, ((0, 0), (1, 1))) + np.log(np.exp(1 - MIN_DERIVATIVE) - 1)
    return cumulative(uw), cumulative(uh), MIN_DERIVATIVE + np.logaddexp(0.0, padded)


def bins_of(x, cumwidths, tail_bound):
    """Per element of x [B, ...]: its bin among cumwidths [P, K + 1] (P = 1 or one row per position), -1 below the range, K above."""
    B = x.shape[0]
    flat = np.asarray(x, dtype=np.float64).reshape(B, -1)
    cw = np.broadcast_to(cumwidths[None], (B, flat.shape[1] if cumwidths.shape[0] > 1 else 1, cumwidths.shape[1]))
    K = cumwidths.shape[1] - 1
    idx = np.clip((flat[..., None] >= cw[..., :K]).sum(-1) - 1, 0, K - 1)
    return np.where(flat < -tail_bound, -1, np.where(flat > tail_bound, K, idx)).reshape(x.shape)


def planted_inputs(rng, shape, cumwidths, tail_bound):
    """6 * randn in fp32 with, in image 0: exactly +-tail_bound, exactly 0, +-1.2 tail_bound, and at position j the middle of bin j of
    that position's knots (one element inside every bin); fp32 values, so that every precision sees the same numbers."""
    x = (6.0 * rng.standard_normal(shape)).astype(np.float32)
    flat = x.reshape(shape[0], -1)
    K = cumwidths.shape[1] - 1
    for j in range(K):
        row = cumwidths[j if cumwidths.shape[0] > 1 else 0]
        flat[0, j] = np.float32(0.5 * (row[j] + row[j + 1]))
    flat[0, K:K + 5] = np.asarray([tail_bound, -tail_bound, 0.0, 1.2 * tail_bound, -1.2 * tail_bound], dtype=np.float32)
    return x


def spline_plan(B, C, HW):
    """The launch of a spline call on [B][C][HW], by hand: what _lib.pixel_plan("parts", "spline", B, C, HW) must report."""
    blocks = -(-C * HW // 256)
    Q = min(B, -(-2048 // blocks))
    return dict(io=1, threads=256, grid=blocks * Q, parts=Q, items=256 * B, trips=-(-B // Q), outer=blocks, lds=0)


#: the GPU cases' shapes with what they launch, written out (spline_plan above must agree: tests/test_spline_host.py checks both
#: against the library)
PLANS = {
    (2, 3, 4, 4): dict(io=1, threads=256, grid=2, parts=2, items=512, trips=1, outer=1, lds=0),      # 16-byte rows
    (3, 2, 3, 5): dict(io=1, threads=256, grid=3, parts=3, items=768, trips=1, outer=1, lds=0),      # HW = 15
    (4, 12, 4, 4): dict(io=1, threads=256, grid=4, parts=4, items=1024, trips=1, outer=1, lds=0),    # the stack's first level
    (4, 24, 2, 2): dict(io=1, threads=256, grid=4, parts=4, items=1024, trips=1, outer=1, lds=0),    # and its second
    # multi-trip: 1024 blocks leave room for 2 parts, 3 images -> part 0 walks images 0 and 2, part 1 image 1 (a second, partial trip)
    (3, 4, 256, 256): dict(io=1, threads=256, grid=2048, parts=2, items=768, trips=2, outer=1024, lds=0),
    # 2048 blocks fill the chip: one part walks both images, and grad_table is written without partials
    (2, 2, 512, 512): dict(io=1, threads=256, grid=2048, parts=1, items=512, trips=2, outer=2048, lds=0),
}
MULTI_TRIP = ((3, 4, 256, 256), (2, 2, 512, 512))
