"""Shapes, planted inputs, the parameter box and the hand-stated launch plans of the smooth invertible activations' tests (not
collected): shared by tests/golden/make_golden_activations.py, tests/test_activations_host.py and tests/test_gpu_activations.py.

The plans are written out from the rule of finc_activation.h, not read from the library: the tensor is [B][N], N = C * HW; io = 4 when
N % 4 == 0 (whatever HW is) and the pointers are 16-byte aligned, else 1; items = N / io per image; P = min(ceil(items / 256),
ceil(2048 / B)) parts share an image; grid = B * P; trips = ceil(items / (256 * P))."""
import numpy as np

GOLDEN = "activations_reference.npz"
GOLDEN_SHAPE = (3, 2, 4, 5)
#: what every input tensor carries in its first elements: both zeros (the comparison is x < 0 strictly), the two sides of zero, and
#: values where softplus and tanh are saturated
PLANTED = (0.0, -0.0, 1e-6, -1e-6, 30.0, -30.0)

KINDS = ("smooth_leaky_relu", "leaky_relu", "learnable_leaky_relu", "smooth_tanh")
#: the box in which the inverse's accuracy is claimed
BOX = {"smooth_leaky_relu": ((0.01,), (0.1,), (0.3,), (0.9,), (1.0,), (1.5,)),
       "smooth_tanh": ((1.0, 0.1), (3.0, 0.05), (8.0, 0.01), (0.5, 1.0), (0.1, 0.01))}
#: the trip count the sweep of DESIGN 3.26 gives: the worst case of the box is at its floor after 7, plus 2 of margin
CONVERGED_AFTER, TRIPS = 7, 9

#: kernel-test shapes: wide form in one trip; N = 30, dwords; HW odd but N % 4 == 0, wide; a 2-D input
SHAPES = ((2, 3, 4, 4), (3, 2, 3, 5), (2, 4, 3, 5), (4, 37))
#: multi-trip by plan: (shape, alignment of the pointers).  [512, 8, 23, 25] has N = 4600, a multiple of four although HW = 575 is
#: not: on 16-byte pointers it takes the wide form (1150 items, 2 trips), and the 4600 dword items in 5 trips are its plan on pointers
#: two floats into their allocation -- which is how the test runs it.
MULTI_TRIP = (((512, 8, 24, 24), 16), ((512, 8, 23, 25), 8))


def _plan(io, grid, parts, items, trips, outer):
    return dict(io=io, threads=256, grid=grid, parts=parts, items=items, trips=trips, outer=outer, lds=0)


#: (shape, align) -> plan
PLANS = {
    ((2, 3, 4, 4), 16): _plan(4, 2, 1, 12, 1, 2),
    ((2, 3, 4, 4), 8): _plan(1, 2, 1, 48, 1, 2),
    ((3, 2, 3, 5), 16): _plan(1, 3, 1, 30, 1, 3),
    ((3, 2, 3, 5), 8): _plan(1, 3, 1, 30, 1, 3),
    ((2, 4, 3, 5), 16): _plan(4, 2, 1, 15, 1, 2),
    ((2, 4, 3, 5), 8): _plan(1, 2, 1, 60, 1, 2),
    ((4, 37), 16): _plan(1, 4, 1, 37, 1, 4),
    ((4, 37), 8): _plan(1, 4, 1, 37, 1, 4),
    ((512, 8, 24, 24), 16): _plan(4, 2048, 4, 1152, 2, 512),
    ((512, 8, 23, 25), 8): _plan(1, 2048, 4, 4600, 5, 512),
    ((512, 8, 23, 25), 16): _plan(4, 2048, 4, 1150, 2, 512),
}


def dims(shape):
    """(B, C, HW) as the entry points take a tensor of two or more dimensions."""
    return shape[0], shape[1], int(np.prod(shape[2:], dtype=np.int64))


def planted(x):
    """`x` (a numpy array or a tensor, changed in place) with PLANTED in the first elements of image 0."""
    flat = x.reshape(x.shape[0], -1)
    for k, v in enumerate(PLANTED):
        flat[0, k] = v
    return x


def layer(kind, params=()):
    """The glow layer of a kind; `params` empty: the constructor's defaults."""
    from fincflow_amd import glow
    cls = {"smooth_leaky_relu": glow.SmoothLeakyRelu, "leaky_relu": glow.LeakyRelu, "learnable_leaky_relu": glow.LearnableLeakyRelu,
           "smooth_tanh": glow.SmoothTanh}[kind]
    return cls(*params)


def bisect64(layer64, y, steps=200):
    """f^-1(y) of a smooth layer by float64 bisection on the layer's own forward lines (`y` float64): the truth of the inverse tests."""
    import torch
    a = getattr(layer64, "alpha")
    slope = min(a, 1.0) if layer64.kind == "smooth_leaky_relu" else layer64.beta
    lo = -(y.abs() + 1) / slope - 10
    hi = -lo
    for _ in range(steps):
        m = 0.5 * (lo + hi)
        up = layer64._lines(m, False)[0] < y
        lo, hi = torch.where(up, m, lo), torch.where(up, hi, m)
    return 0.5 * (lo + hi)


BAR = 1e-5


def judge(tag, names, got, want, yard, asserting=True, **fields):
    """Every tensor of `got` (the HIP result) against `want` (float64) under max(1e-5, 2 * e_ref), e_ref = `yard` (the layer's fp32
    lines on the CPU) against `want`, all by flow_twin.error; one line per call in the parity report (kind `activations`), every
    figure printed before it is asserted.  `asserting=False`: figures that are reported only (the line says so)."""
    import flow_twin
    from helpers import report
    fields = {("activation" if k == "kind" else k): v for k, v in fields.items()}    # (`kind` is the report's own first field)
    errs = {n: flow_twin.error(g, w) for n, g, w in zip(names, got, want)}
    refs = {n: flow_twin.error(y, w) for n, y, w in zip(names, yard, want)}
    bars = {n: max(BAR, 2 * refs[n]) for n in names}
    report("activations", case=tag, hip=errs, e_ref=refs, bar=bars if asserting else None, reported_only=not asserting, **fields)
    print("activations %s %s: " % (tag, fields or "") + ", ".join("%s HIP %.2e e_ref %.2e" % (n, errs[n], refs[n]) for n in names))
    over = {n: (errs[n], bars[n]) for n in names if not errs[n] <= bars[n]}
    assert not (asserting and over), (tag, fields, over)
    return errs
