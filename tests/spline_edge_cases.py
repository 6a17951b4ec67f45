"""Edge cases of the rational-quadratic spline shared by tests/test_spline_edges_host.py and tests/test_gpu_spline_edges.py (not
collected): inputs that sit ON a knot and one ulp beside it, tables in which a steep bin lies next to a flat one, and the ragged and
multi-trip launches with their plans written out by hand from the rule of tests/spline_cases.py.

Every value is fp32 and every table is the fp32 table the kernels read; a float64 reference reads the same numbers and so chooses
the same bin by exact comparison -- a knot input is a knot input in every precision."""
import numpy as np
import torch

import spline_twin as st
from spline_cases import bins_of

TAIL = 3.0
KNOT_SHAPE = (2, 3, 5, 7)                      # N = 105: thirds of 35 positions, each longer than the 17 knots of K = 16
SPECIALS = (-0.0, float("inf"), float("-inf"), float(np.float32(2.0 ** -149)))    # the last four positions of image 1


def knots_of(table, inverse):
    """[K + 1, P]: the cumwidths (the cumheights for the reverse) of a knot table [3 (K + 1), P]."""
    K = table.shape[0] // 3 - 1
    return table[K + 1:2 * (K + 1)] if inverse else table[:K + 1]


def lines_per_element(v, table, input_size, tail_bound, inverse):
    """`spline_twin.lines_on_table` without the sum: (out, the forward map's log-derivative per element)."""
    from fincflow_amd import glow
    K, P = table.shape[0] // 3 - 1, table.shape[1]
    shape = (K + 1,) if P == 1 else (1, *input_size, K + 1)
    cw, ch, d = (table[a * (K + 1):(a + 1) * (K + 1)].t().reshape(shape) for a in range(3))
    return glow.rq_spline_lines(v, cw, ch, d, tail_bound, inverse)


def knot_plan(N, K):
    """Per position n of image 1: (knot k = n mod (K + 1), variant) with variant 0 = the knot exactly (first third of the positions),
    -1 = one ulp below (second third; knot 0: above), +1 = one ulp above (last third; knot K: below).  The last four positions hold
    SPECIALS instead (variant None)."""
    plan = []
    for n in range(N):
        k, third = n % (K + 1), min(2, 3 * n // N)
        step = (0, -1, 1)[third]
        if (k == 0 and step < 0) or (k == K and step > 0):
            step = -step
        plan.append((k, None if n >= N - len(SPECIALS) else step))
    return plan


def knot_inputs(table, shape, tail_bound, inverse, seed=7):
    """`spline_twin.inputs` with image 1 replaced: position n holds knot n mod (K + 1) of ITS OWN table row (row 0 with shared
    weights) exactly, one ulp below or one ulp above (`knot_plan`), and the last four positions -0.0, +inf, -inf and the smallest
    subnormal.  Image 0 keeps +-tail_bound (the end knots), 0, +-1.2 tail_bound and its spread over the range."""
    x = st.inputs(shape, tail_bound, seed)
    assert shape[0] >= 2 and table.dtype == torch.float32 and x.dtype == torch.float32
    flat = x.view(shape[0], -1)
    N, P = flat.shape[1], table.shape[1]
    K = table.shape[0] // 3 - 1
    knots = knots_of(table, inverse)
    up, down = torch.tensor(float("inf")), torch.tensor(float("-inf"))
    for n, (k, step) in enumerate(knot_plan(N, K)):
        if step is None:
            flat[1, n] = SPECIALS[n - (N - len(SPECIALS))]
            continue
        v = knots[k, n if P > 1 else 0]
        flat[1, n] = v if step == 0 else torch.nextafter(v, up if step > 0 else down)
    return x


#: name -> (shape, n_bins, individual_weights, seed, tail_bound, scale of the randn parameters): a softmax of 3 or 6 x randn puts a
#: bin of a few thousandths of the range next to one that takes most of it.  `indiv_k8_s3` is the case in which the fp32 lines,
#: before the root was clamped, returned a NaN log-det from y one ulp below an inner knot (a bin with w = 6.1e-3, h = 5.67, d0 = 3.56,
#: d1 = 0.233: root 1 + 1.2e-4); `shared_k5_s6` the same with shared weights.
STEEP_FLAT = {
    "indiv_k8_s3": (KNOT_SHAPE, 8, True, 108, TAIL, 3.0),
    "shared_k5_s6": (KNOT_SHAPE, 5, False, 105, TAIL, 6.0),
    "indiv_k9_s6": (KNOT_SHAPE, 9, True, 109, TAIL, 6.0),
    "shared_k16_s3": (KNOT_SHAPE, 16, False, 116, TAIL, 3.0),
}


def steep_flat_tables(name):
    """(shape, K, tail_bound, the fp32 knot table [3 (K + 1), P]) of a STEEP_FLAT case."""
    shape, K, individual, seed, tail_bound, scale = STEEP_FLAT[name]
    return shape, K, tail_bound, st.table_of(st.unit_scale_layer(shape[1:], K, tail_bound, individual, seed, scale=scale))


def rows64(table, inverse_knots):
    """The chosen knot array as numpy float64 [P, K + 1] (what spline_cases.bins_of takes)."""
    return knots_of(table, inverse_knots).double().t().contiguous().numpy()


def bin_ends(v, table, tail_bound, search_heights, ends_heights):
    """Per element of v [B, ...]: (knot[bin], knot[bin + 1]) as float64 tensors -- the bin by spline_cases.bins_of among the float64
    values of the searched knots (`search_heights`: the cumheights, as the reverse searches), the ends from the cumwidths or
    (`ends_heights`) the cumheights."""
    K, B = table.shape[0] // 3 - 1, v.shape[0]
    bins = np.clip(bins_of(v.numpy(), rows64(table, search_heights), tail_bound), 0, K - 1).reshape(B, -1)
    ends = np.broadcast_to(rows64(table, ends_heights), (bins.shape[1], K + 1))
    lo, hi = (np.take_along_axis(ends, bins.T + o, axis=1).T.reshape(v.shape).copy() for o in (0, 1))
    return torch.from_numpy(lo), torch.from_numpy(hi)


SWEEP = 256


def consecutive_heights(table):
    """For a shared table (P = 1): [1, 1, 2 K - 1, SWEEP] fp32, row by row SWEEP CONSECUTIVE floats in rising order -- around every
    inner cumheight (the knot between two bins: rows 0 .. K - 2) and around every bin's mid-height ch0 + h / 2, where the inverse
    changes from the solve at the lower knot to the one at the upper knot (rows K - 1 .. 2 K - 2)."""
    K = table.shape[0] // 3 - 1
    assert table.shape[1] == 1 and table.dtype == torch.float32
    ch = knots_of(table, True)[:, 0]
    centres = [ch[k] for k in range(1, K)] + [ch[j] + (ch[j + 1] - ch[j]) * 0.5 for j in range(K)]
    rows = []
    for c in centres:
        bits = int(c.reshape(1).view(torch.int32)) + torch.arange(-SWEEP // 2, SWEEP // 2, dtype=torch.int32)
        rows.append(bits.view(torch.float32).sort()[0])                             # (a negative float's bits fall as it rises)
    return torch.stack(rows).view(1, 1, len(rows), SWEEP)


#: the ragged and multi-trip launches, K = 2: shape -> what a spline call on it launches, by hand from spline_cases.spline_plan's
#: rule (blocks = ceil(C HW / 256); Q = min(B, ceil(2048 / blocks)); trips = ceil(B / Q))
LAUNCH_PLANS = {
    # N = 429 = 256 + 2 * 64 + 45: a ragged second block whose wave 3 has no valid lane (it still writes its log-det partial)
    (2, 3, 11, 13): dict(io=1, threads=256, grid=4, parts=2, items=512, trips=1, outer=2, lds=0),
    # B = 1, so Q = 1: per-position grad_table is written from the walk, without the reduce; with P = 1 the reduce adds two partials
    (1, 3, 11, 13): dict(io=1, threads=256, grid=2, parts=1, items=256, trips=1, outer=2, lds=0),
    # N = 15: with P = N, T = 3 * 3 * 15 = 135 table entries, an odd count for the pair reduce
    (2, 1, 3, 5): dict(io=1, threads=256, grid=2, parts=2, items=512, trips=1, outer=1, lds=0),
    # N = 262143 (odd): 1024 blocks, the last with 255 valid lanes; 5 images over 2 parts: three trips, part 1's third missing;
    # T = 9 * 262143 odd, with partials
    (5, 1, 511, 513): dict(io=1, threads=256, grid=2048, parts=2, items=1280, trips=3, outer=1024, lds=0),
}
THREE_TRIPS = (5, 1, 511, 513)
DIRECT_GRAD_TABLE = (1, 3, 11, 13)
