"""The spline at its knots, without a GPU: the fp32 PyTorch lines (`glow.rq_spline_lines`) one ulp beside a knot between a steep and
a flat bin -- where a root of the far-knot quadratic leaves [0, 1] and the log-det of a finite in-range input is NaN --, consecutive
floats across knots and mid-heights, the bit facts at an exact knot, the hand-written plans of the ragged and multi-trip GPU launches, and the knot inputs' own coverage."""
import numpy as np
import pytest
import torch

import spline_edge_cases as ec
import spline_twin as st
from spline_cases import bins_of, spline_plan
from fincflow_amd import _lib


def in_range(v, tail_bound):
    return (v >= -tail_bound) & (v <= tail_bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the regression: a steep bin beside a flat one, y one ulp beside the knot between them
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ec.STEEP_FLAT))
def test_fp32_inverse_lines_stay_finite_and_inside_the_bin(name):
    """Every finite in-range input gives a finite x with cw[bin] <= x <= cw[bin + 1] and |x| <= tail_bound, a finite log-det, and
    finite parameter gradients.  (Solved from knot 0 without a clamp, `indiv_k8_s3` has 1 NaN log-det, `shared_k5_s6` 6, `indiv_k9_s6`
    2, and the four cases 2, 5, 10 and 8 elements outside their bin.)"""
    shape, K, tb, table = ec.steep_flat_tables(name)
    y = ec.knot_inputs(table, shape, tb, True)
    inside = in_range(y, tb)
    assert int(inside.sum()) >= y.numel() - shape[0] * y[0].numel() // 2 and not bool(torch.isnan(y).any())
    x, lad = ec.lines_per_element(y, table, shape[1:], tb, True)
    bad = inside & ~(torch.isfinite(x) & torch.isfinite(lad))
    assert not bool(bad.any()), (name, "non-finite x or log-derivative at in-range inputs", y[bad].tolist()[:4], lad[bad].tolist()[:4])
    lo, hi = ec.bin_ends(y, table, tb, True, False)
    xd = x.double()
    out = inside & ~((lo <= xd) & (xd <= hi) & (xd.abs() <= tb))
    assert not bool(out.any()), (name, "x outside its bin", y[out].tolist()[:4], xd[out].tolist()[:4], lo[out].tolist()[:4], hi[out].tolist()[:4])
    assert same(x[~inside], y[~inside]) and not bool(lad[~inside].any())
    # through the layer: the gradients of the three parameters
    case = ec.STEEP_FLAT[name]
    m = st.unit_scale_layer(shape[1:], K, tb, case[2], case[3], scale=case[5])
    assert torch.equal(st.table_of(m), table)
    out, ld = m.reverse_with_logdet(y)
    (torch.where(inside, out, torch.zeros_like(out)).sum() + ld.sum()).backward()
    for p_name, p in m.named_parameters():
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (name, p_name)


def same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", [n for n in sorted(ec.STEEP_FLAT) if not ec.STEEP_FLAT[n][2]])
def test_fp32_inverse_lines_are_monotone_over_consecutive_floats(name):
    """The shared-weight steep/flat tables over `consecutive_heights`: x never falls while y rises float by float, across every knot
    and across every bin's mid-height, where the solve changes knots.  (With -b - sqrt for every sign of b, `shared_k16_s3` fell 140
    times in its three flattest bins, by up to 5e-6, and was 4.4e-5 off float64; it is 3.6e-7 off now.)"""
    shape, K, tb, table = ec.steep_flat_tables(name)
    y = ec.consecutive_heights(table)
    assert bool((y[..., 1:] > y[..., :-1]).all()) and bool((y.abs() <= tb).all())
    x, lad = ec.lines_per_element(y, table, tuple(y.shape[1:]), tb, True)
    assert bool(torch.isfinite(x).all() and torch.isfinite(lad).all())
    falls = x[..., 1:] < x[..., :-1]
    assert not bool(falls.any()), (name, int(falls.sum()), falls.nonzero()[:4].tolist())
    lo, hi = ec.bin_ends(y, table, tb, True, False)
    assert bool(((lo <= x.double()) & (x.double() <= hi)).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. exact knots
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (1.0, 3.0, 6.0))
@pytest.mark.parametrize("individual", (False, True), ids=("P1", "PCHW"))
@pytest.mark.parametrize("K", (2, 5, 8, 9, 16))
def test_an_exact_knot_maps_to_the_other_knot_bit_for_bit(K, individual, scale):
    """Image k holds knot k < K of every position's own row: th = 0 there, every term beside ch0 / cw0 is an exact zero, and the
    fp32 lines return ch[k] from cw[k] (forward) and cw[k] from ch[k] (inverse).  (Knot K is reached from the last bin at th = 1.)"""
    size = ec.KNOT_SHAPE[1:]
    table = st.table_of(st.unit_scale_layer(size, K, ec.TAIL, individual, 200 + K, scale=scale))
    for inverse in (False, True):
        src, dst = (ec.knots_of(table, inverse)[:K], ec.knots_of(table, not inverse)[:K])              # [K, P]
        v = src.reshape(K, *(size if individual else (1, 1, 1))).expand(K, *size).contiguous()
        want = dst.reshape(K, *(size if individual else (1, 1, 1))).expand(K, *size).contiguous()
        out, lad = ec.lines_per_element(v, table, size, ec.TAIL, inverse)
        assert same(out, want), (K, individual, scale, inverse, float((out - want).abs().max()))
        assert bool(torch.isfinite(lad).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the plans of the ragged and multi-trip launches
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pixel_plans_of_the_edge_launches():
    """Stated by hand (tests/spline_edge_cases.py), by the rule written out in tests/spline_cases.py, and by the library."""
    for (B, C, H, W), want in ec.LAUNCH_PLANS.items():
        assert spline_plan(B, C, H * W) == want, (B, C, H, W)
        for align in (4, 8, 16):
            assert _lib.pixel_plan("parts", "spline", B, C, H * W, align=align) == want, (B, C, H, W, align)
    N = 3 * 11 * 13
    assert N == 256 + 2 * 64 + 45                                                   # block 1: waves 0 and 1 full, wave 2 with 45 lanes, wave 3 empty
    assert ec.LAUNCH_PLANS[ec.THREE_TRIPS]["trips"] == 3 and 5 % ec.LAUNCH_PLANS[ec.THREE_TRIPS]["parts"] != 0
    assert (511 * 513) % 256 == 255 and (9 * 511 * 513) % 2 == 1 and (9 * 15) % 2 == 1
    assert ec.LAUNCH_PLANS[ec.DIRECT_GRAD_TABLE]["parts"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the knot inputs hit what they claim
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", (False, True), ids=("forward", "reverse"))
@pytest.mark.parametrize("individual", (False, True), ids=("P1", "PCHW"))
@pytest.mark.parametrize("K", (2, 5, 8, 9, 16))
def test_knot_inputs_sit_on_and_beside_every_knot(K, individual, inverse):
    """By exact float64 comparison with the fp32 table's values: position n of image 1 holds knot n mod (K + 1) of its own row --
    exactly, the next fp32 below or the next above; every knot index appears in all three variants (with shared weights: every knot
    of THE row); and the three variants of an inner knot k fall in bins k, k - 1 and k."""
    shape = ec.KNOT_SHAPE
    table = st.table_of(st.unit_scale_layer(shape[1:], K, ec.TAIL, individual, 300 + K))
    x = ec.knot_inputs(table, shape, ec.TAIL, inverse)
    assert x.dtype == torch.float32 and same(x[0], st.inputs(shape, ec.TAIL, 7)[0])
    rows = ec.rows64(table, inverse)                                                # [P, K + 1]
    flat = x.view(shape[0], -1)[1].double().numpy()
    bins = bins_of(x.numpy(), rows, ec.TAIL).reshape(shape[0], -1)[1]
    seen = set()
    for n, (k, step) in enumerate(ec.knot_plan(flat.size, K)):
        if step is None:
            continue
        knot = rows[n if individual else 0, k]
        f32 = np.float32(knot)
        assert f32 == knot
        want = {0: f32, -1: np.nextafter(f32, np.float32(-np.inf)), 1: np.nextafter(f32, np.float32(np.inf))}[step]
        assert flat[n] == np.float64(want) and (flat[n] < knot, flat[n] == knot, flat[n] > knot)[step + 1], (n, k, step)
        assert abs(flat[n]) <= ec.TAIL
        seen.add((k, step))
        if 0 < k < K:
            assert bins[n] == (k - 1 if step < 0 else k), (n, k, step, bins[n])
        else:
            assert bins[n] == (0 if k == 0 else K - 1), (n, k, step, bins[n])
    inner = {(k, s) for k in range(1, K) for s in (-1, 0, 1)}
    assert inner | {(0, 0), (0, 1), (K, 0), (K, -1)} == seen, sorted(inner - seen)
    tail = x.view(shape[0], -1)[1, -len(ec.SPECIALS):]
    assert same(tail, torch.tensor(ec.SPECIALS, dtype=torch.float32)) and float(tail[3]) > 0.0 and float(tail[3]) == 2.0 ** -149
    assert bool(in_range(tail, ec.TAIL)[[0, 3]].all()) and not bool(in_range(tail, ec.TAIL)[[1, 2]].any())
