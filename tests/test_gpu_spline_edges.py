"""The spline kernels where an element-wise spline goes wrong (cases: tests/spline_edge_cases.py): inputs ON a knot and one ulp beside
it, tables with a steep bin beside a flat one (where the inverse's quadratic cancels and its root used to leave [0, 1]), the 8 / 9
bin seam between the two instantiations, and launches that are ragged, odd-sized, one-image or three trips long.  Every accuracy
figure goes through spline_twin.judge -- max(1e-5, 2 * e_ref), e_ref the layer's own fp32 PyTorch lines on the CPU against the same
float64 values -- and so into the parity report (kind `spline`)."""
import ctypes
import functools

import pytest
import torch

import spline_edge_cases as ec
import spline_twin as st
from helpers import guarded, guards_intact, nan_filled, report, same_bits
from test_gpu_spline import PARAMS, record_calls, twins

pytestmark = pytest.mark.gpu
TAIL = ec.TAIL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def in_range(v):
    return (v >= -TAIL) & (v <= TAIL)


def all_intact(*pairs):
    return all(guards_intact(buf, view) for buf, view in pairs)


def raw_backward(dev, inverse, gy, gl, x, table, gx, gt):
    """The backward entry point itself on buffers of the caller's (ops' wrappers allocate grad_table themselves): gx / gt may be None."""
    from fincflow_amd import _lib
    L = _lib.lib()
    name = "finc_spline_reverse_backward_f32" if inverse else "finc_spline_backward_f32"
    B, C, H, W = x.shape
    K, P = table.shape[0] // 3 - 1, table.shape[1]
    nbytes = L.finc_spline_workspace_bytes(B, C, H * W, K, P)
    ws = nan_filled((nbytes // 4,), torch.float32, dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        status = getattr(L, name)(p(gy), p(gl), p(x), p(table), P, K, TAIL, p(gx), p(gt), B, C, H * W, p(ws), nbytes, None)
    torch.cuda.synchronize(dev)
    _lib.check(status, name)


def autograd_lines(dtype, v, table, size, inverse, g, gl):
    """(out, logdet, grad_v, grad_table) of the layer's lines on the CPU in `dtype`; g / gl None: that term is absent."""
    a, t = v.clone().to(dtype).requires_grad_(True), table.clone().to(dtype).requires_grad_(True)
    out, ld = st.lines_on_table(a, t, size, TAIL, inverse)
    loss = 0
    if g is not None:
        loss = loss + (out * g.to(dtype)).sum()
    if gl is not None:
        loss = loss + (ld * gl.to(dtype)).sum()
    ga, gt = torch.autograd.grad(loss, (a, t))
    return out.detach(), ld.detach(), ga, gt


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. knots, well conditioned (unit-scale parameters)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("individual", (False, True), ids=("P1", "PCHW"))
@pytest.mark.parametrize("K", (2, 8, 9, 16))
def test_knot_inputs_against_float64(K, individual, dev):
    """K = 8: every slot of the 8-bin instantiation a real knot; K = 9: the smallest count in the 16-bin one."""
    from fincflow_amd import _lib, ops
    shape = ec.KNOT_SHAPE
    size, B = shape[1:], shape[0]
    table = st.table_of(st.unit_scale_layer(size, K, TAIL, individual, 400 + 2 * K + int(individual)))
    P = table.shape[1]
    tg, tbuf = guarded(table, dev)
    gen = torch.Generator().manual_seed(5)
    g, gl = torch.randn(shape, generator=gen), torch.randn(B, generator=gen)
    for direction, inverse in ((1, False), (-1, True)):
        x = ec.knot_inputs(table, shape, TAIL, inverse)
        finite, inside = torch.isfinite(x), in_range(x)
        assert int((~finite).sum()) == 2 and int((finite & ~inside).sum()) == 2
        xg, xbuf = guarded(x, dev)
        yg, ybuf = guarded(torch.zeros_like(x), dev)
        y, ld = ops.finc_spline(xg, tg, TAIL, direction, True, out=yg)
        torch.cuda.synchronize()
        assert y.data_ptr() == yg.data_ptr() and all_intact((xbuf, xg), (tbuf, tg), (ybuf, yg))
        want = st.lines_on_table(x.double(), table.double(), size, TAIL, inverse)
        yard = st.lines_on_table(x, table, size, TAIL, inverse)
        assert bool(torch.isfinite(yard[0][finite]).all() and torch.isfinite(yard[1]).all()), "the fp32 lines: the bar's premise"
        yc = y.cpu()
        fields = dict(shape=list(shape), P=P, K=K, direction=direction)
        st.judge("knots", ["y", "logdet"], [yc[finite], ld], [want[0][finite], want[1]], [yard[0][finite], yard[1]], **fields)
        # an exact knot k < K maps to the other array's knot bit for bit (th = 0: every other term is an exact zero)
        plan = ec.knot_plan(x[0].numel(), K)
        exact = [n for n, (k, step) in enumerate(plan) if step == 0 and k < K]
        other = ec.knots_of(table, not inverse)
        assert len(exact) >= K
        assert same_bits(yc.view(B, -1)[1, exact], torch.stack([other[plan[n][0], n if P > 1 else 0] for n in exact]))
        assert same_bits(yc.view(B, -1)[0, 1:2], torch.tensor([-TAIL]))             # image 0 holds -tail_bound: knot 0 of every row
        # +-inf and everything beyond the tails: the input's bits; -0.0 and the subnormal: in range, finite
        assert same_bits(yc[~inside], x[~inside]) and bool(torch.isfinite(yc[inside]).all())
        special = yc.view(B, -1)[1, -len(ec.SPECIALS):]
        assert bool(torch.isfinite(special[[0, 3]]).all()) and bool(torch.isinf(special[[1, 2]]).all())
        assert same_bits(ops.finc_spline(xg, tg, TAIL, direction)[0], y)              # without the log-det: the same y
        # ... with zero log-derivative: an image of nothing but such values has log-det +0.0, and image 0 keeps its bits
        tails = xg.clone()
        tails[1] = torch.tensor([float("inf"), float("-inf"), 1.2 * TAIL, -1.2 * TAIL, float("nan")], device=dev).repeat(x[1].numel() // 5).view(size)
        y2, ld2 = ops.finc_spline(tails, tg, TAIL, direction, True)
        assert same_bits(y2[1], tails[1]) and same_bits(ld2[1:], torch.zeros(1, device=dev))
        assert same_bits(y2[0], y[0]) and same_bits(ld2[:1], ld[:1])

        # both backwards on the same inputs against float64 autograd through the lines
        backward = ops.finc_spline_reverse_backward if inverse else ops.finc_spline_backward
        for use_g, use_gl in ((True, False), (False, True), (True, True)):
            terms = (g if use_g else None, gl if use_gl else None)
            want_g, yard_g = (autograd_lines(dt, x, table, size, inverse, *terms)[2:] for dt in (torch.float64, torch.float32))
            assert all(bool(torch.isfinite(t).all()) for t in yard_g), "the fp32 lines' gradients: the bar's premise"
            gx, gt = backward(*(None if t is None else t.to(dev) for t in terms), xg, tg, TAIL)
            st.judge("knots_backward", ["grad_x", "grad_table"], [gx, gt], want_g, yard_g, grad_y=use_g, grad_logdet=use_gl, **fields)
            if use_g:                                                               # a tail element hands grad_y through: dL/dx = 0 there
                assert same_bits(gx.cpu()[~inside], g[~inside])
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. knots, a steep bin beside a flat one
# ---------------------------------------------------------------------------------------------------------------------------------
def at_a_bin_end(x, y, table, inside):
    """In-range elements whose x is an end of its bin bit for bit although y is no knot: where the root met the clamp (or rounded
    onto the knot)."""
    lo, hi = ec.bin_ends(y, table, TAIL, True, False)
    chl, chh = ec.bin_ends(y, table, TAIL, True, True)
    xd, yd = x.double(), y.double()
    return int((inside & ((xd == lo) | (xd == hi)) & (yd != chl) & (yd != chh)).sum())


@pytest.mark.parametrize("name", sorted(ec.STEEP_FLAT))
def test_steep_beside_flat_reverse_stays_in_its_bin(name, dev):
    """Asserted for every in-range element, `reverse` and `reverse_with_logdet` and their backward: finite, cw[bin] <= x <= cw[bin+1],
    |x| <= tail_bound, x non-decreasing in y, and the residual |f64(x_hip) - y| / tail_bound under max(1e-5, 2 * e_ref) (e_ref: the same
    residual of the fp32 CPU lines).  x itself and the log-det against the float64 lines are held to the same bar: solved from
    the nearer knot they are well conditioned (one ulp of y moves the float64 log-derivative by 0.65 in `indiv_k8_s3`, yet the
    device is 1.5e-6 off in x [fp32 lines 1.2e-6] and 1.3e-6 in the log-det [1.2e-6]; the residual is 6.3e-5 [6.3e-5], a slope of
    1e3 times an ulp of x)."""
    from fincflow_amd import _lib, ops
    shape, K, tb, table = ec.steep_flat_tables(name)
    assert tb == TAIL
    size, B, P = shape[1:], shape[0], table.shape[1]
    y = ec.knot_inputs(table, shape, TAIL, True)
    inside = in_range(y)
    yg, ybuf = guarded(y, dev)
    tg, tbuf = guarded(table, dev)
    og, obuf = guarded(torch.zeros_like(y), dev)
    x, ld = ops.finc_spline(yg, tg, TAIL, -1, True, out=og)
    x_plain = ops.finc_spline(yg, tg, TAIL, -1)[0]
    torch.cuda.synchronize()
    assert all_intact((ybuf, yg), (tbuf, tg), (obuf, og)) and same_bits(x_plain, x)
    xc = x.cpu()
    x32, lad32 = ec.lines_per_element(y, table, size, TAIL, True)
    fields = dict(name=name, K=K, P=P)
    hip_ends, cpu_ends = at_a_bin_end(xc, y, table, inside), at_a_bin_end(x32, y, table, inside)
    print("spline steep_flat %s: x at a bin end from a y that is no knot: HIP %d, fp32 lines %d of %d in-range elements; logdet HIP %s"
          % (name, hip_ends, cpu_ends, int(inside.sum()), ld.tolist()))
    report("spline", case="steep_flat_bin_ends", name=name, hip=hip_ends, cpu=cpu_ends, in_range=int(inside.sum()), logdet=ld.tolist())
    assert bool(torch.isfinite(xc[inside]).all() and torch.isfinite(ld).all()), (name, xc[inside & ~torch.isfinite(xc)], ld)
    assert same_bits(xc[~inside], y[~inside])
    lo, hi = ec.bin_ends(y, table, TAIL, True, False)
    xd = xc.double()
    out = inside & ~((lo <= xd) & (xd <= hi) & (xd.abs() <= TAIL))
    assert not bool(out.any()), (name, "x outside its bin", y[out].tolist()[:4], xd[out].tolist()[:4], lo[out].tolist()[:4], hi[out].tolist()[:4])
    # monotone: one spline for all elements (P = 1), else one per position over its images
    ys, xs = (t.view(1, -1) if P == 1 else t.view(B, -1).t() for t in (torch.where(inside, y, torch.full_like(y, TAIL)),
                                                                       torch.where(inside, xc, torch.full_like(xc, TAIL))))
    order = ys.argsort(dim=1, stable=True)
    ys, xs = ys.gather(1, order), xs.gather(1, order)
    rising = ys[:, 1:] > ys[:, :-1]
    assert bool((xs[:, 1:] >= xs[:, :-1])[rising].all()), (name, "x decreases where y increases")
    # the residual: the forward map in float64 on the returned x against y, in-range elements
    y64 = y.double()
    residual = lambda xs_: ec.lines_per_element(xs_.double(), table.double(), size, TAIL, False)[0][inside]
    st.judge("steep_flat_residual", ["f64(x)"], [residual(xc)], [y64[inside]], [residual(x32)], **fields)
    # x and the log-det against the float64 lines
    want = st.lines_on_table(y64, table.double(), size, TAIL, True)
    yard = st.lines_on_table(y, table, size, TAIL, True)
    finite = torch.isfinite(y)
    st.judge("steep_flat_x_logdet", ["x", "logdet"], [xc[finite], ld], [want[0][finite], want[1]], [yard[0][finite], yard[1]], **fields)
    # the backward of both forms: finite, and a tail element hands its gradient through
    gen = torch.Generator().manual_seed(6)
    g, gl = torch.randn(shape, generator=gen).to(dev), torch.randn(B, generator=gen).to(dev)
    for use_gl in (False, True):
        gy, gt = ops.finc_spline_reverse_backward(g, gl if use_gl else None, yg, tg, TAIL)
        assert bool(torch.isfinite(gy).all() and torch.isfinite(gt).all()), (name, use_gl)
        assert same_bits(gy.cpu()[~inside], g.cpu()[~inside])
    assert not _lib.fault_pending()


@pytest.mark.parametrize("name", [n for n in sorted(ec.STEEP_FLAT) if not ec.STEEP_FLAT[n][2]])
def test_reverse_is_monotone_over_consecutive_floats(name, dev):
    """The shared-weight steep/flat tables over `consecutive_heights`: x never falls while y rises float by float, across every knot
    and across every bin's mid-height, where the solve changes from the lower knot to the upper one; x stays in its bin and agrees
    with float64 under the judge; the backward is finite."""
    from fincflow_amd import _lib, ops
    shape, K, tb, table = ec.steep_flat_tables(name)
    y = ec.consecutive_heights(table)
    size = tuple(y.shape[1:])
    x, ld = ops.finc_spline(y.to(dev), table.to(dev), TAIL, -1, True)
    xc = x.cpu()
    assert bool(torch.isfinite(xc).all() and torch.isfinite(ld).all())
    falls = xc[..., 1:] < xc[..., :-1]
    assert not bool(falls.any()), (name, int(falls.sum()), falls.nonzero()[:4].tolist())
    lo, hi = ec.bin_ends(y, table, TAIL, True, False)
    assert bool(((lo <= xc.double()) & (xc.double() <= hi)).all())
    want = st.lines_on_table(y.double(), table.double(), size, TAIL, True)
    yard = st.lines_on_table(y, table, size, TAIL, True)
    st.judge("consecutive_floats", ["x", "logdet"], [xc, ld], want, yard, name=name, K=K)
    gy, gt = ops.finc_spline_reverse_backward(torch.ones_like(x), torch.ones_like(ld), y.to(dev), table.to(dev), TAIL)
    assert bool(torch.isfinite(gy).all() and torch.isfinite(gt).all())
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ragged and multi-trip launches
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def launch_case(shape, individual):
    """The table, inputs and incoming gradients of one launch case, and per direction the float64 and fp32 CPU results
    (y, logdet, grad_x, grad_table): computed once, shared by the two leads."""
    table = st.table_of(st.unit_scale_layer(shape[1:], 2, TAIL, individual, 3))
    gen = torch.Generator().manual_seed(11)
    x = 0.7 * TAIL * torch.randn(shape, generator=gen)
    gy, gl = torch.randn(shape, generator=gen), torch.randn(shape[0], generator=gen)
    refs = {d: tuple(autograd_lines(dt, x, table, shape[1:], d < 0, gy, gl) for dt in (torch.float64, torch.float32)) for d in (1, -1)}
    return table, x, gy, gl, refs


@pytest.mark.parametrize("lead", (0, 2), ids=("aligned", "two_floats_in"))
@pytest.mark.parametrize("individual", (False, True), ids=("P1", "PCHW"))
@pytest.mark.parametrize("shape", sorted(ec.LAUNCH_PLANS), ids=lambda s: "x".join(map(str, s)))
def test_ragged_and_multi_trip_launches(shape, individual, lead, dev):
    from fincflow_amd import _lib, ops
    B, C, H, W = shape
    plan = _lib.pixel_plan("parts", "spline", B, C, H * W, align=16 if lead == 0 else 8)
    assert plan == ec.LAUNCH_PLANS[shape]
    table, x, gy, gl, refs = launch_case(shape, individual)
    P, T = table.shape[1], table.numel()
    assert T == 9 * P
    xg, xbuf = guarded(x, dev, lead)
    tg, tbuf = guarded(table, dev, lead)
    gyd, gld = gy.to(dev), gl.to(dev)
    fields = dict(shape=list(shape), P=P, lead=lead)
    for direction in (1, -1):
        inverse = direction < 0
        want, yard = refs[direction]
        yg, ybuf = guarded(torch.zeros_like(x), dev, lead)
        y, ld = ops.finc_spline(xg, tg, TAIL, direction, True, out=yg)
        gxg, gxbuf = guarded(nan_filled(shape, torch.float32, dev), dev, lead)
        gtg, gtbuf = guarded(nan_filled(table.shape, torch.float32, dev), dev, lead)
        raw_backward(dev, inverse, gyd, gld, xg, tg, gxg, gtg)
        assert all_intact((xbuf, xg), (tbuf, tg), (ybuf, yg), (gxbuf, gxg), (gtbuf, gtg)), (shape, direction)
        backward = ops.finc_spline_reverse_backward if inverse else ops.finc_spline_backward
        gx, gt = backward(gyd, gld, xg, tg, TAIL)
        assert same_bits(gx, gxg) and same_bits(gt, gtg)
        # every entry of grad_table was written (NaN on entry), the last even and the last odd output of the pair reduce included
        assert bool(torch.isfinite(gt).all())
        st.judge("edge_launch", ["y", "logdet", "grad_x", "grad_table"], [y, ld, gx, gt], want, yard, direction=direction, **fields)
        last = gt.flatten()[-2:].cpu().double()
        bar = max(st.BAR, 2 * st.error(yard[3], want[3])) * float(want[3].abs().max())
        assert float((last - want[3].flatten()[-2:]).abs().max()) <= bar

        if shape == ec.DIRECT_GRAD_TABLE and individual:
            # Q = 1: grad_table is written from the walk.  Either output alone: the bits of the joint call, between intact guards
            only_t, only_tbuf = guarded(nan_filled(table.shape, torch.float32, dev), dev, lead)
            raw_backward(dev, inverse, gyd, gld, xg, tg, None, only_t)
            only_x, only_xbuf = guarded(nan_filled(shape, torch.float32, dev), dev, lead)
            raw_backward(dev, inverse, gyd, gld, xg, tg, only_x, None)
            assert same_bits(only_t, gt) and same_bits(only_x, gx) and all_intact((only_tbuf, only_t), (only_xbuf, only_x))
            assert same_bits(backward(gyd, gld, xg, tg, TAIL, need_gx=False)[1], gt)
            assert same_bits(backward(gyd, gld, xg, tg, TAIL, need_gt=False)[0], gx)

        if shape == ec.THREE_TRIPS and lead == 0:
            # a lane walks three images (part 1: two): the bits of one-image calls; per-position grad_table is their sum
            assert plan["trips"] == 3 and _lib.pixel_plan("parts", "spline", 1, C, H * W)["trips"] == 1
            parts = []
            for b in range(B):
                one = slice(b, b + 1)
                y1, ld1 = ops.finc_spline(xg[one].contiguous(), tg, TAIL, direction, True)
                gx1, gt1 = backward(gyd[one].contiguous(), gld[one].contiguous(), xg[one].contiguous(), tg, TAIL)
                assert same_bits(y1[0], y[b]) and same_bits(ld1, ld[one]) and same_bits(gx1[0], gx[b]), (direction, b)
                parts.append(gt1.double())
            if individual:
                # five fp32 terms per entry, each within an ulp of the double sum's terms: 1e-5 of the largest entry is generous
                assert st.error(gt, sum(parts)) <= 1e-5
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the 8 / 9 bin seam through the module
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("individual", (False, True), ids=("shared", "individual"))
@pytest.mark.parametrize("n_bins", (8, 9))
def test_module_at_the_seam_against_the_float64_twin(n_bins, individual, dev, monkeypatch):
    """n_bins = 8 runs the KB = 8 instantiations, 9 the KB = 16 ones; the call lists show that neither falls back to the lines."""
    from fincflow_amd import _lib, ops
    shape = (3, 2, 3, 5)
    m = st.unit_scale_layer(shape[1:], n_bins, TAIL, individual, 31 + n_bins).to(dev)
    t64, t32 = twins(m)
    x = st.inputs(shape, TAIL, 9)
    gen = torch.Generator().manual_seed(2)
    r, s = torch.randn(shape, generator=gen), torch.randn(shape[0], generator=gen)
    calls = record_calls(monkeypatch)
    with torch.no_grad():
        got = [*m(x.to(dev)), m.reverse(x.to(dev)), *m.reverse_with_logdet(x.to(dev))]
        want, yard = ([*t(x.to(d)), t.reverse(x.to(d)), *t.reverse_with_logdet(x.to(d))] for t, d in ((t64, torch.float64), (t32, torch.float32)))
    assert calls == ["finc_spline_f32"] * 3, calls
    st.judge("seam_no_grad", ["y", "logdet", "reverse", "reverse_wl", "reverse_wl_logdet"], got, want, yard, n_bins=n_bins, individual=individual)

    def training(layer, dtype, d, reverse):
        layer.zero_grad(set_to_none=True)
        a = x.clone().to(d).to(dtype).requires_grad_(True)
        if reverse:
            with ops.reverse_grad():
                out, ld = layer.reverse_with_logdet(a)
        else:
            out, ld = layer(a)
        ((out * r.to(d).to(dtype)).sum() + (ld * s.to(d).to(dtype)).sum()).backward()
        return [out, ld, a.grad] + [getattr(layer, p).grad for p in PARAMS]

    names = ["out", "logdet", "grad_x"] + ["grad_" + p for p in PARAMS]
    for reverse in (False, True):
        del calls[:]
        got = training(m, torch.float32, dev, reverse)
        assert calls == (["finc_spline_f32", "finc_spline_reverse_backward_f32"] if reverse else ["finc_spline_f32", "finc_spline_backward_f32"]), calls
        st.judge("seam_training", names, got, training(t64, torch.float64, "cpu", reverse), training(t32, torch.float32, "cpu", reverse),
                 n_bins=n_bins, individual=individual, reverse=reverse)
    assert not _lib.fault_pending()
