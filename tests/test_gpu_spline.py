"""The rational-quadratic spline on the GPU: the kernels against float64 between NaN guard bands, their multi-trip launches by plan,
both backwards against float64 autograd through the layer's written-out lines, glow.SplineActivation against its float64 CPU twin,
and a stack that holds the layer through every view of FlowSequential.  Every comparison is held to max(1e-5, 2 * e_ref), e_ref the
error of the layer's own PyTorch lines in float32 on the CPU against the same float64 values (tests/spline_twin.py: judge)."""
import copy

import pytest
import torch

import flow_twin
import spline_twin as st
from helpers import guarded, guards_intact, same_bits
from spline_cases import MULTI_TRIP, PLANS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def record_calls(monkeypatch):
    """Every entry point that goes through ops._call, by name, in order."""
    from fincflow_amd import ops
    names, real = [], ops._call

    def recorded(name, *args, **kwargs):
        names.append(name)
        return real(name, *args, **kwargs)
    monkeypatch.setattr(ops, "_call", recorded)
    return names


SHAPES = ((2, 3, 4, 4), (3, 2, 3, 5))          # rows of 16 bytes; HW = 15
TAIL = 3.0


def case(shape, individual, K, seed=0):
    """(layer on the CPU, its fp32 table, inputs)."""
    m = st.unit_scale_layer(shape[1:], K, TAIL, individual, 10 * K + seed + int(individual))
    return m, st.table_of(m), st.inputs(shape, TAIL, 7 + seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the transform kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", (0, 2), ids=("aligned", "two_floats_in"))
@pytest.mark.parametrize("K", (2, 5, 16))
@pytest.mark.parametrize("individual", (False, True), ids=("P1", "PCHW"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64_between_guard_bands(shape, individual, K, lead, dev):
    from fincflow_amd import _lib, ops
    assert _lib.pixel_plan("parts", "spline", shape[0], shape[1], shape[2] * shape[3], align=16 if lead == 0 else 8) == PLANS[shape]
    m, table, x = case(shape, individual, K)
    xg, xbuf = guarded(x, dev, lead)
    tg, tbuf = guarded(table, dev, lead)
    for direction, inverse in ((1, False), (-1, True)):
        want = st.lines_on_table(x.double(), table.double(), shape[1:], TAIL, inverse)
        yard = st.lines_on_table(x, table, shape[1:], TAIL, inverse)
        yg, ybuf = guarded(torch.zeros_like(x), dev, lead)
        y, ld = ops.finc_spline(xg, tg, TAIL, direction, True, out=yg)
        torch.cuda.synchronize()
        assert y.data_ptr() == yg.data_ptr() and all(guards_intact(b, v) for b, v in ((xbuf, xg), (tbuf, tg), (ybuf, yg)))
        st.judge("kernel", ["y", "logdet"], [y, ld], want, yard, shape=list(shape), P=table.shape[1], K=K, direction=direction, lead=lead)
        outside = (x.abs() > TAIL).to(dev)
        assert int(outside.sum()) >= 2 and same_bits(y[outside], xg[outside])
        y_plain = ops.finc_spline(xg, tg, TAIL, direction)[0]                       # without the log-det: the same y
        y2, ld2 = ops.finc_spline(xg, tg, TAIL, direction, True)
        assert same_bits(y2, y) and same_bits(ld2, ld)                              # bit-stable over two calls
        assert same_bits(y_plain, y)
        # images are isolated: another image 1 (a NaN among its values) leaves image 0's y and logdet as they were
        other = xg.clone()
        other[1] = TAIL * torch.randn(shape[1:], device=dev)
        other[1, 0, 0, 0] = float("nan")
        y3, ld3 = ops.finc_spline(other, tg, TAIL, direction, True)
        assert same_bits(y3[0], y[0]) and same_bits(ld3[:1], ld[:1]) and same_bits(y3[1, 0, 0, :1], other[1, 0, 0, :1])
        assert not same_bits(y3[1], y[1])
        inplace = xg.clone()
        assert same_bits(ops.finc_spline(inplace, tg, TAIL, direction, out=inplace)[0], y)
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. multi-trip launches, by plan
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("individual", (False, True), ids=("P1", "PCHW"))
@pytest.mark.parametrize("shape", MULTI_TRIP, ids=lambda s: "x".join(map(str, s)))
def test_multi_trip_launches_match_one_trip_sub_batches(shape, individual, dev):
    """A lane that walks more than one image (trips = 2; with two parts the second trip is partial): y, logdet and grad_x carry the
    bits of one-image calls, and per-position grad_table is the sum of the one-image ones."""
    from fincflow_amd import _lib, ops
    B, C, H, W = shape
    plan = _lib.pixel_plan("parts", "spline", B, C, H * W)
    assert plan == PLANS[shape] and plan["trips"] == 2 and _lib.pixel_plan("parts", "spline", 1, C, H * W)["trips"] == 1
    m = st.unit_scale_layer(shape[1:], 2, TAIL, individual, 3)
    table = st.table_of(m).to(dev)
    gen = torch.Generator().manual_seed(11)
    x = (0.7 * TAIL * torch.randn(shape, generator=gen)).to(dev)
    gy = torch.randn(shape, generator=gen).to(dev)
    gl = torch.randn(B, generator=gen).to(dev)
    for direction in (1, -1):
        y, ld = ops.finc_spline(x, table, TAIL, direction, True)
        saved = x
        backward = ops.finc_spline_backward if direction == 1 else ops.finc_spline_reverse_backward
        gx, gt = backward(gy, gl, saved, table, TAIL)
        parts = []
        for b in range(B):
            y1, ld1 = ops.finc_spline(x[b:b + 1].contiguous(), table, TAIL, direction, True)
            gx1, gt1 = backward(gy[b:b + 1].contiguous(), gl[b:b + 1].contiguous(), saved[b:b + 1].contiguous(), table, TAIL)
            assert same_bits(y1[0], y[b]) and same_bits(ld1, ld[b:b + 1]) and same_bits(gx1[0], gx[b]), (direction, b)
            parts.append(gt1.double())
        if individual:
            # at most three fp32 terms per entry, each within an ulp of the double sum's terms: 1e-5 of the largest entry is generous
            assert st.error(gt, sum(parts)) <= 1e-5

        # grad_table against float64 autograd through the lines, for both P: with P = 1 this is the launch whose 2048 workgroups each
        # hand one partial per entry to the reduce (the small backward cases have two or three)
        def cpu_grad_table(dtype):
            t = table.cpu().to(dtype).requires_grad_(True)
            out, ld = st.lines_on_table(x.cpu().to(dtype), t, shape[1:], TAIL, direction < 0)
            return torch.autograd.grad((out * gy.cpu().to(dtype)).sum() + (ld * gl.cpu().to(dtype)).sum(), t)[0]
        st.judge("multi_trip_grad_table", ["grad_table"], [gt], [cpu_grad_table(torch.float64)], [cpu_grad_table(torch.float32)],
                 shape=list(shape), P=table.shape[1], direction=direction)
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the backwards
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("forward", "reverse"))
@pytest.mark.parametrize("K", (2, 5, 16))
@pytest.mark.parametrize("individual", (False, True), ids=("P1", "PCHW"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_against_float64_autograd(shape, individual, K, mode, dev):
    from fincflow_amd import _lib, ops
    m, table, v = case(shape, individual, K, seed=1)
    gen = torch.Generator().manual_seed(5)
    g, gl = torch.randn(shape, generator=gen), torch.randn(shape[0], generator=gen)
    inverse = mode == "reverse"

    def autograd(dtype, use_g, use_gl):
        a, t = v.clone().to(dtype).requires_grad_(True), table.clone().to(dtype).requires_grad_(True)
        out, ld = st.lines_on_table(a, t, shape[1:], TAIL, inverse)
        loss = (out * g.to(dtype)).sum() * float(use_g) + (ld * gl.to(dtype)).sum() * float(use_gl)
        return torch.autograd.grad(loss, (a, t))

    vg, tg = v.to(dev), table.to(dev)
    saved = vg                                                                      # both backwards read their pass's INPUT
    backward = ops.finc_spline_reverse_backward if inverse else ops.finc_spline_backward
    for use_g, use_gl in ((True, False), (False, True), (True, True)):
        want, yard = autograd(torch.float64, use_g, use_gl), autograd(torch.float32, use_g, use_gl)
        args = (g.to(dev) if use_g else None, gl.to(dev) if use_gl else None, saved, tg, TAIL)
        gx, gt = backward(*args)
        st.judge("backward", ["grad_x", "grad_table"], [gx, gt], want, yard, shape=list(shape), P=table.shape[1], K=K, mode=mode,
                 grad_y=use_g, grad_logdet=use_gl)
        again = backward(*args)
        assert same_bits(again[0], gx) and same_bits(again[1], gt)
        assert same_bits(backward(*args, need_gt=False)[0], gx) and same_bits(backward(*args, need_gx=False)[1], gt)
        # a tail element adds nothing to grad_table: other tail values (and a NaN) in the planted places, the same bits
        moved = saved.clone()
        flat = moved.view(shape[0], -1)
        assert float(flat[0, 3]) > TAIL and float(flat[0, 4]) < -TAIL
        flat[0, 3], flat[0, 4] = 5.0 * TAIL, float("nan")
        gx2, gt2 = backward(args[0], args[1], moved, tg, TAIL)
        assert same_bits(gt2, gt)
        if use_g:                                                                   # and hands grad_y through
            assert same_bits(gx2.view(shape[0], -1)[0, 3:5], g.to(dev).view(shape[0], -1)[0, 3:5])
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the module against its float64 CPU twin
# ---------------------------------------------------------------------------------------------------------------------------------
def twins(m):
    return copy.deepcopy(m).cpu().double(), copy.deepcopy(m).cpu().float()


PARAMS = ("unnormalized_widths", "unnormalized_heights", "unnormalized_derivatives")


@pytest.mark.parametrize("individual", (False, True), ids=("shared", "individual"))
def test_module_against_the_float64_twin(individual, dev, monkeypatch):
    from fincflow_amd import _lib, ops
    shape = (3, 2, 3, 5)
    m = st.unit_scale_layer(shape[1:], 5, TAIL, individual, 21).to(dev)
    t64, t32 = twins(m)
    x = st.inputs(shape, TAIL, 9)
    gen = torch.Generator().manual_seed(2)
    r, s = torch.randn(shape, generator=gen), torch.randn(shape[0], generator=gen)
    calls = record_calls(monkeypatch)

    with torch.no_grad():
        got = [*m(x.to(dev)), m.reverse(x.to(dev)), *m.reverse_with_logdet(x.to(dev)), m.logdet(x.to(dev))]
        want, yard = ([*t(x.to(d)), t.reverse(x.to(d)), *t.reverse_with_logdet(x.to(d)), t.logdet(x.to(d))]
                      for t, d in ((t64, torch.float64), (t32, torch.float32)))
    assert calls == ["finc_spline_f32"] * 4, calls
    assert "_tab" in m.__dict__ and "_tab" not in t64.__dict__
    st.judge("module_no_grad", ["y", "logdet", "reverse", "reverse_wl", "reverse_wl_logdet", "logdet_alone"], got, want, yard,
             individual=individual)

    def training(layer, dtype, d, reverse):
        layer.zero_grad(set_to_none=True)
        a = x.clone().to(d).to(dtype).requires_grad_(True)
        if reverse:
            with ops.reverse_grad():
                out, ld = layer.reverse_with_logdet(a)
                alone = layer.reverse(a)
        else:
            out, ld = layer(a)
            alone = out
        ((out * r.to(d).to(dtype)).sum() + (ld * s.to(d).to(dtype)).sum() + 0.5 * (alone * alone).sum()).backward()
        return [out, ld, a.grad] + [getattr(layer, p).grad for p in PARAMS]

    names = ["out", "logdet", "grad_x"] + ["grad_" + p for p in PARAMS]
    for reverse in (False, True):
        del calls[:]
        got = training(m, torch.float32, dev, reverse)
        assert calls == (["finc_spline_f32", "finc_spline_f32", "finc_spline_reverse_backward_f32", "finc_spline_reverse_backward_f32"]
                         if reverse else ["finc_spline_f32", "finc_spline_backward_f32"]), calls
        st.judge("module_training", names, got, training(t64, torch.float64, "cpu", reverse), training(t32, torch.float32, "cpu", reverse),
                 individual=individual, reverse=reverse)

    # two fused Adam steps: they write the parameters without advancing Tensor._version; the cached table follows (ops.version_key)
    opt = torch.optim.Adam(m.parameters(), lr=0.05, fused=True)
    for step in range(2):
        training(m, torch.float32, dev, False)
        opt.step()
        for t in (t64, t32):
            flow_twin.sync(t, m)
        with torch.no_grad():
            got = list(m(x.to(dev)))
            want, yard = (list(t(x.to(d))) for t, d in ((t64, torch.float64), (t32, torch.float32)))
        st.judge("module_after_fused_adam", ["y", "logdet"], got, want, yard, individual=individual, step=step)
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a stack that holds the layer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev):
    """(the HIP model, its float64 twin, its float32 twin, x)."""
    from fincflow_amd import _lib
    model = st.stack().to(dev)
    for shape in ((4, 12, 4, 4), (4, 24, 2, 2)):
        assert _lib.pixel_plan("parts", "spline", shape[0], shape[1], shape[2] * shape[3]) == PLANS[shape]
    x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(7))
    return model, flow_twin.twin_of(model), flow_twin.twin_of(model, torch.float32), x


def first(v):
    return v[0] if isinstance(v, tuple) else v


def test_stack_density_and_codes(models, dev, monkeypatch):
    model, t64, t32, x = models
    calls = record_calls(monkeypatch)
    with torch.no_grad():
        lp = model.log_prob(x.to(dev))
        zs, lpe = model.encode(x.to(dev))
        back = model.decode(zs)
        want, yard = ([t.log_prob(x.to(d)), *t.encode(x.to(d))[0], t.encode(x.to(d))[1]] for t, d in ((t64, torch.float64), (t32, torch.float32)))
    assert calls.count("finc_spline_f32") == 6, calls
    st.judge("stack_encode", ["log_prob", "z0", "z1", "log_prob_encode"], [lp, *zs, lpe], want, yard)
    with torch.no_grad():
        want, yard = (t.decode([z.cpu().to(d) for z in zs]) for t, d in ((t64, torch.float64), (t32, torch.float32)))
    st.judge("stack_decode", ["x"], [back], [want], [yard])


def test_stack_sampling_views(models, dev):
    model, t64, t32, x = models
    for view in ("sample", "sample_with_log_prob", "reconstruct"):
        args = (x.to(dev),) if view == "reconstruct" else (4,)
        with torch.no_grad(), flow_twin.recorded_noise(model) as draws:
            got = getattr(model, view)(*args)
        got = [first(got)] + ([got[1]] if view == "sample_with_log_prob" else [])
        both = []
        for t, d in ((t64, torch.float64), (t32, torch.float32)):
            targs = (x.to(d),) if view == "reconstruct" else (4,)
            with torch.no_grad(), flow_twin.replayed_noise(t, draws):
                out = getattr(t, view)(*targs)
            both.append([first(out)] + ([out[1]] if view == "sample_with_log_prob" else []))
        st.judge("stack_" + view, ["x", "log_q"][:len(got)], got, both[0], both[1])
    # log q of a sample is log_prob of that sample
    with torch.no_grad():
        s, lq = model.sample_with_log_prob(4)
        lp = model.log_prob(s)
        s64 = s.cpu().double()
        want, yard = t64.log_prob(s64), t32.log_prob(s.cpu())
    st.judge("stack_log_q_is_log_prob", ["log_q", "log_prob"], [lq, lp], [want, want], [yard, yard])


def test_stack_reparameterised_sampling(models, dev):
    """rsample / rsample_with_log_prob: values and the gradients that reach the splines' parameters."""
    model, t64, t32, x = models
    splines = [n for n, _ in model.named_parameters() if "unnormalized" in n]
    assert len(splines) == 6

    def run(net, view, draws=None):
        net.zero_grad(set_to_none=True)
        ctx = flow_twin.recorded_noise(net) if draws is None else flow_twin.replayed_noise(net, draws)
        with ctx as rec:
            out = getattr(net, view)(4)
        xs, lq = (out, None) if view == "rsample" else out
        loss = (xs * xs).sum() if lq is None else (xs * xs).sum() + lq.sum()
        loss.backward()
        params = dict(net.named_parameters())
        return [xs] + ([lq] if lq is not None else []) + [params[n].grad for n in splines], rec

    for view in ("rsample", "rsample_with_log_prob"):
        got, draws = run(model, view)
        want, yard = run(t64, view, draws)[0], run(t32, view, draws)[0]
        names = ["x"] + (["log_q"] if view != "rsample" else []) + ["grad_" + n for n in splines]
        st.judge("stack_" + view, names, got, want, yard)
    model.zero_grad(set_to_none=True)


def test_unit_scale_stack_layer_by_layer(dev):
    """The stack at unit-scale spline parameters.  Its `decode` is ill-conditioned -- the fp32 CPU lines are themselves per mille off
    float64 -- so the whole chain is REPORTED beside that figure, not asserted.  What is asserted: each spline layer's `reverse` and
    `reverse_with_logdet` on the float64 twin's own input to that layer in the same decode (rounded to fp32), against float64 on
    that same input, under the usual bar.  A defect of the kernel would show there; the amplification of earlier layers' rounding
    cannot."""
    from fincflow_amd import glow
    model = st.stack(scale=1.0).to(dev)
    t64, t32 = flow_twin.twin_of(model), flow_twin.twin_of(model, torch.float32)
    splines = [[m for m in net.modules() if isinstance(m, glow.SplineActivation)] for net in (model, t64, t32)]
    assert len(splines[0]) == 2
    x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(7))
    seen = []
    for layer in splines[1]:
        layer.reverse = lambda v, context=None, _l=layer: (seen.append((_l, v.detach().clone())), type(_l).reverse(_l, v, context))[1]
    with torch.no_grad():
        zs, _ = model.encode(x.to(dev))
        back = model.decode(zs)
        want = t64.decode([z.cpu().double() for z in zs])
        yard = t32.decode([z.cpu() for z in zs])
    st.judge("stack_unit_scale_decode", ["x"], [back], [want], [yard], asserting=False)
    assert [l for l, _ in seen] == splines[1][::-1]                                 # the reverse chain meets the second level first
    for layer64, v in seen:
        i = splines[1].index(layer64)
        v32 = v.float()
        with torch.no_grad():
            got = [splines[0][i].reverse(v32.to(dev)), *splines[0][i].reverse_with_logdet(v32.to(dev))]
            ref = [type(layer64).reverse(layer64, v32.double()), *layer64.reverse_with_logdet(v32.double())]
            fp32 = [splines[2][i].reverse(v32), *splines[2][i].reverse_with_logdet(v32)]
        st.judge("stack_unit_scale_layer", ["reverse", "reverse_wl", "reverse_wl_logdet"], got, ref, fp32, layer=i)


def test_stack_sample_in_a_captured_graph(models, dev):
    """`sample` captured in a HIP graph with the draws held fixed, replayed twice: the bits of the eager call."""
    from fincflow_amd import _lib
    model = models[0]
    priors = flow_twin._priors(model)
    fixed = {id(p): torch.randn(4, *p.size, device=dev) for p in priors}
    for p in priors:
        p.sample = lambda n, context=None, _p=p: (fixed[id(_p)], None)
    try:
        with torch.no_grad():
            eager = first(model.sample(4)).clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = first(model.sample(4))
            for _ in range(2):
                out.zero_()
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager)
    finally:
        for p in priors:
            del p.sample
    assert not _lib.fault_pending()
