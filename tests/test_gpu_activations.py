"""The smooth invertible activations on the GPU: the kernels against float64 between NaN guard bands, their multi-trip launches by
plan, the bracketed inverse over the whole parameter box against float64 bisection, the three backward modes against float64 autograd
through the layers' written-out lines, the modules against their float64 CPU twins, and stacks that hold the layers through every
view of FlowSequential.  Every comparison is held to max(1e-5, 2 * e_ref), e_ref the error of the layer's own PyTorch lines in float32
on the CPU against the same float64 values (tests/activation_cases.py: judge)."""
import copy

import pytest
import torch

import activation_cases as ac
import flow_twin
from helpers import golden, guarded, guards_intact, offset_view, same_bits

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


#: the parameters of the kernel, backward and module tests: away from the defaults where that costs nothing
PARAMS = {"smooth_leaky_relu": (0.3,), "leaky_relu": (0.1,), "learnable_leaky_relu": (), "smooth_tanh": (3.0, 0.05)}


def case(kind, logit=0.4):
    """The layer on the CPU in fp32 (the learnable kind with a slope that is not 1)."""
    m = ac.layer(kind, PARAMS[kind])
    if kind == "learnable_leaky_relu":
        with torch.no_grad():
            m.alpha_logit.fill_(logit)
    return m


def args_of(m, dev):
    """(kind, p0, p1, slope on the device) as the ops wrappers take them."""
    with torch.no_grad():
        slope = m._slope()
    return (m.kind, *m._numbers(), slope.to(dev) if slope is not None else None)


def inputs(shape, seed):
    return ac.planted(4 * torch.randn(shape, generator=torch.Generator().manual_seed(seed)))


def lines(m, v, inverse):
    out, lad = m._lines(v, inverse)
    return out, lad.flatten(1).sum(-1)


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the transform kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", (0, 2), ids=("aligned", "two_floats_in"))
@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=ids)
def test_kernel_against_float64_between_guard_bands(shape, kind, lead, dev):
    from fincflow_amd import _lib, ops
    align = 16 if lead == 0 else 8
    plan = _lib.pixel_plan("parts", "activation", *ac.dims(shape), align=align)
    assert plan == ac.PLANS[(shape, align)] and (lead == 0 or plan["io"] == 1)
    m = case(kind)
    args = args_of(m, dev)
    x = inputs(shape, 3)
    xg, xbuf = guarded(x, dev, lead)
    for direction, inverse in ((1, False), (-1, True)):
        with torch.no_grad():
            want, yard = lines(copy.deepcopy(m).double(), x.double(), inverse), lines(m, x, inverse)
        yg, ybuf = guarded(torch.zeros_like(x), dev, lead)
        y, ld = ops.finc_activation(xg, *args, direction, True, out=yg)
        torch.cuda.synchronize()
        assert y.data_ptr() == yg.data_ptr() and all(guards_intact(b, v) for b, v in ((xbuf, xg), (ybuf, yg)))
        ac.judge("kernel", ["y", "logdet"], [y, ld], want, yard, kind=kind, shape=list(shape), direction=direction, lead=lead)
        y_plain = ops.finc_activation(xg, *args, direction)[0]                     # without the log-det: the same y
        y2, ld2 = ops.finc_activation(xg, *args, direction, True)
        assert same_bits(y2, y) and same_bits(ld2, ld)                              # bit-stable over two calls
        assert same_bits(y_plain, y)
        # the zeros keep their bits through the leaky kinds and both take the identity branch (no log-derivative)
        if kind in ("leaky_relu", "learnable_leaky_relu"):
            assert same_bits(y.reshape(shape[0], -1)[0, :2], xg.reshape(shape[0], -1)[0, :2])
        # images are isolated: another image 1 (a NaN among its values) leaves image 0's y and logdet as they were
        # (in a buffer of xg's alignment class: the log-det's partials are sums of 64 thread items, which the wide form fills with four
        # elements each)
        moved = x.clone()
        moved[1] = 4 * torch.randn(shape[1:])
        moved.view(shape[0], -1)[1, 0] = float("nan")
        other = guarded(moved, dev, lead)[0]
        y3, ld3 = ops.finc_activation(other, *args, direction, True)
        assert same_bits(y3[0], y[0]) and same_bits(ld3[:1], ld[:1]) and same_bits(y3.view(shape[0], -1)[1, :1], other.view(shape[0], -1)[1, :1])
        assert not same_bits(y3[1], y[1]) and bool(torch.isfinite(ld3).all())      # (a NaN adds 0 to its image's log-det)
        inplace = xg.clone()
        assert same_bits(ops.finc_activation(inplace, *args, direction, out=inplace)[0], y)
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. multi-trip launches, by plan
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def multi_trip_data():
    """Per shape: x, grad_y, grad_logdet on the CPU -- drawn once, shared by the kinds."""
    out = {}
    for shape, _ in ac.MULTI_TRIP:
        gen = torch.Generator().manual_seed(11)
        out[shape] = (4 * torch.randn(shape, generator=gen), torch.randn(shape, generator=gen), torch.randn(shape[0], generator=gen))
    return out


@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("shape,align", ac.MULTI_TRIP, ids=ids)
def test_multi_trip_launches_match_one_trip_sub_batches(shape, align, kind, dev, multi_trip_data):
    """A thread that takes more than one trip through its loop (2 in the wide form, 5 in dwords, the last one partial): y, logdet,
    grad_x and the rebuilt x carry the bits of sub-batch calls that take ONE trip -- the log-det's partials are laid out per chunk of
    256 items, not per part, so its sum does not depend on the batch around an image -- and the slope's gradient is the float64 sum."""
    from fincflow_amd import _lib, ops
    B, C, HW = ac.dims(shape)
    plan = _lib.pixel_plan("parts", "activation", B, C, HW, align=align)
    assert plan == ac.PLANS[(shape, align)] and plan["trips"] >= 2
    SUB = 64
    assert _lib.pixel_plan("parts", "activation", SUB, C, HW, align=align)["trips"] == 1
    m = case(kind)
    args = args_of(m, dev)
    place = (lambda t: t.to(dev)) if align == 16 else (lambda t: offset_view(t, dev, lead=2))
    x, gy, gl = multi_trip_data[shape]
    xd, gyd, gld = place(x), place(gy), gl.to(dev)
    learnable = kind == "learnable_leaky_relu"
    for direction in (1, -1):
        y, ld = ops.finc_activation(xd, *args, direction, True)
        saved, mode = (xd, "forward") if direction == 1 else (place(y), "reverse")
        _, gx, gs = ops.finc_activation_backward(gyd, gld, saved, *args, mode=mode, need_gs=learnable)
        whole = [y, ld, gx]
        if direction == 1:
            xr, gxr, gsr = ops.finc_activation_backward(gyd, gld, place(y), *args, mode="rebuild", need_x=True, need_gs=learnable)
            assert same_bits(xr, ops.finc_activation(place(y), *args, -1)[0])      # the rebuilt x has the bits `reverse` returns
            whole += [xr, gxr]
        for b0 in (0, 192, B - SUB):
            sl = slice(b0, b0 + SUB)
            xs, gys = xd[sl], gyd[sl]
            assert xs.is_contiguous() and xs.data_ptr() % 16 == (0 if align == 16 else 8)
            y1, ld1 = ops.finc_activation(xs, *args, direction, True)
            parts = [y1, ld1, ops.finc_activation_backward(gys, gld[sl].contiguous(), saved[sl], *args, mode=mode)[1]]
            if direction == 1:
                parts += ops.finc_activation_backward(gys, gld[sl].contiguous(), place(y)[sl], *args, mode="rebuild", need_x=True)[:2]
            for name, a, b in zip(("y", "logdet", "grad_x", "x_rebuilt", "grad_x_rebuild"), parts, whole):
                assert same_bits(a, b[sl]), (kind, direction, b0, name)
        if learnable:
            # the slope's gradient against float64 autograd through the lines (and the rebuild mode's against the same sum)
            def cpu(dtype):
                t = copy.deepcopy(m).to(dtype)
                out, logdet = lines(t, x.to(dtype), direction < 0)
                ((out * gy.to(dtype)).sum() + (logdet * gl.to(dtype)).sum()).backward()
                s = torch.sigmoid(t.alpha_logit.detach())
                return [t.alpha_logit.grad / (s * (1 - s))]                        # d / d alpha: the chain to the logit undone
            want, yard = cpu(torch.float64), cpu(torch.float32)
            ac.judge("multi_trip_grad_slope", ["grad_slope"], [gs], want, yard, shape=list(shape), direction=direction)
            if direction == 1:
                ac.judge("multi_trip_grad_slope_rebuild", ["grad_slope"], [gsr], want, yard, shape=list(shape))
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the inverse
# ---------------------------------------------------------------------------------------------------------------------------------
BOX = [(kind, p) for kind in ("smooth_leaky_relu", "smooth_tanh") for p in ac.BOX[kind]]


@pytest.mark.parametrize("kind,params", BOX, ids=ids)
def test_inverse_over_the_parameter_box_against_float64_bisection(kind, params, dev):
    """linspace(-40, 40, 16001) and 3 * randn(3999) as a [2, 10000] tensor: the kernel's inverse against float64 bisection under the
    bar, finite, monotone over the grid; and the round trip reverse(forward(x))."""
    from fincflow_amd import ops
    m, m64 = ac.layer(kind, params), ac.layer(kind, params).double()
    gen = torch.Generator().manual_seed(0)
    y = torch.cat([torch.linspace(-40, 40, 16001), 3 * torch.randn(3999, generator=gen)]).view(2, 10000)
    with torch.no_grad():
        want, yard = ac.bisect64(m64, y.double()), m.reverse(y)
    args = (m.kind, *m._numbers(), None)
    x = ops.finc_activation(y.to(dev), *args, -1)[0]
    ac.judge("inverse_box", ["x"], [x], [want], [yard], kind=kind, params=list(params))
    flat = x.view(-1)[:16001]
    assert bool(torch.isfinite(x).all()) and bool((flat[1:] >= flat[:-1]).all())
    far = ops.finc_activation(torch.tensor([[1e30, -1e30, 3e38, -3e38]], device=dev), *args, -1)[0]
    assert bool(torch.isfinite(far).all())
    v = 4 * torch.randn(2, 10000, generator=gen)
    with torch.no_grad():
        yard = m.reverse(m(v)[0])
    back = ops.finc_activation(ops.finc_activation(v.to(dev), *args, 1)[0], *args, -1)[0]
    ac.judge("round_trip", ["x"], [back], [v.double()], [yard], kind=kind, params=list(params))


def test_the_kernels_run_the_derived_trip_count(dev):
    """The library these tests launch was compiled with the count the sweep of DESIGN 3.26 gives (tests/test_activations_host.py
    repeats that sweep), and the modules' PyTorch lines run the same count.  Two trips of margin mean that no accuracy test can tell 8
    trips from 9 -- that is what the margin is for -- so the count itself is held."""
    from fincflow_amd import glow, ops
    assert [ops.activation_inverse_trips(k) for k in ac.KINDS] == [ac.TRIPS, 0, 0, ac.TRIPS]
    assert glow.ACTIVATION_TRIPS == ac.TRIPS == ac.CONVERGED_AFTER + 2


def test_smooth_tanh_3_005_converges_where_the_recorded_reference_does_not(dev):
    from fincflow_amd import ops
    recorded = golden(ac.GOLDEN[:-4])
    y = torch.from_numpy(recorded["x"])
    m = ac.layer("smooth_tanh", (3.0, 0.05))
    with torch.no_grad():
        want, yard = ac.bisect64(copy.deepcopy(m).double(), y.double()), m.reverse(y)
    x = ops.finc_activation(y.to(dev), "smooth_tanh", 3.0, 0.05, None, -1)[0]
    ac.judge("smooth_tanh_3_0.05", ["x"], [x], [want], [yard])
    ref = ac.judge("smooth_tanh_3_0.05_reference_recording", ["x"], [torch.from_numpy(recorded["smooth_tanh_3_0.05/rev_of_x32"])], [want], [yard],
                   asserting=False)
    assert ref["x"] > 1e-3                                                          # the recording is of an iteration that did not settle


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the backwards
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("forward", "reverse", "rebuild"))
@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("shape", ((2, 3, 4, 4), (3, 2, 3, 5)), ids=ids)
def test_backward_modes_against_float64_autograd(shape, kind, mode, dev):
    """grad_input (and the learnable slope's gradient) of each mode against autograd through the written-out lines in float64: with
    grad_y alone, grad_logdet alone and both; then a grad_input that is not asked for, and one written over grad_y."""
    from fincflow_amd import _lib, ops
    m = case(kind)
    args = args_of(m, dev)
    learnable = kind == "learnable_leaky_relu"
    v = inputs(shape, 5)                                      # the input of the pass that is differentiated
    gen = torch.Generator().manual_seed(6)
    g, gl = torch.randn(shape, generator=gen), torch.randn(shape[0], generator=gen)
    inverse = mode == "reverse"

    def autograd(dtype, use_g, use_gl):
        t = copy.deepcopy(m).to(dtype)
        a = v.clone().to(dtype).requires_grad_(True)
        out, ld = lines(t, a, inverse)
        ((out * g.to(dtype)).sum() * float(use_g) + (ld * gl.to(dtype)).sum() * float(use_gl)).backward()
        grads = [a.grad]
        if learnable:
            s = torch.sigmoid(t.alpha_logit.detach())
            grads.append(t.alpha_logit.grad / (s * (1 - s)))
        return grads, out.detach()

    with torch.no_grad():
        out32 = lines(m, v, inverse)[0]
    # what each mode reads: the forward's input, the reverse's OUTPUT, the forward's OUTPUT -- the device's own
    saved = {"forward": v.to(dev), "reverse": ops.finc_activation(v.to(dev), *args, -1)[0],
             "rebuild": ops.finc_activation(v.to(dev), *args, 1)[0]}[mode]
    assert flow_twin.error(saved, (v if mode == "forward" else out32).double()) <= 1e-5
    names = ["grad_input"] + (["grad_slope"] if learnable else [])
    for use_g, use_gl in ((True, False), (False, True), (True, True)):
        (want, _), (yard, _) = autograd(torch.float64, use_g, use_gl), autograd(torch.float32, use_g, use_gl)
        gd, gld = (g.to(dev) if use_g else None), (gl.to(dev) if use_gl else None)
        xo, gx, gs = ops.finc_activation_backward(gd, gld, saved, *args, mode=mode, need_x=mode == "rebuild", need_gs=learnable)
        ac.judge("backward", names, [gx] + ([gs] if learnable else []), want, yard, kind=kind, shape=list(shape), mode=mode, grad_y=use_g,
                 grad_logdet=use_gl)
        again = ops.finc_activation_backward(gd, gld, saved, *args, mode=mode, need_x=mode == "rebuild", need_gs=learnable)
        assert all(a is None and b is None or same_bits(a, b) for a, b in zip(again, (xo, gx, gs)))
        if mode == "rebuild":
            assert same_bits(xo, ops.finc_activation(saved, *args, -1)[0])
            only_x = ops.finc_activation_backward(gd, gld, saved, *args, mode=mode, need_x=True, need_gx=False)
            assert same_bits(only_x[0], xo) and only_x[1] is None
        if learnable:
            only_gs = ops.finc_activation_backward(gd, gld, saved, *args, mode=mode, need_gx=False, need_gs=True)
            assert only_gs[1] is None and same_bits(only_gs[2], gs)
        if use_g:                                             # grad_input written over grad_y
            over = gd.clone()
            assert ops.finc_activation_backward(over, gld, saved, *args, mode=mode, out=over)[1].data_ptr() == over.data_ptr()
            assert same_bits(over, gx)
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the modules against their float64 CPU twins
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((3, 2, 3, 5), (4, 37)), ids=ids)
@pytest.mark.parametrize("kind", ac.KINDS)
def test_module_against_the_float64_twin(kind, shape, dev, monkeypatch):
    from fincflow_amd import _lib, ops
    m = case(kind).to(dev)
    t64, t32 = copy.deepcopy(m).cpu().double(), copy.deepcopy(m).cpu().float()
    x = inputs(shape, 9)
    gen = torch.Generator().manual_seed(2)
    r, s = torch.randn(shape, generator=gen), torch.randn(shape[0], generator=gen)
    calls = record_calls(monkeypatch)

    with torch.no_grad():
        got = [*m(x.to(dev)), m.reverse(x.to(dev)), *m.reverse_with_logdet(x.to(dev)), m.logdet(x.to(dev))]
        want, yard = ([*t(x.to(d)), t.reverse(x.to(d)), *t.reverse_with_logdet(x.to(d)), t.logdet(x.to(d))]
                      for t, d in ((t64, torch.float64), (t32, torch.float32)))
    assert calls == ["finc_activation_f32"] * 4, calls                              # ONE entry point per call (transform + its reduce)
    ac.judge("module_no_grad", ["y", "logdet", "reverse", "reverse_wl", "reverse_wl_logdet", "logdet_alone"], got, want, yard, kind=kind,
             shape=list(shape))

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
        return [out, ld, a.grad] + [p.grad for p in layer.parameters()]

    names = ["out", "logdet", "grad_x"] + ["grad_" + n for n, _ in m.named_parameters()]
    for reverse in (False, True):
        del calls[:]
        got = training(m, torch.float32, dev, reverse)
        assert calls == (["finc_activation_f32", "finc_activation_f32", "finc_activation_backward_f32", "finc_activation_backward_f32"]
                         if reverse else ["finc_activation_f32", "finc_activation_backward_f32"]), calls
        ac.judge("module_training", names, got, training(t64, torch.float64, "cpu", reverse), training(t32, torch.float32, "cpu", reverse),
                 kind=kind, shape=list(shape), reverse=reverse)

    # the step of a training backward that stores no activations: ONE launch, the input with the bits `reverse` returns
    from fincflow_amd.layers import BackwardNeeds
    with torch.no_grad():
        y, _ = m(x.to(dev))
        del calls[:]
        assert m.invertible_backward_supported(x.to(dev))
        xo, gx, gc, pg = m.backward_from_output(y, r.to(dev), s.to(dev), None, BackwardNeeds())
        assert calls == ["finc_activation_backward_f32"], calls
        assert same_bits(xo, m.reverse(y)) and gc is None and len(pg) == len(list(m.parameters()))

    def stored(layer, dtype, d):
        layer.zero_grad(set_to_none=True)
        a = x.clone().to(d).to(dtype).requires_grad_(True)
        out, ld = layer(a)
        ((out * r.to(d).to(dtype)).sum() + (ld * s.to(d).to(dtype)).sum()).backward()
        return [a.grad] + [p.grad for p in layer.parameters()]
    ac.judge("module_backward_from_output", names[2:], [gx, *pg], stored(t64, torch.float64, "cpu"), stored(t32, torch.float32, "cpu"),
             kind=kind, shape=list(shape))
    assert not _lib.fault_pending()


def test_learnable_slope_is_read_on_the_device_and_a_captured_reverse_replays(dev):
    """The learnable kind never reads its slope on the host: `reverse` captured in a HIP graph replays with the eager call's bits, and
    follows a slope that changed between replays (the graph holds the sigmoid line and the launch, not a number)."""
    from fincflow_amd import _lib
    m = case("learnable_leaky_relu").to(dev)
    z = inputs((4, 6, 4, 4), 1).to(dev)
    with torch.no_grad():
        eager = m.reverse(z).clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m.reverse(z)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert same_bits(out, eager)
        m.alpha_logit.fill_(-0.8)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, m.reverse(z)) and not same_bits(out, eager)
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. stacks that hold the layers, through every view
# ---------------------------------------------------------------------------------------------------------------------------------
def stack(first_kind, second_kind, seed=1):
    """[Squeeze, FastFlowUnit, activation, ActNorm, Conv1x1, Coupling], a SplitPrior, then the same again, on 3 x 8 x 8 images."""
    import numpy as np
    from fincflow_amd import FastFlowUnit, FlowSequential, glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    layers, size = [], (3, 8, 8)
    for level, kind in enumerate((first_kind, second_kind)):
        layers.append(glow.Squeeze())
        size = (size[0] * 4, size[1] // 2, size[2] // 2)
        layers += [FastFlowUnit(size[0], size[0], (3, 3)), case(kind, logit=0.4 - 0.3 * level), glow.ActNorm(size[0]), glow.Conv1x1(size[0]),
                   glow.Coupling(size, width=16)]
        if level == 0:
            layers.append(glow.SplitPrior(size, glow.GaussianPrior, width=16))
            size = (size[0] // 2, size[1], size[2])
    model = FlowSequential(glow.GaussianPrior(size), *layers)
    return flow_twin.randomise(model, seed=seed, actnorm=True)


STACKS = (("smooth_leaky_relu", "smooth_leaky_relu"), ("smooth_tanh", "learnable_leaky_relu"))


@pytest.fixture(scope="module", params=STACKS, ids=lambda p: "+".join(p))
def models(request, dev):
    """(the HIP model, its float64 twin, its float32 twin, x)."""
    model = stack(*request.param).to(dev)
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
    assert calls.count("finc_activation_f32") == 6, calls                           # two layers in each of log_prob, encode, decode
    ac.judge("stack_encode", ["log_prob", "z0", "z1", "log_prob_encode"], [lp, *zs, lpe], want, yard)
    with torch.no_grad():
        want, yard = (t.decode([z.cpu().to(d) for z in zs]) for t, d in ((t64, torch.float64), (t32, torch.float32)))
    ac.judge("stack_decode", ["x"], [back], [want], [yard])
    ac.judge("stack_decode_of_encode", ["x"], [back], [x.double()], [t32.decode(t32.encode(x)[0]).detach()])


@pytest.mark.parametrize("invertible", (False, True), ids=("stored", "invertible"))
def test_stack_training_gradients(models, dev, invertible):
    """-log_prob.mean() and every parameter's gradient, with stored activations and with `invertible_backward` -- where each
    activation sits INSIDE a run of layers that differentiate from their output, not at the end of one."""
    from fincflow_amd import glow, layers
    model, t64, t32, x = models
    acts = [m for m in model.sequence_modules if isinstance(m, glow._Activation)]
    assert len(acts) == 2

    def one_pass(net, d, dtype, masks=None):
        net.zero_grad(set_to_none=True)
        ctx = flow_twin.recorded_masks(net) if masks is None else flow_twin.replayed_masks(net, masks)
        with ctx as rec:
            lp = net.log_prob(x.to(d).to(dtype))
            loss = -lp.mean()
            nodes = set()
            todo = [loss.grad_fn]
            while todo:
                fn = todo.pop()
                if fn is None or fn in nodes:
                    continue
                nodes.add(fn)
                todo += [f for f, _ in fn.next_functions]
            loss.backward()
        if masks is None:
            rec = {n: v[-1:] for n, v in rec.items()}                               # the call whose branch the gradients took
        else:
            flow_twin.mask_unit_grads(net)
        params = dict(net.named_parameters())
        return [lp.detach()] + [params[n].grad for n in sorted(params)], rec, nodes

    model.invertible_backward = invertible
    try:
        if invertible:
            mods = list(model.sequence_modules)
            split = [i for i, m in enumerate(mods) if isinstance(m, glow.SplitPrior)][0]
            with torch.no_grad():
                mid = model._forward_layers(mods[:split + 1], x.to(dev), None)[0]
            for run, inp in ((mods[:split], x.to(dev)), (mods[split + 1:], mid)):
                at = [i for i, m in enumerate(run) if isinstance(m, glow._Activation)]
                assert len(at) == 1 and 0 < at[0] < len(run) - 1
                assert model._invertible_run_end(run, 0, inp, None) == len(run)
        got, masks, nodes = one_pass(model, dev, torch.float32)
        runs = [n for n in nodes if type(n).__name__.startswith("_InvertibleRunFunction")]
        assert len(runs) == (2 if invertible else 0), [type(n).__name__ for n in nodes]
    finally:
        model.invertible_backward = False
    want, yard = one_pass(t64, "cpu", torch.float64, masks)[0], one_pass(t32, "cpu", torch.float32, masks)[0]
    names = ["log_prob"] + ["grad_" + n for n in sorted(dict(model.named_parameters()))]
    grads = dict(zip(names, zip(got, want, yard)))
    for n, mask in flow_twin.stored_masks(model).items():                           # (the corner taps under the units' mask: exact zeros)
        assert not bool(grads["grad_" + n][0].cpu()[mask == 0].any())
    ac.judge("stack_training", names, got, want, yard, invertible=invertible)
    assert any("alpha_logit" in n for n in names) == any(isinstance(m, glow.LearnableLeakyRelu) for m in acts)
    assert layers is not None


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
        ac.judge("stack_" + view, ["x", "log_q"][:len(got)], got, both[0], both[1])
    with torch.no_grad():                                                           # log q of a sample is log_prob of that sample
        s, lq = model.sample_with_log_prob(4)
        lp = model.log_prob(s)
        want, yard = t64.log_prob(s.cpu().double()), t32.log_prob(s.cpu())
    ac.judge("stack_log_q_is_log_prob", ["log_q", "log_prob"], [lq, lp], [want, want], [yard, yard])


def test_stack_reparameterised_sampling(models, dev):
    """rsample_with_log_prob: values and every parameter's gradient (the reverse chain recorded inside ops.reverse_grad())."""
    model, t64, t32, x = models

    def run(net, draws=None, masks=None):
        net.zero_grad(set_to_none=True)
        noise = flow_twin.recorded_noise(net) if draws is None else flow_twin.replayed_noise(net, draws)
        relus = flow_twin.recorded_masks(net) if masks is None else flow_twin.replayed_masks(net, masks)
        with noise as rec, relus as pattern:
            xs, lq = net.rsample_with_log_prob(4)
            ((xs * xs).sum() + lq.sum()).backward()
        if masks is None:
            pattern = {n: v[-1:] for n, v in pattern.items()}
        else:
            flow_twin.mask_unit_grads(net)
        params = dict(net.named_parameters())
        return [xs.detach(), lq.detach()] + [params[n].grad for n in sorted(params) if params[n].grad is not None], rec, pattern

    got, draws, masks = run(model)
    want, yard = run(t64, draws, masks)[0], run(t32, draws, masks)[0]
    assert len(got) == len(want) == len(yard) and len(got) > 10
    ac.judge("stack_rsample_with_log_prob", ["x", "log_q"] + ["grad_%d" % k for k in range(len(got) - 2)], got, want, yard)
    model.zero_grad(set_to_none=True)


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
