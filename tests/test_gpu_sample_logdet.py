"""Sampling with the log-density on the GPU (include/finc.h: finc_coupling_reverse_logdet_f32,
finc_coupling_reverse_logdet_backward_f32), `reverse_with_logdet` of glow.Coupling / SplitPrior / ActNorm / Conv1x1 and
FlowSequential.sample_with_log_prob / rsample_with_log_prob: DESIGN 3.17.

Reference everywhere: the formulas of include/finc.h (layers/coupling.py:79-101) and the modules in float64 on the CPU, autograd for
gradients.  Bar: 1e-5 in helpers.rel_err, the bar of tests/test_gpu_reverse_backward.py; whole chains at that file's CHAIN_TOL, 5e-5.
Every Conv2dZero is randomised, ActNorm has a non-zero log_scale, Conv1x1 a W that is not orthogonal, and every comparison of a log-det
first asserts that it is not small (at the zero initialisation s == 0, and a log-det of zero proves nothing).  Every case prints what
it achieved and appends it to the parity report (kind `sample_logdet`).
"""
import copy
import functools
import itertools

import numpy as np
import pytest
import torch

import test_gpu_coupling as cpl
import test_sample_logdet_host as host
from helpers import coupling_ref, offset_view, rel_err, report, same_bits
from test_gpu_bounds import F32, check_bounds, check_isolation, grads, judge_outputs, pixel_inputs, run
from test_gpu_inverse_backward import CHAIN_TOL

pytestmark = pytest.mark.gpu

TOL = 1e-5
# the dword path with HW % 4 != 0; the 16-byte path with one workgroup per image; a mid-sized one; several parts per image and a
# partial last pass (3 pairs x 400 pieces = 1200 items on 5 parts of 256 threads)
SHAPES = [(3, 4, 5, 3), (2, 8, 4, 4), (3, 12, 8, 8), (2, 6, 40, 40)]
OFFSET = (2, 12, 8, 8)                  # a 16-byte shape forced onto dwords by a view one float into its allocation
CASES = [(s, False) for s in SHAPES] + [(OFFSET, True)]
NAMES = ("grad_x", "grad_raw", "grad_a", "grad_b")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# references (float64, once per shape)
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_reverse_logdet(x, raw, a, b):
    """float64: y of the reverse direction and the FORWARD map's log-det, sum s per image (it does not depend on x)."""
    return cpl.ref_transform(x, raw, a, b, -1), cpl.ref_transform(x, raw, a, b, 1)[1]


@functools.lru_cache(maxsize=None)
def kernel_case(shape):
    """(x, raw, a, b, grad_y, grad_logdet) of tests/test_gpu_coupling.py, the float64 (y, logdet) and the float64 gradients of
    sum(y * grad_y) + sum(logdet * grad_logdet)."""
    x, raw, a, b, gy, gl = cpl.case(shape)
    leaves = [v.double().requires_grad_(True) for v in (x, raw, a, b)]
    y, ld = ref_reverse_logdet(*leaves)
    ((y * gy.double()).sum() + (ld * gl.double()).sum()).backward()
    assert float(ld.detach().abs().max()) > 0.1, ld
    return (x, raw, a, b, gy, gl), (y.detach().numpy(), ld.detach().numpy()), [v.grad.numpy() for v in leaves]


def judge(kind, shape, names, got, ref, tol=TOL):
    errs = {n: rel_err(g.detach().cpu().numpy(), r) for n, g, r in zip(names, got, ref)}
    print(kind, shape, errs)
    report("sample_logdet", case=kind, shape=list(shape), **errs)
    for n, e in errs.items():
        assert e <= tol, (kind, shape, n, e)


def mover(dev, offset):
    return (lambda v: offset_view(v, dev)) if offset else (lambda v: v.to(dev))


# ---------------------------------------------------------------------------------------------------------------------------------
# the two kernels through ops
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_reverse_with_logdet_against_the_float64_formula(shape, offset, dev):
    from fincflow_amd import ops
    (x, raw, a, b, _, _), (y_ref, ld_ref), _ = kernel_case(shape)
    move = mover(dev, offset)
    xd, rawd, ad, bd = move(x), move(raw), a.to(dev), b.to(dev)
    assert not offset or all(v.data_ptr() % 16 == 4 for v in (xd, rawd))
    y, ld = ops.finc_coupling_reverse_logdet(xd, rawd, ad, bd, out=move(torch.zeros_like(x)))
    y2, ld2 = ops.finc_coupling_reverse_logdet(xd, rawd, ad, bd, out=move(torch.zeros_like(x)))
    plain = ops.finc_coupling(xd, rawd, ad, bd, -1, out=move(torch.zeros_like(x)))[0]
    buf = move(x)
    inplace, ld3 = ops.finc_coupling_reverse_logdet(buf, rawd, ad, bd, out=buf)
    torch.cuda.synchronize()
    assert ld.shape == (shape[0],) and float(ld.abs().max()) > 0.1
    judge("kernel" + ("_offset" if offset else ""), shape, ("y", "logdet"), (y, ld), (y_ref, ld_ref))
    assert same_bits(y, plain)                                       # the log-det is a by-product: the y of the plain reverse
    assert same_bits(y, y2) and same_bits(ld, ld2)                   # fixed-order sums: two calls, the same bits
    assert inplace is buf and same_bits(inplace, y) and same_bits(ld3, ld)


def test_an_empty_batch_launches_nothing(dev, monkeypatch):
    from fincflow_amd import ops
    calls = record_calls(monkeypatch)
    x = torch.empty(0, 4, 5, 3, device=dev)
    a = torch.ones(4, device=dev)
    y, ld = ops.finc_coupling_reverse_logdet(x, x.clone(), a, a)
    assert y.shape == x.shape and ld.shape == (0,)
    got = ops.finc_coupling_reverse_logdet_backward(x, ld, x, x.clone(), a, a)
    assert got[0].shape == x.shape and not bool(got[2].any()) and not bool(got[3].any()) and calls == []


def backward_args(dev, shape, offset):
    from fincflow_amd import ops
    (x, raw, a, b, gy, gl), _, ref = kernel_case(shape)
    move = mover(dev, offset)
    rawd, ad, bd = move(raw), a.to(dev), b.to(dev)
    y = ops.finc_coupling_reverse_logdet(move(x), rawd, ad, bd, out=move(torch.zeros_like(x)))[0]      # the reverse's own output
    return (move(gy), gl.to(dev), y, rawd, ad, bd), ref


@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_all_four_gradients_against_float64_autograd(shape, offset, dev):
    from fincflow_amd import ops
    args, ref = backward_args(dev, shape, offset)
    got = ops.finc_coupling_reverse_logdet_backward(*args)
    again = ops.finc_coupling_reverse_logdet_backward(*args)
    gy, _, y, rawd, ad, bd = args
    none = ops.finc_coupling_reverse_logdet_backward(gy, None, y, rawd, ad, bd)
    sibling = ops.finc_coupling_reverse_backward(gy, y, rawd, ad, bd)
    torch.cuda.synchronize()
    judge("backward" + ("_offset" if offset else ""), shape, NAMES, got, ref)
    half = shape[1] // 2
    assert torch.equal(got[0][:, :half], gy[:, :half])               # the untouched half's gradient passes through
    for n, g, h, z, s in zip(NAMES, got, again, none, sibling):
        assert same_bits(g, h), n                                    # fixed-order sums: two calls, the same bits
        assert same_bits(z, s), n                                    # without grad_logdet: the sibling's bits
    assert not same_bits(got[1], none[1])                            # (and grad_logdet does reach grad_raw)


def test_every_combination_of_skipped_outputs(dev):
    """Straight through the C ABI on (2, 16, 5, 3): a skipped output is NULL, a buffer that was not passed is not written, and the
    outputs that are asked for have the bits of the call that asks for all of them."""
    from fincflow_amd import _lib, ops
    shape = (2, 16, 5, 3)
    B, C, H, W = shape
    L = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    args, _ = backward_args(dev, shape, False)
    full = ops.finc_coupling_reverse_logdet_backward(*args)
    ws = torch.empty(L.finc_coupling_workspace_bytes(B, C, H * W), dtype=torch.uint8, device=dev)
    f = L.finc_coupling_reverse_logdet_backward_f32
    ins = [v.data_ptr() for v in args]
    for want in itertools.product((False, True), repeat=4):
        bufs = [torch.full_like(args[0], 7.0) for _ in range(2)] + [torch.full((C,), 7.0, device=dev) for _ in range(2)]
        ptrs = [v.data_ptr() if w else None for v, w in zip(bufs, want)]
        rc = f(*ins, *ptrs, B, C, H * W, ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        if not any(want):
            assert rc == 1
            continue
        assert rc == 0, (want, rc)
        for v, w, ref in zip(bufs, want, full):
            assert same_bits(v, ref) if w else bool((v == 7.0).all()), want
    gx = torch.empty_like(args[0])                                   # without the per-channel sums the call needs no workspace
    rc = f(*ins, gx.data_ptr(), None, None, None, B, C, H * W, None, 0, st)
    torch.cuda.synchronize()
    assert rc == 0 and same_bits(gx, full[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# guard bands and problem isolation (tests/test_gpu_bounds.py's machinery)
# ---------------------------------------------------------------------------------------------------------------------------------
def bounds_spec(op, shape, dev):
    from fincflow_amd import _lib
    L = _lib.lib()
    B, C, H, W = shape
    HW, half = H * W, C // 2
    T = pixel_inputs(shape)
    D = {k: v.to(dev) for k, v in T.items()}
    d64 = {k: v.double() for k, v in T.items()}
    image = (B // 2,)
    sym, ws = "finc_coupling_" + op + "_f32", L.finc_coupling_workspace_bytes(B, C, HW)
    if op == "reverse_logdet":
        ins, acts = dict(x=D["x"], raw=D["raw"], a=D["a"], b=D["b"]), ("x", "raw", "y")
        outs = dict(y=(shape, F32), logdet=((B,), F32))
        argf = lambda p, w, n: (p["x"], p["raw"], p["a"], p["b"], p["y"], p["logdet"], B, C, HW, w, n, None)
        ld = coupling_ref(d64["x"], d64["raw"], d64["a"], d64["b"], 1)[1]
        assert float(ld.abs().max()) > 0.1
        refs, alias = dict(y=coupling_ref(d64["x"], d64["raw"], d64["a"], d64["b"], -1)[0].numpy(), logdet=ld.numpy()), dict(y="x")
        # one image's raw reaches that image's y and log-det and nothing else; its x reaches its y only
        spots = [("raw", image, dict(y=image, logdet=image)), ("x", image, dict(y=image, logdet=None))]
    else:
        y32 = coupling_ref(T["x"], T["raw"], T["a"], T["b"], -1)[0].contiguous()        # the reverse's output, as the kernel is handed it
        ins, acts = dict(gy=D["gy"], gl=D["gl"], y=y32.to(dev), raw=D["raw"], a=D["a"], b=D["b"]), ("gy", "y", "raw", "gx", "graw")
        outs = dict(gx=(shape, F32), graw=(shape, F32), ga=((C,), F32), gb=((C,), F32))
        argf = lambda p, w, n: (p["gy"], p["gl"], p["y"], p["raw"], p["a"], p["b"], p["gx"], p["graw"], p["ga"], p["gb"], B, C, HW, w, n, None)
        both = lambda x, raw, a, b: (coupling_ref(x, raw, a, b, -1)[0], coupling_ref(x, raw, a, b, 1)[1])
        g = grads(both, [T["x"], T["raw"], T["a"], T["b"]], [T["gy"], T["gl"]])
        refs, alias = dict(zip(("gx", "graw", "ga", "gb"), g)), None
        j = half // 2
        pair = (slice(None), slice(2 * j, 2 * j + 2))
        spots = [("raw", image, dict(gx=image, graw=image)), ("y", image, dict(gx=None, graw=image)),
                 ("gl", image, dict(gx=None, graw=image)),
                 ("raw", pair, dict(ga=pair[1], gb=pair[1], gx=(slice(None), half + j), graw=pair))]
    return dict(sym=sym, ins=ins, outs=outs, ws=ws, argf=argf, acts=acts, alias=alias, refs=refs, spots=spots)


@pytest.mark.parametrize("shape", [(3, 4, 5, 3), (5, 6, 9, 8)], ids=str)
@pytest.mark.parametrize("op", ["reverse_logdet", "reverse_logdet_backward"])
def test_guard_bands_and_problem_isolation(op, shape, dev):
    """As tests/test_gpu_reverse_backward.py::test_guard_bands_and_problem_isolation: the 16-byte form and, one float into every
    activation's allocation, the dword form, each between NaN guards with an exactly-sized NaN workspace -- nothing is written outside
    y, logdet or the gradients; y over x in place; a NaN / +inf in one image (or channel pair) reaching only what the operation's
    definition lets it reach: changing one image changes only that image's log-det."""
    spec = bounds_spec(op, shape, dev)
    call = lambda ins, guard=False, lead=(), alias=None: run(dev, spec["sym"], spec["argf"], ins, spec["outs"], spec["ws"], guard, lead, alias)
    wide = "16-byte" if shape[2] * shape[3] % 4 == 0 else "dword"
    plain = check_bounds(op, lambda guard: call(spec["ins"], guard), dict(kernel=spec["sym"], form=wide), judge_outputs(spec["refs"]),
                         shape=list(shape))
    shifted = check_bounds(op, lambda guard: call(spec["ins"], guard, spec["acts"]), dict(kernel=spec["sym"], form="dword"),
                           judge_outputs(spec["refs"]), shape=list(shape), lead_floats=1)
    if wide == "dword":
        assert all(same_bits(plain.outs[k], shifted.outs[k]) for k in plain.outs)      # one kernel form, one answer
    if spec["alias"]:
        for lead, base in (((), plain), (spec["acts"], shifted)):
            inplace = check_bounds(op, lambda guard: call(spec["ins"], guard, lead, spec["alias"]),
                                   dict(kernel=spec["sym"], in_place=True), shape=list(shape), lead_floats=len(lead) and 1)
            assert all(same_bits(base.outs[k], inplace.outs[k]) for k in base.outs), "in place differs from out of place"
    for lead in ((), spec["acts"]):
        check_isolation(dev, op, lambda ins: call(ins, False, lead), spec["ins"], spec["spots"],
                        dict(kernel=spec["sym"], form="dword" if lead else wide), shape=list(shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------------------
def record_calls(monkeypatch):
    """Every entry point that goes through ops._call, by name, in order."""
    from fincflow_amd import ops
    names, real = [], ops._call

    def recorded(name, *args, **kwargs):
        names.append(name)
        return real(name, *args, **kwargs)
    monkeypatch.setattr(ops, "_call", recorded)
    return names


FWD, BWD = "finc_coupling_reverse_logdet_f32", "finc_coupling_reverse_logdet_backward_f32"
OLD = ("finc_coupling_f32", "finc_coupling_reverse_backward_f32", "finc_coupling_backward_f32")


def make(kind, C, hw):
    """(module, context channels, channels of `reverse`'s input), randomised as the host tests do."""
    from fincflow_amd import glow
    torch.manual_seed(11)
    np.random.seed(11)
    if kind == "actnorm":
        return host._randomise(glow.ActNorm(C)), None, C
    if kind == "conv1x1":
        return host._randomise(glow.Conv1x1(C)), None, C
    if kind == "split":
        return host._randomise(glow.SplitPrior((C,) + hw, glow.GaussianPrior, width=32)), None, C // 2
    n_context = 5 if kind == "coupling_context" else None
    return host._randomise(glow.Coupling((C,) + hw, width=32, n_context=n_context)), n_context, C


def fix_base_draw(m, x2):
    """SplitPrior draws its second half: the draw is fixed, on the module's own device and dtype."""
    p = next(m.parameters())
    m.base.sample = lambda n, context=None: (x2.to(p.device, p.dtype), None)


def module_loss(out, logdet, w):
    return out.square().mean() + (w * logdet).sum()


def float64_module(m, x, ctx, w):
    """out = reverse(x), logdet = forward(out)[1] on the float64 module; gradients of the loss for x, (the context,) every parameter."""
    xa = x.double().requires_grad_(True)
    ca = None if ctx is None else ctx.double().requires_grad_(True)
    out = m.reverse(xa, ca)
    logdet = torch.as_tensor(m.forward(out, ca)[1]).expand(len(x))
    leaves = [xa] + ([] if ca is None else [ca]) + list(m.parameters())
    g = torch.autograd.grad(module_loss(out, logdet, w.double()), leaves)
    return [out.detach().numpy(), logdet.detach().numpy()] + [v.numpy() for v in g]


MODULE_CASES = [(k, hw) for hw in ((8, 8), (5, 3)) for k in ("coupling", "coupling_context", "split", "actnorm", "conv1x1")]


@pytest.mark.parametrize("kind,hw", MODULE_CASES, ids=str)
def test_modules_inside_reverse_grad_against_the_float64_module(kind, hw, dev, monkeypatch):
    import fincflow_amd
    B, C = 3, 12
    m, n_context, c_in = make(kind, C, hw)
    torch.manual_seed(C + sum(hw))
    x, w = torch.randn(B, c_in, *hw), torch.randn(B)
    ctx = None if n_context is None else torch.randn(B, n_context, *hw)
    x2 = torch.randn(B, C // 2, *hw)
    m64, md = copy.deepcopy(m).double(), copy.deepcopy(m).to(dev)
    if kind == "split":
        fix_base_draw(m64, x2), fix_base_draw(md, x2)
    ref = float64_module(m64, x, ctx, w)
    assert float(np.abs(ref[1]).max()) > 0.1, ref[1]

    calls = record_calls(monkeypatch)
    xa = x.to(dev).requires_grad_(True)
    ca = None if ctx is None else ctx.to(dev).requires_grad_(True)
    with fincflow_amd.reverse_grad():
        out, logdet = md.reverse_with_logdet(xa, ca)
    assert logdet.shape == (B,) and out.requires_grad and logdet.requires_grad
    coupling = kind in ("coupling", "coupling_context", "split")
    if coupling:
        assert calls == [FWD], calls
        assert type(out.grad_fn).__name__ == "_FincCouplingReverseLogdetFunctionBackward"
    else:
        assert FWD not in calls and len(calls) == 1, calls           # ActNorm's / the mix's own launch, nothing else
    del calls[:]
    leaves = [xa] + ([] if ca is None else [ca]) + list(md.parameters())
    g = torch.autograd.grad(module_loss(out, logdet, w.to(dev)), leaves)
    if coupling:
        assert calls.count(BWD) == 1 and not any(n in calls for n in OLD), calls
    names = ["out", "logdet", "grad_input"] + ([] if ctx is None else ["grad_context"]) + ["grad_" + n for n, _ in md.named_parameters()]
    assert len(names) == len(ref)
    judge("module_" + kind, (B, C) + hw, names, [out, logdet] + list(g), ref)

    # the inference path: the same numbers from the launch without a graph, bit for bit where the same kernel ran
    del calls[:]
    with torch.no_grad():
        out0, logdet0 = md.reverse_with_logdet(xa.detach(), None if ca is None else ca.detach())
        plain = md.reverse(xa.detach(), None if ca is None else ca.detach())
    assert not out0.requires_grad and same_bits(out0, plain)
    if coupling:
        assert calls.count(FWD) == 1, calls
    judge("module_inference_" + kind, (B, C) + hw, ("out", "logdet"), (out0, logdet0), ref[:2])


@pytest.mark.parametrize("kind", ["coupling", "coupling_context", "split", "actnorm", "conv1x1"])
def test_outside_the_context_and_in_fp64_the_pytorch_lines_are_taken(kind, dev, monkeypatch):
    import fincflow_amd
    B, C, hw = 3, 12, (5, 3)
    m, n_context, c_in = make(kind, C, hw)
    torch.manual_seed(5)
    x, w = torch.randn(B, c_in, *hw), torch.randn(B)
    ctx = None if n_context is None else torch.randn(B, n_context, *hw)
    x2 = torch.randn(B, C // 2, *hw)
    m64 = copy.deepcopy(m).double()
    if kind == "split":
        fix_base_draw(m64, x2)
    ref = float64_module(m64, x, ctx, w)
    calls = record_calls(monkeypatch)
    to = lambda v, f: None if v is None else f(v)

    def run_on(md, xa, ca, inside):
        if kind == "split":
            fix_base_draw(md, x2)
        with (fincflow_amd.reverse_grad() if inside else torch.enable_grad()):
            out, logdet = md.reverse_with_logdet(xa, ca)
        assert out.requires_grad and logdet.requires_grad and logdet.shape == (B,)
        assert "Finc" not in type(out.grad_fn).__name__ and "Finc" not in type(logdet.grad_fn).__name__
        assert calls == [], calls                                    # no entry point of the library at all
        leaves = [xa] + ([] if ca is None else [ca]) + list(md.parameters())
        return [out, logdet] + list(torch.autograd.grad(module_loss(out, logdet, w.to(xa.device, xa.dtype)), leaves))
    names = ["out", "logdet", "grad_input"] + ([] if ctx is None else ["grad_context"]) + ["grad_" + n for n, _ in m.named_parameters()]
    # fp32 on the device, outside reverse_grad(): recorded on PyTorch's lines
    md = copy.deepcopy(m).to(dev)
    got = run_on(md, x.to(dev).requires_grad_(True), to(ctx, lambda v: v.to(dev).requires_grad_(True)), False)
    judge("outside_" + kind, (B, C) + hw, names, got, ref)
    # fp64 on the device, inside it: the HIP gates are for fp32
    md = copy.deepcopy(m).double().to(dev)
    got = run_on(md, x.double().to(dev).requires_grad_(True), to(ctx, lambda v: v.double().to(dev).requires_grad_(True)), True)
    # (both sides float64: 1.1e-16 per rounding, growing at worst linearly over the <= 1e5 terms of the net's sums, times ten)
    judge("fp64_" + kind, (B, C) + hw, names, got, ref, tol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole chain
# ---------------------------------------------------------------------------------------------------------------------------------
def build_model(dev):
    from fincflow_amd import glow
    torch.manual_seed(0)
    np.random.seed(0)
    model = glow.create_model(num_blocks=2, block_size=2, actnorm=True, split_prior=True, image_size=(4, 8, 8), preprocess=False,
                              coupling_width=16)
    gen = torch.Generator().manual_seed(1)
    r = lambda shape, s: s * torch.randn(shape, generator=gen)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, glow.ActNorm):
                m.log_scale.copy_(r(m.log_scale.shape, 0.1))
                m.translation.copy_(r(m.translation.shape, 0.1))
                m.mark_initialized()
            elif isinstance(m, glow.Conv2dZero):
                for p in (m.weight, m.bias, m.logs):
                    p.copy_(r(p.shape, 0.05))
            elif isinstance(m, glow.Conv1x1):
                m.W.mul_(1.1).add_(r(m.W.shape, 0.05))
                assert abs(float(torch.slogdet(m.W)[1])) > 0.1
    return model.to(dev)


def fix_latents(model, n, monkeypatch, seed=3):
    """The base draw and every SplitPrior's draw fixed (device tensors made once: replayable)."""
    from fincflow_amd import glow
    dev = next(model.parameters()).device
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, *model.base_distribution.size, generator=gen).to(dev)
    monkeypatch.setattr(model.base_distribution, "sample", lambda n_samples, context=None: (z, None))
    for m in model.modules():
        if isinstance(m, glow.SplitPrior):
            x2 = torch.randn(n, *m.base.size, generator=gen).to(dev)
            monkeypatch.setattr(m.base, "sample", lambda n_samples, context=None, x2=x2: (x2, None))
    return z


def float64_log_prob(model, x, monkeypatch):
    """`model.double().cpu().log_prob(x.double().cpu())`: the unit has no CPU path, so its forward is the PyTorch restatement of
    tests/test_sample_logdet_host.py (checked there against nothing but itself; here it stands against the HIP inverse)."""
    from fincflow_amd import FastFlowUnit, ops
    m64 = build_model(torch.device("cpu"))                 # (a used unit's cache holds a lock: no deepcopy; same layers, same state)
    m64.load_state_dict(model.state_dict())
    m64.double()
    owner = {u.conv_tl.conv.weight.data_ptr(): u for u in m64.modules() if isinstance(u, FastFlowUnit)}
    monkeypatch.setattr(ops.PackedWeights, "forward", lambda self, t, weights, G, orient, **kw: host._unit_forward(owner[weights[0].data_ptr()], t))
    monkeypatch.setattr(ops.PackedWeights, "forward_affine", lambda self, *a, **kw: None)
    with torch.no_grad():
        return m64.log_prob(x.double().cpu())


def test_sample_with_log_prob_against_log_prob_in_float64(dev, monkeypatch):
    from fincflow_amd import glow
    model = build_model(dev)
    z = fix_latents(model, 4, monkeypatch)
    calls = record_calls(monkeypatch)
    x, log_q = model.sample_with_log_prob(4)
    record = list(calls)
    with torch.no_grad():
        x_plain, _ = model.sample(4)
    torch.cuda.synchronize()
    assert x.shape == (4, 4, 8, 8) and log_q.shape == (4,) and not x.requires_grad and not log_q.requires_grad
    assert same_bits(x, x_plain)                                     # the pass of `sample`, folds included
    # the folds ran: an ActNorm folded into the unit behind it launches no ActNorm kernel of its own
    n_actnorm = sum(isinstance(m, glow.ActNorm) for m in model.modules())
    n_coupling = sum(isinstance(m, (glow.Coupling)) for m in model.modules())
    assert record.count("finc_actnorm_f32") < n_actnorm == 4, record
    assert "finc_pack_inverse_weights_affine_f32" in record, record
    assert record.count(FWD) == n_coupling == 5 and "finc_coupling_f32" not in record, record
    logdet = log_q - model.base_distribution.log_prob(z)
    assert float(logdet.abs().max()) > 0.1, logdet
    ref = float64_log_prob(model, x, monkeypatch)
    err = rel_err(log_q.cpu().numpy(), ref.numpy())
    print("chain: log_q against log_prob(x) in float64 %.3e (bar %.0e); folded ActNorms: %d of %d"
          % (err, CHAIN_TOL, n_actnorm - record.count("finc_actnorm_f32"), n_actnorm))
    report("sample_logdet", case="chain_log_q", err=err, folded=n_actnorm - record.count("finc_actnorm_f32"))
    assert err <= CHAIN_TOL, err


def gates_off(monkeypatch):
    """The HIP gates of the recorded reverse answer False: PyTorch's lines, log-det included."""
    from fincflow_amd import glow
    for cls in (glow.Coupling, glow.ActNorm, glow.Conv1x1):
        monkeypatch.setattr(cls, "_hip_reverse_grad", lambda self, *a, **k: False)


def test_rsample_with_log_prob_against_the_same_chain_with_the_gates_off(dev, monkeypatch):
    from fincflow_amd import _lib
    model = build_model(dev)
    fix_latents(model, 4, monkeypatch)
    calls = record_calls(monkeypatch)
    names = [n for n, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]

    def chain_grads():
        model.zero_grad()
        x, log_q = model.rsample_with_log_prob(4)
        assert x.requires_grad and log_q.requires_grad and log_q.shape == (4,)
        (log_q - x.square().flatten(1).sum(1)).mean().backward()
        torch.cuda.synchronize()
        return x.detach(), log_q.detach(), [p.grad for p in params]
    x_on, q_on, on = chain_grads()
    assert calls.count(FWD) == 5 and calls.count(BWD) == 5 and not any(n in calls for n in OLD), calls
    for n, g in zip(names, on):
        assert g is not None and bool(torch.isfinite(g).all()), n
    on = [g.clone() for g in on]
    _lib.raise_if_faulted("test_rsample_with_log_prob_against_the_same_chain_with_the_gates_off")
    gates_off(monkeypatch)
    del calls[:]
    x_off, q_off, off = chain_grads()
    assert FWD not in calls and BWD not in calls
    e_x, e_q = rel_err(x_on.cpu().numpy(), x_off.cpu().numpy()), rel_err(q_on.cpu().numpy(), q_off.cpu().numpy())
    worst, where = 0.0, None
    for n, a, b in zip(names, on, off):
        assert b is not None and float(b.abs().max()) > 0, n
        e = rel_err(a.cpu().numpy(), b.cpu().numpy())
        worst, where = (e, n) if e > worst else (worst, where)
    print("chain: x %.3e, log_q %.3e, worst of %d parameter gradients %.3e at %s (bar %.0e)" % (e_x, e_q, len(names), worst, where, CHAIN_TOL))
    report("sample_logdet", case="chain_rsample", x=e_x, log_q=e_q, parameters=len(names), worst_parameter=worst)
    assert len(names) >= 20 and e_x <= CHAIN_TOL and e_q <= CHAIN_TOL and worst <= CHAIN_TOL, (e_x, e_q, worst, where)


def test_captured_sample_with_log_prob_replays_with_the_bits_of_the_eager_call(dev, monkeypatch):
    from fincflow_amd import _lib
    model = build_model(dev)
    fix_latents(model, 4, monkeypatch)
    x0, q0 = model.sample_with_log_prob(4)                           # eager first: results to compare with, caches and workspace filled
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x, q = model.sample_with_log_prob(4)
    for _ in range(2):
        x.zero_(), q.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(x, x0) and same_bits(q, q0)
    assert not _lib.fault_pending()
