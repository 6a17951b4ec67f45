"""The backwards of the per-pixel layers' reverse direction on the GPU (include/finc.h: finc_coupling_reverse_backward_f32,
finc_actnorm_reverse_backward_f32) and glow.Coupling / SplitPrior / ActNorm / Conv1x1 on HIP inside `reverse_grad()`: DESIGN 3.16.

Reference everywhere: the module formulas (layers/coupling.py:95-101, layers/actnorm.py:47-52, layers/conv1x1.py:37-43) in float64 on
the CPU, autograd for gradients.  Bar: 1e-5 in helpers.rel_err, the bar of these layers' forward-direction backward tests; the
whole-chain case compares against the same chain with the three new gates patched off (PyTorch's lines, the path before this
feature) at the chain bar of tests/test_gpu_inverse_backward.py, 5e-5.  Every case prints what it achieved and appends it to the
parity report (kind `reverse_backward`).
"""
import contextlib
import copy
import functools
import itertools

import numpy as np
import pytest
import torch

import test_gpu_actnorm as act
import test_gpu_coupling as cpl
from actnorm_cases import BIG, inputs as actnorm_inputs
from helpers import actnorm_ref, coupling_ref, offset_view, rel_err, report, same_bits
from test_gpu_bounds import F32, check_bounds, check_isolation, grads, judge_outputs, pixel_inputs, run
from test_gpu_inverse_backward import CHAIN_TOL, build_chain

pytestmark = pytest.mark.gpu

TOL = 1e-5
CPL_NAMES = ("grad_x", "grad_raw", "grad_a", "grad_b")
ACT_NAMES = ("grad_x", "grad_log_scale", "grad_translation")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# references (float64 autograd, once per shape)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coupling_case(shape):
    """(x, raw, a, b, grad_y) of tests/test_gpu_coupling.py and the float64 gradients of sum(reverse(x) * grad_y)."""
    x, raw, a, b, gy, _ = cpl.case(shape)
    leaves = [v.double().requires_grad_(True) for v in (x, raw, a, b)]
    (cpl.ref_transform(*leaves, -1) * gy.double()).sum().backward()
    return (x, raw, a, b, gy), [v.grad.numpy() for v in leaves]


def actnorm_gradients(x, ls, t, gy):
    leaves = [v.double().requires_grad_(True) for v in (x, ls, t)]
    (act.ref_transform(*leaves, -1) * gy.double()).sum().backward()
    return [v.grad.numpy() for v in leaves]


@functools.lru_cache(maxsize=None)
def actnorm_case(shape):
    """(x, log_scale, translation, grad_y) of tests/test_gpu_actnorm.py, or the cancellation case (`shape` = "cancel": the inputs of
    the actnorm_B64_C12_16x16_cancel fixture, per-channel offsets up to 1000 and deviations down to 0.01), and the float64 gradients."""
    if shape == "cancel":
        x, gy, _ = (torch.from_numpy(v) for v in actnorm_inputs(BIG))
        torch.manual_seed(12)
        ls, t = 0.3 * torch.randn(x.shape[1]), torch.randn(x.shape[1])
    else:
        x, ls, t, gy, _ = act.case(shape)
    return (x, ls, t, gy), actnorm_gradients(x, ls, t, gy)


def judge(kind, shape, names, got, ref):
    errs = {n: rel_err(g.cpu().numpy(), r) for n, g, r in zip(names, got, ref)}
    print(kind, shape, errs)
    report("reverse_backward", case=kind, shape=list(shape) if not isinstance(shape, str) else shape, **errs)
    for n, e in errs.items():
        assert e <= TOL, (kind, shape, n, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two kernels through ops
# ---------------------------------------------------------------------------------------------------------------------------------
def coupling_call(dev, shape, move):
    from fincflow_amd import ops
    (x, raw, a, b, gy), ref = coupling_case(shape)
    rawd, ad, bd = move(raw), a.to(dev), b.to(dev)
    y = ops.finc_coupling(move(x), rawd, ad, bd, -1, out=move(torch.zeros_like(x)))[0]        # the reverse's own output
    return (move(gy), y, rawd, ad, bd), ref


@pytest.mark.parametrize("shape", cpl.SHAPES)
def test_coupling_all_four_gradients_against_float64_autograd(shape, dev):
    from fincflow_amd import ops
    args, ref = coupling_call(dev, shape, lambda v: v.to(dev))
    got = ops.finc_coupling_reverse_backward(*args)
    again = ops.finc_coupling_reverse_backward(*args)
    torch.cuda.synchronize()
    judge("coupling_kernel", shape, CPL_NAMES, got, ref)
    half = shape[1] // 2
    assert torch.equal(got[0][:, :half], args[0][:, :half])         # the untouched half's gradient passes through
    for n, g, h in zip(CPL_NAMES, got, again):                      # fixed-order sums: two calls, the same bits
        assert torch.equal(g, h), n


@pytest.mark.parametrize("shape", act.SHAPES + ["cancel"], ids=str)
def test_actnorm_all_three_gradients_against_float64_autograd(shape, dev):
    from fincflow_amd import ops
    (x, ls, t, gy), ref = actnorm_case(shape)
    args = (gy.to(dev), x.to(dev), ls.to(dev))
    got = ops.finc_actnorm_reverse_backward(*args)
    again = ops.finc_actnorm_reverse_backward(*args)
    torch.cuda.synchronize()
    judge("actnorm_kernel", shape, ACT_NAMES, got, ref)
    for n, g, h in zip(ACT_NAMES, got, again):
        assert torch.equal(g, h), n


@pytest.mark.parametrize("shape", [(2, 12, 8, 8), (3, 4, 5, 3)])
def test_gradients_on_views_offset_by_one_float(shape, dev):
    """HW % 4 == 0 or not, the pointers are only 4-byte aligned: the dword form, not a refusal."""
    from fincflow_amd import ops
    args, ref = coupling_call(dev, shape, lambda v: offset_view(v, dev))
    assert all(v.data_ptr() % 16 == 4 for v in args[:3])
    judge("coupling_kernel_offset", shape, CPL_NAMES, ops.finc_coupling_reverse_backward(*args), ref)
    x, ls, t, gy, _ = act.case(shape)
    got = ops.finc_actnorm_reverse_backward(offset_view(gy, dev), offset_view(x, dev), ls.to(dev))
    judge("actnorm_kernel_offset", shape, ACT_NAMES, got, actnorm_gradients(x, ls, t, gy))


@pytest.mark.parametrize("shape", [(2, 16, 5, 3), (3, 96, 20, 24)])
def test_every_combination_of_skipped_outputs(shape, dev):
    """Straight through the C ABI: a skipped output is NULL, a buffer that was not passed is not written, and the outputs that are
    asked for have the bits of the call that asks for all of them."""
    from fincflow_amd import _lib, ops
    B, C, H, W = shape
    L = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream

    def sweep(sym, ins, full, like, nbytes):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        acts = sum(1 for f in full if f.dim() == 4)
        for want in itertools.product((False, True), repeat=len(full)):
            bufs = [torch.full_like(like, 7.0) for _ in range(acts)] + [torch.full((C,), 7.0, device=dev) for _ in range(len(full) - acts)]
            ptrs = [v.data_ptr() if w else None for v, w in zip(bufs, want)]
            rc = getattr(L, sym)(*[v.data_ptr() for v in ins], *ptrs, B, C, H * W, ws.data_ptr(), ws.numel(), st)
            torch.cuda.synchronize()
            if not any(want):
                assert rc == 1, sym
                continue
            assert rc == 0, (sym, want, rc)
            for v, w, f in zip(bufs, want, full):
                assert torch.equal(v, f) if w else bool((v == 7.0).all()), (sym, want)
        # without the per-channel sums the call needs no workspace at all
        gx = torch.empty_like(like)
        rc = getattr(L, sym)(*[v.data_ptr() for v in ins], gx.data_ptr(), *[None] * (len(full) - 1), B, C, H * W, None, 0, st)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(gx, full[0]), sym

    args, _ = coupling_call(dev, shape, lambda v: v.to(dev))
    sweep("finc_coupling_reverse_backward_f32", args, ops.finc_coupling_reverse_backward(*args), args[0],
          L.finc_coupling_workspace_bytes(B, C, H * W))
    x, ls, t, gy, _ = act.case(shape)
    args = (gy.to(dev), x.to(dev), ls.to(dev))
    sweep("finc_actnorm_reverse_backward_f32", args, ops.finc_actnorm_reverse_backward(*args), args[0],
          L.finc_actnorm_workspace_bytes(B, C, H * W))


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
    b1, c0 = B // 2, C - 1 if C < 3 else C // 2 + 1
    image, chan = (b1,), (slice(None), c0)
    if op == "coupling_reverse_backward":
        y32 = coupling_ref(T["x"], T["raw"], T["a"], T["b"], -1)[0].contiguous()        # the reverse's output, as the kernel is handed it
        sym, ws = "finc_coupling_reverse_backward_f32", L.finc_coupling_workspace_bytes(B, C, HW)
        ins, acts = dict(gy=D["gy"], y=y32.to(dev), raw=D["raw"], a=D["a"], b=D["b"]), ("gy", "y", "raw", "gx", "graw")
        outs = dict(gx=(shape, F32), graw=(shape, F32), ga=((C,), F32), gb=((C,), F32))
        argf = lambda p, w, n: (p["gy"], p["y"], p["raw"], p["a"], p["b"], p["gx"], p["graw"], p["ga"], p["gb"], B, C, HW, w, n, None)
        g = grads(lambda x, raw, a, b: (coupling_ref(x, raw, a, b, -1)[0],), [T["x"], T["raw"], T["a"], T["b"]], [T["gy"]])
        refs, alias = dict(zip(("gx", "graw", "ga", "gb"), g)), None
        j = half // 2
        pair = (slice(None), slice(2 * j, 2 * j + 2))
        spots = [("raw", image, dict(gx=image, graw=image)), ("y", image, dict(gx=None, graw=image)),
                 ("raw", pair, dict(ga=pair[1], gb=pair[1], gx=(slice(None), half + j), graw=pair))]
    else:
        sym, ws = "finc_actnorm_reverse_backward_f32", L.finc_actnorm_workspace_bytes(B, C, HW)
        ins, acts = dict(gy=D["gy"], x=D["x"], ls=D["ls"]), ("gy", "x", "gx")
        outs = dict(gx=(shape, F32), gls=((C,), F32), gt=((C,), F32))
        argf = lambda p, w, n: (p["gy"], p["x"], p["ls"], p["gx"], p["gls"], p["gt"], B, C, HW, w, n, None)
        g = grads(lambda x, ls, tr: (actnorm_ref(x, ls, tr, -1)[0],), [T["x"], T["ls"], T["tr"]], [T["gy"]])
        refs, alias = dict(zip(("gx", "gls", "gt"), g)), dict(gx="gy")
        spots = [("x", chan, dict(gx=None, gls=(c0,), gt=None)), ("gy", chan, dict(gx=chan, gls=(c0,), gt=(c0,)))]
    return dict(sym=sym, ins=ins, outs=outs, ws=ws, argf=argf, acts=acts, alias=alias, refs=refs, spots=spots)


@pytest.mark.parametrize("shape", [(3, 12, 8, 8), (3, 4, 5, 3), (5, 6, 9, 8)], ids=str)
@pytest.mark.parametrize("op", ["coupling_reverse_backward", "actnorm_reverse_backward"])
def test_guard_bands_and_problem_isolation(op, shape, dev):
    """As tests/test_gpu_bounds.py::test_per_pixel_layer: the 16-byte form and, one float into every activation's allocation, the
    dword form, each between NaN guards with an exactly-sized NaN workspace; the in-place form the ABI allows (ActNorm: grad_x over
    grad_y); a NaN / +inf in one image, channel or channel pair reaching only what the operation's definition lets it reach."""
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
class Counter:
    """Counts the calls of the new entry points of fincflow_amd.ops and of the mix's (patched in place, restored by monkeypatch), and
    keeps the keyword arguments of the last call of each."""
    NAMES = ("coupling_reverse", "finc_coupling_reverse_backward", "actnorm_reverse", "finc_actnorm_reverse_backward", "mix_forward",
             "finc_mix_backward")

    def __init__(self, monkeypatch):
        from fincflow_amd import ops
        self.n, self.kwargs = dict.fromkeys(self.NAMES, 0), {}
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def counted(*args, **kwargs):
            self.n[name] += 1
            self.kwargs[name] = kwargs
            return fn(*args, **kwargs)
        return counted

    def take(self):
        n, self.n = self.n, dict.fromkeys(self.NAMES, 0)
        return {k: v for k, v in n.items() if v}


def gates_off(monkeypatch):
    """The three new gates answer False: `reverse` under autograd keeps its PyTorch lines, as before this feature."""
    from fincflow_amd import glow
    for cls in (glow.Coupling, glow.ActNorm, glow.Conv1x1):
        monkeypatch.setattr(cls, "_hip_reverse_grad", lambda self, *a, **k: False)


def make(kind, C, hw):
    """(module, context channels).  Parameters filled as tests/test_gpu_coupling.py does; ActNorm's by hand; Conv1x1 keeps its
    orthogonal W."""
    from fincflow_amd import glow
    torch.manual_seed(11)
    np.random.seed(11)
    if kind == "actnorm":
        m = glow.ActNorm(C)
        with torch.no_grad():
            m.log_scale.copy_(0.3 * torch.randn(C))
            m.translation.copy_(torch.randn(C))
        m.mark_initialized()
        return m, None
    if kind == "conv1x1":
        return glow.Conv1x1(C), None
    if kind == "split":
        return cpl.fill(glow.SplitPrior((C,) + hw, glow.GaussianPrior, width=32)).transform, None
    n_context = 5 if kind == "coupling_context" else None
    return cpl.fill(glow.Coupling((C,) + hw, width=32, n_context=n_context)), n_context


EXPECT = {"coupling": ("_FincCouplingReverseFunctionBackward", dict(coupling_reverse=1), dict(finc_coupling_reverse_backward=1)),
          "actnorm": ("_FincActNormReverseFunctionBackward", dict(actnorm_reverse=1), dict(finc_actnorm_reverse_backward=1)),
          "conv1x1": ("_FincMixFunctionBackward", dict(mix_forward=1), dict(finc_mix_backward=1))}
MODULE_CASES = [(k, C, s) for s in ((4, 6, 6), (3, 5, 3)) for k, C in (("coupling", 12), ("coupling_context", 12), ("split", 12),
                                                                     ("actnorm", 12), ("conv1x1", 12), ("conv1x1", 48))]


def reverse_run(m, x, ctx, g, inside=True):
    """reverse + backward of sum(y * g): (y, the node's name, [grad_x, (grad_context,) every parameter's gradient])."""
    import fincflow_amd
    m.zero_grad()
    xa = x.clone().requires_grad_(True)
    ca = None if ctx is None else ctx.clone().requires_grad_(True)
    with (fincflow_amd.reverse_grad() if inside else contextlib.nullcontext()):
        y = m.reverse(xa, ca)
    (y * g).sum().backward()
    out = [xa.grad] + ([] if ca is None else [ca.grad]) + [p.grad for p in m.parameters()]
    assert all(v is not None for v in out)
    return y.detach(), type(y.grad_fn).__name__, [v.clone() for v in out]


@pytest.mark.parametrize("kind,C,bhw", MODULE_CASES, ids=str)
def test_modules_inside_reverse_grad_against_the_float64_module(kind, C, bhw, dev, monkeypatch):
    B, hw = bhw[0], bhw[1:]
    m, n_context = make(kind, C, hw)
    m64, md = copy.deepcopy(m).double(), copy.deepcopy(m).to(dev)
    torch.manual_seed(C + sum(bhw))
    x, g = torch.randn(B, C, *hw), torch.randn(B, C, *hw)
    ctx = None if n_context is None else torch.randn(B, n_context, *hw)
    to = lambda v, f: None if v is None else f(v)
    counter = Counter(monkeypatch)
    family = "coupling" if kind in ("coupling_context", "split") else kind
    node_want, fwd_want, bwd_want = EXPECT[family]

    import fincflow_amd
    md.zero_grad()
    xa = x.to(dev).requires_grad_(True)
    ca = to(ctx, lambda v: v.to(dev).requires_grad_(True))
    with fincflow_amd.reverse_grad():
        y = md.reverse(xa, ca)
    assert type(y.grad_fn).__name__ == node_want and counter.take() == fwd_want
    (y * g.to(dev)).sum().backward()
    assert counter.take() == bwd_want
    got = [y.detach(), xa.grad] + ([] if ca is None else [ca.grad]) + [p.grad for p in md.parameters()]
    y64, _, ref = reverse_run(m64, x.double(), to(ctx, lambda v: v.double()), g.double(), inside=False)
    names = ["result", "grad_input"] + ([] if ctx is None else ["grad_context"]) + ["grad_" + n for n, _ in md.named_parameters()]
    assert len(got) == len(names) == len(ref) + 1 and all(v is not None for v in got)
    judge("module_" + kind, (B, C) + hw, names, got, [y64.numpy()] + [r.numpy() for r in ref])

    # frozen parameters: only what the input's gradient needs is computed (the coupling's raw carries the net's share of it)
    md.requires_grad_(False)
    md.zero_grad()
    with fincflow_amd.reverse_grad():
        y = md.reverse(xa, to(ctx, lambda v: v.to(dev)))
    assert type(y.grad_fn).__name__ == node_want and counter.take() == fwd_want
    xa.grad = None
    (y * g.to(dev)).sum().backward()
    assert counter.take() == bwd_want
    kw = counter.kwargs[next(iter(bwd_want))]
    want_kw = {"coupling": dict(need_gx=True, need_graw=True, need_ga=False, need_gb=False),
               "actnorm": dict(need_gx=True, need_gls=False, need_gt=False), "conv1x1": dict(need_gx=True, need_gm=False, need_gb=False)}[family]
    assert kw == want_kw, kw
    assert all(p.grad is None for p in md.parameters())
    assert rel_err(xa.grad.cpu().numpy(), ref[0].numpy()) <= TOL


def test_split_prior_reverse_takes_the_new_path(dev, monkeypatch):
    import fincflow_amd
    from fincflow_amd import glow
    m = cpl.fill(glow.SplitPrior((12, 6, 6), glow.GaussianPrior, width=32)).to(dev)
    counter = Counter(monkeypatch)
    with fincflow_amd.reverse_grad():
        y = m.reverse(torch.randn(2, 6, 6, 6, device=dev))
    assert type(y.grad_fn).__name__ == "_FincCouplingReverseFunctionBackward" and counter.take() == dict(coupling_reverse=1)
    y.square().mean().backward()
    assert counter.take() == dict(finc_coupling_reverse_backward=1)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def recorded_nodes(y):
    """The autograd nodes behind `y`, by class name, in the order a walk from y.grad_fn meets them."""
    names, todo, seen = [], [y.grad_fn], set()
    while todo:
        fn = todo.pop(0)
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo += [nxt for nxt, _ in fn.next_functions]
    return names


@pytest.mark.parametrize("kind,C", [("coupling", 12), ("coupling_context", 12), ("split", 12), ("actnorm", 12), ("conv1x1", 12)])
def test_outside_the_context_nothing_changed(kind, C, dev, monkeypatch):
    """`reverse` under autograd outside `reverse_grad()`: no new Function, no call of a new entry point, the same recorded graph, and
    result and gradients with the bits of the same call with the gates patched off.  PyTorch's own convolution backward (MIOpen) is
    not bit-reproducible from call to call on every shape, and a gradient that differs only now and then (the coupling net's middle
    weight) can agree between two calls and differ in a third.  So every leg is run RUNS times: a gradient that PyTorch reproduces
    bit for bit in every run of both legs of a comparison must be bit-equal between them, the others are named in the output and
    held to the float64 bar against each other."""
    import fincflow_amd
    RUNS = 4
    m, n_context = make(kind, C, (6, 6))
    md = m.to(dev)
    torch.manual_seed(7)
    x, g = torch.randn(4, C, 6, 6, device=dev), torch.randn(4, C, 6, 6, device=dev)
    ctx = None if n_context is None else torch.randn(4, n_context, 6, 6, device=dev)
    counter = Counter(monkeypatch)

    def leg(inside):
        """RUNS calls: (y, node) of the first -- every call's y and node must equal them --, its gradients, and per gradient whether
        every call gave the same bits."""
        runs = [reverse_run(md, x, ctx, g, inside=inside) for _ in range(RUNS)]
        assert all(r[1] == runs[0][1] and same_bits(r[0], runs[0][0]) for r in runs)
        return runs[0][0], runs[0][1], runs[0][2], [all(same_bits(r[2][i], runs[0][2][i]) for r in runs) for i in range(len(runs[0][2]))]

    reverse_run(md, x, ctx, g, inside=False)                 # (the first call of a shape is where MIOpen picks its kernels)
    y, node, got, got_stable = leg(False)
    graph = recorded_nodes(md.reverse(x.clone().requires_grad_(True), ctx))
    assert "Finc" not in node and not any("Finc" in n for n in graph) and counter.take() == {}, graph
    gates_off(monkeypatch)
    y0, node0, want, want_stable = leg(False)
    assert node == node0 and graph == recorded_nodes(md.reverse(x.clone().requires_grad_(True), ctx)) and same_bits(y, y0)
    names = ["grad_input"] + ([] if ctx is None else ["grad_context"]) + ["grad_" + n for n, _ in md.named_parameters()]
    stable = [a and b for a, b in zip(got_stable, want_stable)]
    print(kind, "gradients PyTorch does not reproduce between its own %d calls:" % RUNS, [n for n, ok in zip(names, want_stable) if not ok],
          "; between the calls with the gates as they are:", [n for n, ok in zip(names, got_stable) if not ok])
    report("reverse_backward", case="outside_" + kind, gradients=len(names), reproducible_in_pytorch=sum(stable), runs=RUNS)
    for n, ok, a, b in zip(names, stable, got, want):
        assert same_bits(a, b) if ok else rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL, (kind, n, ok)
    # and with the gates off the context changes nothing either: they are the only switch
    with fincflow_amd.reverse_grad():
        assert recorded_nodes(md.reverse(x.clone().requires_grad_(True), ctx)) == graph
    y1, node1, inside, inside_stable = leg(True)
    assert node1 == node0 and same_bits(y1, y0) and counter.take() == {}
    for n, ok, ok_in, a, b in zip(names, want_stable, inside_stable, inside, want):
        assert same_bits(a, b) if ok and ok_in else rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL, (kind, n, ok, ok_in)


def test_what_keeps_the_pytorch_lines_inside_the_context(dev, monkeypatch):
    """float64 on the device, an odd channel count, a 2-D ActNorm input and a channel count without a mix kernel: inside
    `reverse_grad()` they record PyTorch's nodes and raise nothing new."""
    import fincflow_amd
    from fincflow_amd import glow, ops
    counter = Counter(monkeypatch)
    torch.manual_seed(8)
    with fincflow_amd.reverse_grad():
        for kind in ("coupling", "actnorm", "conv1x1"):
            m64 = make(kind, 12, (6, 6))[0].double().to(dev)
            x = torch.randn(2, 12, 6, 6, device=dev, dtype=torch.float64, requires_grad=True)
            y = m64.reverse(x)
            assert y.requires_grad and "Finc" not in type(y.grad_fn).__name__, kind
            y.sum().backward()
            assert x.grad is not None
        odd = make("coupling", 7, (6, 6))[0].to(dev)
        with pytest.raises(RuntimeError):           # (the PyTorch formula itself cannot split seven channels: layers/coupling.py:79)
            odd.reverse(torch.randn(2, 7, 6, 6, device=dev, requires_grad=True))
        odd_act = make("actnorm", 7, (6, 6))[0].to(dev)               # ActNorm's kernels take any channel count ...
        flat = odd_act.reverse(torch.randn(5, 7, device=dev, requires_grad=True))       # ... but 4-D activations only
        assert "Finc" not in type(flat.grad_fn).__name__
        assert counter.take() == {}
        mix = make("conv1x1", 12, (6, 6))[0].to(dev)
        monkeypatch.setattr(ops, "mix_supported", lambda C: False)
        y = mix.reverse(torch.randn(2, 12, 6, 6, device=dev, requires_grad=True))
        assert "Finc" not in type(y.grad_fn).__name__ and counter.take() == {}
        y.sum().backward()
        assert mix.W.grad is not None


@pytest.mark.parametrize("kind", ["coupling", "actnorm", "conv1x1"])
def test_each_function_saves_one_activation(kind, dev, monkeypatch):
    """Inside the context a layer's recorded reverse holds exactly one activation-sized tensor beyond the coupling's `raw`: the
    coupling its OUTPUT, ActNorm and the mix their INPUT.  PyTorch's count on the same call is reported beside it."""
    import fincflow_amd
    m = make(kind, 12, (8, 8))[0].to(dev)
    torch.manual_seed(9)
    x = torch.randn(8, 12, 8, 8, device=dev)
    n = x.numel()
    storage = lambda v: v.untyped_storage().data_ptr()

    def saved():
        kept = []
        xa = x.clone().requires_grad_(True)
        with fincflow_amd.reverse_grad(), torch.autograd.graph.saved_tensors_hooks(lambda v: kept.append(v) or v, lambda v: v):
            y = m.reverse(xa)
        return xa, y, [v for v in kept if v.numel() == n]
    xa, y, big = saved()
    if kind == "coupling":
        beyond = [v for v in big if storage(v) == storage(y)]       # the other one is `raw`: it is neither the output nor the input
        assert len(big) == 2 and len(beyond) == 1 and all(storage(v) != storage(xa) for v in big)
    else:
        beyond = big
        assert len(big) == 1 and storage(big[0]) == storage(xa)
    gates_off(monkeypatch)
    _, _, big_torch = saved()
    report("reverse_backward", case="saved_activations", layer=kind, hip=len(beyond), pytorch=len(big_torch))
    print(kind, "activation-sized tensors saved: HIP", len(beyond), "beyond raw; PyTorch", len(big_torch))
    assert len(big_torch) >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole chain
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_whole_chain_against_the_same_chain_with_the_gates_off(dev, monkeypatch):
    import fincflow_amd
    model = build_chain(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    torch.manual_seed(2)
    z0 = torch.randn(4, 48, 4, 4, device=dev)
    g = torch.randn(4, 3, 16, 16, device=dev)
    counter = Counter(monkeypatch)

    def chain_grads():
        z = z0.clone().requires_grad_(True)
        with fincflow_amd.reverse_grad():
            x = model._reverse_chain(z, None)
        assert x.requires_grad and x.shape == g.shape
        return x.detach(), torch.autograd.grad(x, [z] + params, g)
    x_on, on = chain_grads()
    steps = 4                                           # 2 blocks x 2 steps: one ActNorm, Conv1x1 and Coupling each
    assert counter.take() == dict(coupling_reverse=steps, finc_coupling_reverse_backward=steps, actnorm_reverse=steps,
                                  finc_actnorm_reverse_backward=steps, mix_forward=steps, finc_mix_backward=steps)
    gates_off(monkeypatch)
    x_off, off = chain_grads()
    assert counter.take() == {}
    e_x = rel_err(x_on.cpu().numpy(), x_off.cpu().numpy())
    e_z = rel_err(on[0].cpu().numpy(), off[0].cpu().numpy())
    worst, n = 0.0, 0
    for a, b in zip(on[1:], off[1:]):
        assert float(b.abs().max()) > 0
        worst = max(worst, rel_err(a.cpu().numpy(), b.cpu().numpy()))
        n += 1
    print("whole chain: x %.3e, grad_z %.3e, worst of %d parameter gradients %.3e (bar %.0e)" % (e_x, e_z, n, worst, CHAIN_TOL))
    report("reverse_backward", case="whole_chain", x=e_x, grad_z=e_z, parameters=n, worst_parameter=worst)
    assert n == len(params) >= 20 and e_x <= CHAIN_TOL and e_z <= CHAIN_TOL and worst <= CHAIN_TOL, (e_x, e_z, worst)


def test_rsample_backward_reaches_every_parameter_on_the_new_path(dev, monkeypatch):
    from fincflow_amd import _lib
    model = build_chain(dev)
    counter = Counter(monkeypatch)
    x = model.rsample(4)
    assert x.requires_grad and counter.take() == dict(coupling_reverse=4, actnorm_reverse=4, mix_forward=4)
    x.square().mean().backward()
    assert counter.take() == dict(finc_coupling_reverse_backward=4, finc_actnorm_reverse_backward=4, finc_mix_backward=4)
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    _lib.raise_if_faulted("test_rsample_backward_reaches_every_parameter_on_the_new_path")
