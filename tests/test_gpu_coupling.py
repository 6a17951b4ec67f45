"""The affine coupling on its HIP kernels (finc_coupling_f32, finc_coupling_backward_f32, finc_bias_relu_f32) and glow.Coupling /
SplitPrior on them.

Reference everywhere: the formulas of include/finc.h (layers/coupling.py:79-101) in float64 on the CPU, autograd for gradients.
Bar: 1e-5 in helpers.rel_err, the project's bar for every fp32-against-fp64 parity and backward test.  PyTorch's own fp32
evaluation of these formulas on these inputs is within 1.5e-7 (outputs, log-det) and 6.8e-7 (gradients) of float64, so the bar leaves
more than a factor of ten.  Every case appends its achieved errors to the parity report (helpers.report).
"""
import copy
import itertools

import pytest
import torch

from helpers import offset_view, rel_err, report

pytestmark = pytest.mark.gpu

TOL = 1e-5

SHAPES = [(128, 12, 16, 16), (128, 24, 8, 8), (128, 48, 4, 4), (3, 96, 20, 24), (2, 4, 7, 7), (5, 2, 1, 1), (8, 96, 32, 32), (2, 192, 9, 8),
          (16, 12, 64, 64), (2, 16, 5, 3)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def case(shape):
    """x, raw, a, b, grad_y, grad_logdet (fp32, CPU).  a = exp(3 logs), b = bias * a are rounded to fp32 once: they are the kernel's
    inputs, and the reference starts from the same numbers."""
    B, C, H, W = shape
    torch.manual_seed(sum(shape))
    x = torch.randn(B, C, H, W)
    gy = torch.randn(B, C, H, W)
    gl = torch.randn(B)
    raw = 1.5 * torch.randn(B, C, H, W)
    logs = 0.1 * torch.randn(C)
    bias = 0.3 * torch.randn(C)
    a = torch.exp(3.0 * logs.double())
    return x, raw, a.float(), (bias.double() * a).float(), gy, gl


def ref_transform(x, raw, a, b, direction):
    """float64: (y, logdet) of the forward direction, y of the reverse."""
    half = x.shape[1] // 2
    h = a.view(1, -1, 1, 1) * raw + b.view(1, -1, 1, 1)
    s = 2.0 * torch.tanh(h[:, ::2] / 2.0)
    t = h[:, 1::2]
    x1, x2 = x[:, :half], x[:, half:]
    if direction > 0:
        return torch.cat([x1, x2 * torch.exp(s) + t], dim=1), s.flatten(start_dim=1).sum(-1)
    return torch.cat([x1, (x2 - t) * torch.exp(-s)], dim=1)


def ref_gradients(x, raw, a, b, gy, gl):
    """float64 autograd of sum(y * gy) + sum(logdet * gl) with respect to x, raw, a, b."""
    leaves = [t.double().requires_grad_(True) for t in (x, raw, a, b)]
    y, ld = ref_transform(*leaves, 1)
    loss = (y * gy.double()).sum()
    if gl is not None:
        loss = loss + (ld * gl.double()).sum()
    loss.backward()
    return [t.grad.numpy() for t in leaves]


def check_transform(shape, dev, move, kind):
    from fincflow_amd import ops
    x, raw, a, b, _, _ = case(shape)
    y_ref, ld_ref = ref_transform(x.double(), raw.double(), a.double(), b.double(), 1)
    r_ref = ref_transform(x.double(), raw.double(), a.double(), b.double(), -1)
    xd, rawd, ad, bd = move(x), move(raw), a.to(dev), b.to(dev)
    y, ld = ops.finc_coupling(xd, rawd, ad, bd, 1, True, out=move(torch.zeros_like(x)))
    y_plain, none = ops.finc_coupling(xd, rawd, ad, bd, 1, False)
    r, none2 = ops.finc_coupling(xd, rawd, ad, bd, -1, True, out=move(torch.zeros_like(x)))
    back, _ = ops.finc_coupling(y, rawd, ad, bd, -1, False)
    torch.cuda.synchronize()
    assert none is None and none2 is None and ld.shape == (shape[0],)
    assert torch.equal(y, y_plain)                                   # the log-det is a by-product: the same y without it
    half = shape[1] // 2
    assert torch.equal(y[:, :half].cpu(), x[:, :half]) and torch.equal(r[:, :half].cpu(), x[:, :half])
    errs = {"forward": rel_err(y.cpu().numpy(), y_ref.numpy()), "logdet": rel_err(ld.cpu().numpy(), ld_ref.numpy()),
            "reverse": rel_err(r.cpu().numpy(), r_ref.numpy()), "round_trip": rel_err(back.cpu().numpy(), x.double().numpy())}
    print(kind, shape, errs)
    report(kind, shape=list(shape), **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)


@pytest.mark.parametrize("shape", SHAPES)
def test_transform_forward_logdet_reverse_and_round_trip(shape, dev):
    check_transform(shape, dev, lambda t: t.to(dev), "coupling_transform")


@pytest.mark.parametrize("shape", [(2, 12, 8, 8), (3, 4, 5, 3)])
def test_transform_on_views_offset_by_one_float(shape, dev):
    """HW % 4 == 0 but the pointers are only 4-byte aligned: the dword form, not a refusal."""
    check_transform(shape, dev, lambda t: offset_view(t, dev), "coupling_transform_offset")


def test_transform_in_place(dev):
    from fincflow_amd import ops
    x, raw, a, b, _, _ = case((3, 96, 20, 24))
    xd, rawd, ad, bd = x.to(dev), raw.to(dev), a.to(dev), b.to(dev)
    for direction in (1, -1):
        want, _ = ops.finc_coupling(xd, rawd, ad, bd, direction, False)
        buf = xd.clone()
        got, _ = ops.finc_coupling(buf, rawd, ad, bd, direction, False, out=buf)
        assert got is buf and torch.equal(got, want)


def test_reverse_ignores_a_logdet_pointer_and_needs_no_workspace(dev):
    """include/finc.h: finc_coupling_f32 ignores `logdet` in direction -1 (finc_coupling_reverse_logdet_f32 is the entry point that
    sums there).  A log-det buffer handed in all the same keeps its bits, and the call succeeds without a workspace."""
    from fincflow_amd import ops
    shape = (2, 4, 4, 4)
    x, raw, a, b, _, _ = case(shape)
    xd, rawd, ad, bd = x.to(dev), raw.to(dev), a.to(dev), b.to(dev)
    want, _ = ops.finc_coupling(xd, rawd, ad, bd, -1, False)
    y, logdet = torch.zeros_like(xd), torch.full((shape[0],), -12345.5, device=dev)
    status = ops._lib.lib().finc_coupling_f32(xd.data_ptr(), rawd.data_ptr(), ad.data_ptr(), bd.data_ptr(), y.data_ptr(), logdet.data_ptr(),
                                              shape[0], shape[1], shape[2] * shape[3], -1, None, 0,
                                              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert status == 0                                               # FINC_OK
    assert torch.equal(logdet.cpu(), torch.full((shape[0],), -12345.5))
    assert torch.equal(y, want)


@pytest.mark.parametrize("with_logdet", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_all_four_gradients_against_float64_autograd(shape, with_logdet, dev):
    from fincflow_amd import ops
    x, raw, a, b, gy, gl = case(shape)
    if not with_logdet:
        gl = None
    ref = ref_gradients(x, raw, a, b, gy, gl)
    args = (gy.to(dev), None if gl is None else gl.to(dev), x.to(dev), raw.to(dev), a.to(dev), b.to(dev))
    got = ops.finc_coupling_backward(*args)
    again = ops.finc_coupling_backward(*args)
    torch.cuda.synchronize()
    names = ("grad_x", "grad_raw", "grad_a", "grad_b")
    errs = {n: rel_err(g.cpu().numpy(), r) for n, g, r in zip(names, got, ref)}
    print(shape, with_logdet, errs)
    report("coupling_backward", shape=list(shape), with_logdet=with_logdet, **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)
    for n, g, h in zip(names, got, again):                          # fixed-order sums: two calls, the same bits
        assert torch.equal(g, h), n


def test_gradients_on_views_offset_by_one_float(dev):
    from fincflow_amd import ops
    shape = (2, 12, 8, 8)
    x, raw, a, b, gy, gl = case(shape)
    ref = ref_gradients(x, raw, a, b, gy, gl)
    got = ops.finc_coupling_backward(offset_view(gy, dev), gl.to(dev), offset_view(x, dev), offset_view(raw, dev), a.to(dev), b.to(dev))
    errs = {n: rel_err(g.cpu().numpy(), r) for n, g, r in zip(("grad_x", "grad_raw", "grad_a", "grad_b"), got, ref)}
    report("coupling_backward_offset", shape=list(shape), **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)


@pytest.mark.parametrize("shape", [(3, 96, 20, 24), (2, 16, 5, 3), (128, 24, 8, 8)])
def test_every_combination_of_skipped_outputs(shape, dev):
    """Straight through the C ABI: a skipped output is NULL, a buffer that was not passed is not written, and the outputs that are
    asked for have the bits of the call that asks for all four."""
    from fincflow_amd import _lib, ops
    B, C, H, W = shape
    x, raw, a, b, gy, gl = case(shape)
    xd, rawd, ad, bd, gyd, gld = (t.to(dev) for t in (x, raw, a, b, gy, gl))
    L = _lib.lib()
    ws = torch.empty(L.finc_coupling_workspace_bytes(B, C, H * W), dtype=torch.uint8, device=dev)
    full = ops.finc_coupling_backward(gyd, gld, xd, rawd, ad, bd)
    st = torch.cuda.current_stream(dev).cuda_stream
    for want in itertools.product((False, True), repeat=4):
        bufs = [torch.full_like(xd, 7.0), torch.full_like(xd, 7.0), torch.full((C,), 7.0, device=dev), torch.full((C,), 7.0, device=dev)]
        ptrs = [t.data_ptr() if w else None for t, w in zip(bufs, want)]
        rc = L.finc_coupling_backward_f32(gyd.data_ptr(), gld.data_ptr(), xd.data_ptr(), rawd.data_ptr(), ad.data_ptr(), bd.data_ptr(),
                                          *ptrs, B, C, H * W, ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        if not any(want):
            assert rc == 1
            continue
        assert rc == 0, (want, rc)
        for t, w, f in zip(bufs, want, full):
            if w:
                assert torch.equal(t, f), want
            else:
                assert bool((t == 7.0).all()), want
    # without grad_a and grad_b the call needs no workspace at all
    gx = torch.empty_like(xd)
    rc = L.finc_coupling_backward_f32(gyd.data_ptr(), gld.data_ptr(), xd.data_ptr(), rawd.data_ptr(), ad.data_ptr(), bd.data_ptr(),
                                      gx.data_ptr(), None, None, None, B, C, H * W, None, 0, st)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(gx, full[0])


def test_autograd_function_computes_only_what_is_needed(dev):
    from fincflow_amd import ops
    shape = (3, 12, 6, 10)
    x, raw, a, b, gy, gl = case(shape)
    ref = ref_gradients(x, raw, a, b, gy, gl)
    for mask in ((True, True, True, True), (True, False, False, False), (False, True, True, True), (False, False, True, False)):
        leaves = [t.to(dev).requires_grad_(m) for t, m in zip((x, raw, a, b), mask)]
        y, ld = ops.coupling_forward(*leaves)
        ((y * gy.to(dev)).sum() + (ld * gl.to(dev)).sum()).backward()
        for t, m, r in zip(leaves, mask, ref):
            if m:
                assert rel_err(t.grad.cpu().numpy(), r) <= TOL, mask
            else:
                assert t.grad is None
    # a loss that uses the output alone: grad_logdet arrives as zeros
    leaves = [t.to(dev).requires_grad_(True) for t in (x, raw, a, b)]
    y, _ = ops.coupling_forward(*leaves)
    (y * gy.to(dev)).sum().backward()
    for t, r in zip(leaves, ref_gradients(x, raw, a, b, gy, None)):
        assert rel_err(t.grad.cpu().numpy(), r) <= TOL


@pytest.mark.parametrize("shape", [(4, 512, 16, 16), (2, 32, 7, 7), (3, 5, 5, 3), (1, 16, 1, 1), (128, 64, 4, 4), (2, 6, 9, 8)])
def test_bias_relu_is_torch_relu_bit_for_bit(shape, dev):
    from fincflow_amd import ops
    torch.manual_seed(sum(shape))
    x = torch.randn(shape)
    bias = 0.3 * torch.randn(shape[1])
    want_cpu = torch.relu(x + bias.view(1, -1, 1, 1))
    for move, tag in ((lambda t: t.to(dev), "aligned"), (lambda t: offset_view(t, dev), "offset")):
        xd, bd = move(x), bias.to(dev)
        want = torch.relu(xd + bd.view(1, -1, 1, 1))
        out = ops.finc_bias_relu(xd, bd)
        assert torch.equal(xd.cpu(), x), tag                        # out of place: the input is untouched
        assert torch.equal(out, want) and torch.equal(out.cpu(), want_cpu), tag
        got = ops.finc_bias_relu(xd, bd, out=xd)                    # in place
        assert got is xd and torch.equal(xd, want), tag
    assert bool((want_cpu == 0).any()) and bool((want_cpu > 0).any())


# ---------------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------------
def fill(m, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            scale = 0.1 if name.endswith(("bias", "logs")) else 0.05
            p.copy_(torch.randn(p.shape, generator=g) * scale)
    return m


class Counter:
    """Counts the calls of the HIP entry points of fincflow_amd.ops (patched in place, restored by monkeypatch)."""
    NAMES = ("finc_coupling", "finc_coupling_backward", "coupling_forward", "finc_bias_relu")

    def __init__(self, monkeypatch):
        from fincflow_amd import ops
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def counted(*args, **kwargs):
            self.n[name] += 1
            return fn(*args, **kwargs)
        return counted

    def take(self):
        n, self.n = self.n, dict.fromkeys(self.NAMES, 0)
        return n


def make_module(kind, size, n_context):
    from fincflow_amd import glow
    if kind == "split":
        m = glow.SplitPrior(size, glow.GaussianPrior, width=32)
    else:
        m = glow.Coupling(size, width=32, n_context=n_context)
    return fill(m)


MODULES = [("coupling", (12, 8, 8), None, 4), ("coupling", (24, 5, 3), None, 3), ("coupling", (12, 8, 8), 5, 4), ("coupling", (48, 4, 4), None, 16),
           ("split", (12, 8, 8), None, 4)]


@pytest.mark.parametrize("kind,size,n_context,B", MODULES)
def test_module_forward_reverse_and_every_gradient_against_float64(kind, size, n_context, B, dev, monkeypatch):
    m = make_module(kind, size, n_context)
    m64 = copy.deepcopy(m).double()
    md = copy.deepcopy(m).to(dev)
    cpl = md.transform if kind == "split" else md
    torch.manual_seed(sum(size) + B)
    x = torch.randn(B, *size)
    ctx = None if n_context is None else torch.randn(B, n_context, *size[1:])
    ctx64 = None if ctx is None else ctx.double()
    ctxd = None if ctx is None else ctx.to(dev)
    counter = Counter(monkeypatch)
    errs = {}

    # inference: forward and reverse
    with torch.no_grad():
        assert cpl._hip(x.to(dev), ctxd)
        y, ld = md(x.to(dev), ctxd)
        y64, ld64 = m64(x.double(), ctx64)
        assert counter.take() == {"finc_coupling": 1, "finc_coupling_backward": 0, "coupling_forward": 0, "finc_bias_relu": 2}
        errs["forward"] = rel_err(y.cpu().numpy(), y64.numpy())
        errs["logdet"] = rel_err(ld.cpu().numpy(), ld64.numpy())
        if kind == "split":
            z = torch.randn(B, size[0] // 2, *size[1:])
            torch.manual_seed(5)
            r = md.reverse(z.to(dev))
            torch.manual_seed(5)
            x2, _ = md.base.sample(B)                                # the same draw on the same device
            r64 = m64.transform.reverse(torch.cat([z, x2.cpu()], dim=1).double())
        else:
            r = md.reverse(x.to(dev), ctxd)
            r64 = m64.reverse(x.double(), ctx64)
        assert counter.take() == {"finc_coupling": 1, "finc_coupling_backward": 0, "coupling_forward": 0, "finc_bias_relu": 2}
        errs["reverse"] = rel_err(r.cpu().numpy(), r64.numpy())

    # training: a loss that uses the output and the log-det
    gy = torch.randn(y64.shape)
    gl = torch.randn(B)
    xd = x.to(dev).requires_grad_(True)
    assert cpl._hip_train(xd, ctxd) and not cpl._hip(xd, ctxd)
    yt, ldt = md(xd, ctxd)
    ((yt * gy.to(dev)).sum() + (ldt * gl.to(dev)).sum()).backward()
    # (coupling_forward runs finc_coupling inside: one call of each)
    assert counter.take() == {"finc_coupling": 1, "finc_coupling_backward": 1, "coupling_forward": 1, "finc_bias_relu": 0}
    x64 = x.double().requires_grad_(True)
    y64, ld64 = m64(x64, ctx64)
    ((y64 * gy.double()).sum() + (ld64 * gl.double()).sum()).backward()
    errs["train_forward"] = rel_err(yt.detach().cpu().numpy(), y64.detach().numpy())
    errs["train_logdet"] = rel_err(ldt.detach().cpu().numpy(), ld64.detach().numpy())
    errs["grad_input"] = rel_err(xd.grad.cpu().numpy(), x64.grad.numpy())
    names = [n for n, _ in md.named_parameters()]
    assert [n.split("net.")[-1] for n in names] == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "4.logs"]
    for (n, p), (_, p64) in zip(md.named_parameters(), m64.named_parameters()):
        assert p.grad is not None, n
        errs["grad_" + n] = rel_err(p.grad.cpu().numpy(), p64.grad.numpy())
    print(kind, size, n_context, errs)
    report("coupling_module", module=kind, size=list(size), n_context=n_context, batch=B, **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)


def test_which_calls_take_the_hip_path(dev, monkeypatch):
    from fincflow_amd import glow
    counter = Counter(monkeypatch)
    zero = dict.fromkeys(Counter.NAMES, 0)
    torch.manual_seed(2)
    x = torch.randn(2, 12, 6, 6)
    m = fill(glow.Coupling((12, 6, 6), width=16))

    # float64 on the device: the PyTorch formula
    m64d = copy.deepcopy(m).double().to(dev)
    with torch.no_grad():
        assert not m64d._hip(x.double().to(dev)) and not m64d._hip_device(x.double().to(dev))
        y, ld = m64d(x.double().to(dev))
        r = m64d.reverse(x.double().to(dev))
    assert counter.take() == zero
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        y64, _ = m64(x.double())
        assert rel_err(y.cpu().numpy(), y64.numpy()) <= 1e-12 and rel_err(r.cpu().numpy(), m64.reverse(x.double()).numpy()) <= 1e-12

    # CPU tensors
    with torch.no_grad():
        m(x), m.reverse(x)
    assert counter.take() == zero

    # an odd channel count: no kernel, and the gate says so (the PyTorch formula itself cannot split it: layers/coupling.py:79)
    odd = fill(glow.Coupling((7, 6, 6), width=16)).to(dev)
    assert not odd._hip_device(torch.randn(2, 7, 6, 6, device=dev))
    with torch.no_grad(), pytest.raises(RuntimeError):
        odd(torch.randn(2, 7, 6, 6, device=dev))
    assert counter.take() == zero

    # reverse under autograd: PyTorch, and differentiable
    md = copy.deepcopy(m).to(dev)
    xd = x.to(dev).requires_grad_(True)
    r = md.reverse(xd)
    r.sum().backward()
    assert counter.take() == zero
    x64 = x.double().requires_grad_(True)
    m64.reverse(x64).sum().backward()
    assert rel_err(xd.grad.cpu().numpy(), x64.grad.numpy()) <= TOL

    # frozen parameters and an input without a graph, grad mode on: nothing to record, the inference path
    for p in md.parameters():
        p.requires_grad_(False)
    assert md._hip(x.to(dev))
    md(x.to(dev))
    assert counter.take() == {"finc_coupling": 1, "finc_coupling_backward": 0, "coupling_forward": 0, "finc_bias_relu": 2}


@pytest.mark.parametrize("size,B", [((12, 16, 16), 8), ((48, 4, 4), 8)])
def test_captured_forward_and_reverse_replay_with_the_bits_of_the_eager_call(size, B, dev):
    from fincflow_amd import glow
    m = fill(glow.Coupling(size, width=32)).to(dev)
    torch.manual_seed(sum(size))
    x = torch.randn(B, *size, device=dev)
    with torch.no_grad():
        y0, ld0 = m(x)
        r0 = m.reverse(x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y, ld = m(x)
            r = m.reverse(x)
        for _ in range(3):
            y.zero_(), ld.zero_(), r.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, y0) and torch.equal(ld, ld0) and torch.equal(r, r0)
    from fincflow_amd import _lib
    assert not _lib.fault_pending()
