"""Backward of the per-pixel channel mix on its HIP kernels (finc_mix_backward_f32) and glow.Conv1x1 training on it.

Reference everywhere: autograd through F.conv2d (layers/conv1x1.py:29-31) on the CPU in float64.  Bar: 1e-5 in helpers.rel_err,
the tolerance of BASELINE.json that the backward tests of tests/test_gpu_parity.py use (a B*H*W-term fp32 reduction against
fp64).  Every case appends its achieved errors to the parity report (helpers.report).
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err, report

pytestmark = pytest.mark.gpu

TOL = 1e-5

# the shapes of test_mix_kernel_is_the_1x1_conv, one whose sum crosses many workgroups (B*HW = 2^17 at C = 96), one more at C = 192
SHAPES = [(3, 96, 20, 24), (2, 12, 16, 16), (5, 24, 8, 8), (4, 48, 4, 4), (2, 192, 9, 8), (1, 4, 7, 7), (2, 16, 5, 3), (3, 64, 6, 10),
          (1, 128, 3, 5), (2, 8, 1, 1), (32, 96, 64, 64), (6, 192, 32, 24)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def reference(go, x, M):
    """grad_in, grad_mat, grad_bias of sum(conv2d(x, M, b) * go) by autograd on the CPU in float64."""
    C = M.shape[0]
    xd = x.double().requires_grad_(True)
    Md = M.double().requires_grad_(True)
    bd = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xd, Md.view(C, C, 1, 1), bd) * go.double()).sum().backward()
    return xd.grad.numpy(), Md.grad.numpy(), bd.grad.numpy()


def case(shape):
    B, C, H, W = shape
    torch.manual_seed(sum(shape))
    return torch.randn(B, C, H, W), torch.randn(B, C, H, W), torch.randn(C, C) / C ** 0.5


@pytest.mark.parametrize("shape", SHAPES)
def test_all_three_gradients_against_float64_autograd(shape, dev):
    from fincflow_amd import ops
    go, x, M = case(shape)
    ref = reference(go, x, M)
    got = ops.finc_mix_backward(go.to(dev), x.to(dev), M.to(dev), need_gx=True, need_gm=True, need_gb=True)
    errs = {n: rel_err(g.cpu().numpy(), r) for n, g, r in zip(("grad_in", "grad_mat", "grad_bias"), got, ref)}
    print(shape, errs)
    report("mix_backward", shape=list(shape), **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)


@pytest.mark.parametrize("shape", [(3, 96, 20, 24), (2, 12, 5, 3), (2, 192, 9, 8)])
def test_every_combination_of_skipped_outputs(shape, dev):
    """Straight through the C ABI: a skipped output is NULL, and a buffer that was not passed is not written; the outputs that
    are asked for do not depend on which others are."""
    from fincflow_amd import _lib, ops
    B, C, H, W = shape
    go, x, M = case(shape)
    ref = reference(go, x, M)
    god, xd, Md = go.to(dev), x.to(dev), M.to(dev)
    L = _lib.lib()
    ws = torch.empty(L.finc_mix_backward_workspace_bytes(B, C, H * W), dtype=torch.uint8, device=dev)
    full = ops.finc_mix_backward(god, xd, Md, True, True, True)
    st = torch.cuda.current_stream(dev).cuda_stream
    for want in itertools.product((False, True), repeat=3):
        bufs = [torch.full_like(xd, 7.0), torch.full_like(Md, 7.0), torch.full((C,), 7.0, device=dev)]
        ptrs = [b.data_ptr() if w else None for b, w in zip(bufs, want)]
        rc = L.finc_mix_backward_f32(god.data_ptr(), xd.data_ptr() if want[1] else None, Md.data_ptr(), ptrs[0], ptrs[1], ptrs[2], B, C, H * W,
                                     ws.data_ptr(), ws.numel(), st)
        if not any(want):
            assert rc == 1
            continue
        assert rc == 0, (want, rc)
        torch.cuda.synchronize(dev)
        for n, b, w, r, f in zip(("grad_in", "grad_mat", "grad_bias"), bufs, want, ref, full):
            if w:
                assert rel_err(b.cpu().numpy(), r) <= TOL, (want, n)
                assert torch.equal(b, f), (want, n)
            else:
                assert bool((b == 7.0).all()), (want, n)
    # the Python wrapper: None for what was not asked for
    gx, gm, gb = ops.finc_mix_backward(god, None, Md, need_gx=True, need_gm=False, need_gb=False)
    assert gm is None and gb is None and torch.equal(gx, full[0])


@pytest.mark.parametrize("shape", [(2, 48, 8, 8), (3, 96, 20, 24), (2, 24, 5, 3), (1, 192, 16, 16)])
def test_activations_at_a_four_byte_offset(shape, dev):
    """grad_out, in and grad_in as float-aligned views into larger buffers (the kernels fall back to dword accesses): within
    the bar, nothing written outside the view."""
    from fincflow_amd import ops
    B, C, H, W = shape
    go, x, M = case(shape)
    ref = reference(go, x, M)
    n = x.numel()

    def view(src, off):
        buf = torch.zeros(n + 8, device=dev)
        buf[off:n + off] = src.flatten().to(dev)
        v = buf[off:n + off].view(B, C, H, W)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
        return v
    gov, xv = view(go, 1), view(x, 3)
    Md = M.to(dev)
    got = ops.finc_mix_backward(gov, xv, Md, True, True, True)
    for nme, g, r in zip(("grad_in", "grad_mat", "grad_bias"), got, ref):
        e = rel_err(g.cpu().numpy(), r)
        report("mix_backward_unaligned", shape=list(shape), output=nme, err=e)
        assert e <= TOL, (nme, e)
    # an output view at a 4-byte offset, through the C ABI
    from fincflow_amd import _lib
    L = _lib.lib()
    obuf = torch.zeros(n + 8, device=dev)
    ov = obuf[1:n + 1].view(B, C, H, W)
    rc = L.finc_mix_backward_f32(gov.data_ptr(), None, Md.data_ptr(), ov.data_ptr(), None, None, B, C, H * W, None, 0,
                                 torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert rel_err(ov.cpu().numpy(), ref[0]) <= TOL
    assert float(obuf[:1].abs().sum()) == 0.0 and float(obuf[n + 1:].abs().sum()) == 0.0     # nothing written outside the view


@pytest.mark.parametrize("shape", [(3, 96, 20, 24), (32, 96, 64, 64), (2, 192, 9, 8), (2, 16, 5, 3)])
def test_same_bits_twice_whatever_the_workspace_held(shape, dev):
    from fincflow_amd import _lib
    B, C, H, W = shape
    go, x, M = case(shape)
    god, xd, Md = go.to(dev), x.to(dev), M.to(dev)
    L = _lib.lib()
    nbytes = L.finc_mix_backward_workspace_bytes(B, C, H * W)
    ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def run():
        out = [torch.empty_like(xd), torch.empty_like(Md), torch.empty(C, device=dev)]
        rc = L.finc_mix_backward_f32(god.data_ptr(), xd.data_ptr(), Md.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                     B, C, H * W, ws.data_ptr(), nbytes, st)
        assert rc == 0
        torch.cuda.synchronize(dev)
        return out
    first = run()
    ws.fill_(float("nan"))
    second = run()
    for a, b in zip(first, second):
        assert not bool(torch.isnan(b).any())
        assert torch.equal(a, b)


def test_mix_forward_under_autograd_with_bias(dev):
    from fincflow_amd import ops
    B, C, H, W = 3, 48, 6, 10
    torch.manual_seed(11)
    x, M, b, t = torch.randn(B, C, H, W), torch.randn(C, C) / C ** 0.5, torch.randn(C), torch.randn(B, C, H, W)
    xr, Mr, br = (v.double().requires_grad_(True) for v in (x, M, b))
    ((F.conv2d(xr, Mr.view(C, C, 1, 1), br) * t.double()).sum() + 0.5 * (F.conv2d(xr, Mr.view(C, C, 1, 1), br) ** 2).sum()).backward()
    xd, Md, bd = (v.to(dev).requires_grad_(True) for v in (x, M, b))
    out = ops.mix_forward(xd, Md, bd)
    ((out * t.to(dev)).sum() + 0.5 * (out ** 2).sum()).backward()
    for n, g, r in (("x", xd.grad, xr.grad), ("mat", Md.grad, Mr.grad), ("bias", bd.grad, br.grad)):
        e = rel_err(g.cpu().numpy(), r.numpy())
        report("mix_forward_autograd", output=n, err=e)
        assert e <= TOL, (n, e)
    # gradients only where needed
    x2 = x.to(dev).requires_grad_(True)
    ops.mix_forward(x2, M.to(dev), b.to(dev)).sum().backward()
    assert x2.grad is not None
    M3 = M.to(dev).requires_grad_(True)
    ops.mix_forward(x.to(dev), M3).sum().backward()
    assert rel_err(M3.grad.cpu().numpy(), reference(torch.ones(B, C, H, W), x, M)[1]) <= TOL


def _conv1x1_pair(C, dev, seed):
    from fincflow_amd import glow
    np.random.seed(seed)
    torch.manual_seed(seed)
    c = glow.Conv1x1(C)
    ref = glow.Conv1x1(C).double()
    with torch.no_grad():
        ref.W.copy_(c.W.double())
    return c.to(dev), ref


@pytest.mark.parametrize("C", [12, 48, 96])
def test_conv1x1_trains_on_the_hip_kernels(C, dev, monkeypatch):
    """glow.Conv1x1 on the device under grad, loss (z^2).sum() + ldj.sum(), against the float64 CPU module -- and with
    torch.nn.functional.conv2d patched to raise the forward and the backward still run: the HIP path is the one taken."""
    c, ref = _conv1x1_pair(C, dev, C)
    x = torch.randn(4, C, 10, 12)
    xr = x.double().requires_grad_(True)
    zr, lr = ref(xr)
    ((zr ** 2).sum() + lr.sum()).backward()

    def run():
        c.W.grad = None
        xd = x.to(dev).requires_grad_(True)
        z, ldj = c(xd)
        ((z ** 2).sum() + ldj.sum()).backward()
        return z, xd.grad, c.W.grad
    z, gx, gw = run()
    errs = {"z": rel_err(z.detach().cpu().numpy(), zr.detach().numpy()), "x.grad": rel_err(gx.cpu().numpy(), xr.grad.numpy()),
            "W.grad": rel_err(gw.cpu().numpy(), ref.W.grad.numpy())}
    print(C, errs)
    report("conv1x1_training", C=C, **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)

    def boom(*a, **k):
        raise AssertionError("F.conv2d was called: Conv1x1 did not take the HIP path")
    monkeypatch.setattr(torch.nn.functional, "conv2d", boom)
    z2, gx2, gw2 = run()
    assert torch.equal(z2, z) and torch.equal(gx2, gx) and torch.equal(gw2, gw)


def test_unsupported_channel_count_still_trains_through_conv2d(dev):
    from fincflow_amd import ops
    C = 20
    assert not ops.mix_supported(C)
    c, ref = _conv1x1_pair(C, dev, 20)
    x = torch.randn(3, C, 6, 6)
    xr = x.double().requires_grad_(True)
    zr, lr = ref(xr)
    ((zr ** 2).sum() + lr.sum()).backward()
    xd = x.to(dev).requires_grad_(True)
    z, ldj = c(xd)
    ((z ** 2).sum() + ldj.sum()).backward()
    assert rel_err(xd.grad.cpu().numpy(), xr.grad.numpy()) <= TOL
    assert rel_err(c.W.grad.cpu().numpy(), ref.W.grad.numpy()) <= TOL


def test_flow_step_gradients_equal_the_conv2d_path(dev, monkeypatch):
    """[FastFlowUnit, ActNorm, Conv1x1] log_prob(...).mean().backward(): every parameter's gradient against the same run with
    ops.mix_supported patched to False, i.e. Conv1x1 on F.conv2d autograd."""
    from fincflow_amd import FastFlowUnit, FlowSequential, glow, ops
    from fincflow_amd.layers import StandardNormal
    torch.manual_seed(4)
    np.random.seed(4)
    B, C, H, W = 8, 48, 16, 16
    unit, an, c = FastFlowUnit(C, C, 3), glow.ActNorm(C), glow.Conv1x1(C)
    seq = FlowSequential(StandardNormal((C, H, W)), unit, an, c).to(dev)
    with torch.no_grad():
        an.log_scale.copy_(0.2 * torch.randn(C, device=dev))
        an.translation.copy_(torch.randn(C, device=dev))
        an.initialized.fill_(1)
    x = torch.randn(B, C, H, W, device=dev)

    def grads():
        seq.zero_grad(set_to_none=True)
        seq.log_prob(x).mean().backward()
        return {n: p.grad.detach().cpu().numpy().copy() for n, p in seq.named_parameters()}
    new = grads()
    monkeypatch.setattr(ops, "mix_supported", lambda C: False)
    old = grads()
    monkeypatch.undo()
    assert set(new) == set(old) and any(n.endswith("W") for n in new)
    for n in new:
        e = rel_err(new[n], old[n])
        report("flow_step_gradients", parameter=n, err=e)
        assert e <= TOL, (n, e)
