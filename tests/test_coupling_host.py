"""Host side of the coupling kernels (finc_coupling_f32, finc_coupling_backward_f32, finc_bias_relu_f32; include/finc.h): the
exported symbols and the ABI version gate, argument refusals before any HIP call, the workspace size, the kernels' register
allocation, and the unchanged PyTorch path of glow.Coupling / SplitPrior on CPU tensors -- no GPU needed, the library built."""
import os

import pytest
import torch
import torch.nn.functional as F

from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("finc_coupling_supported_f32", "finc_coupling_workspace_bytes", "finc_coupling_f32", "finc_coupling_backward_f32",
               "finc_bias_relu_f32")


def test_new_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    from fincflow_amd import ops
    for name in ("finc_coupling", "finc_coupling_backward", "coupling_forward", "finc_bias_relu", "coupling_supported"):
        assert callable(getattr(ops, name)), name
    assert ops.coupling_supported(12) and ops.coupling_supported(2) and not ops.coupling_supported(7) and not ops.coupling_supported(0)


def test_version_is_104_and_a_103_library_is_refused_by_name(tmp_path):
    assert _lib.lib().finc_version() >= 104
    assert _lib.ABI_VERSION >= 104
    out = load_stub_library(tmp_path, 103)
    assert "= 103" in out and "at least 104" in out, out


def test_coupling_status_codes_without_touching_the_gpu():
    """NULL -> 1, bad dims / direction / aliasing -> 2, alignment below 4 bytes -> 7, odd C -> 3, workspace -> 4, in that order of
    precedence, with fake pointers: nothing is launched."""
    L = _lib.lib()
    x, raw, a, b, y, ld, ws = _p(0x1000), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000), _p(0x6000), _p(0x10000)
    big = 1 << 40
    f = L.finc_coupling_f32
    for k in range(5):                                                       # each required pointer
        args = [x, raw, a, b, y]
        args[k] = None
        assert f(*args, ld, 2, 12, 64, 1, ws, big, None) == 1, k
    assert f(None, raw, a, b, y, ld, 0, 12, 64, 1, ws, big, None) == 1           # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64)):
        assert f(x, raw, a, b, y, ld, B, C, HW, 1, ws, big, None) == 2, (B, C, HW)
    for d in (0, 2, -2):
        assert f(x, raw, a, b, y, ld, 2, 12, 64, d, ws, big, None) == 2, d
    assert f(x, raw, a, b, raw, ld, 2, 12, 64, 1, ws, big, None) == 2            # y == raw
    assert f(_p(0x1002), raw, a, b, y, ld, 0, 12, 64, 1, ws, big, None) == 2     # (dims come before the alignment)
    assert f(_p(0x1002), raw, a, b, y, ld, 2, 12, 64, 1, ws, big, None) == 7
    assert f(x, raw, a, b, _p(0x5001), ld, 2, 12, 64, 1, ws, big, None) == 7
    assert f(_p(0x1002), raw, a, b, y, ld, 2, 13, 64, 1, ws, big, None) == 7     # (alignment comes before the channel count)
    for C in (13, 7, 1):
        assert L.finc_coupling_supported_f32(C) == 0
        assert f(x, raw, a, b, y, ld, 2, C, 64, 1, ws, big, None) == 3, C
        assert f(x, raw, a, b, y, ld, 2, C, 64, 1, None, 0, None) == 3, C        # (... before the workspace)
        assert f(x, raw, a, b, y, None, 2, C, 64, -1, None, 0, None) == 3, C
    for C in (2, 4, 12, 96, 192, 4096):
        assert L.finc_coupling_supported_f32(C) == 1
    # the forward with a log-det needs the workspace; nothing else of this call does (those cases would launch: not tried here)
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(x, raw, a, b, y, ld, 2, 12, 64, 1, None, big, None) == 4
    assert f(x, raw, a, b, y, ld, 2, 12, 64, 1, ws, need - 1, None) == 4
    assert f(x, raw, a, b, y, ld, 2, 12, 64, 1, ws, 0, None) == 4


def test_coupling_backward_status_codes_without_touching_the_gpu():
    L = _lib.lib()
    gy, gl, x, raw, a, b = _p(0x1000), _p(0x1800), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000)
    gx, gr, ga, gb, ws = _p(0x6000), _p(0x7000), _p(0x8000), _p(0x9000), _p(0x10000)
    big = 1 << 40
    f = L.finc_coupling_backward_f32
    for k in (0, 2, 3, 4, 5):                                                # grad_y, x, raw, a, b are required; grad_logdet is not
        args = [gy, gl, x, raw, a, b]
        args[k] = None
        assert f(*args, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 1, k
    assert f(gy, gl, x, raw, a, b, None, None, None, None, 2, 12, 64, ws, big, None) == 1      # nothing asked for
    assert f(None, gl, x, raw, a, b, gx, gr, ga, gb, 0, 12, 64, ws, big, None) == 1            # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 1 << 20, 64)):
        assert f(gy, gl, x, raw, a, b, gx, gr, ga, gb, B, C, HW, ws, big, None) == 2, (B, C, HW)
    for alias in (gy, x, raw):
        assert f(gy, gl, x, raw, a, b, alias, gr, ga, gb, 2, 12, 64, ws, big, None) == 2      # grad_x on an input
        assert f(gy, gl, x, raw, a, b, gx, alias, ga, gb, 2, 12, 64, ws, big, None) == 2      # grad_raw on an input
    assert f(gy, gl, x, raw, a, b, gx, gx, ga, gb, 2, 12, 64, ws, big, None) == 2              # grad_raw == grad_x
    assert f(_p(0x1002), gl, x, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, _p(0x1801), x, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, gl, x, raw, a, b, gx, gr, _p(0x8003), gb, 2, 12, 64, ws, big, None) == 7
    assert f(_p(0x1002), gl, x, raw, a, b, gx, gr, ga, gb, 2, 13, 64, ws, big, None) == 7      # (alignment before the channel count)
    for C in (13, 7):
        assert f(gy, gl, x, raw, a, b, gx, gr, ga, gb, 2, C, 64, ws, big, None) == 3
        assert f(gy, gl, x, raw, a, b, gx, gr, ga, gb, 2, C, 64, None, 0, None) == 3           # (... before the workspace)
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(gy, gl, x, raw, a, b, gx, gr, ga, gb, 2, 12, 64, None, big, None) == 4
    assert f(gy, gl, x, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, need - 1, None) == 4
    assert f(gy, None, x, raw, a, b, None, None, ga, None, 2, 12, 64, ws, 0, None) == 4
    assert f(gy, None, x, raw, a, b, None, None, None, gb, 2, 12, 64, None, 0, None) == 4


def test_bias_relu_status_codes_without_touching_the_gpu():
    L = _lib.lib()
    i, b, o = _p(0x1000), _p(0x2000), _p(0x3000)
    f = L.finc_bias_relu_f32
    assert f(None, b, o, 2, 512, 64, None) == 1
    assert f(i, None, o, 2, 512, 64, None) == 1
    assert f(i, b, None, 2, 512, 64, None) == 1
    assert f(None, b, o, 0, 512, 64, None) == 1
    for B, C, HW in ((0, 512, 64), (2, 0, 64), (2, 512, 0), (-1, 512, 64), (1 << 20, 1 << 20, 1 << 10)):
        assert f(i, b, o, B, C, HW, None) == 2, (B, C, HW)
    assert f(_p(0x1002), b, o, 0, 512, 64, None) == 2
    assert f(_p(0x1002), b, o, 2, 512, 64, None) == 7
    assert f(i, _p(0x2001), o, 2, 512, 64, None) == 7
    assert f(i, b, _p(0x3003), 2, 512, 64, None) == 7


def test_workspace_size_is_positive_monotone_and_a_function_of_its_arguments():
    L = _lib.lib()
    Bs = (1, 2, 3, 5, 8, 16, 64, 128, 255, 256, 1000, 1025, 2048, 2049, 5000, 65536)
    HWs = (1, 3, 15, 16, 49, 64, 256, 720, 1024, 4096, 16384, 65536)
    for C in (2, 4, 12, 24, 48, 96, 192, 512):
        table = {}
        for B in Bs:
            for HW in HWs:
                n = int(L.finc_coupling_workspace_bytes(B, C, HW))
                assert n > 0, (C, B, HW)
                assert n == int(L.finc_coupling_workspace_bytes(B, C, HW)), (C, B, HW)
                table[B, HW] = n
        for HW in HWs:
            col = [table[B, HW] for B in Bs]
            assert col == sorted(col), ("B", C, HW, col)
        for B in Bs:
            row = [table[B, HW] for HW in HWs]
            assert row == sorted(row), ("HW", C, B, row)
    for bad in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-4, 12, 64)):
        assert int(L.finc_coupling_workspace_bytes(*bad)) > 0


def plain_coupling(m, x, context, reverse):
    """Today's formula (layers/coupling.py:69-101), restated."""
    half = m.n_channels // 2
    x1, x2 = x[:, :half], x[:, half:]
    n = m.net
    h = x1 if context is None else torch.cat([x1, context], dim=1)
    h = F.relu(F.conv2d(h, n[0].weight, n[0].bias, padding=1))
    h = F.relu(F.conv2d(h, n[2].weight, n[2].bias))
    h = F.conv2d(h, n[4].weight, n[4].bias, padding=1) * torch.exp(n[4].logs * 3).view(1, -1, 1, 1)
    log_s = 2.0 * torch.tanh(h[:, ::2] / 2.0)
    t = h[:, 1::2]
    if reverse:
        return torch.cat([x1, (x2 - t) * torch.exp(-log_s)], dim=1)
    return torch.cat([x1, x2 * torch.exp(log_s) + t], dim=1), log_s.flatten(start_dim=1).sum(-1)


def _fill(m, dtype):
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, p in m.named_parameters():
            scale = 0.1 if name.endswith(("bias", "logs")) else 0.05
            p.copy_(torch.randn(p.shape, generator=g) * scale)
    return m.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n_context", [None, 3])
@pytest.mark.parametrize("C", [12, 2])
def test_coupling_on_cpu_tensors_is_the_plain_formula_bit_for_bit(dtype, n_context, C):
    from fincflow_amd import glow
    torch.manual_seed(3)
    m = _fill(glow.Coupling((C, 6, 5), width=16, n_context=n_context), dtype)
    x = torch.randn(3, C, 6, 5, dtype=dtype)
    ctx = None if n_context is None else torch.randn(3, n_context, 6, 5, dtype=dtype)
    assert not m._hip(x, ctx) and not m._hip_train(x, ctx)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            y, ld = m(x, ctx)
            r = m.reverse(x, ctx)
            y0, ld0 = plain_coupling(m, x, ctx, False)
            r0 = plain_coupling(m, x, ctx, True)
        assert torch.equal(y, y0) and torch.equal(ld, ld0) and torch.equal(r, r0), (dtype, n_context, C, grad)
    # and its gradients are autograd's through that formula
    xa = x.clone().requires_grad_(True)
    y, ld = m(xa, ctx)
    ((y ** 2).sum() + ld.sum()).backward()
    got = [xa.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    m.zero_grad()
    xb = x.clone().requires_grad_(True)
    y0, ld0 = plain_coupling(m, xb, ctx, False)
    ((y0 ** 2).sum() + ld0.sum()).backward()
    want = [xb.grad] + [p.grad for p in m.parameters()]
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_splitprior_on_cpu_tensors_is_the_plain_formula_bit_for_bit(dtype):
    from fincflow_amd import glow
    m = glow.SplitPrior((12, 4, 6), glow.GaussianPrior, width=16)
    _fill(m.transform, dtype)
    m = m.to(dtype)
    torch.manual_seed(4)
    x = torch.randn(2, 12, 4, 6, dtype=dtype)
    with torch.no_grad():
        z, ldj = m(x)
        y0, ld0 = plain_coupling(m.transform, x, None, False)
    assert torch.equal(z, y0[:, :6])
    assert torch.equal(ldj, m.base.log_prob(y0[:, 6:]) + ld0)
    # reverse draws its second half: the same seed, the same draw
    with torch.no_grad():
        torch.manual_seed(9)
        r = m.reverse(z)
        torch.manual_seed(9)
        x2, _ = m.base.sample(2)
        r0 = plain_coupling(m.transform, torch.cat([z, x2.to(dtype)], dim=1), None, True)
    assert torch.equal(r, r0)


def test_state_dict_keys_of_coupling_did_not_move():
    from fincflow_amd import glow
    keys = list(glow.Coupling((12, 4, 4), width=8).state_dict())
    assert keys == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "net.4.logs"], keys
    keys = list(glow.SplitPrior((12, 4, 4), glow.GaussianPrior, width=8).state_dict())
    assert keys == ["transform." + k for k in ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias",
                                               "net.4.logs")], keys


def test_coupling_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    want = {"finc_coupling_kernel": 6, "finc_coupling_bwd_kernel": 2, "finc_coupling_reduce_kernel": 1, "finc_bias_relu_kernel": 2}
    for name, count in want.items():
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == count, (name, sorted(ks))
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)
