"""Host side of the backwards of the per-pixel layers' reverse direction (finc_coupling_reverse_backward_f32,
finc_actnorm_reverse_backward_f32; include/finc.h): the exported symbols and the fourth ABI version gate, argument refusals before
any HIP call, the kernels' register allocation, and the unchanged PyTorch lines of glow.Coupling / SplitPrior / ActNorm / Conv1x1 on
CPU tensors inside `reverse_grad()` -- no GPU needed, the library built."""
import os

import pytest
import torch

from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("finc_coupling_reverse_backward_f32", "finc_actnorm_reverse_backward_f32")


def test_new_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    from fincflow_amd import ops
    for name in ("finc_coupling_reverse_backward", "finc_actnorm_reverse_backward", "coupling_reverse", "actnorm_reverse"):
        assert callable(getattr(ops, name)), name


def test_version_is_108_and_a_107_library_is_refused_by_name(tmp_path):
    assert _lib.lib().finc_version() >= _lib.REVERSE_BACKWARD_ABI_VERSION == 108
    assert _lib.ABI_VERSION == 104 and _lib.ACTNORM_ABI_VERSION == 105 and _lib.INVERSE_BACKWARD_ABI_VERSION == 107
    out = load_stub_library(tmp_path, 107)
    assert "= 107" in out and "108" in out and "finc_coupling_reverse_backward_f32" in out, out
    assert "finc_actnorm_reverse_backward_f32" in out, out


def test_coupling_reverse_backward_status_codes_without_touching_the_gpu():
    """NULL -> 1, bad dims / aliasing -> 2, alignment below 4 bytes -> 7, odd C -> 3, workspace -> 4, in that order of precedence,
    with fake pointers: nothing is launched."""
    L = _lib.lib()
    gy, y, raw, a, b = _p(0x1000), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000)
    gx, gr, ga, gb, ws = _p(0x6000), _p(0x7000), _p(0x8000), _p(0x9000), _p(0x10000)
    big = 1 << 40
    f = L.finc_coupling_reverse_backward_f32
    for k in range(5):                                                       # grad_y, y, raw, a, b are all required
        args = [gy, y, raw, a, b]
        args[k] = None
        assert f(*args, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 1, k
    assert f(gy, y, raw, a, b, None, None, None, None, 2, 12, 64, ws, big, None) == 1          # nothing asked for
    assert f(None, y, raw, a, b, gx, gr, ga, gb, 0, 12, 64, ws, big, None) == 1                # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64), (1 << 20, 4096, 1 << 20)):
        assert f(gy, y, raw, a, b, gx, gr, ga, gb, B, C, HW, ws, big, None) == 2, (B, C, HW)
    for alias in (gy, y, raw):
        assert f(gy, y, raw, a, b, alias, gr, ga, gb, 2, 12, 64, ws, big, None) == 2          # grad_x on an input
        assert f(gy, y, raw, a, b, gx, alias, ga, gb, 2, 12, 64, ws, big, None) == 2          # grad_raw on an input
    assert f(gy, y, raw, a, b, gx, gx, ga, gb, 2, 12, 64, ws, big, None) == 2                  # grad_raw == grad_x
    assert f(_p(0x1002), y, raw, a, b, gx, gr, ga, gb, 0, 12, 64, ws, big, None) == 2          # (dims come before the alignment)
    assert f(_p(0x1002), y, raw, a, b, y, gr, ga, gb, 2, 12, 64, ws, big, None) == 2           # (aliasing comes before the alignment)
    assert f(_p(0x1002), y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, _p(0x2001), raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, y, raw, a, b, gx, gr, _p(0x8003), gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, y, raw, a, b, gx, _p(0x7002), ga, gb, 2, 12, 64, None, 0, None) == 7          # (alignment before the workspace)
    assert f(_p(0x1002), y, raw, a, b, gx, gr, ga, gb, 2, 13, 64, ws, big, None) == 7          # (alignment before the channel count)
    for C in (13, 7, 1):
        assert f(gy, y, raw, a, b, gx, gr, ga, gb, 2, C, 64, ws, big, None) == 3, C
        assert f(gy, y, raw, a, b, gx, gr, ga, gb, 2, C, 64, None, 0, None) == 3, C            # (... before the workspace)
        assert f(gy, y, raw, a, b, gx, None, None, None, 2, C, 64, None, 0, None) == 3, C
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(gy, y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, None, big, None) == 4
    assert f(gy, y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, need - 1, None) == 4
    assert f(gy, y, raw, a, b, None, None, ga, None, 2, 12, 64, ws, 0, None) == 4
    assert f(gy, y, raw, a, b, None, None, None, gb, 2, 12, 64, None, 0, None) == 4
    assert f(gy, y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, _p(0x10002), big, None) == 4


def test_actnorm_reverse_backward_status_codes_without_touching_the_gpu():
    """NULL -> 1, bad dims / aliasing -> 2, alignment below 4 bytes -> 7, workspace -> 4, in that order, nothing launched."""
    L = _lib.lib()
    gy, x, ls = _p(0x1000), _p(0x2000), _p(0x3000)
    gx, gls, gt, ws = _p(0x6000), _p(0x8000), _p(0x9000), _p(0x10000)
    big = 1 << 40
    f = L.finc_actnorm_reverse_backward_f32
    for k in range(3):                                                       # grad_y, x, log_scale are all required
        args = [gy, x, ls]
        args[k] = None
        assert f(*args, gx, gls, gt, 2, 12, 64, ws, big, None) == 1, k
    assert f(gy, x, ls, None, None, None, 2, 12, 64, ws, big, None) == 1         # nothing asked for
    assert f(None, x, ls, gx, gls, gt, 0, 12, 64, ws, big, None) == 1            # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64), (1 << 20, 4096, 1 << 20)):
        assert f(gy, x, ls, gx, gls, gt, B, C, HW, ws, big, None) == 2, (B, C, HW)
    assert f(gy, x, ls, x, gls, gt, 2, 12, 64, ws, big, None) == 2               # grad_x on x
    assert f(_p(0x1002), x, ls, gx, gls, gt, 0, 12, 64, ws, big, None) == 2      # (dims come before the alignment)
    assert f(_p(0x1002), x, ls, x, gls, gt, 2, 12, 64, ws, big, None) == 2       # (aliasing comes before the alignment)
    assert f(_p(0x1002), x, ls, gx, gls, gt, 2, 12, 64, ws, big, None) == 7
    assert f(gy, _p(0x2001), ls, gx, gls, gt, 2, 12, 64, ws, big, None) == 7
    assert f(gy, x, _p(0x3002), gx, gls, gt, 2, 12, 64, ws, big, None) == 7
    assert f(gy, x, ls, gx, _p(0x8003), gt, 2, 12, 64, ws, big, None) == 7
    assert f(gy, x, ls, gx, gls, _p(0x9002), 2, 12, 64, None, 0, None) == 7      # (alignment comes before the workspace)
    for C in (13, 1, 513):                                                   # any channel count has a kernel: the workspace is next
        assert f(gy, x, ls, gx, gls, gt, 2, C, 64, None, 0, None) == 4, C
    need = L.finc_actnorm_workspace_bytes(2, 12, 64)
    assert f(gy, x, ls, gx, gls, gt, 2, 12, 64, None, big, None) == 4
    assert f(gy, x, ls, gx, gls, gt, 2, 12, 64, ws, need - 1, None) == 4
    assert f(gy, x, ls, None, gls, None, 2, 12, 64, ws, 0, None) == 4
    assert f(gy, x, ls, None, None, gt, 2, 12, 64, None, 0, None) == 4
    assert f(gy, x, ls, gx, gls, gt, 2, 12, 64, _p(0x10002), big, None) == 4


def test_reverse_backward_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    for name in ("finc_coupling_rev_bwd_kernel", "finc_actnorm_rev_bwd_kernel"):
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == 2, (name, sorted(ks))                             # the 16-byte and the dword form
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the module gates on CPU tensors: inside reverse_grad() nothing changes, fp32 or fp64
# ---------------------------------------------------------------------------------------------------------------------------------
def _fill(m, dtype, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            scale = 0.1 if name.endswith(("bias", "logs", "log_scale", "translation")) else 0.05
            if name == "W":
                continue                                                    # (Conv1x1 keeps its orthogonal initialisation)
            p.copy_(torch.randn(p.shape, generator=g) * scale)
    return m.to(dtype)


def _modules(dtype):
    from fincflow_amd import glow
    torch.manual_seed(3)
    act = glow.ActNorm(12)
    act.mark_initialized()
    split = glow.SplitPrior((12, 6, 5), glow.GaussianPrior, width=16)
    return [("coupling", _fill(glow.Coupling((12, 6, 5), width=16), dtype), (3, 12, 6, 5), None),
            ("coupling_context", _fill(glow.Coupling((12, 6, 5), width=16, n_context=3), dtype), (3, 12, 6, 5), (3, 3, 6, 5)),
            ("coupling_two_channels", _fill(glow.Coupling((2, 6, 5), width=16), dtype), (3, 2, 6, 5), None),
            ("split_prior", _fill(split, dtype), (3, 6, 6, 5), None),
            ("actnorm", _fill(act, dtype), (3, 12, 6, 5), None),
            ("actnorm_2d", _fill(act, dtype), (7, 12), None),
            ("conv1x1", _fill(glow.Conv1x1(12), dtype), (3, 12, 6, 5), None)]


def _reverse_and_gradients(m, x, ctx, inside):
    import fincflow_amd
    import contextlib
    m.zero_grad()
    xa = x.clone().requires_grad_(True)
    torch.manual_seed(9)                                                    # (SplitPrior.reverse draws its second half)
    with (fincflow_amd.reverse_grad() if inside else contextlib.nullcontext()):
        y = m.reverse(xa, ctx)
    (y ** 2).sum().backward()
    return y.detach(), type(y.grad_fn).__name__, [xa.grad.clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_tensors_keep_the_pytorch_lines_inside_the_context(dtype):
    """Unlike the unit, these layers do not raise inside `reverse_grad()` for CPU tensors or fp64: result, recorded node and every
    gradient are bit-equal to the call outside the context."""
    for name, m, shape, cshape in _modules(dtype):
        torch.manual_seed(5)
        x = torch.randn(shape, dtype=dtype)
        ctx = None if cshape is None else torch.randn(cshape, dtype=dtype)
        y0, node0, g0 = _reverse_and_gradients(m, x, ctx, False)
        y1, node1, g1 = _reverse_and_gradients(m, x, ctx, True)
        assert node0 == node1 and "Finc" not in node1, (name, node0, node1)
        assert torch.equal(y0, y1), name
        assert len(g0) == len(g1) >= 2 and all(torch.equal(a, b) for a, b in zip(g0, g1)), name


def test_frozen_modules_on_cpu_record_nothing_new_either():
    import fincflow_amd
    for name, m, shape, cshape in _modules(torch.float32):
        m.requires_grad_(False)
        x = torch.randn(shape)
        ctx = None if cshape is None else torch.randn(cshape)
        torch.manual_seed(9)
        want = m.reverse(x, ctx)
        torch.manual_seed(9)
        with fincflow_amd.reverse_grad():
            got = m.reverse(x, ctx)
        assert not got.requires_grad and torch.equal(got, want), name
