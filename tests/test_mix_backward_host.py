"""Host side of the mix's backward (finc_mix_backward_f32, include/finc.h): argument validation before any HIP call, the
workspace size, the ABI version gate of the ctypes binding, the unchanged CPU path of glow.Conv1x1, and the register
allocation of the new weight-gradient kernel -- no GPU needed, the library built."""
import os

import pytest
import torch

from fincflow_amd import _lib
from helpers import fake_ptr as p, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_CHANNELS = (4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192)


def test_status_codes_without_touching_the_gpu():
    """NULL -> 1, bad dims / aliasing -> 2, alignment below 4 bytes -> 7, unsupported C -> 3, workspace -> 4, in that order of
    precedence, with fake pointers: nothing is launched."""
    L = _lib.lib()
    go, x, m, gi, gm, gb, ws = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000), p(0x6000), p(0x10000)
    big = 1 << 40
    f = L.finc_mix_backward_f32
    # NULL pointers
    assert f(None, x, m, gi, gm, gb, 2, 48, 64, ws, big, None) == 1
    assert f(go, x, None, gi, gm, gb, 2, 48, 64, ws, big, None) == 1
    assert f(go, x, m, None, None, None, 2, 48, 64, ws, big, None) == 1          # nothing asked for
    assert f(go, None, m, gi, gm, None, 2, 48, 64, ws, big, None) == 1           # grad_mat needs `in`
    assert f(None, x, m, gi, gm, gb, 0, 48, 64, ws, big, None) == 1              # (NULL comes before the dims)
    # bad dims, aliasing
    for B, C, HW in ((0, 48, 64), (2, 0, 64), (2, 48, 0), (-1, 48, 64), (2, 1 << 20, 64)):
        assert f(go, x, m, gi, gm, gb, B, C, HW, ws, big, None) == 2
    assert f(go, x, m, go, gm, gb, 2, 48, 64, ws, big, None) == 2                # grad_in == grad_out
    assert f(go, x, m, x, gm, gb, 2, 48, 64, ws, big, None) == 2                 # grad_in == in
    assert f(p(0x1002), x, m, gi, gm, gb, 0, 48, 64, ws, big, None) == 2         # (dims come before the alignment)
    # alignment
    assert f(p(0x1002), x, m, gi, gm, gb, 2, 48, 64, ws, big, None) == 7
    assert f(go, p(0x2001), m, gi, gm, gb, 2, 48, 64, ws, big, None) == 7
    assert f(go, x, m, gi, p(0x5003), gb, 2, 48, 64, ws, big, None) == 7
    assert f(p(0x1002), x, m, gi, gm, gb, 2, 20, 64, ws, big, None) == 7         # (alignment comes before the channel count)
    # channel counts without an instantiation
    for C in (20, 7):
        assert L.finc_mix_supported_f32(C) == 0
        assert f(go, x, m, gi, gm, gb, 2, C, 64, ws, big, None) == 3
        assert f(go, x, m, gi, gm, gb, 2, C, 64, None, 0, None) == 3             # (... before the workspace)
    # workspace missing or too small while grad_mat or grad_bias is wanted
    need = L.finc_mix_backward_workspace_bytes(2, 48, 64)
    assert f(go, x, m, gi, gm, gb, 2, 48, 64, None, big, None) == 4
    assert f(go, x, m, gi, gm, gb, 2, 48, 64, ws, need - 1, None) == 4
    assert f(go, x, m, None, gm, None, 2, 48, 64, ws, 0, None) == 4
    assert f(go, None, m, None, None, gb, 2, 48, 64, None, 0, None) == 4


def test_workspace_size_is_positive_and_monotone_in_the_pixel_count():
    L = _lib.lib()
    shapes = [(1, 1), (2, 1), (1, 7), (16, 1), (1, 32), (3, 25), (2, 64), (5, 64), (64, 1024), (256, 4096), (64, 16384), (1024, 16384)]
    shapes.sort(key=lambda s: s[0] * s[1])
    for C in MIX_CHANNELS:
        assert L.finc_mix_supported_f32(C) == 1
        last = 0
        for B, HW in shapes:
            n = int(L.finc_mix_backward_workspace_bytes(B, C, HW))
            assert n > 0, (C, B, HW)
            assert n >= last, (C, B, HW, n, last)
            last = n


def test_version_is_103_and_an_older_library_is_refused_by_name(tmp_path):
    assert _lib.lib().finc_version() >= 103
    assert _lib.ABI_VERSION >= 103
    out = load_stub_library(tmp_path, 102, mask_path=False)
    assert "102" in out and "103" in out, out


def test_conv1x1_on_cpu_tensors_is_plain_conv2d_autograd():
    """The fallback path is unchanged: output and both gradients EQUAL those of F.conv2d autograd."""
    import numpy as np
    import torch.nn.functional as F
    from fincflow_amd import glow
    np.random.seed(5)
    torch.manual_seed(5)
    for C in (12, 20, 48):
        c = glow.Conv1x1(C)
        x = torch.randn(3, C, 5, 6, requires_grad=True)
        z, ldj = c(x)
        ((z ** 2).sum() + ldj.sum()).backward()
        W = c.W.detach().clone().requires_grad_(True)
        x2 = x.detach().clone().requires_grad_(True)
        z2 = F.conv2d(x2, W.view(C, C, 1, 1))
        ldj2 = 5 * 6 * torch.slogdet(W)[1]
        ((z2 ** 2).sum() + ldj2.sum()).backward()
        assert torch.equal(z, z2) and torch.equal(ldj, ldj2)
        assert torch.equal(x.grad, x2.grad) and torch.equal(c.W.grad, W.grad)


def test_weight_gradient_kernel_is_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    main = {k: v for k, v in md.items() if "finc_mix_gradw_kernel" in k}
    assert len(main) == 2 * len(MIX_CHANNELS), sorted(main)              # dword and 16-byte form of every channel count
    reduce = {k: v for k, v in md.items() if "mix_gradw_reduce_kernel" in k}
    assert len(reduce) == 1, sorted(reduce)
    for k, v in {**main, **reduce}.items():
        assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)
