"""Host side of the ActNorm kernels (finc_actnorm_f32, finc_actnorm_backward_f32, finc_actnorm_init_f32; include/finc.h): the
exported symbols and the second ABI version gate, argument refusals before any HIP call, the workspace size, the kernels' register
allocation, and the unchanged PyTorch path of glow.ActNorm on CPU tensors against the reference-made fixtures
(tests/golden/make_golden_actnorm.py) -- no GPU needed, the library built."""
import os

import numpy as np
import pytest
import torch

from actnorm_cases import BIG, BIG_IMAGES, CASES, inputs
from fincflow_amd import _lib
from helpers import fake_ptr as _p, golden, load_stub_library, rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("finc_actnorm_workspace_bytes", "finc_actnorm_f32", "finc_actnorm_backward_f32", "finc_actnorm_init_f32")


def test_new_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    from fincflow_amd import ops
    for name in ("finc_actnorm", "finc_actnorm_backward", "finc_actnorm_init", "actnorm_forward", "actnorm_supported"):
        assert callable(getattr(ops, name)), name
    assert ops.actnorm_supported()


def test_version_is_105_and_older_libraries_are_refused_by_name(tmp_path):
    assert _lib.lib().finc_version() >= 105
    assert _lib.ABI_VERSION == 104 and _lib.ACTNORM_ABI_VERSION == 105
    out = load_stub_library(tmp_path, 104)
    assert "= 104" in out and "105" in out and "finc_actnorm_f32" in out, out
    out = load_stub_library(tmp_path, 103)
    assert "= 103" in out and "at least 104" in out, out


def test_actnorm_status_codes_without_touching_the_gpu():
    """NULL -> 1, bad dims / direction -> 2, alignment below 4 bytes -> 7, in that order of precedence, with fake pointers: nothing is
    launched."""
    L = _lib.lib()
    x, ls, t, y, ld = _p(0x1000), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000)
    f = L.finc_actnorm_f32
    for k in range(4):                                                       # each required pointer; logdet is not one
        args = [x, ls, t, y]
        args[k] = None
        assert f(*args, ld, 2, 12, 64, 1, None) == 1, k
    assert f(None, ls, t, y, ld, 0, 12, 64, 1, None) == 1                        # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64), (1 << 20, 4096, 1 << 20)):
        assert f(x, ls, t, y, ld, B, C, HW, 1, None) == 2, (B, C, HW)
    for d in (0, 2, -2):
        assert f(x, ls, t, y, ld, 2, 12, 64, d, None) == 2, d
    assert f(_p(0x1002), ls, t, y, ld, 0, 12, 64, 1, None) == 2                  # (dims come before the alignment)
    assert f(_p(0x1002), ls, t, y, ld, 2, 12, 64, 3, None) == 2                  # (and so does the direction)
    assert f(_p(0x1002), ls, t, y, ld, 2, 12, 64, 1, None) == 7
    assert f(x, _p(0x2001), t, y, ld, 2, 12, 64, 1, None) == 7
    assert f(x, ls, _p(0x3003), y, ld, 2, 12, 64, -1, None) == 7
    assert f(x, ls, t, _p(0x4002), None, 2, 12, 64, 1, None) == 7
    assert f(x, ls, t, y, _p(0x5001), 2, 12, 64, 1, None) == 7


def test_actnorm_backward_status_codes_without_touching_the_gpu():
    L = _lib.lib()
    gy, gl, y, ls = _p(0x1000), _p(0x1800), _p(0x2000), _p(0x3000)
    gx, gls, gt, ws = _p(0x6000), _p(0x8000), _p(0x9000), _p(0x10000)
    big = 1 << 40
    f = L.finc_actnorm_backward_f32
    for k in (0, 2, 3):                                                      # grad_y, y, log_scale are required; grad_logdet is not
        args = [gy, gl, y, ls]
        args[k] = None
        assert f(*args, gx, gls, gt, 2, 12, 64, ws, big, None) == 1, k
    assert f(gy, gl, y, ls, None, None, None, 2, 12, 64, ws, big, None) == 1     # nothing asked for
    assert f(None, gl, y, ls, gx, gls, gt, 0, 12, 64, ws, big, None) == 1        # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 1 << 20, 64)):
        assert f(gy, gl, y, ls, gx, gls, gt, B, C, HW, ws, big, None) == 2, (B, C, HW)
    assert f(gy, gl, y, ls, y, gls, gt, 2, 12, 64, ws, big, None) == 2           # grad_x on y
    assert f(_p(0x1002), gl, y, ls, y, gls, gt, 2, 12, 64, ws, big, None) == 2   # (aliasing comes before the alignment)
    assert f(_p(0x1002), gl, y, ls, gx, gls, gt, 2, 12, 64, ws, big, None) == 7
    assert f(gy, _p(0x1801), y, ls, gx, gls, gt, 2, 12, 64, ws, big, None) == 7
    assert f(gy, gl, y, ls, gx, _p(0x8003), gt, 2, 12, 64, ws, big, None) == 7
    assert f(gy, gl, y, ls, gx, gls, _p(0x9002), 2, 12, 64, None, 0, None) == 7  # (alignment comes before the workspace)
    need = L.finc_actnorm_workspace_bytes(2, 12, 64)
    assert f(gy, gl, y, ls, gx, gls, gt, 2, 12, 64, None, big, None) == 4
    assert f(gy, gl, y, ls, gx, gls, gt, 2, 12, 64, ws, need - 1, None) == 4
    assert f(gy, None, y, ls, None, gls, None, 2, 12, 64, ws, 0, None) == 4
    assert f(gy, None, y, ls, None, None, gt, 2, 12, 64, None, 0, None) == 4
    assert f(gy, gl, y, ls, gx, gls, gt, 2, 12, 64, _p(0x10002), big, None) == 4


def test_actnorm_init_status_codes_without_touching_the_gpu():
    L = _lib.lib()
    x, ls, t, ws = _p(0x1000), _p(0x2000), _p(0x3000), _p(0x10000)
    big = 1 << 40
    f = L.finc_actnorm_init_f32
    for k in range(3):
        args = [x, ls, t]
        args[k] = None
        assert f(*args, 2, 12, 64, ws, big, None) == 1, k
    assert f(None, ls, t, 0, 12, 64, ws, big, None) == 1
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 1 << 20, 64), (1, 12, 1)):   # (1, 12, 1): one value per channel
        assert f(x, ls, t, B, C, HW, ws, big, None) == 2, (B, C, HW)
    assert f(x, ls, ls, 2, 12, 64, ws, big, None) == 2                           # one buffer for both parameters
    assert f(_p(0x1002), ls, t, 1, 12, 1, ws, big, None) == 2                    # (dims come before the alignment)
    assert f(_p(0x1002), ls, t, 2, 12, 64, ws, big, None) == 7
    assert f(x, _p(0x2002), t, 2, 12, 64, None, 0, None) == 7                    # (alignment comes before the workspace)
    assert f(x, ls, _p(0x3001), 2, 12, 64, ws, big, None) == 7
    need = L.finc_actnorm_workspace_bytes(2, 12, 64)
    assert f(x, ls, t, 2, 12, 64, None, big, None) == 4
    assert f(x, ls, t, 2, 12, 64, ws, need - 1, None) == 4
    assert f(x, ls, t, 2, 12, 64, ws, 0, None) == 4


def test_workspace_size_is_positive_monotone_and_a_function_of_its_arguments():
    L = _lib.lib()
    Bs = (1, 2, 3, 5, 8, 16, 64, 128, 255, 256, 1000, 1025, 2048, 2049, 5000, 65536)
    HWs = (1, 3, 15, 16, 49, 64, 256, 720, 1024, 4096, 16384, 65536)
    for C in (1, 2, 4, 12, 24, 48, 96, 192, 512, 513):
        table = {}
        for B in Bs:
            for HW in HWs:
                n = int(L.finc_actnorm_workspace_bytes(B, C, HW))
                assert n > 0, (C, B, HW)
                assert n == int(L.finc_actnorm_workspace_bytes(B, C, HW)), (C, B, HW)
                table[B, HW] = n
        for HW in HWs:
            col = [table[B, HW] for B in Bs]
            assert col == sorted(col), ("B", C, HW, col)
        for B in Bs:
            row = [table[B, HW] for HW in HWs]
            assert row == sorted(row), ("HW", C, B, row)
    for bad in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-4, 12, 64)):
        assert int(L.finc_actnorm_workspace_bytes(*bad)) > 0


def plain_actnorm(m, x, reverse=False):
    """Today's formula (layers/actnorm.py:25-37, :51, :57-65), restated."""
    shape = (1, -1) + (1,) * (x.dim() - 2)
    t, ls = m.translation.view(shape), m.log_scale.view(shape)
    if reverse:
        return x * torch.exp(ls) + t
    pixels = int(np.prod(x.shape[2:])) if x.dim() > 2 else 1
    return (x - t) * torch.exp(-ls), -m.log_scale.sum().expand(x.size(0)) * pixels


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(6, 5, 7, 3), (4, 12, 8, 8), (3, 4, 1, 1), (7, 9)])
def test_actnorm_on_cpu_tensors_is_the_plain_formula_bit_for_bit(dtype, shape):
    from fincflow_amd import glow
    torch.manual_seed(sum(shape))
    C = shape[1]
    x = (torch.randn(shape, dtype=torch.float64) * 1.7 + 0.4).to(dtype)
    m = glow.ActNorm(C).to(dtype)
    assert not m._hip_device(x)
    assert list(m.state_dict()) == ["translation", "log_scale", "initialized"]
    # first call = the data-dependent initialisation (layers/actnorm.py:17-23)
    with torch.no_grad():
        y, ld = m(x)
    dims = [d for d in range(x.dim()) if d != 1]
    assert int(m.initialized) == 1
    assert torch.equal(m.translation.detach(), x.mean(dim=dims))
    assert torch.equal(m.log_scale.detach(), torch.log(x.std(dim=dims) + 1e-8))
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            y, ld = m(x)
            r = m.reverse(x)
            y0, ld0 = plain_actnorm(m, x)
            r0 = plain_actnorm(m, x, reverse=True)
        assert torch.equal(y, y0) and torch.equal(ld, ld0) and torch.equal(r, r0), (dtype, shape, grad)
        assert y.requires_grad == grad and ld.requires_grad == grad
    # and its gradients are autograd's through that formula
    gy = torch.randn(shape, dtype=dtype)
    gl = torch.randn(shape[0], dtype=dtype)
    xa = x.clone().requires_grad_(True)
    y, ld = m(xa)
    ((y * gy).sum() + (ld * gl).sum()).backward()
    got = [xa.grad.clone(), m.log_scale.grad.clone(), m.translation.grad.clone()]
    m.zero_grad()
    xb = x.clone().requires_grad_(True)
    y0, ld0 = plain_actnorm(m, xb)
    ((y0 * gy).sum() + (ld0 * gl).sum()).backward()
    for g, w in zip(got, [xb.grad, m.log_scale.grad, m.translation.grad]):
        assert torch.equal(g, w)
    # an `initialized` flag written directly before the first call is honoured, as is reset_initialization
    m2 = glow.ActNorm(C).to(dtype)
    m2.initialized.fill_(1)
    with torch.no_grad():
        assert torch.equal(m2(x)[0], x)
    m2.reset_initialization()
    with torch.no_grad():
        m2(x)
    assert torch.equal(m2.translation.detach(), m.translation.detach())


@pytest.mark.parametrize("name", sorted(CASES))
def test_actnorm_on_cpu_tensors_equals_the_reference_fixtures_in_float64(name):
    from fincflow_amd import glow
    g = golden(name)
    x, gy, gl = inputs(name)
    assert tuple(g["shape"]) == x.shape
    assert np.allclose(x.astype(np.float64).sum(axis=(0, 2, 3)), g["x_channel_sums"], rtol=1e-13, atol=0)
    if name != BIG:
        assert np.array_equal(x, g["x"]) and np.array_equal(gy, g["gy"])
    assert np.array_equal(gl, g["gl"])
    keep = (lambda a: a[list(BIG_IMAGES)]) if name == BIG else (lambda a: a)
    m = glow.ActNorm(x.shape[1]).double()
    x64 = torch.from_numpy(x).double()
    with torch.no_grad():
        out, ldj = m(x64)
        rev = m.reverse(out)
    leaf = x64.clone().requires_grad_(True)
    o2, l2 = m(leaf)
    ((o2 * torch.from_numpy(gy).double()).sum() + (l2 * torch.from_numpy(gl).double()).sum()).backward()
    got = dict(translation=m.translation.detach().numpy(), log_scale=m.log_scale.detach().numpy(), out=keep(out.numpy()),
               ldj=ldj.numpy(), rev=keep(rev.numpy()), grad_x=keep(leaf.grad.numpy()), grad_log_scale=m.log_scale.grad.numpy(),
               grad_translation=m.translation.grad.numpy())
    for k, v in got.items():
        assert rel_err(v, g[k]) <= 1e-12, (name, k, rel_err(v, g[k]))


def test_actnorm_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    want = {"finc_actnorm_kernel": 4, "finc_actnorm_bwd_kernel": 2, "finc_actnorm_stats_kernel": 2, "finc_actnorm_stats_final_kernel": 1,
            "finc_coupling_reduce_kernel": 1}
    for name, count in want.items():
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == count, (name, sorted(ks))
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)

