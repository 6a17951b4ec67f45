"""Host side of the bfloat16 entry points (the six finc_coupling_*_rawbf16_f32 and finc_bias_relu_bf16; include/finc.h): the exported
symbols and the ABI version gate, the refusal order of each entry point with fake pointers -- the order of its _f32 sibling
(tests/test_coupling_host.py), with the 2-byte alignment rule of the bf16 pointers -- and a CPU Coupling under CPU autocast, which
stays on the PyTorch lines and returns fp32.  No GPU needed, the library built."""
import os

import pytest
import torch

from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("finc_coupling_rawbf16_f32", "finc_coupling_backward_rawbf16_f32", "finc_coupling_reverse_backward_rawbf16_f32",
               "finc_coupling_reverse_logdet_rawbf16_f32", "finc_coupling_reverse_logdet_backward_rawbf16_f32",
               "finc_coupling_backward_reconstruct_rawbf16_f32", "finc_bias_relu_bf16")
BIG = 1 << 40


def test_the_seven_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    # each takes the argument list of its _f32 sibling
    for name in NEW_SYMBOLS[:-1]:
        assert len(getattr(L, name).argtypes) == len(getattr(L, name.replace("_rawbf16", "")).argtypes), name
    assert len(L.finc_bias_relu_bf16.argtypes) == len(L.finc_bias_relu_f32.argtypes)


def test_version_is_113_and_a_112_library_is_told_to_rebuild(tmp_path):
    assert _lib.AUTOCAST_ABI_VERSION == 113
    assert _lib.lib().finc_version() >= _lib.AUTOCAST_ABI_VERSION
    out = load_stub_library(tmp_path, 112)
    assert "= 112" in out and "113" in out and "rebuild it" in out and "finc_bias_relu_bf16" in out, out


@pytest.mark.parametrize("entry", ["finc_coupling_rawbf16_f32", "finc_coupling_reverse_logdet_rawbf16_f32"])
def test_transform_refusal_order(entry):
    """NULL -> 1, bad dims / direction / y == raw -> 2, alignment (4 bytes, 2 for raw) -> 7, odd C -> 3, workspace -> 4, in that order."""
    L = _lib.lib()
    x, raw, a, b, y, ld, ws = _p(0x1000), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000), _p(0x6000), _p(0x10000)
    takes_direction = entry == "finc_coupling_rawbf16_f32"
    fn = getattr(L, entry)

    def f(x, raw, a, b, y, ld, B, C, HW, ws, nbytes, direction=1):
        return fn(x, raw, a, b, y, ld, B, C, HW, *((direction,) if takes_direction else ()), ws, nbytes, None)
    for k in range(5):                                                       # each required pointer
        args = [x, raw, a, b, y]
        args[k] = None
        assert f(*args, ld, 2, 12, 64, ws, BIG) == 1, k
    if not takes_direction:
        assert f(x, raw, a, b, y, None, 2, 12, 64, ws, BIG) == 1                 # this one always reports the log-det
    assert f(None, raw, a, b, y, ld, 0, 12, 64, ws, BIG) == 1                    # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64)):
        assert f(x, raw, a, b, y, ld, B, C, HW, ws, BIG) == 2, (B, C, HW)
    if takes_direction:
        for d in (0, 2, -2):
            assert f(x, raw, a, b, y, ld, 2, 12, 64, ws, BIG, d) == 2, d
    assert f(x, raw, a, b, raw, ld, 2, 12, 64, ws, BIG) == 2                     # y == raw, as the sibling forbids it
    assert f(x, _p(0x2001), a, b, y, ld, 0, 12, 64, ws, BIG) == 2                # (dims come before the alignment)
    assert f(x, _p(0x2001), a, b, y, ld, 2, 12, 64, ws, BIG) == 7                # a bf16 pointer on an odd address
    assert f(_p(0x1002), raw, a, b, y, ld, 2, 12, 64, ws, BIG) == 7              # an fp32 pointer is still held to 4 bytes
    assert f(x, raw, a, b, _p(0x5002), ld, 2, 12, 64, ws, BIG) == 7
    assert f(x, _p(0x2001), a, b, y, ld, 2, 13, 64, ws, BIG) == 7                # (alignment comes before the channel count)
    for C in (13, 7, 1):
        assert f(x, raw, a, b, y, ld, 2, C, 64, ws, BIG) == 3, C
        assert f(x, raw, a, b, y, ld, 2, C, 64, None, 0) == 3, C                 # (... before the workspace)
    # raw on 2 bytes but not on 4 gets past the alignment rule: the next refusal is the workspace's
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(x, _p(0x2002), a, b, y, ld, 2, 12, 64, None, BIG) == 4
    assert f(x, raw, a, b, y, ld, 2, 12, 64, ws, need - 1) == 4
    assert f(x, raw, a, b, y, ld, 2, 12, 64, ws, 0) == 4


BACKWARDS = {   # entry -> (takes grad_logdet, writes x_out)
    "finc_coupling_backward_rawbf16_f32": (True, False),
    "finc_coupling_reverse_backward_rawbf16_f32": (False, False),
    "finc_coupling_reverse_logdet_backward_rawbf16_f32": (True, False),
    "finc_coupling_backward_reconstruct_rawbf16_f32": (True, True),
}


@pytest.mark.parametrize("entry", sorted(BACKWARDS))
def test_backward_refusal_order(entry):
    L = _lib.lib()
    takes_gl, rebuilds = BACKWARDS[entry]
    gy, gl, v, raw, a, b = _p(0x1000), _p(0x1800), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000)
    xo, gx, gr, ga, gb, ws = _p(0x5800), _p(0x6000), _p(0x7000), _p(0x8000), _p(0x9000), _p(0x10000)
    fn = getattr(L, entry)

    def f(gy=gy, gl=gl, v=v, raw=raw, a=a, b=b, xo=xo, gx=gx, gr=gr, ga=ga, gb=gb, dims=(2, 12, 64), ws=ws, nbytes=BIG):
        args = [gy] + ([gl] if takes_gl else []) + [v, raw, a, b] + ([xo] if rebuilds else []) + [gx, gr, ga, gb]
        return fn(*args, *dims, ws, nbytes, None)
    for name in ("gy", "v", "raw", "a", "b"):                                # required; grad_logdet is not
        assert f(**{name: None}) == 1, name
    assert f(xo=None, gx=None, gr=None, ga=None, gb=None) == 1                   # nothing asked for
    assert f(gy=None, dims=(0, 12, 64)) == 1                                     # (NULL comes before the dims)
    for dims in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 1 << 20, 64)):
        assert f(dims=dims) == 2, dims
    for alias in (v, raw) + (() if rebuilds else (gy,)):
        assert f(gx=alias) == 2                                                  # grad_x on an input
    for alias in (gy, v, raw, gx):
        assert f(gr=alias) == 2                                                  # grad_raw on an input or on grad_x
    if rebuilds:
        for alias in (gy, raw, gx, gr):
            assert f(xo=alias) == 2
    assert f(raw=_p(0x3001), dims=(0, 12, 64)) == 2                              # (dims come before the alignment)
    assert f(raw=_p(0x3001)) == 7                                                # a bf16 pointer on an odd address
    assert f(gr=_p(0x7001)) == 7
    assert f(gy=_p(0x1002)) == 7                                                 # an fp32 pointer is still held to 4 bytes
    assert f(ga=_p(0x8003)) == 7
    if takes_gl:
        assert f(gl=_p(0x1801)) == 7
    assert f(raw=_p(0x3001), dims=(2, 13, 64)) == 7                              # (alignment before the channel count)
    for C in (13, 7):
        assert f(dims=(2, C, 64)) == 3
        assert f(dims=(2, C, 64), ws=None, nbytes=0) == 3                        # (... before the workspace)
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(raw=_p(0x3002), gr=_p(0x7002), ws=None) == 4                        # 2-byte aligned bf16 pointers pass the alignment rule
    assert f(nbytes=need - 1) == 4
    assert f(xo=None, gx=None, gr=None, gb=None, nbytes=0) == 4
    assert f(xo=None, gx=None, gr=None, ga=None, ws=None, nbytes=0) == 4


def test_bias_relu_bf16_refusal_order():
    L = _lib.lib()
    i, b, o = _p(0x1000), _p(0x2000), _p(0x3000)
    f = L.finc_bias_relu_bf16
    assert f(None, b, o, 2, 512, 64, None) == 1
    assert f(i, None, o, 2, 512, 64, None) == 1
    assert f(i, b, None, 2, 512, 64, None) == 1
    assert f(None, b, o, 0, 512, 64, None) == 1
    for B, C, HW in ((0, 512, 64), (2, 0, 64), (2, 512, 0), (-1, 512, 64), (1 << 20, 1 << 20, 1 << 10)):
        assert f(i, b, o, B, C, HW, None) == 2, (B, C, HW)
    assert f(_p(0x1001), b, o, 0, 512, 64, None) == 2
    assert f(_p(0x1001), b, o, 2, 512, 64, None) == 7                            # bf16 pointers: 2 bytes
    assert f(i, b, _p(0x3003), 2, 512, 64, None) == 7
    assert f(i, _p(0x2002), o, 2, 512, 64, None) == 7                            # the bias is fp32: 4 bytes


def _fill(m):
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if name.endswith(("bias", "logs")) else 0.05))
    return m


@pytest.mark.parametrize("n_context", [None, 3])
def test_a_cpu_coupling_under_cpu_autocast_returns_fp32_through_the_pytorch_lines(n_context):
    from fincflow_amd import glow
    torch.manual_seed(3)
    m = _fill(glow.Coupling((12, 6, 5), width=16, n_context=n_context))
    x = torch.randn(3, 12, 6, 5)
    ctx = None if n_context is None else torch.randn(3, n_context, 6, 5)
    with torch.no_grad():
        y32, ld32 = m(x, ctx)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not m._hip(x, ctx) and not m._hip_train(x, ctx)
        with torch.no_grad():
            assert m._raw_train(x, ctx).dtype == torch.bfloat16              # the net did run in the autocast dtype
            y, ld = m(x, ctx)
            r = m.reverse(y, ctx)
            r2, ld2 = m.reverse_with_logdet(y, ctx)
    with torch.autocast("cpu", dtype=torch.bfloat16):                        # (a context of its own: autocast keeps the weights it cast
        xa = x.clone().requires_grad_(True)                                  # under no_grad, without a graph, until the context ends)
        yt, ldt = m(xa, ctx)
    for t in (y, ld, r, r2, ld2, yt, ldt):
        assert t.dtype == torch.float32
    assert torch.equal(y[:, :6], x[:, :6]) and torch.equal(r, r2) and torch.equal(ld, ld2)
    # the net sees the untouched half only: reverse undoes forward with the same bf16 raw, to fp32 rounding
    assert float((r - x).abs().max()) <= 1e-5 * float(x.abs().max())
    # and the bf16 net is the fp32 net to bf16 precision (8 bits: 2^-8 per rounding, a handful of roundings, |h| and |x| of order 1)
    assert float((y - y32).abs().max()) <= 2.0 ** -4 and float((ld - ld32).abs().max()) <= 2.0 ** -4 * y[0, 6:].numel()
    (yt.square().sum() + ldt.sum()).backward()
    assert xa.grad.dtype == torch.float32 and bool(torch.isfinite(xa.grad).all())
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
