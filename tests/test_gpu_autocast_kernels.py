"""The coupling's kernels on a bfloat16 `raw` (the six finc_coupling_*_rawbf16_f32) and finc_bias_relu_bf16, without a convolution
anywhere: `raw = randn().bfloat16()` is synthetic, and the reference is the fp32 sibling fed `raw.float()`, which holds exactly the
same values (bf16 -> fp32 is exact).

Bars.  One kernel body computes both, in fp32, from the same values: every fp32 output (y, logdet, grad_x, the rebuilt x, grad_a,
grad_b) must have the sibling's BITS, and grad_raw must be the sibling's grad_raw rounded to nearest even once, which is what
`Tensor.bfloat16()` does -- bit for bit, no tolerance.  Against float64 (helpers.coupling_ref on raw.double()) y and the log-det
are held to the suite's 1e-5 (tests/test_gpu_coupling.py: TOL).  The shapes are the smallest at which the packing can go wrong: one
8-byte piece per row, HW = 12, an odd element count (narrow form; the last bf16 element ends on a 2-byte boundary), a single
element, several parts per image, and `raw` offset by 1, 2 and 3 bf16 elements (the narrow form on bf16 misalignment alone)."""
import itertools

import pytest
import torch

from helpers import coupling_ref, guarded, guards_intact, offset_view, rel_err, same_bits
from test_gpu_coupling import TOL, case

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 1, 4), (2, 6, 3, 4), (3, 4, 3, 3), (1, 2, 1, 1), (5, 8, 4, 8)]
BF16_NAN, BF16_INF = 0x7FC1, 0x7F80          # the 2-byte guard patterns: a quiet NaN that no arithmetic produces, and +Inf
GUARD16 = 4096                               # elements per guard (8 KiB: the payload keeps the alignment class of a fresh allocation)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- 2-byte guard bands (helpers.guarded knows 4- and 8-byte elements) ----
def guarded16(t, dev, lead=0, pattern=BF16_NAN):
    """(view, buffer): `t` (bfloat16) inside [front guard | lead elements | payload | back guard], everything but the payload filled
    with `pattern`.  `lead` shifts the payload by that many 2-byte elements."""
    assert t.dtype == torch.bfloat16
    n = t.numel()
    buf = torch.full((2 * GUARD16 + lead + n,), pattern, dtype=torch.int16, device=dev).view(torch.bfloat16)
    view = buf[GUARD16 + lead:GUARD16 + lead + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() - buf.data_ptr()) % 512 == 2 * lead
    return view, buf


def guards16_intact(buf, view, pattern=BF16_NAN):
    off = (view.data_ptr() - buf.data_ptr()) // 2
    ints = buf.view(torch.int16)
    return bool((ints[:off] == pattern).all()) and bool((ints[off + view.numel():] == pattern).all())


def bits16(t):
    return t.contiguous().view(torch.int16)


class Outputs:
    """Where a call's outputs go: every one between guards (fp32: helpers.guarded, bf16: guarded16), kept for `intact()`."""

    def __init__(self, dev, lead16=0):
        self.dev, self.lead16, self.kept = dev, lead16, []

    def f32(self, shape):
        view, buf = guarded(torch.zeros(shape), self.dev)
        self.kept.append((buf, view, False))
        return view

    def like_raw(self, raw):
        if raw.dtype != torch.bfloat16:
            return self.f32(raw.shape)
        view, buf = guarded16(torch.zeros(raw.shape, dtype=torch.bfloat16), self.dev, self.lead16)
        self.kept.append((buf, view, True))
        return view

    def intact(self):
        return all(guards16_intact(b, v) if half else guards_intact(b, v) for b, v, half in self.kept)


def run_six(dev, x, raw, a, b, gy, gl, outs):
    """Every coupling entry point of `raw`'s element type once, straight through the C ABI: {name: output}."""
    from fincflow_amd import _lib
    L = _lib.lib()
    B, C, H, W = x.shape
    HW = H * W
    sfx = "_rawbf16_f32" if raw.dtype == torch.bfloat16 else "_f32"
    ws = torch.empty(L.finc_coupling_workspace_bytes(B, C, HW), dtype=torch.uint8, device=dev)
    tail = (ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    res = {}

    def new(prefix, *names):
        made = []
        for n in names:
            t = (outs.like_raw(raw) if n == "graw" else outs.f32((C,)) if n in ("ga", "gb") else outs.f32((B,)) if n == "logdet"
                 else outs.f32(x.shape))
            res[prefix + n] = t
            made.append(t.data_ptr())
        return made

    def go(name, *args):
        rc = getattr(L, "finc_coupling" + name + sfx)(*args, *tail)
        assert rc == 0, (name + sfx, rc)
    p = [t.data_ptr() for t in (x, raw, a, b)]
    go("", *p, *new("fwd_", "y", "logdet"), B, C, HW, 1)
    y = res["fwd_y"]
    go("", p[0], *p[1:], *new("rev_", "y"), None, B, C, HW, -1)
    r = res["rev_y"]
    go("_reverse_logdet", *p, *new("revld_", "y", "logdet"), B, C, HW)
    go("_backward", gy.data_ptr(), gl.data_ptr(), *p, *new("bwd_", "gx", "graw", "ga", "gb"), B, C, HW)
    go("_reverse_backward", gy.data_ptr(), r.data_ptr(), *p[1:], *new("revbwd_", "gx", "graw", "ga", "gb"), B, C, HW)
    go("_reverse_logdet_backward", gy.data_ptr(), gl.data_ptr(), r.data_ptr(), *p[1:], *new("revldbwd_", "gx", "graw", "ga", "gb"), B, C, HW)
    go("_backward_reconstruct", gy.data_ptr(), gl.data_ptr(), y.data_ptr(), *p[1:], *new("recon_", "x", "gx", "graw", "ga", "gb"), B, C, HW)
    torch.cuda.synchronize()
    return res


def compare(got, want, tag):
    """`got` from a bf16 raw against `want` from the fp32 sibling on the same values."""
    assert sorted(got) == sorted(want)
    for k in got:
        if k.endswith("graw"):
            assert got[k].dtype == torch.bfloat16 and want[k].dtype == torch.float32
            assert torch.equal(bits16(got[k]), bits16(want[k].bfloat16())), (tag, k)
        else:
            assert same_bits(got[k], want[k]), (tag, k)


def device_case(shape, dev):
    x, raw, a, b, gy, gl = case(shape)
    raw16 = raw.bfloat16()
    return [t.to(dev) for t in (x, raw16.float(), a, b, gy, gl)], raw16


@pytest.mark.parametrize("shape", SHAPES)
def test_six_entry_points_have_the_siblings_bits_between_guards(shape, dev):
    (x, raw32, a, b, gy, gl), raw16 = device_case(shape, dev)
    want = run_six(dev, x, raw32, a, b, gy, gl, Outputs(dev))
    outs = Outputs(dev)
    rawd, rawbuf = guarded16(raw16, dev)
    got = run_six(dev, x, rawd, a, b, gy, gl, outs)
    compare(got, want, shape)
    assert outs.intact() and guards16_intact(rawbuf, rawd), shape
    assert torch.equal(bits16(rawd), bits16(raw16.to(dev)))                  # the input is untouched
    # against float64 on the same bf16 values
    d = lambda t: t.double().cpu()
    y_ref, ld_ref = coupling_ref(d(x), raw16.double(), d(a), d(b), 1)
    r_ref, _ = coupling_ref(d(x), raw16.double(), d(a), d(b), -1)
    errs = {"y": rel_err(got["fwd_y"].cpu().numpy(), y_ref.numpy()), "logdet": rel_err(got["fwd_logdet"].cpu().numpy(), ld_ref.numpy()),
            "reverse": rel_err(got["rev_y"].cpu().numpy(), r_ref.numpy()),
            "reverse_logdet": rel_err(got["revld_logdet"].cpu().numpy(), coupling_ref(r_ref, raw16.double(), d(a), d(b), 1)[1].numpy())}
    print(shape, errs)
    for n, e in errs.items():
        assert e <= TOL, (shape, n, e)
    # nothing is read beyond a tensor: Inf in raw's guards changes no output
    rawp, rawpbuf = guarded16(raw16, dev, pattern=BF16_INF)
    again = run_six(dev, x, rawp, a, b, gy, gl, Outputs(dev))
    for k in got:
        assert torch.equal(got[k].view(torch.int16 if got[k].dtype == torch.bfloat16 else torch.int32),
                           again[k].view(torch.int16 if again[k].dtype == torch.bfloat16 else torch.int32)), (shape, k)
    assert guards16_intact(rawpbuf, rawp, BF16_INF)


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_raw_offset_by_bf16_elements_takes_the_narrow_form_with_the_same_bits(lead, dev):
    """x and every fp32 pointer 16-byte aligned, HW % 4 == 0: only raw's (and grad_raw's) address keeps the call off the wide form.
    The sibling it is compared with is in the narrow form for the same reason (its fp32 raw one float off 16 bytes): the two forms
    add their partial sums in different orders, in fp32 as in bf16."""
    shape = (2, 4, 8, 8)
    (x, raw32, a, b, gy, gl), raw16 = device_case(shape, dev)
    want = run_six(dev, x, offset_view(raw32, dev), a, b, gy, gl, Outputs(dev))
    outs = Outputs(dev, lead16=lead)
    rawd, rawbuf = guarded16(raw16, dev, lead)
    assert rawd.data_ptr() % 8 == (2 * lead) % 8 and x.data_ptr() % 16 == 0
    got = run_six(dev, x, rawd, a, b, gy, gl, outs)
    compare(got, want, lead)
    assert outs.intact() and guards16_intact(rawbuf, rawd), lead
    # and the aligned call (wide form) against the aligned sibling
    compare(run_six(dev, x, raw16.to(dev), a, b, gy, gl, Outputs(dev)), run_six(dev, x, raw32, a, b, gy, gl, Outputs(dev)), "aligned")


ENTRIES = [("_backward", ("gx", "graw", "ga", "gb"), "fwd_in"), ("_reverse_logdet_backward", ("gx", "graw", "ga", "gb"), "rev_out"),
           ("_backward_reconstruct", ("x", "gx", "graw", "ga", "gb"), "fwd_out")]


@pytest.mark.parametrize("entry,names,reads", ENTRIES)
def test_every_combination_of_skipped_outputs(entry, names, reads, dev):
    """A skipped output is NULL, a buffer that was not passed is not written, and the outputs that are asked for have the bits of
    the call that asks for all of them."""
    from fincflow_amd import _lib, ops
    shape = (2, 6, 3, 4)
    B, C, H, W = shape
    (x, raw32, a, b, gy, gl), raw16 = device_case(shape, dev)
    raw = raw16.to(dev)
    v = {"fwd_in": x, "rev_out": ops.finc_coupling(x, raw, a, b, -1)[0], "fwd_out": ops.finc_coupling(x, raw, a, b, 1)[0]}[reads]
    L = _lib.lib()
    fn = getattr(L, "finc_coupling" + entry + "_rawbf16_f32")
    ws = torch.empty(L.finc_coupling_workspace_bytes(B, C, H * W), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(want):
        bufs = [torch.full_like(raw, 7.0) if n == "graw" else torch.full((C,), 7.0, device=dev) if n in ("ga", "gb") else torch.full_like(x, 7.0)
                for n in names]
        rc = fn(gy.data_ptr(), gl.data_ptr(), v.data_ptr(), raw.data_ptr(), a.data_ptr(), b.data_ptr(),
                *[t.data_ptr() if w else None for t, w in zip(bufs, want)], B, C, H * W, ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        return rc, bufs
    rc, full = call((True,) * len(names))
    assert rc == 0 and full[names.index("graw")].dtype == torch.bfloat16
    for want in itertools.product((False, True), repeat=len(names)):
        rc, bufs = call(want)
        if not any(want):
            assert rc == 1
            continue
        assert rc == 0, (want, rc)
        for t, w, f in zip(bufs, want, full):
            assert torch.equal(t, f) if w else bool((t == 7.0).all()), want


def test_ops_pick_the_entry_point_by_raws_dtype_and_refuse_float16(dev, monkeypatch):
    from fincflow_amd import ops
    (x, raw32, a, b, gy, gl), raw16 = device_case((2, 6, 3, 4), dev)
    names = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *args, **kw: (names.append(name), real(name, *args, **kw))[1])

    def every(raw):
        del names[:]
        y, _ = ops.finc_coupling(x, raw, a, b, 1, True)
        r, _ = ops.finc_coupling_reverse_logdet(x, raw, a, b)
        g = [ops.finc_coupling_backward(gy, gl, x, raw, a, b), ops.finc_coupling_reverse_backward(gy, r, raw, a, b),
             ops.finc_coupling_reverse_logdet_backward(gy, gl, r, raw, a, b), ops.finc_coupling_backward_reconstruct(gy, gl, y, raw, a, b)]
        return list(names), g
    base = ["finc_coupling", "finc_coupling_reverse_logdet", "finc_coupling_backward", "finc_coupling_reverse_backward",
            "finc_coupling_reverse_logdet_backward", "finc_coupling_backward_reconstruct"]
    called, g = every(raw32)
    assert called == [n + "_f32" for n in base]                              # an fp32 raw still takes the fp32 entry points
    assert all(t[-3].dtype == torch.float32 for t in g)
    called, g = every(raw16.to(dev))
    assert called == [n + "_rawbf16_f32" for n in base]
    for t in g:
        assert t[-3].dtype == torch.bfloat16 and all(o.dtype == torch.float32 for o in t[:-3] + t[-2:])
    # under autograd: the gradient of a bf16 raw is bf16
    leaves = [t.clone().requires_grad_(True) for t in (x, raw16.to(dev), a, b)]
    y, ld = ops.coupling_forward(*leaves)
    ((y * gy).sum() + (ld * gl).sum()).backward()
    assert leaves[1].grad.dtype == torch.bfloat16 and torch.equal(bits16(leaves[1].grad), bits16(g[0][1]))
    assert same_bits(leaves[0].grad, g[0][0])
    for bad in (raw32.half(), raw32.double()):
        with pytest.raises(ValueError, match="raw must be"):
            ops.finc_coupling(x, bad, a, b, 1, True)
    with pytest.raises(ValueError):
        ops.finc_bias_relu(raw32.half(), a)
    with pytest.raises(ValueError):
        ops.finc_bias_relu(raw16.to(dev), a, out=torch.empty_like(raw32))    # `out` must match


@pytest.mark.parametrize("shape,lead", [((2, 3, 1, 8), 0), ((2, 3, 3, 3), 0), ((1, 1, 1, 1), 0), ((2, 5, 4, 6), 0), ((2, 3, 1, 8), 1), ((2, 5, 4, 6), 1)])
def test_bias_relu_on_bf16_is_the_fp32_formula_rounded_once(shape, lead, dev):
    from fincflow_amd import ops
    torch.manual_seed(sum(shape))
    x = torch.randn(shape).bfloat16()
    bias = 0.3 * torch.randn(shape[1])
    want = torch.relu(x.float() + bias.view(1, -1, 1, 1)).bfloat16()
    bd = bias.to(dev)
    xd, xbuf = guarded16(x, dev, lead)
    od, obuf = guarded16(torch.zeros(shape, dtype=torch.bfloat16), dev, lead)
    out = ops.finc_bias_relu(xd, bd, out=od)                                 # out of place
    torch.cuda.synchronize()
    assert out is od and out.dtype == torch.bfloat16
    assert torch.equal(bits16(od).cpu(), bits16(want)) and torch.equal(bits16(xd).cpu(), bits16(x))
    assert guards16_intact(xbuf, xd) and guards16_intact(obuf, od)
    assert torch.equal(bits16(ops.finc_bias_relu(xd, bd)).cpu(), bits16(want))   # an output of its own
    got = ops.finc_bias_relu(xd, bd, out=xd)                                 # in place
    torch.cuda.synchronize()
    assert got is xd and torch.equal(bits16(xd).cpu(), bits16(want)) and guards16_intact(xbuf, xd)
    if x.numel() > 1:
        assert bool((want == 0).any()) and bool((want > 0).any())
    # a NaN stays a NaN, and nothing else moves
    xn = x.clone()
    xn.view(-1)[-1] = float("nan")
    nd, nbuf = guarded16(xn, dev, lead)
    res = ops.finc_bias_relu(nd, bd).cpu()
    assert bool(torch.isnan(res.view(-1)[-1])) and torch.equal(bits16(res).view(-1)[:-1], bits16(want).view(-1)[:-1])
    assert guards16_intact(nbuf, nd)
