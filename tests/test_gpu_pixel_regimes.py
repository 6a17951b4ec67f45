"""The per-pixel layers and the mix in their multi-trip launch regimes, through the C ABI (include/finc.h).

Every case of tests/pixel_regime_cases.py -- a shape at which a thread of the grid-stride or (outer, part) kernels, or a wave of the
mix, takes more than one trip through its loop, plus the 8-byte alignment class of the mix and of F(2,5) -- on every entry point
listed for it:

  1. the library's own plan (`_lib.pixel_plan`) at the alignment the pointers of the call REALLY had is the hand-stated plan, in
     particular its trip count: a later rule change cannot silently turn the case into a one-trip test;
  2. guard bands (test_gpu_bounds.check_bounds): every tensor between NaN guards, outputs and an exact-size workspace NaN on entry;
     guards intact, no NaN left, bit-stable over two launches, the documented in-place form with the same bits;
  3. float64 on the CPU (helpers.coupling_ref / actnorm_ref, the einsums, autograd through them; the mix from 96 channels on torch's
     float64 einsum on the device) at the families' bar, TOL = 1e-5 on helpers.rel_err.  A bfloat16 output is held to the bar of
     tests/test_gpu_autocast_kernels.py instead -- the bits of the fp32 result rounded once -- and its float64 error to the format's
     unit roundoff, 2^-8;
  4. the element-wise outputs of the whole-tensor call are bit-equal to the same entry point on sub-batches that take ONE trip each
     (an element depends on its own inputs and its channel's parameters only): no tolerance, any index error shows.  Sums depend on
     P / Q and are held to float64 only; for the mix the comparison is recorded, not asserted (a sub-batch may take another form);
  5. isolation: one element reached on the LAST trip (the first item only the last trip reaches, and the very last item) is NaN; the
     NaN appears where the operation's definition sends it and nowhere else.

One report line per (case, entry) with the achieved errors (kind `pixel_regime`).  References: layers/{coupling,actnorm,conv1x1}.py.
"""
import zlib

import numpy as np
import pytest
import torch

from helpers import actnorm_ref, coupling_ref, rel_err, report, same_bits
from pixel_regime_cases import (MIX_CASES, PART_CASES, PIXEL_REGIME_CASES, ROW_CASES, WINO5_ALIGN8_CASES, last_trip_item, multi_trip)
from test_gpu_bounds import F32, INF, NAN, TOL, Unit, check_bounds, check_isolation, conv_reference, grads, run, t as to_dev

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
BF16_HALF_ULP = 2.0 ** -8           # round to nearest on 8 significant bits: half a unit in the last place is at most 2^-8 |value|


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def alignment_class(ptr):
    return 16 if ptr % 16 == 0 else 8 if ptr % 8 == 0 else 4


def bits16(v):
    return v.contiguous().view(torch.int16)


class Inputs:
    """Deterministic N(0,1) tensors by name, made when first asked for (a case needs two or three of them)."""

    def __init__(self, case_name):
        self.case_name, self.made = case_name, {}

    def __call__(self, name, *shape):
        if name not in self.made:
            g = torch.Generator().manual_seed(zlib.crc32(("%s.%s" % (self.case_name, name)).encode()))
            self.made[name] = torch.randn(*shape, generator=g)
        return self.made[name]


class Spec:
    """One entry point on one case: how to call it on the first `b` images, what it reads and writes, what is true of the result."""
    values = (NAN,)
    alias = None
    ws = staticmethod(lambda b: None)
    bf16_outs = ()


def plan_of(case, b, align=None):
    """The library's plan for the case's entry-point family on the first b images (b elements for the negate)."""
    from fincflow_amd import _lib
    B, C, H, W = case["shape"]
    if case["family"] == "negate":
        return _lib.pixel_plan("rows", "negate", 1, 1, b, align or case["align"], case["elem"])
    return _lib.pixel_plan(case["rule"], case["family"], b, C, H * W, align or case["align"], case["elem"], case["groups"])


def one_trip_batch(case):
    """The largest batch, by halving, whose plan takes one trip."""
    b = case["shape"][3] if case["family"] == "negate" else case["shape"][0]
    while plan_of(case, b)["trips"] > 1:
        b = (b + 1) // 2
    return b


def pix(p, W):
    return divmod(int(p), W)


def last_trip_spots(case):
    """Two item indices (chunk indices for the mix) that only the LAST trip reaches: the first such item and the very last one."""
    p = case["plan"]
    first = last_trip_item(case) if multi_trip(case) else 0
    assert 0 <= first < p["items"]
    return list(dict.fromkeys((first, p["items"] - 1)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------------
def build(entry, name, case, dev, sibling=False):
    """`sibling`: the fp32 entry point fed the bf16 case's raw as floats (the reference of the bf16 call's bits)."""
    from fincflow_amd import _lib
    L = _lib.lib()
    B, C, H, W = shape = case["shape"]
    HW, half, io = H * W, C // 2, case["plan"]["io"]
    nv = HW // io
    bf16 = case["elem"] == 2 and not sibling
    R = Inputs(name)
    s = Spec()
    s.entry, s.shape = entry, shape
    dd = lambda v: v.double()
    D = lambda v: v.to(dev)
    sh = lambda b: (b, C, H, W)
    par = lambda v: v.view(1, -1, 1, 1)

    if entry in ("actnorm", "actnorm_no_logdet", "actnorm_reverse"):
        direction, logdet = (-1 if entry == "actnorm_reverse" else 1), entry == "actnorm"
        x, ls, tr = R("x", *shape), 0.2 * R("ls", C), R("tr", C)
        s.sym, s.ins, s.batched, s.acts, s.alias = "finc_actnorm_f32", dict(x=D(x), ls=D(ls), tr=D(tr)), ("x",), ("x", "y"), dict(y="x")
        s.outs = lambda b: dict(y=(sh(b), F32), **(dict(logdet=((b,), F32)) if logdet else {}))
        s.argf = lambda b: (lambda p, w, n: (p["x"], p["ls"], p["tr"], p["y"], p.get("logdet"), b, C, HW, direction, None))
        y, ld = actnorm_ref(dd(x), dd(ls), dd(tr), direction)
        s.refs = dict(y=y.numpy(), **(dict(logdet=ld.numpy()) if logdet else {}))
        s.elementwise = ("y",)

        def spot(i, last):
            idx = np.unravel_index((i // nv) * HW + (i % nv) * io + (io - 1 if last else 0), shape)
            idx = tuple(int(v) for v in idx)
            return ("x", idx, dict(y=idx, **(dict(logdet=None) if logdet else {})))
    elif entry in ("bias_relu", "bias_relu_bf16"):
        x, bias = R("x", *shape), R("bias", C)
        if entry == "bias_relu_bf16":
            x = x.bfloat16()
            s.bf16_outs = ("out",)
            s.exact = dict(out=torch.relu(x.float() + par(bias)).bfloat16())          # the fp32 formula rounded once
        s.sym = "finc_bias_relu_bf16" if entry == "bias_relu_bf16" else "finc_bias_relu_f32"
        s.ins, s.batched, s.acts, s.alias = dict(x=D(x), bias=D(bias)), ("x",), ("x", "out"), dict(out="x")
        s.outs = lambda b: dict(out=(sh(b), x.dtype))
        s.argf = lambda b: (lambda p, w, n: (p["x"], p["bias"], p["out"], b, C, HW, None))
        s.refs = dict(out=torch.relu(dd(x) + par(dd(bias))).numpy())
        s.elementwise, s.values = ("out",), (INF,)                     # max(NaN + b, 0) is 0 on the hardware: +inf is the poison

        def spot(i, last):
            idx = tuple(int(v) for v in np.unravel_index((i // nv) * HW + (i % nv) * io + (io - 1 if last else 0), shape))
            return ("x", idx, dict(out=idx))
    elif entry == "lead_product":
        G = case["groups"]
        Cq = C // G
        v = R("v", *shape)
        blocks = torch.triu(0.3 * R("lead", G, Cq, Cq), 1) + torch.eye(Cq)            # unit upper triangular: row r reads channels o >= r
        lead_t = torch.block_diag(*blocks)
        s.sym, s.ins, s.batched, s.acts, s.alias = "finc_lead_product_f32", dict(v=D(v), lead_t=D(lead_t)), ("v",), ("v",), dict(out="v")
        s.outs = lambda b: dict(out=(sh(b), F32))
        s.argf = lambda b: (lambda p, w, n: (p["v"], p["lead_t"], b, G, Cq, HW, None))
        s.refs = dict(out=torch.einsum("gro,bgop->bgrp", dd(blocks), dd(v).view(B, G, Cq, HW)).reshape(shape).numpy())
        s.elementwise, s.always_in_place = ("out",), True

        def spot(i, last):
            bg, (h, w) = i // nv, pix((i % nv) * io + (io - 1 if last else 0), W)
            b, g = bg // G, bg % G
            return ("v", (b, g * Cq + Cq - 1, h, w), dict(out=(b, slice(g * Cq, (g + 1) * Cq), h, w)))
    elif entry == "negate":
        n = W
        p0 = R("p", n)
        s.sym, s.ins, s.batched, s.acts, s.alias = "finc_negate_f32", dict(p=D(p0)), ("p",), ("p",), dict(out="p")
        s.outs = lambda b: dict(out=((b,), F32))
        s.argf = lambda b: (lambda p, w, m: (p["p"], b, None))
        s.refs = dict(out=(-dd(p0)).numpy())
        s.elementwise, s.always_in_place = ("out",), True
        spot = lambda i, last: ("p", (int(i),), dict(out=(int(i),)))
    elif entry in ("coupling", "coupling_no_logdet", "coupling_reverse", "coupling_reverse_logdet"):
        direction = 1 if entry in ("coupling", "coupling_no_logdet") else -1
        logdet = entry in ("coupling", "coupling_reverse_logdet")
        x, raw = R("x", *shape), 1.5 * R("raw", *shape)
        logs = 0.1 * R("logs", C)
        a = torch.exp(3.0 * dd(logs)).float()
        bb = (0.3 * dd(R("b", C)) * dd(a)).float()
        if case["elem"] == 2:
            raw = raw.bfloat16()
            raw = raw.float() if sibling else raw
        base = "finc_coupling_reverse_logdet" if entry == "coupling_reverse_logdet" else "finc_coupling"
        s.sym = base + ("_rawbf16_f32" if bf16 else "_f32")
        s.ins, s.batched, s.acts, s.alias = dict(x=D(x), raw=D(raw), a=D(a), b=D(bb)), ("x", "raw"), ("x", "raw", "y"), dict(y="x")
        s.outs = lambda b: dict(y=(sh(b), F32), **(dict(logdet=((b,), F32)) if logdet else {}))
        s.ws = lambda b: L.finc_coupling_workspace_bytes(b, C, HW) if logdet else None
        if entry == "coupling_reverse_logdet":
            s.argf = lambda b: (lambda p, w, n: (p["x"], p["raw"], p["a"], p["b"], p["y"], p["logdet"], b, C, HW, w, n, None))
        else:
            s.argf = lambda b: (lambda p, w, n: (p["x"], p["raw"], p["a"], p["b"], p["y"], p.get("logdet"), b, C, HW, direction, w, n, None))
        y = coupling_ref(dd(x), dd(raw), dd(a), dd(bb), direction)[0]
        s.refs = dict(y=y.numpy(), **(dict(logdet=coupling_ref(dd(x), dd(raw), dd(a), dd(bb), 1)[1].numpy()) if logdet else {}))
        s.elementwise = ("y",)

        def spot(i, last):
            j, (h, w) = i // nv, pix((i % nv) * io + (io - 1 if last else 0), W)
            return ("raw", (B - 1, 2 * j, h, w), dict(y=(B - 1, half + j, h, w), **(dict(logdet=(B - 1,)) if logdet else {})))
    elif entry in ("coupling_backward", "coupling_reverse_backward", "coupling_reverse_logdet_backward", "coupling_backward_reconstruct"):
        x, raw, gy, gl = R("x", *shape), 1.5 * R("raw", *shape), R("gy", *shape), R("gl", B)
        logs = 0.1 * R("logs", C)
        a = torch.exp(3.0 * dd(logs)).float()
        bb = (0.3 * dd(R("b", C)) * dd(a)).float()
        if case["elem"] == 2:
            raw = raw.bfloat16()
            raw = raw.float() if sibling else raw
        rdt = BF16 if bf16 else F32
        s.bf16_outs = ("graw",) if bf16 else ()
        s.sym = "finc_" + entry + ("_rawbf16_f32" if bf16 else "_f32")
        s.ws = lambda b: L.finc_coupling_workspace_bytes(b, C, HW)
        outs = dict(gx=F32, graw=rdt, ga=F32, gb=F32)
        fwd = lambda x_, r_, a_, b_: coupling_ref(x_, r_, a_, b_, 1)
        rev = lambda x_, r_, a_, b_: coupling_ref(x_, r_, a_, b_, -1)[0]
        leaves = lambda v: [v.clone(), dd(raw), dd(a), dd(bb)]        # (grads() marks its leaves in place)
        if entry == "coupling_backward":
            s.ins, s.batched, s.acts = dict(gy=D(gy), gl=D(gl), x=D(x), raw=D(raw), a=D(a), b=D(bb)), ("gy", "gl", "x", "raw"), ("gy", "x", "raw", "gx", "graw")
            s.argf = lambda b: (lambda p, w, n: (p["gy"], p["gl"], p["x"], p["raw"], p["a"], p["b"], p["gx"], p["graw"], p["ga"], p["gb"], b, C, HW, w, n, None))
            g = grads(fwd, leaves(dd(x)), [gy, gl])
        elif entry == "coupling_backward_reconstruct":
            # handed the forward's OUTPUT as the fp32 tensor it is; the input that output belongs to, in float64, is the reference
            y32 = coupling_ref(x, raw.float(), a, bb, 1)[0].contiguous()
            xin = rev(dd(y32), dd(raw), dd(a), dd(bb))
            s.ins, s.batched = dict(gy=D(gy), gl=D(gl), y=D(y32), raw=D(raw), a=D(a), b=D(bb)), ("gy", "gl", "y", "raw")
            s.acts = ("gy", "y", "raw", "xo", "gx", "graw")
            outs = dict(xo=F32, **outs)
            s.argf = lambda b: (lambda p, w, n: (p["gy"], p["gl"], p["y"], p["raw"], p["a"], p["b"], p["xo"], p["gx"], p["graw"], p["ga"], p["gb"], b, C, HW, w, n, None))
            g = grads(fwd, leaves(xin), [gy, gl])
        else:
            # the reverse direction, handed its OUTPUT y; the reverse's input that output belongs to is forward(y) in float64
            with_ld = entry == "coupling_reverse_logdet_backward"
            y32 = coupling_ref(x, raw.float(), a, bb, -1)[0].contiguous()
            xin = fwd(dd(y32), dd(raw), dd(a), dd(bb))[0]
            s.ins = dict(gy=D(gy), **(dict(gl=D(gl)) if with_ld else {}), y=D(y32), raw=D(raw), a=D(a), b=D(bb))
            s.batched, s.acts = ("gy", "gl", "y", "raw"), ("gy", "y", "raw", "gx", "graw")
            if with_ld:
                s.argf = lambda b: (lambda p, w, n: (p["gy"], p["gl"], p["y"], p["raw"], p["a"], p["b"], p["gx"], p["graw"], p["ga"], p["gb"], b, C, HW, w, n, None))
                g = grads(lambda x_, r_, a_, b_: (rev(x_, r_, a_, b_), fwd(x_, r_, a_, b_)[1]), leaves(xin), [gy, gl])
            else:
                s.argf = lambda b: (lambda p, w, n: (p["gy"], p["y"], p["raw"], p["a"], p["b"], p["gx"], p["graw"], p["ga"], p["gb"], b, C, HW, w, n, None))
                g = grads(lambda x_, r_, a_, b_: (rev(x_, r_, a_, b_),), leaves(xin), [gy])
        s.outs = lambda b: {k: (((C,) if k in ("ga", "gb") else sh(b)), dt) for k, dt in outs.items()}
        s.refs = dict(zip(("gx", "graw", "ga", "gb"), g))
        if entry == "coupling_backward_reconstruct":
            s.refs["xo"] = xin.numpy()
        s.elementwise = tuple(k for k in ("xo", "gx", "graw") if k in outs)

        def spot(i, last):
            img, (h, w), j = i // nv, pix((i % nv) * io + (io - 1 if last else 0), W), half - 1
            pair = slice(2 * j, 2 * j + 2)
            reach = dict(gx=(img, half + j, h, w), graw=(img, pair, h, w), ga=(pair,), gb=(pair,))
            return ("gy", (img, half + j, h, w), dict(reach, **(dict(xo=None) if "xo" in outs else {})))
    elif entry in ("actnorm_backward", "actnorm_reverse_backward", "actnorm_backward_reconstruct"):
        x, gy, gl, ls, tr = R("x", *shape), R("gy", *shape), R("gl", B), 0.2 * R("ls", C), R("tr", C)
        e = torch.exp(-dd(ls))
        s.sym, s.ws = "finc_" + entry + "_f32", lambda b: L.finc_actnorm_workspace_bytes(b, C, HW)
        outs = dict(gx=F32, gls=F32, gt=F32)
        if entry == "actnorm_reverse_backward":       # of y = x * exp(ls) + t, from the reverse's INPUT x
            s.ins, s.batched, s.acts = dict(gy=D(gy), x=D(x), ls=D(ls)), ("gy", "x"), ("gy", "x", "gx")
            s.argf = lambda b: (lambda p, w, n: (p["gy"], p["x"], p["ls"], p["gx"], p["gls"], p["gt"], b, C, HW, w, n, None))
            s.refs = dict(gx=(dd(gy) * par(1.0 / e)).numpy(), gt=dd(gy).sum((0, 2, 3)).numpy(),
                          gls=((1.0 / e) * (dd(gy) * dd(x)).sum((0, 2, 3))).numpy())
        else:                                          # of y = (x - t) * exp(-ls), from the forward's OUTPUT y
            y32 = actnorm_ref(x, ls, tr, 1)[0].contiguous()
            s.refs = dict(gx=(dd(gy) * par(e)).numpy(), gt=(-e * dd(gy).sum((0, 2, 3))).numpy(),
                          gls=(-(dd(gy) * dd(y32)).sum((0, 2, 3)) - HW * dd(gl).sum()).numpy())
            if entry == "actnorm_backward":
                s.ins, s.batched, s.acts, s.alias = dict(gy=D(gy), gl=D(gl), y=D(y32), ls=D(ls)), ("gy", "gl", "y"), ("gy", "y", "gx"), dict(gx="gy")
                s.argf = lambda b: (lambda p, w, n: (p["gy"], p["gl"], p["y"], p["ls"], p["gx"], p["gls"], p["gt"], b, C, HW, w, n, None))
            else:
                s.ins, s.batched = dict(gy=D(gy), gl=D(gl), y=D(y32), ls=D(ls), tr=D(tr)), ("gy", "gl", "y")
                s.acts, outs = ("gy", "y", "xo", "gx"), dict(xo=F32, **outs)
                s.argf = lambda b: (lambda p, w, n: (p["gy"], p["gl"], p["y"], p["ls"], p["tr"], p["xo"], p["gx"], p["gls"], p["gt"], b, C, HW, w, n, None))
                s.refs["xo"] = (dd(y32) * par(1.0 / e) + par(dd(tr))).numpy()
        s.outs = lambda b: {k: (((C,) if k in ("gls", "gt") else sh(b)), dt) for k, dt in outs.items()}
        s.elementwise = tuple(k for k in ("xo", "gx") if k in outs)

        def spot(i, last):
            img, (h, w), c = i // nv, pix((i % nv) * io + (io - 1 if last else 0), W), C - 1
            return ("gy", (img, c, h, w), dict(gx=(img, c, h, w), gls=(c,), gt=(c,), **(dict(xo=None) if "xo" in outs else {})))
    elif entry == "actnorm_init":
        x = R("x", *shape).clone()
        x[:, 1] = 500.0 + 0.5 * x[:, 1]                 # a mean of 1e3 times the spread: the trips change which Chan merges run
        s.sym, s.ws = "finc_actnorm_init_f32", lambda b: L.finc_actnorm_workspace_bytes(b, C, HW)
        s.ins, s.batched, s.acts = dict(x=D(x)), ("x",), ("x",)
        s.outs = lambda b: dict(ls=((C,), F32), tr=((C,), F32))
        s.argf = lambda b: (lambda p, w, n: (p["x"], p["ls"], p["tr"], b, C, HW, w, n, None))
        xc = dd(x).transpose(0, 1).reshape(C, -1)
        s.refs = dict(tr=xc.mean(1).numpy(), ls=torch.log(xc.std(1) + 1e-8).numpy())
        s.elementwise = ()

        def spot(i, last):
            img, (h, w), c = i // nv, pix((i % nv) * io + (io - 1 if last else 0), W), 1
            return ("x", (img, c, h, w), dict(ls=(c,), tr=(c,)))
    elif entry in ("mix", "mix_transposed"):
        x, mat, bias = R("x", *shape), R("mat", C, C) / C ** 0.5, R("bias", C)
        xd, md = D(x), D(mat)
        if entry == "mix":
            s.sym, s.ins, s.batched, s.acts, s.alias = "finc_mix_f32", dict(x=xd, mat=md, bias=D(bias)), ("x",), ("x", "out"), dict(out="x")
            s.argf = lambda b: (lambda p, w, n: (p["x"], p["mat"], p["bias"], p["out"], b, C, HW, None))
            eq = "oi,bihw->bohw"
        else:       # the grad-input of finc_mix_backward_f32: out = mat^T x, no bias, no workspace, never in place
            s.sym, s.ins, s.batched, s.acts = "finc_mix_backward_f32", dict(x=xd, mat=md), ("x",), ("x", "out")
            s.argf = lambda b: (lambda p, w, n: (p["x"], None, p["mat"], p["out"], None, None, b, C, HW, None, 0, None))
            eq = "oi,bohw->bihw"
        s.outs = lambda b: dict(out=(sh(b), F32))
        if C >= 96:                                    # torch's float64 einsum on the device: shares nothing with the kernel under test
            ref = torch.einsum(eq, md.double(), xd.double())
            ref = (ref + par(D(bias).double()) if entry == "mix" else ref).cpu()
        else:
            ref = torch.einsum(eq, dd(mat), dd(x))
            ref = ref + par(dd(bias)) if entry == "mix" else ref
        s.refs = dict(out=ref.numpy())
        s.elementwise, s.record_only = ("out",), True
        cpi = case["plan"]["items"] // B

        def spot(i, last):
            b, (h, w) = i // cpi, pix((i % cpi) * 16 * io, W)
            return ("x", (b, C - 1, h, w), dict(out=(b, slice(None), h, w)))
    else:
        raise KeyError(entry)
    s.spot = spot
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# one (case, entry)
# ---------------------------------------------------------------------------------------------------------------------------------
def judge_regime(spec, errs_out):
    def judge(plain):
        for k, ref in spec.refs.items():
            e = rel_err(plain.outs[k].float().cpu().numpy(), ref)
            bar = BF16_HALF_ULP + TOL if k in spec.bf16_outs else TOL
            print("%s %s vs float64: %.3e (bar %.3e)" % (spec.sym, k, e, bar))
            errs_out[k] = e
        bad = {k: e for k, e in errs_out.items() if e > (BF16_HALF_ULP + TOL if k in spec.bf16_outs else TOL)}
        assert not bad, (spec.sym, bad)
        return dict(errs_out)
    return judge


def regime_case(dev, name, entry):
    from fincflow_amd import _lib
    case = PIXEL_REGIME_CASES[name]
    want = case["plan"]
    assert plan_of(case, case["shape"][3] if case["family"] == "negate" else case["shape"][0]) == want, name
    spec = build(entry, name, case, dev)
    full = case["shape"][3] if case["family"] == "negate" else case["shape"][0]
    lead = spec.acts if case["align"] < 16 else ()
    lead_floats = 2 if case["align"] == 8 else 1
    in_place_only = getattr(spec, "always_in_place", False)

    def call(ins, b=full, guard=False, alias=None):
        return run(dev, spec.sym, spec.argf(b), ins, spec.outs(b), spec.ws(b), guard, lead, spec.alias if in_place_only else alias, lead_floats)

    # 1. the plan at the alignment the call's activation pointers really had
    variant = dict(kernel=spec.sym, plan=want, align=case["align"])
    errs = {}
    seen_align = []

    def bounds_call(guard):
        res = call(spec.ins, guard=guard)
        seen_align.append(min(alignment_class(res.ptrs[k]) for k in spec.acts if res.ptrs.get(k) is not None))
        return res
    plain = check_bounds(name, bounds_call, variant, judge_regime(spec, errs), entry=entry, shape=list(case["shape"]))
    assert seen_align and set(seen_align) == {case["align"]}, (name, seen_align)
    got = plan_of(case, full, align=seen_align[0])
    assert got == want and (got["trips"] >= 2 or not multi_trip(case)), (name, got, want)
    assert multi_trip(case) or name.startswith("mix_align8"), name

    # 2b. the documented in-place form: same bits, guards intact
    if spec.alias and not in_place_only:
        inplace = call(spec.ins, guard=True, alias=spec.alias)
        assert not inplace.bad, (name, entry, inplace.bad)
        assert all(same_bits(plain.outs[k], inplace.outs[k]) for k in plain.outs), (name, entry, "in place differs from out of place")

    # 3b. a bfloat16 output has the bits of the fp32 result rounded once; a bf16 raw gives the fp32 sibling's bits
    for k, exact in getattr(spec, "exact", {}).items():
        assert torch.equal(bits16(plain.outs[k].cpu()), bits16(exact)), (name, entry, k, "not the fp32 formula rounded once")
    if case["elem"] == 2 and case["rule"] == "parts":
        sib = build(entry, name, case, dev, sibling=True)
        sres = run(dev, sib.sym, sib.argf(full), sib.ins, sib.outs(full), sib.ws(full), False, lead, None, lead_floats)
        for k in plain.outs:
            if k in spec.bf16_outs:
                assert torch.equal(bits16(plain.outs[k]), bits16(sres.outs[k].bfloat16())), (name, entry, k, "not the fp32 sibling's value rounded once")
            else:
                assert same_bits(plain.outs[k], sres.outs[k]), (name, entry, k, "differs from the fp32 sibling on the same values")

    # 4. sub-batches of one trip each
    sub_equal = None
    if spec.elementwise and multi_trip(case):
        b1 = one_trip_batch(case)
        assert 1 <= b1 < full
        parts = {k: [] for k in spec.elementwise}
        for start in range(0, full, b1):
            n = min(b1, full - start)
            assert plan_of(case, n)["trips"] == 1, (name, n)
            ins = {k: (v[start:start + n] if k in spec.batched and v is not None else v) for k, v in spec.ins.items()}
            res = call(ins, b=n)
            for k in spec.elementwise:
                parts[k].append(res.outs[k])
        sub_equal = {k: same_bits(torch.cat(parts[k]), plain.outs[k]) for k in spec.elementwise}
        if not getattr(spec, "record_only", False):
            assert all(sub_equal.values()), (name, entry, sub_equal, "the whole-tensor call differs from its one-trip sub-batches")

    # 5. a poisoned element of the last trip shows where the definition sends it, and nowhere else
    items = last_trip_spots(case)
    spots = [spec.spot(i, i == items[-1]) for i in items]
    check_isolation(dev, name, lambda ins: call(ins), spec.ins, spots, variant, spec.values, entry=entry, shape=list(case["shape"]))
    report("pixel_regime", case=name, entry=entry, kernel=spec.sym, shape=list(case["shape"]), align=case["align"], plan=got, err=errs,
           sub_batch=b1 if sub_equal is not None else None, sub_batch_bit_equal=sub_equal, poisoned_items=[int(i) for i in items])
    assert not _lib.fault_pending()


def cases_of(table, transposed=False):
    for name in sorted(table):
        for entry in table[name]["entries"]:
            yield pytest.param(name, entry, id="%s-%s" % (name, entry))
        if transposed and table[name]["transposed"]:
            yield pytest.param(name, "mix_transposed", id="%s-mix_transposed" % name)


@pytest.mark.parametrize("name,entry", list(cases_of(ROW_CASES)))
def test_grid_stride_rows_take_a_second_trip(name, entry, dev):
    """cpl_row_grid's kernels (ActNorm's transform, bias + ReLU on fp32 and bf16, the grouped lead product) beyond 8192 workgroups of
    items, and finc_negate_f32 beyond its 1024."""
    regime_case(dev, name, entry)


@pytest.mark.parametrize("name,entry", list(cases_of(PART_CASES)))
def test_outer_part_workgroups_take_several_trips(name, entry, dev):
    """cpl_parts / cpl_grad_plan: every coupling transform and backward (fp32 and bf16 raw), ActNorm's backwards and its init, at
    P = 4 on 512 images and Q = 256 / 128 per channel unit."""
    regime_case(dev, name, entry)


@pytest.mark.parametrize("name,entry", list(cases_of(MIX_CASES, transposed=True)))
def test_mix_chunk_loop_and_forms(name, entry, dev):
    """finc_mix_launch's regimes: big and just below, every pixels-per-lane x workgroup-size pair the table has beyond the small
    shapes' (8-wave 4-pixel, 16-wave 2-pixel and dword), the C = 128 fallback chain, a wave's second to fourth chunk, and the
    two-pixel form on pointers that are 8-byte but not 16-byte aligned."""
    regime_case(dev, name, entry)


# ---------------------------------------------------------------------------------------------------------------------------------
# F(2,5) on 8-byte aligned activations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WINO5_ALIGN8_CASES))
def test_f25_on_8_byte_aligned_activations(name, dev):
    """finc_wino5.hip moves 8-byte pairs (raw_buffer_load_b64 / raw_buffer_store_b64 at offsets that are whole pairs: W even) and
    finc_wino5_takes asks for align >= 8 only: forward (in, out two floats into their allocations) and grad-input (grad_z, grad_x)
    between guards, bit-stable, against float64 autograd at TOL.  The same views one float in take the strip kernel; both agree with
    the reference."""
    from fincflow_amd import _lib
    case = WINO5_ALIGN8_CASES[name]
    dims = case["dims"]
    B, G, Cq, H, W, KH, KW = dims
    assert _lib.conv_plan(*dims, align=8) == case["plan"] and _lib.conv_plan(*dims, align=4)["form"] == "strip", name
    u = Unit(dev, dims, seed=sum(dims))
    z, gx, _ = conv_reference(u)
    x, gz = to_dev(u.x, dev), to_dev(u.gz, dev)
    L = _lib.lib()
    fws, bws = L.finc_workspace_bytes(G, Cq, KH, KW), L.finc_backward_workspace_bytes(*dims)
    for lead_floats, form in ((2, "winograd25"), (1, "strip")):
        align = 4 * lead_floats
        errs = {}

        def forward(guard):
            res = run(dev, "finc_forward_f32", lambda p, w, n: (p["act"], p["w"], p["out"], *dims, u.orient, _lib.ALGO["auto"], w, n, None),
                      dict(act=x, w=u.wc), dict(out=(u.shape, F32)), fws, guard, ("act", "out"), None, lead_floats)
            assert {alignment_class(res.ptrs[k]) for k in ("act", "out")} == {align}
            return res

        def backward(guard):
            res = run(dev, "finc_backward_f32", lambda p, w, n: (p["gz"], p["x"], p["w"], p["gx"], None, *dims, u.orient, w, n, None),
                      dict(gz=gz, x=x, w=u.wc), dict(gx=(u.shape, F32)), bws, guard, ("gz", "gx"), None, lead_floats)
            assert {alignment_class(res.ptrs[k]) for k in ("gz", "gx")} == {align}
            return res

        def judge(key, ref):
            def j(plain):
                errs[key] = rel_err(plain.outs[key].cpu().numpy(), ref)
                print("%s %s align %d: %.3e" % (name, key, align, errs[key]))
                assert errs[key] <= TOL, (name, key, align, errs[key])
                return errs[key]
            return j
        assert _lib.conv_plan(*dims, align=align)["form"] == form
        variant = dict(conv_form=form, align=align)
        check_bounds(name, forward, variant, judge("out", z), entry="forward", dims=list(dims))
        check_bounds(name, backward, variant, judge("gx", gx), entry="backward_grad_input", dims=list(dims))
        report("pixel_regime", case=name, entry="forward+grad_input", kernel=form, dims=list(dims), align=align, plan=_lib.conv_plan(*dims, align=align), err=errs)
    assert _lib.runtime_switches() == [] and not _lib.fault_pending()
