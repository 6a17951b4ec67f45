"""Training without stored activations on the GPU: the two kernels that differentiate a layer from its OUTPUT and
rebuild its input in the same pass (include/finc.h: finc_actnorm_backward_reconstruct_f32, finc_coupling_backward_reconstruct_f32),
`backward_from_output` of every layer, and `FlowSequential.invertible_backward` on a model.

References: the float64 formulas of helpers.actnorm_ref / coupling_ref with autograd (kernels), the float64 twin of tests/flow_twin.py
(layers, model).  Bars: TOL = 1e-5 in helpers.rel_err, CHAIN_TOL = 5e-5 (tests/test_gpu_inverse_backward.py) for gradients through a
unit and through the model; a gradient whose reference is identically zero must be exactly zero.  The stored HIP autograd path on the
same inputs is recorded beside every layer and model error as the yardstick.  Every case prints what it achieved and appends it to the
parity report (kind `invertible_backward`).

The layer and model gradients are taken at the REBUILT activations: their error includes the inverse's.  The twin differentiates the
branch of every coupling-net ReLU that the recomputation took (flow_twin.recorded_masks around forward and backward, the last call of
each ReLU: inside a run the no-grad forward runs the net on the fused bias + ReLU kernel, so the recomputation is the only call of
the module; a coupling outside a run calls it once, in the forward)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import flow_twin
from flow_twin import recorded_masks, replayed_masks
from helpers import actnorm_ref, coupling_ref, rel_err, report, same_bits
from test_gpu_bounds import F32, grads, pixel_inputs, run
from test_gpu_inverse_backward import CHAIN_TOL

pytestmark = pytest.mark.gpu

TOL = 1e-5
KIND = "invertible_backward"
SHAPES = [(1, 2, 1, 1), (3, 6, 5, 3), (2, 6, 4, 4), (4, 12, 64, 64)]
ODD_C = (3, 7, 5, 3)
#: (op, shape, dword form forced by a 4-byte-aligned pointer)
KERNEL_CASES = ([(op, s, False) for op in ("actnorm", "coupling") for s in SHAPES]
                + [("actnorm", (2, 6, 4, 4), True), ("coupling", (2, 6, 4, 4), True), ("actnorm", ODD_C, False)])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def record_calls(monkeypatch):
    """Every entry point that goes through ops._call, by name, in order."""
    from fincflow_amd import ops
    names, real = [], ops._call

    def recorded(name, *args, **kwargs):
        names.append(name)
        return real(name, *args, **kwargs)
    monkeypatch.setattr(ops, "_call", recorded)
    return names


# ---------------------------------------------------------------------------------------------------------------------------------
# the two kernels through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_case(op, shape, with_gl=True):
    """The call (test_gpu_bounds.run's pieces) and its float64 references, once per case.  `y` is the float32 forward output the
    kernel is handed; the references rebuild x from exactly that y in float64 and differentiate the forward there."""
    from fincflow_amd import _lib
    L = _lib.lib()
    B, C, H, W = shape
    HW = H * W
    T = pixel_inputs(shape)
    gl = T["gl"] if with_gl else None
    if op == "actnorm":
        y = actnorm_ref(T["x"].double(), T["ls"].double(), T["tr"].double(), 1)[0].float().contiguous()
        x_ref = actnorm_ref(y.double(), T["ls"].double(), T["tr"].double(), -1)[0]
        g = grads(lambda x, ls, tr: actnorm_ref(x, ls, tr, 1), [x_ref, T["ls"], T["tr"]], [T["gy"], gl])
        return dict(sym="finc_actnorm_backward_reconstruct_f32", ws=L.finc_actnorm_workspace_bytes(B, C, HW),
                    ins=dict(gy=T["gy"], gl=gl, y=y, ls=T["ls"], tr=T["tr"]), acts=("gy", "y", "xo", "gx"),
                    outs=dict(xo=(shape, F32), gx=(shape, F32), gls=((C,), F32), gt=((C,), F32)),
                    argf=lambda p, w, n: (p["gy"], p["gl"], p["y"], p["ls"], p["tr"], p.get("xo"), p.get("gx"), p.get("gls"), p.get("gt"),
                                          B, C, HW, w, n, None),
                    refs=dict(xo=x_ref.detach().numpy(), gx=g[0], gls=g[1], gt=g[2]))
    d = [T[k].double() for k in ("raw", "a", "b")]
    y = coupling_ref(T["x"].double(), *d, 1)[0].float().contiguous()
    x_ref = coupling_ref(y.double(), *d, -1)[0]
    g = grads(lambda x, raw, a, b: coupling_ref(x, raw, a, b, 1), [x_ref, T["raw"], T["a"], T["b"]], [T["gy"], gl])
    return dict(sym="finc_coupling_backward_reconstruct_f32", ws=L.finc_coupling_workspace_bytes(B, C, HW),
                ins=dict(gy=T["gy"], gl=gl, y=y, raw=T["raw"], a=T["a"], b=T["b"]), acts=("gy", "y", "raw", "xo", "gx", "graw"),
                outs=dict(xo=(shape, F32), gx=(shape, F32), graw=(shape, F32), ga=((C,), F32), gb=((C,), F32)),
                argf=lambda p, w, n: (p["gy"], p["gl"], p["y"], p["raw"], p["a"], p["b"], p.get("xo"), p.get("gx"), p.get("graw"),
                                      p.get("ga"), p.get("gb"), B, C, HW, w, n, None),
                refs=dict(xo=x_ref.detach().numpy(), gx=g[0], graw=g[1], ga=g[2], gb=g[3]))


def call(dev, spec, outs=None, guard=False, lead=False, alias=None):
    ins = {k: (None if v is None else v.to(dev)) for k, v in spec["ins"].items()}
    outs = spec["outs"] if outs is None else {k: spec["outs"][k] for k in outs}
    return run(dev, spec["sym"], spec["argf"], ins, outs, ws=spec["ws"], guard=guard, lead=spec["acts"] if lead else (), alias=alias)


def judge(tag, shape, got, refs, bar=TOL, **fields):
    errs = {k: rel_err(got[k].cpu().numpy(), refs[k]) for k in got}
    print(KIND, tag, shape, fields or "", {k: "%.3e" % e for k, e in errs.items()}, "bar %.1e" % bar)
    report(KIND, case=tag, shape=list(shape), bar=bar, **fields, **errs)
    for k, e in errs.items():
        assert e <= bar, (tag, shape, k, e, bar)
    return errs


@pytest.mark.parametrize("op,shape,dword", KERNEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_kernel_against_float64_autograd(op, shape, dword, dev):
    """Every output at TOL; the same inputs twice give the same bits; the rebuilt input has the bits of the layer's reverse launch;
    the untouched half of the coupling passes through bit for bit."""
    from fincflow_amd import ops
    spec = kernel_case(op, shape)
    res, again = call(dev, spec, lead=dword), call(dev, spec, lead=dword)
    judge(op + "_kernel", shape, res.outs, spec["refs"], form="dword" if dword or (shape[2] * shape[3]) % 4 else "16-byte")
    for k in res.outs:
        assert same_bits(res.outs[k], again.outs[k]), (k, "not bit-stable from launch to launch")
    d = {k: v.to(dev) for k, v in spec["ins"].items()}
    if op == "actnorm":
        rev = ops.finc_actnorm(d["y"], d["ls"], d["tr"], -1)[0]
    else:
        rev = ops.finc_coupling(d["y"], d["raw"], d["a"], d["b"], -1)[0]
        half = shape[1] // 2
        assert same_bits(res.outs["xo"][:, :half], d["y"][:, :half]) and same_bits(res.outs["gx"][:, :half], d["gy"][:, :half])
    assert same_bits(res.outs["xo"], rev), "the rebuilt input differs from the reverse launch's"


@pytest.mark.parametrize("op,shape", [("actnorm", (3, 6, 5, 3)), ("actnorm", ODD_C), ("coupling", (3, 6, 5, 3)), ("coupling", (2, 6, 4, 4))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_every_subset_of_the_outputs_and_no_grad_logdet(op, shape, dev):
    """A skipped output is NULL; what is asked for has the bits of the call that asks for everything.  Without grad_logdet (NULL) the
    results are those of zeros, judged against float64 at TOL."""
    spec = kernel_case(op, shape)
    full = call(dev, spec).outs
    names = list(spec["outs"])
    for want in itertools.product((False, True), repeat=len(names)):
        picked = [n for n, w in zip(names, want) if w]
        if not picked:
            continue
        got = call(dev, spec, outs=picked).outs
        assert sorted(got) == sorted(picked)
        for n in picked:
            assert same_bits(got[n], full[n]), (op, picked, n)
    bare = kernel_case(op, shape, False)
    judge(op + "_kernel_no_grad_logdet", shape, call(dev, bare).outs, bare["refs"])
    per_channel = [n for n in names if len(spec["outs"][n][0]) == 1]
    no_ws = run(dev, spec["sym"], spec["argf"], {k: v.to(dev) for k, v in spec["ins"].items()},
                {k: v for k, v in spec["outs"].items() if k not in per_channel}, ws=None)     # no per-channel sum: no workspace
    assert all(same_bits(no_ws.outs[k], full[k]) for k in no_ws.outs)


@pytest.mark.parametrize("op,shape", [("actnorm", (3, 6, 5, 3)), ("actnorm", (2, 6, 4, 4)), ("coupling", (3, 6, 5, 3)),
                                      ("coupling", (2, 6, 4, 4))], ids=lambda v: str(v).replace(" ", ""))
def test_the_documented_aliasing(op, shape, dev):
    """include/finc.h: x_out == y and grad_x == grad_y are allowed, each alone and both at once, in both alignment classes: the bits
    of the call with outputs of their own.  (Every other overlap is refused: tests/test_invertible_backward_host.py.)"""
    spec = kernel_case(op, shape)
    for lead in (False, True):
        base = call(dev, spec, lead=lead).outs
        for alias in (dict(xo="y"), dict(gx="gy"), dict(xo="y", gx="gy")):
            got = call(dev, spec, lead=lead, alias=alias).outs
            for k in base:
                assert same_bits(got[k], base[k]), (op, shape, lead, alias, k)


@pytest.mark.parametrize("op,shape", [("actnorm", (3, 6, 5, 3)), ("actnorm", (2, 6, 4, 4)), ("actnorm", ODD_C), ("actnorm", (4, 12, 64, 64)),
                                      ("coupling", (3, 6, 5, 3)), ("coupling", (2, 6, 4, 4)), ("coupling", (4, 12, 64, 64)),
                                      ("coupling", (1, 2, 1, 1))], ids=lambda v: str(v).replace(" ", ""))
def test_guard_bands_around_every_output_and_the_workspace(op, shape, dev):
    """Every tensor and the workspace between NaN guards, with 16-byte aligned pointers and shifted by one float: no guard is written,
    no NaN is left in an output, and the outputs have the bits of the plain call."""
    spec = kernel_case(op, shape)
    for lead in (False, True):
        plain, guarded = call(dev, spec, lead=lead), call(dev, spec, guard=True, lead=lead)
        assert not guarded.bad, (op, shape, lead, guarded.bad)
        assert guarded.nguard > 0
        for k in plain.outs:
            assert not bool(torch.isnan(guarded.outs[k]).any()), (op, shape, lead, k, "NaN left in the output")
            assert same_bits(guarded.outs[k], plain.outs[k]), (op, shape, lead, k)
        report(KIND, case=op + "_kernel_guards", shape=list(shape), lead_floats=int(lead), guard_elements=guarded.nguard)


def test_an_empty_batch_launches_nothing_and_zeroes_the_sums(dev, monkeypatch):
    from fincflow_amd import ops
    calls = record_calls(monkeypatch)
    y, gy = torch.empty(0, 6, 4, 4, device=dev), torch.empty(0, 6, 4, 4, device=dev)
    v = torch.ones(6, device=dev)
    x, gx, gls, gt = ops.finc_actnorm_backward_reconstruct(gy, None, y, v, v)
    assert x.shape == gx.shape == y.shape and not bool(gls.any()) and not bool(gt.any())
    x, gx, graw, ga, gb = ops.finc_coupling_backward_reconstruct(gy, None, y, torch.empty_like(y), v, v)
    assert x.shape == gx.shape == graw.shape == y.shape and not bool(ga.any()) and not bool(gb.any())
    assert ops.finc_actnorm_backward_reconstruct(gy, None, y, v, v, False, False, False, False) == (None, None, None, None)
    assert not calls, calls


def test_a_coupling_channel_whose_translation_dwarfs_its_spread(dev):
    """DESIGN 3.18 limit (a): pair j = 1 of a (2, 6, 4, 4) coupling with |t| = 1e3 * max|y - t| and s = 0 on that pair.  y - t is an
    exact float32 subtraction of two numbers near |t|, so what it loses is the ONE rounding of t = a * raw + b at that magnitude:
    at most 2^-24 |t| = 1e3 * 2^-24 relative to the channel's largest |y - t|, which is the largest |x| there (s = 0).
      x:      bar = 2 * 1e3 * 2^-24 (the rounding above, once more for everything else in the pass);
      grad_a: grad_a[2j] = sum gh * u with gh = grad_y2 * (y - t) + grad_logdet carries that error as sum |grad_y2 * u| * 2^-24 |t|; the
              inputs' own worst-case condition sum |grad_y2 * u| * max|y - t| / max|grad_a| is asserted to be below 16 (32 terms of random
              sign: 9.5 here), so bar = 16 * 1e3 * 2^-24.
    Both are judged against float64 at the SAME float32 y, not against TOL; the achieved errors go to the parity report."""
    shape, j = (2, 6, 4, 4), 1
    half = shape[1] // 2
    T = {k: v.clone() for k, v in pixel_inputs(shape).items()}
    T["a"][2 * j], T["b"][2 * j] = 0.0, 0.0                                   # s = 0 on the pair: x2 = y2 - t
    spread = float(T["x"][:, half + j].abs().max())
    T["b"][2 * j + 1] = 1e3 * spread
    d = [T[k].double() for k in ("raw", "a", "b")]
    y = coupling_ref(T["x"].double(), *d, 1)[0].float().contiguous()
    x_ref = coupling_ref(y.double(), *d, -1)[0]
    t = d[1][2 * j + 1] * d[0][:, 2 * j + 1] + d[2][2 * j + 1]
    ratio = float(t.abs().max() / (y[:, half + j].double() - t).abs().max())
    assert 0.9e3 <= ratio <= 1.1e3, ratio
    g = grads(lambda x, raw, a, b: coupling_ref(x, raw, a, b, 1), [x_ref, T["raw"], T["a"], T["b"]], [T["gy"], T["gl"]])
    cond = float((T["gy"][:, half + j].double() * d[0][:, 2 * j]).abs().sum() * (y[:, half + j].double() - t).abs().max()
                 / np.abs(g[2]).max())
    assert cond <= 16.0, cond
    from fincflow_amd import ops
    x, gx, graw, ga, gb = ops.finc_coupling_backward_reconstruct(T["gy"].to(dev), T["gl"].to(dev), y.to(dev), T["raw"].to(dev),
                                                                 T["a"].to(dev), T["b"].to(dev))
    unit = 1e3 * 2.0 ** -24
    e_x, e_ga = rel_err(x.cpu().numpy(), x_ref.detach().numpy()), rel_err(ga.cpu().numpy(), g[2])
    e_pair = rel_err(x[:, half + j].cpu().numpy(), x_ref[:, half + j].detach().numpy())
    print(KIND, "coupling_cancellation: x %.3e (the pair alone %.3e, bar %.3e), grad_a %.3e (bar %.3e), |t| / max|y - t| = %.1f, "
          "condition of the sum %.2f" % (e_x, e_pair, 2 * unit, e_ga, 16 * unit, ratio, cond))
    report(KIND, case="coupling_cancellation", shape=list(shape), x=e_x, x_pair=e_pair, grad_a=e_ga, bar_x=2 * unit, bar_grad_a=16 * unit,
           ratio=ratio, condition=cond)
    assert e_x <= 2 * unit and e_pair <= 2 * unit, (e_x, e_pair, 2 * unit)
    assert e_ga <= 16 * unit, (e_ga, 16 * unit)


# ---------------------------------------------------------------------------------------------------------------------------------
# backward_from_output, layer by layer
# ---------------------------------------------------------------------------------------------------------------------------------
LAYERS = ("unit", "cinc", "padded_bias", "actnorm", "conv1x1", "coupling", "coupling_context", "squeeze")
LAYER_SHAPES = [(3, 12, 9, 12), (2, 12, 4, 4)]                  # the layer's OUTPUT (Squeeze: its input is (B, 3, 2H, 2W))
UNITS = ("unit", "cinc", "padded_bias")


def make_layer(kind, shape):
    from fincflow_amd import CINCFlowUnit, FastFlowUnit, PaddedConv2d, glow
    torch.manual_seed(11)
    np.random.seed(11)
    g = torch.Generator().manual_seed(13)
    r = lambda shp, s: torch.randn(shp, generator=g) * s
    B, C, H, W = shape
    with torch.no_grad():
        if kind == "unit":
            return FastFlowUnit(C, C, (3, 3))
        if kind == "cinc":
            return CINCFlowUnit(C, C, (3, 3))
        if kind == "padded_bias":
            m = PaddedConv2d(C, C, (3, 3), bias=True)
            m.bias.copy_(r(m.bias.shape, 0.3))
            return m
        if kind == "actnorm":
            m = glow.ActNorm(C)
            m.log_scale.copy_(r(m.log_scale.shape, 0.3))
            m.translation.copy_(r(m.translation.shape, 1.0))
            m.mark_initialized()
            return m
        if kind == "conv1x1":
            m = glow.Conv1x1(C)
            m.W.add_(r(m.W.shape, 0.3))
            return m
        if kind == "squeeze":
            return glow.Squeeze()
        m = glow.Coupling((C, H, W), width=16, n_context=3 if kind == "coupling_context" else None)
        for p in m.net.parameters():
            p.copy_(r(p.shape, 0.05))
        return m


def layer_inputs(kind, shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + len(kind))
    x = torch.randn((B, C // 4, 2 * H, 2 * W) if kind == "squeeze" else shape, generator=g)
    ctx = torch.randn(B, 3, H, W, generator=g) if kind == "coupling_context" else None
    return x, ctx, torch.randn(shape, generator=g), torch.randn(B, generator=g)


def layer_loss(m, x, ctx, gy, gl):
    y, ld = m(x, ctx) if ctx is not None else m(x)
    y = y[0] if isinstance(y, tuple) else y
    loss = (y * gy).sum()
    return y, (loss + (ld * gl).sum() if torch.is_tensor(ld) and ld.requires_grad else loss)


def layer_reference(m, kind, x, ctx, gy, gl, dtype=torch.float64):
    """(x, grad_x, grad_context, name -> parameter gradient) of the float64 (or float32: unused) twin, the units' gradients masked."""
    twin = flow_twin.twin_of(m, dtype)
    xin = x.to(dtype).requires_grad_(True)
    cin = None if ctx is None else ctx.to(dtype).requires_grad_(True)
    _, loss = layer_loss(twin, xin, cin, gy.to(dtype), gl.to(dtype))
    names = [n for n, _ in twin.named_parameters()]
    leaves = [xin] + ([cin] if cin is not None else []) + [p for _, p in twin.named_parameters()]
    g = list(torch.autograd.grad(loss, leaves, allow_unused=True))
    gx, gc = g.pop(0), (g.pop(0) if cin is not None else None)
    return gx, gc, flow_twin.masked(twin, dict(zip(names, g)))


@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", LAYERS)
def test_backward_from_output_against_the_float64_module(kind, shape, dev, monkeypatch):
    from fincflow_amd.layers import BackwardNeeds
    m = make_layer(kind, shape)
    x, ctx, gy, gl = layer_inputs(kind, shape)
    gx_ref, gc_ref, gp_ref = layer_reference(m, kind, x, ctx, gy, gl)
    m = m.to(dev)
    put = lambda v: None if v is None else v.to(dev)
    xd, cd, gyd, gld = put(x), put(ctx), put(gy), put(gl)
    names = [n for n, _ in m.named_parameters()]
    assert m.invertible_backward_supported(xd, cd)
    assert not m.invertible_backward_supported(x, ctx) and not m.invertible_backward_supported(xd.double(), cd)   # CPU, fp64: never
    with torch.no_grad():
        y = m(xd, cd)[0] if cd is not None else m(xd)[0]
    calls = record_calls(monkeypatch)
    needs = BackwardNeeds(True, True, ctx is not None, True)
    xr, gx, gc, gp = m.backward_from_output(y, gyd, gld, cd, needs)
    torch.cuda.synchronize()
    launched = list(calls)
    assert len(gp) == len(names) and (gc is None) == (ctx is None)
    # the yardstick: the layer's stored HIP autograd path on the same inputs
    xs = xd.clone().requires_grad_(True)
    cs = None if cd is None else cd.clone().requires_grad_(True)
    _, loss = layer_loss(m, xs, cs, gyd, gld)
    leaves = [xs] + ([cs] if cs is not None else []) + list(m.parameters())
    stored = list(torch.autograd.grad(loss, leaves, allow_unused=True))
    bar = CHAIN_TOL if kind in UNITS else TOL
    got = dict(x=xr, grad_x=gx, **({"grad_context": gc} if ctx is not None else {}), **dict(zip(names, gp)))
    want = dict(x=x.double(), grad_x=gx_ref, **({"grad_context": gc_ref} if ctx is not None else {}), **gp_ref)
    yard = dict(zip(["grad_x"] + (["grad_context"] if ctx is not None else []) + names, stored))
    errs, yards = {}, {}
    for k in got:
        assert got[k] is not None, k
        errs[k] = flow_twin.error(got[k], want[k])
        if k in yard and yard[k] is not None:
            yards[k] = flow_twin.error(yard[k], want[k])
    print(KIND, "layer", kind, shape, {k: "%.3e" % e for k, e in errs.items()}, "stored path", {k: "%.3e" % e for k, e in yards.items()})
    report(KIND, case="layer_" + kind, shape=list(shape), bar=bar, errs=errs, stored_path=yards)
    assert errs["x"] <= TOL, (kind, shape, errs["x"])
    for k, e in errs.items():
        assert e <= bar, (kind, shape, k, e, bar)
    for n, mask in flow_twin.stored_masks(m).items():            # unit gradients are zero under the corner-tap mask
        assert not bool(got[n].cpu()[mask == 0].any()), (kind, n)
    # launches: ONE for ActNorm, ONE for the coupling's transform, the two existing ones for Conv1x1, none for Squeeze
    if kind == "actnorm":
        assert launched == ["finc_actnorm_backward_reconstruct_f32"], launched
    elif kind.startswith("coupling"):
        assert launched == ["finc_coupling_backward_reconstruct_f32"], launched
    elif kind == "conv1x1":
        assert launched == ["finc_mix_f32", "finc_mix_backward_f32"], launched
    elif kind == "squeeze":
        assert launched == [], launched
    else:
        assert "finc_backward_f32" in launched and not any("forward" in n for n in launched), launched
    # needs / frozen parameters give None
    none = m.backward_from_output(y, gyd, gld, cd, BackwardNeeds(False, False, False, False))
    assert none[0] is None and none[1] is None and none[2] is None and all(g is None for g in none[3])
    only_x = m.backward_from_output(y, gyd, gld, cd, BackwardNeeds(True, False, False, False))
    assert same_bits(only_x[0], xr) and only_x[1] is None and all(g is None for g in only_x[3])
    if names:
        first = next(m.parameters())
        first.requires_grad_(False)
        frozen = m.backward_from_output(y, gyd, gld, cd, needs)
        assert frozen[3][0] is None and all(g is not None for g in frozen[3][1:])
        for n, a, b in zip(names[1:], frozen[3][1:], gp[1:]):                # (not bits: the net's convolutions are PyTorch's)
            assert flow_twin.error(a, b) <= TOL, (kind, n)
        last = tuple(i == len(names) - 1 for i in range(len(names)))         # one flag per parameter: the last one alone
        per = m.backward_from_output(y, gyd, gld, cd, BackwardNeeds(True, True, False, last))
        for i, g in enumerate(per[3]):
            assert (g is not None) == (last[i] and i > 0), (kind, names[i])      # (parameter 0 is frozen)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
MODEL = dict(num_blocks=2, block_size=2, actnorm=True, split_prior=True, image_size=(3, 16, 16), preprocess=False, coupling_width=16)
BATCH = 8


def fresh_model(dev, seed=0):
    from fincflow_amd import glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    return flow_twin.randomise(glow.create_model(**MODEL), seed=seed + 1).to(dev)


def images(n=BATCH, seed=4):
    return torch.randn(n, *MODEL["image_size"], generator=torch.Generator().manual_seed(seed))


def initialised_model(dev, seed=0):
    model = fresh_model(dev, seed)
    with torch.no_grad():
        model(images().to(dev))
    return model


def run_nodes(t):
    """The `_InvertibleRunFunction` nodes of the graph behind `t`."""
    seen, todo, found = set(), [t.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "_InvertibleRunFunction" in type(fn).__name__:
            found.append(fn)
        todo += [f for f, _ in fn.next_functions]
    return found


def one_pass(m, x, masks=None):
    """log_prob(x).mean().backward() on `m` (a twin: the given ReLU patterns replayed, unit gradients masked): name -> tensor."""
    p = next(m.parameters())
    xin = x.detach().to(device=p.device, dtype=p.dtype, copy=True).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    if masks is None:
        with recorded_masks(m) as rec:
            lp = m.log_prob(xin)
            nodes = run_nodes(lp)
            lp.mean().backward()
        masks = {n: v[-1:] for n, v in rec.items()}              # the call whose branch the gradients took
    else:
        nodes = []
        with replayed_masks(m, masks) as flips:
            lp = m.log_prob(xin)
            lp.mean().backward()
        if flips[0]:
            print(KIND, "%d of the twin's activations took the model's side of zero" % flips[0])
        flow_twin.mask_unit_grads(m)
    out = {"loss": lp.mean().detach(), "log_prob": lp.detach(), "grad_x": xin.grad}
    out.update({n: q.grad for n, q in m.named_parameters()})
    return out, masks, nodes


def judge_pass(tag, got, want, **fields):
    assert [k for k in got if got[k] is None] == [k for k in want if want[k] is None], "`.grad is None` differs from the twin"
    errs = {k: flow_twin.error(got[k], want[k]) for k in got if got[k] is not None}
    worst = max((k for k in errs if k not in ("loss", "log_prob")), key=errs.get)
    print(KIND, tag, fields or "", "loss %.3e, log_prob %.3e, worst gradient %.3e (%s)" % (errs["loss"], errs["log_prob"], errs[worst], worst))
    report(KIND, case=tag, loss=errs["loss"], log_prob=errs["log_prob"], worst_gradient=errs[worst], worst_at=worst, tensors=len(errs), **fields)
    return errs


def assert_pass(errs):
    assert errs["loss"] <= TOL and errs["log_prob"] <= TOL, (errs["loss"], errs["log_prob"])
    over = {k: e for k, e in errs.items() if not e <= CHAIN_TOL}
    assert not over, over


def test_log_prob_backward_against_the_float64_twin(dev):
    """The whole model with `invertible_backward = True`: loss and log_prob at TOL, every gradient at CHAIN_TOL, zero where the
    reference is identically zero -- and two nodes of the new Function in the graph (this fails on a tree without the feature, where
    the attribute is just an attribute).  The stored path's errors on the same pass are the yardstick."""
    from fincflow_amd import _lib
    model = initialised_model(dev)
    twin = flow_twin.twin_of(model)
    twin.invertible_backward = False
    x = images()
    model.invertible_backward = True
    got, masks, nodes = one_pass(model, x)
    assert len(nodes) == 2, [type(n).__name__ for n in nodes]   # Squeeze .. Coupling either side of the SplitPrior
    want, _, _ = one_pass(twin, x, masks)
    for n, mask in flow_twin.stored_masks(model).items():
        assert not bool(got[n].cpu()[mask == 0].any()), "%s: a gradient under the corner-tap mask is not zero" % n
    errs = judge_pass("model/invertible", got, want)
    model.invertible_backward = False
    stored, smasks, snodes = one_pass(model, x)
    assert not snodes
    want_s, _, _ = one_pass(twin, x, smasks)
    judge_pass("model/stored_yardstick", stored, want_s)
    assert_pass(errs)
    torch.cuda.synchronize()
    _lib.raise_if_faulted("test")


def count_saved(fn):
    """numel of every tensor `fn()` saves for its backward."""
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.numel()) or t, lambda t: t):
        out = fn()
    return saved, out


def test_a_run_saves_its_output_and_nothing_else(dev):
    """Inside each run the invertible forward saves exactly ONE activation-sized tensor, the run's output (and nothing larger than
    that); the stored path on the same layers saves at least one per layer."""
    from fincflow_amd import glow, layers
    model = initialised_model(dev)
    mods = list(model.sequence_modules)
    split = [i for i, m in enumerate(mods) if isinstance(m, glow.SplitPrior)]
    assert len(split) == 1
    x = images().to(dev)
    with torch.no_grad():
        mid = model._forward_layers(mods[:split[0] + 1], x, None)[0]
    for run, inp in ((mods[:split[0]], x), (mods[split[0] + 1:], mid)):
        assert model._invertible_run_end(run, 0, inp, None) == len(run) == 9
        params = [p for m in run for p in m.parameters()]
        act = inp.numel()
        saved, (out, logdet) = count_saved(lambda: layers._InvertibleRunFunction.apply(model, tuple(run), inp, None, *params))
        assert out.numel() == act and logdet.shape == (BATCH,)
        assert [n for n in saved if n >= act] == [act] and all(n == act for n in saved), saved
        stored, _ = count_saved(lambda: model._forward_layers(run, inp, None))
        assert sum(1 for n in stored if n >= act) >= len(run), stored
        report(KIND, case="saved_tensors", layers=len(run), invertible=len(saved), stored=len(stored),
               stored_activation_sized=sum(1 for n in stored if n >= act))


def step_memory(model, x):
    """(peak above the step's start, absolute peak) of one forward + backward, in bytes: what was allocated before the step --
    parameters, the units' bank caches, workspaces -- is there in either mode and is not the step's."""
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    model.log_prob(x).mean().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    return peak - start, peak


def test_peak_memory_does_not_grow_with_depth(dev):
    """[unit, ActNorm, Conv1x1, Coupling] x N at [8, 12, 16, 16], width 16, after a warm-up step (workspaces and caches exist).  The
    peak of a step is what it allocates above its start.  Bounds from the shapes alone:
      invertible: peak(8) - peak(4) <= the added parameters' bytes, twice (their gradients are born in the step; each tensor rounded
                  up to the allocator's 512-byte block) + two activations;
      stored:     peak(8) - peak(4) >= 16 activations (sixteen more layers, each keeps at least one).
    On an MI355X: invertible +69,632 bytes (bound 339,968), stored +2,633,728 (bound 1,572,864).  The ABSOLUTE peaks (printed and
    reported too) differ by 575,488 bytes in the invertible mode, above that bound: every unit's bank cache also holds the inverse's
    packed fragments there (52,224 bytes per unit at this bank, whatever the batch) -- persistent state that exists before the step,
    like the parameters, which is why the step's own peak is what is judged."""
    from fincflow_amd import FastFlowUnit, FlowSequential, glow
    shape = (BATCH, 12, 16, 16)
    act = 4 * int(np.prod(shape))
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(dev)
    peaks, added = {}, 0
    for N in (4, 8):
        torch.manual_seed(N)
        np.random.seed(N)
        mods = []
        for _ in range(N):
            mods += [FastFlowUnit(12, 12, (3, 3)), glow.ActNorm(12), glow.Conv1x1(12), glow.Coupling(shape[1:], width=16)]
        model = flow_twin.randomise(FlowSequential(glow.GaussianPrior(shape[1:]), *mods), seed=N, actnorm=True).to(dev)
        if N == 8:
            added = sum(-(-4 * p.numel() // 512) * 512 for m in mods[16:] for p in m.parameters())
        for mode in (True, False):
            model.invertible_backward = mode
            step_memory(model, x)                                # warm-up
            peaks[N, mode] = step_memory(model, x)
        del model
    inv, sto = peaks[8, True][0] - peaks[4, True][0], peaks[8, False][0] - peaks[4, False][0]
    print(KIND, "peak memory: invertible %d -> %d bytes (+%d, bound %d), stored %d -> %d (+%d, bound %d); absolute peaks %s"
          % (peaks[4, True][0], peaks[8, True][0], inv, 2 * added + 2 * act, peaks[4, False][0], peaks[8, False][0], sto, 16 * act,
             {str(k): v[1] for k, v in peaks.items()}))
    report(KIND, case="peak_memory", activation_bytes=act, added_parameter_bytes=added, invertible=[peaks[4, True][0], peaks[8, True][0]],
           stored=[peaks[4, False][0], peaks[8, False][0]], absolute={"%d_%s" % k: v[1] for k, v in peaks.items()})
    assert inv <= 2 * added + 2 * act, (inv, 2 * added + 2 * act)
    assert sto >= 16 * act, (sto, 16 * act)


def test_the_first_call_initialises_on_the_stored_path_and_the_next_runs_invertible(dev):
    from fincflow_amd import glow
    model = fresh_model(dev)
    twin = flow_twin.twin_of(model)
    twin.invertible_backward = False
    model.invertible_backward = True
    x = images()
    acts = [m for m in model.modules() if isinstance(m, glow.ActNorm)]
    assert len(acts) == 4 and not any(m._is_initialized() for m in acts)
    got, masks, nodes = one_pass(model, x)
    # every ActNorm ended a run on this call (it ran stored and initialised): the runs are the short stretches between them
    assert all(m._is_initialized() for m in acts) and len(nodes) > 2
    want, _, _ = one_pass(twin, x, masks)                        # the twin initialises itself on the same batch
    errs = judge_pass("model/first_call_initialises", got, want, run_nodes=len(nodes))
    assert_pass(errs)
    names = [n for n, _ in model.named_parameters() if n.endswith("log_scale") or n.endswith("translation")]
    mp, tp = dict(model.named_parameters()), dict(twin.named_parameters())
    for n in names:
        assert flow_twin.error(mp[n], tp[n]) <= TOL, n
    _, _, nodes = one_pass(model, x)
    assert len(nodes) == 2                                       # the next call: two full runs


def test_two_sgd_steps_in_each_mode_stay_together(dev):
    model_a, model_b = initialised_model(dev), initialised_model(dev)
    model_a.invertible_backward = True
    xs = [images(seed=4).to(dev), images(seed=5).to(dev)]
    for m in (model_a, model_b):
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        for x in xs:
            opt.zero_grad(set_to_none=True)
            (-m.log_prob(x).mean() / x[0].numel()).backward()
            opt.step()
    pa, pb = dict(model_a.named_parameters()), dict(model_b.named_parameters())
    errs = {n: flow_twin.error(pa[n], pb[n]) for n in pa}
    worst = max(errs, key=errs.get)
    print(KIND, "two SGD steps, invertible against stored: %.3e (%s)" % (errs[worst], worst))
    report(KIND, case="two_sgd_steps", worst=errs[worst], worst_at=worst)
    assert errs[worst] <= CHAIN_TOL, (worst, errs[worst])


def test_backward_twice_under_retain_graph_gives_the_same_bits(dev, monkeypatch):
    """The saved output is never written, so a second backward rebuilds the same activations.  The coupling nets' convolutions are
    PyTorch's: their weight gradient may run a MIOpen kernel that adds with atomics (seen here: `net.2.weight` at 9x12 differs from
    call to call, on the stored path as well), so the test asks PyTorch for its deterministic convolution algorithms; every kernel of
    the library sums in a fixed order as it is."""
    from fincflow_amd import _lib
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model = initialised_model(dev)
    model.invertible_backward = True
    x = images().to(dev).requires_grad_(True)
    loss = model.log_prob(x).mean()
    leaves = [x] + list(model.parameters())
    names = ["x"] + [n for n, _ in model.named_parameters()]
    first = torch.autograd.grad(loss, leaves, retain_graph=True)
    second = torch.autograd.grad(loss, leaves)
    differ = [n for n, a, b in zip(names, first, second) if not same_bits(a, b)]
    assert not differ, differ
    torch.cuda.synchronize()
    _lib.raise_if_faulted("test")


def test_an_input_without_grad_gets_no_grad_input_launch_for_the_first_layer(dev, monkeypatch):
    """[unit, ActNorm, Conv1x1, Coupling]: with x.requires_grad the unit's backward computes grad_x; without, it is asked for the
    weight gradient alone (need_gx False), and the result is the same."""
    from fincflow_amd import FastFlowUnit, FlowSequential, glow, ops
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # (the nets' convolutions: see the test above)
    torch.manual_seed(0)
    np.random.seed(0)
    shape = (BATCH, 12, 8, 8)
    mods = [FastFlowUnit(12, 12, (3, 3)), glow.ActNorm(12), glow.Conv1x1(12), glow.Coupling(shape[1:], width=16)]
    model = flow_twin.randomise(FlowSequential(glow.GaussianPrior(shape[1:]), *mods), actnorm=True).to(dev)
    model.invertible_backward = True
    asked, real = [], ops.finc_backward

    def spy(grad_z, x, w_canon, G, orient, need_gx=True, need_gw=True):
        asked.append((need_gx, need_gw))
        return real(grad_z, x, w_canon, G, orient, need_gx=need_gx, need_gw=need_gw)
    monkeypatch.setattr(ops, "finc_backward", spy)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dev)
    model.log_prob(x).mean().backward()
    g_without = [p.grad.clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    model.log_prob(xg).mean().backward()
    assert asked == [(False, True), (True, True)], asked
    assert xg.grad is not None and all(same_bits(p.grad, g) for p, g in zip(model.parameters(), g_without))
