"""Double precision end to end on the device: finc_backward_f64 (grad-input on the transposed bank, the grad-weight kernel with the
pixels on the MFMA K dimension, the templated direct kernels), finc_check_invariant_f64, and the modules in float64 -- units, a whole
model -- against float64 autograd on the CPU.

Both sides are float64, so the bar is the project's fp64 bar: helpers.rel_err <= 1e-12.  Every functional case computes
the worst-case bound N * 2^-53 * max(sum |terms|) / max |reference| of its sums from the reference's own operands and asserts that it
is below the bar, so the bar cannot pass a shape whose arithmetic could not meet it.  Whole models are judged at 1e-10, the bar
tests/test_gpu_sample_logdet.py uses for whole float64 layers.  The measured worst values go to the parity report (kind
`f64_backward`).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_twin
from helpers import ORDER_BITS, rel_err, report, same_bits
from test_gpu_bounds import F64, bank_std, check_bounds, check_isolation, orient_of, run

pytestmark = pytest.mark.gpu

BAR = 1e-12
MODEL_BAR = 1e-10
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: (B, G, Cq, H, W, KH, KW) and the orientation word
# ---------------------------------------------------------------------------------------------------------------------------------
def case(B, G, Cq, H, W, KH=3, KW=3, orient=None):
    return (B, G, Cq, H, W, KH, KW), (orient_of(G) if orient is None else orient)


MFMA_CASES = {
    "c3_pad4_4x4": case(2, 4, 3, 4, 4),                 # Cq = 3 pads to 4; the map is barely larger than the filter
    "k_remainder_5x7": case(2, 4, 4, 5, 7),             # W < 16, H * W = 35
    "one_row_1x3": case(1, 4, 4, 1, 3),
    "two_strips_17x17": case(3, 4, 12, 17, 17),         # the strip seam at 16, H * W odd
    "two_tiles_6x18_TL": case(2, 1, 20, 6, 18, orient=ORDER_BITS["TL"]),    # two M tiles, the second a quarter full
    "two_tiles_6x18_TR": case(2, 1, 20, 6, 18, orient=ORDER_BITS["TR"]),
    "two_tiles_6x18_BL": case(2, 1, 20, 6, 18, orient=ORDER_BITS["BL"]),
    "two_tiles_6x18_BR": case(2, 1, 20, 6, 18, orient=ORDER_BITS["BR"]),
    "exact_tiles_16x16": case(2, 4, 24, 16, 16),
    "k2_c32_9x16": case(2, 2, 32, 9, 16, 2, 2),
    "k2_pad8_4x4": case(1, 4, 6, 4, 4, 2, 2),           # Cq = 6 pads to 8
}
FALLBACK_CASES = {
    "c28_5x5": case(1, 1, 28, 5, 5),                    # no fp64 bank beyond 24 channels at 3x3
    "k5_6x6": case(2, 4, 4, 6, 6, 5, 5),
    "k3x2_5x6": case(2, 4, 4, 5, 6, 3, 2),
}
ALL_CASES = {**MFMA_CASES, **FALLBACK_CASES}
# one more slab than a grid's y dimension carries (65,535): 8 MiB per tensor, a test of its own below
MANY_SLABS_CASES = {"many_slabs_2x2": case(65536, 1, 4, 2, 2, 2, 2)}


def bank64(G, Cq, KH, KW, seed):
    """A canonical bank of bank_std's spread drawn IN float64 (bits below fp32), its corner tap unit lower triangular."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((G * Cq, Cq, KH, KW)) * bank_std(Cq, max(KH, KW))
    corner = w[:, :, -1, -1].reshape(G, Cq, Cq)
    corner[:] = np.tril(corner, -1) + np.eye(Cq)
    return w


def canonical_mask(G, Cq, KH, KW):
    """get_mask in canonical form: the corner tap of the entries with i >= o is not trainable."""
    m = np.ones((G * Cq, Cq, KH, KW))
    for g in range(G):
        for o in range(Cq):
            m[g * Cq + o, o:, -1, -1] = 0.0
    return m


def flip_dims(o):
    return [d for d, bit in ((2, 2), (3, 1)) if o & bit]


def conv_cpu(x, wc, G, orient):
    """The forward on the canonical bank, group by group: flip to the group's corner, F.pad on the top-left, F.conv2d, flip back."""
    Cq, KH, KW = wc.shape[1], wc.shape[2], wc.shape[3]
    outs = []
    for g in range(G):
        d = flip_dims((orient >> (2 * g)) & 3)
        xg = x[:, g * Cq:(g + 1) * Cq]
        xg = torch.flip(xg, d) if d else xg
        zg = F.conv2d(F.pad(xg, (KW - 1, 0, KH - 1, 0)), wc[g * Cq:(g + 1) * Cq])
        outs.append(torch.flip(zg, d) if d else zg)
    return torch.cat(outs, 1)


def grads_cpu(x, wc, gz, G, orient):
    xr, wr = torch.from_numpy(np.array(x)).requires_grad_(True), torch.from_numpy(np.array(wc)).requires_grad_(True)
    z = conv_cpu(xr, wr, G, orient)
    z.backward(torch.from_numpy(np.array(gz)))
    return z.detach().numpy(), xr.grad.numpy(), wr.grad.numpy()


@functools.lru_cache(maxsize=None)
def problem(name):
    """Operands, the float64 CPU reference and the worst-case bound of one case: computed once, shared, never written to."""
    dims, orient = {**ALL_CASES, **MANY_SLABS_CASES}[name]
    B, G, Cq, H, W, KH, KW = dims
    rng = np.random.default_rng(sum(dims) + orient)
    x, gz = rng.standard_normal((B, G * Cq, H, W)), rng.standard_normal((B, G * Cq, H, W))
    wc = bank64(G, Cq, KH, KW, seed=7 + Cq)
    assert np.any(wc != wc.astype(np.float32).astype(np.float64))
    mask = canonical_mask(G, Cq, KH, KW)
    z, gx, gw = grads_cpu(x, wc, gz, G, orient)
    gw = gw * mask
    # the sums of absolute terms, by the same (linear) maps on absolute operands
    za, gxa, gwa = grads_cpu(np.abs(x), np.abs(wc), np.abs(gz), G, orient)
    bound = dict(z=Cq * KH * KW * EPS * za.max() / np.abs(z).max(), gx=Cq * KH * KW * EPS * gxa.max() / np.abs(gx).max(),
                 gw=B * H * W * EPS * (gwa * mask).max() / np.abs(gw).max())
    for v in (x, gz, wc, z, gx, gw, mask):
        v.setflags(write=False)
    return dict(dims=dims, orient=orient, x=x, gz=gz, wc=wc, mask=mask, z=z, gx=gx, gw=gw, bound=bound)


def t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # (a copy: the shared operands are read-only)


def judge(name, tag, got, keys):
    """The bound of every judged sum is below the bar, then the result is; masked entries of grad_w are +0.0 bit for bit."""
    p, errs = problem(name), {}
    for k in keys:
        assert p["bound"][k] < BAR, (name, k, "the worst-case bound of this shape is not below the bar", p["bound"][k])
        errs[k] = rel_err(got[k].cpu().numpy(), p[k])
        print("f64_backward %s %s %s: %.3e (bound %.3e)" % (name, tag, k, errs[k], p["bound"][k]))
    report("f64_backward", case=name, tag=tag, dims=list(p["dims"]), err=errs, bound={k: float(p["bound"][k]) for k in keys})
    for k in keys:
        assert errs[k] <= BAR, (name, tag, k, errs[k])
    if "gw" in keys:
        masked = got["gw"].cpu().view(torch.int64)[torch.from_numpy(p["mask"] == 0)]
        assert masked.numel() > 0 and bool((masked == 0).all()), (name, tag, "a masked entry of grad_w is not +0.0")
    return errs


def on_side_stream(dev, fn):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = fn()
    side.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# (a), (b): functional parity, masked entries, repeatability, streams
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_backward_f64_against_cpu_autograd(name, dev):
    """ops.finc_backward on float64: both outputs, each alone, on the default and on a side stream, twice -- the same bits every
    time -- against float64 autograd through F.pad + F.conv2d on the CPU; the forward of the same bank beside it."""
    from fincflow_amd import _lib, ops
    p = problem(name)
    (B, G, Cq, H, W, KH, KW), orient = p["dims"], p["orient"]
    x, gz, wc = t(p["x"], dev), t(p["gz"], dev), t(p["wc"], dev)
    ops.check_invariant(wc, G)
    judge(name, "forward", dict(z=ops.finc_forward(x, wc, G, orient)), ("z",))
    both = lambda: ops.finc_backward(gz, x, wc, G, orient)
    gx, gw = both()
    assert gx.dtype == gw.dtype == torch.float64
    judge(name, "both", dict(gx=gx, gw=gw), ("gx", "gw"))
    gx2, gw2 = both()
    assert same_bits(gx, gx2) and same_bits(gw, gw2), (name, "not bit-stable from call to call")
    gxs, gws = on_side_stream(dev, both)
    assert same_bits(gx, gxs) and same_bits(gw, gws), (name, "a side stream gives other bits")
    gx1, none = ops.finc_backward(gz, None, wc, G, orient, need_gw=False)
    assert none is None and same_bits(gx, gx1)
    none, gw1 = ops.finc_backward(gz, x, wc, G, orient, need_gx=False)
    assert none is None and same_bits(gw, gw1)
    none, gw1s = on_side_stream(dev, lambda: ops.finc_backward(gz, x, wc, G, orient, need_gx=False))
    assert same_bits(gw, gw1s)
    assert not _lib.fault_pending()


def test_more_slabs_than_a_grid_y_carries(dev):
    """B * G = 65,536 on the one-wave family: the forward under "mfma" runs (slab and strip share grid.x), the forward and
    finc_backward's grad_x against float64 autograd on the CPU -- the last image on its own as well, so that a wrapped slab index
    cannot hide in the maximum -- and the inverse under "mfma" takes the forward's output back to x."""
    from fincflow_amd import _lib, ops
    name = "many_slabs_2x2"
    p = problem(name)
    (B, G, Cq, H, W, KH, KW), orient = p["dims"], p["orient"]
    assert B * G > 65535 and _lib.f64_plan(*p["dims"])["family"] == 1
    x, gz, wc = t(p["x"], dev), t(p["gz"], dev), t(p["wc"], dev)
    z = ops.finc_forward(x, wc, G, orient, algo="mfma")
    gx, none = ops.finc_backward(gz, None, wc, G, orient, need_gw=False)
    assert none is None
    judge(name, "mfma", dict(z=z, gx=gx), ("z", "gx"))
    for k, got in (("z", z), ("gx", gx)):
        last = rel_err(got[-1].cpu().numpy(), p[k][-1])
        print("f64_backward %s last image %s: %.3e" % (name, k, last))
        assert last <= BAR, (name, "last image", k, last)
    back = ops.finc_inverse(z, wc, G, orient, algo="mfma")
    trip = rel_err(back.cpu().numpy(), p["x"]), rel_err(back[-1].cpu().numpy(), p["x"][-1])
    print("f64_backward %s round trip: %.3e, last image %.3e" % (name, *trip))
    assert max(trip) <= BAR, (name, "round trip", trip)
    assert not _lib.fault_pending()


def test_backward_f64_dtype_rules(dev):
    from fincflow_amd import _lib, ops
    p = problem("c3_pad4_4x4")
    G, orient = p["dims"][1], p["orient"]
    x, gz, wc = t(p["x"], dev), t(p["gz"], dev), t(p["wc"], dev)
    with pytest.raises(ValueError):
        ops.finc_backward(gz, x.float(), wc, G, orient)            # a dtype mismatch is an error, not a silent cast
    with pytest.raises(ValueError):
        ops.finc_backward(gz, x, wc.float(), G, orient)
    with pytest.raises(ValueError):
        ops.finc_backward(gz.float(), x, wc, G, orient)
    with pytest.raises(ValueError):
        ops.finc_backward(gz.half(), x.half(), wc.half(), G, orient)
    bad = wc.clone()
    bad[-1, -1, -1, -1] = 1.0 + 2.0 ** -40                          # (a double that rounds to 1 in fp32)
    with pytest.raises(_lib.FincError):
        ops.check_invariant(bad, G)
    gw = ops.finc_backward(gz, x, wc, G, orient, need_gx=False)[1]
    assert same_bits(ops.canonicalize(ops.canonicalize(gw, G, orient), G, orient), gw)       # the flip is an involution on doubles too


def library_call(dev, name, ins, guard=False, workspace=True, want=("gx", "gw")):
    """finc_backward_f64 itself on plain or guarded tensors; `workspace` False: NULL (the direct kernels)."""
    from fincflow_amd import _lib
    p = problem(name)
    dims, orient = p["dims"], p["orient"]
    B, G, Cq, H, W, KH, KW = dims
    ws = _lib.lib().finc_backward_f64_workspace_bytes(*dims) if workspace else None
    outs = {k: v for k, v in dict(gx=((B, G * Cq, H, W), F64), gw=((G * Cq, Cq, KH, KW), F64)).items() if k in want}
    return run(dev, "finc_backward_f64", lambda q, w, n: (q["gz"], q["x"], q["w"], q.get("gx"), q.get("gw"), *dims, orient, w, n, None),
               dict(gz=ins["gz"], x=ins["x"], w=t(p["wc"], dev)), outs, ws, guard)


def test_the_direct_kernels_without_a_workspace(dev):
    """The first matrix-core shape with the workspace withheld: the templated direct kernels, against the same reference."""
    name = "c3_pad4_4x4"
    p = problem(name)
    ins = dict(gz=t(p["gz"], dev), x=t(p["x"], dev))
    res = library_call(dev, name, ins, workspace=False)
    judge(name, "direct", res.outs, ("gx", "gw"))
    again = library_call(dev, name, ins, workspace=False)
    assert all(same_bits(res.outs[k], again.outs[k]) for k in res.outs)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c): guard bands and isolation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k_remainder_5x7", "two_strips_17x17", "c28_5x5"])
def test_backward_f64_guard_bands_and_isolation(name, dev):
    """Every pointer between NaN guards, the workspace NaN on entry at its exact size: guards intact, the outputs the plain call's
    bits and within the bar; a poisoned image of grad_z reaches its own slab of grad_x (and its group's rows of grad_w), a poisoned
    image of x nothing of grad_x."""
    from fincflow_amd import _lib
    p = problem(name)
    B, G, Cq, H, W, KH, KW = p["dims"]
    ins = dict(gz=t(p["gz"], dev), x=t(p["x"], dev))
    variant = dict(matrix_cores=name in MFMA_CASES)
    check_bounds("backward_f64_" + name, lambda guard: library_call(dev, name, ins, guard), variant,
                 lambda plain: judge(name, "guarded", plain.outs, ("gx", "gw")), may_keep_nan=(), dims=list(p["dims"]))
    check_bounds("backward_f64_gx_" + name, lambda guard: library_call(dev, name, ins, guard, want=("gx",)), variant,
                 lambda plain: judge(name, "guarded_gx", plain.outs, ("gx",)), may_keep_nan=(), dims=list(p["dims"]))
    slabs = [(b, slice(g * Cq, (g + 1) * Cq)) for b in (0, B - 1) for g in (0, G - 1)]
    slabs = sorted(set((b, s.start) for b, s in slabs))
    spots = []
    for b, c0 in slabs:
        s = (b, slice(c0, c0 + Cq))
        rows = slice(c0, c0 + Cq)
        spots.append(("gz", s, {"gx": s, "gw": rows}))
        spots.append(("x", s, {"gx": None, "gw": rows}))
    if G == 1:                                # one group: every entry of grad_w is reachable
        spots = [(n, i, {k: v for k, v in r.items() if k != "gw"}) for n, i, r in spots]
    check_isolation(dev, "backward_f64_" + name, lambda i: library_call(dev, name, i), ins, spots, variant, dims=list(p["dims"]))
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# (d): gradcheck with respect to the input
# ---------------------------------------------------------------------------------------------------------------------------------
def unit64(cls, C, dev, seed, **kw):
    from fincflow_amd import PaddedConv2d
    torch.manual_seed(seed)
    unit = cls(C, C, (3, 3), **kw) if cls is PaddedConv2d else cls(C, C, 3)
    unit = unit.double()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                      # bits below fp32 in every trainable entry, the corner tap as it was
        for m in unit.modules():
            if isinstance(m, PaddedConv2d):
                w = m.conv.weight
                w.add_(1e-9 * torch.randn(w.shape, generator=gen, dtype=torch.float64) * m.get_mask().double())
                if m.bias is not None:
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen, dtype=torch.float64))
    return unit.to(dev)


@pytest.mark.parametrize("kind", ["fastflow", "cinc"])
def test_gradcheck_with_respect_to_the_input(kind, dev):
    from fincflow_amd import CINCFlowUnit, FastFlowUnit
    cls, C = (FastFlowUnit, 16) if kind == "fastflow" else (CINCFlowUnit, 8)
    unit = unit64(cls, C, dev, seed=3)
    for p_ in unit.parameters():
        p_.requires_grad_(False)
    x = torch.randn(1, C, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: unit(v)[0], (x,))


# ---------------------------------------------------------------------------------------------------------------------------------
# (e): the modules in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def unit_reference(unit, x, gz):
    """Float64 CPU restatement of a unit's forward under autograd: (z, grad_x, {parameter name: masked gradient})."""
    tw = flow_twin.twin_of(unit)
    xr = x.detach().cpu().clone().requires_grad_(True)
    z = tw(xr)[0]
    z.backward(gz.cpu())
    flow_twin.mask_unit_grads(tw)
    return z.detach(), xr.grad, {n: q.grad for n, q in tw.named_parameters()}


MODULE_CASES = [("fastflow", None, False), ("cinc", None, False)] + [("padded", o, b) for o in ("TL", "TR", "BL", "BR") for b in (False, True)]


@pytest.mark.parametrize("kind,order,bias", MODULE_CASES, ids=lambda v: str(v))
def test_modules_in_float64(kind, order, bias, dev):
    from fincflow_amd import CINCFlowUnit, FastFlowUnit, PaddedConv2d, _lib, reverse_grad
    C = 16
    if kind == "padded":
        unit = unit64(PaddedConv2d, C, dev, seed=11, order=order, bias=bias)
    else:
        unit = unit64(FastFlowUnit if kind == "fastflow" else CINCFlowUnit, C, dev, seed=11)
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(2, C, 6, 6, dtype=torch.float64, generator=gen).to(dev)
    gz = torch.randn(2, C, 6, 6, dtype=torch.float64, generator=gen).to(dev)
    xg = x.clone().requires_grad_(True)
    z = unit(xg)[0]
    assert z.dtype == torch.float64 and z.requires_grad
    z.backward(gz)
    z_ref, gx_ref, gp_ref = unit_reference(unit, x, gz)
    errs = dict(z=rel_err(z.detach().cpu().numpy(), z_ref.numpy()), gx=rel_err(xg.grad.cpu().numpy(), gx_ref.numpy()))
    for n, q in unit.named_parameters():
        assert q.grad is not None and q.grad.dtype == torch.float64, n
        errs[n] = rel_err(q.grad.cpu().numpy(), gp_ref[n].numpy())
    for n, mask in flow_twin.stored_masks(unit).items():
        under = dict(unit.named_parameters())[n].grad.cpu().view(torch.int64)[mask == 0]
        assert bool((under == 0).all()), (n, "a gradient under the corner-tap mask is not +0.0")
    with torch.no_grad():
        z0 = unit(x)[0]                                            # without a graph: the same launch
        back = unit.reverse(z0)
        back = back[0] if isinstance(back, tuple) else back
        back2, ld = unit.reverse_with_logdet(z0)
    errs["forward_no_grad"] = rel_err(z0.cpu().numpy(), z_ref.numpy())
    errs["round_trip"] = rel_err(back.cpu().numpy(), x.cpu().numpy())
    assert same_bits(back, back2) and ld.dtype == torch.float64 and not bool(ld.any())
    print("f64_backward module %s %s bias=%s: %s" % (kind, order, bias, errs))
    report("f64_backward", case="module_%s_%s_%s" % (kind, order, bias), err=errs)
    assert all(e <= BAR for e in errs.values()), errs
    # dtype mismatches are errors, in both directions and both ways round
    unit32 = (FastFlowUnit(C, C, 3) if kind == "fastflow" else CINCFlowUnit(C, C, 3) if kind == "cinc"
              else PaddedConv2d(C, C, (3, 3), order=order)).to(dev)
    for u, v in ((unit32, x), (unit, x.float())):
        with pytest.raises(ValueError):
            u(v)
        with pytest.raises(ValueError):
            u.reverse(v)
    # the differentiable inverse stays fp32: a float64 unit inside reverse_grad() refuses instead of returning a detached result
    with reverse_grad(), pytest.raises(_lib.FincError):
        unit.reverse(z0.clone().requires_grad_(True))
    assert not unit.invertible_backward_supported(x)


# ---------------------------------------------------------------------------------------------------------------------------------
# (f): a whole float64 model on the device against the CPU float64 twin
# ---------------------------------------------------------------------------------------------------------------------------------
def build_model():
    from test_gpu_sample_logdet import build_model as build
    return build(torch.device("cpu"))


def model_views(model, twin, x, step):
    """log_prob, every parameter's gradient of -log_prob.mean(), a sample with the latents fixed, a reconstruction: model against twin."""
    put = lambda m: x.to(next(m.parameters()).device)
    grads, lps = [], []
    for m in (model, twin):
        m.zero_grad(set_to_none=True)
        lp = m.log_prob(put(m))
        (-lp.mean()).backward()
        lps.append(lp.detach())
        grads.append({n: q.grad for n, q in m.named_parameters()})
    flow_twin.mask_unit_grads(twin)
    names = [n for n in grads[0] if grads[0][n] is not None]
    assert names == [n for n in grads[1] if grads[1][n] is not None] and len(names) > 20
    flow_twin.compare("f64_model/log_prob", ["log_prob"], [lps[0]], [lps[1]], bar=MODEL_BAR, step=step)
    flow_twin.compare("f64_model/grads", names, [grads[0][n] for n in names], [grads[1][n] for n in names], bar=MODEL_BAR, step=step)
    for n, mask in flow_twin.stored_masks(model).items():
        assert not bool(grads[0][n].cpu()[mask == 0].any()), "%s: a gradient under the corner-tap mask is not zero" % n
    with torch.no_grad():
        with flow_twin.recorded_noise(model) as draws:
            xs = model.sample(3)[0]
        with flow_twin.replayed_noise(twin, draws):
            xs_ref = twin.sample(3)[0]
        assert xs.dtype == torch.float64
        flow_twin.compare("f64_model/sample", ["x"], [xs], [xs_ref], bar=MODEL_BAR, step=step)
        with flow_twin.recorded_noise(model) as draws:             # (a reconstruction draws what its split priors dropped)
            xr = model.reconstruct(put(model))
        with flow_twin.replayed_noise(twin, draws):
            xr_ref = twin.reconstruct(put(twin))
        flow_twin.compare("f64_model/reconstruct", ["x"], [xr], [xr_ref], bar=MODEL_BAR, step=step)
    return {n: grads[0][n].clone() for n in names}


def test_a_whole_float64_model_against_the_twin(dev):
    """model.double() on the device evaluates, trains and samples: every view against the float64 CPU twin at 1e-10, over three SGD
    steps (the bank cache follows the float64 parameters), and with invertible_backward the float64 model takes the stored path."""
    from fincflow_amd import _lib
    model = build_model().double().to(dev)
    twin = flow_twin.twin_of(model)
    x = torch.randn(3, 4, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    for step in range(3):
        flow_twin.sync(twin, model)
        stored = model_views(model, twin, x, step)
        if step == 0:
            model.invertible_backward = True
            try:
                model.zero_grad(set_to_none=True)
                (-model.log_prob(x.to(dev)).mean()).backward()
                for n, q in model.named_parameters():
                    if n in stored:
                        assert same_bits(q.grad, stored[n]), (n, "invertible_backward changed a float64 gradient: not the stored path")
            finally:
                model.invertible_backward = False
        opt.step()
    assert not _lib.fault_pending()
