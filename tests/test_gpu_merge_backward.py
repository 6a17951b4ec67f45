"""The merges' backward on the GPU (include/finc.h: finc_split_prior_merge_backward_f32, its _rawbf16_f32 sibling and
finc_gauss_split_merge_backward_f32), `ops.split_prior_merge` / `ops.gauss_split_merge`, and `glow.SplitPrior.merge` /
`glow.Split.merge` recorded inside `ops.reverse_grad()` with `hip_recorded_merge` set: DESIGN 3.23.

References: float64 autograd through the written-out merge formula on the CPU (`merge_formula`), from the leaves (x1, z2, raw, a, b):
grad_x1 there is the direct share, as the kernel's; for bits, `ops.finc_coupling_reverse_backward` on the same (grad_x, x, raw, a, b)
(coupling law, no grad_log_p) and the fp32 sibling rounded once (a bf16 grad_raw, as tests/test_gpu_autocast_kernels.py holds it); for
the modules, their float64 copies on the CPU; for the models, the float64 twin of tests/flow_twin.py with the draws and the ReLUs'
activation patterns replayed.  Bars: the project's 1e-5 in helpers.rel_err (TOL) for every gradient and log-density, 5e-5 (CHAIN_TOL)
for x through a whole model, 2^-7 (GRAD_BAR of tests/test_gpu_autocast_modules.py, derived there) under bf16 autocast against the
upcasting alternative.

The kernels are cpl_grad's fifth mode on the backward's launch geometry, so the shapes, what each is here for (`FORMS`) and the check
in front of every kernel test (`reaches`) are those of tests/test_gpu_split_latent.py:
  (2, 4, 2, 2)        the 16-byte form
  (3, 6, 3, 5)        HW = 15: the dword form
  (2, 12, 16, 16)     16-byte, two parts per image in the merge in front
  (512, 16, 24, 24)   second trips of both thread loops, Q = 256 backward parts
  (2, 12, 4, 4)       on views one float into their allocation: HW % 4 == 0 but the dword form
Inputs: those of tests/test_gpu_coupling.py (split prior) and tests/test_gpu_gauss_split.py (Gaussianized split), the two halves of
their x as (x1, z2).  Every case prints what it achieved and appends it to the parity report (kind `merge_backward`)."""
import copy
import functools
import itertools

import numpy as np
import pytest
import torch

import flow_twin
import test_gpu_coupling as cpl
import test_gpu_gauss_split as gauss
from helpers import rel_err, report, same_bits
from test_gpu_autocast_modules import GRAD_BAR
from test_gpu_split_latent import CASES, LOG_2PI, Guarded, count_cats, mover, move_raw, raw_call, reaches, record_calls

pytestmark = pytest.mark.gpu

TOL = 1e-5
CHAIN_TOL = 5e-5
LAWS = [("prior", torch.float32), ("prior", torch.bfloat16), ("gauss", torch.float32)]
NAMES = ("grad_x1", "grad_z2", "grad_raw", "grad_a", "grad_b")
PRESENT = [(True, True), (False, True), (True, False)]                        # (grad_x, grad_log_p)
FAMILY = {"prior": "finc_split_prior", "gauss": "finc_gauss_split"}
FUNCTION = {"prior": "_FincSplitPriorMergeFunction", "gauss": "_FincGaussSplitMergeFunction"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def merge_of(law):
    from fincflow_amd import ops
    return ops.finc_split_prior_merge if law == "prior" else ops.finc_gauss_split_merge


def backward_of(law):
    from fincflow_amd import ops
    return ops.finc_split_prior_merge_backward if law == "prior" else ops.finc_gauss_split_merge_backward


# ---------------------------------------------------------------------------------------------------------------------------------
# references (float64 on the CPU, once per law, shape and raw type)
# ---------------------------------------------------------------------------------------------------------------------------------
def merge_formula(law, x1, z2, raw, a, b):
    """float64: (x, log_p) of the merge, written out."""
    h = a.view(1, -1, 1, 1) * raw + b.view(1, -1, 1, 1)
    if law == "prior":
        s, t = 2.0 * torch.tanh(h[:, ::2] / 2.0), h[:, 1::2]
        x2, first = (z2 - t) * torch.exp(-s), s.flatten(1).sum(1)
    else:
        m, logs = h[:, 0::2], h[:, 1::2]
        x2, first = z2 * torch.exp(logs) + m, -logs.flatten(1).sum(1)
    c = 0.5 * z2[0].numel() * LOG_2PI
    return torch.cat([x1, x2], dim=1), first - 0.5 * z2.square().flatten(1).sum(1) - c


@functools.lru_cache(maxsize=None)
def kernel_case(law, shape, raw_dtype):
    """(x1, z2, raw, a, b, grad_x, grad_log_p) in fp32 (raw rounded to `raw_dtype` first: the reference starts from the kernel's
    numbers), the float64 (x, log_p), and the float64 gradients of the two terms sum(x * grad_x), sum(log_p * grad_log_p) on their
    own (the backward is linear in them: an absent incoming gradient is its term left out)."""
    if law == "gauss":
        (x, raw, a, b, g1, g2, gl), _, _ = gauss.kernel_case(shape)
        gx = torch.cat([g1, g2], dim=1)
    else:
        x, raw, a, b, gx, gl = cpl.case(shape)
    raw, half = raw.to(raw_dtype), shape[1] // 2
    x1, z2 = x[:, :half].contiguous(), x[:, half:].contiguous()
    leaves = [v.double().requires_grad_(True) for v in (x1, z2, raw, a, b)]
    xw, log_p = merge_formula(law, *leaves)
    terms = []
    for out, g in ((xw, gx), (log_p, gl)):
        got = torch.autograd.grad((out * g.double()).sum(), leaves, retain_graph=True, allow_unused=True)
        terms.append([torch.zeros_like(v) if t is None else t for t, v in zip(got, leaves)])
    assert float(log_p.detach().abs().max()) > 0.1 and float((xw.detach()[:, half:] - z2.double()).abs().max()) > 0.1
    return (x1, z2, raw, a, b, gx, gl), (xw.detach(), log_p.detach()), terms


def want_grads(terms, present):
    return [sum(t[k] for t, p in zip(terms, present) if p).numpy() for k in range(5)]


def judge(kind, law, shape, raw_dtype, names, got, ref, tol=TOL, **fields):
    errs = {n: rel_err(g.detach().float().cpu().numpy(), np.asarray(r)) for n, g, r in zip(names, got, ref)}
    print(kind, law, shape, raw_dtype, errs)
    report("merge_backward", case=kind, law=law, shape=list(shape), raw=str(raw_dtype).replace("torch.", ""), **errs, **fields)
    for n, e in errs.items():
        assert e <= tol, (kind, law, shape, n, e)
    return errs


def on_device(law, shape, offset, raw_dtype, dev, raw=None, x=None):
    """(grad_x, grad_log_p, x, raw, a, b) on the device, x the merge launch's own output (`x`: another tensor in its place)."""
    (x1, z2, raw0, a, b, gx, gl), _, _ = kernel_case(law, shape, raw_dtype)
    move = mover(dev, offset)
    rawd, ad, bd = move_raw(raw0 if raw is None else raw, dev, offset), a.to(dev), b.to(dev)
    xd = merge_of(law)(move(x1), move(z2), rawd, ad, bd, out=move(torch.zeros(shape))) if x is None else move(x)
    return move(gx), gl.to(dev), xd, rawd, ad, bd


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law,raw_dtype", LAWS, ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_every_gradient_against_float64_autograd(shape, offset, law, raw_dtype, dev):
    """With both incoming gradients, and with each absent (NULL) in turn; two launches give the same bits."""
    reaches(shape, offset)
    _, (x_ref, _), terms = kernel_case(law, shape, raw_dtype)
    gx, gl, xd, rawd, ad, bd = on_device(law, shape, offset, raw_dtype, dev)
    if offset:
        assert all(v.data_ptr() % 16 == 4 for v in (gx, xd, rawd)) and (shape[2] * shape[3]) % 4 == 0
    assert rel_err(xd.cpu().numpy(), x_ref.numpy()) <= TOL                    # (the kernel differentiates at the merge's own output)
    fn = backward_of(law)
    for present in PRESENT:
        given = [g if p else None for g, p in zip((gx, gl), present)]
        got = fn(*given, xd, rawd, ad, bd)
        again = fn(*given, xd, rawd, ad, bd)
        torch.cuda.synchronize()
        half = (shape[0], shape[1] // 2) + shape[2:]
        assert got[0].shape == got[1].shape == half and got[0].is_contiguous() and got[1].is_contiguous()
        assert got[2].dtype == raw_dtype and all(same_bits(p.float(), q.float()) for p, q in zip(got, again))
        ref, names = want_grads(terms, present), NAMES
        if raw_dtype == torch.bfloat16:
            # a bf16 grad_raw carries 8 bits: here at 2^-8, and bit for bit against the fp32 call rounded once in the test below
            assert rel_err(got[2].float().cpu().numpy(), ref[2]) <= 2.0 ** -8
            keep = (0, 1, 3, 4)
            got, ref, names = [got[k] for k in keep], [ref[k] for k in keep], [NAMES[k] for k in keep]
        if not present[0]:
            assert not bool(got[0].any())                                    # no grad_x: the direct share of x1 is zero
        judge("backward" + ("_offset" if offset else ""), law, shape, raw_dtype, names, got, ref, present=list(present))


@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_a_bf16_grad_raw_is_the_fp32_result_rounded_once(shape, offset, dev):
    reaches(shape, offset)
    fn = backward_of("prior")
    gx, gl, xd, rawd, ad, bd = on_device("prior", shape, offset, torch.bfloat16, dev)
    got = fn(gx, gl, xd, rawd, ad, bd)
    wide = fn(gx, gl, xd, mover(dev, offset)(rawd.float().cpu()), ad, bd)
    torch.cuda.synchronize()
    assert got[2].dtype == torch.bfloat16 and wide[2].dtype == torch.float32
    assert torch.equal(got[2].view(torch.int16), wide[2].bfloat16().view(torch.int16))
    for k in (0, 1, 3, 4):
        assert same_bits(got[k], wide[k]), NAMES[k]                              # everything else: the bits of the fp32 call


@pytest.mark.parametrize("raw_dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_without_grad_log_p_the_bits_are_the_coupling_reverse_backwards(shape, offset, raw_dtype, dev):
    """Coupling law, grad_log_p None: grad_raw, grad_a, grad_b of `finc_coupling_reverse_backward` on the same (grad_x, x, raw, a, b),
    and its grad_x in two halves."""
    from fincflow_amd import ops
    reaches(shape, offset)
    gx, _, xd, rawd, ad, bd = on_device("prior", shape, offset, raw_dtype, dev)
    got = ops.finc_split_prior_merge_backward(gx, None, xd, rawd, ad, bd)
    want = ops.finc_coupling_reverse_backward(gx, xd, rawd, ad, bd)
    torch.cuda.synchronize()
    half = shape[1] // 2
    assert same_bits(got[0], want[0][:, :half]) and same_bits(got[1], want[0][:, half:])
    assert torch.equal(got[0], gx[:, :half])
    for k in (1, 2, 3):
        assert same_bits(got[k + 1].float(), want[k].float()), NAMES[k + 1]
    report("merge_backward", case="reverse_backward_bits", law="prior", shape=list(shape), raw=str(raw_dtype).replace("torch.", ""),
           offset=offset, equal=True)


@pytest.mark.parametrize("law,raw_dtype", LAWS, ids=str)
@pytest.mark.parametrize("shape", [(3, 6, 3, 5), (2, 12, 16, 16)], ids=str)
def test_every_combination_of_skipped_outputs(shape, law, raw_dtype, dev):
    fn = backward_of(law)
    args = on_device(law, shape, False, raw_dtype, dev)
    full = fn(*args)
    for need in itertools.product((True, False), repeat=5):
        got = fn(*args, *need)
        for n, g, f, name in zip(need, got, full, NAMES):
            assert (g is not None) == n, (need, name)
            if n:
                assert same_bits(g.float(), f.float()), (need, name)
    assert fn(*args, False, False, False, False, False) == (None,) * 5
    report("merge_backward", case="skipped_outputs", law=law, shape=list(shape), raw=str(raw_dtype).replace("torch.", ""), combinations=32)


@pytest.mark.parametrize("law,raw_dtype", LAWS, ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_guard_bands_around_every_output_are_intact(shape, offset, law, raw_dtype, dev):
    """The entry point called directly, every output and the workspace between guard bands: nothing is written beyond a tensor, and
    the results are those of the plain call."""
    reaches(shape, offset)
    from fincflow_amd import _lib
    gx, gl, xd, rawd, ad, bd = on_device(law, shape, offset, raw_dtype, dev)
    B, C, H, W = shape
    hs = (B, C // 2, H, W)
    nbytes = _lib.lib().finc_coupling_workspace_bytes(B, C, H * W)
    g = Guarded(dev, 1 if offset else 0)
    ws = g.new((nbytes // 4,))
    g1, gz, graw, ga, gb = g.new(hs), g.new(hs), g.new(shape, raw_dtype), g.new((C,)), g.new((C,))
    raw_call(dev, FAMILY[law] + "_merge_backward", rawd, gx, gl, xd, rawd, ad, bd, g1, gz, graw, ga, gb, B, C, H * W, ws, nbytes)
    h1, hz, hraw = g.new(hs), g.new(hs), g.new(shape, raw_dtype)
    raw_call(dev, FAMILY[law] + "_merge_backward", rawd, gx, None, xd, rawd, ad, bd, h1, hz, hraw, None, None, B, C, H * W, None, 0)
    torch.cuda.synchronize()
    assert not g.broken(), (law, shape, offset, g.broken())
    fn = backward_of(law)
    for got, want in zip((g1, gz, graw, ga, gb), fn(gx, gl, xd, rawd, ad, bd)):
        assert same_bits(got.float(), want.float())
    for got, want in zip((h1, hz, hraw), fn(gx, None, xd, rawd, ad, bd, need_ga=False, need_gb=False)):
        assert same_bits(got.float(), want.float())
    report("merge_backward", case="guards", law=law, shape=list(shape), raw=str(raw_dtype).replace("torch.", ""), offset=offset,
           guard_elements=sum(b.numel() - v.numel() for b, v, _ in g.kept))


@pytest.mark.parametrize("law,raw_dtype", LAWS, ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_the_images_of_a_batch_are_isolated(shape, offset, law, raw_dtype, dev):
    """NaN in image 0's x and raw: the per-pixel outputs of the other images keep their bits (and image 0 shows the NaN)."""
    reaches(shape, offset)
    fn = backward_of(law)
    (_, _, raw, _, _, _, _), _, _ = kernel_case(law, shape, raw_dtype)
    clean_args = on_device(law, shape, offset, raw_dtype, dev)
    clean = fn(*clean_args)[:3]
    xp, rawp = clean_args[2].cpu().clone(), raw.clone()
    xp[0, -1, 0, 0] = float("nan")
    rawp[0, 0, -1, -1] = float("nan")
    dirty = fn(*on_device(law, shape, offset, raw_dtype, dev, raw=rawp, x=xp))[:3]
    torch.cuda.synchronize()
    for k, (c, d) in enumerate(zip(clean, dirty)):
        assert bool(torch.isfinite(c.float()).all()), NAMES[k]
        assert same_bits(c[1:].float(), d[1:].float()), (NAMES[k], "another image changed")
    assert not bool(torch.isfinite(dirty[1][0]).all()) and not bool(torch.isfinite(dirty[2][0].float()).all())


def test_an_empty_batch_launches_nothing(dev, monkeypatch):
    from fincflow_amd import ops
    calls = record_calls(monkeypatch)
    x = torch.empty(0, 4, 5, 3, device=dev)
    a = torch.ones(4, device=dev)
    for fn in (ops.finc_split_prior_merge_backward, ops.finc_gauss_split_merge_backward):
        got = fn(x, torch.empty(0, device=dev), x, x.clone(), a, a)
        assert got[0].shape == got[1].shape == (0, 2, 5, 3) and got[2].shape == x.shape
        assert not bool(got[3].any()) and not bool(got[4].any())
        with pytest.raises(ValueError):
            fn(None, None, x, x.clone(), a, a)
    assert calls == []


def test_a_bf16_raw_is_refused_by_the_gaussianized_split(dev):
    from fincflow_amd import ops
    x = torch.randn(2, 4, 3, 3, device=dev)
    a = torch.ones(4, device=dev)
    with pytest.raises(ValueError):
        ops.finc_gauss_split_merge_backward(x, None, x, x.bfloat16(), a, a)


@pytest.mark.parametrize("law", ["prior", "gauss"])
def test_the_autograd_function_hands_absent_gradients_over_as_null(law, dev, monkeypatch):
    from fincflow_amd import ops
    shape = (3, 6, 3, 5)
    (x1, z2, raw, a, b, gx, gl), _, terms = kernel_case(law, shape, torch.float32)
    name = "finc_split_prior_merge_backward" if law == "prior" else "finc_gauss_split_merge_backward"
    seen, real = [], getattr(ops, name)

    def spy(grad_x, grad_log_p, *args, **kwargs):
        seen.append((grad_x is not None, grad_log_p is not None, tuple(kwargs[k] for k in sorted(kwargs))))
        return real(grad_x, grad_log_p, *args, **kwargs)
    monkeypatch.setattr(ops, name, spy)
    apply = ops.split_prior_merge if law == "prior" else ops.gauss_split_merge
    for present in PRESENT:
        leaves = [v.to(dev).requires_grad_(True) for v in (x1, z2, raw, a, b)]
        outs = apply(*leaves, want_log_p=True)
        assert type(outs[0].grad_fn).__name__ == FUNCTION[law] + "Backward" and outs[1].shape == (shape[0],)
        loss = sum((o * g.to(dev)).sum() for o, g, p in zip(outs, (gx, gl), present) if p)
        got = torch.autograd.grad(loss, leaves)
        assert seen[-1][:2] == present and all(seen[-1][2]), (seen[-1], present)
        judge("function", law, shape, torch.float32, NAMES, got, want_grads(terms, present), present=list(present))
    # without log p the Function has one result; only what needs a gradient is computed (need_* in keyword order: ga, gb, graw, gx1, gz2)
    leaves = [v.to(dev) for v in (x1, z2, raw, a, b)]
    leaves[1].requires_grad_(True)
    out = apply(*leaves)
    assert torch.is_tensor(out) and torch.equal(out, merge_of(law)(*leaves))
    got, = torch.autograd.grad((out * gx.to(dev)).sum(), [leaves[1]])
    assert seen[-1] == (True, False, (False, False, False, False, True)), seen[-1]
    judge("function_z2_only", law, shape, torch.float32, NAMES[1:2], [got], want_grads(terms, (True, False))[1:2])


# ---------------------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------------------
B, SIZE = 3, (12, 6, 6)
RELU = "finc_bias_relu_f32"


def module_of(kind):
    from fincflow_amd import glow
    if kind == "SplitPrior":
        m = glow.SplitPrior(SIZE, glow.GaussianPrior, width=32)
        cpl.fill(m.transform)
        return m
    return gauss.fill(glow.Split(SIZE, glow.GaussianPrior))


def halves(seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, SIZE[0] // 2, *SIZE[1:], generator=g), torch.randn(B, SIZE[0] // 2, *SIZE[1:], generator=g),
            torch.randn(B, *SIZE, generator=g), torch.randn(B, generator=g))


def module_grads(m, x1, z2, gx, gl, ctx):
    """x, log_p of a recorded merge and the gradients of sum(x * gx) + sum(log_p * gl) for x1, z2 and every parameter."""
    names, params = zip(*m.named_parameters())
    a, b = x1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    with ctx():
        x, lp = m.merge(a, b, with_log_prob=True)
    grads = torch.autograd.grad((x * gx).sum() + (lp * gl).sum(), (a, b) + params)
    return ("x1", "z2") + names, x.detach(), lp.detach(), grads


@pytest.mark.parametrize("kind", ["SplitPrior", "Split"])
def test_a_recorded_merge_is_one_launch_with_one_backward_launch(kind, dev, monkeypatch):
    import fincflow_amd
    m = module_of(kind)
    x1, z2, gx, gl = halves()
    m64, md = copy.deepcopy(m).double(), copy.deepcopy(m).to(dev)
    md.hip_recorded_merge = True
    entry = "finc_split_prior_merge" if kind == "SplitPrior" else "finc_gauss_split_merge"
    calls, cats = record_calls(monkeypatch), count_cats(monkeypatch)
    a, b = x1.to(dev).requires_grad_(True), z2.to(dev).requires_grad_(True)
    with flow_twin.recorded_masks(md) as masks:
        with fincflow_amd.reverse_grad():
            x, lp = md.merge(a, b, with_log_prob=True)
        assert calls == [entry + "_f32"] and not cats, (calls, cats)            # one merge launch, no cat
        assert type(x.grad_fn).__name__ == FUNCTION["prior" if kind == "SplitPrior" else "gauss"] + "Backward"
        del calls[:]
        names, params = zip(*md.named_parameters())
        got = torch.autograd.grad((x * gx.to(dev)).sum() + (lp * gl.to(dev)).sum(), (a, b) + params)
        assert calls == [entry + "_backward_f32"] and not cats, (calls, cats)   # one backward launch
    del calls[:]
    with flow_twin.replayed_masks(m64, masks):
        wnames, x64, lp64, want = module_grads(m64, x1.double(), z2.double(), gx.double(), gl.double(), torch.enable_grad)
    assert wnames == ("x1", "z2") + names
    judge("module", kind, (B,) + SIZE, torch.float32, ("x", "log_p"), (x, lp), (x64, lp64))
    judge("module_gradients", kind, (B,) + SIZE, torch.float32, wnames, got, want)
    assert all(float(w.abs().max()) > 0 for w in want)
    del calls[:], cats[:]                                                       # (the float64 module's own lines)

    # without log p, and with a drawn half through reverse / reverse_with_logdet (Split: `merge` on a draw, SplitPrior: its own lines)
    with fincflow_amd.reverse_grad():
        bare = md.merge(a, b)
        assert calls == [entry + "_f32"] and not cats and torch.equal(bare, x), (calls, cats)
        del calls[:]
        drawn = md.reverse_with_logdet(a)
    if kind == "Split":
        assert calls == [entry + "_f32"] and not cats, (calls, cats)
    else:
        assert calls == ["finc_coupling_reverse_logdet_f32"] and len(cats) == 1, (calls, cats)
    assert drawn[0].requires_grad and drawn[1].requires_grad


@pytest.mark.parametrize("kind", ["SplitPrior", "Split"])
def test_flag_off_or_outside_reverse_grad_the_call_lists_of_today(kind, dev, monkeypatch):
    import fincflow_amd
    md = module_of(kind).to(dev)
    x1, z2, _, _ = halves()
    a, b = x1.to(dev).requires_grad_(True), z2.to(dev)
    calls, cats = record_calls(monkeypatch), count_cats(monkeypatch)
    today = ["finc_coupling_reverse_logdet_f32"] if kind == "SplitPrior" else []
    lists = {}
    for flag in (False, True):
        if flag:
            md.hip_recorded_merge = True
        for ctx in ((torch.enable_grad,) if flag else (fincflow_amd.reverse_grad, torch.enable_grad)):
            with ctx():
                out, lq = md.merge(a, b, with_log_prob=True)
            assert out.requires_grad and lq.requires_grad and not any("merge" in c for c in calls), calls
            lists[(flag, ctx is torch.enable_grad)] = (list(calls), len(cats))
            del calls[:], cats[:]
    assert lists[(False, False)] == (today, 1), lists                           # flag off inside reverse_grad(): today's recorded lines
    assert lists[(True, True)] == lists[(False, True)] and lists[(False, True)][0] == [], lists     # outside it the flag changes nothing
    # without a graph the flag changes nothing either: the no-graph launch
    with torch.no_grad(), fincflow_amd.reverse_grad():
        md.merge(a, b, with_log_prob=True)
    assert calls[-1] == ("finc_split_prior_merge_f32" if kind == "SplitPrior" else "finc_gauss_split_merge_f32") and not cats, calls
    # float64 on the device with the flag set: the PyTorch lines
    del calls[:]
    m64d = copy.deepcopy(md).double()
    with fincflow_amd.reverse_grad():
        m64d.merge(a.double(), b.double(), with_log_prob=True)
    assert calls == [], calls


def test_under_bf16_autocast_the_split_prior_takes_the_rawbf16_entry_points(dev, monkeypatch):
    """Against the upcasting alternative (the coupling's HIP gate off, so that the PyTorch lines run on `raw.float()` under the same
    autocast): the bars of tests/test_gpu_autocast_modules.py."""
    import fincflow_amd
    from fincflow_amd import glow
    md = module_of("SplitPrior").to(dev)
    md.hip_recorded_merge = True
    x1, z2, gx, gl = (t.to(dev) for t in halves())
    calls = record_calls(monkeypatch)

    def ctx():
        stack = __import__("contextlib").ExitStack()
        stack.enter_context(torch.autocast("cuda", dtype=torch.bfloat16))
        stack.enter_context(fincflow_amd.reverse_grad())
        return stack
    names, x_on, lp_on, on = module_grads(md, x1, z2, gx, gl, ctx)
    assert calls == ["finc_split_prior_merge_rawbf16_f32", "finc_split_prior_merge_backward_rawbf16_f32"], calls
    assert x_on.dtype == lp_on.dtype == torch.float32 and all(g.dtype == torch.float32 for g in on)
    del calls[:]
    monkeypatch.setattr(glow.Coupling, "_hip_device", lambda self, x: False)
    _, x_off, lp_off, off = module_grads(md, x1, z2, gx, gl, ctx)
    assert calls == [], calls
    errs = {"x": rel_err(x_on.cpu().numpy(), x_off.cpu().numpy()), "log_p": rel_err(lp_on.cpu().numpy(), lp_off.cpu().numpy())}
    for n, g, w in zip(names, on, off):
        assert float(w.abs().max()) > 0, n
        errs["grad_" + n] = rel_err(g.cpu().numpy(), w.cpu().numpy())
    print("autocast", errs)
    report("merge_backward", case="module_bf16_autocast_against_upcast", bar=GRAD_BAR, **errs)
    for n, e in errs.items():
        assert e <= GRAD_BAR, (n, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_pair(gaussianize):
    """(the HIP model with the switch set, its float64 twin, x): two levels at 3x16x16, B = 4."""
    from fincflow_amd import glow
    torch.manual_seed(1)
    np.random.seed(1)
    model = glow.create_model(num_blocks=2, block_size=1, split_prior=True, gaussianize_split=gaussianize, actnorm=True,
                              preprocess=False, image_size=(3, 16, 16), coupling_width=16, hip_recorded_merge=True)
    flow_twin.randomise(model, seed=1, actnorm=True)
    for m in model.modules():
        if isinstance(m, glow.Gaussianize):
            gauss.fill(m, seed=2)
    model = model.to(torch.device("cuda:0"))
    bounds = [m for m in model.sequence_modules if isinstance(m, (glow.SplitPrior, glow.Split))]
    assert len(bounds) == 1 and bounds[0].hip_recorded_merge is True
    x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(7))
    return model, flow_twin.twin_of(model), x


def entries(gaussianize):
    family = "finc_gauss_split" if gaussianize else "finc_split_prior"
    return family + "_merge_f32", family + "_merge_backward_f32"


def compare(tag, names, got, want, bar, **fields):
    return flow_twin.compare(tag, names, got, want, bar=bar, kind="merge_backward", **fields)


def twin_grads(twin, names, loss, extra=()):
    tparams = [dict(twin.named_parameters())[n] for n in names]
    got = torch.autograd.grad(loss, list(extra) + tparams, allow_unused=True)
    masked = flow_twin.masked(twin, dict(zip(names, got[len(extra):])))
    return list(got[:len(extra)]) + [masked[n] for n in names]


def objective(x, log_q=None):
    """A loss on the sample and on its log-density: the reverse KL against a standard normal, as tests/test_gpu_train_loop.py has it."""
    e = 0.5 * x.square().flatten(1).sum(1)
    return (e if log_q is None else log_q + e).mean()


def judge_grads(tag, names, got, want, gaussianize):
    assert [n for n, g in zip(names, got) if g is None] == [n for n, g in zip(names, want) if g is None], tag
    keep = [k for k, g in enumerate(got) if g is not None]
    compare(tag, [names[k] for k in keep], [got[k] for k in keep], [want[k] for k in keep], TOL, gaussianize=gaussianize)
    return keep


@pytest.mark.parametrize("gaussianize", [False, True], ids=["split_prior", "gaussianized"])
def test_a_recorded_decode_against_the_twin(gaussianize, dev, monkeypatch):
    import fincflow_amd
    model, twin, x = model_pair(gaussianize)
    flow_twin.sync(twin, model)
    merge, merge_backward = entries(gaussianize)
    with torch.no_grad():
        zs = [z.detach() for z in model.encode(x.to(dev))[0]]
    calls = record_calls(monkeypatch)
    names, params = zip(*model.named_parameters())
    leaves = [z.clone().requires_grad_(True) for z in zs]
    with flow_twin.recorded_masks(model) as masks:
        with fincflow_amd.reverse_grad():
            out, log_q = model.decode(leaves, with_log_prob=True)
        assert calls.count(merge) == 1 and calls.count(merge_backward) == 0, calls
        got = torch.autograd.grad(objective(out, log_q), leaves + list(params), allow_unused=True)
    assert calls.count(merge_backward) == 1 and calls.count(merge) == 1, calls
    leaves64 = [z.double().cpu().requires_grad_(True) for z in zs]
    with flow_twin.replayed_masks(twin, masks):
        out64, log_q64 = twin.decode(leaves64, with_log_prob=True)
        want = twin_grads(twin, names, objective(out64, log_q64), leaves64)
    compare("decode/x", ["x"], [out], [out64], CHAIN_TOL, gaussianize=gaussianize)
    compare("decode/log_q", ["log_q"], [log_q], [log_q64], TOL, gaussianize=gaussianize)
    all_names = ["z%d" % k for k in range(len(zs))] + list(names)
    keep = judge_grads("decode/gradients", all_names, got, want, gaussianize)
    assert len(keep) == len(all_names)                                          # every latent and every parameter is reached


@pytest.mark.parametrize("gaussianize", [False, True], ids=["split_prior", "gaussianized"])
def test_a_tempered_rsample_against_the_twin_on_the_same_draws(gaussianize, dev, monkeypatch):
    model, twin, _ = model_pair(gaussianize)
    flow_twin.sync(twin, model)
    merge, merge_backward = entries(gaussianize)
    calls = record_calls(monkeypatch)
    names, params = zip(*model.named_parameters())
    torch.manual_seed(21)
    with flow_twin.recorded_noise(model) as draws, flow_twin.recorded_masks(model) as masks:
        out = model.rsample(4, temperature=0.7)
        got = torch.autograd.grad(objective(out), params, allow_unused=True)
    assert calls.count(merge) == 1 and calls.count(merge_backward) == 1 and len(draws) == 2, calls
    with flow_twin.replayed_noise(twin, draws), flow_twin.replayed_masks(twin, masks):
        out64 = twin.rsample(4, temperature=0.7)
        want = twin_grads(twin, names, objective(out64))
    compare("rsample_tempered/x", ["x"], [out], [out64], CHAIN_TOL, gaussianize=gaussianize)
    judge_grads("rsample_tempered/gradients", list(names), got, want, gaussianize)


def test_rsample_with_log_prob_through_the_gaussianized_split_against_the_twin(dev, monkeypatch):
    model, twin, _ = model_pair(True)
    flow_twin.sync(twin, model)
    merge, merge_backward = entries(True)
    calls = record_calls(monkeypatch)
    names, params = zip(*model.named_parameters())
    torch.manual_seed(22)
    with flow_twin.recorded_noise(model) as draws, flow_twin.recorded_masks(model) as masks:
        out, log_q = model.rsample_with_log_prob(4)
        got = torch.autograd.grad(objective(out, log_q), params, allow_unused=True)
    assert calls.count(merge) == 1 and calls.count(merge_backward) == 1 and len(draws) == 2, calls
    with flow_twin.replayed_noise(twin, draws), flow_twin.replayed_masks(twin, masks):
        out64, log_q64 = twin.rsample_with_log_prob(4)
        want = twin_grads(twin, names, objective(out64, log_q64))
    compare("rsample_with_log_prob/x", ["x"], [out], [out64], CHAIN_TOL, gaussianize=True)
    compare("rsample_with_log_prob/log_q", ["log_q"], [log_q], [log_q64], TOL, gaussianize=True)
    keep = judge_grads("rsample_with_log_prob/gradients", list(names), got, want, True)
    assert len(keep) == len(names)
    # a plain rsample on the same model takes the same path
    del calls[:]
    model.rsample(2).square().mean().backward()
    model.zero_grad(set_to_none=True)
    assert calls.count(merge) == 1 and calls.count(merge_backward) == 1, calls
