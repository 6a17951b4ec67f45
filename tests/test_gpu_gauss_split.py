"""The Gaussianized split on the GPU (include/finc.h: finc_gauss_split_f32, finc_gauss_split_merge_f32,
finc_gauss_split_backward_f32), `glow.Split.split` / `merge` and a two-level model through `FlowSequential.encode` / `decode`:
DESIGN 3.22.

References: the float64 formula on the CPU (m = h[:, 0::2], logs = h[:, 1::2], z2 = (x2 - m) exp(-logs), log p = -sum logs -
1/2 sum z2^2 - c) and float64 autograd through it; for the model, the float64 twin of tests/flow_twin.py (a deep copy in float64
on the CPU whose units run the reference formulas: the units have no CPU path of their own).  Bars: the project's 1e-5 in
helpers.rel_err (TOL), 5e-5 for a round trip (CHAIN_TOL).

The kernels are the split prior's bodies under another arithmetic law with its launch geometry, so the shapes, what each is here
for (`FORMS`) and the check in front of every kernel test (`reaches`) are those of tests/test_gpu_split_latent.py:
  (2, 4, 2, 2)        the 16-byte form, one part per image
  (3, 6, 3, 5)        HW = 15: the dword form
  (2, 12, 16, 16)     16-byte, P = 2 parts per image
  (512, 16, 24, 24)   P = 4 parts and a second trip of the thread loop (forward), Q = 256 parts and second trips (backward)
  (2, 12, 4, 4)       on views one float into their allocation: HW % 4 == 0 but the dword form
Inputs: raw = 0.5 randn -- what a 3x3 convolution with weights of scale 0.05 over some eight channels gives (0.05 * sqrt(72) = 0.42)
-- with a = exp(0.1 randn) and b = 0.1 randn * a, the scales of tests/test_split_latent_host.py::_split_prior: logs stays within
+-3 at five sigma, exp(+-logs) is O(1) to O(10).  Every case prints what it achieved and appends it to the parity report (kind
`gauss_split`)."""
import copy
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import flow_twin
from helpers import rel_err, report, same_bits
from test_gpu_split_latent import CASES, PRESENT, Guarded, count_cats, half_outs, mover, reaches, record_calls

pytestmark = pytest.mark.gpu

TOL = 1e-5
CHAIN_TOL = 5e-5
NAMES = ("grad_x", "grad_raw", "grad_a", "grad_b")
LOG_2PI = math.log(2.0 * math.pi)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# references (float64 on the CPU, once per shape)
# ---------------------------------------------------------------------------------------------------------------------------------
def formula(x, raw, a, b):
    """float64: (x1, z2, log_p) of the split, and logs."""
    half = x.shape[1] // 2
    h = a.view(1, -1, 1, 1) * raw + b.view(1, -1, 1, 1)
    m, logs = h[:, 0::2], h[:, 1::2]
    z2 = (x[:, half:] - m) * torch.exp(-logs)
    c = 0.5 * z2[0].numel() * LOG_2PI
    return x[:, :half], z2, -logs.flatten(1).sum(1) - 0.5 * z2.square().flatten(1).sum(1) - c


@functools.lru_cache(maxsize=None)
def kernel_case(shape):
    """fp32 inputs (a, b rounded to fp32 once: the reference starts from the kernel's numbers), grad_x1 / grad_z2 / grad_log_p, the
    float64 results, and the float64 gradients of each of the three terms sum(x1 * grad_x1), sum(z2 * grad_z2),
    sum(log_p * grad_log_p) on their own (the backward is linear in them: an absent incoming gradient is its term left out)."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(1000 + sum(shape))
    x, gy = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    gl = torch.randn(B, generator=gen)
    raw = 0.5 * torch.randn(B, C, H, W, generator=gen)
    a = torch.exp(0.1 * torch.randn(C, generator=gen).double())
    b = (0.1 * torch.randn(C, generator=gen).double() * a).float()
    a = a.float()
    half = C // 2
    g1, g2 = gy[:, :half].contiguous(), gy[:, half:].contiguous()
    leaves = [v.double().requires_grad_(True) for v in (x, raw, a, b)]
    x1, z2, log_p = formula(*leaves)
    terms = []
    for out, g in ((x1, g1), (z2, g2), (log_p, gl)):
        got = torch.autograd.grad((out * g.double()).sum(), leaves, retain_graph=True, allow_unused=True)
        terms.append([torch.zeros_like(v) if t is None else t for t, v in zip(got, leaves)])
    assert float(log_p.detach().abs().max()) > 0.1 and float((z2.detach() - x[:, half:].double()).abs().max()) > 0.1
    return (x, raw, a, b, g1, g2, gl), [v.detach() for v in (x1, z2, log_p)], terms


def want_grads(terms, present):
    return [sum(t[k] for t, p in zip(terms, present) if p).numpy() for k in range(4)]


def judge(kind, shape, names, got, ref, tol=TOL, **fields):
    errs = {n: rel_err(g.detach().float().cpu().numpy(), np.asarray(r)) for n, g, r in zip(names, got, ref)}
    print(kind, shape, errs)
    report("gauss_split", case=kind, shape=list(shape), **errs, **fields)
    for n, e in errs.items():
        assert e <= tol, (kind, shape, n, e)
    return errs


def on_device(shape, offset, dev):
    (x, raw, a, b, g1, g2, gl), _, _ = kernel_case(shape)
    move = mover(dev, offset)
    return move(x), move(raw), a.to(dev), b.to(dev), move(g1), move(g2), gl.to(dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# the split and the merge
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_split_and_merge_against_the_float64_formula(shape, offset, dev):
    from fincflow_amd import ops
    reaches(shape, offset)
    _, (x1_ref, z2_ref, lp_ref), _ = kernel_case(shape)
    xd, rawd, ad, bd, _, _, _ = on_device(shape, offset, dev)
    half, move = shape[1] // 2, mover(dev, offset)
    if offset:
        assert all(v.data_ptr() % 16 == 4 for v in (xd, rawd)) and (shape[2] * shape[3]) % 4 == 0
    x1, z2, lp = ops.finc_gauss_split(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
    x1b, z2b, lpb = ops.finc_gauss_split(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
    assert torch.equal(x1, xd[:, :half])                                           # the kept half: the input's bits
    assert same_bits(x1, x1b) and same_bits(z2, z2b) and same_bits(lp, lpb)         # fixed-order sums: two runs, the same bits
    assert lp.shape == (shape[0],)

    back, lpm = ops.finc_gauss_split_merge(x1, z2, rawd, ad, bd, want_log_p=True, out=move(torch.zeros(shape)))
    back2, lpm2 = ops.finc_gauss_split_merge(x1, z2, rawd, ad, bd, want_log_p=True, out=move(torch.zeros(shape)))
    bare = ops.finc_gauss_split_merge(x1, z2, rawd, ad, bd, out=move(torch.zeros(shape)))
    torch.cuda.synchronize()
    assert same_bits(back, back2) and same_bits(lpm, lpm2) and same_bits(bare, back)
    assert torch.equal(back[:, :half], x1)
    # the merge reports the split's value at its result: the formula on the z2 it was handed
    (x, raw, a, b, _, _, _), _, _ = kernel_case(shape)
    z2_given = z2.double().cpu()
    h = a.double().view(1, -1, 1, 1) * raw.double() + b.double().view(1, -1, 1, 1)
    merged_ref = torch.cat([x1.double().cpu(), z2_given * torch.exp(h[:, 1::2]) + h[:, 0::2]], 1)
    lpm_ref = lp_ref + 0.5 * z2_ref.square().flatten(1).sum(1) - 0.5 * z2_given.square().flatten(1).sum(1)
    judge("split" + ("_offset" if offset else ""), shape, ("x1", "z2", "log_p", "merge", "merge_log_p"),
          (x1, z2, lp, back, lpm), (x1_ref, z2_ref, lp_ref, merged_ref, lpm_ref))
    judge("round_trip" + ("_offset" if offset else ""), shape, ("x",), (back,), (x.double(),), tol=CHAIN_TOL)


def test_an_empty_batch_launches_nothing(dev, monkeypatch):
    from fincflow_amd import ops
    calls = record_calls(monkeypatch)
    x = torch.empty(0, 4, 5, 3, device=dev)
    a = torch.ones(4, device=dev)
    x1, z2, lp = ops.finc_gauss_split(x, x.clone(), a, a)
    assert x1.shape == z2.shape == (0, 2, 5, 3) and lp.shape == (0,)
    back, lpm = ops.finc_gauss_split_merge(x1, z2, x.clone(), a, a, want_log_p=True)
    assert back.shape == x.shape and lpm.shape == (0,)
    got = ops.finc_gauss_split_backward(x1, z2, lp, x, x.clone(), a, a)
    assert got[0].shape == x.shape and not bool(got[2].any()) and not bool(got[3].any()) and calls == []


def test_a_bf16_raw_is_refused(dev):
    from fincflow_amd import ops
    xd, rawd, ad, bd, _, _, _ = on_device((2, 4, 2, 2), False, dev)
    with pytest.raises(ValueError):
        ops.finc_gauss_split(xd, rawd.bfloat16(), ad, bd)


def raw_call(dev, name, *args):
    from fincflow_amd import ops
    ops._call(name + "_f32", dev, *[None if a is None else (a.data_ptr() if torch.is_tensor(a) else a) for a in args],
              ops._stream_ptr(args[0]))


@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_guard_bands_around_every_output_are_intact(shape, offset, dev):
    """The three entry points called directly, every output and the workspace between guard bands: nothing is written beyond a
    tensor, the results are those of the plain calls, and a merge without log p leaves the workspace alone."""
    from fincflow_amd import _lib, ops
    xd, rawd, ad, bd, g1, g2, gl = on_device(shape, offset, dev)
    B, C, H, W = shape
    hs = (B, C // 2, H, W)
    nbytes = _lib.lib().finc_coupling_workspace_bytes(B, C, H * W)
    g = Guarded(dev, 1 if offset else 0)
    ws, untouched = g.new((nbytes // 4,)), g.new((nbytes // 4,))
    x1, z2, lp = g.new(hs), g.new(hs), g.new((B,))
    raw_call(dev, "finc_gauss_split", xd, rawd, ad, bd, x1, z2, lp, B, C, H * W, ws, nbytes)
    back, lpm, bare = g.new(shape), g.new((B,)), g.new(shape)
    raw_call(dev, "finc_gauss_split_merge", x1, z2, rawd, ad, bd, back, lpm, B, C, H * W, ws, nbytes)
    raw_call(dev, "finc_gauss_split_merge", x1, z2, rawd, ad, bd, bare, None, B, C, H * W, untouched, nbytes)
    gx, graw, ga, gb = g.new(shape), g.new(shape), g.new((C,)), g.new((C,))
    raw_call(dev, "finc_gauss_split_backward", g1, g2, gl, xd, rawd, ad, bd, gx, graw, ga, gb, B, C, H * W, ws, nbytes)
    torch.cuda.synchronize()
    assert not g.broken(), (shape, offset, g.broken())
    assert not bool(untouched.any())                                               # NULL log p: no partials were written
    plain = ops.finc_gauss_split(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
    for got, want in zip((x1, z2, lp), plain):
        assert same_bits(got, want)
    pm = ops.finc_gauss_split_merge(plain[0], plain[1], rawd, ad, bd, want_log_p=True, out=mover(dev, offset)(torch.zeros(shape)))
    assert same_bits(back, pm[0]) and same_bits(lpm, pm[1]) and same_bits(bare, pm[0])
    for got, want in zip((gx, graw, ga, gb), ops.finc_gauss_split_backward(g1, g2, gl, xd, rawd, ad, bd)):
        assert same_bits(got, want)
    report("gauss_split", case="guards", shape=list(shape), offset=offset,
           guard_elements=sum(b.numel() - v.numel() for b, v, _ in g.kept))


@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_the_images_of_a_batch_are_isolated(shape, offset, dev):
    """NaN in image 0's x and raw: every per-image output of the other images keeps its bits (and image 0 shows the NaN)."""
    from fincflow_amd import ops
    (x, raw, a, b, g1, g2, gl), _, _ = kernel_case(shape)
    move = mover(dev, offset)

    def every(x, raw):
        xd, rawd, ad, bd = move(x), move(raw), a.to(dev), b.to(dev)
        x1, z2, lp = ops.finc_gauss_split(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
        back, lpm = ops.finc_gauss_split_merge(x1, z2, rawd, ad, bd, want_log_p=True, out=move(torch.zeros(shape)))
        gx, graw, _, _ = ops.finc_gauss_split_backward(move(g1), move(g2), gl.to(dev), xd, rawd, ad, bd)
        return x1, z2, lp, back, lpm, gx, graw
    clean = every(x, raw)
    xp, rawp = x.clone(), raw.clone()
    xp[0, -1, 0, 0] = float("nan")
    rawp[0, 0, -1, -1] = float("nan")
    dirty = every(xp, rawp)
    for k, (c, d) in enumerate(zip(clean, dirty)):
        assert bool(torch.isfinite(c).all()), k
        assert same_bits(c[1:], d[1:]), (k, "another image changed")
    assert not bool(torch.isfinite(dirty[2][0])) and not bool(torch.isfinite(dirty[4][0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_all_four_gradients_against_float64_autograd(shape, offset, dev):
    """With all three incoming gradients, and with each absent (NULL) in turn."""
    from fincflow_amd import ops
    reaches(shape, offset)
    _, _, terms = kernel_case(shape)
    xd, rawd, ad, bd, g1, g2, gl = on_device(shape, offset, dev)
    for present in PRESENT:
        given = [g if p else None for g, p in zip((g1, g2, gl), present)]
        got = ops.finc_gauss_split_backward(*given, xd, rawd, ad, bd)
        again = ops.finc_gauss_split_backward(*given, xd, rawd, ad, bd)
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(got, again))
        judge("backward" + ("_offset" if offset else ""), shape, NAMES, got, want_grads(terms, present), present=list(present))


@pytest.mark.parametrize("shape", [(3, 6, 3, 5), (2, 12, 16, 16)], ids=str)
def test_every_combination_of_skipped_outputs(shape, dev):
    from fincflow_amd import ops
    xd, rawd, ad, bd, g1, g2, gl = on_device(shape, False, dev)
    full = ops.finc_gauss_split_backward(g1, g2, gl, xd, rawd, ad, bd)
    for need in itertools.product((True, False), repeat=4):
        got = ops.finc_gauss_split_backward(g1, g2, gl, xd, rawd, ad, bd, *need)
        for n, g, f, name in zip(need, got, full, NAMES):
            assert (g is not None) == n, (need, name)
            if n:
                assert same_bits(g, f), (need, name)
    assert ops.finc_gauss_split_backward(g1, g2, gl, xd, rawd, ad, bd, False, False, False, False) == (None,) * 4


def test_the_autograd_function_hands_absent_gradients_over_as_null(dev, monkeypatch):
    from fincflow_amd import ops
    shape = (3, 6, 3, 5)
    (x, raw, a, b, g1, g2, gl), _, terms = kernel_case(shape)
    seen = []
    real = ops.finc_gauss_split_backward

    def spy(grad_x1, grad_z2, grad_log_p, *args, **kwargs):
        seen.append((grad_x1 is not None, grad_z2 is not None, grad_log_p is not None))
        return real(grad_x1, grad_z2, grad_log_p, *args, **kwargs)
    monkeypatch.setattr(ops, "finc_gauss_split_backward", spy)
    for present in PRESENT[1:] + [(False, False, True)]:
        leaves = [v.to(dev).requires_grad_(True) for v in (x, raw, a, b)]
        outs = ops.gauss_split_forward(*leaves)
        assert type(outs[0].grad_fn).__name__ == "_FincGaussSplitFunctionBackward"
        loss = sum((o * g.to(dev)).sum() for o, g, p in zip(outs, (g1, g2, gl), present) if p)
        got = torch.autograd.grad(loss, leaves)
        assert seen[-1] == present, (seen[-1], present)
        judge("function", shape, NAMES, got, want_grads(terms, present), present=list(present))


# ---------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------
def fill(m, seed=11):
    """0.05, and 0.1 for biases and log-scales: tests/test_split_latent_host.py::_split_prior."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if name.endswith(("bias", "log_scale_factor")) else 0.05))
    return m


def count_convs(monkeypatch):
    import torch.nn.functional as F
    convs, real = [], F.conv2d

    def conv2d(*args, **kwargs):
        convs.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(F, "conv2d", conv2d)
    return convs


def test_which_calls_the_module_makes(dev, monkeypatch):
    import fincflow_amd
    from fincflow_amd import glow
    B, size = 3, (12, 6, 6)
    m = fill(glow.Split(size, glow.GaussianPrior))
    torch.manual_seed(3)
    x = torch.randn(B, *size)
    m64, md = copy.deepcopy(m).double(), copy.deepcopy(m).to(dev)
    with torch.no_grad():
        x1_ref, z2_ref, lp_ref = m64.split(x.double())
        assert float((z2_ref - x[:, 6:].double()).abs().max()) > 0.05             # (not the identity layer)
    calls, cats, convs = record_calls(monkeypatch), count_cats(monkeypatch), count_convs(monkeypatch)
    xd = x.to(dev)

    # without a graph: ONE convolution and ONE launch per split / merge, no cat
    with torch.no_grad():
        x1, z2, lp = md.split(xd)
        assert calls == ["finc_gauss_split_f32"] and len(convs) == 1 and not cats, (calls, convs, cats)
        del calls[:], convs[:]
        back, lpm = md.merge(x1, z2, with_log_prob=True)
        assert calls == ["finc_gauss_split_merge_f32"] and len(convs) == 1 and not cats, (calls, convs, cats)
        del calls[:], convs[:]
        bare = md.merge(x1, z2)
        first, lpf = md(xd)
        assert calls == ["finc_gauss_split_merge_f32", "finc_gauss_split_f32"] and len(convs) == 2 and not cats, (calls, convs, cats)
        del calls[:], convs[:]
    judge("module", (B,) + size, ("x1", "z2", "log_p", "merge_log_p"), (x1, z2, lp, lpm), (x1_ref, z2_ref, lp_ref, lp_ref))
    judge("module_round_trip", (B,) + size, ("x",), (back,), (x.double(),), tol=CHAIN_TOL)
    assert torch.equal(bare, back) and torch.equal(first, x1) and torch.equal(lpf, lp)

    # while autograd records: the split's Function and its one backward launch
    xa = xd.clone().requires_grad_(True)
    x1g, z2g, lpg = md.split(xa)
    assert calls == ["finc_gauss_split_f32"] and type(lpg.grad_fn).__name__ == "_FincGaussSplitFunctionBackward", calls
    del calls[:]
    (-lpg.mean() + z2g.square().mean() + x1g.sum()).backward()
    assert calls == ["finc_gauss_split_backward_f32"], calls
    xw = x.double().requires_grad_(True)
    w1, w2, wlp = m64.split(xw)
    (-wlp.mean() + w2.square().mean() + w1.sum()).backward()
    names, params = zip(*md.named_parameters())
    judge("module_gradients", (B,) + size, ("x",) + names, (xa.grad,) + tuple(p.grad for p in params),
          (xw.grad,) + tuple(dict(m64.named_parameters())[n].grad for n in names))
    del calls[:], cats[:]

    # a recorded merge (inside reverse_grad() too) keeps the PyTorch lines: no call into the new entry points
    for ctx in (fincflow_amd.reverse_grad, torch.enable_grad):
        with ctx():
            out, lq = md.merge(x1.clone().requires_grad_(True), z2, with_log_prob=True)
        assert calls == [] and len(cats) == 1 and out.requires_grad and lq.requires_grad, (calls, cats)
        assert rel_err(out.detach().cpu().numpy(), x.numpy()) <= CHAIN_TOL
        del cats[:]

    # float64 on the device: the PyTorch lines
    m64d = copy.deepcopy(m).double().to(dev)
    with torch.no_grad():
        a1, a2, alp = m64d.split(xd.double())
        aback = m64d.merge(a1, a2)
    assert calls == []
    assert rel_err(alp.cpu().numpy(), lp_ref.numpy()) <= 1e-12 and rel_err(aback.cpu().numpy(), x.double().numpy()) <= 1e-12


def test_the_scale_and_shift_are_cached_per_parameter_version(dev):
    from fincflow_amd import glow
    md = fill(glow.Split((4, 4, 4), glow.GaussianPrior)).to(dev)
    g = md.gaussianize
    x = torch.randn(2, 4, 4, 4, device=dev)
    with torch.no_grad():
        before = md.split(x)
        a = g._ab[0]
        assert md.split(x)[2].equal(before[2]) and g._ab[0] is a
        g.log_scale_factor.add_(0.5)
        after = md.split(x)
    assert g._ab[0] is not a and not torch.equal(after[1], before[1])
    assert not any(k in copy.deepcopy(g).__dict__ for k in g._derived)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev):
    """(the HIP model, its float64 twin, x): two levels at 3x16x16, B = 4, a Gaussianized split between them."""
    from fincflow_amd import glow
    torch.manual_seed(1)
    np.random.seed(1)
    model = glow.create_model(num_blocks=2, block_size=1, split_prior=True, gaussianize_split=True, actnorm=True, preprocess=False,
                              image_size=(3, 16, 16), coupling_width=16)
    flow_twin.randomise(model, seed=1, actnorm=True)
    for m in model.modules():
        if isinstance(m, glow.Gaussianize):
            fill(m, seed=2)
    model = model.to(dev)
    x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(7))
    return model, flow_twin.twin_of(model), x


def compare(tag, names, got, want, bar):
    return flow_twin.compare(tag, names, got, want, bar=bar, kind="gauss_split")


def test_encode_against_the_twin(models, dev, monkeypatch):
    model, twin, x = models
    calls = record_calls(monkeypatch)
    with torch.no_grad():
        zs, log_prob = model.encode(x.to(dev))
        log_prob_forward = model.log_prob(x.to(dev))
        zs64, lp64 = twin.encode(x.double())
    assert calls.count("finc_gauss_split_f32") == 2 and [tuple(z.shape) for z in zs] == [(4, 6, 8, 8), (4, 24, 4, 4)], calls
    compare("encode", ["z0", "z1", "log_prob", "log_prob_of_forward"], zs + [log_prob, log_prob_forward], zs64 + [lp64, lp64], TOL)


def test_gradients_of_the_encode_loss_against_the_twin(models, dev, monkeypatch):
    model, twin, x = models
    flow_twin.sync(twin, model)
    calls = record_calls(monkeypatch)
    names, params = zip(*model.named_parameters())
    with flow_twin.recorded_masks(model) as masks:
        loss = -model.encode(x.to(dev))[1].mean()
        got = torch.autograd.grad(loss, params)
    assert calls.count("finc_gauss_split_f32") == 1 and calls.count("finc_gauss_split_backward_f32") == 1, calls
    tparams = [dict(twin.named_parameters())[n] for n in names]
    with flow_twin.replayed_masks(twin, masks):
        loss64 = -twin.encode(x.double())[1].mean()
        want = flow_twin.masked(twin, dict(zip(names, torch.autograd.grad(loss64, tparams))))
    assert any("gaussianize" in n for n in names)
    compare("encode_loss", ["loss"], [loss], [loss64], TOL)
    compare("encode_gradients", list(names), list(got), [want[n] for n in names], TOL)


def test_decode_of_encode_is_the_input(models, dev, monkeypatch):
    model, twin, x = models
    with torch.no_grad():
        zs, log_prob = model.encode(x.to(dev))
        calls = record_calls(monkeypatch)
        back, log_q = model.decode(zs, with_log_prob=True)
        assert calls.count("finc_gauss_split_merge_f32") == 1, calls
        bare = model.decode(zs)
        want_q = twin.log_prob(twin.decode([z.double().cpu() for z in zs]))
    assert torch.equal(bare, back)
    compare("round_trip", ["x"], [back], [x.double()], CHAIN_TOL)
    compare("decode_log_q", ["log_q", "log_q_of_encode"], [log_q, log_q], [want_q, log_prob.double().cpu()], TOL)


def test_decode_of_tempered_latents_against_the_twin(models, dev):
    model, twin, _ = models
    with torch.no_grad():
        torch.manual_seed(21)
        zs = model.draw_latents(4, temperature=0.7)
        x = model.decode(zs)
        torch.manual_seed(21)
        sampled = model.sample(4, temperature=0.7)[0]
        want = twin.decode([z.double().cpu() for z in zs])
    assert len(zs) == 2 and torch.equal(x, sampled)
    compare("tempered_decode", ["x"], [x], [want], TOL)


def test_the_round_trip_under_bf16_autocast(models, dev, monkeypatch):
    """Both directions run the boundary's convolution in bf16 on the same x1 and upcast it: they see the same raw."""
    model, _, x = models
    calls = record_calls(monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        zs, _ = model.encode(x.to(dev))
        back = model.decode(zs)
    assert calls.count("finc_gauss_split_f32") == 1 and calls.count("finc_gauss_split_merge_f32") == 1, calls
    assert all(z.dtype == torch.float32 for z in zs) and back.dtype == torch.float32
    compare("round_trip_bf16_autocast", ["x"], [back], [x.double()], CHAIN_TOL)


def test_a_captured_decode_replays_with_the_bits_of_the_eager_call(models, dev):
    from fincflow_amd import _lib
    model, _, x = models
    with torch.no_grad():
        zs, _ = model.encode(x.to(dev))
        eager, eager_q = model.decode(zs, with_log_prob=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, log_q = model.decode(zs, with_log_prob=True)
        for _ in range(2):
            out.zero_(), log_q.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager) and torch.equal(log_q, eager_q)
    assert not _lib.fault_pending()
