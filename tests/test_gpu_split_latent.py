"""The split prior with its latent on the GPU (include/finc.h: finc_split_prior_f32, finc_split_prior_merge_f32,
finc_split_prior_backward_f32 and their _rawbf16_f32 siblings), `glow.SplitPrior.split` / `merge` and
`FlowSequential.encode` / `decode` / `draw_latents` / `sample(temperature=)`: DESIGN 3.20.

References: for bits, the coupling's own kernels (`ops.finc_coupling` in both directions: the split and the merge are the same
arithmetic lines with other pointers); for values, the float64 formula (x1, z2, sum s - 1/2 sum z2^2 - c) on the CPU and float64
autograd through it; for the model, the float64 twin of tests/flow_twin.py.  Bars: the project's 1e-5 in helpers.rel_err (TOL), 5e-5
for the fp32 round trip through a whole model (the bar `reconstruct` has in tests/test_gpu_stack_orders.py).

Kernel shapes, with the launch counts recomputed here from cpl_parts (fincflow_amd/csrc/finc_coupling.h: parts = min(ceil(items /
256), ceil(2048 / outer)); with CPL_THREADS and CPL_CHIP_WGS read from that file; `reaches` asserts them in front of the kernel tests):
  (2, 4, 2, 2)        the 16-byte form, 2 items, one part per image
  (3, 6, 3, 5)        HW = 15: the dword form
  (2, 12, 16, 16)     16-byte; items = 6 * 64 = 384: P = 2 parts per image
  (512, 16, 24, 24)   forward: 1,152 items on P = min(5, ceil(2048 / 512)) = 4 parts of 256 threads, a second trip of the thread loop;
                      backward: 73,728 items per channel pair on Q = min(288, ceil(2048 / 8)) = 256 parts, second trips there too;
                      19 MB per tensor
  (2, 12, 4, 4)       on views one float into their allocation: HW % 4 == 0 but the dword form
Every case prints what it achieved and appends it to the parity report (kind `split_latent`).
"""
import copy
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import flow_twin
import test_gpu_coupling as cpl
from helpers import guarded, guards_intact, offset_view, rel_err, report, same_bits
from test_gpu_autocast_kernels import guarded16, guards16_intact

pytestmark = pytest.mark.gpu

TOL = 1e-5
CHAIN_TOL = 5e-5
SHAPES = [(2, 4, 2, 2), (3, 6, 3, 5), (2, 12, 16, 16), (512, 16, 24, 24)]
OFFSET = (2, 12, 4, 4)
CASES = [(s, False) for s in SHAPES] + [(OFFSET, True)]
RAWS = [torch.float32, torch.bfloat16]
NAMES = ("grad_x", "grad_raw", "grad_a", "grad_b")
LOG_2PI = math.log(2.0 * math.pi)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def launch_constants():
    """(CPL_THREADS, CPL_CHIP_WGS) as fincflow_amd/csrc/finc_coupling.h has them: the counts below follow the kernel file's numbers."""
    import os
    import re
    from helpers import REPO
    text = open(os.path.join(REPO, "fincflow_amd", "csrc", "finc_coupling.h")).read()
    threads = int(re.search(r"constexpr int CPL_THREADS = (\d+);", text).group(1))
    wgs = re.search(r"constexpr long long CPL_CHIP_WGS = (\d+) \* (\d+);", text)
    return threads, int(wgs.group(1)) * int(wgs.group(2))


def cpl_parts(items, outer):
    threads, chip = launch_constants()
    return max(1, min(-(-items // threads), -(-chip // outer)))


def launch_form(shape, offset=False):
    """(wide, P, trips of the forward's thread loop, Q, trips of the backward's) -- cpl_launch's and cpl_grad_plan's arithmetic."""
    B, C, H, W = shape
    threads = launch_constants()[0]
    wide = (H * W) % 4 == 0 and not offset
    nv = H * W // (4 if wide else 1)
    P, Q = cpl_parts(C // 2 * nv, B), cpl_parts(B * nv, C // 2)
    return wide, P, -(-(C // 2 * nv) // (P * threads)), Q, -(-(B * nv) // (Q * threads))


#: what each shape is here for; every kernel test asserts it of its shape before it runs (`reaches`), so a change of the kernel
#: file's constants that moves a shape off its form fails the tests that rely on it
FORMS = {((2, 4, 2, 2), False): (True, 1, 1, 1, 1), ((3, 6, 3, 5), False): (False, 1, 1, 1, 1), ((2, 12, 16, 16), False): (True, 2, 1, 1, 1),
         ((512, 16, 24, 24), False): (True, 4, 2, 256, 2), (OFFSET, True): (False, 1, 1, 1, 1)}


def reaches(shape, offset):
    assert launch_form(shape, offset) == FORMS[(shape, offset)], (shape, offset, launch_form(shape, offset))
    assert shape != OFFSET or launch_form(OFFSET)[0] is True                  # (aligned, it would be the 16-byte form)


# ---------------------------------------------------------------------------------------------------------------------------------
# references (float64 on the CPU, once per shape and raw type)
# ---------------------------------------------------------------------------------------------------------------------------------
def formula(x, raw, a, b):
    """float64: (x1, z2, log_p) of the split."""
    half = x.shape[1] // 2
    h = a.view(1, -1, 1, 1) * raw + b.view(1, -1, 1, 1)
    s, t = 2.0 * torch.tanh(h[:, ::2] / 2.0), h[:, 1::2]
    z2 = x[:, half:] * torch.exp(s) + t
    c = 0.5 * z2[0].numel() * LOG_2PI
    return x[:, :half], z2, s.flatten(1).sum(1) - 0.5 * z2.square().flatten(1).sum(1) - c


@functools.lru_cache(maxsize=None)
def kernel_case(shape, raw_dtype):
    """The inputs of tests/test_gpu_coupling.py (raw rounded to `raw_dtype` first: the reference starts from the kernel's numbers),
    grad_x1 / grad_z2 / grad_log_p, the float64 results, and the float64 gradients of each of the three terms
    sum(x1 * grad_x1), sum(z2 * grad_z2), sum(log_p * grad_log_p) on their own (the backward is linear in them: an absent incoming
    gradient is its term left out)."""
    x, raw, a, b, gy, gl = cpl.case(shape)
    raw = raw.to(raw_dtype)
    half = shape[1] // 2
    g1, g2 = gy[:, :half].contiguous(), gy[:, half:].contiguous()
    leaves = [v.double().requires_grad_(True) for v in (x, raw, a, b)]
    x1, z2, log_p = formula(*leaves)
    terms = []
    for out, g in ((x1, g1), (z2, g2), (log_p, gl)):
        got = torch.autograd.grad((out * g.double()).sum(), leaves, retain_graph=True, allow_unused=True)
        terms.append([torch.zeros_like(v) if t is None else t for t, v in zip(got, leaves)])
    assert float(log_p.detach().abs().max()) > 0.1
    return (x, raw, a, b, g1, g2, gl), [v.detach() for v in (x1, z2, log_p)], terms


def want_grads(terms, present):
    return [sum(t[k] for t, p in zip(terms, present) if p).numpy() for k in range(4)]


def judge(kind, shape, raw_dtype, names, got, ref, tol=TOL, **fields):
    errs = {n: rel_err(g.detach().float().cpu().numpy(), np.asarray(r)) for n, g, r in zip(names, got, ref)}
    print(kind, shape, raw_dtype, errs)
    report("split_latent", case=kind, shape=list(shape), raw=str(raw_dtype).replace("torch.", ""), **errs, **fields)
    for n, e in errs.items():
        assert e <= tol, (kind, shape, n, e)
    return errs


def mover(dev, offset):
    return (lambda v: offset_view(v, dev)) if offset else (lambda v: v.to(dev))


def move_raw(raw, dev, offset):
    """A bf16 raw one float (two elements) into its allocation: 4-byte aligned, not 8 -- the narrow form's condition for it."""
    if not offset or raw.dtype == torch.float32:
        return mover(dev, offset)(raw)
    buf = torch.empty(raw.numel() + 2, dtype=raw.dtype, device=dev)
    v = buf[2:].view(raw.shape)
    v.copy_(raw)
    return v


def on_device(shape, offset, raw_dtype, dev):
    (x, raw, a, b, g1, g2, gl), _, _ = kernel_case(shape, raw_dtype)
    move = mover(dev, offset)
    return move(x), move_raw(raw, dev, offset), a.to(dev), b.to(dev), move(g1), move(g2), gl.to(dev)


def half_outs(shape, dev, offset):
    B, C, H, W = shape
    return tuple(mover(dev, offset)(torch.zeros(B, C // 2, H, W)) for _ in range(2))


# ---------------------------------------------------------------------------------------------------------------------------------
# the split and the merge
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw_dtype", RAWS, ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_split_and_merge_carry_the_couplings_bits_and_the_float64_log_p(shape, offset, raw_dtype, dev):
    from fincflow_amd import ops
    reaches(shape, offset)
    _, (x1_ref, z2_ref, lp_ref), _ = kernel_case(shape, raw_dtype)
    xd, rawd, ad, bd, _, _, _ = on_device(shape, offset, raw_dtype, dev)
    half, move = shape[1] // 2, mover(dev, offset)
    if offset:
        assert all(v.data_ptr() % 16 == 4 for v in (xd, rawd)) and (shape[2] * shape[3]) % 4 == 0
    y = ops.finc_coupling(xd, rawd, ad, bd, 1)[0]
    x1, z2, lp = ops.finc_split_prior(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
    x1b, z2b, lpb = ops.finc_split_prior(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
    assert torch.equal(x1, y[:, :half]) and torch.equal(z2, y[:, half:])           # the halves of the coupling's forward, bit for bit
    assert same_bits(x1, x1b) and same_bits(z2, z2b) and same_bits(lp, lpb)         # fixed-order sums: two runs, the same bits
    assert lp.shape == (shape[0],)

    whole = ops.finc_coupling(move(torch.cat([x1, z2], 1).cpu()), rawd, ad, bd, -1)[0]
    back, lpm = ops.finc_split_prior_merge(x1, z2, rawd, ad, bd, want_log_p=True, out=move(torch.zeros(shape)))
    back2, lpm2 = ops.finc_split_prior_merge(x1, z2, rawd, ad, bd, want_log_p=True, out=move(torch.zeros(shape)))
    bare = ops.finc_split_prior_merge(x1, z2, rawd, ad, bd, out=move(torch.zeros(shape)))
    torch.cuda.synchronize()
    assert torch.equal(back, whole) and torch.equal(bare, whole)                   # the coupling's reverse on cat(x1, z2), without the cat
    assert same_bits(back, back2) and same_bits(lpm, lpm2)
    # the merge reports the split's value at its result: the formula on the z2 it was handed
    s_sum = lp_ref + 0.5 * z2_ref.square().flatten(1).sum(1)
    lpm_ref = s_sum - 0.5 * z2.double().cpu().square().flatten(1).sum(1)
    judge("split" + ("_offset" if offset else ""), shape, raw_dtype, ("x1", "z2", "log_p", "merge_log_p", "round_trip"),
          (x1, z2, lp, lpm, back), (x1_ref, z2_ref, lp_ref, lpm_ref, xd.double().cpu()))


def test_an_empty_batch_launches_nothing(dev, monkeypatch):
    from fincflow_amd import ops
    calls = record_calls(monkeypatch)
    x = torch.empty(0, 4, 5, 3, device=dev)
    a = torch.ones(4, device=dev)
    x1, z2, lp = ops.finc_split_prior(x, x.clone(), a, a)
    assert x1.shape == z2.shape == (0, 2, 5, 3) and lp.shape == (0,)
    back, lpm = ops.finc_split_prior_merge(x1, z2, x.clone(), a, a, want_log_p=True)
    assert back.shape == x.shape and lpm.shape == (0,)
    got = ops.finc_split_prior_backward(x1, z2, lp, x, x.clone(), a, a)
    assert got[0].shape == x.shape and not bool(got[2].any()) and not bool(got[3].any()) and calls == []


def raw_call(dev, name, raw, *args):
    from fincflow_amd import ops
    ops._call(name + ("_rawbf16_f32" if raw.dtype == torch.bfloat16 else "_f32"), dev, *[None if a is None else
              (a.data_ptr() if torch.is_tensor(a) else a) for a in args], ops._stream_ptr(raw))


class Guarded:
    """Outputs between guard bands (fp32: helpers.guarded, bf16: the 2-byte bands of tests/test_gpu_autocast_kernels.py); `lead`: the
    payload one float into its band (the dword forms)."""

    def __init__(self, dev, lead):
        self.dev, self.lead, self.kept = dev, lead, []

    def new(self, shape, dtype=torch.float32):
        if dtype == torch.bfloat16:
            view, buf = guarded16(torch.zeros(shape, dtype=dtype), self.dev, 2 * self.lead)
        else:
            view, buf = guarded(torch.zeros(shape), self.dev, self.lead if len(shape) == 4 else 0)
        self.kept.append((buf, view, dtype == torch.bfloat16))
        return view

    def broken(self):
        return [k for k, (b, v, half) in enumerate(self.kept) if not (guards16_intact(b, v) if half else guards_intact(b, v))]


@pytest.mark.parametrize("raw_dtype", RAWS, ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_guard_bands_around_every_output_are_intact(shape, offset, raw_dtype, dev):
    """The three entry points called directly, every output and the workspace between guard bands: nothing is written beyond a
    tensor, and the results are those of the plain calls."""
    from fincflow_amd import _lib, ops
    xd, rawd, ad, bd, g1, g2, gl = on_device(shape, offset, raw_dtype, dev)
    B, C, H, W = shape
    hs = (B, C // 2, H, W)
    nbytes = _lib.lib().finc_coupling_workspace_bytes(B, C, H * W)
    g = Guarded(dev, 1 if offset else 0)
    ws = g.new((nbytes // 4,))
    x1, z2, lp = g.new(hs), g.new(hs), g.new((B,))
    raw_call(dev, "finc_split_prior", rawd, xd, rawd, ad, bd, x1, z2, lp, B, C, H * W, ws, nbytes)
    back, lpm, bare = g.new(shape), g.new((B,)), g.new(shape)
    raw_call(dev, "finc_split_prior_merge", rawd, x1, z2, rawd, ad, bd, back, lpm, B, C, H * W, ws, nbytes)
    raw_call(dev, "finc_split_prior_merge", rawd, x1, z2, rawd, ad, bd, bare, None, B, C, H * W, None, 0)
    gx, graw, ga, gb = g.new(shape), g.new(shape, raw_dtype), g.new((C,)), g.new((C,))
    raw_call(dev, "finc_split_prior_backward", rawd, g1, g2, gl, xd, rawd, ad, bd, gx, graw, ga, gb, B, C, H * W, ws, nbytes)
    torch.cuda.synchronize()
    assert not g.broken(), (shape, offset, g.broken())
    plain = ops.finc_split_prior(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
    for got, want in zip((x1, z2, lp), plain):
        assert same_bits(got, want)
    pm = ops.finc_split_prior_merge(plain[0], plain[1], rawd, ad, bd, want_log_p=True, out=mover(dev, offset)(torch.zeros(shape)))
    assert same_bits(back, pm[0]) and same_bits(lpm, pm[1]) and same_bits(bare, pm[0])
    report("split_latent", case="guards", shape=list(shape), raw=str(raw_dtype).replace("torch.", ""), offset=offset,
           guard_elements=sum(b.numel() - v.numel() for b, v, _ in g.kept))


@pytest.mark.parametrize("raw_dtype", RAWS, ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_the_images_of_a_batch_are_isolated(shape, offset, raw_dtype, dev):
    """NaN in image 0's x and raw: every output of the other images keeps its bits (and image 0 shows the NaN: not vacuous)."""
    from fincflow_amd import ops
    (x, raw, a, b, g1, g2, gl), _, _ = kernel_case(shape, raw_dtype)
    move = mover(dev, offset)

    def every(x, raw):
        xd, rawd, ad, bd = move(x), move_raw(raw, dev, offset), a.to(dev), b.to(dev)
        x1, z2, lp = ops.finc_split_prior(xd, rawd, ad, bd, out=half_outs(shape, dev, offset))
        back, lpm = ops.finc_split_prior_merge(x1, z2, rawd, ad, bd, want_log_p=True, out=move(torch.zeros(shape)))
        gx, graw, _, _ = ops.finc_split_prior_backward(move(g1), move(g2), gl.to(dev), xd, rawd, ad, bd)
        return x1, z2, lp, back, lpm, gx, graw
    clean = every(x, raw)
    xp, rawp = x.clone(), raw.clone()
    xp[0, -1, 0, 0] = float("nan")
    rawp[0, 0, -1, -1] = float("nan")
    dirty = every(xp, rawp)
    for k, (c, d) in enumerate(zip(clean, dirty)):
        assert bool(torch.isfinite(c.float()).all()), k
        assert same_bits(c[1:].float(), d[1:].float()), (k, "another image changed")
    assert not bool(torch.isfinite(dirty[2][0])) and not bool(torch.isfinite(dirty[4][0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the backward
# ---------------------------------------------------------------------------------------------------------------------------------
PRESENT = [(True, True, True), (False, True, True), (True, False, True), (True, True, False)]


@pytest.mark.parametrize("raw_dtype", RAWS, ids=str)
@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_all_four_gradients_against_float64_autograd(shape, offset, raw_dtype, dev):
    """With all three incoming gradients, and with each absent (NULL) in turn."""
    from fincflow_amd import ops
    reaches(shape, offset)
    _, _, terms = kernel_case(shape, raw_dtype)
    xd, rawd, ad, bd, g1, g2, gl = on_device(shape, offset, raw_dtype, dev)
    for present in PRESENT:
        given = [g if p else None for g, p in zip((g1, g2, gl), present)]
        got = ops.finc_split_prior_backward(*given, xd, rawd, ad, bd)
        again = ops.finc_split_prior_backward(*given, xd, rawd, ad, bd)
        torch.cuda.synchronize()
        assert got[1].dtype == raw_dtype and all(same_bits(a.float(), b.float()) for a, b in zip(got, again))
        # a bf16 grad_raw carries 8 bits: it is judged below against the fp32 call rounded once, here at 2^-8
        ref = want_grads(terms, present)
        if raw_dtype == torch.bfloat16:
            assert rel_err(got[1].float().cpu().numpy(), ref[1]) <= 2.0 ** -8
            got, ref, names = (got[0], got[2], got[3]), (ref[0], ref[2], ref[3]), (NAMES[0], NAMES[2], NAMES[3])
        else:
            names = NAMES
        judge("backward" + ("_offset" if offset else ""), shape, raw_dtype, names, got, ref, present=list(present))


@pytest.mark.parametrize("shape,offset", CASES, ids=str)
def test_a_bf16_grad_raw_is_the_fp32_result_rounded_once(shape, offset, dev):
    from fincflow_amd import ops
    xd, rawd, ad, bd, g1, g2, gl = on_device(shape, offset, torch.bfloat16, dev)
    got = ops.finc_split_prior_backward(g1, g2, gl, xd, rawd, ad, bd)
    wide = ops.finc_split_prior_backward(g1, g2, gl, xd, mover(dev, offset)(rawd.float().cpu()), ad, bd)
    torch.cuda.synchronize()
    assert got[1].dtype == torch.bfloat16 and wide[1].dtype == torch.float32
    assert torch.equal(got[1].view(torch.int16), wide[1].bfloat16().view(torch.int16))
    for k in (0, 2, 3):
        assert same_bits(got[k], wide[k]), NAMES[k]                                  # everything else: the bits of the fp32 call


@pytest.mark.parametrize("raw_dtype", RAWS, ids=str)
@pytest.mark.parametrize("shape", [(3, 6, 3, 5), (2, 12, 16, 16)], ids=str)
def test_every_combination_of_skipped_outputs(shape, raw_dtype, dev):
    from fincflow_amd import ops
    xd, rawd, ad, bd, g1, g2, gl = on_device(shape, False, raw_dtype, dev)
    full = ops.finc_split_prior_backward(g1, g2, gl, xd, rawd, ad, bd)
    for need in itertools.product((True, False), repeat=4):
        got = ops.finc_split_prior_backward(g1, g2, gl, xd, rawd, ad, bd, *need)
        for n, g, f, name in zip(need, got, full, NAMES):
            assert (g is not None) == n, (need, name)
            if n:
                assert same_bits(g.float(), f.float()), (need, name)
    assert ops.finc_split_prior_backward(g1, g2, gl, xd, rawd, ad, bd, False, False, False, False) == (None,) * 4


def test_the_autograd_function_hands_absent_gradients_over_as_null(dev, monkeypatch):
    from fincflow_amd import ops
    shape = (3, 6, 3, 5)
    (x, raw, a, b, g1, g2, gl), _, terms = kernel_case(shape, torch.float32)
    seen = []
    real = ops.finc_split_prior_backward

    def spy(grad_x1, grad_z2, grad_log_p, *args, **kwargs):
        seen.append((grad_x1 is not None, grad_z2 is not None, grad_log_p is not None))
        return real(grad_x1, grad_z2, grad_log_p, *args, **kwargs)
    monkeypatch.setattr(ops, "finc_split_prior_backward", spy)
    for present in PRESENT[1:] + [(False, False, True)]:
        leaves = [v.to(dev).requires_grad_(True) for v in (x, raw, a, b)]
        outs = ops.split_prior_forward(*leaves)
        assert type(outs[0].grad_fn).__name__ == "_FincSplitPriorFunctionBackward"
        loss = sum((o * g.to(dev)).sum() for o, g, p in zip(outs, (g1, g2, gl), present) if p)
        got = torch.autograd.grad(loss, leaves)
        assert seen[-1] == present, (seen[-1], present)
        judge("function", shape, torch.float32, NAMES, got, want_grads(terms, present), present=list(present))


# ---------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------
def record_calls(monkeypatch):
    """Every entry point that goes through ops._call, by name, in order."""
    from fincflow_amd import ops
    names, real = [], ops._call

    def recorded(name, *args, **kwargs):
        names.append(name)
        return real(name, *args, **kwargs)
    monkeypatch.setattr(ops, "_call", recorded)
    return names


def count_cats(monkeypatch):
    cats, real = [], torch.cat

    def cat(*args, **kwargs):
        cats.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(torch, "cat", cat)
    return cats


RELU = "finc_bias_relu_f32"


def test_which_calls_the_module_makes(dev, monkeypatch):
    import fincflow_amd
    from fincflow_amd import glow
    B, size = 3, (12, 6, 6)
    m = glow.SplitPrior(size, glow.GaussianPrior, width=32)
    cpl.fill(m.transform)
    torch.manual_seed(3)
    x = torch.randn(B, *size)
    m64, md = copy.deepcopy(m).double(), copy.deepcopy(m).to(dev)
    with torch.no_grad():
        x1_ref, z2_ref, lp_ref = m64.split(x.double())
        assert torch.equal(lp_ref, m64(x.double())[1])
    calls, cats = record_calls(monkeypatch), count_cats(monkeypatch)
    xd = x.to(dev)

    # without a graph: the net on the inference path, ONE launch of the split, no cat; the same for the merge
    with torch.no_grad():
        x1, z2, lp = md.split(xd)
        assert calls == [RELU, RELU, "finc_split_prior_f32"] and not cats, (calls, cats)
        del calls[:]
        back, lpm = md.merge(x1, z2, with_log_prob=True)
        bare = md.merge(x1, z2)
        assert calls == [RELU, RELU, "finc_split_prior_merge_f32"] * 2 and not cats, (calls, cats)
        del calls[:]
    judge("module", (B,) + size, torch.float32, ("x1", "z2", "log_p", "merge", "merge_log_p"), (x1, z2, lp, back, lpm),
          (x1_ref, z2_ref, lp_ref, x.double(), lp_ref))
    assert torch.equal(bare, back)

    # while autograd records: the PyTorch net, the split's Function; the merge inside reverse_grad() on today's recorded lines
    xa = xd.clone().requires_grad_(True)
    x1g, z2g, lpg = md.split(xa)
    assert calls == ["finc_split_prior_f32"] and type(lpg.grad_fn).__name__ == "_FincSplitPriorFunctionBackward", calls
    del calls[:]
    (-lpg.mean() + z2g.square().mean()).backward()
    assert calls == ["finc_split_prior_backward_f32"], calls
    assert xa.grad is not None and all(p.grad is not None for p in md.parameters())
    del calls[:], cats[:]
    with fincflow_amd.reverse_grad():
        out, lq = md.merge(x1.clone().requires_grad_(True), z2, with_log_prob=True)
    assert calls == ["finc_coupling_reverse_logdet_f32"] and len(cats) == 1, (calls, cats)
    assert type(out.grad_fn).__name__ == "_FincCouplingReverseLogdetFunctionBackward"
    del calls[:], cats[:]

    # float64 on the device: the PyTorch lines
    m64d = copy.deepcopy(m).double().to(dev)
    with torch.no_grad():
        a1, a2, alp = m64d.split(xd.double())
        aback = m64d.merge(a1, a2)
    assert calls == []
    assert rel_err(alp.cpu().numpy(), lp_ref.numpy()) <= 1e-12 and rel_err(aback.cpu().numpy(), x.double().numpy()) <= 1e-12
    del cats[:]

    # forward / reverse / reverse_with_logdet: the calls they always made
    with torch.no_grad():
        z, ldj = md(xd)
        assert calls == [RELU, RELU, "finc_coupling_f32"], calls
        del calls[:]
        md.reverse(z)
        assert calls == [RELU, RELU, "finc_coupling_f32"] and len(cats) == 1, (calls, cats)
        del calls[:]
        md.reverse_with_logdet(z)
        assert calls == [RELU, RELU, "finc_coupling_reverse_logdet_f32"], calls
    assert torch.equal(z, x1) and rel_err(ldj.cpu().numpy(), lp_ref.numpy()) <= TOL


def test_under_bf16_autocast_the_module_takes_the_rawbf16_entry_points(dev, monkeypatch):
    from fincflow_amd import glow
    size = (12, 6, 6)
    md = glow.SplitPrior(size, glow.GaussianPrior, width=32)
    cpl.fill(md.transform)
    md = md.to(dev)
    torch.manual_seed(5)
    x = torch.randn(3, *size, device=dev)
    calls = record_calls(monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        x1, z2, lp = md.split(x)
        back = md.merge(x1, z2)
    assert calls == ["finc_bias_relu_bf16"] * 2 + ["finc_split_prior_rawbf16_f32"] + ["finc_bias_relu_bf16"] * 2 + \
        ["finc_split_prior_merge_rawbf16_f32"], calls
    assert all(t.dtype == torch.float32 for t in (x1, z2, lp, back))
    err = rel_err(back.cpu().numpy(), x.cpu().numpy())
    print("module round trip under bf16 autocast: %.3e" % err)
    assert err <= TOL
    del calls[:]
    with torch.autocast("cuda", dtype=torch.float16), torch.no_grad():
        md.split(x)
    assert calls[-1] == "finc_split_prior_f32", calls                               # fp16: raw is upcast, the fp32 entry point


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev):
    """(the HIP model, its float64 twin, x): tests/test_split_latent_host.py's model at 16x16, B = 4."""
    from fincflow_amd import glow
    torch.manual_seed(1)
    np.random.seed(1)
    model = glow.create_model(num_blocks=3, block_size=1, split_prior=True, actnorm=True, preprocess=False, image_size=(3, 16, 16),
                              coupling_width=16)
    flow_twin.randomise(model, seed=1, actnorm=True)
    model = model.to(dev)
    x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(7))
    return model, flow_twin.twin_of(model), x


def compare(tag, names, got, want, bar):
    return flow_twin.compare(tag, names, got, want, bar=bar, kind="split_latent")


def test_encode_against_the_twin(models, dev, monkeypatch):
    model, twin, x = models
    calls = record_calls(monkeypatch)
    with torch.no_grad():
        zs, log_prob = model.encode(x.to(dev))
        log_prob_forward = model.log_prob(x.to(dev))
        zs64, lp64 = twin.encode(x.double())
    assert calls.count("finc_split_prior_f32") == 2 and [tuple(z.shape) for z in zs] == [(4, 6, 8, 8), (4, 12, 4, 4), (4, 48, 2, 2)]
    compare("encode", ["z0", "z1", "z2", "log_prob", "log_prob_of_forward"], zs + [log_prob, log_prob_forward], zs64 + [lp64, lp64], TOL)


def test_gradients_of_the_encode_loss_against_the_twin(models, dev, monkeypatch):
    model, twin, x = models
    flow_twin.sync(twin, model)
    calls = record_calls(monkeypatch)
    names, params = zip(*model.named_parameters())
    with flow_twin.recorded_masks(model) as masks:
        loss = -model.encode(x.to(dev))[1].mean()
        got = torch.autograd.grad(loss, params)
    assert calls.count("finc_split_prior_f32") == 2 and calls.count("finc_split_prior_backward_f32") == 2, calls
    tparams = [dict(twin.named_parameters())[n] for n in names]
    with flow_twin.replayed_masks(twin, masks):
        loss64 = -twin.encode(x.double())[1].mean()
        want = flow_twin.masked(twin, dict(zip(names, torch.autograd.grad(loss64, tparams))))
    compare("encode_loss", ["loss"], [loss], [loss64], TOL)
    compare("encode_gradients", list(names), list(got), [want[n] for n in names], TOL)


def test_decode_of_encode_is_the_input(models, dev, monkeypatch):
    model, twin, x = models
    with torch.no_grad():
        zs, log_prob = model.encode(x.to(dev))
        calls = record_calls(monkeypatch)
        back, log_q = model.decode(zs, with_log_prob=True)
        assert calls.count("finc_split_prior_merge_f32") == 2 and "finc_coupling_reverse_logdet_f32" in calls, calls
        bare = model.decode(zs)
        resampled = model.reconstruct(x.to(dev))
        zs64 = [z.double().cpu() for z in zs]
        want_q = twin.log_prob(twin.decode(zs64))
    assert torch.equal(bare, back)
    compare("round_trip", ["x"], [back], [x.double()], CHAIN_TOL)
    compare("decode_log_q", ["log_q", "log_q_of_encode"], [log_q, log_q], [want_q, log_prob.double().cpu()], TOL)
    assert rel_err(resampled.cpu().numpy(), x.numpy()) > 1e-2                       # what `reconstruct` does in this model: a resample
    with pytest.raises(ValueError):
        model.decode(zs[:-1])
    with pytest.raises(ValueError):
        model.decode([zs[0], zs[1][:, :, :2], zs[2]])


def test_a_tempered_sample_against_the_twin_on_the_same_draws(models, dev):
    model, twin, _ = models
    T = 0.7
    with torch.no_grad():
        torch.manual_seed(21)
        with flow_twin.recorded_noise(model) as draws:
            x, x_true = model.sample(4, temperature=T)
        torch.manual_seed(21)
        via_decode = model.decode(model.draw_latents(4, temperature=T))
        torch.manual_seed(21)
        plain = model.decode(model.draw_latents(4))
        torch.manual_seed(21)
        sampled = model.sample(4)[0]
        # the draws arrive base first, then the split layers from the last to the first: the code is that list backwards
        want = twin.decode([T * d.double().cpu() for d in draws][::-1])
    assert len(draws) == 3 and x_true is x and torch.equal(x, via_decode)
    # at temperature 1 `sample` keeps its own path (cat + the coupling's reverse): the same draws, the same x to fp32 rounding (the split
    # layers' nets see x1 as a slice of the cat there and as a tensor of its own in `decode`; bit-equal on the CPU, tests/test_split_latent_host.py)
    assert rel_err(plain.cpu().numpy(), sampled.cpu().numpy()) <= TOL
    compare("tempered_sample", ["x"], [x], [want], TOL)


def test_the_round_trip_under_bf16_autocast(models, dev, monkeypatch):
    model, _, x = models
    calls = record_calls(monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        zs, _ = model.encode(x.to(dev))
        back = model.decode(zs)
    assert calls.count("finc_split_prior_rawbf16_f32") == 2 and calls.count("finc_split_prior_merge_rawbf16_f32") == 2, calls
    assert all(z.dtype == torch.float32 for z in zs) and back.dtype == torch.float32
    compare("round_trip_bf16_autocast", ["x"], [back], [x.double()], TOL)


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
