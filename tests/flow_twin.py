"""A float64 CPU twin of any `FlowSequential`, for tests that use the model the way its users do (tests/test_flow_twin_host.py,
tests/test_gpu_train_loop.py).  A helper, not collected.

`twin_of(model)` is an independent copy on the CPU in float64 (or float32: the yardstick).  The glow layers are the model's own
classes: on CPU tensors they run their PyTorch lines, which are the reference's formulas.  The units have no CPU path, so on the
twin's INSTANCES (never on the class: the HIP model lives in the same process) `forward` becomes `inverse_backward_ref.forward` and
`reverse` / `reverse_with_logdet` become `inverse_backward_ref.solve`, both on the stored weights of the groups and differentiable.
The twin runs with `fuse_affine = False`: every fold of the HIP model is compared with the layers one after the other.

`sync(twin, model)` copies every parameter and buffer exactly ("teacher forcing": every comparison is made at the HIP model's
current parameters, so optimiser round-off never accumulates into the bar).  `recorded_noise(model)` keeps what every
`GaussianPrior.sample` of the model returned, in order; `replayed_noise(twin, draws, pick)` makes the twin's reverse consume the
same draws, sliced to the picked images.  `compare` judges with helpers.rel_err and appends to the parity report (kind
`train_loop`), the float32 twin's own error against the float64 twin beside every HIP error.
"""
import contextlib
import copy

import numpy as np
import torch

import inverse_backward_ref as ref
from helpers import report, rel_err


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------------------
def _twin_padded(m, orient):
    """PaddedConv2d on the reference formulas (one group, its own orientation; the optional bias as the module applies it)."""
    def bias():
        return m.bias if m.bias is not None else m.conv.bias

    def forward(x, context=None, compute_expensive=None):
        out = ref.forward(x, m.conv.weight, 1, orient)
        return (out if bias() is None else out + bias().view(1, -1, 1, 1)), 0.0

    def reverse(x, context=None, compute_expensive=None):
        if bias() is not None:
            x = x - bias().reshape(-1, x.shape[1], 1, 1)
        return ref.solve(x, m.conv.weight, 1, orient), 0

    def reverse_with_logdet(x, context=None):
        out = reverse(x, context)[0]
        return out, out.new_zeros(len(out))

    m.forward, m.reverse, m.reverse_with_logdet = forward, reverse, reverse_with_logdet


def _twin_unit(m, orient):
    """FastFlowUnit on the reference formulas: four groups, the stored banks concatenated in the graph."""
    def forward(x, context=None):
        return ref.forward(x, torch.cat(m._weights(), 0), 4, orient), 0.0

    def reverse(x, context=None):
        return ref.solve(x, torch.cat(m._weights(), 0), 4, orient)

    def reverse_with_logdet(x, context=None):
        out = reverse(x, context)
        return out, out.new_zeros(len(out))

    m.forward, m.reverse, m.reverse_with_logdet = forward, reverse, reverse_with_logdet


def _twin_mix(m):
    """Conv1x1 keeps W^-1 and log|det W| per (address, version) of W (`ops.version_key`): the twin computes both on every call, so that
    nothing the library does to its cache keys can reach the reference."""
    m._inverse_matrix = lambda: torch.inverse(m.W.detach())
    m._log_abs_det = lambda: torch.slogdet(m.W)[1]


#: what the layers cache per parameter version (fincflow_amd/glow.py): a twin starts without any of it
_DERIVED = ("_w_inv", "_inv_key", "_ld", "_ld_key", "_m_aff", "_b_aff", "_aff_key", "_m_lead", "_b_lead", "_lead_key", "_lead_inv",
            "_lead_obj", "_ab", "_ab_key")


def twin_of(model, dtype=torch.float64):
    """An independent CPU model with `model`'s layers and parameters in `dtype`; `model` itself is not touched.  (The replaced methods
    are closures over the twin's own modules: make another twin with `twin_of`, not with a copy of this one.)"""
    from fincflow_amd import FastFlowUnit, PaddedConv2d, glow, ops
    twin = copy.deepcopy(model).cpu().to(dtype)
    twin.fuse_affine = False                             # (on the instance: the class attribute stays)
    for m in twin.modules():
        for name in _DERIVED:
            m.__dict__.pop(name, None)
        if hasattr(m, "_init_known"):
            m._init_known = None
        if isinstance(m, FastFlowUnit):
            _twin_unit(m, ops.ORIENT_FASTFLOW)
        elif isinstance(m, PaddedConv2d):                # (a CINCFlowUnit goes through its conv_tl)
            _twin_padded(m, ops.ORDER_BITS[m.order])
        elif isinstance(m, glow.Conv1x1):
            _twin_mix(m)
    sync(twin, model)
    return twin


def randomise(model, seed=1, actnorm=False):
    """Conv2dZero parameters as tests/test_gpu_inverse_backward.py's build_chain fills them (at their zero initialisation every
    coupling is the identity); `actnorm`: ActNorm's by hand as well, marked initialised (otherwise its first forward computes them
    from the data)."""
    from fincflow_amd import glow
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, glow.ActNorm) and actnorm:
                m.log_scale.copy_(0.1 * torch.randn(m.n_dims, generator=gen))
                m.translation.copy_(0.1 * torch.randn(m.n_dims, generator=gen))
                m.mark_initialized()
            elif isinstance(m, glow.Conv2dZero):
                m.weight.copy_(0.05 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.01 * torch.randn(m.bias.shape, generator=gen))
                m.logs.copy_(0.01 * torch.randn(m.logs.shape, generator=gen))
    return model


def sync(twin, model):
    """Every parameter and buffer of `model` into `twin`, exactly (float32 -> float64 has no rounding), ActNorm's `initialized`
    with its host-side mirror included; the twin's gradients are dropped."""
    with torch.no_grad():
        for kind in ("named_parameters", "named_buffers"):
            src, dst = dict(getattr(model, kind)()), dict(getattr(twin, kind)())
            assert src.keys() == dst.keys(), sorted(src.keys() ^ dst.keys())
            for name, t in dst.items():
                t.copy_(src[name].detach().cpu().to(t.dtype))
    for m in twin.modules():
        if hasattr(m, "_init_known"):
            m._init_known = None
    twin.zero_grad(set_to_none=True)


def unit_weights(model):
    """name -> (parameter, G, Cq, KH, KW, orient of its one group) for every stored bank of the model's units."""
    from fincflow_amd import PaddedConv2d, ops
    out = {}
    for name, m in model.named_modules():
        if isinstance(m, PaddedConv2d):
            w = m.conv.weight
            out[(name + "." if name else "") + "conv.weight"] = (w, 1, w.shape[1], w.shape[2], w.shape[3], ops.ORDER_BITS[m.order])
    return out


def stored_masks(model):
    """name -> float64 mask (1: trainable) of every stored bank, from `inverse_backward_ref.stored_mask`."""
    return {name: ref.stored_mask(G, Cq, KH, KW, o) for name, (_, G, Cq, KH, KW, o) in unit_weights(model).items()}


def mask_unit_grads(twin):
    """The free autograd gradient of a stored bank is non-zero under the corner-tap mask; the HIP backward masks in-kernel."""
    masks = stored_masks(twin)
    for name, p in twin.named_parameters():
        if name in masks and p.grad is not None:
            p.grad.mul_(masks[name].to(p.grad.dtype))


def masked(twin, grads):
    """`grads`: name -> tensor (or None), e.g. from torch.autograd.grad: the same with the units' masks applied."""
    masks = stored_masks(twin)
    return {n: (g if g is None or n not in masks else g * masks[n].to(g.dtype)) for n, g in grads.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------------------------------------------
def _priors(model):
    from fincflow_amd import glow
    return [m for m in model.modules() if isinstance(m, glow.GaussianPrior)]


@contextlib.contextmanager
def recorded_noise(model):
    """Yields a list that receives, in order, the draw of every `GaussianPrior.sample` of `model` (the base and every
    `SplitPrior.base`, wrapped per instance) made inside the context."""
    draws, priors = [], _priors(model)
    for p in priors:
        def sample(n_samples, context=None, _orig=p.sample):
            out = _orig(n_samples, context)
            draws.append(out[0].detach().clone())
            return out
        p.sample = sample
    try:
        yield draws
    finally:
        for p in priors:
            del p.sample


@contextlib.contextmanager
def replayed_noise(twin, draws, pick=None):
    """Inside the context every `GaussianPrior.sample` of `twin` returns the next recorded draw (rows `pick`, in the prior's
    dtype) instead of drawing; every draw must be consumed, with the sizes asked for."""
    queue, priors = list(draws), _priors(twin)
    for p in priors:
        def sample(n_samples, context=None, _p=p):
            x = queue.pop(0).cpu()
            x = (x if pick is None else x[list(pick)]).to(_p._anchor.dtype)
            assert tuple(x.shape) == (n_samples,) + _p.size, (tuple(x.shape), n_samples, _p.size)
            return x, _p.log_prob(x, context)
        p.sample = sample
    try:
        yield
        assert not queue, "%d recorded draws were not consumed" % len(queue)
    finally:
        for p in priors:
            del p.sample


# ---------------------------------------------------------------------------------------------------------------------------------
# the ReLUs' activation pattern
# ---------------------------------------------------------------------------------------------------------------------------------
# The derivative of a ReLU jumps where its input crosses zero, and a gradient pass of model A evaluates some 1e5 of them: the smallest
# |input| of a pass is a few 1e-6, within the float32 rounding of the convolution in front of it, so about one pass in twenty has an
# activation whose sign differs between two correct evaluations -- and with it every gradient behind it, by per cent (seen on the
# device: 8.net.0.weight off by 5.5e-2 with x and log_q of the same pass within 8e-7; gone with PyTorch's own convolution in place of
# MIOpen's, whose rounding differs).  The coupling net under autograd is PyTorch's, not the library's, so a gradient comparison
# differentiates the SAME branch on both sides: the pattern the model's nn.ReLU modules produced is recorded and replayed into the
# twin, where it may only differ from the twin's own at inputs that small.
FLIP_BOUND = 1e-5            # |input| of a replayed activation that changed sides, relative to the largest input of that call


def _relus(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.ReLU)]


@contextlib.contextmanager
def recorded_masks(model):
    """Yields name -> list of the activation patterns (output > 0) of every call of every nn.ReLU module of `model` inside the
    context, in call order."""
    masks = {n: [] for n, _ in _relus(model)}
    handles = [m.register_forward_hook(lambda mod, inp, out, _n=n: masks[_n].append((out > 0).cpu())) for n, m in _relus(model)]
    try:
        yield masks
    finally:
        for h in handles:
            h.remove()


@contextlib.contextmanager
def replayed_masks(twin, masks):
    """Inside the context the nn.ReLU modules of `twin` take the recorded patterns, call by call (a module with nothing recorded left
    runs as it is); yields a one-element list counting the activations that changed sides, each checked against FLIP_BOUND."""
    queues, flips = {n: list(v) for n, v in masks.items()}, [0]

    def hook(mod, inp, out, name):
        if not queues.get(name):
            return None
        x, mask = inp[0], queues[name].pop(0)
        changed = mask != (out.detach() > 0)
        if bool(changed.any()):
            size = float(x.detach()[changed].abs().max() / x.detach().abs().max())
            assert size <= FLIP_BOUND, "%s: an activation of relative size %.1e changed sides" % (name, size)
            flips[0] += int(changed.sum())
        return x * mask.to(x.dtype)
    handles = [m.register_forward_hook(lambda mod, inp, out, _n=n: hook(mod, inp, out, _n)) for n, m in _relus(twin)]
    try:
        yield flips
        assert not any(queues.values()), "recorded activation patterns were not consumed"
    finally:
        for h in handles:
            h.remove()


# ---------------------------------------------------------------------------------------------------------------------------------
# judging
# ---------------------------------------------------------------------------------------------------------------------------------
def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def error(got, want):
    """helpers.rel_err; a reference that is identically zero asks for exact zeros (0.0 or inf)."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.any(want):
        return 0.0 if not np.any(got) else float("inf")
    return rel_err(got, want)


def compare(tag, names, got, want, yard=None, bar=None, kind="train_loop", **fields):
    """`got` (the HIP model) against `want` (the float64 twin), one `helpers.rel_err` per tensor; `yard`: the float32 twin's
    tensors, judged against `want` the same way -- the reference's own error, recorded beside the HIP one.  Appends one line to the
    parity report (under `kind`) and prints it; with a `bar`, asserts every HIP error under it.  Returns name -> error."""
    assert len(names) == len(got) == len(want) and (yard is None or len(yard) == len(want)), (tag, len(names), len(got), len(want))
    errs = {n: error(g, w) for n, g, w in zip(names, got, want)}
    yards = {n: error(y, w) for n, y, w in zip(names, yard, want)} if yard is not None else {}
    worst = max(errs, key=errs.get)
    worst_yard = max(yards, key=yards.get) if yards else None
    line = dict(case=tag, tensors=len(names), hip=errs[worst], hip_at=worst, yardstick=yards.get(worst_yard), yardstick_at=worst_yard,
                bar=bar, **fields)
    report(kind, **line)
    print("%s %s %s: HIP %.3e (%s), float32 twin %s, bar %s" % (
        kind, tag, fields or "", errs[worst], worst, "%.3e (%s)" % (yards[worst_yard], worst_yard) if yards else "-", bar))
    if bar is not None:
        over = {n: e for n, e in errs.items() if not e <= bar}
        assert not over, (tag, fields, over, bar)
    return errs
