"""Whole models on the GPU against recordings of the reference's own create_model (tests/golden/make_golden_model.py; layout and
helpers: tests/reference_model.py).  Reads fixtures only.

The recorded state dict is loaded strictly, the model moved to the device and handed the recorded noise (the draw is patched: a
device generator cannot reproduce a draw made on the CPU).  Two models: `model_mnist` (1x28x28: units of 1 and 2 channels per group
on 14x14 and 7x7 maps, whose width is no multiple of 4; a SplitPrior with half = 2) and `model_cifar` (3x16x16: 12 and 24 channels
on 8x8 and 4x4 maps).

  * every layer, units included, on the float64 recording's input of its position, forward and reverse: 1e-5 in float32, 1e-12
    for `model.double()`;
  * the whole model in float32 against the float64 recording at 5e-5, the project's bar for values through a stack: `forward`,
    `log_prob`, `encode` (its latents against the recorded factored-out halves and the top z), `bits_per_dim`, `decode` of the
    recorded latents (the image in front of the floor, and the images behind it exactly except pixels whose recorded continuous
    value lies within 0.02 of an integer), the parameter gradients of -log_prob.mean() with the units' masked entries exactly 0;
  * the same views under every switch the project has grown -- `fuse_image_boundary`, `invertible_backward`, `hip_recorded_merge`
    inside `reverse_grad()`, `convert_conv1x1(model, to="lu")` -- at the same 5e-5 (no existing test of a switch has a looser
    bar: tests/test_gpu_image_boundary.py, test_gpu_invertible_backward.py, test_gpu_merge_backward.py and test_gpu_plu.py hold
    their model views to 1e-5 or 5e-5), and under `model.double()` at 1e-12, the project's float64 bar;
  * a fresh model's first forward on the recorded 8-image batch reaches the recorded ActNorm parameters within 1e-5.

A bar is the recorded one (`yard`): the value above unless the reference's own float32 error asked for more (four times that error;
tests/test_reference_model_host.py checks the rule).  Every case prints what it achieved and appends it to the parity report (kind
`reference_model`): per quantity the achieved error, the reference's own float32 error and the bar.
"""
import math

import numpy as np
import pytest
import torch

import reference_model as rm
from helpers import report

pytestmark = pytest.mark.gpu

NAMES = sorted(rm.MODELS)
SWITCHES = ["plain", "fuse_image_boundary", "invertible_backward", "hip_recorded_merge", "lu", "double"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def loaded(name, dev, **overrides):
    from fincflow_amd import load_reference_checkpoint
    model = rm.build(name, **overrides)
    result = load_reference_checkpoint(model, {"model_state_dict": rm.recorded_state(name)}, strict=True)
    assert list(result.missing_keys) == [] and list(result.unexpected_keys) == []
    return model.to(dev)


def switched(name, dev, switch):
    from fincflow_amd import glow
    model = loaded(name, dev, hip_recorded_merge=(switch == "hip_recorded_merge"))
    if switch == "fuse_image_boundary":
        model.fuse_image_boundary = True
    elif switch == "invertible_backward":
        model.invertible_backward = True
    elif switch == "lu":
        glow.convert_conv1x1(model, to="lu")
        assert sum(type(m) is glow.Conv1x1LU for m in model) == 2
    elif switch == "double":
        model = model.double()
    return model


def judge(name, case, errs, double=False):
    """Print, report and assert: quantity -> achieved error, against the recorded bar (1e-12 in float64)."""
    yard = rm.yard(name)
    alias = {"bits_per_dim": "log_prob"}
    lines = {q: [e, yard.get(alias.get(q, q), {}).get("ref32"), rm.bar(name, alias.get(q, q), double)] for q, e in errs.items()}
    worst = max(lines, key=lambda q: lines[q][0] / max(lines[q][2], 1e-300))
    report("reference_model", model=name, case=case, quantities=lines)
    print("reference_model %s %s: %d quantities, worst %s achieved %.3e (reference float32 %s, bar %.1e)"
          % (name, case, len(lines), worst, lines[worst][0], lines[worst][1], lines[worst][2]))
    over = {q: v for q, v in lines.items() if not v[0] <= v[2]}
    assert not over, (name, case, over)


# ---------------------------------------------------------------------------------------------------------------------------------
# every layer on the recorded input of its position
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_every_layer_on_its_recorded_input(name, dtype, dev):
    """The units' forward and inverse on what the reference fed them (in `model_mnist` the inverse at 1 channel per group on a
    14x14 map and at 2 on a 7x7 map), ActNorm, Conv1x1, Coupling and SplitPrior on their HIP kernels, the image boundary's layers."""
    model = loaded(name, dev)
    if dtype == torch.float64:
        model = model.double()
    errs = rm.layer_walk(model, name, dtype, dev)
    n_layers = len(model.sequence_modules)
    assert len([q for q in errs if q.startswith("rev.")]) == n_layers == len([q for q in errs if q.endswith(".logdet")])
    judge(name, "layers/" + ("f64" if dtype == torch.float64 else "f32"), errs, dtype == torch.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole model, under every switch
# ---------------------------------------------------------------------------------------------------------------------------------
def lu_factor_grads(layer, grad_w):
    """The gradients of a Conv1x1LU's factors that belong to the recorded gradient `grad_w` of the dense matrix: the chain rule in
    float64 on the CPU through W[r] = (L (U + diag(sign_s * exp(log_s))))[perm[r]], written out here.  (The loss depends on the
    factors through W alone: log|det W| = sum(log_s) is the same function of them.)"""
    lower, upper, log_s = (p.detach().cpu().double().requires_grad_() for p in (layer.lower, layer.upper, layer.log_s))
    eye = torch.eye(len(log_s), dtype=torch.float64)
    diag = torch.diag(layer.sign_s.detach().cpu().double() * torch.exp(log_s))
    w = ((torch.tril(lower, -1) + eye) @ (torch.triu(upper, 1) + diag))[layer.perm.cpu().long()]
    grads = torch.autograd.grad(w, (lower, upper, log_s), torch.from_numpy(np.array(grad_w, dtype=np.float64)))
    return dict(zip(("lower", "upper", "log_s"), grads))


def model_views(model, name, dev, switch):
    from fincflow_amd import FlowSequential, PaddedConv2d, ops
    fx = rm.fixture(name)
    dtype = torch.float64 if switch == "double" else torch.float32
    mods = list(model.sequence_modules)
    splits = [i for i, m in enumerate(mods) if hasattr(m, "split")]
    x, u = rm.tensor(name, "x").to(dev, dtype), rm.tensor(name, "u", dtype, dev)
    want_z, want_lp = fx["f64.fwd.L%d.out" % (len(mods) - 1)], fx["f64.log_prob"]
    errs = {}

    def worst(q, got, want):
        errs[q] = max(errs.get(q, 0.0), rm.error(got.detach().cpu().numpy(), want))

    with torch.no_grad(), rm.handed_noise(u):
        z, lp = model(x)
        worst("z", z, want_z)
        worst("log_prob", lp, want_lp)
        worst("log_prob", model.log_prob(x), want_lp)
        zs, lp = model.encode(x)
        assert len(zs) == len(splits) + 1
        for i, half in zip(splits, zs):
            worst("half.L%d" % i, half, fx["f64.fwd.L%d.half" % i])
        worst("z", zs[-1], want_z)
        worst("log_prob", lp, want_lp)
        worst("bits_per_dim", model.bits_per_dim(x), -want_lp / (fx["x"][0].size * math.log(2.0)))

    # decode of the recorded latents: the images behind the floor, and the image in front of it from the model without the floor
    latents = [rm.tensor(name, "rev.z.L%d" % i, dtype, dev) for i in splits] + [rm.tensor(name, "rev.z.top", dtype, dev)]
    inner = FlowSequential(model.base_distribution, *mods[1:])
    near = rm.near_integer(fx["f64.rev.L1.out"])
    assert near.mean() <= rm.MAX_EXCLUDED

    def decode_views():
        images = model.decode(latents).detach().cpu().numpy()
        errs["images"] = max(errs.get("images", 0.0), float(((images != fx["f64.rev.L0.out"]) & ~near).any()))
        worst("decode.image", inner.decode(latents), fx["f64.rev.L1.out"])

    with torch.no_grad():
        decode_views()
    if switch == "hip_recorded_merge":                      # the reverse chain recorded for autograd: the boundaries' merge on HIP
        assert all(mods[i].hip_recorded_merge for i in splits)
        with torch.enable_grad(), ops.reverse_grad():
            decode_views()

    # the parameter gradients of -log_prob.mean()
    model.zero_grad(set_to_none=True)
    with rm.handed_noise(u):
        lp = model.log_prob(x)
    worst("log_prob", lp, want_lp)
    (-lp.mean()).backward()
    masks = {n + ".conv.weight": m.mask for n, m in model.named_modules() if isinstance(m, PaddedConv2d)}
    compared = 0
    for key, p in model.named_parameters():
        assert p.grad is not None, key
        if "f64.grad." + key not in fx:                     # a Conv1x1LU's factors: the recorded gradient of W, through the chain rule
            layer, factor = key.rsplit(".", 1)
            assert switch == "lu" and factor in ("lower", "upper", "log_s"), key
            want = lu_factor_grads(dict(model.named_modules())[layer], fx["f64.grad.%s.W" % layer])[factor]
            errs["grad.%s.W" % layer] = max(errs.get("grad.%s.W" % layer, 0.0), rm.error(p.grad.cpu().numpy(), want.numpy()))
            continue
        worst("grad." + key, p.grad, fx["f64.grad." + key])
        compared += 1
        if key in masks:
            assert bool((p.grad[masks[key].to(dev) == 0] == 0).all()), key
    assert compared == len([k for k in fx if k.startswith("f64.grad.")]) - (2 if switch == "lu" else 0)
    return errs


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_the_whole_model_under_every_switch(name, switch, dev):
    """A switch must not change what a reference checkpoint means."""
    model = switched(name, dev, switch)
    judge(name, "model/" + switch, model_views(model, name, dev, switch), switch == "double")


# ---------------------------------------------------------------------------------------------------------------------------------
# the data-dependent initialisation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_fresh_model_reaches_the_recorded_actnorm_parameters(name, dev):
    """The reference's model as constructed (its units and 1x1 matrices are on file; its zero-initialised couplings are the
    identity) makes its first forward on the recorded 8-image batch and noise: every ActNorm here must reach the parameters the
    reference's reached (in float64), on the HIP initialisation kernel."""
    from fincflow_amd import glow
    fx = rm.fixture(name)
    model = rm.build(name)
    state = {k[len("init.state."):]: torch.from_numpy(v.copy()) for k, v in fx.items() if k.startswith("init.state.")}
    result = model.load_state_dict(state, strict=False)
    assert state and list(result.unexpected_keys) == []
    assert all(not bool(m.weight.any()) and not bool(m.bias.any()) and not bool(m.logs.any())
               for m in model.modules() if isinstance(m, glow.Conv2dZero))
    model = model.to(dev)
    norms = {n: m for n, m in model.named_modules() if isinstance(m, glow.ActNorm)}
    assert len(norms) == 2 and not any(m._is_initialized() for m in norms.values())
    x, u = rm.tensor(name, "init.x").to(dev, torch.float32), rm.tensor(name, "init.u", torch.float32, dev)
    with torch.no_grad(), rm.handed_noise(u):
        model(x)
    assert all(int(m.initialized) == 1 for m in norms.values())
    errs = {}
    for n, m in norms.items():
        for p in ("translation", "log_scale"):
            errs["init.%s.%s" % (n, p)] = rm.error(getattr(m, p).detach().cpu().numpy(), fx["init64.%s.%s" % (n, p)])
    assert set(errs) == {q for q in rm.yard(name) if q.startswith("init.")}
    judge(name, "actnorm_init", errs)
