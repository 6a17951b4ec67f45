"""Recordings of WHOLE models built from the REFERENCE's own classes in the order of its create_model (build container only):

    python oracle/build_ref.py && python tests/golden/make_golden_model.py

Writes tests/golden/model_mnist.npz, model_cifar.npz (layout: tests/reference_model.py), tests/golden/model_state_keys.json (names
and shapes of the state dict for twelve configurations; nothing is run for those) and profiles/reference_model/
recorder_yardsticks.json.  Imports from the reference, where it lies: layers/{dequantize,normalize,transforms,squeeze,actnorm,
conv1x1,coupling,splitprior,flowsequential}.py, layers/distributions/uniform.py and fastflow.py::FastFlowUnit, all on the CPU.

What the reference needs to run here:
  * torch.utils.cpp_extension.load is stubbed (fastflow.py builds a CUDA extension on import), `wandb` is an empty module
    (layers/selfnorm.py imports it), the Cython solver comes from oracle.build_ref.build();
  * train/losses.py:25 hard-codes device='cuda', so the base of FlowSequential and SplitPrior is `QueuedNormal` below: the same
    log_prob / sample(n, context) interface, its `sample` hands out the latents the recorder queued;
  * the dequantisation noise is handed to the reference's Dequantization through its distribution's `sample`: an input on file;
  * FastFlowUnit.reverse calls the CUDA extension: the reverse is walked by hand with `reverse_level1`.  That one rounds the
    solver's float64 result to float32 (layers/conv.py:126), so the float64 walk calls the same solver on the same flipped
    operands and keeps its doubles.

Every recorded quantity carries the reference's own float32 error against its float64 recording (helpers.rel_err): it has to lie
within a quarter of the quantity's bar, the recorder re-seeds until it does and keeps the seed; a quantity that no draw brings
there gets four times its recorded error as its bar, written into the fixture and the profile.
"""
import copy
import importlib.util
import json
import math
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/fastflow"
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import build_ref  # noqa: E402
from helpers import det_fill  # noqa: E402
import reference_model as rm  # noqa: E402

import torch  # noqa: E402
import torch.utils.cpp_extension  # noqa: E402

so = build_ref.build()
spec = importlib.util.spec_from_file_location("utils.fastflow_inverse.solve_parallel_mc", so)
ref_cy = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_cy)
sys.modules["utils.fastflow_inverse.solve_parallel_mc"] = ref_cy
sys.modules.setdefault("wandb", types.ModuleType("wandb"))
torch.utils.cpp_extension.load = lambda *a, **k: None
sys.path.insert(0, REF)
_cwd = os.getcwd()
os.chdir(tempfile.mkdtemp())
from layers import Dequantization, Normalization  # noqa: E402
from layers.distributions.uniform import UniformDistribution  # noqa: E402
from layers.splitprior import SplitPrior  # noqa: E402
from layers.flowsequential import FlowSequential  # noqa: E402
from layers.conv1x1 import Conv1x1  # noqa: E402
from layers.actnorm import ActNorm  # noqa: E402
from layers.squeeze import Squeeze  # noqa: E402
from layers.transforms import LogitTransform  # noqa: E402
from layers.coupling import Coupling  # noqa: E402
from layers.conv import PaddedConv2d  # noqa: E402
from fastflow import FastFlowUnit  # noqa: E402
os.chdir(_cwd)
torch.set_num_threads(1)

FIRST_SEED = {"model_mnist": 2801, "model_cifar": 3161}
MAX_DRAWS = 48
LATENT_TEMPERATURE = 0.7           # of the (first) SplitPrior's latent; the top latent is taken at 1
QUEUE = []                         # the latents `QueuedNormal.sample` hands out, in the order the reverse walk asks for them
NOISE = {}                         # "u": the dequantisation noise of the next forward


class QueuedNormal(torch.nn.Module):
    """A standard normal with the interface of train/losses.py:17-45, in the dtype of what it is given; no parameters, no buffers
    (the reference's has none either).  `sample` pops the recorder's queue."""

    def __init__(self, size):
        super().__init__()
        self.size = size
        self.dim = int(np.prod(size))

    def log_prob(self, input, context=None, sum=True):
        z = input.reshape(-1, self.dim)
        return -0.5 * (z * z).sum(-1) - 0.5 * self.dim * math.log(2 * math.pi)

    def forward(self, input, context=None):
        return -self.log_prob(input, context).sum(-1)

    def sample(self, n_samples, context=None):
        x = QUEUE.pop(0)
        assert tuple(x.shape) == (n_samples, *self.size), (tuple(x.shape), n_samples, self.size)
        return x, self.log_prob(x, context)


def build(image, num_blocks, block_size, actnorm, split_prior, width=512):
    """The layers of fastflow/fastflow_cifar.py:35-63 at `image`, with the coupling width as an argument (the file has 512)."""
    size, alpha = tuple(image), 1e-6
    layers = [Dequantization(UniformDistribution(size=size)), Normalization(translation=0, scale=256),
              Normalization(translation=-alpha, scale=1 / (1 - 2 * alpha)), LogitTransform()]
    for level in range(num_blocks):
        layers.append(Squeeze())
        size = (size[0] * 4, size[1] // 2, size[2] // 2)
        for _ in range(block_size):
            layers.append(FastFlowUnit(size[0], size[0], (3, 3)))
            if actnorm:
                layers.append(ActNorm(size[0]))
            layers.append(Conv1x1(size[0]))
            layers.append(Coupling(size, width=width))
        if split_prior and level < num_blocks - 1:
            layers.append(SplitPrior(size, QueuedNormal, width=width))
            size = (size[0] // 2, size[1], size[2])
    model = FlowSequential(QueuedNormal(size), *layers)
    model.sequence_modules[0].distribution.sample = lambda n, context=None: (NOISE["u"].to(context.dtype), 0.)
    return model


def move_parameters(name, model):
    """Every parameter away from its initial value, by numbers that depend on the parameter's name alone."""
    masks = {n + ".conv.weight": m.mask for n, m in model.named_modules() if isinstance(m, PaddedConv2d)}
    with torch.no_grad():
        for key, p in model.named_parameters():
            step = torch.from_numpy(det_fill(name + "." + key, tuple(p.shape), 1.0))
            if key in masks:                               # the unit-triangular corner tap stays as it is
                p.add_(0.05 * step * masks[key])
            elif key.endswith(".W"):                       # 1.25 (Q + a small step): well conditioned, log|det| well away from 0
                p.copy_(1.25 * (p + 0.02 * step))
            elif key.endswith("net.4.logs"):
                p.copy_(0.1 * step)
            elif key.endswith("net.4.bias"):               # ONE tensor with logs (layers/coupling.py:31-35): written there
                continue
            elif key.endswith("net.4.weight"):
                p.copy_(0.05 * step)
            elif key.endswith(("translation", "log_scale")):
                p.add_(0.1 * step)
            else:
                p.add_(0.02 * step)
    for n, m in model.named_modules():
        if hasattr(m, "logs"):
            assert torch.equal(m.bias, m.logs) and bool(m.logs.abs().sum() > 0), n
    for m in model.modules():
        if isinstance(m, PaddedConv2d):
            corner = {"TL": [], "TR": [3], "BL": [2], "BR": [2, 3]}[m.order]
            w = torch.flip(m.conv.weight.data, corner) if corner else m.conv.weight.data
            assert torch.equal(torch.triu(w[:, :, -1, -1]), torch.eye(w.shape[0]))


_FLIPS = {"TL": [], "TR": [3], "BL": [2], "BR": [2, 3]}


def unit_reverse(unit, x):
    """fastflow.py:57-76.  In float32 the reference's own `reverse_level1`; in float64 the same solver calls on the same flipped
    operands (layers/conv.py:113-157) without the rounding of its result to float32."""
    if x.dtype == torch.float32:
        return unit.reverse_level1(x)
    outs = []
    for conv, part in zip((unit.conv_tl, unit.conv_tr, unit.conv_bl, unit.conv_br), torch.chunk(x, 4, dim=1)):
        dims = _FLIPS[conv.order]
        xf = torch.flip(part, dims) if dims else part
        wf = torch.flip(conv.conv.weight.data, dims) if dims else conv.conv.weight.data
        y = ref_cy.solve_parallel(np.array(xf.detach().numpy(), dtype=np.float64), np.array(wf.numpy(), dtype=np.float64),
                                  conv.kernel_size)
        y = torch.from_numpy(np.asarray(y))
        outs.append(torch.flip(y, dims) if dims else y)
    return torch.cat(outs, dim=1)


def per_image(logdet, n, dtype):
    return (torch.as_tensor(logdet, dtype=dtype) * torch.ones(n, dtype=dtype)).detach()


def forward_walk(model, x, u):
    """FlowSequential.forward, layers/flowsequential.py:21-44, layer by layer: name -> tensor."""
    out, h = {}, x
    NOISE["u"] = u
    with torch.no_grad():
        for i, m in enumerate(model.sequence_modules):
            if isinstance(m, SplitPrior):
                out["fwd.L%d.half" % i] = m.transform(h, None)[0][:, m.n_channels // 2:].clone()
            h, ld = m(h, None)
            out["fwd.L%d.out" % i], out["fwd.L%d.logdet" % i] = h.clone(), per_image(ld, len(x), x.dtype)
        out["log_prob"] = model(x)[1].clone()
    total = sum(out["fwd.L%d.logdet" % i] for i in range(len(model.sequence_modules)))
    assert torch.allclose(out["log_prob"], model.base_distribution.log_prob(h) + total, rtol=1e-5)
    return out


def forward_steps(model, recorded, x, u):
    """Every layer of `model` on the input that `recorded` (another walk) has at its position."""
    out, dtype = {}, x.dtype
    NOISE["u"] = u
    with torch.no_grad():
        for i, m in enumerate(model.sequence_modules):
            h = x if i == 0 else recorded["fwd.L%d.out" % (i - 1)].to(dtype)
            if isinstance(m, SplitPrior):
                out["fwd.L%d.half" % i] = m.transform(h, None)[0][:, m.n_channels // 2:].clone()
            y, ld = m(h, None)
            out["fwd.L%d.out" % i], out["fwd.L%d.logdet" % i] = y, per_image(ld, len(x), dtype)
    return out


def gradients(model, x, u):
    NOISE["u"] = u
    model.zero_grad()
    (-model.log_prob(x).mean()).backward()
    for m in model.modules():
        if isinstance(m, PaddedConv2d):
            m.reset_gradients()                            # layers/conv.py:98-99
    return {"grad." + k: p.grad.detach().clone() for k, p in model.named_parameters()}


def reverse_layer(m, h):
    with torch.no_grad():
        return unit_reverse(m, h) if isinstance(m, FastFlowUnit) else m.reverse(h, None)


def reverse_walk(model, z_top, latents, recorded=None):
    """FlowSequential.sample's walk, layers/flowsequential.py:94-100, layer by layer; with `recorded` every layer takes the input
    that walk has at its position."""
    out, mods, h = {}, model.sequence_modules, z_top
    QUEUE[:] = [latents[i].to(z_top.dtype) for i in sorted(latents, reverse=True)]
    for i in reversed(range(len(mods))):
        if recorded is not None and i < len(mods) - 1:
            h = recorded["rev.L%d.out" % (i + 1)].to(z_top.dtype)
        h = reverse_layer(mods[i], h)
        out["rev.L%d.out" % i] = h.clone()
    assert not QUEUE
    return out


def record(name, seed):
    """One draw: (arrays, yard, worst share of a bar that the reference's float32 error takes)."""
    image = rm.MODELS[name]["image_size"]
    torch.manual_seed(seed)
    np.random.seed(seed)
    cfg = rm.CONFIG
    fresh = build(image, cfg["num_blocks"], cfg["block_size"], cfg["actnorm"], cfg["split_prior"], cfg["coupling_width"])
    n_layers = len(fresh.sequence_modules)
    arrays = {"seed": np.asarray(seed), "image": np.asarray(image)}
    got64, got32 = {}, {}

    # the data-dependent initialisation of every ActNorm, as the reference makes it on its first forward
    # (dark images, levels 256 r^2: the first ActNorm's mean is well away from 0, where a relative error means something)
    x8, u8 = (256 * torch.rand(8, *image) ** 2).floor().clamp(0, 255).to(torch.uint8), torch.rand(8, *image)
    fresh64 = copy.deepcopy(fresh).double()
    for k, v in fresh.state_dict().items():                # what that forward depends on: the couplings still are the identity
        if k.endswith((".conv.weight", ".W")):
            arrays["init.state." + k] = v.detach().numpy().copy()
    NOISE["u"] = u8
    with torch.no_grad():
        fresh(x8.float())
        fresh64(x8.double())
    arrays["init.x"], arrays["init.u"] = x8.numpy(), u8.numpy()
    for key, p in fresh.named_parameters():
        if key.endswith(("translation", "log_scale")):
            got32["init." + key], got64["init." + key] = p.detach().clone(), dict(fresh64.named_parameters())[key].detach().clone()
            arrays["init32." + key], arrays["init64." + key] = got32["init." + key].numpy(), got64["init." + key].numpy()

    model = fresh
    move_parameters(name, model)
    for k, v in model.state_dict().items():
        arrays["state." + k] = v.detach().numpy().copy()
    model64 = copy.deepcopy(model).double()

    x = torch.randint(0, 256, (3, *image), dtype=torch.uint8)
    x.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)       # the whole range of grey levels, whatever the draw
    u = torch.rand(3, *image)
    arrays["x"], arrays["u"] = x.numpy(), u.numpy()
    f64, f32 = forward_walk(model64, x.double(), u), forward_walk(model, x.float(), u)
    f64.update(gradients(model64, x.double(), u))
    f32.update(gradients(model, x.float(), u))
    step32 = forward_steps(model, f64, x.float(), u)

    # the reverse walk: a top latent and one per SplitPrior, the first of those at a temperature; re-drawn until the images
    # behind the floor can be compared exactly outside the pixels that lie too close to an integer
    splits = [i for i, m in enumerate(model.sequence_modules) if isinstance(m, SplitPrior)]
    for _ in range(MAX_DRAWS):
        z_top = torch.randn(3, *model.base_distribution.size)
        eps = {i: torch.randn(3, *model.sequence_modules[i].base.size) for i in splits}
        temperature = {i: (LATENT_TEMPERATURE if i == splits[0] else 1.0) for i in splits}
        latents = {i: eps[i] * temperature[i] for i in splits}
        r64 = reverse_walk(model64, z_top.double(), latents)
        r32 = reverse_walk(model, z_top, latents)
        near = rm.near_integer(r64["rev.L1.out"].numpy())
        same = (r32["rev.L0.out"].numpy() == r64["rev.L0.out"].numpy()) | near
        if near.mean() <= rm.MAX_EXCLUDED and bool(same.all()):
            break
    else:
        raise RuntimeError("no draw of the latents gives comparable images")
    rstep32 = reverse_walk(model, z_top, latents, recorded=r64)
    arrays["rev.z.top"] = z_top.numpy()
    for i in splits:
        arrays["rev.z.L%d" % i], arrays["rev.eps.L%d" % i] = latents[i].numpy(), eps[i].numpy()
        arrays["rev.temperature.L%d" % i] = np.asarray(temperature[i])
    f64.update(r64)
    f32.update(r32)
    step32.update(rstep32)

    for k, v in f64.items():
        arrays["f64." + k] = v.numpy()
    for k, v in f32.items():
        arrays["f32." + k] = v.numpy()
    got64.update(f64)
    got32.update(f32)

    # the recorder's condition: the reference's own float32 error within a quarter of every bar
    yard, worst = {}, 0.0
    pairs = {q: ((step32[q] if q in step32 else got32[q]), want) for q, want in got64.items() if q != "rev.L0.out"}
    # through the whole model, on the float32 chain: the top latent, the factored-out halves, the image in front of the floor
    chain = {"z": "fwd.L%d.out" % (n_layers - 1), "decode.image": "rev.L1.out", **{"half.L%d" % i: "fwd.L%d.half" % i for i in splits}}
    pairs.update({q: (got32[src], got64[src]) for q, src in chain.items()})
    for q, (got, want) in pairs.items():
        ref32 = rm.error(got.numpy(), want.numpy())
        yard[q] = {"ref32": ref32, "bar": rm.base_bar(q)}
        worst = max(worst, ref32 / (rm.YARD_SHARE * rm.base_bar(q)))
    yard["images"] = {"excluded": float(near.mean()), "ref32_differ": int((~same).sum()), "bar": rm.MAX_EXCLUDED}
    return arrays, yard, worst, n_layers


def record_model(name):
    tried = []
    for k in range(MAX_DRAWS):
        arrays, yard, worst, _ = record(name, FIRST_SEED[name] + k)
        tried.append((worst, FIRST_SEED[name] + k))
        print("%s seed %d: worst share of a quarter bar %.2f" % (name, FIRST_SEED[name] + k, worst))
        if worst <= 1.0:
            break
    else:                                                  # no draw meets it: the best one, and four times its errors as bars
        arrays, yard, worst, _ = record(name, min(tried)[1])
        for q, y in yard.items():
            if y.get("ref32", 0.0) > rm.YARD_SHARE * y["bar"]:
                y["bar"] = y["ref32"] / rm.YARD_SHARE
                print("  %s: reference float32 error %.3e, bar raised to %.3e" % (q, y["ref32"], y["bar"]))
    arrays["yard"] = np.asarray(json.dumps(yard, sort_keys=True))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("%s: seed %d, %d KiB" % (name, int(arrays["seed"]), os.path.getsize(path) // 1024))
    return yard, int(arrays["seed"])


def record_keys():
    keys = {}
    for image in rm.KEY_IMAGES:
        for actnorm in (False, True):
            for split_prior in (False, True):
                model = build(image, rm.KEY_CONFIG["num_blocks"], rm.KEY_CONFIG["block_size"], actnorm, split_prior)
                keys[rm.key_config_name(image, actnorm, split_prior)] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(rm.KEYS_FILE, "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write("\n")
    print("model_state_keys:", len(keys), "configurations,", os.path.getsize(rm.KEYS_FILE) // 1024, "KiB")


if __name__ == "__main__":
    profile = {}
    for model_name in rm.MODELS:
        y, s = record_model(model_name)
        profile[model_name] = {"seed": s, "quantities": y}
    record_keys()
    out = os.path.join(REPO, "profiles", "reference_model")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "recorder_yardsticks.json"), "w") as f:
        json.dump(profile, f, indent=1, sort_keys=True)
        f.write("\n")
