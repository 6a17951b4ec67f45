"""What tests/golden/make_golden_model.py (the recorder), tests/test_reference_model_host.py and tests/test_gpu_reference_model.py
share: the two recorded models, the names of the recorded quantities, the bars and the yardstick.  A helper, not collected.

The fixtures `tests/golden/model_mnist.npz` / `model_cifar.npz` hold a whole model built from the reference's own classes in the
order of its create_model (fastflow/fastflow_cifar.py:35-63), walked on the CPU in float64 and in float32:

    seed, image                                the recorder's seed (after re-draws) and the image shape
    state.<key>                                the complete state dict under the reference's keys (float32, as it stores them)
    init.x, init.u                             the 8-image batch (uint8) and its noise of the ActNorm initialisation
    init.state.<key>                           the units' weights and the Conv1x1 matrices as constructed, which that forward depends on
    init64.<key>, init32.<key>                 the ActNorm parameters that first forward leaves, in float64 and float32
    x, u                                       the 3-image batch (uint8) and its noise
    f64.fwd.L<i>.out / .logdet [B]             layer i's output and log-det on the recorded input of its position (L<i-1>.out; x + 0)
    f64.fwd.L<i>.half                          what SplitPrior i factors out: the second half of its transform's output
    f64.log_prob [B]                           of the whole model (z is the last layer's out)
    f64.grad.<parameter>                       of -log_prob.mean(), the units' after their own reset_gradients()
    rev.z.top, rev.z.L<i>, rev.eps.L<i>, rev.temperature.L<i>     the latents of the reverse walk (z = temperature * eps)
    f64.rev.L<i>.out                           layer i's reverse on the recorded input of its position (L<i+1>'s out; rev.z.top)
    f32.*                                      the same walks in the reference's native float32, each layer on ITS OWN chain
    yard                                       JSON: quantity -> {"ref32": the reference's float32 error, "bar": what the quantity is held to}

`yard` has one entry per recorded quantity.  For `fwd.L<i>.*` and `rev.L<i>.out` ref32 is the float32 LAYER on the float64
recording's input (what the per-layer walks do); for everything else it is the float32 chain.
"""
import contextlib
import functools
import json
import os

import numpy as np

from helpers import GOLDEN, rel_err

#: the recorded models: what `glow.create_model` takes beside CONFIG
MODELS = {"model_mnist": dict(image_size=(1, 28, 28)), "model_cifar": dict(image_size=(3, 16, 16))}
CONFIG = dict(num_blocks=2, block_size=1, actnorm=True, split_prior=True, coupling_width=16)
#: the key lists: 3 blocks of 2 at the reference's own coupling width, (actnorm, split_prior) in all four combinations
KEY_IMAGES = [(1, 28, 28), (3, 32, 32), (3, 64, 64)]
KEY_CONFIG = dict(num_blocks=3, block_size=2)
KEYS_FILE = os.path.join(GOLDEN, "model_state_keys.json")

#: the project's bars: one layer in float32, values through a stack in float32, anything in float64
BAR_LAYER, BAR_MODEL, BAR_F64 = 1e-5, 5e-5, 1e-12
#: a recorded quantity's bar holds only where the reference's own float32 error is within this share of it
YARD_SHARE = 0.25
#: images behind the floor are compared exactly except where the recorded continuous value is this close to an integer
#: (5e-5 of a 0..256 range is 0.013), which may exclude at most this share of the pixels (expected: 4 %)
NEAR_INTEGER, MAX_EXCLUDED = 0.02, 0.10


def base_bar(quantity):
    """The bar the issue sets for a quantity, before the recorder's condition is applied."""
    return BAR_LAYER if quantity.startswith(("fwd.", "rev.", "init.")) else BAR_MODEL


def error(got, want):
    """helpers.rel_err; a reference that is identically zero (a unit's log-det, a masked gradient) asks for exact zeros."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.any(want):
        return 0.0 if not np.any(got) else float("inf")
    return rel_err(got, want)


def key_config_name(image, actnorm, split_prior):
    return "%dx%dx%d.actnorm%d.split%d" % (*image, int(actnorm), int(split_prior))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """The arrays of one recorded model, read once and shared; read-only."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        out = {k: f[k] for k in f.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def yard(name):
    return json.loads(str(fixture(name)["yard"]))


def bar(name, quantity, double=False):
    """What a quantity is held to: the recorded bar in float32, 1e-12 in float64; the images behind the floor (`rev.L0.out`,
    `images`: 1.0 for any difference outside the pixels left out) are compared exactly."""
    if quantity in ("rev.L0.out", "images"):
        return 0.0
    return BAR_F64 if double else yard(name)[quantity]["bar"]


def recorded_state(name, prefix=""):
    """The recorded state dict as fresh tensors, in the recorded order."""
    import torch
    return {prefix + k[len("state."):]: torch.from_numpy(v.copy()) for k, v in fixture(name).items() if k.startswith("state.")}


def tensor(name, key, dtype=None, device=None):
    """A fresh tensor of one recorded array."""
    import torch
    t = torch.from_numpy(fixture(name)[key].copy())
    return t.to(device=device, dtype=dtype if dtype is not None else t.dtype)


def build(name, **overrides):
    from fincflow_amd import glow
    return glow.create_model(**dict(CONFIG, **MODELS[name], **overrides))


def forward_input(name, i, dtype, device=None, which="f64"):
    """The recorded input of layer i's position in the forward walk: the images themselves in front of layer 0."""
    if i == 0:
        return tensor(name, "x").to(device=device, dtype=dtype)
    return tensor(name, "%s.fwd.L%d.out" % (which, i - 1), dtype, device)


def reverse_input(name, i, n_layers, dtype, device=None, which="f64"):
    """The recorded input of layer i's position in the reverse walk: the top latent behind the last layer."""
    if i == n_layers - 1:
        return tensor(name, "rev.z.top", dtype, device)
    return tensor(name, "%s.rev.L%d.out" % (which, i + 1), dtype, device)


def near_integer(values):
    """The pixels of a recorded continuous image that the comparison behind the floor leaves out."""
    v = np.asarray(values, dtype=np.float64)
    return np.abs(v - np.round(v)) < NEAR_INTEGER


# ---------------------------------------------------------------------------------------------------------------------------------
# the walks: every layer on the recorded input of its position
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def handed_noise(u):
    """Inside the context the dequantisation noise is `u`: `torch.rand_like` and `torch.rand` hand it out where its shape is asked
    for (the layer's draw and the fused image boundary's), and draw as they always do anywhere else.  A device generator cannot
    reproduce a draw made on the CPU, so seeding is no alternative."""
    import torch
    rand, rand_like = torch.rand, torch.rand_like

    def patched_rand(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        return u.clone() if shape == tuple(u.shape) else rand(*size, **kw)

    def patched_rand_like(t, **kw):
        return u.clone() if tuple(t.shape) == tuple(u.shape) else rand_like(t, **kw)

    torch.rand, torch.rand_like = patched_rand, patched_rand_like
    try:
        yield
    finally:
        torch.rand, torch.rand_like = rand, rand_like


@contextlib.contextmanager
def handed_latent(layer, z):
    """Inside the context `layer.base.sample` returns `z` (a SplitPrior's draw in `reverse`)."""
    layer.base.sample = lambda n_samples, context=None: (z, None)
    try:
        yield
    finally:
        del layer.base.sample


def per_image(logdet, n):
    """A layer's log-det as [n] float64: the layers hand out 0.0, a 0-dim tensor or [B]."""
    import torch
    v = logdet.detach().double().cpu().numpy() if torch.is_tensor(logdet) else np.float64(logdet)
    return np.broadcast_to(v, (n,)).astype(np.float64)


def layer_walk(model, name, dtype, device=None, skip=()):
    """Every layer of `model` (but those of the types in `skip`) on the float64 recording's input of its position, forward and
    reverse, without a graph: quantity -> achieved error against the float64 recording.  A SplitPrior is asked three ways: `forward`
    (out, log p), `split` (the factored-out half as well) and, backwards, `reverse` on the recorded draw and `merge`.  The floor of
    Dequantization.reverse is compared exactly (1.0 for any difference) outside the pixels `near_integer` leaves out."""
    import torch
    fx, mods, errs = fixture(name), list(model.sequence_modules), {}
    n = len(fx["x"])
    u = tensor(name, "u", dtype, device)
    with torch.no_grad():
        for i, m in enumerate(mods):
            if isinstance(m, skip):
                continue
            h = forward_input(name, i, dtype, device)
            with handed_noise(u):
                out, ld = m(h, None)
            errs["fwd.L%d.out" % i] = error(out.cpu().numpy(), fx["f64.fwd.L%d.out" % i])
            errs["fwd.L%d.logdet" % i] = error(per_image(ld, n), fx["f64.fwd.L%d.logdet" % i])
            if hasattr(m, "split"):
                x1, z2, lp = m.split(h, None)
                errs["fwd.L%d.half" % i] = error(z2.cpu().numpy(), fx["f64.fwd.L%d.half" % i])
                errs["fwd.L%d.out" % i] = max(errs["fwd.L%d.out" % i], error(x1.cpu().numpy(), fx["f64.fwd.L%d.out" % i]))
                errs["fwd.L%d.logdet" % i] = max(errs["fwd.L%d.logdet" % i], error(per_image(lp, n), fx["f64.fwd.L%d.logdet" % i]))
        for i in reversed(range(len(mods))):
            m = mods[i]
            if isinstance(m, skip):
                continue
            h, want = reverse_input(name, i, len(mods), dtype, device), fx["f64.rev.L%d.out" % i]
            if hasattr(m, "merge"):
                z = tensor(name, "rev.z.L%d" % i, dtype, device)
                with handed_latent(m, z):
                    outs = [m.reverse(h, None), m.merge(h, z, None)]
            else:
                out = m.reverse(h, None)
                outs = [out[0] if isinstance(out, tuple) else out]
            for out in outs:
                if i == 0:
                    differ = (out.cpu().numpy() != want) & ~near_integer(fx["f64.rev.L1.out"])
                    e = float(differ.any())
                else:
                    e = error(out.cpu().numpy(), want)
                errs["rev.L%d.out" % i] = max(errs.get("rev.L%d.out" % i, 0.0), e)
    return errs
