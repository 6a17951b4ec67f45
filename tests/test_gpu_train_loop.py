"""The model used the way its users use it -- `create_model(...)`, an optimiser, `log_prob(x).mean().backward()`, `step()`, with
`sample` / `sample_with_log_prob` / `rsample_with_log_prob` between the steps -- against the float64 CPU twin of tests/flow_twin.py
at the HIP model's CURRENT parameters ("teacher forcing": the twin is synced before every comparison, so no optimiser round-off
reaches a bar).  What this sees and no kernel test can: a value derived from the parameters on the host (the PackedWeights bank
cache, Conv1x1's inverse / log-det / folded matrices, the coupling's scale and shift, ActNorm's data-dependent init) that is one
optimiser step old gives a plausible answer from last step's weights.

Bars (helpers.rel_err: max-norm, relative to the reference tensor's maximum): loss, log_prob, log_q and ActNorm's init parameters
1e-5 (BASELINE.json); gradients and samples through the whole model CHAIN_TOL of tests/test_gpu_inverse_backward.py (5e-5);
a gradient whose float64 reference is identically zero must be exactly zero.  Beside every HIP error the parity report (kind
`train_loop`) holds the yardstick: the float32 twin on the CPU against the float64 twin, same parameters, inputs and draws.
Worst over a run on an MI355X, HIP / yardstick: gradients 5.0e-6 / 7.1e-6, loss and log_prob 3.6e-7 / 2.6e-7, samples and
reconstructions 1.1e-6 / 1.0e-6, log_q 2.5e-7 / 2.7e-7, ActNorm's init 1.3e-6 / 1.0e-6; a sample from caches one SGD step old: 4.9e-3.

Gradient comparisons differentiate the same branch of the coupling nets' ReLUs on both sides (flow_twin.recorded_masks): without
that, about one pass in twenty has an activation within float32 rounding of zero whose side differs, and gradients behind it are
off by per cent (found here: `reverse_kl/grads` 5.5e-2 at 8.net.0.weight with x and log_q of the same pass within 8e-7).

What this test found: PyTorch's fused optimisers do not advance `Tensor._version`, so every cache keyed on (address, version) kept
last step's values -- `log_prob` under no_grad 5.7e-3 off after the first `Adam(fused=True)` step.  `ops.version_key` now also counts
optimiser steps.
"""
import copy
import inspect
import math

import numpy as np
import pytest
import torch

import flow_twin
from flow_twin import compare, recorded_masks, recorded_noise, replayed_masks, replayed_noise
from helpers import rel_err, same_bits
from test_gpu_inverse_backward import CHAIN_TOL

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODEL_A = dict(num_blocks=3, block_size=2, actnorm=True, split_prior=True, image_size=(3, 16, 16), preprocess=False, coupling_width=16)
MODEL_B = dict(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 32, 32), preprocess=True, coupling_width=16)
BATCH = 8
STEPS = 6
MAX_NORM = 1.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# the pieces
# ---------------------------------------------------------------------------------------------------------------------------------
class Counter:
    """Counts the calls of the entry points of fincflow_amd.ops the model's layers go through, and the launches of the units' bank
    cache that returned a result (patched in place, restored by monkeypatch)."""
    OPS = ("conv_forward", "inverse_reverse", "actnorm_forward", "actnorm_reverse", "finc_actnorm_init", "mix_forward", "coupling_forward",
           "coupling_reverse_logdet", "finc_coupling", "finc_coupling_reverse_logdet", "finc_mix")
    CACHE = ("forward_affine", "inverse", "inverse_affine", "inverse_premultiplied")

    def __init__(self, monkeypatch):
        from fincflow_amd import ops
        self.n = {}
        for name in self.OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        for name in self.CACHE:
            monkeypatch.setattr(ops.PackedWeights, name, self._wrap("cache." + name, getattr(ops.PackedWeights, name)))

    def _wrap(self, name, fn):
        def counted(*args, **kwargs):
            out = fn(*args, **kwargs)
            if out is not None:
                self.n[name] = self.n.get(name, 0) + 1
            return out
        return counted

    def take(self):
        n, self.n = self.n, {}
        return n


def counts_of(model):
    kinds = [type(m).__name__ for m in model.modules()]
    return dict(units=kinds.count("FastFlowUnit"), actnorms=kinds.count("ActNorm"), mixes=kinds.count("Conv1x1"),
                couplings=kinds.count("Coupling"))


def make_model(dev, cfg, seed=0):
    from fincflow_amd import glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    return flow_twin.randomise(glow.create_model(**cfg), seed=seed + 1).to(dev)


def images(cfg, n=BATCH, seed=4):
    return torch.randn(n, *cfg["image_size"], generator=torch.Generator().manual_seed(seed))


def on_device(model):
    return next(model.parameters()).is_cuda


def placer(model):
    """CPU float32 tensor -> a fresh tensor on the model's device, in its dtype."""
    p = next(model.parameters())
    return lambda t: t.detach().to(device=p.device, dtype=p.dtype, copy=True)


def bpd(log_prob, x):
    """The loss: bits per dimension."""
    return -log_prob.mean() / (x[0].numel() * math.log(2))


class Twins:
    """The float64 twin (the reference) and the float32 twin (the yardstick) of one model."""

    def __init__(self, model):
        self.t64, self.t32 = flow_twin.twin_of(model), flow_twin.twin_of(model, torch.float32)

    def sync(self, model):
        flow_twin.sync(self.t64, model)
        flow_twin.sync(self.t32, model)

    def __iter__(self):
        return iter((self.t64, self.t32))


def three(model, twins, fn, pick=None):
    """`fn(m, put)` on the HIP model with its draws and the activation patterns of its nn.ReLU modules recorded (the coupling nets
    under autograd: see flow_twin.recorded_masks), then on both twins with both replayed: (got, want, yard, draws)."""
    with recorded_noise(model) as draws, recorded_masks(model) as masks:
        got = fn(model, placer(model))
    outs = []
    for tw in twins:
        with replayed_noise(tw, draws, pick), replayed_masks(tw, masks) as flips:
            outs.append(fn(tw, placer(tw)))
        if flips[0]:
            print("train_loop: %d of the twin's activations took the model's side of zero" % flips[0])
    return got, outs[0], outs[1], draws


def named_grads(model):
    return {n: p.grad for n, p in model.named_parameters()}


def forward_kl(model, x_parts):
    """The training direction: bits per dimension of the batch, as one backward per micro-batch accumulating into `.grad`.  Returns
    [loss, log_prob per image, the input's gradient]; the parameters' gradients are left in `.grad` (masked on a twin)."""
    put = placer(model)
    total, lps, gxs = 0.0, [], []
    for part in x_parts:
        x = put(part).requires_grad_(True)
        lp = model.log_prob(x)
        loss = bpd(lp, x) / len(x_parts)
        loss.backward()
        total = total + loss.detach()
        lps.append(lp.detach())
        gxs.append(x.grad)
    if not on_device(model):
        flow_twin.mask_unit_grads(model)
    return [total, torch.cat(lps), torch.cat(gxs)]


def judge_grads(tag, model, twins, extra_names, extra, **fields):
    """Every parameter gradient in `.grad` of the three models, and `extra` = (got, want, yard) lists: None on the same parameters,
    CHAIN_TOL on the rest, exact zeros under the corner-tap mask on the HIP side."""
    g, w, y = named_grads(model), named_grads(twins.t64), named_grads(twins.t32)
    assert [n for n in g if g[n] is None] == [n for n in w if w[n] is None], "`.grad is None` differs between the HIP model and the twin"
    names = [n for n in g if g[n] is not None]
    for n, mask in flow_twin.stored_masks(model).items():
        assert not bool(g[n].cpu()[mask == 0].any()), "%s: a gradient under the corner-tap mask is not zero" % n
    compare(tag, names + extra_names, [g[n] for n in names] + extra[0], [w[n] for n in names] + extra[1],
            [y[n] for n in names] + extra[2], bar=CHAIN_TOL, **fields)


def clip(model, twins, **fields):
    norms = [torch.nn.utils.clip_grad_norm_(m.parameters(), MAX_NORM) for m in (model, twins.t64, twins.t32)]
    compare("clip_grad_norm", ["total_norm"], *[[n] for n in norms], bar=CHAIN_TOL, **fields)


def initialise(model, x, dev):
    """The first call: ActNorm's data-dependent init, layer by layer."""
    with torch.no_grad():
        model(x.to(dev))
    return model


def optimiser(name, params):
    if name == "sgd":
        return torch.optim.SGD(params, lr=0.05, momentum=0.9)
    if name == "adam":
        return torch.optim.Adam(params, lr=1e-3)
    if "fused" not in inspect.signature(torch.optim.Adam).parameters:
        pytest.skip("this torch build has no Adam(fused=True)")
    return torch.optim.Adam(params, lr=1e-3, fused=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the inference views of one set of parameters (c)
# ---------------------------------------------------------------------------------------------------------------------------------
def view_log_prob(model, twins, x, counter=None, **fields):
    def fn(m, put):
        with torch.no_grad():
            return [m.log_prob(put(x))]
    got, want, yard, _ = three(model, twins, fn)
    if counter is not None:
        n, c = counter.take(), counts_of(model)
        assert n.get("cache.forward_affine") == c["units"] and n.get("finc_mix") == c["mixes"] and n.get("finc_coupling") == c["couplings"], n
    return compare("log_prob_no_grad", ["log_prob"], got, want, yard, bar=TOL, **fields)


def view_sample(model, twins, n=BATCH, bar=CHAIN_TOL, counter=None, **fields):
    def fn(m, put):
        with torch.no_grad():
            x, x_true = m.sample(n)
            assert x_true is x
            return [x]
    got, want, yard, _ = three(model, twins, fn)
    if counter is not None:
        k, c = counter.take(), counts_of(model)
        solved = k.get("cache.inverse_affine", 0) + k.get("cache.inverse_premultiplied", 0) + k.get("cache.inverse", 0)
        assert solved == c["units"] and k.get("cache.inverse_affine", 0) > 0 and k.get("finc_coupling") == c["couplings"], k
    return compare("sample", ["x"], got, want, yard, bar=bar, **fields)


def view_sample_true_inverse(model, twins, counter=None, **fields):
    def fn(m, put):
        with torch.no_grad():
            x, x_true = m.sample(BATCH, also_true_inverse=True)
            assert x_true is not x
            return [x, x_true]
    got, want, yard, draws = three(model, twins, fn)
    assert len(draws) == 1 + 2 * sum(1 for _ in flow_twin._priors(model)[1:])      # one base draw, every split prior twice
    if counter is not None:
        k, c = counter.take(), counts_of(model)
        assert k.get("cache.inverse", 0) >= c["units"], k                           # the second chain folds nothing
    return compare("sample_true_inverse", ["x", "x_true"], got, want, yard, bar=CHAIN_TOL, **fields)


def view_sample_with_log_prob(model, twins, n=BATCH, pick=None, counter=None, **fields):
    """x against the twin's reverse with the replayed noise; log_q against `twin.log_prob(x)` at the HIP model's x."""
    def fn(m, put):
        return list(m.sample_with_log_prob(n if m is model or pick is None else len(pick)))
    got, want, yard, _ = three(model, twins, fn, pick)
    assert not got[0].requires_grad and not got[1].requires_grad
    if counter is not None:
        k, c = counter.take(), counts_of(model)
        assert k.get("finc_coupling_reverse_logdet") == c["couplings"], k
    if pick is not None:
        got = [g[list(pick)] for g in got]
    compare("sample_with_log_prob/x", ["x"], got[:1], want[:1], yard[:1], bar=CHAIN_TOL, **fields)
    x = got[0].cpu()
    with torch.no_grad():
        lq64, lq32 = (tw.log_prob(placer(tw)(x)) for tw in twins)
    compare("sample_with_log_prob/log_q", ["log_q", "log_q_replayed"], [got[1], got[1]], [lq64, want[1]], [lq32, yard[1]], bar=TOL, **fields)


def view_reconstruct(model, twins, x, **fields):
    def fn(m, put):
        with torch.no_grad():
            return [m.reconstruct(put(x))]
    got, want, yard, _ = three(model, twins, fn)
    return compare("reconstruct", ["x"], got, want, yard, bar=CHAIN_TOL, **fields)


def view_reverse_kl(model, twins, x, counter=None, **fields):
    """`rsample_with_log_prob` and a forward-KL term in ONE backward: the unit's forward and inverse autograd functions sit on the same
    bank-cache entry.  x and log_q of the sample, every gradient of (log_q + |x|^2 / 2).mean() alone, and every gradient of the sum of
    the two objectives (left in `.grad` for the optimiser)."""
    def fn(m, put):
        params = [p for _, p in m.named_parameters()]
        m.zero_grad(set_to_none=True)
        xs, log_q = m.rsample_with_log_prob(BATCH)
        assert xs.requires_grad and log_q.requires_grad
        rev = (log_q + 0.5 * xs.square().flatten(1).sum(1)).mean()
        g_rev = dict(zip([n for n, _ in m.named_parameters()], torch.autograd.grad(rev, params, retain_graph=True, allow_unused=True)))
        xin = put(x)
        (bpd(m.log_prob(xin), xin) + rev / (xin[0].numel() * math.log(2))).backward()
        if not on_device(m):
            g_rev = flow_twin.masked(m, g_rev)
            flow_twin.mask_unit_grads(m)
        return [xs.detach(), log_q.detach()], g_rev
    (got, g_got), (want, g_want), (yard, g_yard), _ = three(model, twins, fn)
    if counter is not None:
        k, c = counter.take(), counts_of(model)
        assert (k.get("inverse_reverse"), k.get("conv_forward")) == (c["units"], c["units"]), k
        assert (k.get("actnorm_reverse"), k.get("actnorm_forward")) == (c["actnorms"], c["actnorms"]), k
        assert (k.get("coupling_reverse_logdet"), k.get("coupling_forward")) == (c["couplings"], c["couplings"]), k
        assert k.get("mix_forward") == 2 * c["mixes"], k
    compare("rsample_with_log_prob/x", ["x"], got[:1], want[:1], yard[:1], bar=CHAIN_TOL, **fields)
    compare("rsample_with_log_prob/log_q", ["log_q"], got[1:], want[1:], yard[1:], bar=TOL, **fields)
    assert [n for n, g in g_got.items() if g is None] == [n for n, g in g_want.items() if g is None]
    names = [n for n, g in g_got.items() if g is not None]
    assert len(names) == len(g_got)                                   # the reverse pass reaches every parameter
    for n, mask in flow_twin.stored_masks(model).items():
        assert not bool(g_got[n].cpu()[mask == 0].any()), n
    compare("reverse_kl/grads", names, [g_got[n] for n in names], [g_want[n] for n in names], [g_yard[n] for n in names], bar=CHAIN_TOL,
            **fields)
    judge_grads("forward_plus_reverse_kl/grads", model, twins, [], ([], [], []), **fields)


def every_view(model, twins, x, counter=None, **fields):
    twins.sync(model)
    if counter is not None:
        counter.take()
    view_log_prob(model, twins, x, counter, **fields)
    view_sample(model, twins, counter=counter, **fields)
    view_sample_true_inverse(model, twins, counter, **fields)
    view_sample_with_log_prob(model, twins, counter=counter, **fields)
    view_reconstruct(model, twins, x, **fields)
    if counter is not None:
        counter.take()
    view_reverse_kl(model, twins, x, counter, **fields)


# ---------------------------------------------------------------------------------------------------------------------------------
# a. data-dependent init in stack order
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_data_dependent_init_runs_in_stack_order(dev, monkeypatch):
    """The first call on a fresh model A initialises every ActNorm on the activations the layers in front of it produce (six
    launches of the init kernel); a fresh float64 twin does the same on the same batch."""
    from fincflow_amd import glow
    model = make_model(dev, MODEL_A)
    twins = Twins(model)
    x = images(MODEL_A)
    counter = Counter(monkeypatch)
    acts = [n for n, m in model.named_modules() if isinstance(m, glow.ActNorm)]
    assert len(acts) == 6 and all(int(m.initialized) == 0 for m in model.modules() if isinstance(m, glow.ActNorm))
    outs = []
    for m in (model, twins.t64, twins.t32):
        xin = placer(m)(x).requires_grad_(True)
        outs.append(m.log_prob(xin).detach())
    k = counter.take()
    assert k.get("finc_actnorm_init") == 6 and k.get("actnorm_forward") == 6 and k.get("conv_forward") == 6, k
    names = [n + s for n in acts for s in (".log_scale", ".translation")]
    params = [dict(m.named_parameters()) for m in (model, twins.t64, twins.t32)]
    compare("actnorm_init/parameters", names, *[[p[n] for n in names] for p in params], bar=TOL)
    compare("actnorm_init/log_prob", ["log_prob"], *[[o] for o in outs], bar=TOL)
    assert all(int(m.initialized) == 1 and m._is_initialized() for tw in (model, twins.t64) for m in tw.modules() if isinstance(m, glow.ActNorm))
    before = {n: params[0][n].detach().clone() for n in names}
    model.log_prob(x.to(dev))
    k = counter.take()
    assert "finc_actnorm_init" not in k and k.get("actnorm_forward") == 6, k
    assert all(same_bits(before[n], params[0][n].detach()) for n in names)


# ---------------------------------------------------------------------------------------------------------------------------------
# b, c. the training direction and every inference view, at every step of a loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["sgd", "adam", "adam_fused"])
def test_every_step_of_a_training_loop_against_the_twin(opt_name, dev, monkeypatch):
    """Six iterations: a forward-KL step compared in the training direction (loss, log_prob, every gradient, the input's gradient),
    then every inference view of the NEW parameters -- which must be this step's answer, not the last one's -- the last of which
    leaves the gradient of forward + reverse KL behind for a second optimiser step.  Iteration 3 accumulates two micro-batches into
    the existing `.grad` buffers."""
    model = initialise(make_model(dev, MODEL_A), images(MODEL_A), dev)
    opt = optimiser(opt_name, model.parameters())
    twins = Twins(model)
    x = images(MODEL_A)
    counter = Counter(monkeypatch)
    c = counts_of(model)
    assert (c["units"], c["actnorms"], c["mixes"], c["couplings"]) == (6, 6, 6, 8)
    for step in range(STEPS):
        tag = dict(opt=opt_name, step=step)
        twins.sync(model)
        accumulate = step == 3
        parts = [x[:BATCH // 2], x[BATCH // 2:]] if accumulate else [x]
        if accumulate:                                      # into the buffers the step before left behind
            buffers = {n: p.grad.data_ptr() for n, p in model.named_parameters()}
            opt.zero_grad(set_to_none=False)
        else:
            opt.zero_grad(set_to_none=True)
        counter.take()
        got, want, yard, _ = three(model, twins, lambda m, put: forward_kl(m, parts))
        k = counter.take()
        assert (k.get("conv_forward"), k.get("actnorm_forward"), k.get("mix_forward"), k.get("coupling_forward")) == \
            tuple(len(parts) * c[n] for n in ("units", "actnorms", "mixes", "couplings")), k
        if accumulate:
            assert buffers == {n: p.grad.data_ptr() for n, p in model.named_parameters()}
        compare("forward_kl/loss", ["bits_per_dim", "log_prob"], got[:2], want[:2], yard[:2], bar=TOL, **tag)
        judge_grads("forward_kl/grads", model, twins, ["input"], (got[2:], want[2:], yard[2:]), **tag)
        clip(model, twins, **tag)
        opt.step()
        every_view(model, twins, x, counter, **tag)
        clip(model, twins, **tag)
        opt.step()                                          # the reverse-KL step of the same iteration


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the test has teeth
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_cache_keyed_on_addresses_alone_is_caught(dev, monkeypatch):
    """With `_version` and the optimiser-step count dropped from `ops.version_key` every derived value survives an in-place optimiser
    step (every pointer stays valid: this only produces wrong numbers): `sample` answers from last step's weights and the comparison
    of (c) says so.  With the key restored it passes again."""
    from fincflow_amd import ops
    x = images(MODEL_A)
    model = initialise(make_model(dev, MODEL_A), x, dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    twins = Twins(model)
    with monkeypatch.context() as patch:
        patch.setattr(ops, "version_key", lambda *tensors: tuple(t.data_ptr() for t in tensors))
        view_sample(model, twins, step="before")            # right, and fills every cache of the sampling pass under the weak key
        forward_kl(model, [x])
        opt.step()
        twins.sync(model)
        stale = view_sample(model, twins, bar=None, step="stale")
    assert stale["x"] > CHAIN_TOL, stale
    fresh = view_sample(model, twins, step="restored")
    assert fresh["x"] <= CHAIN_TOL < stale["x"]


# ---------------------------------------------------------------------------------------------------------------------------------
# e. preprocessing and the premultiplied fold
# ---------------------------------------------------------------------------------------------------------------------------------
def pixel_batch(seed=6):
    """(integer images, the same plus the dequantisation noise U[0,1), drawn once for both sides).  Grey levels 16..239: next to 255
    the logit's 1 - x is a difference of nearly equal float32 numbers, and the float32 twin itself misses the gradient bar there
    (input gradient 1.2e-3 against the float64 twin with levels 0..255) -- the inputs were changed, not the bar."""
    gen = torch.Generator().manual_seed(seed)
    pixels = torch.randint(16, 240, (BATCH,) + MODEL_B["image_size"], generator=gen)
    return pixels, pixels.float() + torch.rand(pixels.shape, generator=gen)


def model_b(dev):
    """(the full model, the container from `list(model)[1:]`: the same modules without the dequantisation layer)."""
    from fincflow_amd import FlowSequential, glow
    model = make_model(dev, MODEL_B)
    assert isinstance(list(model)[0], glow.Dequantization)
    inner = FlowSequential(model.base_distribution, *list(model)[1:])
    assert all(p is q for p, q in zip(model.parameters(), inner.parameters()))
    return model, inner


def test_a_training_step_through_the_preprocessing_layers(dev, monkeypatch):
    """Integer images, the dequantisation noise drawn once and fed to both sides; Normalization, LogitTransform and their log-dets
    are in the chain."""
    model, inner = model_b(dev)
    pixels, x = pixel_batch()
    assert pixels.dtype == torch.int64
    initialise(inner, x, dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    twins = Twins(inner)
    counter = Counter(monkeypatch)
    for step in range(2):                                  # (the second round: the same comparison after the step)
        twins.sync(inner)
        opt.zero_grad(set_to_none=True)
        got, want, yard, _ = three(inner, twins, lambda m, put: forward_kl(m, [x]))
        k = counter.take()
        assert (k.get("conv_forward"), k.get("actnorm_forward"), k.get("mix_forward"), k.get("coupling_forward")) == (2, 2, 2, 3), k
        compare("preprocess/forward_kl/loss", ["bits_per_dim", "log_prob"], got[:2], want[:2], yard[:2], bar=TOL, step=step)
        judge_grads("preprocess/forward_kl/grads", inner, twins, ["input"], (got[2:], want[2:], yard[2:]), step=step)
        opt.step()


def test_sampling_on_the_premultiplied_fold(dev, monkeypatch):
    """`sample_with_log_prob` at the smallest batch for which the library says the first level's inverse takes the premultiplied form
    (mix -> ActNorm -> unit in two launches); the twin evaluates the first, the last and two inner images.  The comparison stops in
    front of the dequantisation's floor; the full model's sample is the floor of that."""
    from fincflow_amd import _lib
    model, inner = model_b(dev)
    C, H, W = MODEL_B["image_size"][0] * 4, MODEL_B["image_size"][1] // 2, MODEL_B["image_size"][2] // 2
    n = next(b for b in range(1, 1025) if _lib.lib().finc_inverse_premultiplied_supported(b, 4, C // 4, H, W, 3, 3))
    assert n > BATCH and not _lib.lib().finc_inverse_premultiplied_supported(n - 1, 4, C // 4, H, W, 3, 3)
    initialise(inner, pixel_batch()[1], dev)
    twins = Twins(inner)
    pick = [0, n // 3, 2 * n // 3, n - 1]
    counter = Counter(monkeypatch)
    view_sample_with_log_prob(inner, twins, n=n, pick=pick, batch=n)
    k = counter.take()
    assert k.get("cache.inverse_premultiplied") == 1 and k.get("cache.inverse_affine") == 1 and "cache.inverse" not in k, k
    torch.manual_seed(8)
    x_inner, lq_inner = inner.sample_with_log_prob(n)
    torch.manual_seed(8)
    x_full, lq_full = model.sample_with_log_prob(n)
    assert same_bits(x_full, x_inner.floor()) and not same_bits(x_full, x_inner)
    assert rel_err(lq_full.cpu().numpy(), lq_inner.cpu().numpy()) <= 1e-6        # (the floor's layer adds zeros)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. copies and checkpoints mid-training
# ---------------------------------------------------------------------------------------------------------------------------------
def seeded_sample(model, seed=21):
    torch.manual_seed(seed)
    with torch.no_grad():
        return model.sample(BATCH)[0]


def test_copies_and_checkpoints_mid_training(dev):
    x = images(MODEL_A)
    model = initialise(make_model(dev, MODEL_A), x, dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        forward_kl(model, [x])
        opt.step()
    for _ in range(3):
        step()
        seeded_sample(model)                               # (the model's caches are warm when it is copied)
    ema = copy.deepcopy(model)
    then = seeded_sample(model)
    ema_then = seeded_sample(ema)
    assert same_bits(ema_then, then)
    step()
    assert not same_bits(seeded_sample(model), then)       # the model moved on ...
    assert same_bits(seeded_sample(ema), ema_then)         # ... the copy did not: no shared bank
    with torch.no_grad():
        for p_ema, p in zip(ema.parameters(), model.parameters()):
            p_ema.lerp_(p, 0.1)
    assert not same_bits(seeded_sample(ema), ema_then)
    view_sample_with_log_prob(ema, Twins(ema), case_of="ema_after_lerp")

    # a state dict into a fresh model: the same sample from the same seed, bit for bit
    fresh = make_model(dev, MODEL_A, seed=5)
    fresh.load_state_dict(model.state_dict())
    assert same_bits(seeded_sample(fresh), seeded_sample(model))
    # ... and into a model that has sampled already: it follows the loaded weights without anyone calling invalidate()
    other = initialise(make_model(dev, MODEL_A, seed=7), x, dev)
    was = seeded_sample(other)
    other.load_state_dict(model.state_dict())
    assert not same_bits(seeded_sample(other), was) and same_bits(seeded_sample(other), seeded_sample(model))
    twins = Twins(model)
    view_sample(other, twins, case_of="load_state_dict")
    view_sample_with_log_prob(other, twins, case_of="load_state_dict")


# ---------------------------------------------------------------------------------------------------------------------------------
# g. an optimiser that breaks the invariant is refused, not obeyed
# ---------------------------------------------------------------------------------------------------------------------------------
def test_weight_decay_on_the_corner_tap_is_refused(dev):
    """SGD(weight_decay) on the units' raw gradients moves the unit diagonal of the corner tap off 1 (the in-kernel mask zeroes the
    gradient there, the decay term is added behind it): the next `sample` raises instead of solving a different system."""
    from fincflow_amd import PaddedConv2d, _lib
    x = images(MODEL_A)
    model = initialise(make_model(dev, MODEL_A), x, dev)
    seeded_sample(model)
    convs = [m for m in model.modules() if isinstance(m, PaddedConv2d)]
    taps = [m.conv.weight.detach().clone() for m in convs]
    opt = torch.optim.SGD(model.parameters(), lr=0.1, weight_decay=0.1)
    forward_kl(model, [x])
    opt.step()
    with pytest.raises(_lib.FincError):
        model.sample(BATCH)
    with pytest.raises(_lib.FincError):
        model.sample_with_log_prob(BATCH)
    with torch.no_grad():
        for m, w in zip(convs, taps):
            keep = m.mask.to(dev).bool()
            m.conv.weight.copy_(torch.where(keep, m.conv.weight, w))
    twins = Twins(model)
    view_sample(model, twins, case_of="taps_restored")
    view_sample_with_log_prob(model, twins, case_of="taps_restored")
