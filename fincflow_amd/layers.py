"""Drop-in modules for the reference's hot-path layers.

Same constructor signatures, attribute names, state-dict keys and
forward -> (out, logdet) / reverse protocol as

  * fastflow/layers/flowlayer.py:8-30      FlowLayer (ABC)
  * fastflow/layers/conv.py:21-221          PaddedConv2d
  * fastflow/fastflow.py:13-100             FastFlowUnit

so a reference `FlowSequential` (layers/flowsequential.py:21-44,89-115) or
`FastFlowStep` (fastflow_cifar_multi_gpu.py:224-256) can hold them unchanged.
The arithmetic runs in libfinc_hip.so; there is no CPU path.
"""
import math
from abc import ABCMeta, abstractmethod
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib, ops


def _hip_tensor(x):
    """The activations every HIP path of the model takes: fp32, [B,C,H,W], on the device."""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4


def _records_graph(x, *params):
    """Does a call on `x` with these parameters (None: absent) record an autograd graph?"""
    return torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params))


def _per_image_logdet(logdet, out):
    """A layer's log-det as a [B] tensor beside `out`: a Python number or a 0-dim tensor (the same for every image) is broadcast."""
    if not torch.is_tensor(logdet):
        return out.new_full((len(out),), float(logdet))
    return logdet.expand(len(out)) if logdet.dim() == 0 else logdet


class BackwardNeeds(NamedTuple):
    """What a `backward_from_output` call has to produce (everything else comes back as None and costs no launch)."""
    input: bool = True           # the rebuilt input: what the layer in front is handed as ITS output
    grad_input: bool = True
    grad_context: bool = False
    params: object = True        # one bool for all of `list(layer.parameters())`, or one per parameter


def _param_needs(layer, needs):
    """`needs.params` per parameter of `layer`, False for a frozen one."""
    params = list(layer.parameters())
    asked = [bool(needs.params)] * len(params) if isinstance(needs.params, bool) else list(needs.params)
    if len(asked) != len(params):
        raise ValueError("needs.params must hold one entry per parameter of the layer")
    return params, [a and p.requires_grad for a, p in zip(asked, params)]


def _params_on_device(x, *params):
    return all(p.dtype == torch.float32 and p.device == x.device for p in params)


def _unit_backward_from_output(cache, cache_args, y, grad_y, need_x, need_gx, need_gw):
    """The invertible backward of a unit on the cache `cache`: x = inverse(y) without the invariant check (the training path: the
    in-kernel gradient mask keeps the corner tap unit triangular, and a check per unit and step is a host synchronisation), then
    `ops.finc_backward` at (grad_y, x) and canonical -> stored as `ops._FincConvFunction.backward` does.  There is no re-forward.
    Returns (x, grad_x, [grad of each stored bank] or None)."""
    weights, G, orient = cache_args
    x = gx = gws = None
    if need_x or need_gw:
        x = cache.inverse(y.contiguous(), weights, G, orient, validate=False)
    if need_gx or need_gw:
        w_canon = cache._get(weights, G, orient, validate=False).w_canon         # (same entry: no check, no synchronisation)
        gx, gw = ops.finc_backward(grad_y.contiguous(), x, w_canon, G, orient, need_gx=need_gx, need_gw=need_gw)
        if gw is not None:
            gw = ops.canonicalize(gw, G, orient)  # canonical -> stored orientation
            gws = list(gw.chunk(len(weights), dim=0)) if len(weights) > 1 else [gw]
    return x, gx, gws


class FlowLayer(nn.Module, metaclass=ABCMeta):
    """layers/flowlayer.py:8-30."""

    @abstractmethod
    def forward(self, input, context=None):
        pass

    @abstractmethod
    def reverse(self, input, context=None):
        pass

    @abstractmethod
    def logdet(self, input, context=None):
        pass

    def reverse_with_logdet(self, input, context=None):
        """`(out, logdet[B])`: `out` is what `reverse(input, context)` returns on the same path, `logdet` what
        `forward(out, context)[1]` returns -- the FORWARD map's log-det at the recovered input, so that a sampler adds it to the base
        density: log q(x) = log p(z) + sum over the layers.  Every layer of this package overrides it with a form that costs no second
        pass; this default is for a layer from elsewhere (one `forward` more)."""
        out = self.reverse(input, context)
        out = out[0] if isinstance(out, tuple) else out
        return out, _per_image_logdet(self.forward(out, context)[1], out)

    # The protocol of `FlowSequential.invertible_backward`: a layer that can differentiate from its OUTPUT.
    def invertible_backward_supported(self, input, context=None):
        """Can `backward_from_output` serve a `forward(input, context)` call?  Reads the tensors' shape, dtype and device only (the
        container asks before the activations exist).  A layer from elsewhere inherits this False and keeps its stored activations."""
        return False

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """Given `forward`'s output, the gradient that reaches it, the gradient of the log-det ([B] or None) and a `BackwardNeeds`:
        `(input, grad_input, grad_context, param_grads)` -- the input REBUILT from the output and the gradients taken there, in the
        same pass.  `param_grads` is aligned with `list(self.parameters())`; whatever `needs` does not ask for, and the gradient of
        a frozen parameter, is None."""
        raise NotImplementedError

    def reconstruct_forward(self, input, context=None):
        return self.forward(input)

    def reconstruct_reverse(self, input, context=None):
        return self.reverse(input)


class PaddedConv2d(FlowLayer):
    """One-corner zero-padded, bias-free, unit-triangular conv (layers/conv.py:21-221).

    `self.conv.weight` is stored flipped per `order` exactly like the reference
    (layers/conv.py:72-79), so reference checkpoints load with `load_state_dict`.
    """

    def __init__(self, in_channels, out_channels, kernel_size, bias=False, order='TL'):
        super().__init__()
        assert len(kernel_size) == 2
        assert order in {'TL', 'TR', 'BL', 'BR'}, 'unknown order: {}'.format(order)
        if in_channels != out_channels:
            raise ValueError("an invertible conv needs in_channels == out_channels")
        self.kernel_size = kernel_size
        self.order = order
        K_H, K_W = kernel_size[0], kernel_size[1]
        # (left, right, top, bottom), layers/conv.py:41-55
        self.pad = {'TL': (K_W - 1, 0, K_H - 1, 0), 'TR': (0, K_W - 1, K_H - 1, 0),
                    'BL': (K_W - 1, 0, 0, K_H - 1), 'BR': (0, K_W - 1, 0, K_H - 1)}[order]
        # Parameter holder only, and bias-free WHATEVER the argument says -- exactly as the reference builds it
        # (layers/conv.py:60 hard-codes bias=False), so the state dict has the one key `conv.weight` and reference
        # checkpoints load strictly.  The reference then carries a dead `conv.bias is not None` branch in its reverse
        # (layers/conv.py:113-117); here `bias=True` makes that branch live through a parameter of the layer's OWN,
        # `bias` (zero-initialised, as the reference's reset would leave a bias): conv(x) + b, and the reverse subtracts b
        # first -- a per-channel add around the same two launches.  The FInC unit never sets it (fastflow.py:24-27).
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self._cache = ops.PackedWeights()
        self.reset_parameters()

    @property
    def _orient(self):
        return ops.ORDER_BITS[self.order]

    def _flip(self, t):
        if self.order == 'TR':
            return torch.flip(t, [3])
        if self.order == 'BL':
            return torch.flip(t, [2])
        if self.order == 'BR':
            return torch.flip(t, [2, 3])
        return t

    def reset_parameters(self):
        """layers/conv.py:63-79."""
        nn.init.normal_(self.conv.weight.data, mean=0.0, std=0.05)
        self.mask = self.get_mask()
        w = self.conv.weight.data
        for c_out in range(w.shape[0]):
            w[c_out, c_out, -1, -1] = 1.0
            w[c_out, c_out + 1:, -1, -1] = 0.0
        self.conv.weight.data = self._flip(w).contiguous()

    def get_mask(self):
        """layers/conv.py:81-96."""
        mask = torch.ones_like(self.conv.weight.data)
        for c_out in range(mask.shape[0]):
            mask[c_out, c_out:, -1, -1] = 0.0
        return self._flip(mask).contiguous()

    def reset_gradients(self):
        """layers/conv.py:98-99.  The HIP backward already writes masked gradients; kept for the runner's
        `model.apply(clear_grad)` (train/experiment.py:16-18)."""
        if self.conv.weight.grad is not None:
            self.conv.weight.grad = self.conv.weight.grad * self.mask.to(self.conv.weight.grad.device)

    def _cache_args(self):   # (weights, G, orient): what the cache's methods take after the activations
        return [self.conv.weight], 1, self._orient

    def forward(self, x, context=None, compute_expensive=None):
        if _records_graph(x, self.conv.weight):
            out = ops.conv_forward(x, *self._cache_args(), self._cache)
        else:  # density evaluation / sampling checks: cached fragments, one launch
            out = self._cache.forward(x.contiguous(), *self._cache_args())
        b = self.bias if self.bias is not None else self.conv.bias          # (conv.bias: set by hand, the reference's dead branch)
        if b is not None:
            out = out + b.view(1, -1, 1, 1)
        return out, 0.0

    def reverse(self, x, context=None, compute_expensive=None):
        """The inverse, DETACHED from autograd (the reference's `reverse` solves outside the graph too, layers/conv.py:109-163) -- unless
        the call sits inside `fincflow_amd.reverse_grad()` and autograd is recording: then the result is attached, with the HIP backward
        of `ops.inverse_reverse` behind it (the bias subtraction stays a differentiable PyTorch line)."""
        b = self.bias if self.bias is not None else self.conv.bias
        if b is not None and b.dtype != x.dtype:      # (the subtraction below would promote the input past the launch's own check)
            raise ValueError(f"input must be {b.dtype}, got {x.dtype}")
        if ops.reverse_grad_enabled() and _records_graph(x, self.conv.weight, b):
            if b is not None:
                x = x - b.reshape(-1, x.shape[1], 1, 1)
            return ops.inverse_reverse(x, *self._cache_args(), self._cache), 0
        with torch.no_grad():
            if b is not None:
                x = x - b.reshape(-1, x.shape[1], 1, 1)
            y = self._cache.inverse(x.contiguous(), *self._cache_args())
        return y, 0

    def reverse_with_logdet(self, x, context=None):
        """`reverse(x)[0]` and the layer's log-det per image: zeros (unit-triangular)."""
        out = self.reverse(x, context)[0]
        return out, out.new_zeros(len(out))

    def invertible_backward_supported(self, x, context=None):
        # (a `conv.bias` set by hand, the reference's dead branch, keeps the stored path)
        return _hip_tensor(x) and self.conv.bias is None and _params_on_device(x, *self.parameters())

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """x = inverse(output - bias), then the HIP backward at (grad_output, x); the bias gradient is grad_output summed per channel."""
        params, asked = _param_needs(self, needs)
        want = {id(p): a for p, a in zip(params, asked)}
        y = output if self.bias is None else output - self.bias.detach().view(1, -1, 1, 1)
        x, gx, gws = _unit_backward_from_output(self._cache, self._cache_args(), y, grad_output, needs.input, needs.grad_input,
                                                want[id(self.conv.weight)])
        grads = {id(self.conv.weight): gws[0] if gws is not None else None}
        if self.bias is not None and want[id(self.bias)]:
            grads[id(self.bias)] = grad_output.sum(dim=(0, 2, 3))
        return x, gx, None, [grads.get(id(p)) for p in params]

    def logdet(self, x=None, context=None):
        return 0.0


class FastFlowUnit(nn.Module):
    """Four PaddedConv2d (TL, TR, BL, BR), one per channel quarter (fastflow.py:13-100), evaluated as ONE
    grouped launch in each direction.  `forward` records an autograd graph whenever one is being recorded; `reverse` returns a
    DETACHED tensor, as it always has, except inside `fincflow_amd.reverse_grad()`, where it is differentiable with respect to its
    input and the four stored banks (`ops.inverse_reverse`: the backward runs the inverse kernels on the adjoint bank)."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        if isinstance(kernel_size, int) or len(kernel_size) == 1:
            kernel_size = (kernel_size, kernel_size) if isinstance(kernel_size, int) else (kernel_size[0],) * 2
        assert in_channels % 4 == 0, "Input channels have to be a multiple of 4"
        out_channels = in_channels // 4  # fastflow.py:21: the argument is overridden
        self.conv_tl = PaddedConv2d(out_channels, out_channels, kernel_size, order='TL')
        self.conv_tr = PaddedConv2d(out_channels, out_channels, kernel_size, order='TR')
        self.conv_bl = PaddedConv2d(out_channels, out_channels, kernel_size, order='BL')
        self.conv_br = PaddedConv2d(out_channels, out_channels, kernel_size, order='BR')
        self._cache = ops.PackedWeights()

    def _weights(self):
        return [self.conv_tl.conv.weight, self.conv_tr.conv.weight, self.conv_bl.conv.weight,
                self.conv_br.conv.weight]

    def _cache_args(self):   # (weights, G, orient): what the cache's methods take after the activations
        return self._weights(), 4, ops.ORIENT_FASTFLOW

    def forward(self, x, context=None):
        if _records_graph(x, *self._weights()):
            out = ops.conv_forward(x, *self._cache_args(), self._cache)
        else:  # density evaluation / sampling checks: cached fragments, one launch
            out = self._cache.forward(x.contiguous(), *self._cache_args())
        return out, 0.0

    def reverse(self, x, context=None):
        return self.reverse_level2(x)

    def reverse_with_logdet(self, x, context=None):
        """`reverse(x)` and the unit's log-det per image: zeros (four unit-triangular banks)."""
        out = self.reverse(x, context)
        return out, out.new_zeros(len(out))

    def invertible_backward_supported(self, x, context=None):
        return _hip_tensor(x) and _params_on_device(x, *self.parameters())

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """x = inverse(output) on the cached bank, then the HIP backward at (grad_output, x): the log-det is 0, `grad_logdet` does not
        enter.  Weight gradients are zero under the corner-tap mask, as on the stored path."""
        params, asked = _param_needs(self, needs)
        x, gx, gws = _unit_backward_from_output(self._cache, self._cache_args(), output, grad_output, needs.input, needs.grad_input,
                                                any(asked))
        grads = {id(w): g for w, g in zip(self._weights(), gws)} if gws is not None else {}
        return x, gx, None, [grads.get(id(p)) if a else None for p, a in zip(params, asked)]

    def reverse_level2(self, x):
        """fastflow.py:78-100 without the 6 flip/cat/zeros copies: the kernel indexes the flipped pixel."""
        if ops.reverse_grad_enabled() and _records_graph(x, *self._weights()):
            return ops.inverse_reverse(x, *self._cache_args(), self._cache)
        with torch.no_grad():
            return self._cache.inverse(x.contiguous(), *self._cache_args())

    def reverse_affine(self, y, log_scale, translation):
        """reverse(exp(log_scale) * y + translation): the ActNorm that follows the unit in the model precedes it in the
        reverse chain, and its affine map rides in the inverse's filter bank at no cost per step.
        Returns None if this shape cannot take the fused path."""
        with torch.no_grad():
            return self._cache.inverse_affine(y.contiguous(), *self._cache_args(), log_scale, translation)

    def reverse_after_mix(self, u, mix, affine=None):
        """reverse(affine(mix.reverse(u))) in TWO launches that cost less than the plain two: the channel mix
        in front of the unit in the reverse chain (Conv1x1.reverse, with the ActNorm between them as a row scaling and a
        bias) also applies blockdiag(Linv_g) of this unit -- the same dense C x C product per pixel -- and the inverse
        runs without its z-term.  `mix` exposes `reverse_premultiplied(u, lead, log_scale, translation)`.  None when this
        call cannot take that path (shape without the kernel, autograd on, CPU tensors)."""
        if _records_graph(u, *self._weights()) or not _hip_tensor(u):
            return None
        with torch.no_grad():
            if not self._cache.premultiplied_supported(tuple(u.shape), *self._cache_args()):
                return None
            lead = self._cache.lead_inverse(*self._cache_args())
            zp = mix.reverse_premultiplied(u, lead, *(affine if affine is not None else (None, None)))
            if zp is None:
                return None
            return self._cache.inverse_premultiplied(zp, *self._cache_args())

    def forward_affine(self, x, log_scale, translation):
        """(forward(x) - translation) * exp(-log_scale): the ActNorm behind the unit rides in the forward bank (SURVEY 8
        f3, forward direction).  Inference only; None if this call cannot take the fused path."""
        if _records_graph(x, *self._weights()):
            return None
        with torch.no_grad():
            return self._cache.forward_affine(x.contiguous(), *self._cache_args(), log_scale, translation)

    def reverse_level1(self, x):
        """fastflow.py:57-76: one solve per group."""
        chunks = torch.chunk(x, 4, dim=1)
        outs = [m.reverse(c.contiguous())[0] for m, c in
                zip((self.conv_tl, self.conv_tr, self.conv_bl, self.conv_br), chunks)]
        return torch.cat(outs, dim=1)


class CINCFlowUnit(nn.Module):
    """The groups=1 (CInC) unit of cinc_flow.py:9-80: ONE top-left PaddedConv2d over all channels
    (`out_channels` is overridden with `in_channels`, cinc_flow.py:17), state-dict key `conv_tl.conv.weight`.  `reverse` is
    PaddedConv2d's: detached, differentiable inside `fincflow_amd.reverse_grad()`."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        if isinstance(kernel_size, int) or len(kernel_size) == 1:
            kernel_size = (kernel_size, kernel_size) if isinstance(kernel_size, int) else (kernel_size[0],) * 2
        out_channels = in_channels
        self.conv_tl = PaddedConv2d(out_channels, out_channels, kernel_size, order='TL')

    def forward(self, x, context=None):
        out, logdet = self.conv_tl.forward(x)
        return out, 0.0 + logdet

    def reverse(self, x, context=None):
        return self.reverse_level1(x)

    def reverse_with_logdet(self, x, context=None):
        out = self.reverse(x, context)
        return out, out.new_zeros(len(out))

    def reverse_level1(self, x):
        return self.conv_tl.reverse(x)[0]

    def invertible_backward_supported(self, x, context=None):
        return self.conv_tl.invertible_backward_supported(x, context)

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        return self.conv_tl.backward_from_output(output, grad_output, grad_logdet, context, needs)


def load_reference_checkpoint(model, checkpoint, strict=True, validate=True, trust_pickle=False):
    """Load a reference training checkpoint (train/experiment.py:400-427: a dict holding 'model_state_dict',
    written by `torch.save`) or a bare state-dict into `model`.

    The reference stores every PaddedConv2d weight flipped per its `order` (layers/conv.py:72-79) under
    `<prefix>.conv_{tl,tr,bl,br}.conv.weight`; the modules here keep the same storage and the same keys, so
    this is `load_state_dict` plus what a checkpoint written by `nn.DataParallel` needs (the 'module.' prefix,
    fastflow_cifar_multi_gpu.py wraps the model) and what trained weights need: every packed-fragment cache is
    dropped and, with `validate`, each layer's unit-triangular corner tap is checked once on the device
    (a violated invariant raises RuntimeError instead of silently solving a different system).
    A path is read with `torch.load(weights_only=True)` (tensors and plain containers only).  The reference's files
    also pickle its config dict; if that holds arbitrary objects the safe load fails, and the caller opts in to full
    unpickling -- which executes code from the file -- with `trust_pickle=True`.
    Returns the (missing_keys, unexpected_keys) of `load_state_dict`.
    """
    if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, "__fspath__"):
        try:
            checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=True)
        except Exception as e:
            if not trust_pickle:
                raise RuntimeError(f"checkpoint {checkpoint!r} needs full unpickling ({type(e).__name__}); pass "
                                   "trust_pickle=True only for files you trust") from e
            checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=False)
    state = checkpoint.get("model_state_dict", checkpoint) if isinstance(checkpoint, dict) else checkpoint
    if state and all(k.startswith("module.") for k in state):
        state = {k[len("module."):]: v for k, v in state.items()}
    # a PaddedConv2d built with bias=True owns a `bias` the reference never wrote (its conv is bias-free, layers/conv.py:60):
    # that key may be missing from a reference checkpoint -- the zero initialisation stands -- everything else is strict
    own_bias = {name + ".bias" for name, m in model.named_modules() if isinstance(m, PaddedConv2d) and m.bias is not None}
    own_bias |= {"bias"} if isinstance(model, PaddedConv2d) and model.bias is not None else set()
    result = model.load_state_dict(state, strict=False)
    missing = [k for k in result.missing_keys if k not in own_bias]
    if strict and (missing or result.unexpected_keys):
        raise RuntimeError(f"checkpoint does not match the model: missing {missing}, unexpected {list(result.unexpected_keys)}")
    if any(p.is_cuda for p in model.parameters()):
        _lib.raise_if_faulted("load_reference_checkpoint")   # (the invariant check below synchronises: a natural reporting point)
    for m in model.modules():
        cache = getattr(m, "_cache", None)
        if isinstance(cache, ops.PackedWeights):
            cache.invalidate()
        if validate and isinstance(m, PaddedConv2d):
            w = m.conv.weight.detach()
            if w.is_cuda:
                ops.check_invariant(ops.canonicalize(w.contiguous(), 1, m._orient), 1)
            else:  # host-side check of the same rule, for a model validated before .cuda()
                corner = m._flip(w)[:, :, -1, -1]
                if not torch.equal(torch.triu(corner), torch.eye(corner.shape[0], dtype=corner.dtype)):
                    raise RuntimeError("checkpoint violates the unit-triangular corner tap (layers/conv.py:63-70)")
    return result


class StandardNormal(nn.Module):
    """Base density with the runner's interface (train/losses.py:17-45): log_prob(z) -> [B], sample(n)."""

    def __init__(self, size):
        super().__init__()
        self.size = tuple(size)
        self.register_buffer("_anchor", torch.zeros(1), persistent=False)  # not in reference checkpoints

    def log_prob(self, z, context=None):
        return -0.5 * (z ** 2 + torch.log(torch.tensor(2 * torch.pi, device=z.device))).flatten(1).sum(1)

    def sample(self, n_samples, context=None):
        return torch.randn(n_samples, *self.size, device=self._anchor.device, dtype=self._anchor.dtype), None


def _image_boundary_layers(mods):
    """The image boundary at the head of `mods` (forward order): `(normalisations, length, squeeze)` for exactly [Dequantization, one
    or more Normalization with buffers (not learnable), LogitTransform, (Squeeze)] -- `length` counts the Squeeze when `squeeze` -- or
    None for anything else: a learnable Normalization, a subclass, a layer in between."""
    from . import glow
    if len(mods) < 3 or type(mods[0]) is not glow.Dequantization:
        return None
    j = 1
    while (j < len(mods) and type(mods[j]) is glow.Normalization
           and not any(isinstance(p, nn.Parameter) for p in (mods[j].scale, mods[j].translation))):
        j += 1
    if j == 1 or j >= len(mods) or type(mods[j]) is not glow.LogitTransform:
        return None
    squeeze = j + 1 < len(mods) and type(mods[j + 1]) is glow.Squeeze
    return list(mods[1:j]), j + 1 + int(squeeze), squeeze


class _InvertibleRunFunction(torch.autograd.Function):
    """A run of layers that support `backward_from_output`, as one autograd node (FlowSequential.invertible_backward).
    Inputs: the activation, the context, every parameter of the run.  Outputs: the run's output and its summed log-det [B].
    Forward: the no-grad pass of `FlowSequential.forward` over the run, folds included.  Saved: the run's OUTPUT and the context --
    nothing per layer.  Backward: the layers last to first, each rebuilding its input from its output and differentiating there; a
    rebuilt activation lives until the layer in front has consumed it.  The saved output is never written, so the backward can run
    again under `retain_graph=True`.
    Autocast: a backward runs outside the forward's autocast context, and a coupling's rebuilt input is only right if its net gives
    `raw` the forward's bits.  So the autocast state of the forward (enabled, dtype) is kept and entered again around the backward, as
    torch.utils.checkpoint does; and under autocast the forward runs its nets on the recording path (`ops.recorded_net`), the one the
    backward differentiates.  Both passes run with autocast's weight cache off: a weight cast under no_grad (this forward) and cached
    would be handed, without a graph, to the next recorded use inside the same autocast context -- the backward's, when it is called
    there.  Outside autocast none of this changes a launch."""

    @staticmethod
    def forward(ctx, seq, run, x, context, *params):
        kind = x.device.type
        ctx.autocast = (kind, torch.is_autocast_enabled(kind), torch.get_autocast_dtype(kind))
        if ctx.autocast[1]:
            with ops.recorded_net(), torch.autocast(kind, dtype=ctx.autocast[2], cache_enabled=False):
                out, logdet = seq._forward_layers(list(run), x, context, x.new_zeros(len(x)))
        else:
            out, logdet = seq._forward_layers(list(run), x, context, x.new_zeros(len(x)))
        ctx.run = run
        ctx.counts = [len(list(m.parameters())) for m in run]
        ctx.save_for_backward(out, context)
        return out, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, grad_logdet):
        out, context = ctx.saved_tensors
        need_x, need_ctx, need_p = ctx.needs_input_grad[2], ctx.needs_input_grad[3], ctx.needs_input_grad[4:]
        grad, gld = ops._incoming_grads(out, grad_out, grad_logdet)
        starts = [sum(ctx.counts[:k]) for k in range(len(ctx.run))]
        pgrads, gctx, y = [None] * len(need_p), None, out
        kind, enabled, dtype = ctx.autocast
        for k in reversed(range(len(ctx.run))):
            upstream = need_x or need_ctx or any(need_p[:starts[k]])     # does anything in front of this layer want a gradient?
            needs = BackwardNeeds(input=k > 0 and upstream, grad_input=upstream, grad_context=need_ctx,
                                  params=tuple(need_p[starts[k]:starts[k] + ctx.counts[k]]))
            with torch.autocast(kind, dtype=dtype, enabled=enabled, cache_enabled=False):
                y, grad, gc, pg = ctx.run[k].backward_from_output(y, grad, gld, context, needs)
            pgrads[starts[k]:starts[k] + ctx.counts[k]] = pg
            if gc is not None:
                gctx = gc if gctx is None else gctx + gc
            if not upstream:
                break
        if out.is_cuda:
            _lib.raise_if_faulted("FlowSequential.invertible_backward")
        return (None, None, grad if need_x else None, gctx) + tuple(pgrads)


class FlowSequential(nn.Module):
    """Protocol-compatible stand-in for layers/flowsequential.py:9-115 (the reference file cannot travel to
    the GPU box and hard-imports wandb + a cuDNN-only extension).  Only what the hot path's callers use."""

    def __init__(self, base_distribution, *modules):
        super().__init__()
        self.base_distribution = base_distribution
        for i, module in enumerate(modules):
            self.add_module(str(i), module)
        self.sequence_modules = modules

    def __iter__(self):
        yield from self.sequence_modules

    def forward(self, input, context=None, compute_expensive=False):
        output, logdet = self._forward_stack(input, context)
        logprob = self.base_distribution.log_prob(output)
        return output, logprob + logdet

    def _forward_stack(self, input, context, latents=None):
        mods = list(self.sequence_modules)
        if self.invertible_backward and torch.is_grad_enabled():
            return self._forward_invertible(mods, input, context, latents)
        return self._forward_layers(mods, input, context, latents=latents)

    def encode(self, input, context=None):
        """The complete latent code of `input` and its log-density: `(zs, log_prob)`.  `zs` is a list -- the half that every layer
        with a `split` (glow.SplitPrior) factors out, in forward order, then the stack's output -- and log_prob [B] is what
        `forward(input, context)[1]` is.  `forward` throws those halves away; with them `decode(zs)` is the exact inverse
        (`reconstruct` is not, in a stack with split layers).  The walk is `forward`'s, `fuse_affine` folds and `invertible_backward`
        runs included, and it is differentiable: a loss on log_prob reaches every parameter, through a split layer's own HIP
        backward on the device."""
        zs = []
        output, logdet = self._forward_stack(input, context, zs)
        zs.append(output)
        return zs, self.base_distribution.log_prob(output) + logdet

    def _forward_layers(self, mods, input, context, logdet=0, latents=None):
        """`mods` in order on `input`: (output, `logdet` plus the sum of their log-dets).  `latents`: a list that receives what
        every layer with a `split` factors out (`encode`); None: the layers' `forward`."""
        i = 0
        head = self._encode_image(mods, input) if self.fuse_image_boundary else None
        if head is not None:
            i, input, head_logdet = head
            logdet = logdet + head_logdet
        while i < len(mods):
            module = mods[i]
            # density evaluation: a FastFlowUnit followed by an (initialised) per-channel affine layer is one launch
            if (self.fuse_affine and i + 1 < len(mods) and isinstance(module, FastFlowUnit)
                    and hasattr(mods[i + 1], "forward_affine_params") and not torch.is_grad_enabled()):
                params = mods[i + 1].forward_affine_params()
                fused = module.forward_affine(input, *params) if params is not None else None
                if fused is not None:
                    logdet = logdet + mods[i + 1].logdet(input, context)      # (the unit's own logdet is 0)
                    input = output = fused
                    i += 2
                    continue
            if latents is not None and hasattr(module, "split"):
                output, latent, layer_logdet = module.split(input, context)
                latents.append(latent)
            else:
                output, layer_logdet = module(input, context)
            logdet = logdet + layer_logdet        # (not in place: a Conv1x1 in front hands on a 0-dim log-det, the next layer's is [B])
            input = output
            i += 1
        return input, logdet

    #: train without stored activations: while `forward` records an autograd graph, every maximal run of two or more
    #: layers that can differentiate from their output (`invertible_backward_supported`) is ONE autograd node that keeps the run's
    #: output and nothing else; its backward walks the run from the back, each layer rebuilding its input (`backward_from_output`).
    #: Off by default; set per instance.  Costs an inverse per layer and step.
    invertible_backward = False

    def _invertible_run_end(self, mods, i, input, context):
        """The end j of the maximal run mods[i:j] of layers that support `backward_from_output` for this call.  The layers judge a
        tensor's shape, dtype and device only, so the activations between them need not exist yet: a layer that changes the shape
        (`invertible_output_shape`) hands on a stand-in of one element expanded to the new shape."""
        probe, j = input, i
        while j < len(mods):
            supported = getattr(mods[j], "invertible_backward_supported", None)
            if supported is None or not supported(probe, context):
                break
            shape = getattr(mods[j], "invertible_output_shape", None)
            if shape is not None:
                probe = probe.new_empty((1,)).expand(shape(tuple(probe.shape)))
            j += 1
        return j

    def _forward_invertible(self, mods, input, context, latents=None):
        """`_forward_layers` with every run of two or more supporting layers that has something to differentiate behind one
        `_InvertibleRunFunction`; every other layer runs as it always has, with its stored activations.  (A layer with a `split`
        supports no invertible backward: it ends a run and is walked here.)"""
        logdet = 0
        i = 0
        head = self._encode_image(mods, input) if self.fuse_image_boundary else None
        if head is not None:          # (a Squeeze the encode took is not part of the invertible run behind it)
            i, input, logdet = head
        while i < len(mods):
            j = self._invertible_run_end(mods, i, input, context)
            if j - i >= 2:
                run = tuple(mods[i:j])
                params = [p for m in run for p in m.parameters()]
                if (input.requires_grad or (context is not None and context.requires_grad) or any(p.requires_grad for p in params)):
                    input, run_logdet = _InvertibleRunFunction.apply(self, run, input, context, *params)
                    logdet = logdet + run_logdet
                    i = j
                    continue
            if latents is not None and hasattr(mods[i], "split"):
                output, latent, layer_logdet = mods[i].split(input, context)
                latents.append(latent)
            else:
                output, layer_logdet = mods[i](input, context)
            logdet = logdet + layer_logdet
            input = output
            i += 1
        return input, logdet

    def log_prob(self, input, context=None, compute_expensive=True):
        return self.forward(input, context, compute_expensive)[1]

    #: fold a per-channel affine layer (a module exposing `reverse_affine_params()`, e.g. glow.ActNorm) into the
    #: FastFlowUnit that follows it in the reverse chain: one launch instead of two, same result
    fuse_affine = True
    #: let the channel mix in front of a FastFlowUnit (reverse chain) apply the unit's blockdiag(Linv) as well
    fuse_lead = True
    #: the image boundary on its HIP kernels: the prefix [Dequantization, Normalization(s), LogitTransform, (Squeeze)]
    #: of `forward` / `encode` is ONE launch (`ops.finc_image_encode`) and so is the tail of the reverse chain
    #: (`ops.finc_image_decode`), for uint8 or fp32 device images.  Off by default, set per instance: the fused encode computes 1 - y
    #: from the integer pixel and is right at saturated pixels where the layers' lines are not, so its bits are not theirs.
    fuse_image_boundary = False

    def image_boundary_constants(self):
        """What the image boundary's kernels take, composed in float64 from the Normalization buffers' values, or None -- a stack
        without the boundary layers, or a first use inside a stream capture (reading the buffers is a device -> host copy).  With y =
        (..((v - t1) / s1 - t2) / s2..): `mult` = 1 / prod s, `lo` = y at v = 0, `hi` = s1 (the number of grey levels), `hi_comp` = 1 -
        lo - mult * hi (so that 1 - y = mult * (hi - v) + hi_comp), `inv_mult` and `off` of the reverse v = inv_mult * y + off, and
        `sum_log_scale` = sum log s (the per-image log-det constant is -D times it).  Cached per `ops.version_key` of the buffers."""
        found = _image_boundary_layers(list(self.sequence_modules))
        if found is None:
            return None
        bufs = [b for n in found[0] for b in (n.translation, n.scale)]
        key = ops.version_key(*bufs)
        if getattr(self, "_image_key", None) != key:
            if bufs[0].is_cuda and ops._capturing():
                return None
            with torch.no_grad():
                vals = torch.cat([b.detach().double().reshape(1) for b in bufs]).tolist()
            mult, lo, inv_mult, off, sum_log = 1.0, 0.0, 1.0, 0.0, 0.0
            for t, s in zip(vals[0::2], vals[1::2]):
                mult, lo, sum_log = mult / s, (lo - t) / s, sum_log + math.log(s)
            for t, s in reversed(list(zip(vals[0::2], vals[1::2]))):
                inv_mult, off = inv_mult * s, off * s + t
            hi = vals[1]
            self._image_consts = dict(mult=mult, lo=lo, hi=hi, hi_comp=1.0 - lo - mult * hi, inv_mult=inv_mult, off=off,
                                      sum_log_scale=sum_log)
            self._image_key = key
        return self._image_consts

    def _encode_image(self, mods, input):
        """The image boundary at the head of `mods` as one launch on `input`: `(layers consumed, output, logdet[B])`, or None where
        the layers run as they always have -- no boundary at the head, a tensor that is not a 4-D uint8 / fp32 device tensor, an input
        that requires grad (the encode has no backward), odd sides in front of a Squeeze (left to the layer), constants not yet
        cached inside a stream capture.  The noise is the layer's draw: `torch.rand` of the image's shape, fp32, on its device."""
        found = _image_boundary_layers(mods)
        if (found is None or not input.is_cuda or input.dim() != 4 or input.dtype not in (torch.uint8, torch.float32)
                or input.requires_grad or input.numel() == 0):
            return None
        k = self.image_boundary_constants() if mods[0] is self.sequence_modules[0] else None
        if k is None:
            return None
        _, n, squeeze = found
        if squeeze and (input.shape[2] % 2 or input.shape[3] % 2):
            n, squeeze = n - 1, False
        noise = torch.rand(input.shape, dtype=torch.float32, device=input.device)
        out, logdet = ops.finc_image_encode(input.contiguous(), noise, mult=k["mult"], lo=k["lo"], hi=k["hi"], hi_comp=k["hi_comp"],
                                            logdet_const=-input[0].numel() * k["sum_log_scale"], squeeze=squeeze)
        return n, out, logdet

    def _decode_image(self, input, squeeze, with_logdet, dtype):
        """The tail of the reverse chain on `input`, the activation in front of the boundary's reverse: x, or `(x, logdet[B])`."""
        k = self.image_boundary_constants()
        ldc = -input[0].numel() * k["sum_log_scale"] if with_logdet else None
        return ops.finc_image_decode(input.contiguous(), inv_mult=k["inv_mult"], off=k["off"], hi=k["hi"], logdet_const=ldc,
                                     unsqueeze=squeeze, dtype=dtype)

    def _image_tail(self, input, squeeze):
        """Does one decode launch serve `input` at the boundary's end of the reverse chain?  An fp32 4-D device tensor that records
        no graph, four channels per image channel in front of a Squeeze, the constants at hand."""
        if not _hip_tensor(input) or _records_graph(input) or input.numel() == 0 or (squeeze and input.shape[1] % 4):
            return False
        return self.image_boundary_constants() is not None

    def _reverse_chain(self, input, context, fuse=None, with_logdet=False, latents=None, image_dtype=torch.float32):
        """The layers' reverses, last layer first.  `with_logdet`: returns `(x, logdet[B])`, the sum of the layers' FORWARD log-dets
        at their recovered inputs (`reverse_with_logdet`), in the same pass: every fold below stays, and a folded per-channel affine
        layer or channel mix adds its term -- parameters only, a few [C]-sized ops or a cached number -- beside the fused launch (the
        unit's own is zero).  `latents`: the factored-out halves of the layers with a `merge`, in FORWARD order (`decode`): each such
        layer takes its own through `merge` instead of drawing one in `reverse`, and its log p takes the log-det's place.
        With `fuse_image_boundary` the image boundary's reverse at the end of the chain is one launch (`_decode_image`) that writes
        `image_dtype` (fp32: the layers' floor; uint8: clamped, `sample_uint8`); `fuse=False`, the layer-by-layer check of `sample`,
        keeps the layers there too."""
        layer_by_layer = fuse is False
        fuse = self.fuse_affine if fuse is None else fuse
        mods = list(reversed(self.sequence_modules))
        latents = None if latents is None else list(latents)
        logdet = input.new_zeros(len(input)) if with_logdet else None
        boundary = _image_boundary_layers(list(self.sequence_modules)) if self.fuse_image_boundary and not layer_by_layer else None
        tail = len(mods) - boundary[1] if boundary is not None else -1       # where the image boundary's reverse begins
        i = 0
        while i < len(mods):
            m = mods[i]
            if i == tail and self._image_tail(input, boundary[2]):
                out = self._decode_image(input, boundary[2], with_logdet, image_dtype)
                if with_logdet:
                    input, logdet = out[0], logdet + out[1]
                else:
                    input = out
                break
            if (fuse and i + 1 < len(mods) and hasattr(m, "reverse_affine_params")
                    and isinstance(mods[i + 1], FastFlowUnit) and not torch.is_grad_enabled()):
                fused = mods[i + 1].reverse_affine(input, *m.reverse_affine_params())
                if fused is not None:
                    if with_logdet:
                        logdet = logdet + m.logdet(input, context)
                    input = fused
                    i += 2
                    continue
            # channel mix -> [per-channel affine] -> unit: the mix also applies the unit's blockdiag(Linv), the unit's inverse
            # runs without its z-term (full-chip problem sets only; otherwise the folds below)
            if fuse and self.fuse_lead and hasattr(m, "reverse_premultiplied") and not torch.is_grad_enabled():
                j, affine = i + 1, None
                if j < len(mods) and hasattr(mods[j], "reverse_affine_params"):
                    affine = mods[j].reverse_affine_params()
                    j += 1
                if j < len(mods) and isinstance(mods[j], FastFlowUnit) and (j == i + 1 or affine is not None):
                    fused = mods[j].reverse_after_mix(input, m, affine)
                    if fused is not None:
                        if with_logdet:
                            logdet = logdet + m.mix_logdet(input)
                            if affine is not None:
                                logdet = logdet + mods[i + 1].logdet(input, context)
                        input = fused
                        i = j + 1
                        continue
            # a channel mix followed by a per-channel affine layer that no FastFlowUnit takes: one mixing launch
            if (fuse and i + 1 < len(mods) and hasattr(m, "reverse_then_affine") and hasattr(mods[i + 1], "reverse_affine_params")
                    and not (i + 2 < len(mods) and isinstance(mods[i + 2], FastFlowUnit)) and not torch.is_grad_enabled()):
                fused = m.reverse_then_affine(input, *mods[i + 1].reverse_affine_params())
                if fused is not None:
                    if with_logdet:
                        logdet = logdet + m.mix_logdet(input) + mods[i + 1].logdet(input, context)
                    input = fused
                    i += 2
                    continue
            if latents is not None and hasattr(m, "merge"):
                latent = latents.pop()
                if latent.shape != input.shape:
                    raise ValueError(f"the latent of a split layer has shape {tuple(latent.shape)}, its layer expects {tuple(input.shape)}")
                if with_logdet:
                    input, layer_logdet = m.merge(input, latent, context, with_log_prob=True)
                    logdet = logdet + layer_logdet
                else:
                    input = m.merge(input, latent, context)
            elif with_logdet:
                input, layer_logdet = m.reverse_with_logdet(input, context)
                logdet = logdet + layer_logdet
            else:
                output = m.reverse(input, context)
                input = output[0] if isinstance(output, tuple) else output
            i += 1
        return (input, logdet) if with_logdet else input

    def _split_layers(self):
        return [m for m in self.sequence_modules if hasattr(m, "split")]

    def decode(self, zs, context=None, with_log_prob=False):
        """The inverse of `encode`: x from the complete latent code `zs` (the split layers' halves in forward order, then the stack's
        output), through `_reverse_chain` with every fold kept and every split layer's `merge`.  With `with_log_prob`: `(x, log_q)`,
        log_q [B] = base.log_prob(zs[-1]) + the layers' forward log-dets at their recovered inputs, the merges' log p among them --
        `log_prob(x)` from the same pass, as `sample_with_log_prob` builds it.  ValueError for a list of the wrong length or a
        latent of the wrong shape.  Nothing is drawn here, so the call can be captured in a graph; the grad mode is the caller's
        (under `torch.no_grad()` the HIP paths of `sample`); the fault word is checked as in `sample`."""
        zs = list(zs)
        if len(zs) != len(self._split_layers()) + 1:
            raise ValueError(f"expected {len(self._split_layers()) + 1} latents (one per split layer, then the stack's output), "
                             f"got {len(zs)}")
        z, size = zs[-1], getattr(self.base_distribution, "size", None)
        if size is not None and tuple(z.shape[1:]) != tuple(size):
            raise ValueError(f"the last latent has shape {tuple(z.shape)}, the base distribution expects [B, {', '.join(map(str, size))}]")
        if any(len(t) != len(z) for t in zs):
            raise ValueError("the latents hold different numbers of images")
        if with_log_prob:
            x, logdet = self._reverse_chain(z, context, with_logdet=True, latents=zs[:-1])
            out = (x, self.base_distribution.log_prob(z) + logdet)
        else:
            out = x = self._reverse_chain(z, context, latents=zs[:-1])
        if x.is_cuda:
            _lib.raise_if_faulted("FlowSequential.decode")
        return out

    def draw_latents(self, n_samples, context=None, temperature=1.0):
        """A complete latent code drawn from the model's priors, each draw times `temperature` (applied to what a prior's `sample`
        returns): the list `decode` takes.  The draws are made in the order `sample` makes them -- the base first, then the split
        layers from the last to the first -- so from one seed `decode(draw_latents(n))` is `sample(n)[0]`."""
        z = self.base_distribution.sample(n_samples, context)[0]
        zs = [z if temperature == 1 else z * temperature]
        for m in reversed(self._split_layers()):
            zs.append(m.draw(n_samples, context, temperature))
        return zs[::-1]

    def sample(self, n_samples, context=None, compute_expensive=False, also_true_inverse=False, temperature=1.0):
        """layers/flowsequential.py:89-115: returns `(input, input_true)` -- the runner unpacks two values
        (train/experiment.py:311-335).  No layer of the hot path is a ModifiedGradFlowLayer, so the "true inverse"
        differs from the regular sample only in how it is evaluated: it re-runs the reverse chain from the same z
        layer by layer (no affine fold), an independent check of the fused launch.  Without `also_true_inverse` (or with
        `compute_expensive`) the second value IS the first, as in the reference (`input_true = input`).
        `temperature`: every prior's draw times that number (Glow samples at about 0.7).  At 1.0 the path is the one it always was;
        otherwise it is `decode(draw_latents(n_samples, context, temperature), context)`, and the second value follows the same
        rule: with `also_true_inverse` (and without `compute_expensive`) the same latents once more through the reverse chain without
        its folds, else the first value itself."""
        if temperature != 1.0:
            zs = self.draw_latents(n_samples, context, temperature)
            x = self.decode(zs, context)
            if not compute_expensive and also_true_inverse:
                return x, self._reverse_chain(zs[-1], context, fuse=False, latents=zs[:-1])
            return x, x
        z, _ = self.base_distribution.sample(n_samples, context)
        x = self._reverse_chain(z, context)
        if not compute_expensive and also_true_inverse:
            x_true = self._reverse_chain(z, context, fuse=False)
        else:
            x_true = x
        # A helper-wave launch whose protocol wait gave up has returned FINC_OK (launches are asynchronous); every later
        # launching call on the device refuses, but a chain that ENDS on such a launch would hand its garbage out.  The fault
        # word lives in host memory: reading it here costs nothing and catches every launch that has finished by now (the
        # caller's own synchronisation + the next call catch the rest).
        if x.is_cuda:
            _lib.raise_if_faulted("FlowSequential.sample")
        return x, x_true

    def rsample(self, n_samples, context=None, temperature=1.0):
        """A reparameterised sample: x = reverse(z), z drawn from the base, with the reverse chain RECORDED for autograd (grad enabled,
        inside `reverse_grad()`: the fused folds step aside, the units' inverses are differentiable), so that a loss on x reaches
        every parameter -- reverse-KL training, adversarial fine-tuning of the sampler.  Returns x alone, attached to the graph; the
        fault word is checked as in `sample`.  `temperature` as in `sample`: at 1.0 today's path, otherwise `decode` of tempered
        `draw_latents`, recorded the same way."""
        if temperature != 1.0:
            zs = self.draw_latents(n_samples, context, temperature)
            with torch.enable_grad(), ops.reverse_grad():
                return self.decode(zs, context)
        z, _ = self.base_distribution.sample(n_samples, context)
        with torch.enable_grad(), ops.reverse_grad():
            x = self._reverse_chain(z, context)
        if x.is_cuda:
            _lib.raise_if_faulted("FlowSequential.rsample")
        return x

    def sample_with_log_prob(self, n_samples, context=None):
        """A sample and its log-density under the model, from ONE reverse pass: `(x, log_q)` with x = reverse(z), z drawn from the
        base, and log_q[B] = base.log_prob(z) + the layers' forward log-dets at their recovered inputs -- what `log_prob(x)` would
        compute with a second, forward pass over the stack.  Runs under `torch.no_grad()` (the pass of `sample` under no_grad, folds
        included: the same x from the same seed); nothing is recorded.  The fault word is checked as in `sample`.  With a
        Dequantization layer in the stack, log_q is the density of the CONTINUOUS variable in front of its floor."""
        with torch.no_grad():
            z, _ = self.base_distribution.sample(n_samples, context)
            x, logdet = self._reverse_chain(z, context, with_logdet=True)
            log_q = self.base_distribution.log_prob(z) + logdet
        if x.is_cuda:
            _lib.raise_if_faulted("FlowSequential.sample_with_log_prob")
        return x, log_q

    def rsample_with_log_prob(self, n_samples, context=None):
        """`rsample` with the sample's log-density: `(x, log_q)`, both attached to every parameter (the reverse chain is recorded
        inside `reverse_grad()`, the coupling's log-det comes out of its reverse launch and has a backward of its own), so that
        reverse-KL training -- E_q[log q(x) - log p*(x)] -- needs no second pass through `log_prob`."""
        z, _ = self.base_distribution.sample(n_samples, context)
        with torch.enable_grad(), ops.reverse_grad():
            x, logdet = self._reverse_chain(z, context, with_logdet=True)
            log_q = self.base_distribution.log_prob(z) + logdet
        if x.is_cuda:
            _lib.raise_if_faulted("FlowSequential.rsample_with_log_prob")
        return x, log_q

    def reconstruct(self, input, context=None, compute_expensive=False):
        """`forward` then the reverse chain on its output.  In a stack with split layers (glow.SplitPrior) this is NOT the input
        again: `forward` drops the halves those layers factor out and the reverse chain draws fresh ones.  The exact round trip
        there is `decode(encode(input)[0])`."""
        z = self.forward(input, context)[0]
        return self._reverse_chain(z, context)

    def sample_uint8(self, n_samples, context=None, temperature=1.0):
        """`n_samples` images as uint8 [n, C, H, W]: `sample(n_samples, context, temperature=temperature)[0]` clamped to the grey
        levels [0, hi - 1] (hi: the first Normalization's scale, 256) and cast -- from one seed the same draws.  Needs the image
        boundary layers at the head of the stack (ValueError without them).  With `fuse_image_boundary` the decode launch writes the
        bytes itself; otherwise the layers' fp32 result is clamped and cast.  Runs under `torch.no_grad()`."""
        if _image_boundary_layers(list(self.sequence_modules)) is None:
            raise ValueError("sample_uint8 needs the image boundary at the head of the stack: Dequantization, Normalization layers "
                             "with fixed buffers, LogitTransform (create_model(preprocess=True))")
        with torch.no_grad():
            zs = self.draw_latents(n_samples, context, temperature)
            x = self._reverse_chain(zs[-1], context, latents=zs[:-1], image_dtype=torch.uint8)
            if x.dtype != torch.uint8:
                k = self.image_boundary_constants()
                if k is None:
                    raise RuntimeError("sample_uint8 reads the Normalization buffers on its first call: call it once outside the capture")
                x = x.clamp(0, k["hi"] - 1).to(torch.uint8)
        if x.is_cuda:
            _lib.raise_if_faulted("FlowSequential.sample_uint8")
        return x

    def bits_per_dim(self, input, context=None):
        """-log_prob(input) / (D ln 2) per image, [B]: D the number of values of one image."""
        return -self.log_prob(input, context) / (input[0].numel() * math.log(2.0))
