"""The layers either side of the hot path in the reference's CIFAR Glow stack (BASELINE
configs[3]): thin PyTorch modules with the reference's constructor arguments, parameter names and
forward -> (out, logdet[B]) / reverse -> out protocol, so that `create_model` below builds the topology of
fastflow/fastflow_cifar.py:35-63 around fincflow_amd.FastFlowUnit.  ActNorm, Conv1x1 and the coupling's transform run on HIP
kernels of their own (ops.finc_actnorm, ops.finc_mix, ops.finc_coupling), in inference and under autograd -- `forward` always,
`reverse` inside `ops.reverse_grad()` (what `FlowSequential.rsample` records: ops.actnorm_reverse, ops.mix_forward on W^-1,
ops.coupling_reverse); `reverse` under autograd outside that context keeps its PyTorch lines.  `reverse_with_logdet` is `reverse`
plus the forward log-det at its result from the same pass (ops.finc_coupling_reverse_logdet, ops.coupling_reverse_logdet; parameters
only for ActNorm and Conv1x1): what `FlowSequential.sample_with_log_prob` / `rsample_with_log_prob` add up.  `backward_from_output`
differentiates a layer from its OUTPUT and rebuilds its input in the same pass (ops.finc_actnorm_backward_reconstruct,
ops.finc_coupling_backward_reconstruct, the mix on W^-1): the steps of `FlowSequential.invertible_backward`.  The coupling net's
convolutions, Squeeze and the preprocessing layers are ops that PyTorch-ROCm already runs.  The point of this file is that a
whole sampling pass (96 units at 16x16 / 8x8 / 4x4) can run and be captured in one HIP graph.

Reference semantics followed:
  Squeeze        layers/squeeze.py:5-41          space-to-depth, channel order (c, dy, dx)
  ActNorm        layers/actnorm.py:5-66          data-dependent init on first forward; out = (x - t) * exp(-log_scale);
                 on the device one HIP launch each way (ops.finc_actnorm), init and backward included (ops.finc_actnorm_init,
                 ops.actnorm_forward, ops.actnorm_reverse)
  Conv1x1        layers/conv1x1.py:8-49          orthogonal init, ldj = H*W*log|det W|
  Coupling       layers/coupling.py:46-113       affine, net = conv3x3-ReLU-conv1x1-ReLU-Conv2dZero, log_s = 2*tanh(h/2);
                 on the device the part behind the net is one HIP launch (ops.finc_coupling)
  SplitPrior     layers/splitprior.py:7-41       Coupling + factor out the second half under a standard normal; `split` / `merge`
                 hand that half out and take it back (FlowSequential.encode / decode), one HIP launch each (ops.finc_split_prior,
                 ops.finc_split_prior_merge, ops.split_prior_forward); with `hip_recorded_merge` a `merge` recorded inside
                 ops.reverse_grad() too (ops.split_prior_merge)
  Split          layers/split.py:4-52            the Gaussianized split (`Gaussianize`): the second half modelled as N(m, exp(logs)^2) with
                 (m, logs) from ONE zero-initialised 3x3 convolution of the first; the `split` / `merge` / `draw` protocol of SplitPrior,
                 one HIP launch each behind that convolution (ops.finc_gauss_split, ops.finc_gauss_split_merge,
                 ops.gauss_split_forward; with `hip_recorded_merge` ops.gauss_split_merge for a recorded `merge`)
  Normalization, LogitTransform, Dequantization  layers/normalize.py, transforms.py:6-19, dequantize.py
                 (Dequantization owns the reference's UniformDistribution, layers/distributions/uniform.py, whose buffer `empty`
                 every reference checkpoint holds as `0.distribution.empty`)
                 with `FlowSequential.fuse_image_boundary` these and the first Squeeze are one HIP launch each way
                 (ops.finc_image_encode, ops.finc_image_decode: uint8 or fp32 images in, fp32 or uint8 images out)
  GaussianPrior  train/losses.py:17-45           standard-normal base (log_prob per sample, sample(n))
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers import FastFlowUnit, FlowLayer, FlowSequential, _hip_tensor, _param_needs, _params_on_device, _records_graph


def _fp32_maps(x):
    """The context in which a flow layer's own map runs its PyTorch lines: autocast off for the device of `x`.  The flow's maps stay
    fp32 under autocast (invertibility and the log-det need it; only the coupling NET runs in the autocast dtype), and a convolution
    left to autocast would hand bf16 to the next layer.  Outside autocast this changes nothing."""
    return torch.autocast(x.device.type, enabled=False)


def _autocast_dtype(x):
    """The autocast dtype that is active for the device of `x`, or None."""
    kind = x.device.type
    return torch.get_autocast_dtype(kind) if torch.is_autocast_enabled(kind) else None


class _DerivedValues:
    """A layer that keeps values derived from its parameters per parameter version (`ops.version_key`), each with its `ops.Ready`
    token: the stream it was built on and the event behind its fill, asked in front of every use.  A copy of the layer
    (copy.deepcopy for an EMA model, pickle, torch.save of the module) starts without any of them, as a copy of `ops.PackedWeights`
    does: its first call rebuilds them from ITS parameters, and an event belongs to the process and stream that recorded it."""
    _derived = ()

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in self._derived}


class Squeeze(FlowLayer):
    def forward(self, input, context=None):
        b, c, h, w = input.shape
        x = input.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 2, 4)
        return x.reshape(b, c * 4, h // 2, w // 2), self.logdet(input, context)

    def reverse(self, input, context=None):
        b, c, h, w = input.shape
        x = input.reshape(b, c // 4, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3)
        return x.reshape(b, c // 4, h * 2, w * 2)

    def reverse_with_logdet(self, input, context=None):
        return self.reverse(input, context), input.new_zeros(len(input))

    def invertible_backward_supported(self, input, context=None):
        return _hip_tensor(input) and input.shape[2] % 2 == 0 and input.shape[3] % 2 == 0

    def invertible_output_shape(self, shape):
        b, c, h, w = shape
        return b, c * 4, h // 2, w // 2

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """The permutation's inverse applied to the output and to its gradient."""
        x = self.reverse(output) if needs.input else None
        return x, (self.reverse(grad_output) if needs.grad_input else None), None, []

    def logdet(self, input, context=None):
        return input.new_zeros(len(input))


class ActNorm(FlowLayer):
    """layers/actnorm.py:5-66.  Device tensors in fp32, 4-D, with fp32 parameters on the same device run on the HIP ActNorm kernels:
    `forward` without an autograd graph as one launch (`ops.finc_actnorm`, the log-det included), `forward` under autograd through
    `ops.actnorm_forward` (backward: finc_actnorm_backward_f32, from the saved OUTPUT), `reverse` without a graph as one launch, and
    the data-dependent initialisation of the first forward as `ops.finc_actnorm_init` (at least two values per channel).  `reverse`
    under autograd inside `ops.reverse_grad()` (what `FlowSequential.rsample` records) goes through `ops.actnorm_reverse` (backward:
    finc_actnorm_reverse_backward_f32, from the saved INPUT).  Everything else -- CPU tensors, fp64, 2-D inputs, `reverse` under
    autograd outside that context, one value per channel -- keeps the PyTorch lines below, which are differentiable as they are."""

    def __init__(self, n_dims):
        super().__init__()
        self.n_dims = n_dims
        self.translation = nn.Parameter(torch.zeros(n_dims))
        self.log_scale = nn.Parameter(torch.zeros(n_dims))
        self.register_buffer('initialized', torch.tensor(0))
        # host-side mirror of `initialized` (None: unknown, read the buffer once): the buffer lives on the device, and
        # testing it costs a device->host sync per layer and call -- 96 per pass of the CIFAR stack, and no HIP graph
        self._init_known = None

    def _is_initialized(self):
        if self._init_known is None:
            self._init_known = bool(self.initialized)      # one sync, then cached
        return self._init_known

    def _load_from_state_dict(self, *args, **kwargs):
        self._init_known = None                            # a checkpoint brings its own flag
        return super()._load_from_state_dict(*args, **kwargs)

    def mark_initialized(self):
        """Skip the data-dependent initialisation (parameters set by hand or by a checkpoint): no sync, graph-safe."""
        self.initialized.fill_(1)
        self._init_known = True

    def reset_initialization(self):
        """Ask for the data-dependent initialisation again (the next forward computes it).  Writing the `initialized` buffer
        directly is not seen by the host-side mirror once it is known."""
        self.initialized.fill_(0)
        self._init_known = False

    def _shaped(self, input):
        shape = (1, -1) + (1,) * (input.dim() - 2)
        return self.translation.view(shape), self.log_scale.view(shape)

    def _hip_device(self, x):
        p = (self.translation, self.log_scale)
        return (_hip_tensor(x) and x.shape[1] == self.n_dims
                and all(q.dtype == torch.float32 and q.device == x.device for q in p) and ops.actnorm_supported())

    def _records_graph(self, x):
        return _records_graph(x, self.log_scale, self.translation)

    def forward(self, input, context=None):
        hip = self._hip_device(input)
        if not self._is_initialized():
            with torch.no_grad():
                if hip and input.numel() // self.n_dims >= 2:
                            ops.finc_actnorm_init(input.detach().contiguous(), self.log_scale.detach(), self.translation.detach())
                else:
                    dims = [d for d in range(input.dim()) if d != 1]
                    self.translation.copy_(input.mean(dim=dims))
                    self.log_scale.copy_(torch.log(input.std(dim=dims) + 1e-8))
                self.initialized.fill_(1)
                self._init_known = True
        if hip:
            if self._records_graph(input):
                return ops.actnorm_forward(input, self.log_scale, self.translation)
            return ops.finc_actnorm(input.contiguous(), self.log_scale.detach(), self.translation.detach(), 1, True)
        t, ls = self._shaped(input)
        return (input - t) * torch.exp(-ls), self.logdet(input, context)

    def _hip_reverse_grad(self, x):
        """`reverse` while autograd records inside `ops.reverse_grad()`: the HIP launch with a backward of its own."""
        return ops.reverse_grad_enabled() and self._records_graph(x) and self._hip_device(x)

    def reverse(self, input, context=None):
        if self._hip_reverse_grad(input):
            return ops.actnorm_reverse(input, self.log_scale, self.translation)
        if self._hip_device(input) and not self._records_graph(input):
            return ops.finc_actnorm(input.contiguous(), self.log_scale.detach(), self.translation.detach(), -1)[0]
        t, ls = self._shaped(input)
        return input * torch.exp(ls) + t

    def reverse_with_logdet(self, input, context=None):
        """`reverse` and the forward log-det at its result: parameters only (`logdet`: a few [C]-sized ops, recorded when a graph is),
        no kernel of its own."""
        out = self.reverse(input, context)
        return out, self.logdet(out, context)

    def invertible_backward_supported(self, input, context=None):
        """Once initialised.  The call that still has to initialise runs the stored path, as it always has."""
        return self._is_initialized() and self._hip_device(input)

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """ONE launch (`ops.finc_actnorm_backward_reconstruct`): the gradients of `forward` and its input from one read of the output."""
        params, asked = _param_needs(self, needs)
        want = {id(p): a for p, a in zip(params, asked)}
        x, gx, gls, gt = ops.finc_actnorm_backward_reconstruct(
            grad_output.contiguous(), grad_logdet, output.contiguous(), self.log_scale.detach(), self.translation.detach(),
            need_x=needs.input, need_gx=needs.grad_input, need_gls=want[id(self.log_scale)], need_gt=want[id(self.translation)])
        grads = {id(self.log_scale): gls, id(self.translation): gt}
        return x, gx, None, [grads[id(p)] for p in params]

    def forward_affine_params(self):
        """forward(x) = (x - translation) * exp(-log_scale): what FlowSequential folds into the FastFlowUnit in front of
        this layer (only once the data-dependent initialisation has happened)."""
        if not self._is_initialized():
            return None
        return self.log_scale, self.translation

    def reverse_affine_params(self):
        """reverse(y) = exp(log_scale) * y + translation, per channel: what FlowSequential folds into the FastFlowUnit
        that comes next in the reverse chain."""
        return self.log_scale, self.translation

    def logdet(self, input, context=None):
        pixels = int(np.prod(input.shape[2:])) if input.dim() > 2 else 1
        return -self.log_scale.sum().expand(input.size(0)) * pixels


def rq_spline_lines(v, cumwidths, cumheights, derivatives, tail_bound, inverse):
    """rational_quadratic.py:117-175 between [-tail_bound, tail_bound] and the identity outside, on knots that broadcast against
    `v.shape + (K + 1,)`, restated without masks or host synchronisations: an element outside the range, or a NaN, is computed at 0
    in its place and `torch.where` keeps the input there -- so its arithmetic is finite and, as in the kernels, it adds exactly
    nothing to the knots' gradients (a NaN carried through the unselected branch would reach every summed gradient as 0 * NaN); the
    inverse's discriminant is clamped at 0 instead of asserted.
    Returns (out, log-derivative of the FORWARD map per element -- in the inverse at the recovered input, minus what the reference's
    inverse returns).  Differentiable in `v` and the knots."""
    K, tb = cumwidths.shape[-1] - 1, tail_bound
    cw, ch, d = (k.expand(*v.shape, K + 1) for k in (cumwidths, cumheights, derivatives))
    inside = (v >= -tb) & (v <= tb)
    u = torch.where(inside, v, torch.zeros_like(v))
    # the knots <= u counted, minus one; knot K stays out of the count, so u == tail_bound lands in the last bin
    idx = ((u.unsqueeze(-1) >= (ch if inverse else cw)[..., :K]).sum(dim=-1) - 1).clamp(0, K - 1).unsqueeze(-1)
    pick = lambda t, o=0: t.gather(-1, idx + o).squeeze(-1)
    cw0, cw1, ch0, d0, d1 = pick(cw), pick(cw, 1), pick(ch), pick(d), pick(d, 1)
    w, h = cw1 - cw0, pick(ch, 1) - ch0
    delta = h / w
    sd = d0 + d1 - 2 * delta
    if inverse:
        # The quadratic is solved from the NEARER knot: the spline is its own mirror image under th -> 1 - th, d0 <-> d1,
        # y - ch0 -> ch1 - y.  Seen from the far knot b^2 and 4ac cancel as y nears it (error 1e-7 (delta / d)^2 in fp32: enough to
        # put the root of a steep bin beside a flat one at 1 + 1e-4); seen from the near one c is small.
        upper = 2 * (u - ch0) > h
        dy = torch.where(upper, pick(ch, 1) - u, u - ch0)
        da = torch.where(upper, d1, d0)
        a = dy * sd + h * (delta - da)
        b = h * da - dy * sd
        c = -delta * dy
        disc = b.pow(2) - 4 * a * c
        # clamped at 0, and the square root taken where it is positive only: autograd's sqrt'(0) = inf times the clamp's 0 is a NaN
        # in every summed knot gradient (beside a steep bin's knot b^2 and 4ac, both ~1e7, cancel to 0 in fp32)
        positive = disc > 0
        root = torch.where(positive, torch.sqrt(torch.where(positive, disc, torch.ones_like(disc))), torch.zeros_like(disc))
        # the root in [0, 1] in the form that adds, never subtracts, two numbers of one sign: 2c / (-b - sqrt) for b >= 0 (the
        # reference's), (-b + sqrt) / 2a for b < 0 -- a flat bin between large derivatives, where -b - sqrt cancels (a + b =
        # h delta > 0, so a > 0 there)
        stable = b >= 0
        r = torch.where(stable, 2 * c, root - b) / torch.where(stable, -b - root, 2 * a)
        # A position in the bin: kept inside [0, 1].  Outside it d1 th^2 + 2 delta tm + d0 (1 - th)^2 can go negative and its log
        # is NaN, from a finite in-range input, and `out` leaves the bin.  The value alone is clamped, straight-through for autograd
        # (r - r.detach() is an exact zero): the kernels' adjoint is analytic at the clamped position, a plain clamp would zero the
        # gradient there.
        r = r.detach().clamp(0, 1) + (r - r.detach())
        th = torch.where(upper, 1 - r, r)
        out = torch.where(upper, cw1 - r * w, r * w + cw0)
        # (and so is the result, the same way: at r = 1 the rounded w + cw0 can land half an ulp of w beyond the knot -- or beyond
        # tail_bound, where the next layer would take it for a tail element)
        out = torch.minimum(torch.maximum(out, cw0), cw1).detach() + (out - out.detach())
    else:
        th = (u - cw0) / w
    tm = th * (1 - th)
    den = delta + sd * tm
    if not inverse:
        out = ch0 + h * (delta * th.pow(2) + d0 * tm) / den
    dnum = delta.pow(2) * (d1 * th.pow(2) + 2 * delta * tm + d0 * (1 - th).pow(2))
    lad = torch.log(dnum) - 2 * torch.log(den)
    return torch.where(inside, out, v), torch.where(inside, lad, torch.zeros_like(lad))


class SplineActivation(_DerivedValues, FlowLayer):
    """layers/activations.py SplineActivation: the element-wise monotone rational-quadratic spline with linear tails
    (layers/splines/rational_quadratic.py), with the reference's constructor, parameter names, shapes and initialisation.  The three
    parameters are composed into the knot table [3 * (n_bins + 1), P] (cumwidths, cumheights, derivatives; P = 1, or one row per
    position with `individual_weights`) by the PyTorch lines of `_knots` -- parameter-sized work, recorded while a graph records,
    otherwise cached per parameter version -- and the map over the activations runs on the HIP spline kernels: fp32 4-D device
    tensors of this layer's `input_size`, fp32 parameters on the same device, 2 <= n_bins <= 16.  `forward` is one launch plus the
    log-det's small reduce (`ops.finc_spline`; under autograd `ops.spline_forward`), `reverse` and `reverse_with_logdet` likewise,
    recorded inside `ops.reverse_grad()` (`ops.spline_reverse`, `ops.spline_reverse_logdet`).  Everything else -- CPU tensors, fp64,
    2-D inputs, other bin counts, `reverse` under autograd outside that context -- runs `_lines`: the same spline restated without
    masks, gathers of masked elements or host synchronisations (`torch.where` on the range, the discriminant clamped at 0), which is
    differentiable as it stands.  The map stays fp32 under autocast."""

    _derived = ("_tab", "_tab_key", "_tab_ready")
    min_bin_width = min_bin_height = min_derivative = 1e-3

    def __init__(self, input_size, n_bins=5, tail_bound=10., individual_weights=False):
        super().__init__()
        self.input_size = tuple(input_size)
        self.n_bins = n_bins
        self.tail_bound = tail_bound
        self.individual_weights = individual_weights
        lead = (1, *self.input_size) if individual_weights else ()
        self.unnormalized_widths = nn.Parameter(torch.randn(*lead, n_bins) * 0.01)
        self.unnormalized_heights = nn.Parameter(torch.randn(*lead, n_bins) * 0.01)
        self.unnormalized_derivatives = nn.Parameter(torch.randn(*lead, n_bins - 1) * 0.01)

    def _params(self):
        return self.unnormalized_widths, self.unnormalized_heights, self.unnormalized_derivatives

    def _knots(self):
        """(cumwidths, cumheights, derivatives), each [P, n_bins + 1]: rational_quadratic.py:97-115 with the padded end derivatives of
        :38-46 (the end knots are pinned by concatenation instead of an in-place write: the same values, and no gradient either)."""
        K, tb = self.n_bins, self.tail_bound
        if self.min_bin_width * K > 1.0 or self.min_bin_height * K > 1.0:
            raise ValueError('Minimal bin width or height too large for the number of bins')
        uw, uh, ud = (p.reshape(-1, p.shape[-1]) for p in self._params())

        def cumulative(u, floor):
            part = floor + (1 - floor * K) * F.softmax(u, dim=-1)
            cum = 2 * tb * torch.cumsum(part, dim=-1) - tb
            ends = cum.new_full((cum.shape[0], 1), tb)
            return torch.cat([-ends, cum[:, :-1], ends], dim=-1)

        constant = float(np.log(np.exp(1 - self.min_derivative) - 1))
        derivatives = self.min_derivative + F.softplus(F.pad(ud, pad=(1, 1)) + constant)
        return cumulative(uw, self.min_bin_width), cumulative(uh, self.min_bin_height), derivatives

    def _compose(self):
        """The knot table as the kernels read it: [3 * (n_bins + 1), P], knot-major."""
        with _fp32_maps(self.unnormalized_widths):
            return torch.cat([k.t() for k in self._knots()], dim=0).contiguous()

    def _table(self):
        params = self._params()
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return self._compose()                                  # recorded: grad_table reaches the parameters through these lines
        key = ops.version_key(*params) + (params[0].device,)
        if getattr(self, "_tab_key", None) != key:
            with torch.no_grad():
                self._tab = self._compose()
            self._tab_key, self._tab_ready = key, ops.Ready(params[0].device)
        else:
            self._tab_ready.wait(self._tab)
        return self._tab

    def _lines(self, v, inverse):
        """The spline on `v` in PyTorch: (out, log-derivative of the FORWARD map per element, at `v` or at the recovered input)."""
        K = self.n_bins
        with _fp32_maps(v):
            shape = (1, *self.input_size, K + 1) if self.individual_weights else (K + 1,)
            return rq_spline_lines(v, *(k.reshape(shape) for k in self._knots()), self.tail_bound, inverse)

    def _hip_device(self, x):
        return (_hip_tensor(x) and tuple(x.shape[1:]) == self.input_size and _params_on_device(x, *self._params())
                and ops.spline_supported(self.n_bins))

    def _records_graph(self, x):
        return _records_graph(x, *self._params())

    def forward(self, input, context=None):
        if self._hip_device(input):
            if self._records_graph(input):
                return ops.spline_forward(input, self._table(), self.tail_bound)
            return ops.finc_spline(input.contiguous(), self._table(), self.tail_bound, 1, True)
        out, lad = self._lines(input, False)
        return out, lad.flatten(start_dim=1).sum(dim=-1)

    def _hip_reverse_grad(self, x):
        """`reverse` while autograd records inside `ops.reverse_grad()`: the HIP launch with a backward of its own."""
        return ops.reverse_grad_enabled() and self._records_graph(x) and self._hip_device(x)

    def reverse(self, input, context=None):
        if self._hip_reverse_grad(input):
            return ops.spline_reverse(input, self._table(), self.tail_bound)
        if self._hip_device(input) and not self._records_graph(input):
            return ops.finc_spline(input.contiguous(), self._table(), self.tail_bound, -1)[0]
        return self._lines(input, True)[0]

    def reverse_with_logdet(self, input, context=None):
        """`reverse` and the forward log-det at its result from the same pass."""
        if self._hip_reverse_grad(input):
            return ops.spline_reverse_logdet(input, self._table(), self.tail_bound)
        if self._hip_device(input) and not self._records_graph(input):
            return ops.finc_spline(input.contiguous(), self._table(), self.tail_bound, -1, True)
        out, lad = self._lines(input, True)
        return out, lad.flatten(start_dim=1).sum(dim=-1)

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]


#: Newton trips of the smooth activations' bracketed inverse, here and in the kernels (finc_activation.h ACT_TRIPS): over the parameter
#: box of DESIGN 3.26 the worst case is at its fp32 floor after 7, plus 2 of margin
ACTIVATION_TRIPS = 9
_FLT_MAX = 3.4028234663852886e38


def bracketed_newton(t, f_and_prime, lo, hi, x, trips=ACTIVATION_TRIPS):
    """`trips` Newton steps on f(x) = t from `x`, kept inside [lo, hi]: each trip shrinks the bracket on the sign of f(x) - t and
    replaces a step that LEAVES it by the midpoint (a step onto an end is inside).  The same count for every element, written with
    `torch.where`: no masks, no host synchronisation.  The arithmetic of finc_activation.h act_inverse."""
    for _ in range(trips):
        f, fp = f_and_prime(x)
        r = f - t
        hi = torch.where(r > 0, x, hi)
        lo = torch.where(r < 0, x, lo)
        xn = x - r / fp
        x = torch.where((xn >= lo) & (xn <= hi), xn, lo + 0.5 * (hi - lo))
    return x


class _Activation(FlowLayer):
    """What the four element-wise activations of layers/activations.py share: the dispatch of `SplineActivation` -- fp32 device
    tensors of two or more dimensions run on the HIP activation kernels (`ops.finc_activation`; under autograd
    `ops.activation_forward`, and for `reverse` / `reverse_with_logdet` inside `ops.reverse_grad()` `ops.activation_reverse` /
    `ops.activation_reverse_logdet`); CPU tensors, float64 and `reverse` under autograd outside that context run the layer's PyTorch
    lines (`_lines`).  `backward_from_output` is ONE launch (finc_activation_backward_f32, rebuild mode): the layer's input with the
    bits `reverse` returns and the gradients taken there, so the layers join `FlowSequential.invertible_backward` runs.  The map stays
    fp32 under autocast."""
    kind = None

    def _numbers(self):
        """(p0, p1) of the entry points."""
        return 0.0, 0.0

    def _slope(self):
        """The learnable kind's slope as a tensor of one element (recorded while a graph records); None otherwise."""
        return None

    def _lines(self, v, inverse):
        """(out, log-derivative of the FORWARD map per element, at `v` or at the recovered input), differentiable."""
        raise NotImplementedError

    def _hip_device(self, x):
        return x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and _params_on_device(x, *self.parameters())

    def _records_graph(self, x):
        return _records_graph(x, *self.parameters())

    def _hip_reverse_grad(self, x):
        """`reverse` while autograd records inside `ops.reverse_grad()`: the HIP launch with a backward of its own."""
        return ops.reverse_grad_enabled() and self._records_graph(x) and self._hip_device(x)

    def _detached_slope(self):
        with torch.no_grad():
            return self._slope()

    def forward(self, input, context=None):
        if self._hip_device(input):
            if self._records_graph(input):
                return ops.activation_forward(input, self.kind, *self._numbers(), self._slope())
            return ops.finc_activation(input.contiguous(), self.kind, *self._numbers(), self._detached_slope(), 1, True)
        out, lad = self._lines(input, False)
        return out, lad.flatten(start_dim=1).sum(dim=-1)

    def reverse(self, input, context=None):
        if self._hip_reverse_grad(input):
            return ops.activation_reverse(input, self.kind, *self._numbers(), self._slope())
        if self._hip_device(input) and not self._records_graph(input):
            return ops.finc_activation(input.contiguous(), self.kind, *self._numbers(), self._detached_slope(), -1)[0]
        return self._lines(input, True)[0]

    def reverse_with_logdet(self, input, context=None):
        """`reverse` and the forward log-det at its result from the same pass."""
        if self._hip_reverse_grad(input):
            return ops.activation_reverse_logdet(input, self.kind, *self._numbers(), self._slope())
        if self._hip_device(input) and not self._records_graph(input):
            return ops.finc_activation(input.contiguous(), self.kind, *self._numbers(), self._detached_slope(), -1, True)
        out, lad = self._lines(input, True)
        return out, lad.flatten(start_dim=1).sum(dim=-1)

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]

    def invertible_backward_supported(self, input, context=None):
        return self._hip_device(input)

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """ONE launch: x = f^-1(output) with the inverse kernel's arithmetic and the forward's gradients at that x."""
        params, asked = _param_needs(self, needs)
        x, gx, gs = ops.finc_activation_backward(grad_output.contiguous(), grad_logdet, output.contiguous(), self.kind, *self._numbers(),
                                                 self._detached_slope(), "rebuild", need_x=needs.input, need_gx=needs.grad_input,
                                                 need_gs=any(asked))
        return x, gx, None, self._slope_chain(gs) if params else []

    def _slope_chain(self, grad_slope):
        return []


def _positive(name, value):
    value = float(value)
    if not (0.0 < value < math.inf):
        raise ValueError(f"{name} must be positive and finite, got {value}")
    return value


def _magnitude(x):
    """|x| as a select: the values of `abs`, and the derivative +1 at 0 where autograd's `abs` has 0 -- the maps built on it are smooth
    there, and their gradient at an input of exactly 0 is to be the analytic one."""
    return torch.where(x < 0, -x, x)


def _softplus_and_sigmoid(x):
    """softplus as max(x, 0) + log1p(exp(-|x|)) and the sigmoid from the same exponential (the maximum as a select too: `clamp` hands
    a gradient of 1 through at 0, and with |x|'s 0 beside it softplus'(0) would come out as 1 instead of 1/2)."""
    e = torch.exp(-_magnitude(x))
    return torch.where(x < 0, torch.zeros_like(x), x) + torch.log1p(e), torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def _implicit_inverse(y, solve, f_and_prime):
    """The result of `solve(y)` (no graph) with the derivative of an inverse function attached: dx/dy = 1 / f'(x), ONE f' at the
    result instead of the unrolled iteration; the log-derivative is then taken at that x, so its gradient reaches y as L' / f'."""
    with torch.no_grad():
        x = solve(y.detach())
        fp = f_and_prime(x)[1]
    if y.requires_grad and torch.is_grad_enabled():
        x = x + (y - y.detach()) / fp                        # (the value is x exactly: y - y.detach() is an exact zero)
    lad = torch.log(f_and_prime(x)[1])
    nan = torch.isnan(y)
    return torch.where(nan, y, x), torch.where(nan, torch.zeros_like(lad), lad)


class SmoothLeakyRelu(_Activation):
    """layers/activations.py:36-54: f(x) = alpha x + (1 - alpha) softplus(x), the reference's constructor.  `reverse` is the bracketed
    Newton iteration of `bracketed_newton` with ACTIVATION_TRIPS trips where the reference runs 100 unbracketed steps: x lies between
    g^-1(y) and g^-1(y - (1 - alpha) ln 2), g the leaky ReLU of slope alpha, and the start is g^-1(y).  Accuracy is claimed at alpha
    among 0.01, 0.1, 0.3, 0.9, 1.0, 1.5, the points the sweep of DESIGN 3.26 covers; elsewhere the result is finite and inside the bracket."""
    kind = "smooth_leaky_relu"

    def __init__(self, alpha=0.3):
        super().__init__()
        self.alpha = _positive("alpha", alpha)

    def _numbers(self):
        return self.alpha, 0.0

    def _map(self, x):
        a = self.alpha
        sp, s = _softplus_and_sigmoid(x)
        return a * x + (1 - a) * sp, a + (1 - a) * s

    def _solve(self, y):
        a = self.alpha
        ginv = lambda v: torch.where(v < 0, v / a, v).clamp(-_FLT_MAX, _FLT_MAX)
        g1, g2 = ginv(y), ginv(y - (1 - a) * math.log(2.0))
        return bracketed_newton(y, self._map, torch.minimum(g1, g2), torch.maximum(g1, g2), g1)

    def _lines(self, v, inverse):
        with _fp32_maps(v):
            if inverse:
                return _implicit_inverse(v, self._solve, self._map)
            f, fp = self._map(v)
            lad = torch.log(fp)
            return f, torch.where(torch.isnan(v), torch.zeros_like(lad), lad)


class SmoothTanh(_Activation):
    """layers/activations.py:108-123: f(x) = tanh(alpha x) + beta x, the reference's constructor; sech^2 is 4 e / (1 + e)^2 with
    e = exp(-2 |alpha x|) (cosh overflows, 1 - tanh^2 cancels).  `reverse` is the bracketed Newton iteration on |y| (f is odd), between
    max(|y| / (alpha + beta), (|y| - 1) / beta) and |y| / beta, from the lower end: the reference's unbracketed iteration cycles for
    (alpha, beta) = (3, 0.05).  Accuracy is claimed at (alpha, beta) among (1, 0.1), (3, 0.05), (8, 0.01), (0.5, 1), (0.1, 0.01), the
    points the sweep of DESIGN 3.26 covers; elsewhere, a finite bracketed value."""
    kind = "smooth_tanh"

    def __init__(self, alpha=1.0, beta=0.1):
        super().__init__()
        self.alpha = _positive("alpha", alpha)
        self.beta = _positive("beta", beta)

    def _numbers(self):
        return self.alpha, self.beta

    def _map(self, x):
        a, b = self.alpha, self.beta
        u = a * x
        e = torch.exp(-2 * _magnitude(u))
        t = (1 - e) / (1 + e)
        return torch.where(u < 0, -t, t) + b * x, b + a * (4 * e / ((1 + e) * (1 + e)))

    def _solve(self, y):
        a, b = self.alpha, self.beta
        t = y.abs()
        hi = (t / b).clamp(max=_FLT_MAX)
        lo = torch.minimum(torch.maximum(t / (a + b), (t - 1) / b), hi)
        x = bracketed_newton(t, self._map, lo, hi, lo)
        return torch.where(y < 0, -x, x)

    def _lines(self, v, inverse):
        with _fp32_maps(v):
            if inverse:
                return _implicit_inverse(v, self._solve, self._map)
            f, fp = self._map(v)
            lad = torch.log(fp)
            return f, torch.where(torch.isnan(v), torch.zeros_like(lad), lad)


def _leaky_lines(v, alpha, inverse):
    """x < 0 ? alpha x : x and back (x < 0 strictly, as the reference compares), `alpha` a number or a tensor of one element.  The
    unselected branch is computed at 0: a NaN carried through it would reach the slope's summed gradient as 0 * NaN."""
    alpha = torch.as_tensor(alpha, dtype=v.dtype, device=v.device)
    neg = v < 0
    u = torch.where(neg, v, torch.zeros_like(v))
    out = torch.where(neg, u / alpha if inverse else alpha * u, v)
    return out, torch.where(neg, torch.log(alpha).expand_as(v), torch.zeros_like(v))


class LeakyRelu(_Activation):
    """layers/activations.py:57-79, the reference's constructor."""
    kind = "leaky_relu"

    def __init__(self, alpha=0.1):
        super().__init__()
        self.alpha = _positive("alpha", alpha)

    def _numbers(self):
        return self.alpha, 0.0

    def _lines(self, v, inverse):
        with _fp32_maps(v):
            return _leaky_lines(v, self.alpha, inverse)


class LearnableLeakyRelu(_Activation):
    """layers/activations.py:82-105: the leaky ReLU with slope sigmoid(alpha_logit) + 0.5, the reference's parameter name, shape [1]
    and initialisation.  `alpha_logit -> alpha` is one recorded, parameter-sized PyTorch line; the kernels read the slope from that
    device tensor, so nothing goes to the host and the layer can be captured in a HIP graph.  The slope's gradient comes from the
    backward launch (a fixed-order sum) and reaches `alpha_logit` through that line."""
    kind = "learnable_leaky_relu"

    def __init__(self):
        super().__init__()
        self.alpha_logit = nn.Parameter(torch.zeros([1]))

    def get_alpha(self):
        with _fp32_maps(self.alpha_logit):
            return torch.sigmoid(self.alpha_logit) + .5

    def _slope(self):
        return self.get_alpha()

    def _slope_chain(self, grad_slope):
        if grad_slope is None:
            return [None]
        s = torch.sigmoid(self.alpha_logit.detach())
        return [grad_slope.view_as(s) * s * (1 - s)]

    def _lines(self, v, inverse):
        with _fp32_maps(v):
            return _leaky_lines(v, self.get_alpha(), inverse)


class Conv1x1(_DerivedValues, FlowLayer):
    """layers/conv1x1.py:8-49.  Device tensors in fp32 with a channel count the library instantiates run on the HIP mixing
    kernel: inference / sampling (no autograd graph) as one streaming launch (`ops.finc_mix`), `forward` under autograd through
    `ops.mix_forward` (backward: finc_mix_backward_f32), and so does `reverse` under autograd inside `ops.reverse_grad()` (what
    `FlowSequential.rsample` records), on `torch.inverse(W)` -- a recorded [C, C] op -- or, with W frozen, on the cached inverse.
    Everything else -- CPU tensors, fp64, other channel counts, `reverse` under autograd outside that context -- keeps F.conv2d,
    with autocast switched off around it: this layer is part of the flow's own map and stays fp32 under autocast."""

    _derived = ("_w_inv", "_inv_key", "_inv_ready", "_ld", "_ld_key", "_ld_ready", "_m_aff", "_b_aff", "_aff_key", "_aff_ready",
                "_m_lead", "_b_lead", "_lead_key", "_lead_inv", "_lead_obj", "_lead_ready")

    def __init__(self, n_channels):
        super().__init__()
        self.n_channels = n_channels
        q = np.linalg.qr(np.random.randn(n_channels, n_channels))[0]
        self.W = nn.Parameter(torch.from_numpy(q.astype('float32')))

    def _hip_device(self, x):
        return _hip_tensor(x) and ops.mix_supported(self.n_channels)

    def _hip(self, x):
        return not _records_graph(x, self.W) and self._hip_device(x)

    def forward(self, x, context=None):
        h, w = x.shape[2:]
        ldj = h * w * torch.slogdet(self.W)[1]
        if self._hip(x):
            return ops.finc_mix(x.contiguous(), self.W.detach().contiguous()), ldj
        if torch.is_grad_enabled() and self._hip_device(x):      # training: the same kernel under autograd
            return ops.mix_forward(x, self.W), ldj
        with _fp32_maps(x):
            return F.conv2d(x, self.W.view(self.n_channels, self.n_channels, 1, 1)), ldj

    def _inverse_matrix(self):
        # the reference inverts W on every call (layers/conv1x1.py:37-39); cache it per weight version so that a
        # sampling pass has no LU factorisation (and no host sync) in it and can be captured in a HIP graph
        key = ops.version_key(self.W) + (self.W.device,)
        if getattr(self, "_inv_key", None) != key:
            with torch.no_grad():
                self._w_inv = torch.inverse(self.W.detach()).contiguous()
            self._inv_key, self._inv_ready = key, ops.Ready(self.W.device)
            self._aff_key = None
        else:
            self._inv_ready.wait(self._w_inv)
        return self._w_inv

    def _hip_reverse_grad(self, z):
        """`reverse` while autograd records inside `ops.reverse_grad()`: the mix kernel under autograd."""
        return ops.reverse_grad_enabled() and _records_graph(z, self.W) and self._hip_device(z)

    def reverse(self, z, context=None):
        if self._hip(z):
            return ops.finc_mix(z.contiguous(), self._inverse_matrix())
        if torch.is_grad_enabled() and self.W.requires_grad:
            w_inv = torch.inverse(self.W)
        else:
            w_inv = self._inverse_matrix()
        if self._hip_reverse_grad(z):
            return ops.mix_forward(z, w_inv)
        with _fp32_maps(z):
            return F.conv2d(z, w_inv.view(self.n_channels, self.n_channels, 1, 1))

    def invertible_backward_supported(self, x, context=None):
        return self._hip_device(x) and x.shape[1] == self.n_channels and _params_on_device(x, self.W)

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """Two existing launches: x = finc_mix(output, W^-1) on the cached inverse, then finc_mix_backward at (grad_output, x); the
        log-det's share, H * W * (sum_b grad_logdet[b]) * W^-T, is a [C, C] op."""
        need_gw = _param_needs(self, needs)[1][0]
        w_inv = self._inverse_matrix()
        x = ops.finc_mix(output.contiguous(), w_inv) if (needs.input or need_gw) else None
        gx, gw, _ = ops.finc_mix_backward(grad_output.contiguous(), x, self.W.detach().contiguous(), need_gx=needs.grad_input,
                                          need_gm=need_gw)
        if need_gw and grad_logdet is not None:
            h, w = output.shape[2:]
            gw = gw + (h * w) * grad_logdet.sum() * w_inv.t()
        return x, gx, None, [gw]

    def _log_abs_det(self):
        """log|det W|, 0-dim: recorded (`torch.slogdet`) while autograd records through W; otherwise cached per weight version, as
        `_inverse_matrix` is, so that a no-grad sampling pass has no LU factorisation (and no host sync) in it."""
        if torch.is_grad_enabled() and self.W.requires_grad:
            return torch.slogdet(self.W)[1]
        key = ops.version_key(self.W) + (self.W.device,)
        if getattr(self, "_ld_key", None) != key:
            with torch.no_grad():
                self._ld = torch.slogdet(self.W.detach())[1]
            self._ld_key, self._ld_ready = key, ops.Ready(self.W.device)
        else:
            self._ld_ready.wait(self._ld)
        return self._ld

    def mix_logdet(self, x):
        """The layer's forward log-det for activations shaped like `x`, [B]: h * w * log|det W| (the same in and out of the layer)."""
        h, w = x.shape[2:]
        return (h * w * self._log_abs_det()).expand(len(x))

    def reverse_with_logdet(self, z, context=None):
        out = self.reverse(z, context)
        return out, self.mix_logdet(out)

    def reverse_then_affine(self, z, log_scale, translation):
        """exp(log_scale) * reverse(z) + translation in ONE launch: the ActNorm that precedes this layer in
        the model follows it in the reverse chain (layers/actnorm.py:47-52), and a per-channel affine map after a channel
        mix is a row scaling of the matrix plus a bias.  None when this call cannot take the HIP path."""
        if not self._hip(z):
            return None
        w_inv = self._inverse_matrix()
        key = ops.version_key(log_scale, translation)
        if getattr(self, "_aff_key", None) != key:
            with torch.no_grad():
                self._m_aff = (torch.exp(log_scale.detach().float()).view(-1, 1) * w_inv).contiguous()
                self._b_aff = translation.detach().float().contiguous()
            self._aff_key, self._aff_ready = key, ops.Ready(z.device)
        else:
            self._aff_ready.wait(self._m_aff, self._b_aff)
        return ops.finc_mix(z.contiguous(), self._m_aff, self._b_aff)

    def reverse_premultiplied(self, z, lead, log_scale=None, translation=None):
        """blockdiag(lead) (exp(log_scale) * reverse(z) + translation) in ONE launch: `lead` [G, Cq, Cq] is the inverse of
        the unit triangular tap of the FastFlowUnit that follows in the reverse chain, which then runs
        without its z-term.  The product with a block-diagonal matrix is folded into the mix's matrix and bias on the host,
        once per weight version.  None when this call cannot take the HIP path."""
        if not self._hip(z):
            return None
        w_inv = self._inverse_matrix()
        # (`lead` and `w_inv` are compared by identity and kept alive here: both are cache entries that are REPLACED when their
        # weights change, and the address of a freed tensor is the first one the allocator hands out again)
        key = () if log_scale is None else ops.version_key(log_scale, translation)
        if (getattr(self, "_lead_key", None) != key or getattr(self, "_lead_inv", None) is not w_inv
                or getattr(self, "_lead_obj", None) is not lead):
            with torch.no_grad():
                m = w_inv.double()
                b = None
                if log_scale is not None:
                    m = torch.exp(log_scale.detach().double()).view(-1, 1) * m
                    b = translation.detach().double()
                blk = torch.block_diag(*lead.double().unbind(0))
                self._m_lead = (blk @ m).float().contiguous()
                self._b_lead = None if b is None else (blk @ b).float().contiguous()
            self._lead_key, self._lead_inv, self._lead_obj, self._lead_ready = key, w_inv, lead, ops.Ready(z.device)
        else:
            self._lead_ready.wait(self._m_lead, self._b_lead)
        return ops.finc_mix(z.contiguous(), self._m_lead, self._b_lead)

    def logdet(self, input, context=None):
        raise NotImplementedError


def _plu_factor(W):
    """W = P L U on the CPU in float64: (lower, upper, log_s, sign_s, perm) with W[r] = (L (U + diag(sign_s * exp(log_s))))[perm[r]]
    (torch.linalg.lu's P: perm = P.argmax(1)); the triangles strict, zero elsewhere."""
    A = torch.as_tensor(W).detach().to("cpu", torch.float64)
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError("expected a square matrix")
    P, L, U = torch.linalg.lu(A)
    d = U.diagonal()
    if not bool(torch.isfinite(d).all() and (d != 0).all()):
        raise ValueError("the matrix is singular: it has no PLU parametrisation with a finite log_s")
    return L.tril(-1), U.triu(1), d.abs().log(), d.sign(), P.argmax(1).to(torch.int32)


def _check_permutation(perm, n):
    """On the host, once, where `perm` is set: the kernels cannot report a bad entry without a synchronisation per call."""
    p = torch.as_tensor(perm).detach().cpu().reshape(-1)
    if p.dtype.is_floating_point or p.numel() != n or not torch.equal(p.long().sort()[0], torch.arange(n)):
        raise ValueError("perm must be a permutation of 0 .. %d" % (n - 1))


class Conv1x1LU(Conv1x1):
    """The 1x1 convolution in Glow's PLU parametrisation (Kingma & Dhariwal 2018, 3.2): W = P L (U + diag(s)) with a fixed permutation
    and a fixed sign of s, so that log|det W| = sum(log_s) and W^-1 is two triangular solves -- no factorisation and no host
    synchronisation on any path.  Parameters `lower`, `upper` [C, C] (strict triangles), `log_s` [C]; buffers `sign_s` [C], `perm` [C]
    int32 (W[r] = (L Ut)[perm[r]]).  Constructed from the orthogonal matrix `Conv1x1` draws (the same np.random calls: one seed gives
    both layers the same matrix), factorised on the CPU in float64.

    On the device in fp32 up to `ops.plu_supported` (512 channels), W, W^-1 and the log-det come from ONE HIP launch
    (`ops.finc_plu_compose`): recorded per call while autograd records through the parameters (`ops.plu_compose`, its backward one
    launch), otherwise cached per parameter version with an `ops.Ready` token.  Everything `Conv1x1` does with its matrix -- the mix
    kernel, the folds of FlowSequential, `backward_from_output` -- this layer does with the composed one.  CPU tensors, float64 and
    wider matrices run the written-out composition in PyTorch (`dense`, `_compose_torch`).  `W` is that composition, read-only."""

    _derived = Conv1x1._derived + ("_plu", "_plu_key", "_plu_ready")

    def __init__(self, n_channels):
        FlowLayer.__init__(self)
        self.n_channels = n_channels
        q = np.linalg.qr(np.random.randn(n_channels, n_channels))[0]
        self._set_factors(_plu_factor(torch.from_numpy(q)), torch.float32)

    def _set_factors(self, factors, dtype, device=None):
        lower, upper, log_s, sign_s, perm = factors
        _check_permutation(perm, self.n_channels)
        self.lower = nn.Parameter(lower.to(device=device, dtype=dtype))
        self.upper = nn.Parameter(upper.to(device=device, dtype=dtype))
        self.log_s = nn.Parameter(log_s.to(device=device, dtype=dtype))
        self.register_buffer("sign_s", sign_s.to(device=device, dtype=dtype))
        self.register_buffer("perm", perm.to(device=device))

    @classmethod
    def from_dense(cls, W):
        """The layer whose matrix is `W` [C, C] (a tensor or an array): factorised on the CPU in float64, stored in float32 (float64
        for a float64 `W`) on W's device."""
        W = torch.as_tensor(W)
        layer = cls.__new__(cls)
        FlowLayer.__init__(layer)
        layer.n_channels = W.shape[0]
        layer._set_factors(_plu_factor(W), torch.float64 if W.dtype == torch.float64 else torch.float32, W.device)
        return layer

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if prefix + "perm" in state_dict:
            _check_permutation(state_dict[prefix + "perm"], self.n_channels)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ---- the written-out composition: the PyTorch lines (differentiable as they are) ----
    def _triangles(self):
        eye = torch.eye(self.n_channels, dtype=self.lower.dtype, device=self.lower.device)
        return torch.tril(self.lower, -1) + eye, torch.triu(self.upper, 1) + torch.diag(self.sign_s * torch.exp(self.log_s)), eye

    def _compose_torch(self, need_w=True, need_winv=True, need_logdet=True):
        w = w_inv = logdet = None
        with _fp32_maps(self.lower):
            L, Ut, eye = self._triangles()
            rows = self.perm.long()
            if need_w:
                w = (L @ Ut).index_select(0, rows)
            if need_winv:                        # column r: Ut^-1 L^-1 e_perm[r]
                y = torch.linalg.solve_triangular(L, eye.index_select(1, rows), upper=False, unitriangular=True)
                w_inv = torch.linalg.solve_triangular(Ut, y, upper=True)
            if need_logdet:
                logdet = self.log_s.sum()
        return w, w_inv, logdet

    def dense(self):
        """The composed matrix [C, C] by the PyTorch lines, recorded when autograd records."""
        return self._compose_torch(True, False, False)[0]

    @property
    def W(self):
        return self.dense()

    # ---- where W, W^-1 and log|det W| come from ----
    def _factors(self):
        return self.lower, self.upper, self.log_s

    def _plu_kernel(self):
        p = self.lower
        return (p.is_cuda and all(q.dtype == torch.float32 and q.device == p.device for q in (p, self.upper, self.log_s, self.sign_s))
                and self.perm.device == p.device and ops.plu_supported(self.n_channels))

    def _records(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self._factors())

    def _recorded(self, need_w, need_winv, need_logdet):
        """One recorded composition: `ops.plu_compose` (one launch, its backward another) or the PyTorch lines."""
        if self._plu_kernel():
            return ops.plu_compose(self.lower, self.upper, self.log_s, self.sign_s, self.perm, need_w, need_winv, need_logdet)
        return self._compose_torch(need_w, need_winv, need_logdet)

    def _values(self):
        """(W, W^-1, log|det W|) without a graph, per parameter version as `Conv1x1._inverse_matrix` keeps its inverse: one compose
        launch fills all three."""
        p = self.lower
        key = ops.version_key(p, self.upper, self.log_s, self.sign_s, self.perm) + (p.device, p.dtype)
        if getattr(self, "_plu_key", None) != key:
            with torch.no_grad():
                if self._plu_kernel():
                    self._plu = ops.finc_plu_compose(p.detach().contiguous(), self.upper.detach().contiguous(),
                                                     self.log_s.detach().contiguous(), self.sign_s, self.perm)
                else:
                    self._plu = tuple(t.contiguous() for t in self._compose_torch())
            self._plu_key, self._plu_ready = key, ops.Ready(p.device)
            self._aff_key = None
        else:
            self._plu_ready.wait(*self._plu)
        return self._plu

    def _inverse_matrix(self):
        return self._values()[1]

    def _log_abs_det(self):
        if self._records():
            return self._recorded(False, False, True)[2]
        return self._values()[2]

    def _hip(self, x):
        return not _records_graph(x, *self._factors()) and self._hip_device(x)

    def _hip_reverse_grad(self, z):
        return ops.reverse_grad_enabled() and _records_graph(z, *self._factors()) and self._hip_device(z)

    # ---- the layer ----
    def forward(self, x, context=None):
        h, w = x.shape[2:]
        if not self._plu_kernel():               # the PyTorch lines
            mat, ld = (self.W if self._records() else self._values()[0]), self._log_abs_det()
        elif self._records():
            mat, _, ld = self._recorded(True, False, True)
        else:
            mat, _, ld = self._values()
        ldj = h * w * ld
        if self._hip(x):
            return ops.finc_mix(x.contiguous(), mat), ldj
        if torch.is_grad_enabled() and self._hip_device(x):
            return ops.mix_forward(x, mat), ldj
        with _fp32_maps(x):
            return F.conv2d(x, mat.view(self.n_channels, self.n_channels, 1, 1)), ldj

    def _reverse_on(self, z, w_inv):
        if self._hip(z):
            return ops.finc_mix(z.contiguous(), w_inv)
        if self._hip_reverse_grad(z):
            return ops.mix_forward(z, w_inv)
        with _fp32_maps(z):
            return F.conv2d(z, w_inv.view(self.n_channels, self.n_channels, 1, 1))

    def reverse(self, z, context=None):
        return self._reverse_on(z, self._recorded(False, True, False)[1] if self._records() else self._inverse_matrix())

    def reverse_with_logdet(self, z, context=None):
        if not (self._records() and self._plu_kernel()):
            return super().reverse_with_logdet(z, context)
        _, w_inv, ld = self._recorded(False, True, True)        # one recorded composition for both
        out = self._reverse_on(z, w_inv)
        return out, (out.shape[2] * out.shape[3] * ld).expand(len(out))

    def invertible_backward_supported(self, x, context=None):
        return (self._hip_device(x) and x.shape[1] == self.n_channels and _params_on_device(x, *self._factors())
                and self._plu_kernel())

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """x = finc_mix(output, W^-1) and finc_mix_backward at (grad_output, x) on the cached matrices, then ONE compose-backward
        launch from grad_mat to the parameters; the log-det's share, H * W * sum_b grad_logdet[b], is added to every grad_log_s
        there (no W^-T)."""
        params, asked = _param_needs(self, needs)
        want = {id(p): a for p, a in zip(params, asked)}
        need_gw = any(asked)
        mat, w_inv, _ = self._values()
        x = ops.finc_mix(output.contiguous(), w_inv) if (needs.input or need_gw) else None
        gx, gw, _ = ops.finc_mix_backward(grad_output.contiguous(), x, mat, need_gx=needs.grad_input, need_gm=need_gw)
        grads = {}
        if need_gw:
            h, w = output.shape[2:]
            gld = None if grad_logdet is None else ((h * w) * grad_logdet.sum()).float().contiguous()
            grads = dict(zip(map(id, self._factors()), ops.finc_plu_compose_backward(
                gw, gld, self.lower.detach().contiguous(), self.upper.detach().contiguous(), self.log_s.detach().contiguous(),
                self.sign_s, self.perm, *(want.get(id(p), False) for p in self._factors()))))
        return x, gx, None, [grads.get(id(p)) for p in params]


def convert_conv1x1(model, to="lu"):
    """Swap every 1x1 convolution of a `FlowSequential` for its other parametrisation with the same matrix, in `sequence_modules`
    and in the registered children: `to="lu"` a `Conv1x1` becomes a `Conv1x1LU` (factorised on the CPU in float64), `to="dense"` the
    reverse (composed in float64).  The new layers keep the old ones' dtype and device; optimisers hold the old parameters and have to
    be rebuilt.  Returns `model`."""
    if to not in ("lu", "dense"):
        raise ValueError('to must be "lu" or "dense"')
    mods = list(model.sequence_modules)
    for i, m in enumerate(mods):
        if to == "lu" and type(m) is Conv1x1:
            new = Conv1x1LU.from_dense(m.W.detach())
        elif to == "dense" and isinstance(m, Conv1x1LU):
            new = Conv1x1.__new__(Conv1x1)
            FlowLayer.__init__(new)
            new.n_channels = m.n_channels
            with torch.no_grad():
                p = m.lower
                twin = Conv1x1LU.__new__(Conv1x1LU)
                FlowLayer.__init__(twin)
                twin.n_channels = m.n_channels
                twin._set_factors(tuple(t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu()
                                        for t in (m.lower, m.upper, m.log_s, m.sign_s, m.perm)), torch.float64)
                new.W = nn.Parameter(twin.dense().to(device=p.device, dtype=p.dtype))
        else:
            continue
        new.train(m.training)
        mods[i] = new
        for name, child in list(model.named_children()):
            if child is m:
                setattr(model, name, new)
    model.sequence_modules = tuple(mods)
    return model


class Conv2dZero(nn.Module):
    """Zero-initialised 3x3 conv with a learned per-channel log-scale (layers/coupling.py:10-43)."""

    def __init__(self, in_channels, out_channels, logscale_factor=3):
        super().__init__()
        self.logscale_factor = logscale_factor
        self.weight = nn.Parameter(torch.zeros(out_channels, in_channels, 3, 3))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.logs = nn.Parameter(torch.zeros(out_channels))

    def forward(self, input):
        out = F.conv2d(input, self.weight, self.bias, padding=1)
        return out * torch.exp(self.logs * self.logscale_factor).view(1, -1, 1, 1)


class Coupling(_DerivedValues, FlowLayer):
    """layers/coupling.py:44-105.  Device tensors in fp32 with an even channel count run everything behind the net's last convolution
    on the HIP coupling kernel (`ops.finc_coupling`: affine transform, log-det and the copy of the untouched half in one launch).
    Without an autograd graph (inference, sampling) the net's `Conv2d(bias) + ReLU` pairs are `F.conv2d(bias=None)` +
    `ops.finc_bias_relu` in place as well; under autograd `forward` goes through `ops.coupling_forward` (backward:
    finc_coupling_backward_f32) and the net stays PyTorch; so does `reverse` under autograd inside `ops.reverse_grad()` (what
    `FlowSequential.rsample` records), through `ops.coupling_reverse` (backward: finc_coupling_reverse_backward_f32, from the saved
    OUTPUT).  Everything else -- CPU tensors, fp64, odd channel counts, `reverse` under autograd outside that context -- keeps the
    PyTorch formula below.

    Under `torch.autocast(device_type="cuda", dtype=torch.bfloat16)` only the NET runs in bfloat16; x, y, the scale and shift and the
    log-det stay fp32.  The net's bf16 output goes to the HIP transform as it lies (the `_rawbf16_f32` entry points: no cast of `raw`
    in front, grad_raw written in bf16 for the net's backward), and the inference path's bias + ReLU runs in place on the bf16 hidden
    tensor (finc_bias_relu_bf16).  The two paths round the hidden activations at different points there -- the recording path's
    `Conv2d` adds its bf16 bias inside the convolution, the inference path adds the fp32 bias behind a bf16-rounded convolution -- so
    `log_prob` with and without a graph differ at the bf16 level (1e-7 in fp32); each path is invertible in itself.  There are no
    float16 kernels: under fp16 autocast the net runs as PyTorch has it and its output is upcast (`raw.float()`) for the fp32 entry
    points.  The PyTorch formula lines upcast the net's output the same way, in front of the same h = a * raw + b."""

    _derived = ("_ab", "_ab_key", "_ab_ready")

    def __init__(self, input_size, width=512, n_context=None):
        super().__init__()
        self.n_channels = input_size[0]
        self.half_channels = self.n_channels // 2
        self.width = width
        self.uses_context = n_context is not None
        in_channels = self.half_channels + (n_context or 0)
        self.net = nn.Sequential(nn.Conv2d(in_channels, width, kernel_size=(3, 3), padding=(1, 1)), nn.ReLU(),
                                 nn.Conv2d(width, width, (1, 1)), nn.ReLU(),
                                 Conv2dZero(width, self.n_channels))

    def _hip_device(self, x):
        return _hip_tensor(x) and ops.coupling_supported(self.n_channels)

    def _records_graph(self, x, context):
        # (the net's parameters are walked only where a graph can be recorded at all: not per layer of a sampling pass)
        return torch.is_grad_enabled() and _records_graph(x, context, *self.net.parameters())

    def _hip(self, x, context=None):
        """The inference path: HIP transform and HIP bias + ReLU, nothing recorded for autograd."""
        return not self._records_graph(x, context) and self._hip_device(x)

    def _hip_train(self, x, context=None):
        """`forward` under autograd: PyTorch net, HIP transform with its own backward."""
        return self._records_graph(x, context) and self._hip_device(x)

    def _hip_reverse_grad(self, x, context=None):
        """`reverse` while autograd records inside `ops.reverse_grad()`: PyTorch net, HIP transform with its own backward."""
        return ops.reverse_grad_enabled() and self._hip_train(x, context)

    def _raw_train(self, x, context):
        n = self.net
        return self._kernel_raw(F.conv2d(n[:4](self._net_input(x, context)), n[4].weight, None, padding=1))

    @staticmethod
    def _kernel_raw(raw):
        """`raw` as the transform takes it: fp32 and bfloat16 as they are; float16 (fp16 autocast has no kernels) upcast."""
        return raw.float() if raw.dtype == torch.float16 else raw

    def _scale_shift(self):
        # h = a * raw + b with raw the last convolution WITHOUT its bias: Conv2dZero is (conv + bias) * exp(logs * factor)
        last = self.net[4]
        a = torch.exp(last.logs * last.logscale_factor)
        return a, last.bias * a

    def _scale_shift_cached(self):
        # once per parameter version: a sampling pass has no [C]-sized launches in it.  (During a stream capture nothing is cached:
        # a tensor made there is only filled when the graph replays.)
        last = self.net[4]
        key = ops.version_key(last.logs, last.bias) + (last.logs.device,)
        if getattr(self, "_ab_key", None) == key:
            self._ab_ready.wait(*self._ab)
            return self._ab
        with torch.no_grad():
            a, b = self._scale_shift()
            ab = (a.contiguous(), b.contiguous())
        if not (last.logs.is_cuda and ops._capturing()):
            self._ab, self._ab_key, self._ab_ready = ab, key, ops.Ready(last.logs.device)
        return ab

    def _net_input(self, x, context):
        assert (context is not None) == self.uses_context
        x1 = x[:, :self.half_channels]
        return x1 if context is None else torch.cat([x1, context], dim=1)

    def _raw_inference(self, x, context):
        n = self.net
        with torch.no_grad():
            if _autocast_dtype(x) == torch.float16 or ops.recorded_net_enabled():
                return self._raw_train(x, context).contiguous()
            h = F.conv2d(self._net_input(x, context), n[0].weight, None, padding=1).contiguous()
            ops.finc_bias_relu(h, n[0].bias.detach(), out=h)
            h = F.conv2d(h, n[2].weight, None).contiguous()
            ops.finc_bias_relu(h, n[2].bias.detach(), out=h)
            return F.conv2d(h, n[4].weight, None, padding=1).contiguous()

    def _params(self, x, context):
        assert (context is not None) == self.uses_context
        x1, x2 = x[:, :self.half_channels], x[:, self.half_channels:]
        if _autocast_dtype(x) is None:
            h = self.net(x1 if context is None else torch.cat([x1, context], dim=1))
        else:                       # the net in the autocast dtype, its output upcast in front of h = a * raw + b (as on the HIP path)
            a, b = self._scale_shift()
            h = self._raw_train(x, context).to(x.dtype) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        log_s = 2.0 * torch.tanh(h[:, ::2] / 2.0)
        return x1, x2, log_s, h[:, 1::2]

    def forward(self, input, context=None):
        if self._hip(input, context):
            x = input.contiguous()
            a, b = self._scale_shift_cached()
            return ops.finc_coupling(x, self._raw_inference(x, context), a, b, 1, True)
        if self._hip_train(input, context):
            a, b = self._scale_shift()
            return ops.coupling_forward(input, self._raw_train(input, context), a, b)
        x1, x2, log_s, t = self._params(input, context)
        return torch.cat([x1, x2 * torch.exp(log_s) + t], dim=1), log_s.flatten(start_dim=1).sum(-1)

    def reverse(self, input, context=None):
        if self._hip(input, context):
            x = input.contiguous()
            a, b = self._scale_shift_cached()
            return ops.finc_coupling(x, self._raw_inference(x, context), a, b, -1, False)[0]
        if self._hip_reverse_grad(input, context):
            a, b = self._scale_shift()
            return ops.coupling_reverse(input, self._raw_train(input, context), a, b)
        x1, x2, log_s, t = self._params(input, context)
        return torch.cat([x1, (x2 - t) * torch.exp(-log_s)], dim=1)

    def reverse_with_logdet(self, input, context=None):
        """`reverse` with the forward log-det at its result, sum s per image, from the same pass (s depends on the untouched half
        only): the three branches of `reverse`, on `ops.finc_coupling_reverse_logdet` / `ops.coupling_reverse_logdet` (backward:
        finc_coupling_reverse_logdet_backward_f32) where that one launches the HIP kernel."""
        if self._hip(input, context):
            x = input.contiguous()
            a, b = self._scale_shift_cached()
            return ops.finc_coupling_reverse_logdet(x, self._raw_inference(x, context), a, b)
        if self._hip_reverse_grad(input, context):
            a, b = self._scale_shift()
            return ops.coupling_reverse_logdet(input, self._raw_train(input, context), a, b)
        x1, x2, log_s, t = self._params(input, context)
        return torch.cat([x1, (x2 - t) * torch.exp(-log_s)], dim=1), log_s.flatten(start_dim=1).sum(-1)

    def invertible_backward_supported(self, input, context=None):
        if (context is not None) != self.uses_context or not self._hip_device(input) or input.shape[1] != self.n_channels:
            return False
        acts = (input,) if context is None else (input, context)
        return all(_hip_tensor(t) for t in acts) and _params_on_device(input, *acts[1:], *self.net.parameters())

    def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
        """The net sees the untouched half only, and that half of the input IS that half of the output, bit for bit: the net is run
        again on it under autograd (`_raw_train` on a detached leaf), ONE launch (`ops.finc_coupling_backward_reconstruct`) gives the
        input, the direct grad_input and the gradients of raw, a and b, and one `torch.autograd.grad` pushes those three through the net
        and `_scale_shift()` to the net's parameters, the untouched half and the context."""
        params, asked = _param_needs(self, needs)
        y, half = output.contiguous(), self.half_channels
        with torch.enable_grad():
            y1 = y[:, :half].detach().requires_grad_(needs.grad_input)
            ctx = None if context is None else context.detach().requires_grad_(needs.grad_context)
            raw = self._raw_train(y1, ctx)
            a, b = self._scale_shift()
        wanted = [t for t, w in [(y1, needs.grad_input), (ctx, needs.grad_context)] + list(zip(params, asked)) if w]
        through = bool(wanted)                                  # does anything behind raw, a and b want a gradient?
        x, gx, graw, ga, gb = ops.finc_coupling_backward_reconstruct(
            grad_output.contiguous(), grad_logdet, y, raw.detach().contiguous(), a.detach().contiguous(), b.detach().contiguous(),
            need_x=needs.input, need_gx=needs.grad_input, need_graw=through and raw.requires_grad,
            need_ga=through and a.requires_grad, need_gb=through and b.requires_grad)
        heads = [(t, g) for t, g in ((raw, graw), (a, ga), (b, gb)) if g is not None]
        got = iter(torch.autograd.grad([t for t, _ in heads], wanted, [g for _, g in heads], allow_unused=True)
                   if heads else [None] * len(wanted))
        if needs.grad_input:
            g1 = next(got)
            if g1 is not None:
                gx[:, :half] += g1
        gctx = next(got) if needs.grad_context else None
        return x, gx, gctx, [next(got) if w else None for w in asked]

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]


class GaussianPrior(nn.Module):
    """Standard-normal base with the interface of train/losses.py:17-45 (device follows the module)."""

    def __init__(self, size):
        super().__init__()
        self.size = tuple(size)
        self.dim = int(np.prod(size))
        self.register_buffer('_anchor', torch.zeros(1), persistent=False)  # not in reference checkpoints

    def log_prob(self, input, context=None, sum=True):
        z = input.reshape(-1, self.dim)
        return -0.5 * (z * z).sum(-1) - 0.5 * self.dim * math.log(2 * math.pi)

    def forward(self, input, context=None):
        return -self.log_prob(input, context).sum(-1)

    def sample(self, n_samples, context=None):
        x = torch.randn(n_samples, *self.size, device=self._anchor.device, dtype=self._anchor.dtype)   # (model.double() draws doubles)
        return x, self.log_prob(x, context)


class SplitPrior(FlowLayer):
    """layers/splitprior.py:7-41: a coupling whose second output half is factored out under `base`.  `forward` / `reverse` are the
    reference's protocol: `forward` scores that half and drops it, `reverse` draws a fresh one.  `split` / `merge` are the same two
    maps with the half handed out and taken back -- what `FlowSequential.encode` / `decode` walk, an exact round trip -- and on the
    device, with a `GaussianPrior` base, one HIP launch each (`ops.finc_split_prior`, `ops.finc_split_prior_merge`: the transform,
    the two half tensors and log p = log-det + the base's score from one pass; no `cat`, no slices, no PyTorch log-prob chain).
    `hip_recorded_merge` (per instance, off by default; `create_model(hip_recorded_merge=True)` sets it): a `merge` that autograd
    records inside `ops.reverse_grad()` is then that one launch as well, with ONE HIP backward (`ops.split_prior_merge`:
    finc_split_prior_merge_backward_f32) in place of `cat`, the coupling's reverse and the `base.log_prob` chain; its sums round
    differently from those lines, which is why it is a switch."""

    #: record `merge` inside `ops.reverse_grad()` as one HIP launch with a HIP backward of its own (see the class docstring)
    hip_recorded_merge = False

    def __init__(self, input_size, distribution, width=512):
        super().__init__()
        assert len(input_size) == 3
        self.n_channels = input_size[0]
        self.transform = Coupling(input_size, width=width)
        self.base = distribution((self.n_channels // 2, input_size[1], input_size[2]))

    def _hip_latent(self, *halves_or_input):
        """Do the split prior's own kernels serve these tensors?  The coupling's conditions, and a base that is exactly the standard
        normal the kernels score (a subclass or another distribution keeps `base.log_prob`)."""
        t = halves_or_input[0]
        return (type(self.base) is GaussianPrior and self.transform._hip_device(t) and tuple(t.shape[2:]) == self.base.size[1:]
                and all(_hip_tensor(h) and h.shape == t.shape and h.device == t.device for h in halves_or_input[1:]))

    def split(self, input, context=None):
        """`forward` with the factored-out half handed back: `(x1, z2, log_p)`, log_p [B] = what `forward` returns as its second value
        (the coupling's log-det plus log p(z2) under the base).  The three paths of `Coupling.forward`: without a graph the net on
        `_raw_inference` and `ops.finc_split_prior`; while autograd records, `_raw_train` and `ops.split_prior_forward` (backward:
        finc_split_prior_backward_f32); the PyTorch lines for everything else -- CPU tensors, fp64, odd channel counts, a base that
        is not exactly `GaussianPrior`.  Under bf16 autocast the net's bf16 output goes to the `_rawbf16_f32` entry points as it
        lies; under fp16 autocast it is upcast, as everywhere in `Coupling`."""
        t, half = self.transform, self.n_channels // 2
        if input.dim() == 4 and input.shape[1] == self.n_channels and self._hip_latent(input):
            if t._hip(input, context):
                x = input.contiguous()
                a, b = t._scale_shift_cached()
                return ops.finc_split_prior(x, t._raw_inference(x, context), a, b)
            if t._hip_train(input, context):
                a, b = t._scale_shift()
                return ops.split_prior_forward(input, t._raw_train(input, context), a, b)
        x, ldj = t(input, context)
        z2 = x[:, half:]
        return x[:, :half], z2, self.base.log_prob(z2) + ldj

    def draw(self, n_samples, context=None, temperature=1.0):
        """The factored-out half as `reverse` draws it, times `temperature` (applied to what `base.sample` returns, so that any base
        with that interface serves; at 1 the draw is handed on untouched)."""
        z2 = self.base.sample(n_samples, context)[0]
        return z2 if temperature == 1 else z2 * temperature

    def merge(self, x1, z2=None, context=None, temperature=1.0, with_log_prob=False):
        """The inverse of `split`: x from the kept half `x1` and the factored-out half `z2` (None: drawn from the base, times
        `temperature`); with `with_log_prob`, `(x, log_p)` with log_p [B] = `split`'s value at x.  Without a graph, on the device: the
        net on `x1` itself and `ops.finc_split_prior_merge` -- no `cat`.  While autograd records (inside `ops.reverse_grad()` that is
        the HIP path of `Coupling.reverse` / `reverse_with_logdet`) and everywhere else: `cat`, the coupling's reverse and
        `base.log_prob`, the lines of `reverse` / `reverse_with_logdet`.  With `hip_recorded_merge` set, a merge recorded inside
        `ops.reverse_grad()` is instead the net on `x1` itself (`_raw_train`) and `ops.split_prior_merge`: one launch, one HIP backward."""
        if z2 is None:
            z2 = self.draw(len(x1), context, temperature)
        t = self.transform
        records = torch.is_grad_enabled() and (z2.requires_grad or t._records_graph(x1, context))
        hip_recorded = records and self.hip_recorded_merge and ops.reverse_grad_enabled()
        if (not records or hip_recorded) and x1.dim() == 4 and x1.shape[1] == self.n_channels // 2 and self._hip_latent(x1, z2):
            if hip_recorded:
                a, b = t._scale_shift()
                return ops.split_prior_merge(x1, z2, t._raw_train(x1, context), a, b, want_log_p=with_log_prob)
            x1, z2 = x1.contiguous(), z2.contiguous()
            a, b = t._scale_shift_cached()
            return ops.finc_split_prior_merge(x1, z2, t._raw_inference(x1, context), a, b, want_log_p=with_log_prob)
        whole = torch.cat([x1, z2], dim=1)
        if not with_log_prob:
            return t.reverse(whole, context)
        out, ldj = t.reverse_with_logdet(whole, context)
        return out, self.base.log_prob(z2) + ldj

    def forward(self, input, context=None):
        x, ldj = self.transform(input, context)
        half = self.n_channels // 2
        return x[:, :half], self.base.log_prob(x[:, half:]) + ldj

    def reverse(self, input, context=None):
        x2, _ = self.base.sample(input.shape[0], context)
        return self.transform.reverse(torch.cat([input, x2], dim=1), context)

    def reverse_with_logdet(self, input, context=None):
        """Mirrors `forward`: the drawn half's density under the base plus the coupling's log-det."""
        x2, _ = self.base.sample(input.shape[0], context)
        out, ldj = self.transform.reverse_with_logdet(torch.cat([input, x2], dim=1), context)
        return out, self.base.log_prob(x2) + ldj

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]


class Gaussianize(_DerivedValues, nn.Module):
    """layers/split.py:24-52 (RealNVP 3.6 / figure 4b): x2 ~ N(m, exp(logs)^2) with (m, logs) the even and odd output channels of
    `net(x1) * exp(log_scale_factor)`, `net` one zero-initialised 3x3 convolution.  Parameter names and shapes are the reference's.
    `forward(x1, x2) -> (z2, logdet)` and `reverse(x1, z2) -> x2` are its PyTorch lines; the helpers below are what `Split` hands to
    the HIP kernels: `raw` = the convolution WITHOUT its bias, and h = a * raw + b with a = exp(log_scale_factor), b = bias * a (the
    convention of `Coupling._scale_shift`).  Under autocast only the convolution runs in the autocast dtype; its output is upcast in
    front of h, in the PyTorch lines and on the HIP path alike."""

    _derived = ("_ab", "_ab_key", "_ab_ready")

    def __init__(self, n_channels):
        super().__init__()
        self.net = nn.Conv2d(n_channels, 2 * n_channels, kernel_size=3, padding=1)
        self.log_scale_factor = nn.Parameter(torch.zeros(2 * n_channels, 1, 1))
        with torch.no_grad():
            self.net.weight.zero_()
            self.net.bias.zero_()

    def _records_graph(self, *tensors):
        return torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in self.parameters()))

    def _scale_shift(self):
        a = torch.exp(self.log_scale_factor).reshape(-1)
        return a, self.net.bias * a

    def _scale_shift_cached(self):
        # once per parameter version, as Coupling._scale_shift_cached (nothing is cached during a stream capture)
        key = ops.version_key(self.log_scale_factor, self.net.bias) + (self.log_scale_factor.device,)
        if getattr(self, "_ab_key", None) == key:
            self._ab_ready.wait(*self._ab)
            return self._ab
        with torch.no_grad():
            a, b = self._scale_shift()
            ab = (a.contiguous(), b.contiguous())
        if not (self.log_scale_factor.is_cuda and ops._capturing()):
            self._ab, self._ab_key, self._ab_ready = ab, key, ops.Ready(self.log_scale_factor.device)
        return ab

    def _raw(self, x1):
        """The convolution without its bias, fp32 whatever autocast made of it (there are no bf16 / fp16 kernels behind it)."""
        raw = F.conv2d(x1, self.net.weight, None, padding=1)
        return raw if raw.dtype == x1.dtype else raw.to(x1.dtype)

    def _raw_inference(self, x1):
        with torch.no_grad():
            return self._raw(x1).contiguous()

    def _mean_logs(self, x1):
        if _autocast_dtype(x1) is None:
            h = self.net(x1) * self.log_scale_factor.exp()                      # layers/split.py:41
        else:
            a, b = self._scale_shift()
            h = self._raw(x1) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        return h[:, 0::2], h[:, 1::2]

    def forward(self, x1, x2):
        m, logs = self._mean_logs(x1)
        return (x2 - m) * torch.exp(-logs), -logs.flatten(start_dim=1).sum(-1)

    def reverse(self, x1, z2):
        return self.reverse_with_logdet(x1, z2)[0]

    def reverse_with_logdet(self, x1, z2):
        """x2 and the FORWARD map's log-det at it, -sum logs (logs depends on x1 only, which both directions share)."""
        m, logs = self._mean_logs(x1)
        return m + z2 * torch.exp(logs), -logs.flatten(start_dim=1).sum(-1)


class Split(FlowLayer):
    """layers/split.py:4-22 as the FlowLayer of fastflow_cifar_multi_gpu.py:77-105: the level boundary of Glow / RealNVP.  The
    second half of the channels is factored out as z2 = (x2 - m) * exp(-logs) and scored under `base`; (m, logs) cost ONE 3x3
    convolution of the kept half, where `SplitPrior` runs a whole coupling net.  The interface is `SplitPrior`'s: `forward` scores
    z2 and drops it, `reverse` draws a fresh one, `split` / `merge` / `draw` hand it out and take it back (`FlowSequential.encode` /
    `decode` / `draw_latents` / `sample(temperature=)`).  On the device, with fp32 tensors and a base that is exactly
    `GaussianPrior`, everything behind the convolution is one HIP launch: `ops.finc_gauss_split` / `ops.finc_gauss_split_merge`
    without a graph, `ops.gauss_split_forward` (backward: finc_gauss_split_backward_f32) while autograd records `split` /
    `forward`.  Everything else -- CPU tensors, float64, another base, a `merge` that autograd records (inside
    `ops.reverse_grad()` too) -- keeps the PyTorch lines, which are differentiable as they are.  The layer takes no part in an
    invertible run (`FlowSequential.invertible_backward` ends one at it, as at a `SplitPrior`).
    `hip_recorded_merge` (per instance, off by default; `create_model(hip_recorded_merge=True)` sets it): a `merge` that autograd
    records inside `ops.reverse_grad()` is then the convolution and ONE launch with ONE HIP backward (`ops.gauss_split_merge`:
    finc_gauss_split_merge_backward_f32) -- `reverse` / `reverse_with_logdet` are `merge` on a draw and follow it."""

    #: record `merge` inside `ops.reverse_grad()` as one HIP launch with a HIP backward of its own (see the class docstring)
    hip_recorded_merge = False

    def __init__(self, input_size, distribution):
        super().__init__()
        assert len(input_size) == 3
        self.n_channels = input_size[0]
        self.gaussianize = Gaussianize(self.n_channels // 2)
        self.base = distribution((self.n_channels // 2, input_size[1], input_size[2]))

    def _hip_latent(self, *halves_or_input):
        """Do the kernels serve these tensors?  fp32 [B,C,H,W] on the device with the parameters beside them, an even channel count
        with a kernel, and a base that is exactly the standard normal the kernels score."""
        t = halves_or_input[0]
        return (type(self.base) is GaussianPrior and _hip_tensor(t) and self.n_channels % 2 == 0
                and ops.coupling_supported(self.n_channels) and tuple(t.shape[2:]) == self.base.size[1:]
                and _params_on_device(t, *self.gaussianize.parameters())
                and all(_hip_tensor(h) and h.shape == t.shape and h.device == t.device for h in halves_or_input[1:]))

    def split(self, input, context=None):
        """`forward` with the factored-out half handed back: `(x1, z2, log_p)`, log_p [B] = the split's log-det, -sum logs, plus
        log p(z2) under the base."""
        g, half = self.gaussianize, self.n_channels // 2
        if input.dim() == 4 and input.shape[1] == self.n_channels and self._hip_latent(input):
            if not g._records_graph(input):
                x = input.contiguous()
                a, b = g._scale_shift_cached()
                return ops.finc_gauss_split(x, g._raw_inference(x[:, :half]), a, b)
            a, b = g._scale_shift()
            return ops.gauss_split_forward(input, g._raw(input[:, :half]), a, b)
        x1 = input[:, :half]
        z2, ldj = g(x1, input[:, half:])
        return x1, z2, self.base.log_prob(z2) + ldj

    def draw(self, n_samples, context=None, temperature=1.0):
        """The factored-out half as `reverse` draws it, times `temperature` (at 1 the draw is handed on untouched)."""
        z2 = self.base.sample(n_samples, context)[0]
        return z2 if temperature == 1 else z2 * temperature

    def merge(self, x1, z2=None, context=None, temperature=1.0, with_log_prob=False):
        """The inverse of `split`: x from the kept half `x1` and the factored-out half `z2` (None: drawn from the base, times
        `temperature`); with `with_log_prob`, `(x, log_p)` with log_p [B] = `split`'s value at x.  Without a graph, on the device: the
        convolution of `x1` and `ops.finc_gauss_split_merge`, which writes the whole x -- no `cat`.  While autograd records, and
        everywhere else: the PyTorch lines -- unless `hip_recorded_merge` is set and the merge is recorded inside
        `ops.reverse_grad()`: then the recorded convolution of `x1` and `ops.gauss_split_merge`, one launch with one HIP backward."""
        if z2 is None:
            z2 = self.draw(len(x1), context, temperature)
        g = self.gaussianize
        records = g._records_graph(x1, z2)
        hip_recorded = records and self.hip_recorded_merge and ops.reverse_grad_enabled()
        if (not records or hip_recorded) and x1.dim() == 4 and x1.shape[1] == self.n_channels // 2 and self._hip_latent(x1, z2):
            if hip_recorded:
                a, b = g._scale_shift()
                return ops.gauss_split_merge(x1, z2, g._raw(x1), a, b, want_log_p=with_log_prob)
            x1, z2 = x1.contiguous(), z2.contiguous()
            a, b = g._scale_shift_cached()
            return ops.finc_gauss_split_merge(x1, z2, g._raw_inference(x1), a, b, want_log_p=with_log_prob)
        x2, ldj = g.reverse_with_logdet(x1, z2)
        x = torch.cat([x1, x2], dim=1)
        return (x, self.base.log_prob(z2) + ldj) if with_log_prob else x

    def forward(self, input, context=None):
        x1, _, log_p = self.split(input, context)
        return x1, log_p

    def reverse(self, input, context=None):
        return self.merge(input, None, context)

    def reverse_with_logdet(self, input, context=None):
        """Mirrors `forward`: the drawn half's density under the base plus the split's log-det at the result."""
        return self.merge(input, None, context, with_log_prob=True)

    def logdet(self, input, context=None):
        return self.forward(input, context)[1]


class Normalization(FlowLayer):
    def __init__(self, translation, scale, learnable=False):
        super().__init__()
        if learnable:
            self.translation = nn.Parameter(torch.Tensor([translation]))
            self.scale = nn.Parameter(torch.Tensor([scale]))
        else:
            self.register_buffer('translation', torch.Tensor([translation]))
            self.register_buffer('scale', torch.Tensor([scale]))

    def forward(self, input, context=None):
        return (input - self.translation) / self.scale, self.logdet(input, context)

    def reverse(self, input, context=None):
        return input * self.scale + self.translation

    def reverse_with_logdet(self, input, context=None):
        out = self.reverse(input, context)
        return out, self.logdet(out, context)

    def logdet(self, input, context=None):
        n, c, h, w = input.shape
        return (-c * h * w * torch.log(self.scale)).expand(n)


class LogitTransform(FlowLayer):
    def forward(self, input, context=None):
        return torch.log(input) - torch.log(1 - input), self.logdet(input, context)

    def reverse(self, input, context=None):
        return torch.sigmoid(input)

    def reverse_with_logdet(self, input, context=None):
        out = self.reverse(input, context)
        return out, self.logdet(out, context)

    def logdet(self, input, context=None):
        return (-torch.log(input) - torch.log(1 - input)).flatten(start_dim=1).sum(-1)


class UniformDistribution(nn.Module):
    """U[0, 1)^size with the interface of layers/distributions/uniform.py:6-37.  The reference registers a buffer `empty` (:14) to
    know its device, so every checkpoint its `create_model` writes holds `0.distribution.empty`: the buffer is kept, under that
    name, and the key sets of the two projects are equal in both directions."""

    def __init__(self, size=None):
        super().__init__()
        self.size = None if size is None else tuple(size)
        self.dim = None if size is None else int(np.prod(size))
        self.register_buffer('empty', torch.zeros(1))

    def forward(self, input, context=None):
        return self.log_prob(input, context)

    def log_prob(self, input, context=None):
        inside = (input >= 0) & (input <= 1.)
        return torch.where(inside, torch.zeros_like(input), torch.full_like(input, -1e30)).flatten(start_dim=1).sum(-1)

    def sample(self, n_samples, context=None):
        return torch.rand((n_samples, *self.size), device=self.empty.device), 0.


class Dequantization(FlowLayer):
    """Uniform dequantisation (layers/dequantize.py + distributions/uniform.py): forward adds U[0,1) noise.  `distribution` is the
    reference's child module (`Dequantization(UniformDistribution(size))` there, layers/dequantize.py:7-10; a module handed in is
    kept as it is) and carries its `empty` buffer into the state dict.  The noise itself is drawn on the input's device, in the
    input's shape, whatever `size` says."""

    def __init__(self, size=None):
        super().__init__()
        if isinstance(size, nn.Module):
            self.distribution, size = size, getattr(size, "size", None)
        else:
            self.distribution = UniformDistribution(size)
        self.size = size

    def forward(self, input, context=None):
        return input + torch.rand_like(input.float()), input.new_zeros(len(input), dtype=torch.float32)

    def reverse(self, input, context=None):
        return input.floor()

    def reverse_with_logdet(self, input, context=None):
        """`floor` and zeros, as `forward` reports zero: the density a sampler carries through this layer is the CONTINUOUS one of
        the variable in front of the floor, not a probability mass of the integer result."""
        return input.floor(), input.new_zeros(len(input), dtype=torch.float32)

    def logdet(self, input, context=None):
        raise NotImplementedError


def create_model(num_blocks=3, block_size=32, actnorm=False, split_prior=False, image_size=(3, 32, 32),
                 preprocess=True, coupling_width=512, gaussianize_split=False, hip_recorded_merge=False, lu_conv1x1=False):
    """fastflow/fastflow_cifar.py:35-63: Squeeze -> [FastFlowUnit, (ActNorm), Conv1x1, Coupling] x block_size
    (-> SplitPrior) per block, under a standard-normal base.  `gaussianize_split` (with `split_prior`): the level boundary is the
    Gaussianized `Split` instead of a `SplitPrior`, the switch of fastflow_cifar_multi_gpu.py:264-265.  `hip_recorded_merge`: the
    boundaries record their `merge` inside `ops.reverse_grad()` on the HIP kernels (`SplitPrior.hip_recorded_merge`).  `lu_conv1x1`:
    every 1x1 convolution in Glow's PLU parametrisation (`Conv1x1LU`: the same matrices from the same seed, no factorisation per call)."""
    size = tuple(image_size)
    layers = []
    if preprocess:
        alpha = 1e-6
        layers += [Dequantization(size), Normalization(translation=0, scale=256),
                   Normalization(translation=-alpha, scale=1 / (1 - 2 * alpha)), LogitTransform()]
    for level in range(num_blocks):
        layers.append(Squeeze())
        size = (size[0] * 4, size[1] // 2, size[2] // 2)
        for _ in range(block_size):
            layers.append(FastFlowUnit(size[0], size[0], (3, 3)))
            if actnorm:
                layers.append(ActNorm(size[0]))
            layers.append(Conv1x1LU(size[0]) if lu_conv1x1 else Conv1x1(size[0]))
            layers.append(Coupling(size, width=coupling_width))
        if split_prior and level < num_blocks - 1:
            layers.append(Split(size, GaussianPrior) if gaussianize_split else SplitPrior(size, GaussianPrior, width=coupling_width))
            if hip_recorded_merge:
                layers[-1].hip_recorded_merge = True
            size = (size[0] // 2, size[1], size[2])
    return FlowSequential(GaussianPrior(size), *layers)
