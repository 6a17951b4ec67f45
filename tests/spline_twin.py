"""Helpers of tests/test_gpu_spline.py (not collected): layers and knot tables at unit-scale parameters, the float64 / float32 CPU
references of the kernels on a given table, the stack the GPU test walks, and the judge that holds every comparison to
max(1e-5, 2 * e_ref), e_ref the error of the layer's own PyTorch lines in float32 on the CPU against the same float64 values.

`flow_twin.twin_of` needs no entry for the layer: a deep copy of it starts without its cached table, and on CPU tensors the layer
runs its PyTorch lines, which tests/test_spline_host.py holds to the recording of the reference."""
import numpy as np
import torch

import flow_twin
from helpers import report

BAR = 1e-5


def unit_scale_layer(input_size, K, tail_bound, individual, seed, scale=1.0):
    """glow.SplineActivation with `scale` * randn parameters (the constructor's 0.01 * randn is the identity to four digits)."""
    from fincflow_amd import glow
    m = glow.SplineActivation(input_size, n_bins=K, tail_bound=tail_bound, individual_weights=individual)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(scale * torch.randn(p.shape, generator=gen))
    return m


def table_of(m):
    """The layer's knot table [3 (K + 1), P] in fp32, detached: what the kernels read."""
    with torch.no_grad():
        return m._compose().clone()


def lines_on_table(v, table, input_size, tail_bound, inverse):
    """The layer's written-out lines on a given table (any dtype; differentiable in both): (out, logdet [B])."""
    from fincflow_amd import glow
    K, P = table.shape[0] // 3 - 1, table.shape[1]
    shape = (K + 1,) if P == 1 else (1, *input_size, K + 1)
    cw, ch, d = (table[a * (K + 1):(a + 1) * (K + 1)].t().reshape(shape) for a in range(3))
    out, lad = glow.rq_spline_lines(v, cw, ch, d, tail_bound, inverse)
    return out, lad.flatten(1).sum(-1)


def inputs(shape, tail_bound, seed, table=None):
    """0.6 * tail_bound * randn with image 0 holding +-tail_bound, 0, +-1.2 tail_bound and a NaN-free spread over the range."""
    gen = torch.Generator().manual_seed(seed)
    x = 0.6 * tail_bound * torch.randn(shape, generator=gen)
    flat = x.view(shape[0], -1)
    flat[0, :5] = torch.tensor([tail_bound, -tail_bound, 0.0, 1.2 * tail_bound, -1.2 * tail_bound])
    n = flat.shape[1] - 5
    flat[0, 5:] = torch.linspace(-0.999 * tail_bound, 0.999 * tail_bound, n)
    return x


def error(got, want):
    return flow_twin.error(got, want)


def judge(tag, names, got, want, yard, asserting=True, **fields):
    """Every tensor of `got` (the HIP result) against `want` (float64) under max(1e-5, 2 * e_ref), e_ref = `yard` (the fp32 lines on
    the CPU) against `want`; one line per call in the parity report (kind `spline`), every figure printed before it is asserted.
    `asserting=False`: a figure that is reported only (the line says so)."""
    errs = {n: error(g, w) for n, g, w in zip(names, got, want)}
    refs = {n: error(y, w) for n, y, w in zip(names, yard, want)}
    bars = {n: max(BAR, 2 * refs[n]) for n in names}
    report("spline", case=tag, hip=errs, e_ref=refs, bar=bars if asserting else None, reported_only=not asserting, **fields)
    print("spline %s %s: " % (tag, fields or "") + ", ".join("%s HIP %.2e e_ref %.2e" % (n, errs[n], refs[n]) for n in names))
    over = {n: (errs[n], bars[n]) for n in names if not errs[n] <= bars[n]}
    assert not (asserting and over), (tag, fields, over)
    return errs


def stack(seed=1, scale=0.3):
    """[FastFlowUnit, SplineActivation, ActNorm, Conv1x1, Coupling] x 2 with a Squeeze in front of each and a SplitPrior between, on
    3 x 8 x 8 images; the splines one with individual and one with shared weights, their parameters `scale` * randn.  The views
    are asserted at 0.3, not at the unit scale of the kernel and module tests: there a bin's slope h / w can spread over two orders
    of magnitude (a softmax of randn over five bins for the widths, another for the heights), the inverse of a flat bin multiplies
    every rounding in front of it by the reciprocal, and two such layers with couplings between them put the float32 CPU lines
    themselves 2.3e-3 off float64 on `decode` -- a figure that is one ill-conditioned element's, which a differently ordered fp32
    chain does not reproduce within a factor of 2 (the device came out at 5.9e-3).  At 0.3 the slopes stay within e^(+-1) or so and
    a comparison of the chains means something.  The unit-scale stack stays in the suite
    (test_unit_scale_stack_layer_by_layer): its `decode` is reported beside the CPU's figure without an assertion, and each of
    its spline layers is asserted on the float64 twin's own input to that layer, where no earlier layer's rounding is amplified."""
    from fincflow_amd import FastFlowUnit, FlowSequential, glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    layers, size = [], (3, 8, 8)
    for level, individual in enumerate((True, False)):
        layers.append(glow.Squeeze())
        size = (size[0] * 4, size[1] // 2, size[2] // 2)
        layers += [FastFlowUnit(size[0], size[0], (3, 3)), unit_scale_layer(size, 5, 4.0, individual, seed + level, scale=scale),
                   glow.ActNorm(size[0]), glow.Conv1x1(size[0]), glow.Coupling(size, width=16)]
        if level == 0:
            layers.append(glow.SplitPrior(size, glow.GaussianPrior, width=16))
            size = (size[0] // 2, size[1], size[2])
    model = FlowSequential(glow.GaussianPrior(size), *layers)
    return flow_twin.randomise(model, seed=seed, actnorm=True)
