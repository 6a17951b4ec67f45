"""Host side of sampling with the log-density (finc_coupling_reverse_logdet_f32, finc_coupling_reverse_logdet_backward_f32;
include/finc.h): the exported symbols and the fifth ABI version gate, argument refusals before any HIP call, the new
kernels' register allocation, and `reverse_with_logdet` of every layer / `FlowSequential.sample_with_log_prob` on CPU tensors -- no
GPU needed, the library built.

Bars: 1e-5 in helpers.rel_err against float64 (the bar of tests/test_gpu_reverse_backward.py), 5e-5 for the whole chain (its
CHAIN_TOL).  Every Conv2dZero is randomised (0.05 randn: at its zero initialisation s == 0 and a log-det of zero proves nothing), ActNorm
has a non-zero log_scale, Conv1x1 a W that is not orthogonal; each comparison first asserts that the log-det is not small."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library, rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("finc_coupling_reverse_logdet_f32", "finc_coupling_reverse_logdet_backward_f32")
TOL = 1e-5
CHAIN_TOL = 5e-5


def test_new_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    from fincflow_amd import ops
    for name in ("finc_coupling_reverse_logdet", "finc_coupling_reverse_logdet_backward", "coupling_reverse_logdet"):
        assert callable(getattr(ops, name)), name


def test_version_is_109_and_a_108_library_is_refused_by_name(tmp_path):
    assert _lib.lib().finc_version() >= _lib.SAMPLE_LOGDET_ABI_VERSION == 109
    assert _lib.ABI_VERSION == 104 and _lib.ACTNORM_ABI_VERSION == 105 and _lib.INVERSE_BACKWARD_ABI_VERSION == 107
    assert _lib.REVERSE_BACKWARD_ABI_VERSION == 108
    out = load_stub_library(tmp_path, 108)
    assert "= 108" in out and "109" in out, out
    for name in NEW_SYMBOLS:
        assert name in out, out


def test_reverse_logdet_status_codes_without_touching_the_gpu():
    """NULL (logdet included) -> 1, bad dims / y == raw -> 2, alignment below 4 bytes -> 7, odd C -> 3, workspace -> 4, in that order
    of precedence, with fake pointers: nothing is launched."""
    L = _lib.lib()
    x, raw, a, b, y, ld, ws = _p(0x1000), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000), _p(0x6000), _p(0x10000)
    big = 1 << 40
    f = L.finc_coupling_reverse_logdet_f32
    for k in range(6):                                                       # x, raw, a, b, y AND logdet are required
        args = [x, raw, a, b, y, ld]
        args[k] = None
        assert f(*args, 2, 12, 64, ws, big, None) == 1, k
    assert f(x, raw, a, b, y, None, 0, 12, 64, ws, big, None) == 1                                 # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64), (1 << 20, 4096, 1 << 20)):
        assert f(x, raw, a, b, y, ld, B, C, HW, ws, big, None) == 2, (B, C, HW)
    assert f(x, raw, a, b, raw, ld, 2, 12, 64, ws, big, None) == 2                                 # y == raw
    assert f(_p(0x1002), raw, a, b, raw, ld, 2, 12, 64, ws, big, None) == 2                        # (... before the alignment)
    assert f(_p(0x1002), raw, a, b, y, ld, 0, 12, 64, ws, big, None) == 2                          # (dims before the alignment)
    assert f(_p(0x1002), raw, a, b, y, ld, 2, 12, 64, ws, big, None) == 7
    assert f(x, _p(0x2001), a, b, y, ld, 2, 12, 64, ws, big, None) == 7
    assert f(x, raw, a, b, y, _p(0x6003), 2, 12, 64, ws, big, None) == 7
    assert f(x, raw, a, b, _p(0x5002), ld, 2, 12, 64, None, 0, None) == 7                          # (alignment before the workspace)
    assert f(_p(0x1002), raw, a, b, y, ld, 2, 13, 64, ws, big, None) == 7                          # (alignment before the channel count)
    for C in (13, 7, 1):
        assert f(x, raw, a, b, y, ld, 2, C, 64, ws, big, None) == 3, C
        assert f(x, raw, a, b, y, ld, 2, C, 64, None, 0, None) == 3, C                             # (... before the workspace)
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(x, raw, a, b, y, ld, 2, 12, 64, None, big, None) == 4                                 # the workspace is always needed
    assert f(x, raw, a, b, y, ld, 2, 12, 64, ws, need - 1, None) == 4
    assert f(x, raw, a, b, y, ld, 2, 12, 64, ws, 0, None) == 4
    assert f(x, raw, a, b, y, ld, 2, 12, 64, _p(0x10002), big, None) == 4
    assert f(x, raw, a, b, x, ld, 2, 12, 64, ws, need - 1, None) == 4                              # y == x passes every earlier check


def test_reverse_logdet_backward_status_codes_without_touching_the_gpu():
    """As finc_coupling_reverse_backward_f32, with grad_logdet optional (NULL = zeros) but aligned when given."""
    L = _lib.lib()
    gy, gl, y, raw, a, b = _p(0x1000), _p(0x1800), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000)
    gx, gr, ga, gb, ws = _p(0x6000), _p(0x7000), _p(0x8000), _p(0x9000), _p(0x10000)
    big = 1 << 40
    f = L.finc_coupling_reverse_logdet_backward_f32
    for k in (0, 2, 3, 4, 5):                                                # grad_y, y, raw, a, b are required; grad_logdet is not
        args = [gy, gl, y, raw, a, b]
        args[k] = None
        assert f(*args, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 1, k
    assert f(gy, gl, y, raw, a, b, None, None, None, None, 2, 12, 64, ws, big, None) == 1          # nothing asked for
    assert f(None, gl, y, raw, a, b, gx, gr, ga, gb, 0, 12, 64, ws, big, None) == 1                # (NULL comes before the dims)
    for B, C, HW in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64), (1 << 20, 4096, 1 << 20)):
        assert f(gy, gl, y, raw, a, b, gx, gr, ga, gb, B, C, HW, ws, big, None) == 2, (B, C, HW)
        assert f(gy, None, y, raw, a, b, gx, gr, ga, gb, B, C, HW, ws, big, None) == 2, (B, C, HW)
    for alias in (gy, y, raw):
        assert f(gy, gl, y, raw, a, b, alias, gr, ga, gb, 2, 12, 64, ws, big, None) == 2          # grad_x on an input
        assert f(gy, gl, y, raw, a, b, gx, alias, ga, gb, 2, 12, 64, ws, big, None) == 2          # grad_raw on an input
    assert f(gy, gl, y, raw, a, b, gx, gx, ga, gb, 2, 12, 64, ws, big, None) == 2                  # grad_raw == grad_x
    assert f(_p(0x1002), gl, y, raw, a, b, gx, gr, ga, gb, 0, 12, 64, ws, big, None) == 2          # (dims come before the alignment)
    assert f(_p(0x1002), gl, y, raw, a, b, y, gr, ga, gb, 2, 12, 64, ws, big, None) == 2           # (aliasing comes before the alignment)
    assert f(_p(0x1002), gl, y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, _p(0x1801), y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 7          # grad_logdet, when given
    assert f(gy, gl, _p(0x2001), raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, gl, y, raw, a, b, gx, gr, _p(0x8003), gb, 2, 12, 64, ws, big, None) == 7
    assert f(gy, gl, y, raw, a, b, gx, _p(0x7002), ga, gb, 2, 12, 64, None, 0, None) == 7          # (alignment before the workspace)
    assert f(_p(0x1002), gl, y, raw, a, b, gx, gr, ga, gb, 2, 13, 64, ws, big, None) == 7          # (alignment before the channel count)
    for C in (13, 7, 1):
        assert f(gy, gl, y, raw, a, b, gx, gr, ga, gb, 2, C, 64, ws, big, None) == 3, C
        assert f(gy, None, y, raw, a, b, gx, gr, ga, gb, 2, C, 64, None, 0, None) == 3, C          # (... before the workspace)
        assert f(gy, gl, y, raw, a, b, gx, None, None, None, 2, C, 64, None, 0, None) == 3, C
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(gy, gl, y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, None, big, None) == 4
    assert f(gy, gl, y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, ws, need - 1, None) == 4
    assert f(gy, None, y, raw, a, b, None, None, ga, None, 2, 12, 64, ws, 0, None) == 4
    assert f(gy, gl, y, raw, a, b, None, None, None, gb, 2, 12, 64, None, 0, None) == 4
    assert f(gy, gl, y, raw, a, b, gx, gr, ga, gb, 2, 12, 64, _p(0x10002), big, None) == 4


def test_the_forward_workspace_bound_covers_the_reverse_partials():
    """The reverse launch with its log-det writes B x P partials on the forward direction's grid, P <= ceil(half * HW / 256) and
    B * P < 2048 + B (finc_coupling.h: cpl_parts): finc_coupling_workspace_bytes holds at least that many floats."""
    L = _lib.lib()
    for B, C, HW in ((1, 2, 1), (3, 4, 15), (2, 8, 16), (2, 6, 1600), (256, 96, 4096), (5000, 12, 64), (7, 512, 333)):
        half = C // 2
        parts = min(-(-half * HW // 256), -(-2048 // B))
        assert L.finc_coupling_workspace_bytes(B, C, HW) >= 4 * B * max(parts, 1), (B, C, HW)


def test_new_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    for name in ("finc_coupling_rev_logdet_kernel", "finc_coupling_rev_bwd_kernel"):
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == 2, (name, sorted(ks))                             # the 16-byte and the dword form
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layers on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def _randomise(m, seed=11):
    """Conv2dZero's weight, bias and logs at 0.05 randn (issue: never at their zero initialisation), the rest of a net as the other
    host tests fill it; ActNorm: log_scale 0.3 randn, initialised; Conv1x1: W = orthogonal + 0.3 randn (|log det| > 0.1)."""
    from fincflow_amd import glow
    g = torch.Generator().manual_seed(seed)
    r = lambda shape, s: torch.randn(shape, generator=g) * s
    with torch.no_grad():
        for sub in m.modules():
            if isinstance(sub, glow.Coupling):
                for p in sub.net.parameters():
                    p.copy_(r(p.shape, 0.05))
            elif isinstance(sub, glow.ActNorm):
                sub.log_scale.copy_(r(sub.log_scale.shape, 0.3))
                sub.translation.copy_(r(sub.translation.shape, 1.0))
                sub.mark_initialized()
            elif isinstance(sub, glow.Conv1x1):
                sub.W.add_(r(sub.W.shape, 0.3))
                assert abs(float(torch.slogdet(sub.W)[1])) > 0.1
    return m


def _unit_forward(u, x):
    """FastFlowUnit restated on PyTorch (fastflow.py:38-55: four one-corner-padded convolutions on the stored, flipped weights)."""
    convs = (u.conv_tl, u.conv_tr, u.conv_bl, u.conv_br)
    return torch.cat([F.conv2d(F.pad(c, m.pad), m.conv.weight.to(c.dtype)) for m, c in zip(convs, torch.chunk(x, 4, dim=1))], dim=1)


def _unit_inverse(u, z):
    """The inverse of that by a dense float64 solve (small maps only): column k of the matrix is the forward of basis vector k."""
    n = z[0].numel()
    eye = torch.eye(n, dtype=torch.float64).view(n, *z.shape[1:])
    mat = _unit_forward(u, eye).reshape(n, n).t()
    return torch.linalg.solve(mat, z.double().reshape(len(z), n).t()).t().reshape(z.shape).to(z.dtype)


@pytest.fixture
def host_unit(monkeypatch):
    """FastFlowUnit has no CPU path: for the container logic its cache's launches are replaced by the restatement above."""
    from fincflow_amd import FastFlowUnit, ops
    units = {}

    def owner(weights):
        return units[weights[0].data_ptr()]

    def register(u):
        units[u.conv_tl.conv.weight.data_ptr()] = u
        return u
    monkeypatch.setattr(ops.PackedWeights, "forward", lambda self, x, weights, G, orient, **kw: _unit_forward(owner(weights), x))
    monkeypatch.setattr(ops.PackedWeights, "inverse", lambda self, z, weights, G, orient, **kw: _unit_inverse(owner(weights), z))
    monkeypatch.setattr(ops.PackedWeights, "inverse_affine", lambda self, *a, **kw: None)     # (the folds step aside, as for a
    monkeypatch.setattr(ops.PackedWeights, "forward_affine", lambda self, *a, **kw: None)     # shape without the fused kernel)
    return register


def _layers(dtype, host_unit):
    """(name, layer, input of `reverse`, context)."""
    from fincflow_amd import FastFlowUnit, glow
    torch.manual_seed(3)
    np.random.seed(3)
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).to(dtype)
    return [("unit", host_unit(FastFlowUnit(12, 12, (3, 3)).to(dtype)), r(3, 12, 3, 2), None),
            ("actnorm", _randomise(glow.ActNorm(12)).to(dtype), r(3, 12, 5, 3), None),
            ("conv1x1", _randomise(glow.Conv1x1(12)).to(dtype), r(3, 12, 5, 3), None),
            ("coupling", _randomise(glow.Coupling((12, 5, 3), width=16)).to(dtype), r(3, 12, 5, 3), None),
            ("coupling_context", _randomise(glow.Coupling((12, 5, 3), width=16, n_context=3)).to(dtype), r(3, 12, 5, 3), r(3, 3, 5, 3)),
            ("squeeze", glow.Squeeze(), r(3, 12, 5, 3), None),
            ("normalization", glow.Normalization(translation=-0.25, scale=3.0).to(dtype), r(3, 3, 4, 4), None),
            ("logit", glow.LogitTransform(), r(3, 3, 4, 4), None)]


ZERO_LOGDET = ("unit", "squeeze")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
def test_every_layer_on_cpu_tensors(dtype, host_unit):
    """`out` is `reverse(input)` bit for bit, `logdet` [B] is `forward(out)[1]` within the bar (float64: of the float64 layer)."""
    for name, m, x, ctx in _layers(dtype, host_unit):
        with torch.no_grad():
            want = m.reverse(x, ctx)
            out, logdet = m.reverse_with_logdet(x, ctx)
            m64 = m.double()
            if name == "unit":
                host_unit(m64)                                               # (its weights moved)
            ref = m64.forward(out.double(), None if ctx is None else ctx.double())[1]
        ref = torch.as_tensor(ref, dtype=torch.float64).expand(len(x))
        assert torch.equal(out, want), name
        assert logdet.shape == (len(x),), (name, logdet.shape)
        if name in ZERO_LOGDET:
            assert not bool(logdet.any()) and not bool(ref.any()), name
            continue
        assert float(logdet.abs().max()) > 0.1, (name, logdet)
        err = rel_err(logdet.numpy(), ref.numpy())
        print(name, dtype, "logdet against forward(out)[1] in float64: %.3e" % err)
        assert err <= TOL, (name, err)


def test_dequantization_floors_and_reports_zero():
    from fincflow_amd import glow
    x = 7.0 * torch.rand(3, 3, 4, 4)
    out, logdet = glow.Dequantization().reverse_with_logdet(x)
    assert torch.equal(out, x.floor()) and logdet.shape == (3,) and not bool(logdet.any())


def test_padded_conv_and_cinc_unit_report_zero(host_unit, monkeypatch):
    from fincflow_amd import CINCFlowUnit, PaddedConv2d, ops
    x = torch.randn(2, 4, 3, 3)
    monkeypatch.setattr(ops.PackedWeights, "inverse", lambda self, z, weights, G, orient, **kw: z + 1.0)
    for m in (PaddedConv2d(4, 4, (3, 3)), CINCFlowUnit(4, 4, (3, 3))):
        out, logdet = m.reverse_with_logdet(x)
        assert torch.equal(out, x + 1.0) and logdet.shape == (2,) and not bool(logdet.any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
def test_split_prior_against_forward_on_the_returned_tensor(dtype):
    from fincflow_amd import glow
    m = _randomise(glow.SplitPrior((12, 5, 3), glow.GaussianPrior, width=16)).to(dtype)
    x = torch.randn(3, 6, 5, 3, generator=torch.Generator().manual_seed(2)).to(dtype)
    with torch.no_grad():
        torch.manual_seed(9)
        want = m.reverse(x)
        torch.manual_seed(9)
        out, logdet = m.reverse_with_logdet(x)
        kept, ref = m.double().forward(out.double())
    assert torch.equal(out, want) and logdet.shape == (3,)
    assert rel_err(kept.numpy(), x.double().numpy()) <= TOL                  # forward keeps the half that `reverse` was given
    ldj = m.transform.forward(out.double())[1]
    assert float(ldj.detach().abs().max()) > 0.1, ldj                                 # the coupling's share alone is not small
    err = rel_err(logdet.numpy(), ref.numpy())
    print("split prior", dtype, "%.3e" % err)
    assert err <= TOL, err


def test_conv1x1_caches_its_log_det_per_weight_version(monkeypatch):
    """Nothing recorded: one `slogdet` per weight version (no LU factorisation in a sampling pass); recording: `slogdet` is in the
    graph and W gets its gradient."""
    from fincflow_amd import glow
    m = _randomise(glow.Conv1x1(12))
    calls = []
    real = torch.slogdet
    monkeypatch.setattr(torch, "slogdet", lambda w: calls.append(1) or real(w))
    x = torch.randn(2, 12, 4, 4)
    with torch.no_grad():
        first = m.reverse_with_logdet(x)[1]
        again = m.reverse_with_logdet(x)[1]
        assert len(calls) == 1 and torch.equal(first, again)
        m.W.mul_(1.5)
        moved = m.reverse_with_logdet(x)[1]
    assert len(calls) == 2
    assert rel_err(moved.numpy(), (first + 16 * 12 * np.log(1.5)).numpy()) <= TOL
    out, logdet = m.reverse_with_logdet(x)                                   # grad enabled, W requires grad
    assert len(calls) == 3 and logdet.requires_grad
    logdet.sum().backward()
    assert rel_err(m.W.grad.numpy(), (2 * 16 * torch.inverse(m.W.detach().double()).t()).numpy()) <= TOL


def test_sample_with_log_prob_on_a_cpu_stack(host_unit):
    """[Squeeze, FastFlowUnit, ActNorm, Conv1x1, Coupling] at (3, 4, 4): log_q of the one reverse pass against `log_prob(x)` of the
    float64 model, and the same x as `sample` from the same seed."""
    from fincflow_amd import FastFlowUnit, FlowSequential, glow
    torch.manual_seed(4)
    np.random.seed(4)
    unit = host_unit(FastFlowUnit(12, 12, (3, 3)))
    layers = [glow.Squeeze(), unit, glow.ActNorm(12), glow.Conv1x1(12), glow.Coupling((12, 2, 2), width=16)]
    model = _randomise(FlowSequential(glow.GaussianPrior((12, 2, 2)), *layers))
    torch.manual_seed(6)
    x, log_q = model.sample_with_log_prob(5)
    assert x.shape == (5, 3, 4, 4) and log_q.shape == (5,) and not x.requires_grad and not log_q.requires_grad
    torch.manual_seed(6)
    with torch.no_grad():
        x_plain, _ = model.sample(5)
    assert torch.equal(x, x_plain)
    torch.manual_seed(6)
    z, _ = model.base_distribution.sample(5)
    logdet = log_q - model.base_distribution.log_prob(z)
    assert float(logdet.abs().max()) > 0.1, logdet
    model.double()
    host_unit(unit)                                                          # (its weights moved)
    with torch.no_grad():
        ref = model.log_prob(x.double())
    err = rel_err(log_q.numpy(), ref.numpy())
    print("cpu stack: log_q against log_prob(x) in float64: %.3e" % err)
    assert err <= CHAIN_TOL, err


def test_rsample_with_log_prob_on_cpu_layers_is_attached():
    """Without a unit (it has no CPU path) the recorded chain runs on PyTorch's lines: both results are attached, and the gradient of
    a reverse-KL style loss reaches every parameter."""
    from fincflow_amd import FlowSequential, glow
    torch.manual_seed(4)
    np.random.seed(4)
    layers = [glow.Squeeze(), glow.ActNorm(12), glow.Conv1x1(12), glow.Coupling((12, 2, 2), width=16)]
    model = _randomise(FlowSequential(glow.GaussianPrior((12, 2, 2)), *layers))
    torch.manual_seed(6)
    x, log_q = model.rsample_with_log_prob(5)
    assert x.requires_grad and log_q.requires_grad and log_q.shape == (5,)
    (log_q - x.square().flatten(1).sum(1)).mean().backward()
    with torch.no_grad():
        ref = model.double().log_prob(x.detach().double())
    assert rel_err(log_q.detach().numpy(), ref.numpy()) <= CHAIN_TOL
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
