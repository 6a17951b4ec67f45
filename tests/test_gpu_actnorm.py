"""ActNorm on its HIP kernels (finc_actnorm_f32, finc_actnorm_backward_f32, finc_actnorm_init_f32) and glow.ActNorm on them.

Reference everywhere: the reference-made fixtures (tests/golden/make_golden_actnorm.py), and for the larger shapes the formulas of
include/finc.h (layers/actnorm.py:17-65) in float64 on the CPU, autograd for gradients.  Bar: 1e-5 in helpers.rel_err, the
project's bar for every fp32-against-fp64 parity and backward test.  PyTorch's own fp32 mean / log(std + 1e-8) on six shapes
including the offset-1000 case is within 5.0e-7 / 1.2e-7 of float64, so the bar leaves a factor of twenty over what fp32 arithmetic
in a sound order does; the one-pass sum(x^2) - sum(x)^2 / n variance misses it by six orders of magnitude.  Every case appends its
achieved errors to the parity report (helpers.report).
"""
import copy
import itertools
import warnings

import numpy as np
import pytest
import torch

from actnorm_cases import BIG, BIG_IMAGES, CASES, inputs
from helpers import STACK_INPUT, fill_stack_parameters, golden, offset_view, rel_err, report

pytestmark = pytest.mark.gpu

TOL = 1e-5

SHAPES = [(128, 12, 16, 16), (128, 24, 8, 8), (128, 48, 4, 4), (3, 96, 20, 24), (2, 4, 7, 7), (5, 1, 1, 1), (8, 96, 32, 32), (2, 192, 9, 8),
          (16, 12, 64, 64), (2, 16, 5, 3), (2, 513, 3, 3)]
assert all(s[0] * s[2] * s[3] >= 2 for s in SHAPES)                  # every shape takes part in the init test: none is left out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def case(shape):
    """x, log_scale, translation, grad_y, grad_logdet (fp32, CPU)."""
    B, C, H, W = shape
    torch.manual_seed(sum(shape))
    x = torch.randn(B, C, H, W) * (0.5 + torch.rand(C)).view(1, C, 1, 1) + torch.randn(C).view(1, C, 1, 1)
    gy = torch.randn(B, C, H, W)
    gl = torch.randn(B)
    return x, 0.3 * torch.randn(C), torch.randn(C), gy, gl


def ref_transform(x, ls, t, direction):
    """float64: (y, logdet) of the forward direction, y of the reverse."""
    s, tr = ls.view(1, -1, 1, 1), t.view(1, -1, 1, 1)
    if direction > 0:
        return (x - tr) * torch.exp(-s), -ls.sum().expand(x.shape[0]) * (x.shape[2] * x.shape[3])
    return x * torch.exp(s) + tr


def ref_gradients(x, ls, t, gy, gl):
    """float64 autograd of sum(y * gy) + sum(logdet * gl) with respect to x, log_scale, translation."""
    leaves = [v.double().requires_grad_(True) for v in (x, ls, t)]
    y, ld = ref_transform(*leaves, 1)
    loss = (y * gy.double()).sum()
    if gl is not None:
        loss = loss + (ld * gl.double()).sum()
    loss.backward()
    return [v.grad.numpy() for v in leaves]


def fixture_case(name):
    g = golden(name)
    x, gy, gl = (torch.from_numpy(a) for a in inputs(name))
    keep = (lambda a: a[list(BIG_IMAGES)]) if name == BIG else (lambda a: a)
    return g, x, gy, gl, keep


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2: the transform
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_logdet_reverse_and_round_trip(shape, dev):
    from fincflow_amd import ops
    x, ls, t, _, _ = case(shape)
    y_ref, ld_ref = ref_transform(x.double(), ls.double(), t.double(), 1)
    r_ref = ref_transform(x.double(), ls.double(), t.double(), -1)
    xd, lsd, td = x.to(dev), ls.to(dev), t.to(dev)
    y, ld = ops.finc_actnorm(xd, lsd, td, 1, True)
    y_plain, none = ops.finc_actnorm(xd, lsd, td, 1, False)
    r, none2 = ops.finc_actnorm(xd, lsd, td, -1, True)
    back, _ = ops.finc_actnorm(y, lsd, td, -1)
    torch.cuda.synchronize()
    assert none is None and none2 is None and ld.shape == (shape[0],)
    assert torch.equal(y, y_plain)                                   # the log-det is a by-product: the same y without it
    assert torch.equal(xd.cpu(), x)
    errs = {"forward": rel_err(y.cpu().numpy(), y_ref.numpy()), "logdet": rel_err(ld.cpu().numpy(), ld_ref.numpy()),
            "reverse": rel_err(r.cpu().numpy(), r_ref.numpy()), "round_trip": rel_err(back.cpu().numpy(), x.double().numpy())}
    print("actnorm_transform", shape, errs)
    report("actnorm_transform", shape=list(shape), **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)


def fixture_parameters(g, dev):
    """The fixture's float64 parameters and what the kernels get of them: the same numbers rounded to fp32, once.

    The kernel's inputs are fp32, the fixture's `out` and gradients were made from float64 parameters.  On the cancellation case that
    rounding alone moves the exact result by more than the bar: a translation near 1000 is off by up to 3e-5 in fp32, which a standard
    deviation of 0.01 turns into 3e-3 in y (1e-3 of max |y|) whatever computes it.  So, as tests/test_gpu_coupling.py does for its `a`,
    `b`, the float64 reference starts from the numbers the kernel starts from; the restated formula is first pinned to the reference's
    own arrays with the float64 parameters, at 1e-12."""
    ls64, t64 = torch.from_numpy(g["log_scale"]), torch.from_numpy(g["translation"])
    ls32, t32 = ls64.float(), t64.float()
    return ls64, t64, ls32, t32, ls32.to(dev), t32.to(dev)


@pytest.mark.parametrize("name", sorted(CASES))
def test_transform_against_the_reference_fixtures(name, dev):
    from fincflow_amd import ops
    g, x, _, _, keep = fixture_case(name)
    ls64, t64, ls32, t32, ls, t = fixture_parameters(g, dev)
    out64, ldj64 = ref_transform(x.double(), ls64, t64, 1)
    assert rel_err(keep(out64.numpy()), g["out"]) <= 1e-12 and rel_err(ldj64.numpy(), g["ldj"]) <= 1e-12
    assert rel_err(keep(ref_transform(out64, ls64, t64, -1).numpy()), g["rev"]) <= 1e-12
    y_ref, ld_ref = ref_transform(x.double(), ls32.double(), t32.double(), 1)
    y, ld = ops.finc_actnorm(x.to(dev), ls, t, 1, True)
    # reverse(out) of the fixture starts from the float64 `out`; here it starts from the device's y
    r, _ = ops.finc_actnorm(y, ls, t, -1)
    errs = {"forward": rel_err(y.cpu().numpy(), y_ref.numpy()), "logdet": rel_err(ld.cpu().numpy(), ld_ref.numpy()),
            "logdet_vs_fixture": rel_err(ld.cpu().numpy(), g["ldj"]), "reverse": rel_err(keep(r.cpu().numpy()), g["rev"]),
            "forward_vs_fixture": rel_err(keep(y.cpu().numpy()), g["out"])}
    print("actnorm_fixture_transform", name, errs)
    report("actnorm_fixture_transform", case=name, **errs)
    for n, e in errs.items():
        if n != "forward_vs_fixture":
            assert e <= TOL, (n, e)
    # The distance to the fixture's own `out` is bounded too, on every case: by the triangle inequality it is at most the distance
    # the parameters' rounding alone puts between the two float64 results (`gap`) plus the bar, and PyTorch's fp32 formula on the
    # CPU, which starts from the same fp32 parameters, sits at that same distance (on the cancellation case both are 9.5e-4).
    gap = rel_err(keep(y_ref.numpy()), g["out"])
    torch_fp32 = rel_err(keep(ref_transform(x, ls32, t32, 1)[0].numpy()), g["out"])
    report("actnorm_fixture_transform_gap", case=name, parameter_rounding=gap, pytorch_fp32=torch_fp32, hip=errs["forward_vs_fixture"])
    assert errs["forward_vs_fixture"] <= gap + TOL, (errs["forward_vs_fixture"], gap)
    assert errs["forward_vs_fixture"] <= 2 * torch_fp32 + TOL, (errs["forward_vs_fixture"], torch_fp32)
    if name != BIG:                                                  # away from the cancellation case the fixture itself is within the bar
        assert errs["forward_vs_fixture"] <= TOL


@pytest.mark.parametrize("shape", [(2, 12, 8, 8), (3, 4, 5, 4), (128, 24, 8, 8)])
def test_transform_on_offset_views_and_in_place_has_the_bits_of_the_plain_call(shape, dev):
    """HW % 4 == 0 but the pointers are only 4-byte aligned: the dword form, not a refusal -- and the same bits."""
    from fincflow_amd import ops
    x, ls, t, _, _ = case(shape)
    xd, lsd, td = x.to(dev), ls.to(dev), t.to(dev)
    for direction in (1, -1):
        want, wld = ops.finc_actnorm(xd, lsd, td, direction, True)
        got, gld = ops.finc_actnorm(offset_view(x, dev), lsd, td, direction, True, out=offset_view(torch.zeros_like(x), dev))
        assert torch.equal(got, want), direction
        if direction > 0:
            assert torch.equal(gld, wld)
        buf = xd.clone()
        same, _ = ops.finc_actnorm(buf, lsd, td, direction, out=buf)
        assert same is buf and torch.equal(buf, want), direction
        obuf = offset_view(x, dev)
        ops.finc_actnorm(obuf, lsd, td, direction, out=obuf)
        assert torch.equal(obuf, want), direction


# ---------------------------------------------------------------------------------------------------------------------------
# 3: the backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_logdet", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_all_three_gradients_against_float64_autograd(shape, with_logdet, dev):
    from fincflow_amd import ops
    x, ls, t, gy, gl = case(shape)
    if not with_logdet:
        gl = None
    ref = ref_gradients(x, ls, t, gy, gl)
    lsd = ls.to(dev)
    y, _ = ops.finc_actnorm(x.to(dev), lsd, t.to(dev), 1)
    args = (gy.to(dev), None if gl is None else gl.to(dev), y, lsd)
    got = ops.finc_actnorm_backward(*args)
    again = ops.finc_actnorm_backward(*args)
    torch.cuda.synchronize()
    names = ("grad_x", "grad_log_scale", "grad_translation")
    errs = {n: rel_err(g.cpu().numpy(), r) for n, g, r in zip(names, got, ref)}
    print("actnorm_backward", shape, with_logdet, errs)
    report("actnorm_backward", shape=list(shape), with_logdet=with_logdet, **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)
    for n, g, h in zip(names, got, again):                          # fixed-order sums: two calls, the same bits
        assert torch.equal(g, h), n
    # each subset of the outputs: None where skipped, the same bits where asked for
    for want in itertools.product((False, True), repeat=3):
        sub = ops.finc_actnorm_backward(*args, need_gx=want[0], need_gls=want[1], need_gt=want[2])
        for n, w, s, f in zip(names, want, sub, got):
            assert (s is None) == (not w), (want, n)
            if w:
                assert torch.equal(s, f), (want, n)
    # grad_x may land on grad_y
    gyd = args[0].clone()
    inplace = ops._lib.lib().finc_actnorm_backward_f32(gyd.data_ptr(), None, y.data_ptr(), lsd.data_ptr(), gyd.data_ptr(), None, None,
                                                       shape[0], shape[1], shape[2] * shape[3], None, 0,
                                                       torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert inplace == 0 and torch.equal(gyd, got[0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_against_the_reference_fixtures(name, dev):
    """Reference: float64 autograd of the formula from the fp32-rounded parameters (fixture_parameters says why); the formula's
    float64 gradients from the float64 parameters are the fixture's, at 1e-12."""
    from fincflow_amd import ops
    g, x, gy, gl, keep = fixture_case(name)
    ls64, t64, ls32, t32, ls, t = fixture_parameters(g, dev)
    pinned = ref_gradients(x, ls64, t64, gy, gl)
    for k, v in zip(("grad_x", "grad_log_scale", "grad_translation"), pinned):
        assert rel_err(keep(v) if k == "grad_x" else v, g[k]) <= 1e-12, k
    ref = ref_gradients(x, ls32, t32, gy, gl)
    y, _ = ops.finc_actnorm(x.to(dev), ls, t, 1)
    gx, gls, gt = ops.finc_actnorm_backward(gy.to(dev), gl.to(dev), y, ls)
    errs = {"grad_x": rel_err(gx.cpu().numpy(), ref[0]), "grad_log_scale": rel_err(gls.cpu().numpy(), ref[1]),
            "grad_translation": rel_err(gt.cpu().numpy(), ref[2])}
    fixture_errs = {"grad_x": rel_err(keep(gx.cpu().numpy()), g["grad_x"]), "grad_log_scale": rel_err(gls.cpu().numpy(), g["grad_log_scale"]),
                    "grad_translation": rel_err(gt.cpu().numpy(), g["grad_translation"])}
    print("actnorm_fixture_backward", name, errs, "against the fixture's float64 parameters:", fixture_errs)
    report("actnorm_fixture_backward", case=name, **errs, **{k + "_vs_fixture": v for k, v in fixture_errs.items()})
    for n, e in errs.items():
        assert e <= TOL, (n, e)
    # the distance to the fixture's own gradients: at most what the parameters' rounding alone puts between the float64 results, plus the bar
    for k, n in enumerate(("grad_x", "grad_log_scale", "grad_translation")):
        gap = rel_err(keep(ref[k]) if n == "grad_x" else ref[k], g[n])
        report("actnorm_fixture_backward_gap", case=name, output=n, parameter_rounding=gap, hip=fixture_errs[n])
        assert fixture_errs[n] <= gap + TOL, (n, fixture_errs[n], gap)
    if name != BIG:
        for n, e in fixture_errs.items():
            assert e <= TOL, (n, e)


def test_gradients_on_views_offset_by_one_float(dev):
    from fincflow_amd import ops
    shape = (2, 12, 8, 8)
    x, ls, t, gy, gl = case(shape)
    lsd = ls.to(dev)
    y, _ = ops.finc_actnorm(x.to(dev), lsd, t.to(dev), 1)
    want = ops.finc_actnorm_backward(gy.to(dev), gl.to(dev), y, lsd)
    got = ops.finc_actnorm_backward(offset_view(gy, dev), gl.to(dev), offset_view(y.cpu(), dev), lsd)
    ref = ref_gradients(x, ls, t, gy, gl)
    for n, a, b, r in zip(("grad_x", "grad_log_scale", "grad_translation"), got, want, ref):
        e = rel_err(a.cpu().numpy(), r)
        report("actnorm_backward_offset", shape=list(shape), output=n, err=e)
        assert e <= TOL, (n, e)
        if n == "grad_x":
            assert torch.equal(a, b)


def test_autograd_function_computes_only_what_is_needed(dev):
    from fincflow_amd import ops
    shape = (3, 12, 6, 10)
    x, ls, t, gy, gl = case(shape)
    ref = ref_gradients(x, ls, t, gy, gl)
    for mask in ((True, True, True), (True, False, False), (False, True, True), (False, False, True), (False, True, False)):
        leaves = [v.to(dev).requires_grad_(m) for v, m in zip((x, ls, t), mask)]
        y, ld = ops.actnorm_forward(*leaves)
        ((y * gy.to(dev)).sum() + (ld * gl.to(dev)).sum()).backward()
        for v, m, r in zip(leaves, mask, ref):
            if m:
                assert rel_err(v.grad.cpu().numpy(), r) <= TOL, mask
            else:
                assert v.grad is None
    leaves = [v.to(dev).requires_grad_(True) for v in (x, ls, t)]     # a loss that uses the output alone: grad_logdet arrives as None
    y, _ = ops.actnorm_forward(*leaves)
    (y * gy.to(dev)).sum().backward()
    for v, r in zip(leaves, ref_gradients(x, ls, t, gy, None)):
        assert rel_err(v.grad.cpu().numpy(), r) <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 4: the data-dependent initialisation
# ---------------------------------------------------------------------------------------------------------------------------
def check_init(x, dev, kind, **tags):
    from fincflow_amd import ops
    C = x.shape[1]
    x64 = x.double()
    mean = x64.mean(dim=(0, 2, 3))
    ls_ref = torch.log(x64.std(dim=(0, 2, 3)) + 1e-8)
    xd = x.to(dev)
    ls, t = torch.full((C,), 7.0, device=dev), torch.full((C,), 7.0, device=dev)
    ops.finc_actnorm_init(xd, ls, t)
    ls2, t2 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ops.finc_actnorm_init(xd, ls2, t2)
    torch.cuda.synchronize()
    assert torch.equal(ls, ls2) and torch.equal(t, t2)               # fixed-order merges: two calls, the same bits
    errs = {"translation": rel_err(t.cpu().numpy(), mean.numpy()), "log_scale": rel_err(ls.cpu().numpy(), ls_ref.numpy())}
    print(kind, tags, errs)
    report(kind, **tags, **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)
    return ls, t


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] * s[2] * s[3] >= 2])
def test_init_against_float64_mean_and_unbiased_std(shape, dev):
    check_init(case(shape)[0], dev, "actnorm_init", shape=list(shape))


@pytest.mark.parametrize("name", sorted(CASES))
def test_init_against_the_reference_fixtures(name, dev):
    """Includes the cancellation case: channel means up to 1000 beside standard deviations down to 0.01."""
    g, x, _, _, _ = fixture_case(name)
    ls, t = check_init(x, dev, "actnorm_fixture_init", case=name)
    errs = {"translation": rel_err(t.cpu().numpy(), g["translation"]), "log_scale": rel_err(ls.cpu().numpy(), g["log_scale"])}
    report("actnorm_fixture_init_vs_reference", case=name, **errs)
    for n, e in errs.items():
        assert e <= TOL, (name, n, e)


def test_init_on_an_offset_view(dev):
    from fincflow_amd import ops
    x = case((4, 12, 8, 8))[0]
    ls, t = check_init(x, dev, "actnorm_init_offset", shape=[4, 12, 8, 8])
    ls2, t2 = torch.zeros(12, device=dev), torch.zeros(12, device=dev)
    ops.finc_actnorm_init(offset_view(x, dev), ls2, t2)
    assert rel_err(ls2.cpu().numpy(), ls.cpu().numpy()) <= TOL and rel_err(t2.cpu().numpy(), t.cpu().numpy()) <= TOL


def test_one_value_per_channel_keeps_the_pytorch_result(dev, monkeypatch):
    from fincflow_amd import glow, ops
    calls = []
    real = ops.finc_actnorm_init
    monkeypatch.setattr(ops, "finc_actnorm_init", lambda *a: calls.append(1) or real(*a))
    m = glow.ActNorm(3).to(dev)
    x = torch.randn(1, 3, 1, 1, device=dev)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # (torch.std of one value warns about its degrees of freedom)
        m(x)
    assert calls == [] and int(m.initialized) == 1
    assert torch.equal(m.translation.detach(), x.view(3)) and bool(torch.isnan(m.log_scale).all())    # as the reference: NaN
    with pytest.raises(ValueError):
        ops.finc_actnorm_init(x, torch.zeros(3, device=dev), torch.zeros(3, device=dev))


# ---------------------------------------------------------------------------------------------------------------------------
# 5, 6: the module
# ---------------------------------------------------------------------------------------------------------------------------
class Counter:
    NAMES = ("finc_actnorm", "finc_actnorm_backward", "finc_actnorm_init", "actnorm_forward")

    def __init__(self, monkeypatch):
        from fincflow_amd import ops
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def counted(*args, **kwargs):
            self.n[name] += 1
            return fn(*args, **kwargs)
        return counted

    def take(self):
        n, self.n = self.n, dict.fromkeys(self.NAMES, 0)
        return n


def counts(**kw):
    return dict(dict.fromkeys(Counter.NAMES, 0), **kw)


@pytest.mark.parametrize("shape", [(16, 12, 8, 8), (6, 5, 7, 3)])
def test_module_initialises_and_runs_on_the_hip_path(shape, dev, monkeypatch):
    from fincflow_amd import glow
    counter = Counter(monkeypatch)
    C = shape[1]
    x = case(shape)[0] * 3.0 + 2.0
    m = glow.ActNorm(C).to(dev)
    assert list(m.state_dict()) == ["translation", "log_scale", "initialized"]
    v0 = m.log_scale._version
    with torch.no_grad():
        y, ld = m(x.to(dev))
    assert counter.take() == counts(finc_actnorm_init=1, finc_actnorm=1)
    assert int(m.initialized) == 1 and m._is_initialized() and m.log_scale._version > v0
    y64 = y.double().cpu()
    mean_err = float(y64.mean(dim=(0, 2, 3)).abs().max())
    std_err = float((y64.std(dim=(0, 2, 3)) - 1).abs().max())
    report("actnorm_module_init", shape=list(shape), mean=mean_err, std=std_err)
    assert mean_err <= 1e-5 and std_err <= 1e-5, (mean_err, std_err)
    ref = copy.deepcopy(m).double().cpu()
    with torch.no_grad():
        y_ref, ld_ref = ref(x.double())
        r = m.reverse(y)
    assert counter.take() == counts(finc_actnorm=1)
    assert rel_err(y.cpu().numpy(), y_ref.numpy()) <= TOL and rel_err(ld.cpu().numpy(), ld_ref.numpy()) <= TOL
    assert rel_err(r.cpu().numpy(), x.double().numpy()) <= TOL

    # under autograd: actnorm_forward, every gradient against float64
    gy, gl = torch.randn(shape), torch.randn(shape[0])
    xd = x.to(dev).requires_grad_(True)
    yt, ldt = m(xd)
    ((yt * gy.to(dev)).sum() + (ldt * gl.to(dev)).sum()).backward()
    assert counter.take() == counts(actnorm_forward=1, finc_actnorm=1, finc_actnorm_backward=1)
    x64 = x.double().requires_grad_(True)
    y64, ld64 = ref(x64)
    ((y64 * gy.double()).sum() + (ld64 * gl.double()).sum()).backward()
    errs = {"grad_input": rel_err(xd.grad.cpu().numpy(), x64.grad.numpy()),
            "grad_log_scale": rel_err(m.log_scale.grad.cpu().numpy(), ref.log_scale.grad.numpy()),
            "grad_translation": rel_err(m.translation.grad.cpu().numpy(), ref.translation.grad.numpy())}
    report("actnorm_module_gradients", shape=list(shape), **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)

    # reverse under autograd, float64 on the device, 2-D inputs: the PyTorch lines
    m.reverse(y.detach().requires_grad_(True)).sum().backward()
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        m64(x.double().to(dev))
        glow.ActNorm(C).to(dev)(torch.randn(8, C, device=dev))
    assert counter.take() == counts()

    # the flag: a state dict, mark_initialized, reset_initialization and a direct write before the first call
    fresh = glow.ActNorm(C).to(dev)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(x.to(dev))[0], y)
    assert counter.take() == counts(finc_actnorm=1)
    hand = glow.ActNorm(C).to(dev)
    hand.mark_initialized()
    direct = glow.ActNorm(C).to(dev)
    direct.initialized.fill_(1)
    with torch.no_grad():
        assert torch.equal(hand(x.to(dev))[0], x.to(dev)) and torch.equal(direct(x.to(dev))[0], x.to(dev))
    assert counter.take() == counts(finc_actnorm=2)
    hand.reset_initialization()
    with torch.no_grad():
        assert torch.equal(hand(x.to(dev))[0], y)
    assert counter.take() == counts(finc_actnorm_init=1, finc_actnorm=1)
    assert torch.equal(hand.log_scale, m.log_scale) and torch.equal(hand.translation, m.translation)


def test_autograd_saves_one_activation_and_it_is_the_output(dev, monkeypatch):
    from fincflow_amd import glow, ops
    shape = (8, 12, 8, 8)
    x = case(shape)[0]
    m = glow.ActNorm(12).to(dev)
    m.mark_initialized()
    n = x.numel()

    def saved_by_forward():
        kept = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: kept.append(t) or t, lambda t: t):
            y, ld = m(x.to(dev).requires_grad_(True))
        return y, [t for t in kept if t.numel() == n]
    def beside_the_output(y, big):
        return [t for t in big if t.untyped_storage().data_ptr() != y.untyped_storage().data_ptr()]
    y, big = saved_by_forward()
    assert len(big) == 1 and beside_the_output(y, big) == []         # exactly one, and it is the returned y
    monkeypatch.setattr(ops, "actnorm_supported", lambda: False)
    y_torch, big_torch = saved_by_forward()
    extra_torch = beside_the_output(y_torch, big_torch)
    report("actnorm_saved_activations", hip=len(big), hip_beside_output=0, pytorch=len(big_torch), pytorch_beside_output=len(extra_torch))
    print("saved activation-sized tensors: HIP", len(big), "(all the output); PyTorch", len(big_torch), "of which beside the output",
          len(extra_torch))
    assert len(extra_torch) > 0                                      # PyTorch keeps x - translation alive: memory the HIP path does not hold


# ---------------------------------------------------------------------------------------------------------------------------
# 7, 8: inside a flow step and the stack
# ---------------------------------------------------------------------------------------------------------------------------
def test_flow_step_gradients_equal_the_pytorch_actnorm(dev, monkeypatch):
    """[FastFlowUnit, ActNorm, Conv1x1] log_prob(...).mean().backward(): every parameter's gradient against the same run with
    ops.actnorm_supported patched to False, i.e. ActNorm on PyTorch's autograd."""
    from fincflow_amd import FastFlowUnit, FlowSequential, glow, ops
    from fincflow_amd.layers import StandardNormal
    torch.manual_seed(4)
    np.random.seed(4)
    B, C, H, W = 8, 48, 16, 16
    unit, an, c = FastFlowUnit(C, C, 3), glow.ActNorm(C), glow.Conv1x1(C)
    seq = FlowSequential(StandardNormal((C, H, W)), unit, an, c).to(dev)
    with torch.no_grad():
        an.log_scale.copy_(0.2 * torch.randn(C, device=dev))
        an.translation.copy_(torch.randn(C, device=dev))
        an.initialized.fill_(1)
    x = torch.randn(B, C, H, W, device=dev)
    counter = Counter(monkeypatch)

    def grads():
        seq.zero_grad(set_to_none=True)
        seq.log_prob(x).mean().backward()
        return {n: p.grad.detach().cpu().numpy().copy() for n, p in seq.named_parameters()}
    new = grads()
    assert counter.take() == counts(actnorm_forward=1, finc_actnorm=1, finc_actnorm_backward=1)
    monkeypatch.setattr(ops, "actnorm_supported", lambda: False)
    old = grads()
    assert counter.take() == counts()
    assert set(new) == set(old) and any(n.endswith("log_scale") for n in new)
    for n in new:
        e = rel_err(new[n], old[n])
        report("actnorm_flow_step_gradients", parameter=n, err=e)
        assert e <= TOL, (n, e)


def test_stack_under_autograd_matches_the_reference_trace_and_the_pytorch_gradients(dev, monkeypatch):
    from fincflow_amd import ops
    from test_glow_stack import build_ours
    g = golden("stack_c4_small")
    layers = build_ours()
    fill_stack_parameters(layers, ffu_weights=g)
    layers = [l.to(dev) for l in layers]
    params = [p for l in layers for p in l.parameters()]
    assert params and all(p.requires_grad for p in params)
    x = torch.from_numpy(g["x"]).to(dev)
    assert tuple(x.shape) == STACK_INPUT
    counter = Counter(monkeypatch)

    def run():
        for p in params:
            p.grad = None
        h, logdet = x, 0
        for m in layers:
            h, ld = m(h, None)
            logdet = logdet + ld
        logp = logdet - 0.5 * (h * h).flatten(start_dim=1).sum(-1)
        logp.mean().backward()
        return h.detach(), logdet.detach(), [p.grad.detach().cpu().numpy().copy() for p in params]
    h, logdet, new = run()
    assert counter.take() == counts(actnorm_forward=3, finc_actnorm=3, finc_actnorm_backward=3)
    assert rel_err(h.cpu().numpy(), g["z"]) <= 1e-5
    assert np.allclose(logdet.cpu().numpy(), g["logdet"], rtol=1e-5, atol=1e-4)
    monkeypatch.setattr(ops, "actnorm_supported", lambda: False)
    _, _, old = run()
    assert counter.take() == counts()
    for k, (a, b) in enumerate(zip(new, old)):
        e = rel_err(a, b)
        report("actnorm_stack_gradients", parameter=k, err=e)
        assert e <= TOL, (k, e)


# ---------------------------------------------------------------------------------------------------------------------------
# 9: capture
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 12, 16, 16), (8, 48, 4, 4)])
def test_captured_forward_reverse_and_init_replay_with_the_bits_of_the_eager_call(shape, dev):
    from fincflow_amd import _lib, glow, ops
    C = shape[1]
    x1, ls, t, _, _ = case(shape)
    x2 = case((shape[0] + 1,) + shape[1:])[0][:shape[0]].contiguous() * 1.5
    m = glow.ActNorm(C).to(dev)
    with torch.no_grad():
        m.log_scale.copy_(ls.to(dev))
        m.translation.copy_(t.to(dev))
        m.mark_initialized()
        x = x1.to(dev)
        pl, pt = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        want = {}
        for k, v in (("a", x1), ("b", x2)):                         # eager first: results to compare with, workspace allocated
            x.copy_(v)
            y0, ld0 = m(x)
            r0 = m.reverse(x)
            ops.finc_actnorm_init(x, pl, pt)
            want[k] = [u.clone() for u in (y0, ld0, r0, pl, pt)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y, ld = m(x)
            r = m.reverse(x)
            ops.finc_actnorm_init(x, pl, pt)
        for k, v in (("b", x2), ("a", x1), ("b", x2)):
            x.copy_(v)
            for u in (y, ld, r, pl, pt):
                u.zero_()
            g.replay()
            torch.cuda.synchronize()
            for u, w in zip((y, ld, r, pl, pt), want[k]):
                assert torch.equal(u, w), k
    assert not _lib.fault_pending()
