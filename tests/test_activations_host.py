"""The smooth invertible activations without a GPU: the layers' PyTorch lines against recordings of the reference's own classes, the
state-dict keys, the bracketed Newton inverse against float64 bisection over the whole parameter box (with the sweep that fixes its
trip count), the launch plans against the hand-stated ones, workspace sizes, the entry points' refusal order and the constructors'
checks."""
import numpy as np
import pytest
import torch

import activation_cases as ac
import flow_twin
from helpers import fake_ptr, golden

EPS32 = float(np.finfo(np.float32).eps)


def lines(m, v, inverse=False):
    out, lad = m._lines(v, inverse)
    return out, lad.flatten(1).sum(-1)


@pytest.fixture(scope="module")
def recorded():
    return golden(ac.GOLDEN[:-4])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the lines against the reference's recordings
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ac.KINDS)
def test_lines_match_the_reference_at_its_defaults(kind, recorded):
    """float64 lines against the reference's float64 (another formula for the same function: 1e-12), float32 lines under
    max(1e-5, 2 * the reference's own float32 error).  LeakyRelu's recorded float64 log-det is float32 arithmetic -- the reference's
    torch.where(input < 0, self.alpha, 1.0) has two Python numbers to choose from and returns the default dtype -- so it is held to
    float32's epsilon."""
    x = torch.from_numpy(recorded["x"])
    assert torch.equal(x.reshape(3, -1)[0, :6], torch.tensor(ac.PLANTED)) and bool(torch.signbit(x.reshape(3, -1)[0, 1]))
    want = {k: recorded[f"{kind}/{k}64"] for k in ("y", "logdet", "rev", "rev_of_x")}
    ref32 = {k: recorded[f"{kind}/{k}32"] for k in want}
    for dtype in (torch.float64, torch.float32):
        t = ac.layer(kind).to(dtype)
        tight = 1e-12
        with torch.no_grad():
            y, ld = t(x.to(dtype))
            got = dict(y=y, logdet=ld, rev=t.reverse(torch.from_numpy(want["y"]).to(dtype)), rev_of_x=t.reverse(x.to(dtype)))
            ld_rev = t.reverse_with_logdet(torch.from_numpy(want["y"]).to(dtype))[1]
        for k in want:
            err, e_ref = flow_twin.error(got[k], want[k]), flow_twin.error(ref32[k], want[k])
            tight = EPS32 if (kind, k) == ("leaky_relu", "logdet") else 1e-12
            bar = tight if dtype == torch.float64 else max(1e-5, 2 * e_ref)
            print("%s %s %s: lines %.2e reference float32 %.2e bar %.1e" % (kind, dtype, k, err, e_ref, bar))
            assert err <= bar, (kind, dtype, k, err, bar)
        tight = EPS32 if kind == "leaky_relu" else 1e-12
        assert flow_twin.error(ld_rev, want["logdet"]) <= (tight if dtype == torch.float64 else 1e-5)
        assert flow_twin.error(t.logdet(x.to(dtype)), want["logdet"]) <= (tight if dtype == torch.float64 else 1e-5)


def test_zero_takes_the_identity_branch_and_a_nan_passes_through():
    x = ac.planted(torch.randn(2, 3, 4))
    x.view(2, -1)[1, 0] = float("nan")
    for kind in ac.KINDS:
        m = ac.layer(kind)
        with torch.no_grad():
            for inverse in (False, True):
                out, lad = m._lines(x, inverse)
                assert torch.isnan(out.view(2, -1)[1, 0]) and float(lad.view(2, -1)[1, 0]) == 0.0, (kind, inverse)
                assert int(torch.isnan(out).sum()) == 1 and bool(torch.isfinite(lad).all())
                if "leaky_relu" in kind and "smooth" not in kind:
                    # 0.0 and -0.0 are not < 0: no log-derivative, and the bits pass through
                    assert lad.view(2, -1)[0, :2].tolist() == [0.0, 0.0] and bool(torch.signbit(out.view(2, -1)[0, 1]))
                    assert float(lad.view(2, -1)[0, 3]) == pytest.approx(float(np.log(m._numbers()[0] if kind == "leaky_relu" else 1.0)))


def test_state_dicts_carry_the_reference_keys():
    from fincflow_amd import glow
    assert list(glow.LearnableLeakyRelu().state_dict()) == ["alpha_logit"]
    assert tuple(glow.LearnableLeakyRelu().alpha_logit.shape) == (1,) and float(glow.LearnableLeakyRelu().alpha_logit.detach()) == 0.0
    assert float(glow.LearnableLeakyRelu().get_alpha().detach()) == 1.0
    for m in (glow.SmoothLeakyRelu(), glow.LeakyRelu(), glow.SmoothTanh()):
        assert list(m.state_dict()) == [] and list(m.parameters()) == []
    assert (glow.SmoothLeakyRelu().alpha, glow.LeakyRelu().alpha, glow.SmoothTanh().alpha, glow.SmoothTanh().beta) == (0.3, 0.1, 1.0, 0.1)
    src = torch.nn.Sequential(glow.SmoothLeakyRelu(), glow.LearnableLeakyRelu())
    with torch.no_grad():
        src[1].alpha_logit.fill_(0.7)
    state = src.state_dict()
    assert list(state) == ["1.alpha_logit"]
    dst = torch.nn.Sequential(glow.SmoothLeakyRelu(), glow.LearnableLeakyRelu())
    dst.load_state_dict(state, strict=True)
    assert torch.equal(dst[1].alpha_logit, src[1].alpha_logit)


def test_constructors_refuse_parameters_that_are_not_positive_and_finite():
    from fincflow_amd import glow
    for bad in (0.0, -0.3, float("inf"), float("nan")):
        for make in (lambda v: glow.SmoothLeakyRelu(v), lambda v: glow.LeakyRelu(v), lambda v: glow.SmoothTanh(v, 0.1),
                     lambda v: glow.SmoothTanh(1.0, v)):
            with pytest.raises(ValueError):
                make(bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the bracketed inverse
# ---------------------------------------------------------------------------------------------------------------------------------
def sweep(points, draws, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.linspace(-40, 40, points), 3 * torch.randn(draws, generator=gen)


def elementwise(x, x64):
    return float(((x.double() - x64).abs() / x64.abs().clamp(min=1)).max())


BOX = [(kind, p) for kind in ("smooth_leaky_relu", "smooth_tanh") for p in ac.BOX[kind]]


@pytest.mark.parametrize("kind,params", BOX, ids=lambda v: str(v))
def test_bracketed_inverse_against_float64_bisection(kind, params):
    """Over the box, on linspace(-40, 40, 16001) and 3 * randn(4000) in fp32.  Bars: flow_twin.error under 1e-5, the fixed part of the
    project's bar (the fp32 lines ARE the yardstick here), and per element |x - x64| / max(1, |x64|) under 4 eps / min f': y and the
    evaluation of f each carry a relative rounding of eps / 2, which the inverse divides by f' >= min(alpha, 1) or beta -- the factor 4
    covers both and the final Newton step's own two roundings.  Then: inside the bracket, monotone over the grid, finite at +-1e30."""
    m, m64 = ac.layer(kind, params), ac.layer(kind, params).double()
    grid, draws = sweep(16001, 4000)
    y = torch.cat([grid, draws])
    with torch.no_grad():
        x = m.reverse(y.view(1, -1)).view(-1)
        x64 = ac.bisect64(m64, y.double())
        assert float((m64._lines(x64, False)[0] - y.double()).abs().max()) <= 1e-12 * 4000
    min_slope = min(params[0], 1.0) if kind == "smooth_leaky_relu" else params[1]
    err, each = flow_twin.error(x, x64), elementwise(x, x64)
    print("inverse %s %s: error %.2e, per element %.2e (bar %.2e)" % (kind, params, err, each, 4 * EPS32 / min_slope))
    assert err <= 1e-5 and each <= 4 * EPS32 / min_slope
    assert bool(torch.isfinite(x).all())
    # inside the analytic bracket
    if kind == "smooth_tanh":
        a, b = params
        t = y.abs()
        assert bool(((x.abs() >= torch.maximum(t / (a + b), (t - 1) / b)) & (x.abs() <= t / b)).all())
        assert bool((torch.signbit(x) == torch.signbit(y)).all())
    else:
        a = params[0]
        ginv = lambda v: torch.where(v < 0, v / a, v)
        g1, g2 = ginv(y), ginv(y - (1 - a) * float(np.log(2.0)))
        assert bool(((x >= torch.minimum(g1, g2)) & (x <= torch.maximum(g1, g2))).all())
    xs = x[:len(grid)]
    assert bool((xs[1:] >= xs[:-1]).all()), "not monotone over consecutive grid points"
    with torch.no_grad():
        far = m.reverse(torch.tensor([[1e30, -1e30, 3e38, -3e38]]))
    assert bool(torch.isfinite(far).all()) and bool((far[0, ::2] > 0).all()) and bool((far[0, 1::2] < 0).all())


def test_the_trip_count_is_the_one_the_sweep_gives():
    """DESIGN 3.26's rule on the issue's own sweep (linspace(-40, 40, 400001) and 3 * randn(100000), fp32, error per element), for the
    two cases that decide it: the smallest count at which the error is within 2x of its floor is 7 (smooth tanh (8, 0.01); smooth leaky
    ReLU 0.01 needs 6), plus 2 trips of margin -- the count of the lines and of the kernels."""
    from fincflow_amd import _lib, glow
    y = torch.cat(sweep(400001, 100000))
    need = {}
    for kind, params in (("smooth_leaky_relu", (0.01,)), ("smooth_tanh", (8.0, 0.01))):
        m, m64 = ac.layer(kind, params), ac.layer(kind, params).double()
        x64 = ac.bisect64(m64, y.double())
        errs = []
        for n in range(4, 13):
            if kind == "smooth_tanh":
                t = y.abs()
                lo = torch.maximum(t / (params[0] + params[1]), (t - 1) / params[1])
                x = glow.bracketed_newton(t, m._map, lo, t / params[1], lo, trips=n)
                x = torch.where(y < 0, -x, x)
            else:
                a = params[0]
                ginv = lambda v: torch.where(v < 0, v / a, v)
                g1, g2 = ginv(y), ginv(y - (1 - a) * float(np.log(2.0)))
                x = glow.bracketed_newton(y, m._map, torch.minimum(g1, g2), torch.maximum(g1, g2), g1, trips=n)
            errs.append(elementwise(x, x64))
        need[kind] = 4 + next(k for k, e in enumerate(errs) if e <= 2 * min(errs))
        print(kind, params, "errors by trips 4..12:", " ".join("%.1e" % e for e in errs), "-> within 2x of the floor at", need[kind])
    assert need == {"smooth_leaky_relu": 6, "smooth_tanh": ac.CONVERGED_AFTER}
    assert glow.ACTIVATION_TRIPS == ac.TRIPS == max(need.values()) + 2
    assert [_lib.lib().finc_debug_activation_trips(k) for k in range(-1, 5)] == [-1, ac.TRIPS, 0, 0, ac.TRIPS, -1]


def test_smooth_tanh_3_005_converges_where_the_reference_cycles(recorded):
    """The reference's 100 unbracketed Newton steps end far from the root on these inputs (reported, not a yardstick)."""
    y = torch.from_numpy(recorded["x"])
    m = ac.layer("smooth_tanh", (3.0, 0.05))
    x64 = ac.bisect64(ac.layer("smooth_tanh", (3.0, 0.05)).double(), y.double())
    with torch.no_grad():
        ours = elementwise(m.reverse(y), x64)
    ref = elementwise(torch.from_numpy(recorded["smooth_tanh_3_0.05/rev_of_x32"]), x64)
    print("SmoothTanh(3, 0.05).reverse per element: bracketed %.2e, the reference's recording %.2e" % (ours, ref))
    assert ours <= 4 * EPS32 / 0.05 and ref > 1e-2


@pytest.mark.parametrize("kind,params", (("smooth_leaky_relu", (0.3,)), ("smooth_tanh", (3.0, 0.05))))
def test_reverse_lines_differentiate_by_the_implicit_function(kind, params):
    m = ac.layer(kind, params).double()
    y = (4 * torch.randn(2, 7, dtype=torch.float64)).requires_grad_(True)
    x, ld = m.reverse_with_logdet(y)
    gx, = torch.autograd.grad(x.sum(), y, retain_graph=True)
    leaf = x.detach().requires_grad_(True)
    f, lad = m._lines(leaf, False)
    fp, = torch.autograd.grad(f.sum(), leaf, retain_graph=True)
    lp, = torch.autograd.grad(lad.sum(), leaf)
    assert float((gx - 1 / fp).abs().max()) <= 1e-12
    gl, = torch.autograd.grad(ld.sum(), y)
    assert float((gl - lp / fp).abs().max()) <= 1e-10


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_lines_have_the_analytic_gradient_at_exactly_zero(dtype):
    """|x| and max(x, 0) have a kink at 0 that the smooth maps built on them do not: autograd through the lines at 0.0 and -0.0 gives
    f'(0) = alpha + (1 - alpha) / 2 and alpha + beta, and L'(0) = (1 - alpha) / 4 / f'(0) and 0."""
    x = torch.tensor([[0.0, -0.0, 1e-30, -1e-30]], dtype=dtype)
    for m, fp, lp in ((ac.layer("smooth_leaky_relu", (0.3,)).to(dtype), 0.65, 0.7 / 4 / 0.65), (ac.layer("smooth_tanh", (3.0, 0.05)).to(dtype), 3.05, 0.0)):
        for inverse in ((False, True) if m.kind == "smooth_tanh" else (False,)):    # (the smooth tanh maps 0 to 0: its inverse meets 0 too)
            a = x.clone().requires_grad_(True)
            out, lad = m._lines(a, inverse)
            g, = torch.autograd.grad(out.sum(), a, retain_graph=True)
            gl, = torch.autograd.grad(lad.sum(), a)
            tol = 1e-12 if dtype == torch.float64 else 1e-6
            assert float((g - (1 / fp if inverse else fp)).abs().max()) <= tol, (m.kind, inverse, g)
            assert float((gl - (lp / fp if inverse else lp)).abs().max()) <= tol, (m.kind, inverse, gl)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. plans, workspaces, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_plans_are_the_hand_stated_ones():
    from fincflow_amd import _lib
    for (shape, align), want in ac.PLANS.items():
        B, C, HW = ac.dims(shape)
        assert _lib.pixel_plan("parts", "activation", B, C, HW, align=align) == want, (shape, align)
        assert want["parts"] == min(-(-want["items"] // 256), -(-2048 // B)) and want["trips"] == -(-want["items"] // (256 * want["parts"]))
    # N % 4 decides, not HW % 4
    assert _lib.pixel_plan("parts", "activation", 2, 4, 15)["io"] == 4 and _lib.pixel_plan("parts", "activation", 2, 3, 15)["io"] == 1


def test_workspace_sizes():
    """Four log-det partials per image and chunk of 256 dword items (more than the slope gradient's one per workgroup), padded."""
    from fincflow_amd import _lib
    ws = _lib.lib().finc_activation_workspace_bytes
    for B, C, HW in ((1, 1, 1), (2, 3, 16), (3, 2, 15), (512, 8, 576), (512, 8, 575), (7, 96, 4096)):
        floats = 4 * B * -(-(C * HW) // 256)
        assert ws(B, C, HW) == max(256, -(-4 * floats // 256) * 256), (B, C, HW)
    assert ws(0, 3, 16) == ws(2, -1, 16) == ws(2, 3, 0) == 256
    assert ws(4, 8, 576) <= ws(8, 8, 576) <= ws(8, 8, 1024)


def test_entry_points_refuse_in_the_documented_order():
    from fincflow_amd import _lib
    L = _lib.lib()
    p, odd = fake_ptr(4096), fake_ptr(4098)
    run = lambda **k: L.finc_activation_f32(*[{**dict(kind=0, p0=0.3, p1=0.0, slope=None, direction=1, x=p, y=p, logdet=None, B=2, C=3,
                                                      HW=4, ws=None, nbytes=0, stream=None), **k}[n] for n in
                                              ("kind", "p0", "p1", "slope", "direction", "x", "y", "logdet", "B", "C", "HW", "ws", "nbytes",
                                               "stream")])
    # each call breaks the rule it is named after and every later one: the earlier refusal wins
    null, dims = run(x=None, B=0, kind=9), run(B=0, y=odd, kind=9)
    align, unsupported = run(y=odd, kind=9), run(kind=9, logdet=p)
    workspace = run(logdet=p)
    assert len({0, null, dims, align, unsupported, workspace}) == 6, (null, dims, align, unsupported, workspace)
    assert unsupported == 3
    assert run(direction=0) == dims
    for bad in (dict(p0=0.0), dict(p0=float("inf")), dict(p0=float("nan")), dict(kind=3, p0=1.0, p1=0.0), dict(slope=p), dict(kind=2)):
        assert run(**bad) == unsupported, bad
    back = lambda **k: L.finc_activation_backward_f32(*[{**dict(kind=0, p0=0.3, p1=0.0, slope=None, mode=0, gy=p, gld=None, v=fake_ptr(8192),
                                                                xo=None, gx=p, gs=None, B=2, C=3, HW=4, ws=None, nbytes=0, stream=None), **k}[n]
                                                        for n in ("kind", "p0", "p1", "slope", "mode", "gy", "gld", "v", "xo", "gx", "gs", "B",
                                                                  "C", "HW", "ws", "nbytes", "stream")])
    assert back(gy=None) == null and back(gx=None) == null and back(v=None) == null
    assert back(mode=3) == dims and back(gx=fake_ptr(8192)) == dims and back(mode=2, xo=p) == dims
    assert back(gx=odd) == align
    assert back(xo=fake_ptr(12288)) == unsupported and back(gs=fake_ptr(12288)) == unsupported
    assert back(kind=2, slope=p, gs=fake_ptr(12288)) == workspace
