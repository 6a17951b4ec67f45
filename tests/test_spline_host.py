"""glow.SplineActivation and the spline entry points without a GPU: the layer's PyTorch lines in float64 against the recording of the
reference's layer (tests/golden/make_golden_spline.py), the fixture's coverage of bins and tails, the refusal ladder with fake
pointers, the version rung, the launch plans of the GPU cases, and the layer inside a FlowSequential on the CPU."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from helpers import GOLDEN, fake_ptr as _p, load_stub_library
from spline_cases import CONFIGS, GOLDEN as GOLDEN_FILE, MULTI_TRIP, PLANS, bins_of, knots64, spline_plan
from fincflow_amd import FastFlowUnit, FlowSequential, _lib, glow


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, GOLDEN_FILE))


def layer_of(g, name, dtype=torch.float64):
    shape, K, tb, individual = CONFIGS[name]
    m = glow.SplineActivation(shape[1:], n_bins=K, tail_bound=tb, individual_weights=individual).to(dtype)
    state = {"unnormalized_widths": g[name + "/uw"], "unnormalized_heights": g[name + "/uh"], "unnormalized_derivatives": g[name + "/ud"]}
    missing = m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in state.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_float64_lines_match_the_reference_recording(recorded, name):
    """Outputs and log-det within 1e-12, gradients within 1e-10, and the reference's state-dict keys and shapes load strictly."""
    g = recorded
    m = layer_of(g, name)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "unnormalized_widths": g[name + "/uw"].shape, "unnormalized_heights": g[name + "/uh"].shape,
        "unnormalized_derivatives": g[name + "/ud"].shape}
    x = torch.from_numpy(g[name + "/x"]).double().requires_grad_(True)
    y, ld = m(x)
    assert float((y.detach() - torch.from_numpy(g[name + "/y64"])).abs().max()) <= 1e-12
    assert float((ld.detach() - torch.from_numpy(g[name + "/logdet64"])).abs().max()) <= 1e-12
    with torch.no_grad():
        rev, rld = m.reverse_with_logdet(torch.from_numpy(g[name + "/y64"]))
        assert float((m.reverse(torch.from_numpy(g[name + "/y64"])) - rev).abs().max()) == 0.0
        assert float((m.logdet(x.detach()) - ld.detach()).abs().max()) == 0.0
    assert float((rev - torch.from_numpy(g[name + "/rev64"])).abs().max()) <= 1e-12
    assert float((rld - torch.from_numpy(g[name + "/logdet64"])).abs().max()) <= 1e-10      # (the forward log-det, at the recovered input)
    ((y * torch.from_numpy(g[name + "/r"]).double()).sum() + (ld * torch.from_numpy(g[name + "/s"]).double()).sum()).backward()
    for got, key in ((x.grad, "grad_x"), (m.unnormalized_widths.grad, "grad_uw"), (m.unnormalized_heights.grad, "grad_uh"),
                     (m.unnormalized_derivatives.grad, "grad_ud")):
        assert float((got - torch.from_numpy(g[name + "/" + key])).abs().max()) <= 1e-10, key


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_fixture_hits_every_bin_both_tails_and_the_planted_values(recorded, name):
    """A condition on the fixture, asserted from the knots: no bin may be left out."""
    g = recorded
    shape, K, tb, individual = CONFIGS[name]
    x = g[name + "/x"]
    cw = knots64(g[name + "/uw"], g[name + "/uh"], g[name + "/ud"], tb)[0]
    assert cw.shape == (int(np.prod(shape[1:])) if individual else 1, K + 1)
    bins = bins_of(x, cw, tb)
    assert set(np.unique(bins)) == set(range(-1, K + 1)), sorted(np.unique(bins))
    flat = x.reshape(-1)
    for v in (tb, -tb, 0.0, np.float32(1.2 * tb), np.float32(-1.2 * tb)):
        assert (flat == np.float32(v)).any(), v
    outside = np.abs(x.astype(np.float64)) > tb
    assert (g[name + "/y64"][outside] == x[outside]).all() and outside.sum() >= 2
    # the layer's knots are these knots
    got = layer_of(g, name)._knots()
    for a, b in zip(got, knots64(g[name + "/uw"], g[name + "/uh"], g[name + "/ud"], tb)):
        assert float(np.abs(a.detach().numpy() - b).max()) <= 1e-13


def test_refusal_ladder_with_fake_pointers():
    """NULL -> 1, dims / direction / tail_bound / aliasing -> 2, alignment -> 7, K or P without a kernel -> 3, workspace -> 4, in that
    order of precedence; nothing is read, nothing launched."""
    L = _lib.lib()
    x, tab, y, ld, ws = _p(0x1000), _p(0x2000), _p(0x4000), _p(0x5000), _p(0x10000)
    big = 1 << 30
    f = L.finc_spline_f32
    assert f(None, tab, 1, 5, 10.0, 1, y, ld, 2, 3, 16, ws, big, None) == 1
    assert f(x, None, 1, 5, 10.0, 1, y, ld, 2, 3, 16, ws, big, None) == 1
    assert f(x, tab, 1, 5, 10.0, 1, None, ld, 2, 3, 16, ws, big, None) == 1
    assert f(None, tab, 1, 5, 10.0, 1, y, ld, 0, 3, 16, ws, big, None) == 1              # (NULL comes before the dims)
    assert f(x, tab, 1, 5, 10.0, 1, y, ld, 0, 3, 16, ws, big, None) == 2
    assert f(x, tab, 1, 5, 10.0, 1, y, ld, 2, 1 << 15, 1 << 15, ws, big, None) == 2      # C * HW * 4 >= 2^31
    assert f(x, tab, 1, 5, 0.0, 1, y, ld, 2, 3, 16, ws, big, None) == 2
    assert f(x, tab, 1, 5, float("inf"), 1, y, ld, 2, 3, 16, ws, big, None) == 2
    assert f(x, tab, 1, 5, float("nan"), 1, y, ld, 2, 3, 16, ws, big, None) == 2
    assert f(_p(0x1002), tab, 1, 5, 10.0, 2, y, ld, 2, 3, 16, ws, big, None) == 2        # (the direction comes before the alignment)
    assert f(_p(0x1002), tab, 1, 5, 10.0, 1, y, ld, 2, 3, 16, ws, big, None) == 7
    assert f(x, _p(0x2001), 1, 5, 10.0, -1, y, ld, 2, 3, 16, ws, big, None) == 7
    assert f(x, tab, 1, 5, 10.0, 1, _p(0x4002), None, 2, 3, 16, None, 0, None) == 7
    assert f(x, tab, 1, 17, 10.0, 1, y, _p(0x5001), 2, 3, 16, ws, big, None) == 7        # (the alignment comes before K)
    assert f(x, tab, 1, 17, 10.0, 1, y, ld, 2, 3, 16, None, 0, None) == 3                # (K comes before the workspace)
    assert f(x, tab, 1, 1, 10.0, 1, y, ld, 2, 3, 16, ws, big, None) == 3
    assert f(x, tab, 47, 5, 10.0, 1, y, ld, 2, 3, 16, ws, big, None) == 3                # P is neither 1 nor C * HW = 48
    assert f(x, tab, 3, 5, 10.0, 1, y, ld, 2, 3, 16, ws, big, None) == 3
    need = L.finc_spline_workspace_bytes(2, 3, 16, 5, 48)
    assert f(x, tab, 48, 5, 10.0, 1, y, ld, 2, 3, 16, None, 0, None) == 4
    assert f(x, tab, 48, 5, 10.0, 1, y, ld, 2, 3, 16, ws, need - 1, None) == 4
    assert f(x, tab, 48, 5, 10.0, -1, y, ld, 2, 3, 16, _p(0x10002), big, None) == 4

    gy, gl, gx, gt = _p(0x6000), _p(0x7000), _p(0x8000), _p(0x9000)
    for g in (L.finc_spline_backward_f32, L.finc_spline_reverse_backward_f32):
        assert g(None, None, x, tab, 1, 5, 10.0, gx, gt, 2, 3, 16, ws, big, None) == 1   # neither gradient comes in
        assert g(gy, gl, None, tab, 1, 5, 10.0, gx, gt, 2, 3, 16, ws, big, None) == 1
        assert g(gy, gl, x, None, 1, 5, 10.0, gx, gt, 2, 3, 16, ws, big, None) == 1
        assert g(gy, gl, x, tab, 1, 5, 10.0, None, None, 2, 3, 16, ws, big, None) == 1   # nothing asked for
        assert g(gy, gl, x, tab, 1, 5, 10.0, gx, gt, 2, 0, 16, ws, big, None) == 2
        assert g(gy, gl, x, tab, 1, 5, -1.0, gx, gt, 2, 3, 16, ws, big, None) == 2
        assert g(_p(0x6002), gl, x, tab, 1, 5, 10.0, x, gt, 2, 3, 16, ws, big, None) == 2    # (grad_x == x comes before the alignment)
        assert g(_p(0x6002), gl, x, tab, 1, 5, 10.0, gx, gt, 2, 3, 16, ws, big, None) == 7
        assert g(gy, _p(0x7001), x, tab, 1, 5, 10.0, gx, gt, 2, 3, 16, ws, big, None) == 7
        assert g(gy, gl, x, tab, 1, 99, 10.0, gx, _p(0x9002), 2, 3, 16, ws, big, None) == 7
        assert g(gy, gl, x, tab, 1, 99, 10.0, gx, gt, 2, 3, 16, None, 0, None) == 3
        assert g(gy, gl, x, tab, 5, 5, 10.0, gx, gt, 2, 3, 16, None, 0, None) == 3
        assert g(gy, gl, x, tab, 48, 5, 10.0, gx, gt, 2, 3, 16, None, 0, None) == 4
        assert g(gy, None, x, tab, 1, 5, 10.0, None, gt, 2, 3, 16, ws, L.finc_spline_workspace_bytes(2, 3, 16, 5, 1) - 1, None) == 4


def padded_ws_bytes(n):
    return 256 if n < 256 else (n + 255) // 256 * 256


def test_workspace_sizes():
    """max(the log-det's partials: 4 per block of positions and image; grad_table's: Q per entry, or -- P = 1 -- one per workgroup
    and entry), in floats, padded as every per-pixel workspace is."""
    ws = _lib.lib().finc_spline_workspace_bytes
    for (B, C, H, W) in PLANS:
        plan = spline_plan(B, C, H * W)
        for K in (2, 5, 16):
            for P in (1, C * H * W):
                grads = 3 * (K + 1) * (plan["grid"] if P == 1 else P * plan["parts"])
                assert ws(B, C, H * W, K, P) == padded_ws_bytes(4 * max(4 * B * plan["outer"], grads)), (B, C, H, W, K, P)
    assert ws(0, 3, 16, 5, 1) == 256 and ws(2, 3, 16, 1, 1) == 256 and ws(2, 3, 16, 5, 7) == 256
    assert _lib.lib().finc_spline_supported_f32(1) == 0 and _lib.lib().finc_spline_supported_f32(17) == 0
    assert all(_lib.lib().finc_spline_supported_f32(K) == 1 for K in range(2, 17))


def test_version_is_120_and_a_119_library_is_told_to_rebuild(tmp_path):
    assert _lib.SPLINE_ABI_VERSION == 120 and _lib.PIXEL_PLAN_ABI_VERSION == 119
    assert _lib.lib().finc_version() >= _lib.SPLINE_ABI_VERSION
    for s in ("finc_spline_supported_f32", "finc_spline_workspace_bytes", "finc_spline_f32", "finc_spline_backward_f32",
              "finc_spline_reverse_backward_f32"):
        assert s in _lib.SYMBOLS
    out = load_stub_library(tmp_path, 119)
    assert "= 119" in out and "120" in out and "rebuild it" in out and "finc_spline_f32" in out, out


def test_pixel_plans_of_the_gpu_cases():
    """What every GPU case launches, stated by hand (tests/spline_cases.py) and by the rule written out there, against the library."""
    for (B, C, H, W), want in PLANS.items():
        assert spline_plan(B, C, H * W) == want, (B, C, H, W)
        for align in (4, 8, 16):
            assert _lib.pixel_plan("parts", "spline", B, C, H * W, align=align) == want, (B, C, H, W, align)
    for shape in MULTI_TRIP:
        assert PLANS[shape]["trips"] == 2 and shape[0] % PLANS[shape]["parts"] != 0 or PLANS[shape]["parts"] == 1


@pytest.mark.parametrize("individual", (False, True))
def test_copies_start_without_the_cached_table(individual):
    m = glow.SplineActivation((2, 3, 3), n_bins=4, tail_bound=3.0, individual_weights=individual)
    with torch.no_grad():
        tab = m._table()
        assert tab.shape == (15, 18 if individual else 1) and m._table() is tab and "_tab" in m.__dict__
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert not any(k in twin.__dict__ for k in glow.SplineActivation._derived)
        with torch.no_grad():
            assert torch.equal(twin._table(), tab) and twin._table() is not tab
    with torch.no_grad():
        m.unnormalized_widths.add_(1.0)                     # a new parameter version: rebuilt
        assert m._table() is not tab
    assert m._table().requires_grad                        # while a graph records: composed per call, under autograd


def test_fallback_paths_keep_the_lines():
    """2-D inputs, more bins than the kernels take, NaN and the range ends on the CPU lines."""
    torch.manual_seed(3)
    m = glow.SplineActivation((7,), n_bins=20, tail_bound=2.0, individual_weights=True).double()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p))
    x = torch.randn(5, 7, dtype=torch.float64) * 1.5
    x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 2.0, -2.0, float("nan"), 2.5
    with torch.no_grad():
        y, ld = m(x)
    assert y.shape == x.shape and ld.shape == (5,)
    assert y[0, 3] == 2.5 and torch.isnan(y[0, 2]) and abs(float(y[0, 0]) - 2.0) <= 1e-12 and abs(float(y[0, 1]) + 2.0) <= 1e-12
    keep = ~torch.isnan(x)
    with torch.no_grad():
        back = m.reverse(y)
    assert float((back - x)[keep].abs().max()) <= 1e-10
    # a NaN and the tails add nothing to the parameters' gradients, as in the kernels: finite, and the bits of the same batch with
    # other tail values in their places
    inrange = keep & (x.abs() <= 2.0)

    def grads(inp):
        m.zero_grad(set_to_none=True)
        out, lad = m(inp)
        (torch.where(inrange, out, torch.zeros_like(out)).sum() + lad.sum()).backward()
        return [p.grad.clone() for p in m.parameters()]
    with_nan, moved = grads(x), grads(torch.where(inrange, x, torch.full_like(x, -50.0)))
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in with_nan)
    assert all(torch.equal(a, b) for a, b in zip(with_nan, moved))
    assert torch.autograd.gradcheck(lambda v: m(v)[0], (torch.randn(2, 7, dtype=torch.float64, requires_grad=True),))


def test_flow_sequential_walks_the_layer_on_the_cpu():
    """The layer between a unit and an ActNorm: decode(encode(x)) returns x, sample_with_log_prob agrees with log_prob."""
    torch.manual_seed(5)
    C, H, W = 4, 6, 6
    spline = glow.SplineActivation((C, H, W), n_bins=5, tail_bound=4.0, individual_weights=True)
    with torch.no_grad():
        for p in spline.parameters():
            p.copy_(torch.randn_like(p))
    act = glow.ActNorm(C)
    import flow_twin
    # (the unit has no CPU path: the float64 twin runs it on the reference formulas)
    flow = flow_twin.twin_of(FlowSequential(glow.GaussianPrior((C, H, W)), FastFlowUnit(C, C, 3), spline, act))
    x = torch.randn(3, C, H, W, dtype=torch.float64)
    with torch.no_grad():
        flow.log_prob(x)                                     # ActNorm's data-dependent initialisation
        zs, lp = flow.encode(x)
        assert float((lp - flow.log_prob(x)).abs().max()) <= 1e-10
        assert float((flow.decode(zs) - x).abs().max()) <= 1e-9
        s, lp = flow.sample_with_log_prob(4)
        assert float((flow.log_prob(s) - lp).abs().max()) <= 1e-9
