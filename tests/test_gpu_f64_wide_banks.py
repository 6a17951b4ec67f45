"""Float64 on the matrix cores for the banks of 29 .. 64 channels (3x3) and 33 .. 64 (2x2): finc_f64.hip's M-split family -- the
inverse over a workgroup's waves with one barrier per step, the forward / grad-input and the grad-weight with the 16-row output tile
as one more launch dimension -- through ops and the C ABI, and the modules that reach these widths.

References: the inverse against oracle.inverse_f64 per group in its own orientation (solve_parallel_mc.pyx:77-126; the strict kernel
bit-exact beside it, as tests/test_gpu_round5.py), everything else against float64 autograd through F.pad + F.conv2d on the CPU.  Both
sides are float64, so the bar is the project's fp64 bar, helpers.rel_err <= 1e-12.  Every case first asserts ON THE CPU that the
worst-case rounding bound N * 2^-53 * max(sum |terms|) / max |reference| of its sums is below the bar, and for the inverse that the
forward of the oracle's solution returns z within 1e-13: a shape whose conditioning alone would eat the bar fails there, before the
GPU is judged.  The measured worst values go to the parity report (kind `f64_wide_banks`).

The shapes are the smallest at which each mechanism can go wrong; tests/test_f64_wide_banks_host.py states their launch plans by hand.
`algo="mfma"` insists on the matrix-core form: before these kernels existed it refused every shape below.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import ORDER_BITS, rel_err, report, same_bits
from test_gpu_bounds import F64, check_bounds, check_isolation, orient_of, run
from test_gpu_f64_backward import bank64, canonical_mask, conv_cpu, grads_cpu, on_side_stream, t, unit64, unit_reference
from test_gpu_round5 import _oracle_f64_unit

pytestmark = pytest.mark.gpu

BAR = 1e-12
ROUND_TRIP = 1e-13
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def case(B, G, Cq, H, W, K=3, orient=None):
    return (B, G, Cq, H, W, K, K), (orient_of(G) if orient is None else orient)


CASES = {
    "two_tiles_5x7": case(2, 1, 32, 5, 7),                   # two full tiles, one band, W < 16; two problems in one workgroup
    "odd_problems_5x7": case(3, 1, 30, 5, 7),                # three problems, two per workgroup: the last workgroup's second slot is empty
    "pad32_6x18": case(2, 4, 29, 6, 18),                     # pads to 32: masked channels in the last k-step; the strip seam at 16
    "three_waves_17x17": case(3, 4, 48, 17, 17),             # two bands through the shared FIFO, H * W odd: the 8-byte stores
    "pad48_9x16": case(2, 1, 40, 9, 16),                     # pads to 48, the 32-byte store path
    "four_waves_9x20": case(2, 4, 64, 9, 20),                # W > 16 at W % 4 == 0
    "four_waves_4x4": case(1, 2, 64, 4, 4),                  # the map is barely larger than the filter
    "k2_c48_9x16": case(2, 2, 48, 9, 16, 2),
    "k2_pad48_4x5": case(1, 4, 36, 4, 5, 2),
    "row_chunks_17x17": case(1, 1, 48, 17, 17),              # one problem: the grad-weight cuts its slab into four row chunks
    "orient_TL": case(2, 1, 48, 6, 18, orient=ORDER_BITS["TL"]),
    "orient_TR": case(2, 1, 48, 6, 18, orient=ORDER_BITS["TR"]),
    "orient_BL": case(2, 1, 48, 6, 18, orient=ORDER_BITS["BL"]),
    "orient_BR": case(2, 1, 48, 6, 18, orient=ORDER_BITS["BR"]),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """Operands, the float64 CPU references and the worst-case bounds of one case: computed once, shared, never written to."""
    dims, orient = CASES[name]
    B, G, Cq, H, W, KH, KW = dims
    rng = np.random.default_rng(sum(dims) + orient)
    x, gz, zin = (rng.standard_normal((B, G * Cq, H, W)) for _ in range(3))
    wc = bank64(G, Cq, KH, KW, seed=7 + Cq)
    assert np.any(wc != wc.astype(np.float32).astype(np.float64))
    mask = canonical_mask(G, Cq, KH, KW)
    z, gx, gw = grads_cpu(x, wc, gz, G, orient)
    gw = gw * mask
    za, gxa, gwa = grads_cpu(np.abs(x), np.abs(wc), np.abs(gz), G, orient)
    bound = dict(z=Cq * KH * KW * EPS * za.max() / np.abs(z).max(), gx=Cq * KH * KW * EPS * gxa.max() / np.abs(gx).max(),
                 gw=B * H * W * EPS * (gwa * mask).max() / np.abs(gw).max())
    # the solve: the oracle's solution, the sums of absolute terms of the recurrence at that solution, and the way back
    inv = _oracle_f64_unit(zin, wc, G, orient, Cq)
    wt = torch.from_numpy(wc)
    terms = conv_cpu(torch.from_numpy(np.abs(inv)), wt.abs(), G, orient).numpy()
    bound["inv"] = Cq * KH * KW * EPS * terms.max() / np.abs(inv).max()
    round_trip = rel_err(conv_cpu(torch.from_numpy(inv), wt, G, orient).numpy(), zin)
    for v in (x, gz, zin, wc, z, gx, gw, inv, mask):
        v.setflags(write=False)
    return dict(dims=dims, orient=orient, x=x, gz=gz, zin=zin, wc=wc, mask=mask, z=z, gx=gx, gw=gw, inv=inv, bound=bound,
                round_trip=round_trip)


def judge(name, tag, got, keys):
    """On the CPU first: every judged sum's bound is below the bar (the solve: and its way back within 1e-13).  Then the GPU."""
    p, errs = problem(name), {}
    for k in keys:
        assert p["bound"][k] < BAR, (name, k, "the worst-case bound of this shape is not below the bar", p["bound"][k])
        if k == "inv":
            assert p["round_trip"] <= ROUND_TRIP, (name, "the oracle's own solution does not return z", p["round_trip"])
    for k in keys:
        errs[k] = rel_err(got[k].cpu().numpy(), p[k])
        print("f64_wide_banks %s %s %s: %.3e (bound %.3e)" % (name, tag, k, errs[k], p["bound"][k]))
    report("f64_wide_banks", case=name, tag=tag, dims=list(p["dims"]), err=errs, bound={k: float(p["bound"][k]) for k in keys},
           round_trip=float(p["round_trip"]) if "inv" in keys else None)
    for k in keys:
        assert errs[k] <= BAR, (name, tag, k, errs[k])
    if "gw" in keys:
        masked = got["gw"].cpu().view(torch.int64)[torch.from_numpy(p["mask"] == 0)]
        assert masked.numel() > 0 and bool((masked == 0).all()), (name, tag, "a masked entry of grad_w is not +0.0")
    return errs


def assert_family_2(dims):
    from fincflow_amd import _lib
    p = _lib.f64_plan(*dims)
    assert p["family"] == 2 and p["waves"] == p["cqp"] // 16 in (2, 3, 4), p
    return p


# ---------------------------------------------------------------------------------------------------------------------------------
# the inverse
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_inverse_on_the_wide_banks(name, dev):
    """`mfma` is honoured (it refused these shapes before the M-split family) and `auto` takes the same kernel: within the bar of the
    oracle's fp64 solve, the strict kernel bit-exact with it; the same bits on a second call and on a side stream."""
    from fincflow_amd import _lib, ops
    p = problem(name)
    G, orient = p["dims"][1], p["orient"]
    assert_family_2(p["dims"])
    z, wc = t(p["zin"], dev), t(p["wc"], dev)
    ops.check_invariant(wc, G)
    strict = ops.finc_inverse(z, wc, G, orient, algo="strict")
    assert np.array_equal(strict.cpu().numpy(), p["inv"]), (name, "the strict kernel is not bit-exact with the oracle")
    fast = ops.finc_inverse(z, wc, G, orient, algo="mfma")
    judge(name, "inverse_mfma", dict(inv=fast), ("inv",))
    auto = ops.finc_inverse(z, wc, G, orient)
    assert same_bits(fast, auto), (name, "auto does not take the matrix-core kernel")
    assert same_bits(fast, ops.finc_inverse(z, wc, G, orient, algo="mfma")), (name, "not bit-stable from call to call")
    assert same_bits(fast, on_side_stream(dev, lambda: ops.finc_inverse(z, wc, G, orient, algo="mfma"))), (name, "a side stream gives other bits")
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# forward, grad-input, grad-weight
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_and_backward_on_the_wide_banks(name, dev):
    from fincflow_amd import _lib, ops
    p = problem(name)
    G, orient = p["dims"][1], p["orient"]
    assert_family_2(p["dims"])
    x, gz, wc = t(p["x"], dev), t(p["gz"], dev), t(p["wc"], dev)
    zf = ops.finc_forward(x, wc, G, orient, algo="mfma")
    judge(name, "forward_mfma", dict(z=zf), ("z",))
    assert same_bits(zf, ops.finc_forward(x, wc, G, orient)), (name, "auto does not take the matrix-core kernel")
    assert same_bits(zf, on_side_stream(dev, lambda: ops.finc_forward(x, wc, G, orient, algo="mfma")))
    both = lambda: ops.finc_backward(gz, x, wc, G, orient)
    gx, gw = both()
    judge(name, "backward", dict(gx=gx, gw=gw), ("gx", "gw"))
    gx2, gw2 = both()
    assert same_bits(gx, gx2) and same_bits(gw, gw2), (name, "not bit-stable from call to call")
    gxs, gws = on_side_stream(dev, both)
    assert same_bits(gx, gxs) and same_bits(gw, gws), (name, "a side stream gives other bits")
    assert same_bits(gx, ops.finc_backward(gz, None, wc, G, orient, need_gw=False)[0])
    assert same_bits(gw, ops.finc_backward(gz, x, wc, G, orient, need_gx=False)[1])
    assert not _lib.fault_pending()


def test_the_matrix_core_backward_is_not_the_direct_one(dev):
    """With the workspace withheld the same call runs the direct kernels: within the bar too, but other bits -- so the call above did
    take the matrix-core kernels."""
    name = "pad32_6x18"
    p = problem(name)
    ins = dict(gz=t(p["gz"], dev), x=t(p["x"], dev))
    fast, direct = backward_call(dev, name, ins), backward_call(dev, name, ins, workspace=False)
    judge(name, "direct", direct.outs, ("gx", "gw"))
    assert not same_bits(fast.outs["gx"], direct.outs["gx"]) and not same_bits(fast.outs["gw"], direct.outs["gw"])


# ---------------------------------------------------------------------------------------------------------------------------------
# `mfma` still refuses what has no matrix-core kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 28, 5, 5, 3, 3), (2, 4, 48, 6, 6, 5, 5), (1, 4, 65, 4, 4, 3, 3)], ids=lambda d: "Cq%d_k%d" % (d[2], d[5]))
def test_mfma_still_refuses_the_banks_without_a_kernel(dims, dev):
    from fincflow_amd import _lib, ops
    B, G, Cq, H, W, KH, KW = dims
    assert _lib.f64_plan(*dims)["family"] == 0
    wc = t(bank64(G, Cq, KH, KW, seed=3), dev)
    z = torch.randn(B, G * Cq, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(dev)
    for fn in (ops.finc_inverse, ops.finc_forward):
        with pytest.raises((ValueError, _lib.FincError)):
            fn(z, wc, G, orient_of(G), algo="mfma")
        assert bool(torch.isfinite(fn(z, wc, G, orient_of(G))).all())          # auto: the reference-order kernel
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# guard bands and problem isolation
# ---------------------------------------------------------------------------------------------------------------------------------
def inverse_call(dev, name, ins, guard=False):
    from fincflow_amd import _lib
    p = problem(name)
    dims, orient = p["dims"], p["orient"]
    B, G, Cq, H, W, KH, KW = dims
    ws = _lib.lib().finc_f64_workspace_bytes(G, Cq, KH, KW)
    return run(dev, "finc_inverse_f64_algo", lambda q, w, n: (q["act"], q["w"], q["out"], *dims, orient, _lib.ALGO["mfma"], w, n, None),
               dict(act=ins["act"], w=t(p["wc"], dev)), dict(out=((B, G * Cq, H, W), F64)), ws, guard)


def backward_call(dev, name, ins, guard=False, workspace=True, want=("gx", "gw")):
    from fincflow_amd import _lib
    p = problem(name)
    dims, orient = p["dims"], p["orient"]
    B, G, Cq, H, W, KH, KW = dims
    ws = _lib.lib().finc_backward_f64_workspace_bytes(*dims) if workspace else None
    outs = {k: v for k, v in dict(gx=((B, G * Cq, H, W), F64), gw=((G * Cq, Cq, KH, KW), F64)).items() if k in want}
    return run(dev, "finc_backward_f64", lambda q, w, n: (q["gz"], q["x"], q["w"], q.get("gx"), q.get("gw"), *dims, orient, w, n, None),
               dict(gz=ins["gz"], x=ins["x"], w=t(p["wc"], dev)), outs, ws, guard)


def corner_slabs(B, G, Cq):
    return sorted(set((b, g * Cq) for b in (0, B // 2, B - 1) for g in (0, G - 1)))


@pytest.mark.parametrize("name", ["three_waves_17x17", "pad32_6x18"])
def test_inverse_guard_bands_and_isolation(name, dev):
    """Every pointer between NaN guards, the packed bank's workspace NaN on entry at its exact size; a poisoned (image, group) slab
    of z reaches its own slab of x and nothing else -- the second problem of a shared workgroup and the waves of one problem included."""
    from fincflow_amd import _lib
    p = problem(name)
    B, G, Cq, H, W, KH, KW = p["dims"]
    act = t(p["zin"], dev)
    variant = dict(family=2, algo="mfma")
    check_bounds("f64_wide_inverse_" + name, lambda guard: inverse_call(dev, name, dict(act=act), guard), variant,
                 lambda plain: judge(name, "guarded_inverse", dict(inv=plain.outs["out"]), ("inv",)), may_keep_nan=(), dims=list(p["dims"]))
    spots = [("act", (b, slice(c0, c0 + Cq)), {"out": (b, slice(c0, c0 + Cq))}) for b, c0 in corner_slabs(B, G, Cq)]
    check_isolation(dev, "f64_wide_inverse_" + name, lambda ins: inverse_call(dev, name, ins), dict(act=act), spots, variant, dims=list(p["dims"]))
    assert not _lib.fault_pending()


def test_backward_guard_bands_and_isolation(dev):
    from fincflow_amd import _lib
    name = "pad32_6x18"
    p = problem(name)
    B, G, Cq, H, W, KH, KW = p["dims"]
    ins = dict(gz=t(p["gz"], dev), x=t(p["x"], dev))
    variant = dict(family=2)
    check_bounds("f64_wide_backward_" + name, lambda guard: backward_call(dev, name, ins, guard), variant,
                 lambda plain: judge(name, "guarded_backward", plain.outs, ("gx", "gw")), may_keep_nan=(), dims=list(p["dims"]))
    spots = []
    for b, c0 in corner_slabs(B, G, Cq):
        s, rows = (b, slice(c0, c0 + Cq)), slice(c0, c0 + Cq)
        spots.append(("gz", s, {"gx": s, "gw": rows}))
        spots.append(("x", s, {"gx": None, "gw": rows}))
    check_isolation(dev, "f64_wide_backward_" + name, lambda i: backward_call(dev, name, i), ins, spots, variant, dims=list(p["dims"]))
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# the modules that reach these widths
# ---------------------------------------------------------------------------------------------------------------------------------
MODULES = {"fastflow_192": ("fastflow", 192, 4, (2, 192, 6, 6)), "cinc_48": ("cinc", 48, 1, (2, 48, 6, 18))}


def module_of(kind, C, dev):
    from fincflow_amd import CINCFlowUnit, FastFlowUnit
    return unit64(FastFlowUnit if kind == "fastflow" else CINCFlowUnit, C, dev, seed=11)


@pytest.mark.parametrize("name", sorted(MODULES))
def test_modules_at_the_wide_banks(name, dev):
    """A float64 unit of 48 channels per group: forward, every parameter's gradient and the input's against float64 autograd of the
    CPU twin, the reverse of the twin's z against x (the solve) and the round trip, all under the fp64 bar, on the M-split kernels."""
    from fincflow_amd import _lib
    kind, C, G, shape = MODULES[name]
    assert_family_2((shape[0], G, C // G, shape[2], shape[3], 3, 3))
    unit = module_of(kind, C, dev)
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(*shape, dtype=torch.float64, generator=gen).to(dev)
    gz = torch.randn(*shape, dtype=torch.float64, generator=gen).to(dev)
    xg = x.clone().requires_grad_(True)
    z = unit(xg)[0]
    assert z.dtype == torch.float64
    z.backward(gz)
    z_ref, gx_ref, gp_ref = unit_reference(unit, x, gz)
    errs = dict(z=rel_err(z.detach().cpu().numpy(), z_ref.numpy()), gx=rel_err(xg.grad.cpu().numpy(), gx_ref.numpy()))
    for n, q in unit.named_parameters():
        assert q.grad is not None and q.grad.dtype == torch.float64, n
        errs[n] = rel_err(q.grad.cpu().numpy(), gp_ref[n].numpy())
    with torch.no_grad():
        solve = unit.reverse(z_ref.to(dev))
        solve = solve[0] if isinstance(solve, tuple) else solve
        back = unit.reverse(z.detach())
        back = back[0] if isinstance(back, tuple) else back
    errs["solve"] = rel_err(solve.cpu().numpy(), x.cpu().numpy())
    errs["round_trip"] = rel_err(back.cpu().numpy(), x.cpu().numpy())
    print("f64_wide_banks module %s: %s" % (name, errs))
    report("f64_wide_banks", case="module_" + name, err=errs)
    assert all(e <= BAR for e in errs.values()), errs
    assert not _lib.fault_pending()


def test_gradcheck_with_respect_to_the_input(dev):
    from fincflow_amd import _lib
    kind, C, G, _ = MODULES["cinc_48"]
    assert_family_2((1, G, C // G, 4, 5, 3, 3))
    unit = module_of(kind, C, dev)
    for q in unit.parameters():
        q.requires_grad_(False)
    x = torch.randn(1, C, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: unit(v)[0], (x,))
    assert not _lib.fault_pending()
