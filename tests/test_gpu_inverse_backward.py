"""The backward through the unit's inverse on the GPU (include/finc.h: finc_adjoint_weights_f32, finc_lead_product_f32,
finc_inverse_backward_f32; fincflow_amd.reverse_grad): DESIGN 3.15.

Reference: float64 on the CPU, autograd through `inverse_backward_ref.solve`, a differentiable restatement of the solve (checked
against the reference's own solver in tests/test_inverse_backward_host.py).  Yardstick helpers.rel_err, bar 1e-5 (BASELINE.json's
tolerance, the bar of every inverse and backward parity test here); the whole-chain case uses the module round-trip bar of
tests/test_gpu_stream.py, 5e-5.  Every case prints what it achieved and appends it to the parity report (kind `inverse_backward`).
"""
import numpy as np
import pytest
import torch

import inverse_backward_ref as ref
from oracle import oracle
from helpers import ORDER_BITS, ORIENT_FASTFLOW, report, rel_err, same_bits
from test_gpu_bounds import F32, bank_std, check_bounds, check_isolation, orient_of, run, t

pytestmark = pytest.mark.gpu

TOL = 1e-5
CHAIN_TOL = 5e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def canon_np(ws, G, orient):
    Cq = ws.shape[0] // G
    return np.concatenate([ref.np_flip(ws[g * Cq:(g + 1) * Cq], ref.group_orient(orient, g)) for g in range(G)], 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# finc_adjoint_weights_f32
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank", [(4, 24, 3, 3), (1, 5, 2, 3), (2, 80, 3, 3), (4, 1, 3, 3), (1, 40, 4, 4)], ids=str)
def test_adjoint_weights_against_the_float64_restatement(bank, dev):
    """Every element of w_adj and lead_t within one fp32 ulp of the fp64 restatement; the result is a canonical bank; both outputs are
    written exactly within their bounds (guard bands, NaN on entry)."""
    from fincflow_amd import ops
    G, Cq, KH, KW = bank
    wc = oracle.canonicalize(oracle.make_stored_weights(G, Cq, KH, KW, orient=orient_of(G), seed=7 + Cq, std=bank_std(Cq, max(KH, KW))),
                             G, orient_of(G))
    want_adj, want_lead = ref.adjoint_bank(wc, G)
    C = G * Cq

    def call(guard):
        return run(dev, "finc_adjoint_weights_f32", lambda p, w, n: (p["wc"], p["w_adj"], p["lead_t"], G, Cq, KH, KW, None),
                   dict(wc=t(wc, dev)), dict(w_adj=(tuple(wc.shape), F32), lead_t=((C, C), F32)), None, guard)

    def judge(plain):
        worst = 0.0
        for name, want in (("w_adj", want_adj), ("lead_t", want_lead)):
            got = plain.outs[name].cpu().numpy().astype(np.float64)
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(got - want) / ulp)))
            assert np.all(np.abs(got - want) <= ulp), (bank, name, worst)
        print("adjoint bank %s: worst error %.3f ulp" % (bank, worst))
        ops.check_invariant(plain.outs["w_adj"], G)
        return worst

    check_bounds("adjoint_weights", call, None, judge, may_keep_nan=(), bank=list(bank))
    report("inverse_backward", case="adjoint_weights", bank=list(bank))


# ---------------------------------------------------------------------------------------------------------------------------------
# both gradients through the C ABI, one shape per inverse path
# ---------------------------------------------------------------------------------------------------------------------------------
def helper_wave_dims():
    from fincflow_amd import _lib
    for H, W in ((8, 16), (8, 32), (16, 16), (16, 32)):
        v = _lib.inverse_variant(129, 4, 24, H, W, 3, 3)
        if v is not None and v["sec"] == 3:
            return (129, 4, 24, H, W, 3, 3)
    raise AssertionError("no map of the issue's list reports the helper-wave form")


# name -> (dims or a function returning them, what finc_inverse_kernel_variant must say (None: the strict kernel), remainder images)
FAMILIES = {
    "helper_wave": (helper_wave_dims, dict(sec=3), 0),
    "role_split": ((8, 4, 24, 24, 32, 3, 3), dict(sec=4), 0),
    "short_step": ((4, 4, 3, 16, 16, 3, 3), dict(sec=6), 0),
    "packed_two_wave": ((130, 4, 24, 5, 80, 3, 3), dict(nw=2, npw=2), 0),
    # 80 channels in one group.  On the 5x12 map of tests/test_gpu_bounds.py the library does not answer with the big-bank kernel
    # (finc_big.hip takes maps from 16 columns up; 12 columns of such a bank go to the strict kernel): both are run, the big-bank
    # kernel on the narrowest map it takes
    "big_bank": ((3, 1, 80, 5, 16, 3, 3), dict(sec=5), 0),
    "big_bank_5x12": ((3, 1, 80, 5, 12, 3, 3), None, 0),
    "streaming_bank": ((8, 4, 12, 32, 32, 4, 4), dict(sec=7), 0),
    "remainder_launch": ((260, 4, 24, 8, 16, 3, 3), dict(), 4),
    "padded_copy": ((2, 4, 12, 9, 14, 3, 3), None, 0),
    "strict_kernel": ((2, 4, 4, 12, 12, 9, 9), None, 0),
}
# The forward's weight gradient has no kernel for filters of more than 49 taps (finc_backward_f32 answers FINC_ERR_UNSUPPORTED for a 9x9
# filter, in training the forward as well), and this change edits no grad-weight kernel: there grad_z is checked, and asking for grad_w
# is refused by name before anything is launched.
NO_GRAD_W = {"strict_kernel"}


class Problem:
    """One problem set of the backward: a stored bank, x = N(0,1) (the inverse's output), grad_x = N(0,1); the reference on the first,
    a middle and the last image."""

    def __init__(self, dev, dims, seed):
        from fincflow_amd import ops
        B, G, Cq, H, W, KH, KW = self.dims = dims
        self.orient = orient_of(G)
        self.ws = oracle.make_stored_weights(G, Cq, KH, KW, orient=self.orient, seed=seed, std=bank_std(Cq, max(KH, KW)))
        self.wc = ops.canonicalize(t(self.ws, dev), G, self.orient)
        rng = np.random.default_rng(seed + 1)
        self.shape = (B, G * Cq, H, W)
        self.x = rng.standard_normal(self.shape).astype(np.float32)
        self.gx = rng.standard_normal(self.shape).astype(np.float32)
        self.mask = ref.stored_mask(G, Cq, KH, KW, self.orient).numpy()

    def pick(self):
        B = self.dims[0]
        return sorted({0, B // 2, B - 1})

    def reference_grad_z(self):
        G = self.dims[1]
        pick = self.pick()
        x64 = torch.tensor(self.x[pick].astype(np.float64))
        z64 = ref.forward(x64, torch.tensor(self.ws.astype(np.float64)), G, self.orient).numpy()
        x_back, gz, _ = ref.reference_grads(z64, self.ws, self.gx[pick], G, self.orient)
        assert rel_err(x_back, self.x[pick]) <= 1e-10          # the restatement inverts the forward it was handed
        return gz


def backward_call(dev, p, ins, guard=False, want_gz=True, want_gw=True):
    from fincflow_amd import _lib
    d = p.dims
    outs = {}
    if want_gz:
        outs["gz"] = (p.shape, F32)
    if want_gw:
        outs["gw"] = (tuple(p.wc.shape), F32)
    return run(dev, "finc_inverse_backward_f32",
               lambda q, w, n: (q["gx"], q["x"], q["w"], q.get("gz"), q.get("gw"), *d, p.orient, w, n, None),
               dict(gx=ins["gx"], x=ins["x"] if want_gw else None, w=p.wc), outs,
               _lib.lib().finc_inverse_backward_workspace_bytes(*d), guard)


def judge_backward(p, tag, with_gw=True):
    """grad_z against the reference on the picked images and by its residual on all of them; grad_w against minus the fp64 weight
    gradient of the forward conv at (x, grad_z); exact zeros on the masked entries."""
    B, G, Cq, H, W, KH, KW = p.dims
    gz_ref = p.reference_grad_z()

    def judge(plain):
        gz = plain.outs["gz"].cpu().numpy()
        e_ref = rel_err(gz[p.pick()], gz_ref)
        back, gw_fwd = ref.forward_vjp(p.x, p.ws, gz, G, p.orient)
        e_res = rel_err(back, p.gx)
        e_gw, zeros = 0.0, True
        if with_gw:
            gw = plain.outs["gw"].cpu().numpy()
            e_gw = rel_err(gw, canon_np(-gw_fwd * p.mask, G, p.orient))
            zeros = bool(np.all(gw[canon_np(p.mask, G, p.orient) == 0] == 0))
        print("%s %s: grad_z vs reference %.3e, residual %.3e, grad_w %.3e (bar %.0e)" % (tag, p.dims, e_ref, e_res, e_gw, TOL))
        report("inverse_backward", case=tag, dims=list(p.dims), grad_z=e_ref, residual=e_res, grad_w=e_gw if with_gw else None)
        assert e_ref <= TOL and e_res <= TOL and e_gw <= TOL and zeros, (tag, e_ref, e_res, e_gw, zeros)
        return dict(grad_z=e_ref, residual=e_res, grad_w=e_gw)
    return judge


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_both_gradients_through_the_c_abi(name, dev):
    """finc_inverse_backward_f32 on the smallest shape of one inverse path: the numbers (see judge_backward), guard bands around every
    pointer and the exactly-sized workspace (all NaN on entry), bit-stable from launch to launch, each output skipped in a call of its
    own, and a NaN in one image's grad_x reaching that image's grad_z alone."""
    from fincflow_amd import _lib
    dims, want, remainder = FAMILIES[name]
    dims = dims() if callable(dims) else dims
    B, G, Cq, H, W, KH, KW = dims
    v = _lib.inverse_variant(*dims)
    if want is None:
        assert v is None and _lib.lib().finc_inverse_algo_for(Cq, H, W, KH, KW) == _lib.ALGO["strict"], (name, v)
        if name == "padded_copy":             # the width alone keeps it from the MFMA kernel: AUTO solves the zero-padded copy
            assert W % 4 and _lib.lib().finc_inverse_algo_for(Cq, H, (W + 7) // 8 * 8, KH, KW) == _lib.ALGO["mfma"]
            assert _lib.lib().finc_inverse_workspace_bytes(*dims) > _lib.lib().finc_workspace_bytes(G, Cq, KH, KW)
    else:
        assert v is not None and all(v[k] == x for k, x in want.items()), (name, v, want)
    assert _lib.inverse_remainder_images(*dims) == remainder, name
    p = Problem(dev, dims, seed=sum(dims))
    ins = dict(gx=t(p.gx, dev), x=t(p.x, dev))
    if name in NO_GRAD_W:
        assert KH * KW > 49
        with pytest.raises(_lib.FincError, match="does not support"):
            backward_call(dev, p, ins)
        check_bounds("inverse_backward_" + name, lambda guard: backward_call(dev, p, ins, guard, want_gw=False), v,
                     judge_backward(p, name, with_gw=False), may_keep_nan=(), dims=list(dims))
        return
    both = check_bounds("inverse_backward_" + name, lambda guard: backward_call(dev, p, ins, guard), v, judge_backward(p, name),
                        may_keep_nan=(), dims=list(dims))
    only_gz = backward_call(dev, p, ins, guard=True, want_gw=False)
    only_gw = backward_call(dev, p, ins, guard=True, want_gz=False)
    assert not only_gz.bad and not only_gw.bad, (only_gz.bad, only_gw.bad)
    assert same_bits(only_gz.outs["gz"], both.outs["gz"]) and same_bits(only_gw.outs["gw"], both.outs["gw"])
    if B > 1:
        spots = [("gx", b, {"gz": b}) for b in dict.fromkeys((B // 2, B - 1, 0))]
        check_isolation(dev, "inverse_backward_" + name, lambda i: backward_call(dev, p, i, want_gw=False), ins, spots, v,
                        values=(float("nan"),), dims=list(dims))
    assert _lib.hlp_timeouts() == 0 and not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# a channel count without a mix instantiation: the grouped lead kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(3, 4, 5, 6, 8, 3, 3), (3, 4, 5, 5, 7, 3, 3), (2, 1, 40, 4, 12, 3, 3), (2, 1, 40, 3, 5, 3, 3)], ids=str)
def test_the_grouped_lead_kernel(dims, dev):
    """C = 20 and C = 40 have no finc_mix instantiation: the lead product runs on the grouped kernel, in 16-byte pieces (HW % 4 == 0)
    and in dwords.  The product alone against float64, in place and inside guard bands; then the whole backward."""
    from fincflow_amd import _lib
    B, G, Cq, H, W, KH, KW = dims
    C = G * Cq
    assert _lib.lib().finc_mix_supported_f32(C) == 0
    p = Problem(dev, dims, seed=sum(dims))
    _, lead64 = ref.adjoint_bank(canon_np(p.ws, G, p.orient), G)
    lead = t(lead64.astype(np.float32), dev)
    want = np.einsum("oc,bchw->bohw", lead64.astype(np.float32).astype(np.float64), p.gx.astype(np.float64))

    def call(guard):
        return run(dev, "finc_lead_product_f32", lambda q, w, n: (q["v"], q["lead"], B, G, Cq, H * W, None),
                   dict(v=t(p.gx, dev), lead=lead), dict(out=(p.shape, F32)), None, guard, alias=dict(out="v"))

    def judge(plain):
        e = rel_err(plain.outs["out"].cpu().numpy(), want)
        print("grouped lead product %s: %.3e" % (dims, e))
        report("inverse_backward", case="grouped_lead", dims=list(dims), err=e)
        assert e <= 1e-6, e                  # Cq fused multiply-adds in fp32 on N(0,1) data
        return e

    check_bounds("lead_product", call, None, judge, may_keep_nan=(), dims=list(dims))
    ins = dict(gx=t(p.gx, dev), x=t(p.x, dev))
    check_bounds("inverse_backward_grouped_lead", lambda guard: backward_call(dev, p, ins, guard), None, judge_backward(p, "grouped_lead"),
                 may_keep_nan=(), dims=list(dims))


# ---------------------------------------------------------------------------------------------------------------------------------
# the modules under reverse_grad()
# ---------------------------------------------------------------------------------------------------------------------------------
def module_case(kind, dev):
    """(module, its stored weights in reference order, G, orient, bias or None, input shape)."""
    from fincflow_amd import CINCFlowUnit, FastFlowUnit, PaddedConv2d
    torch.manual_seed(11)
    if kind == "unit":
        m = FastFlowUnit(12, 12, 3).to(dev)
        return m, m._weights(), 4, ORIENT_FASTFLOW, None, (2, 12, 9, 12)
    if kind == "cinc":
        m = CINCFlowUnit(8, 8, 3).to(dev)
        return m, [m.conv_tl.conv.weight], 1, 0, None, (2, 8, 7, 8)
    if kind == "bias":
        m = PaddedConv2d(5, 5, (3, 3), bias=True, order="BL").to(dev)
        with torch.no_grad():
            m.bias.copy_(torch.linspace(-0.5, 0.5, 5))
        return m, [m.conv.weight], 1, ORDER_BITS["BL"], m.bias, (2, 5, 7, 8)
    m = PaddedConv2d(5, 5, (3, 3), order=kind).to(dev)
    return m, [m.conv.weight], 1, ORDER_BITS[kind], None, (2, 5, 7, 8)


def module_reverse(m, z):
    out = m.reverse(z)
    return out[0] if isinstance(out, tuple) else out


def module_reference(weights, bias, G, orient, z, g):
    ws = np.concatenate([w.detach().cpu().numpy() for w in weights], 0).astype(np.float64)
    zin = z.astype(np.float64) - (0 if bias is None else bias.detach().cpu().numpy().astype(np.float64).reshape(1, -1, 1, 1))
    _, gz, gw = ref.reference_grads(zin, ws, g, G, orient)
    Cq, KH, KW = ws.shape[1:]
    return gz, gw, ref.stored_mask(G, Cq, KH, KW, orient).numpy()


@pytest.mark.parametrize("kind", ["unit", "TL", "TR", "BL", "BR", "bias", "cinc"])
def test_modules_are_differentiable_under_reverse_grad(kind, dev):
    import fincflow_amd
    m, weights, G, orient, bias, shape = module_case(kind, dev)
    rng = np.random.default_rng(5)
    z_np, g_np = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    g = t(g_np, dev)
    params = list(weights) + ([bias] if bias is not None else [])
    for step in range(2):                      # the second round: after an in-place SGD step, at the new weight version
        with torch.no_grad():
            x_plain = module_reverse(m, t(z_np, dev))
        z = t(z_np, dev).requires_grad_(True)
        with fincflow_amd.reverse_grad():
            x = module_reverse(m, z)
            x_again = module_reverse(m, z)
        assert x.requires_grad and same_bits(x.detach(), x_plain)
        grads = torch.autograd.grad(x, [z] + params, g)
        gz_ref, gw_ref, mask = module_reference(weights, bias, G, orient, z_np, g_np)
        gw = np.concatenate([gr.cpu().numpy() for gr in grads[1:1 + len(weights)]], 0)
        e_z, e_w = rel_err(grads[0].cpu().numpy(), gz_ref), rel_err(gw, gw_ref * mask)
        e_b = rel_err(grads[-1].cpu().numpy(), -gz_ref.sum((0, 2, 3))) if bias is not None else 0.0
        print("%s step %d: grad_z %.3e grad_w %.3e grad_bias %.3e" % (kind, step, e_z, e_w, e_b))
        report("inverse_backward", case="module_" + kind, step=step, grad_z=e_z, grad_w=e_w, grad_bias=e_b)
        assert e_z <= TOL and e_w <= TOL and e_b <= TOL, (kind, step, e_z, e_w, e_b)
        assert np.all(gw[mask == 0] == 0), "masked entries must be exactly 0"
        # z alone, weights alone: the same numbers, and nothing is computed for an input that did not ask
        (gz_only,) = torch.autograd.grad(x_again, [z], g, retain_graph=True)
        assert same_bits(gz_only, grads[0])
        with fincflow_amd.reverse_grad():
            x_w = module_reverse(m, t(z_np, dev))
        assert x_w.requires_grad
        gws_only = torch.autograd.grad(x_w, list(weights), g)
        assert all(same_bits(a, b) for a, b in zip(gws_only, grads[1:1 + len(weights)]))
        with torch.no_grad():
            for prm, gr in zip(params, grads[1:]):
                prm.sub_(0.05 * gr)


def test_reverse_level1_is_differentiable_too(dev):
    import fincflow_amd
    m, weights, G, orient, _, shape = module_case("unit", dev)
    rng = np.random.default_rng(6)
    z_np, g_np = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    z = t(z_np, dev).requires_grad_(True)
    with fincflow_amd.reverse_grad():
        x = m.reverse_level1(z)
    grads = torch.autograd.grad(x, [z] + list(weights), t(g_np, dev))
    gz_ref, gw_ref, mask = module_reference(weights, None, G, orient, z_np, g_np)
    gw = np.concatenate([gr.cpu().numpy() for gr in grads[1:]], 0)
    assert rel_err(grads[0].cpu().numpy(), gz_ref) <= TOL and rel_err(gw, gw_ref * mask) <= TOL


def test_fp64_and_cpu_tensors_raise_inside_the_context(dev):
    import fincflow_amd
    from fincflow_amd import FastFlowUnit, _lib
    unit = FastFlowUnit(12, 12, 3).to(dev)
    with fincflow_amd.reverse_grad():
        with pytest.raises(_lib.FincError, match="fp32"):
            unit.reverse(torch.randn(1, 12, 4, 4, device=dev, dtype=torch.float64, requires_grad=True))
        with pytest.raises(_lib.FincError, match="fp32"):
            unit.reverse(torch.randn(1, 12, 4, 4, requires_grad=True))


def test_outside_the_context_nothing_changed(dev):
    from fincflow_amd import FastFlowUnit, ops
    torch.manual_seed(3)
    unit = FastFlowUnit(12, 12, 3).to(dev)
    assert all(w.requires_grad for w in unit._weights()) and torch.is_grad_enabled() and not ops.reverse_grad_enabled()
    z = torch.randn(2, 12, 9, 12, device=dev)
    want = ops.finc_inverse(z, ops.canonicalize(torch.cat([w.detach() for w in unit._weights()]), 4, ORIENT_FASTFLOW))
    for zin in (z, z.clone().requires_grad_(True)):
        x = unit.reverse(zin)
        assert not x.requires_grad and x.grad_fn is None
        assert x.cpu().numpy().shape == (2, 12, 9, 12)
        assert rel_err(x.cpu().numpy(), want.cpu().numpy()) <= TOL
        assert same_bits(x, unit._cache.inverse(z, *unit._cache_args()))
    with ops.reverse_grad():
        assert ops.reverse_grad_enabled()
        with ops.reverse_grad():
            pass
        assert ops.reverse_grad_enabled()
        with torch.no_grad():
            assert not unit.reverse(z).requires_grad        # nothing records: the plain path
    assert not ops.reverse_grad_enabled()


def test_the_adjoint_bank_is_cached_per_weight_version(dev, monkeypatch):
    """The library calls of a backward, by name: the adjoint bank and its pack once per weight version, then one solve, one lead
    product, the grad-weight and its sign per backward (tests/test_gpu_unit_host.py pins the calls of every other method this way)."""
    import fincflow_amd
    from fincflow_amd import FastFlowUnit, _lib
    from test_gpu_unit_host import Recorder
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    torch.manual_seed(4)
    unit = FastFlowUnit(16, 16, 3).to(dev)
    g = torch.randn(2, 16, 8, 8, device=dev)
    FORWARD = ["finc_inverse_packed_f32"]
    SOLVE = ["finc_inverse_packed_f32", "finc_lead_product_f32"]
    GRADW = ["finc_backward_f32", "finc_negate_f32", "finc_canonicalize_weights_f32"]
    for _ in range(2):
        z = torch.randn(2, 16, 8, 8, device=dev, requires_grad=True)
        with fincflow_amd.reverse_grad():
            x = unit.reverse(z)
        assert rec.take() == ["finc_canonicalize_weights_f32", "finc_check_invariant_f32", "finc_pack_inverse_weights_f32"] + FORWARD
        torch.autograd.grad(x, [z] + unit._weights(), g)
        assert rec.take() == ["finc_adjoint_weights_f32", "finc_pack_inverse_weights_f32"] + SOLVE + GRADW
        # the weights alone (the solve is needed all the same), then z alone (no grad-weight): what the Function's inputs ask for
        with fincflow_amd.reverse_grad():
            x = unit.reverse(z.detach())
        torch.autograd.grad(x, unit._weights(), g)
        assert rec.take() == FORWARD + SOLVE + GRADW
        unit.requires_grad_(False)
        with fincflow_amd.reverse_grad():
            x = unit.reverse(z)
        torch.autograd.grad(x, [z], g)
        assert rec.take() == FORWARD + SOLVE
        unit.requires_grad_(True)
        with torch.no_grad():
            unit.conv_tr.conv.weight[:, :, 1, 1].mul_(1.5)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole chain, by the inverse-function identity
# ---------------------------------------------------------------------------------------------------------------------------------
def build_chain(dev):
    from fincflow_amd import glow
    torch.manual_seed(0)
    np.random.seed(0)
    model = glow.create_model(num_blocks=2, block_size=2, actnorm=True, split_prior=False, image_size=(3, 16, 16), preprocess=False,
                              coupling_width=32).to(dev)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, glow.ActNorm):
                m.log_scale.copy_(0.1 * torch.randn(m.n_dims, generator=gen))
                m.translation.copy_(0.1 * torch.randn(m.n_dims, generator=gen))
                m.mark_initialized()
            elif isinstance(m, glow.Conv2dZero):
                m.weight.copy_(0.05 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.01 * torch.randn(m.bias.shape, generator=gen))
                m.logs.copy_(0.01 * torch.randn(m.logs.shape, generator=gen))
    return model


def test_the_whole_chain_by_the_inverse_function_identity(dev):
    """x = reverse(z) and z = forward(x) are inverse functions, so their Jacobians are inverse matrices: with g_z = d<g, x>/dz, the
    forward chain's vector-Jacobian product at x with g_z is g again, and a parameter's gradient through the reverse chain is minus its
    gradient through the forward chain at x (detached) with grad_output g_z.  No CPU model is needed."""
    import fincflow_amd
    model = build_chain(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    torch.manual_seed(2)
    z = torch.randn(4, 48, 4, 4, device=dev, requires_grad=True)
    g = torch.randn(4, 3, 16, 16, device=dev)
    with fincflow_amd.reverse_grad():
        x = model._reverse_chain(z, None)
    assert x.requires_grad and x.shape == g.shape
    grads = torch.autograd.grad(x, [z] + params, g, allow_unused=True)
    g_z, g_rev = grads[0], grads[1:]
    xd = x.detach().requires_grad_(True)
    z_fwd = model.forward(xd)[0]
    fwd = torch.autograd.grad(z_fwd, [xd] + params, g_z.detach(), allow_unused=True)
    e_x = rel_err(fwd[0].cpu().numpy(), g.cpu().numpy())
    worst, n = 0.0, 0
    for a, b in zip(g_rev, fwd[1:]):
        assert (a is None) == (b is None)
        if a is not None and float(b.abs().max()) > 0:
            worst = max(worst, rel_err(a.cpu().numpy(), -b.cpu().numpy()))
            n += 1
    print("whole chain: forward VJP gives g back to %.3e; worst of %d parameter gradients %.3e (bar %.0e)" % (e_x, n, worst, CHAIN_TOL))
    report("inverse_backward", case="whole_chain", vjp=e_x, parameters=n, worst_parameter=worst)
    assert n >= 20 and e_x <= CHAIN_TOL and worst <= CHAIN_TOL, (e_x, worst)


def test_rsample_returns_an_attached_sample(dev):
    model = build_chain(dev)
    x = model.rsample(4)
    assert x.requires_grad and x.shape == (4, 3, 16, 16) and torch.is_grad_enabled()
    x.square().mean().backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    x2, _ = model.sample(4)
    assert not x2.requires_grad
