"""Host side of the backward through the unit's inverse (include/finc.h: finc_adjoint_weights_f32, finc_lead_product_f32,
finc_negate_f32, finc_inverse_backward_workspace_bytes, finc_inverse_backward_f32): the symbols, the order of the status codes on
fake pointers (every refusal happens before any HIP call, so no GPU is needed), the workspace bound, and the mathematics the library's
route rests on, pinned in float64 against autograd through a differentiable restatement of the solve.
"""
import ctypes

import numpy as np
import pytest

import inverse_backward_ref as ref
from helpers import ORDER_BITS, ORIENT_FASTFLOW, fake_ptr, golden, rel_err, unit_stored_weights
from fincflow_amd import _lib

OK, NULL, DIMS, UNSUPPORTED, WORKSPACE, LAUNCH, INVARIANT, ALIGN = range(8)
NEW = ("finc_adjoint_weights_f32", "finc_lead_product_f32", "finc_negate_f32", "finc_inverse_backward_workspace_bytes",
       "finc_inverse_backward_f32")
# five distinct 256-byte aligned fake addresses
GX, X, WC, GZ, GW, WS = (fake_ptr(0x1000 * k) for k in range(1, 7))
SHAPE = (2, 4, 6, 8, 8, 3, 3)          # B, G, Cq, H, W, KH, KW


def test_the_new_symbols_are_declared_exported_and_bound():
    import os
    import re
    from helpers import REPO
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "finc.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/finc.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    assert _lib.lib().finc_version() >= _lib.INVERSE_BACKWARD_ABI_VERSION == 107


def test_an_older_library_is_refused_by_name(tmp_path):
    from helpers import load_stub_library
    out = load_stub_library(tmp_path, 106)
    assert "= 106" in out and "107" in out and "finc_inverse_backward_f32" in out, out


def call(gx=GX, x=X, wc=WC, gz=GZ, gw=GW, shape=SHAPE, ws=WS, ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.finc_inverse_backward_workspace_bytes(*shape) if min(shape) > 0 else 1 << 20
    return L.finc_inverse_backward_f32(gx, x, wc, gz, gw, *shape, ORIENT_FASTFLOW, ws, ws_bytes, None)


def test_inverse_backward_refuses_in_the_documented_order():
    # 1. NULL pointers (before the dims: a zero batch beside them is still status 1)
    bad = (0,) + SHAPE[1:]
    assert call(gx=None) == NULL and call(wc=None) == NULL and call(gx=None, shape=bad) == NULL
    assert call(gz=None, gw=None) == NULL and call(gz=None, gw=None, shape=bad) == NULL
    assert call(x=None) == NULL                       # grad_w needs the inverse's output ...
    assert call(x=None, gw=None, ws=None) == WORKSPACE   # ... grad_z alone does not (the next refusal in line is the workspace's)
    # 2. the dims (before the alignment: a misaligned pointer beside them is still status 2)
    off = fake_ptr(0x1002)
    for k in range(7):
        for v in (0, -1):
            s = SHAPE[:k] + (v,) + SHAPE[k + 1:]
            assert call(shape=s) == DIMS and call(gx=off, shape=s) == DIMS, s
    assert call(shape=(2, 17, 6, 8, 8, 3, 3)) == DIMS and call(shape=(2, 4, 257, 8, 8, 3, 3)) == DIMS
    assert call(shape=(2, 16, 256, 8, 8, 3, 3), ws=None) == WORKSPACE      # the limits themselves pass
    # 3. alignment (before the aliasing)
    for name in ("gx", "x", "wc", "gz", "gw"):
        assert call(**{name: off}) == ALIGN, name
    assert call(gx=off, gz=off) == ALIGN
    # 4. aliasing: grad_z may be neither input
    assert call(gz=GX) == DIMS and call(gz=X) == DIMS and call(gz=GX, ws=None) == DIMS
    # 5. the workspace: NULL, short, off a 16-byte boundary; the exact size passes every check before the fault gate
    need = _lib.lib().finc_inverse_backward_workspace_bytes(*SHAPE)
    assert call(ws=None) == WORKSPACE and call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert call(ws=fake_ptr(0x6004)) == WORKSPACE
    assert call(gz=None, ws_bytes=need - 1) == WORKSPACE and call(gw=None, x=None, ws_bytes=need - 1) == WORKSPACE


def test_a_grad_weight_without_a_kernel_is_refused_before_any_launch():
    """The forward's weight gradient has no kernel for filters of more than 49 taps (finc_backward_f32's own limit): with every other
    check passed, asking for grad_w there is FINC_ERR_UNSUPPORTED; grad_z alone goes on to the launch."""
    big = (2, 4, 4, 12, 12, 9, 9)
    assert call(shape=big) == UNSUPPORTED and call(shape=big, gz=None) == UNSUPPORTED
    assert call(shape=big, ws=None) == WORKSPACE                       # (behind the workspace in the order)
    assert call(shape=(2, 4, 4, 12, 12, 7, 7), ws_bytes=0) == WORKSPACE


def test_the_exact_workspace_passes_the_checks():
    """With the exact size nothing is left to refuse: the call goes on to its first HIP call -- which needs a device.  On a machine
    without one that is FINC_ERR_LAUNCH, never one of the argument statuses; with one it would launch on fake pointers, so there the
    same fact is shown through the size function alone."""
    import torch
    need = _lib.lib().finc_inverse_backward_workspace_bytes(*SHAPE)
    assert need >= 256 and need % 256 == 0
    if not torch.cuda.is_available():
        assert call(ws_bytes=need) == LAUNCH


def adj(wc=WC, wa=GZ, lt=GW, G=4, Cq=6, KH=3, KW=3):
    return _lib.lib().finc_adjoint_weights_f32(wc, wa, lt, G, Cq, KH, KW, None)


def test_adjoint_weights_refuses_in_the_documented_order():
    assert adj(wc=None) == NULL and adj(wa=None) == NULL and adj(lt=None) == NULL and adj(wc=None, G=0) == NULL
    off = fake_ptr(0x1001)
    for kw in (dict(G=0), dict(G=-1), dict(Cq=0), dict(KH=0), dict(KW=-3), dict(G=17), dict(Cq=257), dict(KH=16)):
        assert adj(**kw) == DIMS and adj(wc=off, **kw) == DIMS, kw
    assert adj(wc=off) == ALIGN and adj(wa=off) == ALIGN and adj(lt=off) == ALIGN and adj(wa=off, lt=off) == ALIGN
    assert adj(wa=WC) == DIMS and adj(lt=WC) == DIMS and adj(wa=GZ, lt=GZ) == DIMS


def test_the_small_calls_refuse_before_any_hip_call():
    L = _lib.lib()
    assert L.finc_lead_product_f32(None, GW, 2, 4, 6, 64, None) == NULL and L.finc_lead_product_f32(GZ, None, 2, 4, 6, 64, None) == NULL
    for args in ((0, 4, 6, 64), (2, 0, 6, 64), (2, 4, 0, 64), (2, 4, 6, 0), (2, 17, 6, 64), (2, 4, 257, 64), (1, 16, 256, 1 << 18)):
        assert L.finc_lead_product_f32(GZ, GW, *args, None) == DIMS, args
    assert L.finc_lead_product_f32(fake_ptr(0x1002), GW, 2, 4, 6, 64, None) == ALIGN
    assert L.finc_lead_product_f32(GZ, GZ, 2, 4, 6, 64, None) == DIMS
    assert L.finc_negate_f32(None, 4, None) == NULL and L.finc_negate_f32(GW, 0, None) == DIMS
    assert L.finc_negate_f32(GW, 1 << 31, None) == DIMS and L.finc_negate_f32(fake_ptr(0x1001), 4, None) == ALIGN


def test_the_workspace_bound_is_positive_and_never_shrinks():
    f = _lib.lib().finc_inverse_backward_workspace_bytes
    assert f(0, 4, 6, 8, 8, 3, 3) > 0 and f(2, 4, 6, 8, 8, 0, 3) > 0 and f(-1, -1, -1, -1, -1, -1, -1) > 0
    banks = ((4, 24, 3, 3), (1, 5, 2, 3), (4, 12, 3, 3), (1, 80, 3, 3), (4, 12, 4, 4), (4, 4, 9, 9), (4, 48, 5, 5), (1, 192, 3, 3))
    for G, Cq, KH, KW in banks:
        for B in (1, 3, 64, 130, 260):
            for H in (1, 5, 16, 64):
                sizes = [f(B, G, Cq, H, W, KH, KW) for W in range(1, 70)]
                assert all(a > 0 for a in sizes) and sizes == sorted(sizes), ("W", G, Cq, KH, KW, B, H)
        for W in (4, 5, 16, 33, 64):
            for H in (4, 16):
                sizes = [f(B, G, Cq, H, W, KH, KW) for B in range(1, 300)]
                assert sizes == sorted(sizes), ("B", G, Cq, KH, KW, H, W)
            for B in (1, 8, 130):
                sizes = [f(B, G, Cq, H, W, KH, KW) for H in range(1, 70)]
                assert sizes == sorted(sizes), ("H", G, Cq, KH, KW, B, W)
    # ... and it covers what its parts ask for on their own: the bank and lead_t, y, then the larger of the two calls' workspaces
    L = _lib.lib()
    for (B, G, Cq, H, W, KH, KW) in ((256, 4, 24, 64, 64, 3, 3), (2, 4, 6, 8, 7, 3, 3), (8, 1, 80, 5, 12, 3, 3), (64, 4, 48, 32, 32, 5, 5),
                                     (3, 4, 13, 8, 36, 3, 3), (2, 4, 33, 8, 28, 3, 3), (8, 4, 12, 32, 32, 4, 4)):
        C = G * Cq
        own = C * Cq * KH * KW * 4 + C * C * 4 + B * C * H * W * 4
        assert f(B, G, Cq, H, W, KH, KW) >= own + max(L.finc_inverse_workspace_bytes(B, G, Cq, H, W, KH, KW),
                                                      L.finc_backward_workspace_bytes(B, G, Cq, H, W, KH, KW)), (B, G, Cq, H, W, KH, KW)


# ---------------------------------------------------------------------------------------------------------------------
# the mathematics
# ---------------------------------------------------------------------------------------------------------------------
def test_the_restatement_of_the_solve_reproduces_the_reference_solver():
    """`inverse_backward_ref.solve` against `x_rev_cython` (the reference's own fp64 solver on fp32 data) of two unit fixtures."""
    import torch
    for name in ("unit_B2_C8_6x9_k3", "unit_B1_C8_10x14_k3x5"):
        g = golden(name)
        x = ref.solve(torch.tensor(g["z"].astype(np.float64)), torch.tensor(unit_stored_weights(g).astype(np.float64)), 4, ORIENT_FASTFLOW)
        assert rel_err(x.numpy(), g["x_rev_cython"]) <= 2e-7, name      # (the fixture is rounded to fp32: half an ulp of its largest entry)


def random_bank(rng, G, Cq, KH, KW, orient):
    from oracle import oracle
    return oracle.make_stored_weights(G, Cq, KH, KW, orient, seed=int(rng.integers(1 << 30)), std=0.2 / np.sqrt(Cq))


IDENTITY_CASES = [("golden", "unit_B2_C8_6x9_k3"), ("golden", "unit_B1_C8_10x14_k3x5")] + \
                 [("padded", order, k) for order in ("TL", "TR", "BL", "BR") for k in ((3, 3),)] + \
                 [("padded", "TR", (2, 3)), ("padded", "BL", (3, 2)), ("grouped", 2, (3, 3)), ("grouped", 4, (2, 2))]


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_adjoint_identity_reproduces_autograd_through_the_solve(case):
    """DESIGN 3.15 in float64: w_adj, the complemented orientation, the oracle's fp64 inverse and the lead product give the
    reference's grad_z; minus the forward's masked weight gradient at (x, grad_z) gives its masked grad_w.  This pins the mathematics,
    not the library."""
    from oracle import oracle
    import zlib
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    if case[0] == "golden":
        g = golden(case[1])
        ws, z, G, orient = unit_stored_weights(g).astype(np.float64), g["z"].astype(np.float64), 4, ORIENT_FASTFLOW
    elif case[0] == "padded":
        G, orient = 1, ORDER_BITS[case[1]]
        ws = random_bank(rng, 1, 5, *case[2], orient).astype(np.float64)
        z = rng.standard_normal((2, 5, 6, 7))
    else:
        G = case[1]
        orient = int(rng.integers(0, 1 << (2 * G)))                     # mixed orientations
        ws = random_bank(rng, G, 3, *case[2], orient).astype(np.float64)
        z = rng.standard_normal((2, 3 * G, 5, 6))
    g_x = rng.standard_normal(z.shape)
    x_ref, gz_ref, gw_ref = ref.reference_grads(z, ws, g_x, G, orient)
    x, gz, gw = ref.adjoint_identity(z, ws, g_x, G, orient, oracle.inverse_f64)
    Cq, KH, KW = ws.shape[1:]
    mask = ref.stored_mask(G, Cq, KH, KW, orient).numpy()
    assert rel_err(x, x_ref) <= 1e-12 and rel_err(gz, gz_ref) <= 1e-12 and rel_err(gw, gw_ref * mask) <= 1e-12
    assert np.all(gw[mask == 0] == 0) and np.any((gw_ref * (1 - mask)) != 0)      # the free gradient is NOT zero there
    # the adjoint bank is a canonical bank like any other
    w_adj, lead_t = ref.adjoint_bank(np.concatenate([ref.np_flip(ws[k * Cq:(k + 1) * Cq], ref.group_orient(orient, k)) for k in range(G)]), G)
    assert oracle.check_invariant(w_adj.astype(np.float32), G) == 0
    assert np.allclose(np.tril(lead_t, -1), 0) and np.allclose(np.diag(lead_t), 1)
