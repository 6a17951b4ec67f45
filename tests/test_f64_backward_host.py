"""Host side of the double-precision backward (include/finc.h: finc_backward_f64_workspace_bytes, finc_backward_f64,
finc_check_invariant_f64): the symbols, the order of the status codes on fake pointers (every refusal happens before any HIP call, so
no GPU is needed) and the workspace bound.  The grad-weight launch does not cap its grid (one wave per (slab, row chunk): DESIGN 3.11),
so there is no plan entry to pin here.
"""
import ctypes
import os
import re

from helpers import ORIENT_FASTFLOW, REPO, fake_ptr, load_stub_library
from fincflow_amd import _lib

OK, NULL, DIMS, UNSUPPORTED, WORKSPACE, LAUNCH, INVARIANT, ALIGN = range(8)
NEW = ("finc_backward_f64_workspace_bytes", "finc_backward_f64", "finc_check_invariant_f64")
# distinct 256-byte aligned fake addresses
GZ, X, WC, GX, GW, WS = (fake_ptr(0x1000 * k) for k in range(1, 7))
SHAPE = (2, 4, 6, 8, 8, 3, 3)          # B, G, Cq, H, W, KH, KW


def test_the_new_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "finc.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/finc.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    assert _lib.lib().finc_version() >= _lib.F64_BACKWARD_ABI_VERSION == 111


def test_an_older_library_is_refused_by_name(tmp_path):
    out = load_stub_library(tmp_path, 110)
    assert "= 110" in out and "111" in out and "finc_backward_f64" in out and "finc_check_invariant_f64" in out, out


def call(gz=GZ, x=X, wc=WC, gx=GX, gw=GW, shape=SHAPE, ws=WS, ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.finc_backward_f64_workspace_bytes(*shape)
    return L.finc_backward_f64(gz, x, wc, gx, gw, *shape, ORIENT_FASTFLOW, ws, ws_bytes, None)


def test_backward_f64_refuses_in_the_documented_order():
    # 1. NULL pointers (before the dims: a zero batch beside them is still status 1)
    bad = (0,) + SHAPE[1:]
    assert call(gz=None) == NULL and call(gz=None, shape=bad) == NULL
    assert call(gx=None, gw=None) == NULL and call(gx=None, gw=None, shape=bad) == NULL      # either output may be skipped, not both
    assert call(wc=None) == NULL and call(x=None) == NULL                                       # what each output reads
    # (an input nobody reads may be NULL: the next refusal in line is the dims')
    assert call(wc=None, gx=None, shape=bad) == DIMS and call(x=None, gw=None, shape=bad) == DIMS
    # 2. the dims (before the alignment: a misaligned pointer beside them is still status 2)
    off = fake_ptr(0x1004)
    for k in range(7):
        for v in (0, -1):
            s = SHAPE[:k] + (v,) + SHAPE[k + 1:]
            assert call(shape=s) == DIMS and call(gz=off, shape=s) == DIMS, s
    assert call(shape=(2, 17, 6, 8, 8, 3, 3)) == DIMS and call(shape=(2, 4, 257, 8, 8, 3, 3)) == DIMS
    assert call(shape=(2, 4, 6, 8, 8, 16, 3)) == DIMS
    # 3. a tensor off an 8-byte boundary (before the aliasing) -- 4-byte alignment, enough for the f32 call, is not enough here
    for name in ("gz", "x", "wc", "gx", "gw"):
        assert call(**{name: off}) == ALIGN, name
    assert call(gz=off, gx=off) == ALIGN
    # 4. grad_x == grad_z
    assert call(gx=GZ) == DIMS and call(gx=GZ, ws=None) == DIMS and call(gx=GZ, gw=None, x=None) == DIMS
    # (a missing, short or misaligned workspace is no refusal: the direct kernels run)


def test_nothing_is_left_to_refuse_behind_the_ladder():
    """With good arguments the call goes on to its first HIP call, with or without a workspace -- which needs a device.  On a machine
    without one that is FINC_ERR_LAUNCH, never one of the argument statuses; with one it would launch on fake pointers, so there the
    same fact rests on the size function alone."""
    import torch
    assert _lib.lib().finc_backward_f64_workspace_bytes(*SHAPE) >= 256
    if not torch.cuda.is_available():
        for kw in (dict(), dict(ws=None, ws_bytes=0), dict(ws_bytes=8), dict(ws=fake_ptr(0x6004)), dict(gx=None, wc=None),
                   dict(gw=None, x=None), dict(shape=(2, 4, 4, 12, 12, 5, 5)), dict(shape=(1, 1, 28, 5, 5, 3, 3))):
            assert call(**kw) == LAUNCH, kw


def check(wc=WC, G=4, Cq=6, KH=3, KW=3):
    return _lib.lib().finc_check_invariant_f64(wc, G, Cq, KH, KW, None)


def test_check_invariant_f64_refuses_like_the_f32_check():
    L = _lib.lib()
    assert check(wc=None) == NULL and check(wc=None, G=0) == NULL
    for kw in (dict(G=0), dict(G=-1), dict(Cq=0), dict(KH=0), dict(KW=-3), dict(G=17), dict(Cq=257), dict(KH=16)):
        assert check(**kw) == DIMS, kw
        assert L.finc_check_invariant_f32(WC, kw.get("G", 4), kw.get("Cq", 6), kw.get("KH", 3), kw.get("KW", 3), None) == DIMS, kw
    assert L.finc_check_invariant_f32(None, 4, 6, 3, 3, None) == NULL


def test_the_workspace_bound_is_positive_and_never_shrinks():
    f = _lib.lib().finc_backward_f64_workspace_bytes
    assert f(0, 4, 6, 8, 8, 3, 3) > 0 and f(2, 4, 6, 8, 8, 0, 3) > 0 and f(-1, -1, -1, -1, -1, -1, -1) > 0
    # banks with the matrix-core kernels (3x3 up to 24 channels, 2x2 up to 32) and without (28 channels, 5x5, 3x2)
    banks = ((4, 24, 3, 3), (4, 3, 3, 3), (1, 20, 3, 3), (4, 12, 3, 3), (2, 32, 2, 2), (4, 6, 2, 2), (1, 28, 3, 3), (4, 4, 5, 5), (4, 4, 3, 2))
    for G, Cq, KH, KW in banks:
        for B in (1, 3, 64, 130, 260):
            for H in (1, 5, 16, 64):
                sizes = [f(B, G, Cq, H, W, KH, KW) for W in range(1, 70)]
                assert all(a > 0 for a in sizes) and sizes == sorted(sizes), ("W", G, Cq, KH, KW, B, H)
        for W in (3, 4, 16, 33, 64):
            for H in (1, 4, 16, 64):
                sizes = [f(B, G, Cq, H, W, KH, KW) for B in range(1, 300)]
                assert sizes == sorted(sizes), ("B", G, Cq, KH, KW, H, W)
            for B in (1, 8, 130):
                sizes = [f(B, G, Cq, H, W, KH, KW) for H in range(1, 70)]
                assert sizes == sorted(sizes), ("H", G, Cq, KH, KW, B, W)
    # the bank of the grad-input and one set of tiles per wave behind it.  c3: 256 images x 1 chunk, 4 groups, 9 taps x 2 x 2 tiles of
    # 256 doubles; the smallest test shape: 2 images x 1 chunk (4 rows), 9 taps x 1 tile
    L = _lib.lib()
    assert f(256, 4, 24, 64, 64, 3, 3) >= L.finc_f64_workspace_bytes(4, 24, 3, 3) + 256 * 4 * 9 * 4 * 256 * 8
    assert f(2, 4, 3, 4, 4, 3, 3) >= L.finc_f64_workspace_bytes(4, 3, 3, 3) + 2 * 4 * 9 * 256 * 8
    # an underfilled chip cuts its slabs into row chunks of at least four rows: 1 image of 4 groups at 64 rows -> 16 chunks
    assert f(1, 4, 24, 64, 64, 3, 3) >= L.finc_f64_workspace_bytes(4, 24, 3, 3) + 16 * 4 * 9 * 4 * 256 * 8
    # a bank without the kernels asks for the minimum only
    assert f(2, 4, 4, 6, 6, 5, 5) == 256 and f(1, 1, 28, 5, 5, 3, 3) == 256
