"""Host side of the float64 matrix-core kernels of the wider banks (finc_f64.hip's M-split family: 29 .. 64 channels at 3x3, 33 .. 64
at 2x2): the plan query's symbol, the ABI floor, and `_lib.f64_plan` against plan numbers written out by hand from the rules below
(tests/plan_cases.py's way: nothing in the expected numbers calls the library).  No GPU is needed: every call here is host-only.

The rules (finc_f64.hip: DCfg, finc_f64_plan, finc_f64_gradw_plan), with CQP the padded bank, K the filter side:
    family 1   one wave per problem: CQP = Cq rounded up to 4, on the table 3x3 {4 .. 24}, 2x2 {4, 8, 12, 16, 24, 32}
    family 2   CQP = 32 / 48 / 64 for Cq in 29 .. 32 / 33 .. 48 / 49 .. 64 at 3x3, 48 / 64 for 33 .. 48 / 49 .. 64 at 2x2;
               waves per problem = CQP / 16; problems per workgroup 2 at CQP = 32 when two fit the LDS and there are two, else 1
    LDS of one problem = lds_fixed + DF * FSLOT: a cell (one pixel) is 2 * CQP bytes, the ring 6 slots x 64 lanes of cells plus one zero
               cell -> lds_fixed = 770 * CQP; a FIFO slot is 4 x (K - 1) cells -> FSLOT = 8 * (K - 1) * CQP; the FIFO has
               DF = W - P + 2 K - 2 slots (P = min(W, 16) rows per band), and one more in family 2; at most 160 KiB per workgroup
    inverse    grid = ceil(B * G / problems per workgroup)
    forward    grid.x = B * G * ceil(W / 16) workgroups of `waves` (one wave in family 1), grid.y = 1
    grad-w     a slab is 1 wave (family 1) or a workgroup of `waves` (family 2); a launch of fewer than 1024 waves cuts its slabs into
               want = clamp(1024 // (B * G * waves per slab), 1, max(1, H // 4)) chunks: RC = ceil(H / want), nrc = ceil(H / RC),
               grid = B * G * nrc
"""
import ctypes
import os
import re

import pytest

from helpers import REPO, load_stub_library
from fincflow_amd import _lib


def test_the_new_symbol_is_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "finc.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    name = "finc_debug_f64_plan"
    assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/finc.h"
    assert hasattr(raw, name), f"{name} is not exported"
    assert name in _lib.SYMBOLS and getattr(_lib.lib(), name).argtypes is not None, f"{name} is not bound"
    assert callable(_lib.f64_plan)
    assert _lib.lib().finc_version() >= _lib.F64_WIDE_BANKS_ABI_VERSION == 112


def test_an_older_library_is_refused_by_name(tmp_path):
    out = load_stub_library(tmp_path, 111)
    assert "= 111" in out and "112" in out and "finc_debug_f64_plan" in out and "29 .. 64" in out, out


def test_the_plan_query_refuses_bad_arguments():
    L = _lib.lib()
    info = (ctypes.c_int * 11)()
    assert L.finc_debug_f64_plan(2, 4, 48, 8, 8, 3, 3, None) == 1
    for k in range(7):
        a = [2, 4, 48, 8, 8, 3, 3]
        a[k] = 0
        assert L.finc_debug_f64_plan(*a, info) == 2, a


def plan(family, cqp, waves, ppw, lds, inv_grid, fwd_grid, gw_grid, nrc, RC):
    return dict(family=family, cqp=cqp, waves=waves, ppw=ppw, lds=lds, inv_grid=inv_grid, fwd_grid=fwd_grid, gw_grid=gw_grid, nrc=nrc, RC=RC)


NONE = plan(0, 0, 0, 0, 0, 0, (0, 0), 0, 0, 0)
# (B, G, Cq, H, W, KH, KW) -> the plan, by hand.  The first eleven are the shapes tests/test_gpu_f64_wide_banks.py runs.
HAND = {
    # CQP 32: lds_fixed 24,640, FSLOT 512; W = 7: P = 7, DF = 0 + 4 + 1; two problems share a workgroup
    (2, 1, 32, 5, 7, 3, 3): plan(2, 32, 2, 2, 2 * (24640 + 5 * 512), 1, (2 * 1, 1), 2 * 1, 1, 5),
    (3, 1, 30, 5, 7, 3, 3): plan(2, 32, 2, 2, 2 * (24640 + 5 * 512), 2, (3 * 1, 1), 3 * 1, 1, 5),      # (the second workgroup is half empty)
    (2, 4, 29, 6, 18, 3, 3): plan(2, 32, 2, 2, 2 * (24640 + 7 * 512), 4, (8 * 2, 1), 8 * 1, 1, 6),
    # CQP 48: lds_fixed 36,960, FSLOT 768; W = 17: DF = 1 + 4 + 1; grad-w: 1024 // 36 = 28 -> H // 4 = 4 chunks of 5 rows
    (3, 4, 48, 17, 17, 3, 3): plan(2, 48, 3, 1, 36960 + 6 * 768, 12, (12 * 2, 1), 12 * 4, 4, 5),
    (2, 1, 40, 9, 16, 3, 3): plan(2, 48, 3, 1, 36960 + 5 * 768, 2, (2 * 1, 1), 2 * 2, 2, 5),
    # CQP 64: lds_fixed 49,280, FSLOT 1,024
    (2, 4, 64, 9, 20, 3, 3): plan(2, 64, 4, 1, 49280 + 9 * 1024, 8, (8 * 2, 1), 8 * 2, 2, 5),
    (1, 2, 64, 4, 4, 3, 3): plan(2, 64, 4, 1, 49280 + 5 * 1024, 2, (2 * 1, 1), 2 * 1, 1, 4),
    # 2x2: FSLOT = 8 * CQP = 384, DF = W - P + 2 + 1
    (2, 2, 48, 9, 16, 2, 2): plan(2, 48, 3, 1, 36960 + 3 * 384, 4, (4 * 1, 1), 4 * 2, 2, 5),
    (1, 4, 36, 4, 5, 2, 2): plan(2, 48, 3, 1, 36960 + 3 * 384, 4, (4 * 1, 1), 4 * 1, 1, 4),
    # one problem: 1024 // 3 = 341 -> 4 chunks of 5 rows, the last one of 2
    (1, 1, 48, 17, 17, 3, 3): plan(2, 48, 3, 1, 36960 + 6 * 768, 1, (1 * 2, 1), 1 * 4, 4, 5),
    (2, 1, 48, 6, 18, 3, 3): plan(2, 48, 3, 1, 36960 + 7 * 768, 2, (2 * 2, 1), 2 * 1, 1, 6),
    # a single problem has no partner; two problems too wide for one workgroup's LDS (2 x 81,984 > 163,840) run one each
    (1, 1, 32, 5, 7, 3, 3): plan(2, 32, 2, 1, 24640 + 5 * 512, 1, (1 * 1, 1), 1 * 1, 1, 5),
    (2, 1, 32, 4, 123, 3, 3): plan(2, 32, 2, 1, 24640 + 112 * 512, 2, (2 * 8, 1), 2 * 1, 1, 4),
    # the benchmark shapes of scripts/time_f64_wide_banks.py: a full chip, no row chunks
    (256, 4, 48, 32, 32, 3, 3): plan(2, 48, 3, 1, 36960 + 21 * 768, 1024, (1024 * 2, 1), 1024, 1, 32),
    (128, 4, 64, 32, 32, 3, 3): plan(2, 64, 4, 1, 49280 + 21 * 1024, 512, (512 * 2, 1), 512, 1, 32),
    (256, 4, 32, 64, 64, 3, 3): plan(2, 32, 2, 2, 2 * (24640 + 53 * 512), 512, (1024 * 4, 1), 1024, 1, 64),
    # the widest 64-channel map the LDS holds: DF = 122 - 16 + 5 = 111, 49,280 + 113,664 = 162,944 <= 163,840; one column more is not
    (1, 1, 64, 4, 122, 3, 3): plan(2, 64, 4, 1, 49280 + 111 * 1024, 1, (1 * 8, 1), 1 * 1, 1, 4),
    (1, 1, 64, 4, 123, 3, 3): NONE,
    # the first family, unchanged: c3 (cell 48 bytes: 18,480 + 52 * 384 per wave, four waves per workgroup) and a padded small bank
    (256, 4, 24, 64, 64, 3, 3): plan(1, 24, 1, 4, 4 * (18480 + 52 * 384), 256, (4 * 1024, 1), 1024, 1, 64),
    (2, 4, 3, 4, 4, 3, 3): plan(1, 4, 1, 4, 4 * (3080 + 4 * 64), 2, (1 * 8, 1), 8, 1, 4),
    # more slabs than a grid's y dimension carries (65,535): CQP 4 at 2x2, FSLOT 32; W = 2: P = 2, DF = 0 + 2
    (65536, 1, 4, 2, 2, 2, 2): plan(1, 4, 1, 4, 4 * (3080 + 2 * 32), 16384, (65536, 1), 65536, 1, 2),
    # no matrix-core kernel: 25 .. 28 channels at 3x3, 5x5, non-square, beyond 64 channels, the gaps of the 2x2 table
    (1, 1, 28, 5, 5, 3, 3): NONE,
    (2, 4, 25, 8, 8, 3, 3): NONE,
    (2, 4, 4, 6, 6, 5, 5): NONE,
    (2, 4, 48, 6, 6, 5, 5): NONE,
    (2, 4, 4, 5, 6, 3, 2): NONE,
    (2, 4, 65, 8, 8, 3, 3): NONE,
    (2, 4, 65, 8, 8, 2, 2): NONE,
    (2, 4, 96, 8, 8, 3, 3): NONE,
}


@pytest.mark.parametrize("dims", sorted(HAND), ids=lambda d: "B%d_G%d_Cq%d_%dx%d_k%dx%d" % d)
def test_the_plan_against_the_numbers_by_hand(dims):
    assert _lib.f64_plan(*dims) == HAND[dims]
    assert HAND[dims]["lds"] <= 160 * 1024


def test_the_existing_shapes_stay_on_the_first_family():
    from test_gpu_f64_backward import FALLBACK_CASES, MFMA_CASES
    for name, (dims, _) in MFMA_CASES.items():
        p = _lib.f64_plan(*dims)
        assert p["family"] == 1 and p["waves"] == 1 and p["cqp"] == (dims[2] + 3) // 4 * 4, (name, p)
    for name, (dims, _) in FALLBACK_CASES.items():
        assert _lib.f64_plan(*dims)["family"] == 0, name


def test_every_channel_count_has_the_family_the_table_says():
    for K, first, one_wave in ((3, 29, set(range(1, 25))), (2, 33, set(range(1, 17)) | set(range(21, 25)) | set(range(29, 33)))):
        for Cq in range(1, 70):
            p = _lib.f64_plan(2, 2, Cq, 8, 8, K, K)
            want = 1 if Cq in one_wave else 2 if first <= Cq <= 64 else 0
            assert p["family"] == want, (K, Cq, p)
            if want == 2:
                assert p["cqp"] == (32 if Cq <= 32 else 48 if Cq <= 48 else 64) and p["waves"] == p["cqp"] // 16


NEW_BANKS = [(4, 29, 3), (1, 32, 3), (4, 40, 3), (4, 48, 3), (2, 64, 3), (4, 64, 3), (4, 36, 2), (2, 48, 2), (4, 64, 2)]


def test_the_workspaces_cover_the_new_banks():
    L = _lib.lib()
    for G, Cq, K in NEW_BANKS:
        cqp = 32 if Cq <= 32 else 48 if Cq <= 48 else 64
        packed = G * K * K * (cqp // 4) * (cqp // 16) * 64 * 8           # [group][tap][k-step][row tile] fragments of 64 doubles
        assert L.finc_f64_workspace_bytes(G, Cq, K, K) >= packed, (G, Cq, K)
        tiles = K * K * (cqp // 16) ** 2 * 256 * 8                         # one set of partial tiles of a group
        f = L.finc_backward_f64_workspace_bytes
        for H, W in ((4, 4), (17, 17), (32, 32)):
            sizes = [f(B, G, Cq, H, W, K, K) for B in range(1, 300)]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (G, Cq, K, H, W)
            for B in (1, 3, 64, 299):
                p = _lib.f64_plan(B, G, Cq, H, W, K, K)
                assert p["family"] == 2
                assert f(B, G, Cq, H, W, K, K) >= packed + B * p["nrc"] * G * tiles, (B, G, Cq, H, W, K)
        for B in (1, 8, 130):
            sizes = [f(B, G, Cq, H, 16, K, K) for H in range(1, 70)]
            assert sizes == sorted(sizes), ("H", G, Cq, K, B)


def test_the_pinned_workspace_sizes_of_the_first_family_are_unchanged():
    """The three shapes tests/test_f64_backward_host.py bounds from below, at the values the rule gave before the second family: the
    bank (a multiple of 256 bytes here) plus max(B, 1024 / G) partial tile sets, at most B * max(1, H // 4)."""
    f = _lib.lib().finc_backward_f64_workspace_bytes
    assert f(256, 4, 24, 64, 64, 3, 3) == 4 * 9 * 6 * 2 * 64 * 8 + 256 * 4 * 9 * 4 * 256 * 8
    assert f(2, 4, 3, 4, 4, 3, 3) == 4 * 9 * 1 * 1 * 64 * 8 + 2 * 4 * 9 * 1 * 256 * 8
    assert f(1, 4, 24, 64, 64, 3, 3) == 4 * 9 * 6 * 2 * 64 * 8 + 16 * 4 * 9 * 4 * 256 * 8
    assert f(1, 1, 28, 5, 5, 3, 3) == 256 and f(2, 4, 4, 6, 6, 5, 5) == 256 and f(2, 4, 65, 8, 8, 3, 3) == 256
