"""The launch plans behind finc_backward_f32 and the forward, read through the two host-only queries (include/finc.h
finc_debug_gradw_plan, finc_debug_conv_plan): no GPU, no launch.

  * every case of tests/plan_cases.py produces exactly the plan numbers written out there by hand -- the table is the independent
    statement, the queries answer from the plan object the launch runs;
  * a deterministic sweep over banks, groups, batches, widths and alignments: the invariants every plan must keep whatever the rule
    (a workgroup has at least one unit, the grid is whole groups of wpg workgroups, the partials fit the workspace the library asks
    for, the row chunks tile the map and respect the kernel's minimum).
"""
import pytest

from fincflow_amd import _lib
from plan_cases import GRADW_WALK_CASES, MIN_CHUNK_ROWS, ROW_CHUNK_CASES, walk_lands_on_second_trip


@pytest.mark.parametrize("name", sorted(GRADW_WALK_CASES))
def test_grad_weight_walk_case_produces_its_plan(name):
    case = GRADW_WALK_CASES[name]
    dims, want = case["dims"], case["plan"]
    got = _lib.gradw_plan(*dims, align=16)
    assert got == want, (name, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    assert got["units"] > got["wpg"], (name, "no workgroup takes a second unit")
    assert walk_lands_on_second_trip(case), (name, "the last image is reached on a first trip")
    bv = _lib.backward_variant(*dims)
    assert (bv["gradw"], bv["conv_form"], bv["gradx_waves"]) == (want["form"], case["conv_form"], case["gradx_waves"]), (name, bv)
    # the whole tensor stays small: the regime comes from the launch geometry, not from the size
    B, G, Cq, H, W = dims[:5]
    assert B * G * Cq * H * W <= 1_600_000, name


def test_the_staged_walk_takes_the_dword_form_on_float_aligned_activations():
    """walk_staged's shape with grad_z and x only float-aligned (a view into a larger tensor): the plan at align 4 is the dword
    form on the same grid, 258 units on 256 workgroups per group (tests/test_gpu_bounds.py runs it)."""
    dims = GRADW_WALK_CASES["walk_staged"]["dims"]
    p = _lib.gradw_plan(*dims, align=4)
    assert dict(p, bytes=0) == dict(form="dword", strip=16, ns=2, units=258, wpg=256, grid=1024, block=64, mtt=1, fs=1, bytes=0), p
    assert p["bytes"] == 1024 * 9 * 256 * 4


@pytest.mark.parametrize("name", sorted(ROW_CHUNK_CASES))
def test_row_chunk_case_produces_its_plan(name):
    case = ROW_CHUNK_CASES[name]
    dims, want = case["dims"], case["plan"]
    try:
        _lib.set_forward_form(case["pin"])
        got = _lib.conv_plan(*dims, align=16)
        bv = _lib.backward_variant(*dims)
    finally:
        _lib.set_forward_form(0)
    assert got == want, (name, got, want)
    assert (bv["conv_form"], bv["gradw"], bv["gradx_waves"]) == (case["conv_form"], case["gradw"], case["gradx_waves"]), (name, bv)
    H = dims[3]
    assert H >= 16 and got["nrc"] >= 2 and H % got["RC"] != 0, (name, "no ragged chunk seam")


# (Cq, KH, KW): every bank of finc_gradw.hip's table, a 4x4 bank and a 96-channel 5x5 bank (both beyond it: the tile-pair kernels)
SWEEP_BANKS = ([(c, 3, 3) for c in (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 64, 96)] + [(c, 2, 2) for c in (4, 8, 12, 16, 24, 32)] +
               [(c, 5, 5) for c in (4, 8, 12, 16, 24, 32, 48)] + [(4, 3, 5), (4, 1, 3), (4, 3, 1)] + [(8, 4, 4), (96, 5, 5)])
SWEEP_B = (1, 3, 57, 129, 257, 513, 1025)
SWEEP_W = (8, 12, 16, 18, 24, 32, 36, 64)
SWEEP_H = (5, 17, 40)                          # below the one-wave-per-SIMD kernels' second chunk, just above it, several chunks


def gradw_wpg_rule(p, G):
    """finc_gradw.hip gradw_wpg, restated: (waves a unit takes of each group, waves per SIMD, cap) by form."""
    waves, per_simd, cap = {"dword": (1, 1, 1024), "staged": (1, 1, 1024), "tiled": (p["mtt"] ** 2, 2, 256),
                            "winograd": (p["fs"], 1, 1024), "winograd_tiled": (p["mtt"] ** 2, 2, 256)}[p["form"]]
    return min(p["units"], min(max(1024 * per_simd // (G * waves), 1), cap)), waves


@pytest.mark.parametrize("bank", SWEEP_BANKS, ids=lambda b: "Cq%d_k%dx%d" % b)
def test_plan_invariants_sweep(bank):
    Cq, KH, KW = bank
    ws_bytes = _lib.lib().finc_backward_workspace_bytes
    seen, conv_seen, walked, chunked, wino5_at_8 = set(), set(), 0, 0, 0
    for G in (1, 2, 4):
        for B in SWEEP_B:
            for W in SWEEP_W:
                for H in SWEEP_H:
                    dims = (B, G, Cq, H, W, KH, KW)
                    room = ws_bytes(*dims)
                    for align in (4, 8, 16):
                        p = _lib.gradw_plan(*dims, align=align)
                        ctx = (dims, align, p)
                        if align == 8:
                            # 8-byte pointers are float-aligned pointers to every kernel but F(2,5), which moves 8-byte pairs
                            c4, c8 = _lib.conv_plan(*dims, align=4), _lib.conv_plan(*dims, align=8)
                            assert p == _lib.gradw_plan(*dims, align=4), ctx
                            assert c8 == c4 or (c8["form"] == "winograd25" and c8 == _lib.conv_plan(*dims, align=16) and W % 2 == 0), (dims, c4, c8)
                            wino5_at_8 += c8 is not None and c8["form"] == "winograd25"
                        if p["form"] == "direct":
                            assert p["bytes"] == 0 and p["grid"] == 0, ctx
                        else:
                            assert p["units"] == B * p["ns"] and p["ns"] == -(-W // p["strip"]) and p["strip"] in (16, 32), ctx
                            assert 1 <= p["wpg"] <= p["units"], ctx
                            assert p["grid"] % (G * p["wpg"]) == 0, ctx
                            wpg, waves = gradw_wpg_rule(p, G)
                            assert p["wpg"] == wpg and p["grid"] * p["block"] == G * waves * wpg * 64, ctx
                            assert 0 < p["bytes"] <= room, ctx + (room,)
                            assert align == 16 or p["form"] == "dword", ctx          # 16-byte pieces need 16-byte aligned rows (8 is not enough)
                            seen.add(p["form"])
                            walked += p["units"] > p["wpg"]
                        if align == 16:
                            assert p["form"] == _lib.backward_variant(*dims)["gradw"], ctx
                        c = _lib.conv_plan(*dims, align=align)
                        if c is None:
                            continue
                        ctx = (dims, align, c)
                        conv_seen.add(c["form"])
                        assert c["nrc"] >= 1 and (c["nrc"] - 1) * c["RC"] < H <= c["nrc"] * c["RC"], ctx
                        assert c["ns"] == -(-W // c["strip"]) and c["waves"] >= 1, ctx
                        if c["nrc"] > 1:
                            assert c["RC"] >= MIN_CHUNK_ROWS[c["form"]], ctx
                            chunked += 1
                        else:
                            assert c["RC"] == H, ctx
                        if align == 16:
                            assert c["form"] == _lib.backward_variant(*dims)["conv_form"], ctx
    # the sweep is not vacuous: this bank has an MFMA grad-weight form that walks, and a forward that splits its rows (the
    # streaming-bank kernel and the big banks' M-split have no row chunks)
    assert seen and walked and (chunked or conv_seen <= {"stream", "msplit"}), (bank, seen, conv_seen, walked, chunked)
    assert bool(wino5_at_8) == ("winograd25" in conv_seen), (bank, conv_seen, wino5_at_8)      # F(2,5) banks take it at 8 bytes too


def test_plan_queries_refuse_bad_arguments():
    L = _lib.lib()
    import ctypes
    info, cinfo = (ctypes.c_longlong * 10)(), (ctypes.c_int * 6)()
    assert L.finc_debug_gradw_plan(1, 4, 8, 8, 8, 3, 3, 16, None) == 1 and L.finc_debug_conv_plan(1, 4, 8, 8, 8, 3, 3, 16, None) == 1
    assert L.finc_debug_gradw_plan(0, 4, 8, 8, 8, 3, 3, 16, info) == 2 and L.finc_debug_conv_plan(1, 4, 8, 8, 0, 3, 3, 16, cinfo) == 2
    assert L.finc_debug_gradw_plan(1, 4, 8, 8, 8, 3, 3, 12, info) == 2 and L.finc_debug_conv_plan(1, 4, 8, 8, 8, 3, 3, 0, cinfo) == 2
    assert _lib.gradw_plan(3, 4, 2, 6, 8, 1, 8)["form"] == "direct" and _lib.conv_plan(3, 4, 2, 6, 8, 1, 8) is None   # no MFMA kernel takes a 1x8 filter
