"""The launch plans of the per-pixel layers -- the coupling, ActNorm, bias + ReLU, the lead product, the negate and the mix -- read
through the host-only query (include/finc.h finc_debug_pixel_plan, `_lib.pixel_plan`): no GPU, no launch.

  * every case of tests/pixel_regime_cases.py produces exactly the plan numbers written out there by hand -- the table is the
    independent statement, the query answers from the functions the launchers call (cpl_row_plan, cpl_transform_plan, cpl_grad_plan,
    adj_negate_grid, mix_plan);
  * a deterministic sweep over B, C, HW and the three alignment classes: the three rules restated here (grid-stride rows, (outer, part)
    workgroups, the mix's instantiation table and chunk loop) give the query's numbers, and whatever the rule, the grid covers the
    items, nobody takes an empty last trip, the wide forms appear only where the pointers and HW allow them, and the partials fit the
    workspace the library asks for.
"""
import ctypes

import pytest

from fincflow_amd import _lib
from pixel_regime_cases import (MIX_ALIGN16_TWIN, MIX_CASES, PIXEL_REGIME_CASES, WINO5_ALIGN8_CASES, last_trip_item, multi_trip)

THREADS, CHIP = 256, 2048
MIX_CHANNELS = (4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192)


def ceil_div(a, b):
    return -(-a // b)


def query(case, **over):
    c = dict(case, **over)
    B, C, H, W = c["shape"]
    return _lib.pixel_plan(c["rule"], c["family"], B, C, H * W, c["align"], c["elem"], c["groups"])


@pytest.mark.parametrize("name", sorted(PIXEL_REGIME_CASES))
def test_pixel_regime_case_produces_its_plan(name):
    case = PIXEL_REGIME_CASES[name]
    got, want = query(case), case["plan"]
    assert got == want, (name, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    if name.startswith("mix_align8") and not multi_trip(case):
        assert want["io"] == 2 and MIX_ALIGN16_TWIN[name]["io"] == 4, name        # there for its form
    else:
        assert want["trips"] >= 2, (name, "states no second trip")
        # the last trip is not empty and an earlier one does not already cover the items
        per_trip = {"rows": want["grid"] * want["threads"], "parts": want["parts"] * want["threads"], "mix": want["parts"]}[case["rule"]]
        assert last_trip_item(case) == (want["trips"] - 1) * per_trip < want["items"] <= want["trips"] * per_trip, name
    # the largest tensor stays near 170 MB
    B, C, H, W = case["shape"]
    assert B * C * H * W * case["elem"] <= 170_000_000, name


@pytest.mark.parametrize("name", sorted(MIX_ALIGN16_TWIN))
def test_the_8_byte_class_takes_another_form_than_16_byte_pointers(name):
    """The three 8-byte cases: two pixels per lane where 16-byte aligned pointers take four, dwords on float-aligned ones."""
    case = MIX_CASES[name]
    assert query(case, align=16) == MIX_ALIGN16_TWIN[name], name
    assert query(case)["io"] == 2 and query(case, align=16)["io"] == 4 and query(case, align=4)["io"] == 1, name


@pytest.mark.parametrize("name", sorted(WINO5_ALIGN8_CASES))
def test_f25_takes_8_byte_aligned_activations(name):
    """finc_wino5_takes: align >= 8.  At 8 the plan is the one of 16-byte pointers; at 4 the strip kernel runs."""
    case = WINO5_ALIGN8_CASES[name]
    assert _lib.conv_plan(*case["dims"], align=8) == case["plan"] == _lib.conv_plan(*case["dims"], align=16), name
    assert _lib.conv_plan(*case["dims"], align=4)["form"] == "strip", name
    assert case["dims"][4] % 2 == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the three rules, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def rows_rule(rows, HW, V, align, cap=4 * CHIP):
    wide = HW % V == 0 and align == 16
    items = rows * (HW // V if wide else HW)
    grid = min(ceil_div(items, THREADS), cap)
    return dict(io=V if wide else 1, threads=THREADS, grid=grid, parts=0, items=items, trips=ceil_div(items, grid * THREADS), outer=0, lds=0)


def parts_rule(outer, per_outer_rows, HW, align):
    """`per_outer_rows` rows of HW elements per outer unit (C / 2 pairs of an image; the B images of a channel)."""
    wide = HW % 4 == 0 and align == 16
    items = per_outer_rows * (HW // 4 if wide else HW)
    parts = max(1, min(ceil_div(items, THREADS), ceil_div(CHIP, outer)))
    return dict(io=4 if wide else 1, threads=THREADS, grid=outer * parts, parts=parts, items=items, trips=ceil_div(items, parts * THREADS),
                outer=outer, lds=0)


def partials_bound(items, outer):
    """finc_coupling.h cpl_partials_bound: what a workspace reserves per sum, for the dword form's item count."""
    return min(outer * ceil_div(items, THREADS), CHIP + outer)


def mix_instantiations(C):
    """finc_mix.hip make_mix<C>, restated: (pixels per lane, large workgroup) -> waves per workgroup it was compiled with, for the
    pairs that exist."""
    MTN, NK = ceil_div(C, 16), C // 4
    big_lds = MTN * (NK + 1) * 256 > 80 * 1024
    kb = NK if NK <= 32 else 24
    inst = {(1, 0): 16 if big_lds else 4, (1, 1): 16}
    if not big_lds:
        inst[(2, 0)] = 4
    if 2 * kb + 10 * MTN + 24 <= 128:
        inst[(2, 1)] = 16
    if MTN <= 6:
        inst[(4, 0)], inst[(4, 1)] = 4, 8
    return inst


def mix_rule(B, C, HW, align):
    inst = mix_instantiations(C)
    lds = ceil_div(C, 16) * (C // 4 + 1) * 256
    big = int(B * ceil_div(HW, 16) >= 16384)
    px = 4 if (HW % 4 == 0 and align == 16 and HW >= 64) else 2 if (HW % 2 == 0 and align >= 8 and HW >= 32) else 1
    wb = big
    while px > 1 and (px, wb) not in inst:
        if (px, wb ^ 1) in inst:
            wb ^= 1
            break
        px //= 2
    waves = inst[(px, wb)]
    chunks = B * ceil_div(HW, 16 * px)
    per_cu = max(1, min(160 * 1024 // lds, (8 if px == 4 else 16) // waves))
    grid = min(ceil_div(chunks, waves), 256 * per_cu)
    return dict(io=px, threads=64 * waves, grid=grid, parts=grid * waves, items=chunks, trips=ceil_div(chunks, grid * waves), outer=B, lds=lds)


SWEEP_B = (1, 2, 3, 33, 129, 255, 256, 257, 512, 1025)
SWEEP_HW = (1, 2, 15, 16, 30, 32, 49, 62, 64, 66, 575, 576, 1023, 1024, 1054, 4096)
SWEEP_C = MIX_CHANNELS + (2, 6, 10, 20, 30)


def check_cover(p, per_trip, ctx):
    assert p["trips"] >= 1 and p["grid"] >= 1 and p["items"] >= 1, ctx
    assert (p["trips"] - 1) * per_trip < p["items"] <= p["trips"] * per_trip, ctx          # covered, and no empty last trip
    assert p["grid"] * p["threads"] < 2 ** 31, ctx


@pytest.mark.parametrize("C", SWEEP_C)
def test_pixel_plan_invariants_sweep(C):
    L = _lib.lib()
    seen, multi = set(), {"rows": 0, "parts": 0, "mix": 0}
    for B in SWEEP_B:
        for HW in SWEEP_HW:
            cws, aws = L.finc_coupling_workspace_bytes(B, C, HW), L.finc_actnorm_workspace_bytes(B, C, HW)
            for align in (4, 8, 16):
                ctx = (B, C, HW, align)
                # ---- grid-stride rows: fp32 and bf16 channel rows, the grouped lead product, the negate
                for elem, V in ((4, 4), (2, 8)):
                    p = _lib.pixel_plan("rows", "channel_rows", B, C, HW, align, elem)
                    assert p == rows_rule(B * C, HW, V, align), ctx + (p,)
                    check_cover(p, p["grid"] * THREADS, ctx)
                    assert (p["io"] > 1) == (align == 16 and HW % V == 0) and p["grid"] <= 4 * CHIP, ctx + (p,)
                    multi["rows"] += p["trips"] > 1
                for G in (1, 2, 4):
                    if C % G:
                        continue
                    p = _lib.pixel_plan("rows", "lead", B, C, HW, align, groups=G)
                    assert (p is None) == (C in MIX_CHANNELS), ctx              # a channel count the mix takes runs the mix
                    if p is not None:
                        assert p == rows_rule(B * G, HW, 4, align), ctx + (G, p)
                        check_cover(p, p["grid"] * THREADS, ctx)
                p = _lib.pixel_plan("rows", "negate", B, C, HW, align)
                assert p == dict(rows_rule(B * C, HW, 1, align, cap=1024)), ctx + (p,)
                check_cover(p, p["grid"] * THREADS, ctx)
                # ---- (outer, part): transform, coupling backward (fp32 and bf16 raw), ActNorm backward / init
                for elem in (4, 2):
                    if C % 2:
                        continue
                    t = _lib.pixel_plan("parts", "transform", B, C, HW, align, elem)
                    g = _lib.pixel_plan("parts", "coupling_grad", B, C, HW, align, elem)
                    assert t == parts_rule(B, C // 2, HW, align) and g == parts_rule(C // 2, B, HW, align), ctx + (t, g)
                    for p in (t, g):
                        check_cover(p, p["parts"] * THREADS, ctx)
                        assert (p["io"] == 4) == (align == 16 and HW % 4 == 0) and p["grid"] == p["outer"] * p["parts"], ctx + (p,)
                        multi["parts"] += p["trips"] > 1
                    # the partials: one per workgroup and sum -- within the bound the workspace is sized by, and within the workspace
                    assert t["grid"] <= partials_bound((C // 2) * HW, B) and 4 * t["grid"] <= cws, ctx + (t, cws)
                    assert g["grid"] <= partials_bound(B * HW, C // 2) and 4 * 4 * g["grid"] <= cws, ctx + (g, cws)
                a = _lib.pixel_plan("parts", "actnorm_grad", B, C, HW, align)
                assert a == parts_rule(C, B, HW, align), ctx + (a,)
                check_cover(a, a["parts"] * THREADS, ctx)
                assert a["grid"] <= partials_bound(B * HW, C), ctx + (a,)
                Q = a["parts"]
                assert 4 * max(2 * C * (Q + 1), 3 * C * Q) <= aws, ctx + (a, aws)         # the backward's 2 C (Q + 1), the init's 3 C Q
                # ---- the mix
                m = _lib.pixel_plan("mix", "mix", B, C, HW, align)
                assert (m is None) == (C not in MIX_CHANNELS) == (L.finc_mix_supported_f32(C) == 0), ctx
                if m is None:
                    continue
                assert m == mix_rule(B, C, HW, align), ctx + (m, mix_rule(B, C, HW, align))
                check_cover(m, m["parts"], ctx)
                waves = m["threads"] // 64
                # the workgroup has the size the chosen instantiation was compiled for, and the grid's waves are whole workgroups
                assert waves in set(w for (px, _), w in mix_instantiations(C).items() if px == m["io"]), ctx + (m,)
                assert m["parts"] == m["grid"] * waves and m["threads"] == 64 * waves <= 1024, ctx + (m,)
                assert m["io"] in (1, 2, 4) and HW % m["io"] == 0, ctx + (m,)
                assert m["io"] < 4 or (align == 16 and HW >= 64), ctx + (m,)
                assert m["io"] < 2 or (align >= 8 and HW >= 32), ctx + (m,)
                assert m["lds"] <= 160 * 1024 and m["grid"] <= 256 * max(1, 160 * 1024 // m["lds"]), ctx + (m,)
                seen.add((m["io"], waves))
                multi["mix"] += m["trips"] > 1
    # not vacuous: both other rules loop somewhere in the sweep, and the mix shows every instantiation this channel count has
    assert multi["rows"] and (C % 2 or multi["parts"]), (C, multi)
    if C in MIX_CHANNELS:
        assert multi["mix"] and seen == set((px, w) for (px, _), w in mix_instantiations(C).items()), (C, seen, multi)


def test_pixel_plan_refuses_bad_arguments():
    L = _lib.lib()
    info = (ctypes.c_longlong * 8)()
    q = L.finc_debug_pixel_plan
    assert q(0, 0, 0, 1, 4, 16, 16, 4, None) == 1
    assert q(0, 0, 0, 0, 4, 16, 16, 4, info) == 2 and q(0, 0, 0, 1, 0, 16, 16, 4, info) == 2 and q(0, 0, 0, 1, 4, 0, 16, 4, info) == 2
    assert q(0, 0, 0, 1, 4, 16, 12, 4, info) == 2 and q(0, 0, 0, 1, 4, 16, 16, 8, info) == 2          # alignment class, element size
    assert q(3, 0, 0, 1, 4, 16, 16, 4, info) == 2 and q(0, 3, 0, 1, 4, 16, 16, 4, info) == 2 and q(1, 3, 0, 1, 4, 16, 16, 4, info) == 2
    assert q(1, 0, 0, 1, 5, 16, 16, 4, info) == 2 and q(1, 1, 0, 1, 5, 16, 16, 4, info) == 2          # the coupling wants C even
    assert q(0, 1, 3, 1, 20, 16, 16, 4, info) == 2 and q(0, 1, 0, 1, 20, 16, 16, 4, info) == 2        # groups must divide C
    assert q(0, 1, 4, 1, 24, 16, 16, 4, info) == 3 and q(2, 0, 0, 1, 20, 16, 16, 4, info) == 3        # lead on a mix count; no mix for 20
    assert q(2, 0, 0, 1, 12, 16, 16, 2, info) == 2                                                    # the mix is fp32 only
    assert q(0, 2, 0, 1 << 16, 1 << 8, 1 << 8, 16, 4, info) == 2                                      # the negate's n >= 2^31
    assert q(0, 0, 0, 1, 4, 16, 16, 4, info) == 0 and list(info) == [4, 256, 1, 0, 16, 1, 0, 0]
