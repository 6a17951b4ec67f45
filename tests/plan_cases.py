"""Launch-regime cases: shapes whose launch geometry -- not their size -- puts a kernel into a loop regime the small parity shapes
never reach, each with the plan numbers it must produce.

The numbers are written out by hand from the rules (finc_gradw.hip finc_gradw_plan / gradw_wpg; finc_common.h finc_row_chunks) and are
the independent statement: tests/test_launch_plans_host.py compares them with what the library's own plan queries
(`_lib.gradw_plan`, `_lib.conv_plan`) answer, tests/test_gpu_bounds.py runs every case between guards.  Nothing here calls the library.

Grad-weight walk (finc_gradw.hip, all five forms): a workgroup walks `for (u = wslot; u < B * ns; u += wpg)` with
    wpg = min(units, clamp(1024 * per_simd / (G * waves), 1, cap))
    dword, staged        waves 1,       per_simd 1, cap 1024      G = 4: 256
    tiled                waves mtt^2,   per_simd 2, cap 256       G = 4: mtt 1: 512 -> 256, mtt 3: 2048 / 36 = 56
    winograd             waves fs,      per_simd 1, cap 1024      G = 4: fs 1: 256, fs 2: 128; G = 2, fs 2: 256
    winograd_tiled       waves mtt^2,   per_simd 2, cap 256       as tiled
so `units > wpg` means a second trip through the unit loop: LDS row tiles and halo pieces reused, rings and ping-pong buffers primed
again, blockIdx decomposed with wpg * mtt * mtt, partials written at the grid's cap.  grid = G * waves' workgroups * wpg (forms 1, 2, 4:
G * wpg, form 4 with fs waves per workgroup), bytes = grid * floats a workgroup writes * 4:
    dword, staged  KH KW mtt^2 256      tiled  KH KW 256      winograd  6 KH cqp^2      winograd_tiled  6 KH 256

Row chunks (forward and grad-input): the chip is under-filled in all four cases (one round whatever the split), so
finc_row_chunks takes the split with the fewest rows per chunk, H // 8 chunks of ceil(H / nrc) rows; F(4,3), its M-split and
F(2,5) need H >= 16 before they take a second chunk.  A chunk recomputes 2 (3x3) or 4 (5x5) operand rows above its first row and
writes next to another workgroup's rows.
"""

# name -> dict(dims=(B, G, Cq, H, W, KH, KW), conv_form, gradx_waves: pinned from backward_variant like every CONV_CASES entry,
#              plan=the grad-weight plan for 16-byte aligned activations)
GRADW_WALK_CASES = {
    # W % 4 != 0: no 16-byte pieces, the dword form; 129 images x 2 strips on 256 workgroups per group
    "walk_dword": dict(dims=(129, 4, 24, 4, 18, 3, 3), conv_form="strip", gradx_waves=1,
                       plan=dict(form="dword", strip=16, ns=2, units=258, wpg=256, grid=1024, block=64, mtt=2, fs=1,
                                 bytes=1024 * 9 * 4 * 256 * 4)),
    "walk_staged": dict(dims=(129, 4, 12, 4, 24, 3, 3), conv_form="winograd", gradx_waves=1,
                        plan=dict(form="staged", strip=16, ns=2, units=258, wpg=256, grid=1024, block=64, mtt=1, fs=1,
                                  bytes=1024 * 9 * 256 * 4)),
    # 48 channels: 3 x 3 tile pairs, 2048 / (4 * 9) = 56 workgroups per (group, pair): one of them takes a second image
    "walk_tiled_mtt3": dict(dims=(57, 4, 48, 4, 16, 3, 3), conv_form="strip", gradx_waves=2,
                            plan=dict(form="tiled", strip=16, ns=1, units=57, wpg=56, grid=4 * 9 * 56, block=64, mtt=3, fs=1,
                                      bytes=4 * 9 * 56 * 9 * 256 * 4)),
    # ... every workgroup does exactly two
    "walk_tiled_twice": dict(dims=(112, 4, 48, 4, 16, 3, 3), conv_form="strip", gradx_waves=2,
                             plan=dict(form="tiled", strip=16, ns=1, units=112, wpg=56, grid=4 * 9 * 56, block=64, mtt=3, fs=1,
                                       bytes=4 * 9 * 56 * 9 * 256 * 4)),
    # a bank beyond the table (4x4): one tile pair, 2048 / 4 = 512 capped at 256
    "walk_tiled_4x4": dict(dims=(257, 4, 8, 4, 16, 4, 4), conv_form="stream", gradx_waves=1,
                           plan=dict(form="tiled", strip=16, ns=1, units=257, wpg=256, grid=1024, block=64, mtt=1, fs=1,
                                     bytes=1024 * 16 * 256 * 4)),
    # the pair kernel on 16-column strips (W < 32), two waves per workgroup: 1024 / (4 * 2) = 128
    "walk_wino_strip16": dict(dims=(65, 4, 24, 4, 24, 3, 3), conv_form="winograd", gradx_waves=1,
                              plan=dict(form="winograd", strip=16, ns=2, units=130, wpg=128, grid=512, block=128, mtt=2, fs=2,
                                        bytes=512 * 6 * 3 * 24 * 24 * 4)),
    # ... one wave holds all six frequencies (16 channels)
    "walk_wino_fs1": dict(dims=(257, 4, 16, 4, 16, 3, 3), conv_form="winograd", gradx_waves=1,
                          plan=dict(form="winograd", strip=16, ns=1, units=257, wpg=256, grid=1024, block=64, mtt=1, fs=1,
                                    bytes=1024 * 6 * 3 * 16 * 16 * 4)),
    # ... two groups, strips of 32 columns: 1024 / (2 * 2) = 256
    "walk_wino_two_groups": dict(dims=(257, 2, 32, 3, 32, 3, 3), conv_form="strip16", gradx_waves=1,
                                 plan=dict(form="winograd", strip=32, ns=1, units=257, wpg=256, grid=512, block=128, mtt=2, fs=2,
                                           bytes=512 * 6 * 3 * 32 * 32 * 4)),
    # one tile pair per wave, 3 x 3 pairs, F(4,3) transposed on strips of 32 columns
    "walk_winot_mtt3": dict(dims=(57, 4, 48, 4, 32, 3, 3), conv_form="strip", gradx_waves=2,
                            plan=dict(form="winograd_tiled", strip=32, ns=1, units=57, wpg=56, grid=4 * 9 * 56, block=64, mtt=3, fs=1,
                                      bytes=4 * 9 * 56 * 6 * 3 * 256 * 4)),
    # ... F(2,5) transposed on strips of 16 columns
    "walk_winot_5x5_mtt3": dict(dims=(57, 4, 48, 5, 16, 5, 5), conv_form="winograd25", gradx_waves=4,
                                plan=dict(form="winograd_tiled", strip=16, ns=1, units=57, wpg=56, grid=4 * 9 * 56, block=64, mtt=3, fs=1,
                                          bytes=4 * 9 * 56 * 6 * 5 * 256 * 4)),
    "walk_winot_5x5_mtt1": dict(dims=(257, 4, 16, 5, 16, 5, 5), conv_form="winograd25", gradx_waves=1,
                                plan=dict(form="winograd_tiled", strip=16, ns=1, units=257, wpg=256, grid=1024, block=64, mtt=1, fs=1,
                                          bytes=1024 * 6 * 5 * 256 * 4)),
}

# name -> dict(dims, pin: the forward form set_forward_form pins (0: the library's choice), conv_form, gradw, gradx_waves: pinned from
#              backward_variant under that pin, plan=the forward / grad-input plan for 16-byte aligned activations)
ROW_CHUNK_CASES = {
    # 12 waves on 1,024 SIMDs: 17 rows in chunks of 9 and 8
    "chunks_f43": dict(dims=(3, 4, 23, 17, 64, 3, 3), pin=4, conv_form="winograd4", gradw="winograd", gradx_waves=1,
                       plan=dict(form="winograd4", strip=64, ns=1, waves=1, nrc=2, RC=9)),
    # 25 rows: 9, 9 and 7 -- a ragged last chunk shorter than the minimum of 8
    "chunks_f43_three": dict(dims=(3, 4, 23, 25, 64, 3, 3), pin=4, conv_form="winograd4", gradw="winograd", gradx_waves=1,
                             plan=dict(form="winograd4", strip=64, ns=1, waves=1, nrc=3, RC=9)),
    # 32 workgroups of two waves (32 channels: one output tile per wave) on 512 slots
    "chunks_f43_msplit": dict(dims=(8, 4, 32, 17, 64, 3, 3), pin=0, conv_form="winograd4m", gradw="winograd", gradx_waves=1,
                              plan=dict(form="winograd4m", strip=64, ns=1, waves=2, nrc=2, RC=9)),
    # 12 one-wave workgroups on 256 compute units; a chunk recomputes 4 rows
    "chunks_f25": dict(dims=(3, 4, 12, 17, 32, 5, 5), pin=0, conv_form="winograd25", gradw="staged", gradx_waves=1,
                       plan=dict(form="winograd25", strip=32, ns=1, waves=1, nrc=2, RC=9)),
}

# the rows a chunk must hold once there is more than one (the `min_rows` each kernel's launch hands finc_row_chunks), by conv form;
# the forms without row chunks are not listed
MIN_CHUNK_ROWS = {"strip": 4, "strip16": 4, "winograd": 4, "winograd4": 8, "winograd25": 8, "winograd4m": 8}


def walk_lands_on_second_trip(case):
    """The units of the batch's last image -- the image of the last problem, which Unit.slabs() poisons -- all have an index >= wpg
    (a unit is image * ns + strip): a workgroup reaches them on its second trip or later."""
    B, p = case["dims"][0], case["plan"]
    return (B - 1) * p["ns"] >= p["wpg"]
