"""Launch-regime cases of the per-pixel layers: shapes at which a thread (or, in the mix, a wave) takes MORE THAN ONE trip through its
loop, and the 8-byte alignment class -- each with the plan numbers it must produce, written out by hand.

Everything beside the unit runs one of three launch rules (finc_coupling.h, finc_mix.hip); 256 threads per workgroup, CHIP = 2048:
    rows    grid-stride: grid = min(ceil(items / 256), 4 * CHIP = 8192), a thread loops with idx += grid * 256, so a second trip needs
            more than 8192 * 256 = 2,097,152 items.  items = rows * HW / io; io = 4 floats (8 bf16 elements) when HW is whole pieces and
            every activation pointer is on 16 bytes, else 1.  finc_negate_f32 has its own cap: 1024 workgroups = 262,144 per trip.
    parts   (outer, part) workgroups: P = min(ceil(items / 256), ceil(CHIP / outer)), a thread loops with idx += P * 256; grid = outer * P.
            transform: outer = B, items = (C / 2) * HW / io;  coupling backward: outer = C / 2, items = B * HW / io;
            ActNorm backward and init: outer = C, items = B * HW / io.
    mix     px pixels per lane = 4 (HW % 4 == 0, 16-byte pointers, HW >= 64), 2 (HW % 2 == 0, 8-byte pointers, HW >= 32) or 1;
            big = B * ceil(HW / 16) >= 16384 asks for the large workgroup (8 waves at px 4, 16 otherwise), small for 4 waves; where that
            pair has no instantiation the other size, then the next narrower px.  chunks = B * ceil(HW / (16 * px));
            lds = ceil(C / 16) * (C / 4 + 1) * 256 bytes; workgroups per CU = max(1, min(160 KiB / lds, (px 4: 8, else 16) / waves));
            grid = min(ceil(chunks / waves), 256 * that); a wave loops with chunk += grid * waves.

The numbers are the independent statement: tests/test_pixel_plans_host.py compares them with the library's own answer
(`_lib.pixel_plan`), tests/test_gpu_pixel_regimes.py asserts them again at the pointers' actual alignment and then runs the case
between guards.  Nothing here calls the library.  plan = (io, threads, grid, parts, items, trips, outer, lds).
"""


def _plan(io, threads, grid, parts, items, trips, outer=0, lds=0):
    return dict(io=io, threads=threads, grid=grid, parts=parts, items=items, trips=trips, outer=outer, lds=lds)


CHANNEL_ROW_ENTRIES = ("actnorm", "actnorm_no_logdet", "actnorm_reverse", "bias_relu")

# name -> dict(rule, family, shape (B, C, H, W), align, elem (bytes of the raw / bf16 element), groups, plan, entries)
ROW_CASES = {
    # 33 * 64 rows of 1023 dwords = 2,160,576 items on 8192 workgroups: the second trip is partial (63,424 items)
    "rows_dword": dict(rule="rows", family="channel_rows", shape=(33, 64, 31, 33), align=16, elem=4, groups=0,
                       plan=_plan(1, 256, 8192, 0, 2160576, 2), entries=CHANNEL_ROW_ENTRIES),
    # ... the same rows, every activation one float into its allocation
    "rows_dword_float_aligned": dict(rule="rows", family="channel_rows", shape=(33, 64, 31, 33), align=4, elem=4, groups=0,
                                     plan=_plan(1, 256, 8192, 0, 2160576, 2), entries=("actnorm", "bias_relu")),
    # 2112 rows of 1024 pieces = 2,162,688
    "rows_16_byte": dict(rule="rows", family="channel_rows", shape=(33, 64, 64, 64), align=16, elem=4, groups=0,
                         plan=_plan(4, 256, 8192, 0, 2162688, 2), entries=CHANNEL_ROW_ENTRIES),
    # bf16: pieces of 8 elements, 4224 rows of 512 pieces; its dword form on rows_dword's shape
    "rows_bf16_8_element": dict(rule="rows", family="channel_rows", shape=(66, 64, 64, 64), align=16, elem=2, groups=0,
                                plan=_plan(8, 256, 8192, 0, 2162688, 2), entries=("bias_relu_bf16",)),
    "rows_bf16_dword": dict(rule="rows", family="channel_rows", shape=(33, 64, 31, 33), align=16, elem=2, groups=0,
                            plan=_plan(1, 256, 8192, 0, 2160576, 2), entries=("bias_relu_bf16",)),
    # the grouped lead product: C = 20 (G = 4, Cq = 5) has no mix instantiation; 129 * 4 rows of 4095 dwords / 4096 pieces
    "lead_dword": dict(rule="rows", family="lead", shape=(129, 20, 63, 65), align=16, elem=4, groups=4,
                       plan=_plan(1, 256, 8192, 0, 2113020, 2), entries=("lead_product",)),
    "lead_16_byte": dict(rule="rows", family="lead", shape=(129, 20, 128, 128), align=16, elem=4, groups=4,
                         plan=_plan(4, 256, 8192, 0, 2113536, 2), entries=("lead_product",)),
    # finc_negate_f32 (shape = (1, 1, 1, n)): one element beyond its 1024 workgroups, and a partial fourth trip
    "negate_second_trip": dict(rule="rows", family="negate", shape=(1, 1, 1, 262145), align=16, elem=4, groups=0,
                               plan=_plan(1, 256, 1024, 0, 262145, 2), entries=("negate",)),
    "negate_four_trips": dict(rule="rows", family="negate", shape=(1, 1, 1, 3 * 262144 + 7), align=16, elem=4, groups=0,
                              plan=_plan(1, 256, 1024, 0, 786439, 4), entries=("negate",)),
}

TRANSFORM_ENTRIES = ("coupling", "coupling_no_logdet", "coupling_reverse", "coupling_reverse_logdet")
COUPLING_GRAD_ENTRIES = ("coupling_backward", "coupling_reverse_backward", "coupling_reverse_logdet_backward", "coupling_backward_reconstruct")
ACTNORM_GRAD_ENTRIES = ("actnorm_backward", "actnorm_reverse_backward", "actnorm_backward_reconstruct", "actnorm_init")
WIDE, DWORD = (512, 16, 24, 24), (512, 16, 23, 25)       # HW = 576 = 144 pieces; HW = 575 dwords

PART_CASES = {
    # outer = 512 images: P = min(ceil(items / 256), 2048 / 512 = 4); 8 * 144 = 1152 items on 4 * 256 threads: 2 trips; 8 * 575 = 4600: 5
    "transform_16_byte": dict(rule="parts", family="transform", shape=WIDE, align=16, elem=4, groups=0,
                              plan=_plan(4, 256, 2048, 4, 1152, 2, outer=512), entries=TRANSFORM_ENTRIES),
    "transform_dword": dict(rule="parts", family="transform", shape=DWORD, align=16, elem=4, groups=0,
                            plan=_plan(1, 256, 2048, 4, 4600, 5, outer=512), entries=TRANSFORM_ENTRIES),
    "transform_16_byte_rawbf16": dict(rule="parts", family="transform", shape=WIDE, align=16, elem=2, groups=0,
                                      plan=_plan(4, 256, 2048, 4, 1152, 2, outer=512), entries=TRANSFORM_ENTRIES),
    "transform_dword_rawbf16": dict(rule="parts", family="transform", shape=DWORD, align=16, elem=2, groups=0,
                                    plan=_plan(1, 256, 2048, 4, 4600, 5, outer=512), entries=TRANSFORM_ENTRIES),
    # outer = 8 channel pairs: Q = min(ceil(items / 256), 2048 / 8 = 256); 512 * 144 = 73,728 items on 65,536 threads: 2 trips;
    # 512 * 575 = 294,400: 5
    "coupling_grad_16_byte": dict(rule="parts", family="coupling_grad", shape=WIDE, align=16, elem=4, groups=0,
                                  plan=_plan(4, 256, 2048, 256, 73728, 2, outer=8), entries=COUPLING_GRAD_ENTRIES),
    "coupling_grad_dword": dict(rule="parts", family="coupling_grad", shape=DWORD, align=16, elem=4, groups=0,
                                plan=_plan(1, 256, 2048, 256, 294400, 5, outer=8), entries=COUPLING_GRAD_ENTRIES),
    "coupling_grad_16_byte_rawbf16": dict(rule="parts", family="coupling_grad", shape=WIDE, align=16, elem=2, groups=0,
                                          plan=_plan(4, 256, 2048, 256, 73728, 2, outer=8), entries=COUPLING_GRAD_ENTRIES),
    "coupling_grad_dword_rawbf16": dict(rule="parts", family="coupling_grad", shape=DWORD, align=16, elem=2, groups=0,
                                        plan=_plan(1, 256, 2048, 256, 294400, 5, outer=8), entries=COUPLING_GRAD_ENTRIES),
    # outer = 16 channels: Q = 2048 / 16 = 128, 32,768 threads per channel: 73,728 items 3 trips, 294,400 items 9
    "actnorm_grad_16_byte": dict(rule="parts", family="actnorm_grad", shape=WIDE, align=16, elem=4, groups=0,
                                 plan=_plan(4, 256, 2048, 128, 73728, 3, outer=16), entries=ACTNORM_GRAD_ENTRIES),
    "actnorm_grad_dword": dict(rule="parts", family="actnorm_grad", shape=DWORD, align=16, elem=4, groups=0,
                               plan=_plan(1, 256, 2048, 128, 294400, 9, outer=16), entries=ACTNORM_GRAD_ENTRIES),
}

# the mix: plan = (pixels per lane, 64 * waves per workgroup, grid, waves of the grid, chunks, trips, B, lds); `transposed`: the case
# also runs as the grad-input of finc_mix_backward_f32 (one per regime)
MIX_CASES = {
    # big (256 * 64 = 16384), 4 pixels per lane on 8-wave workgroups: 256 * 16 chunks, 1 workgroup per CU
    "mix_big_px4": dict(rule="mix", family="mix", shape=(256, 12, 32, 32), align=16, elem=4, groups=0,
                        plan=_plan(4, 512, 256, 2048, 4096, 2, outer=256, lds=1024), entries=("mix",), transposed=True),
    # one image fewer: 16320 < 16384, the 4-wave form, two workgroups per CU
    "mix_below_big_px4": dict(rule="mix", family="mix", shape=(255, 12, 32, 32), align=16, elem=4, groups=0,
                              plan=_plan(4, 256, 512, 2048, 4080, 2, outer=255, lds=1024), entries=("mix",), transposed=True),
    # the workload's bank: 6 row tiles, 25 k-steps with the bias
    "mix_big_px4_c96": dict(rule="mix", family="mix", shape=(256, 96, 32, 32), align=16, elem=4, groups=0,
                            plan=_plan(4, 512, 256, 2048, 4096, 2, outer=256, lds=6 * 25 * 256), entries=("mix",), transposed=False),
    # HW = 1023: dwords, 16-wave workgroups, 24 channels = a partial last row tile; 256 * 64 chunks on 4096 waves
    "mix_big_dword": dict(rule="mix", family="mix", shape=(256, 24, 31, 33), align=16, elem=4, groups=0,
                          plan=_plan(1, 1024, 256, 4096, 16384, 4, outer=256, lds=2 * 7 * 256), entries=("mix",), transposed=True),
    # HW = 1054, HW % 4 == 2: 2 pixels per lane, 16-wave (249 * 66 = 16434 >= 16384); 249 * 33 chunks, the last of an image partial
    "mix_big_px2": dict(rule="mix", family="mix", shape=(249, 64, 31, 34), align=16, elem=4, groups=0,
                        plan=_plan(2, 1024, 256, 4096, 8217, 3, outer=249, lds=4 * 17 * 256), entries=("mix",), transposed=True),
    # C = 128 at big: no 4-pixel form, no 16-wave 2-pixel form -> the 4-wave 2-pixel form, two workgroups per CU (lds 67,584)
    "mix_fallback_c128": dict(rule="mix", family="mix", shape=(256, 128, 32, 32), align=16, elem=4, groups=0,
                              plan=_plan(2, 256, 512, 2048, 8192, 4, outer=256, lds=8 * 33 * 256), entries=("mix",), transposed=True),
    # C = 192's only form: dwords on 16 waves; 65 * 64 chunks
    "mix_c192": dict(rule="mix", family="mix", shape=(65, 192, 32, 32), align=16, elem=4, groups=0,
                     plan=_plan(1, 1024, 256, 4096, 4160, 2, outer=65, lds=12 * 49 * 256), entries=("mix",), transposed=False),
    # the 8-byte class: in and out two floats into their allocations.  HW = 64 takes 4 pixels per lane on 16-byte pointers, 2 here
    "mix_align8_c12": dict(rule="mix", family="mix", shape=(3, 12, 8, 8), align=8, elem=4, groups=0,
                           plan=_plan(2, 256, 2, 8, 6, 1, outer=3, lds=1024), entries=("mix",), transposed=True),
    "mix_align8_c96": dict(rule="mix", family="mix", shape=(3, 96, 8, 8), align=8, elem=4, groups=0,
                           plan=_plan(2, 256, 2, 8, 6, 1, outer=3, lds=6 * 25 * 256), entries=("mix",), transposed=False),
    # ... at big: the 16-wave 2-pixel form, 256 * 32 chunks
    "mix_align8_big_px2": dict(rule="mix", family="mix", shape=(256, 12, 32, 32), align=8, elem=4, groups=0,
                               plan=_plan(2, 1024, 256, 4096, 8192, 2, outer=256, lds=1024), entries=("mix",), transposed=True),
}
# what the three 8-byte shapes launch on 16-byte pointers (the form their align-8 run must NOT be)
MIX_ALIGN16_TWIN = {"mix_align8_c12": _plan(4, 256, 1, 4, 3, 1, outer=3, lds=1024),
                    "mix_align8_c96": _plan(4, 256, 1, 4, 3, 1, outer=3, lds=6 * 25 * 256),
                    "mix_align8_big_px2": MIX_CASES["mix_big_px4"]["plan"]}

PIXEL_REGIME_CASES = {**ROW_CASES, **PART_CASES, **MIX_CASES}

# F(2,5) on pointers that are 8-byte but not 16-byte aligned: (B, G, Cq, H, W, KH, KW) -> the forward plan at align 8 (at align 4 the
# same views shifted by one float take the strip kernel).  W = 34: W % 4 == 2; H = 17: two row chunks (plan_cases.py chunks_f25)
WINO5_ALIGN8_CASES = {
    "f25_align8": dict(dims=(2, 4, 8, 9, 32, 5, 5), plan=dict(form="winograd25", strip=32, ns=1, waves=1, nrc=1, RC=9)),
    "f25_align8_w34": dict(dims=(2, 4, 12, 3, 34, 5, 5), plan=dict(form="winograd25", strip=32, ns=2, waves=1, nrc=1, RC=3)),
    "f25_align8_two_chunks": dict(dims=(3, 4, 12, 17, 32, 5, 5), plan=dict(form="winograd25", strip=32, ns=1, waves=1, nrc=2, RC=9)),
}


def multi_trip(case):
    """Does the case state a second trip?  (The two small 8-byte mix cases are there for their form, not their trips.)"""
    return case["plan"]["trips"] >= 2


def last_trip_item(case):
    """The first item index only a LAST trip reaches: (trips - 1) * grid * threads for the rows rule, (trips - 1) * parts * threads
    for the parts rule (an index within one outer unit), (trips - 1) * waves for the mix (a chunk index).  Everything at or above it is
    reached on the last trip alone."""
    p = case["plan"]
    if case["rule"] == "rows":
        return (p["trips"] - 1) * p["grid"] * p["threads"]
    if case["rule"] == "parts":
        return (p["trips"] - 1) * p["parts"] * p["threads"]
    return (p["trips"] - 1) * p["parts"]
