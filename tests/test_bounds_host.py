"""The guard-band and isolation checks of tests/test_gpu_bounds.py, proven on the CPU (no GPU needed).

Two halves.  (1) The helpers catch planted defects: plain torch stand-ins for a kernel, each with ONE defect of the kind the GPU
tests exist for, run through the same three assertions -- guards intact, output NaN-free and bit-equal to the plain call, clean
part bit-equal under poison -- and each defect is reported by exactly the assertion meant for it.  (2) The references have the
isolation property themselves: the oracle (plain C) and the float64 formulas of the per-pixel layers keep a NaN inside the
problem it was put in, so a leak seen on the GPU is the kernel's, not the test's.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from helpers import (GUARD_BITS, ORIENT_FASTFLOW, actnorm_ref, broken_guards, coupling_ref, guard_elements, guarded, guards_intact, isolation_check, nan_filled,
                     poison, poison_inf, same_bits)

CPU = torch.device("cpu")
IMAGES, PIXELS = 3, 20


# A stand-in "kernel": out[b, p] = 2 * in[b, p] + 1 on flat storage (store, offset of the first element), as a kernel sees memory.
def good(src, s0, dst, d0, n):
    dst[d0:d0 + n] = 2.0 * src[s0:s0 + n] + 1.0


def writes_past(src, s0, dst, d0, n):
    good(src, s0, dst, d0, n)
    dst[d0 + n] = 0.0


def writes_before(src, s0, dst, d0, n):
    good(src, s0, dst, d0, n)
    dst[d0 - 1] = 0.0


def reads_past_times_zero(src, s0, dst, d0, n):
    good(src, s0, dst, d0, n)
    dst[d0 + n - 1] += 0.0 * src[s0 + n]


def other_image_times_zero(src, s0, dst, d0, n):
    good(src, s0, dst, d0, n)
    dst[d0 + PIXELS:d0 + 2 * PIXELS] += 0.0 * src[s0:s0 + PIXELS]          # image 1 "reads" image 0 with a zero weight


def verdict(kernel):
    """The three assertions of the GPU tests on a stand-in: which of them hold."""
    x = torch.randn(IMAGES, PIXELS, generator=torch.Generator().manual_seed(1))
    n = x.numel()

    def plain(inp):
        src = torch.cat([inp.flatten(), torch.tensor([7.0])])              # a fresh allocation has finite slack behind it
        dst = torch.zeros(n + 2)
        kernel(src, 0, dst, 1, n)
        return dst[1:1 + n].view(x.shape).clone()

    want = plain(x)
    xv, xb = guarded(x, CPU)
    ov, ob = guarded(nan_filled(x.shape, x.dtype, CPU), CPU)
    g = guard_elements(x)
    kernel(xb, g, ob, g, n)
    guards = guards_intact(xb, xv) and guards_intact(ob, ov)
    output = not bool(torch.isnan(ov).any()) and same_bits(ov, want)
    reach = torch.zeros(x.shape, dtype=torch.bool)
    reach[0] = True
    isolation = True
    for dirty_in in (poison(x, 0), poison_inf(x, 0)):
        leaked, reached = isolation_check(want, plain(dirty_in), reach)
        assert reached
        isolation = isolation and leaked == 0
    return dict(guards=guards, output=output, isolation=isolation), broken_guards(ob, ov)


@pytest.mark.parametrize("kernel,fails,side", [
    (good, None, []),
    (writes_past, "guards", ["back"]),
    (writes_before, "guards", ["front"]),
    (reads_past_times_zero, "output", []),
    (other_image_times_zero, "isolation", []),
], ids=lambda v: getattr(v, "__name__", None))
def test_each_planted_defect_is_caught_by_its_own_assertion(kernel, fails, side):
    got, broken = verdict(kernel)
    assert got == {k: k != fails for k in ("guards", "output", "isolation")}, (kernel.__name__, got)
    assert broken == side


def test_guarded_layout():
    """[front | payload | back]: guards of max(4096, 16 H W) elements rounded up to 128 (512 bytes), 4096 for anything that is not a
    map; one fixed quiet-NaN pattern; lead_floats shifts the payload by one element; fp64 counts elements."""
    x = torch.randn(2, 3, 20, 24)
    v, b = guarded(x, CPU)
    g = guard_elements(x)
    assert g == 16 * 20 * 24 == 7680 and g % 128 == 0 and b.numel() == 2 * g + x.numel()
    assert torch.equal(v, x) and v.is_contiguous() and v.data_ptr() - b.data_ptr() == 4 * g
    assert bool((b.view(torch.int32)[:g] == GUARD_BITS[4]).all()) and bool(torch.isnan(b[:g]).all()) and bool(torch.isnan(b[-g:]).all())
    assert guard_elements(torch.zeros(2, 3, 5, 5)) == 4096 and guard_elements(torch.zeros(7)) == 4096 and guard_elements(torch.zeros(9, 9)) == 4096
    assert guard_elements(torch.zeros(1, 1, 17, 17)) == 4736                       # 4624 rounded up to 128
    v1, b1 = guarded(x, CPU, lead_floats=1)
    assert v1.data_ptr() - b1.data_ptr() == 4 * g + 4 and guards_intact(b1, v1) and torch.equal(v1, x)
    b1[g] = 0.0                                                                      # the lead element belongs to the front guard
    assert not guards_intact(b1, v1) and broken_guards(b1, v1) == ["front"]
    d = torch.randn(5, dtype=torch.float64)
    vd, bd = guarded(d, CPU)
    assert bd.numel() == 2 * 4096 + 5 and bool((bd.view(torch.int64)[:4096] == GUARD_BITS[8]).all()) and bool(torch.isnan(bd[:4096]).all())
    bd[-1] = float("nan")                                                            # a NaN of another bit pattern is a write too
    assert not guards_intact(bd, vd)
    assert torch.isnan(poison(x, (1, 2))[1, 2]).all() and torch.isinf(poison_inf(x, (0,))[0]).all() and torch.isfinite(x).all()


# (B, G, Cq, H, W, KH, KW, orient): shapes of tests/test_gpu_bounds.py, one per orientation set -- FastFlow's four corners, a
# single BR bank, four groups of a 2x2 bank
ORACLE_SHAPES = [(3, 4, 5, 9, 11, 3, 3, ORIENT_FASTFLOW), (3, 1, 19, 21, 36, 3, 3, 3), (4, 4, 2, 6, 8, 2, 2, ORIENT_FASTFLOW)]


@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=lambda s: "B%d_G%d_Cq%d_%dx%d_k%dx%d_o%d" % s)
def test_the_oracle_keeps_a_nan_inside_its_slab(shape):
    B, G, Cq, H, W, KH, KW, orient = shape
    ws = oracle.make_stored_weights(G, Cq, KH, KW, orient=orient, seed=3, std=0.05 * min(1.0, (24.0 / Cq) ** 0.5))
    wc = oracle.canonicalize(ws, G, orient)
    z = np.random.default_rng(5).standard_normal((B, G * Cq, H, W)).astype(np.float32)
    n = B * G
    for fn in (oracle.inverse_f32, oracle.inverse_via_f64, oracle.forward_f32):
        clean = torch.from_numpy(fn(z, wc, G, orient))
        for p in dict.fromkeys((min(4 * (n // 8) + 1, n - 1), n - 1, 0)):
            slab = (p // G, slice((p % G) * Cq, (p % G + 1) * Cq))
            dirty = torch.from_numpy(fn(poison(torch.from_numpy(z), slab).numpy(), wc, G, orient))
            reach = torch.zeros(clean.shape, dtype=torch.bool)
            reach[slab] = True
            leaked, reached = isolation_check(clean, dirty, reach)
            assert leaked == 0 and reached and bool(torch.isnan(dirty[slab]).any()), (fn.__name__, p, leaked)


def test_the_float64_formulas_of_the_per_pixel_layers_keep_a_nan_where_it_was_put():
    g = torch.Generator().manual_seed(2)
    B, C, H, W = 3, 6, 5, 3
    x, raw = torch.randn(B, C, H, W, generator=g, dtype=torch.float64), torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    a, b = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    mat = torch.randn(C, C, generator=g, dtype=torch.float64)

    def held(fn, inp, idx, out_idx):
        clean, dirty = fn(inp), fn(poison(inp, idx))
        reach = torch.zeros(clean.shape, dtype=torch.bool)
        reach[out_idx] = True
        leaked, reached = isolation_check(clean, dirty, reach)
        return leaked == 0 and reached

    image, chan, pixel = (1,), (slice(None), 4), (1, slice(None), 2, 2)
    for direction in (1, -1):
        assert held(lambda v: coupling_ref(x, v, a, b, direction)[0], raw, image, image)
        assert held(lambda v: coupling_ref(v, raw, a, b, direction)[0], x, image, image)
        assert held(lambda v: actnorm_ref(v, a, b, direction)[0], x, chan, chan)
    assert held(lambda v: coupling_ref(x, v, a, b, 1)[1], raw, image, image)                     # logdet[b]
    assert held(lambda v: torch.einsum("oi,bihw->bohw", mat, v), x, pixel, pixel)              # the 1x1 mix
    assert held(lambda v: torch.einsum("bohw,bihw->oi", raw, v), x, chan, chan)                # grad_mat: column i0
