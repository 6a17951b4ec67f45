"""The paired remainder tile of the one-wave 3x3 inverse (finc_mfma.hip): on the 24-channel bank the 4-row blocks
of the taps (0,1)|(0,2) and (1,0)|(1,1) ride on one 16-row fragment per k-step, and the partner taps' half of its result is
carried into the lane's next pixel.  Every case is held to the oracle's fp64 path with the bound tests/test_gpu_parity.py
uses for the wave kernel (1e-5, max-normalised).

What can go wrong is the carry: across the band hand-over (H = 17: one, H = 33: two), at a lane's first column (W = 16: every
16th step, W = 32), in the flipped groups, with masked channels in the last group of four, with the premultiplied input and
with a folded shift (a non-zero start of the accumulators).  B in {1, 2} are the problem counts of the role-split kernel
(untouched); B = 129 / 130 with G = 4 (516 / 520 problems) reach this kernel's helper-wave form and G = 1 with B = 513 its
single-wave sector-pairing form; W = 24 / 12 its 32-byte and 16-byte forms.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from helpers import ORIENT_FASTFLOW, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5      # tests/test_gpu_parity.py: TOL, the wave kernel against oracle.inverse_via_f64
STD = 0.05      # tests/test_gpu_variants.py: bank_std(24, 3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


SPLIT = 4       # the variant's `sec` of the role-split kernel (finc_split.hip); 0 .. 3: the forms of the wave kernel


def check(dev, B, G, orient, Cq, H, W, seed, sec):
    from fincflow_amd import _lib, ops
    v = _lib.inverse_variant(B, G, Cq, H, W, 3, 3)
    assert v is not None and v["cqp"] == 24 and v["sec"] == sec, v
    assert sec == SPLIT or v["nw"] == 1, v
    rng = np.random.default_rng(seed)
    ws = oracle.make_stored_weights(G, Cq, 3, 3, orient=orient, seed=seed, std=STD)
    wco = oracle.canonicalize(ws, G, orient)
    x = rng.standard_normal((B, G * Cq, H, W)).astype(np.float32)
    nthr = min(oracle.max_threads(), 16)
    z = oracle.forward_f32(x, wco, G, orient, nthreads=nthr)
    ref = oracle.inverse_via_f64(z, wco, G, orient, nthreads=nthr)
    wc = ops.canonicalize(t(ws, dev), G, orient)
    zt = t(z, dev)
    first = ops.finc_inverse(zt, wc, G, orient, algo="auto")
    e = rel_err(first.cpu().numpy(), ref)
    print("paired_tile B=%d G=%d Cq=%d %dx%d sec=%s err=%.3g" % (B, G, Cq, H, W, v and v["sec"], e))
    assert e <= TOL, (e, v)
    assert torch.equal(ops.finc_inverse(zt, wc, G, orient, algo="auto"), first)      # two launches, the same bits
    assert _lib.hlp_timeouts() == 0


@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("H", [16, 17, 33])
@pytest.mark.parametrize("B", [1, 2, 129])
def test_main_grid_all_four_orientations(B, H, W, dev):
    """G = 4 with the FastFlowUnit orientations: every group flips differently.  B = 129: the helper-wave form; B = 1, 2: the
    role-split kernel, asserted so that what these legs cover stays on record."""
    check(dev, B, 4, ORIENT_FASTFLOW, 24, H, W, seed=100 * H + W + B, sec=3 if B == 129 else SPLIT)


@pytest.mark.parametrize("orient", [0, 1, 2, 3])
def test_single_wave_sector_pairing_form(orient, dev):
    """An odd problem count keeps the bank's one-wave row but not its helper waves; one orientation at a time."""
    check(dev, 513, 1, orient, 24, 17, 16, seed=7 + orient, sec=2)


@pytest.mark.parametrize("HW,sec", [((17, 24), 1), ((18, 12), 0)])
def test_32_byte_and_16_byte_forms(HW, sec, dev):
    check(dev, 129, 4, ORIENT_FASTFLOW, 24, HW[0], HW[1], seed=sec, sec=sec)


@pytest.mark.parametrize("Cq", [21, 22, 23])
def test_masked_padding(Cq, dev):
    check(dev, 130, 4, ORIENT_FASTFLOW, Cq, 17, 32, seed=Cq, sec=3)


@pytest.mark.parametrize("C", [96, 88])
def test_premultiplied_input_and_folded_actnorm(C, dev):
    """ZPRE (alone and through reverse_after_mix) and a folded shift, at 33 rows: a carry that is wrongly zero or wrongly kept
    is invisible with a zero start of the accumulators."""
    from fincflow_amd import FastFlowUnit, _lib, glow, ops
    B, H, W = 129, 33, 32
    torch.manual_seed(C)
    unit = FastFlowUnit(C, C, 3).to(dev)
    ws = unit._weights()
    assert _lib.inverse_variant(B, 4, C // 4, H, W, 3, 3)["sec"] == 3
    assert _lib.lib().finc_inverse_premultiplied_supported(B, 4, C // 4, H, W, 3, 3) == 1
    wco = oracle.canonicalize(torch.cat(ws).detach().cpu().numpy(), 4, ORIENT_FASTFLOW)
    nthr = min(oracle.max_threads(), 16)
    log_scale = 0.2 * torch.randn(C, device=dev)
    translation = torch.randn(C, device=dev)
    y = torch.randn(B, C, H, W, device=dev)
    z = torch.exp(log_scale).view(1, -1, 1, 1) * y + translation.view(1, -1, 1, 1)
    ref = oracle.inverse_via_f64(z.cpu().numpy(), wco, nthreads=nthr)
    with torch.no_grad():
        fused = unit.reverse_affine(y, log_scale, translation)                  # non-zero accumulator start
        assert fused is not None
        e_aff = rel_err(fused.cpu().numpy(), ref)
        lead = unit._cache.lead_inverse(ws, 4, ORIENT_FASTFLOW)
        zp = torch.einsum("gok,bgkhw->bgohw", lead.double(), z.view(B, 4, C // 4, H, W).double()).float().reshape(B, C, H, W).contiguous()
        x_pre = unit._cache.inverse_premultiplied(zp, ws, 4, ORIENT_FASTFLOW)   # the kernel without its z-term
        assert x_pre is not None
        e_pre = rel_err(x_pre.cpu().numpy(), ref)
        print("paired_tile C=%d affine err=%.3g premultiplied err=%.3g" % (C, e_aff, e_pre))
        assert e_aff <= TOL and e_pre <= TOL
        assert torch.equal(unit._cache.inverse_premultiplied(zp, ws, 4, ORIENT_FASTFLOW), x_pre)
        assert torch.equal(unit.reverse_affine(y, log_scale, translation), fused)
        assert ops.mix_supported(96)
        if C == 96:                                                              # through the mix in front of the unit (no mix kernel at 88)
            an = glow.ActNorm(C).to(dev)
            mix = glow.Conv1x1(C).to(dev)
            an.log_scale.copy_(log_scale)
            an.translation.copy_(translation)
            an.mark_initialized()
            u = torch.randn(B, C, H, W, device=dev)
            got = unit.reverse_after_mix(u, mix, an.reverse_affine_params())
            assert got is not None
            zz = an.reverse(mix.reverse(u))
            zz = zz[0] if isinstance(zz, tuple) else zz
            want = oracle.inverse_via_f64(zz.cpu().numpy(), wco, nthreads=nthr)
            e_mix = rel_err(got.cpu().numpy(), want)
            print("paired_tile C=%d reverse_after_mix err=%.3g" % (C, e_mix))
            assert e_mix <= TOL
    assert _lib.hlp_timeouts() == 0
