"""The compute wave's step of the paired-tile inverse (finc_mfma.hip): the accumulators of the pixel being
solved ARE the S_0 ring entry of their phase (no copy), the wrap zeroing of that entry follows the x-ring write, the FIFO push and
the row shifts, and the wrap test is a scalar every use tests for itself.  In the helper-wave forms the taps (2,0)|(2,1) ride on the
paired tile as well: they OPEN the next step's tile during phase B, and the carry and the reduced blocks are added onto it a step
later.  Every case is held to the bound of tests/test_gpu_paired_tile.py (1e-5 against oracle.inverse_via_f64, max-normalised),
two launches must give the same bits, and no helper wave may time out.  (Measured at the commit that added them: worst 1.40e-6,
profiles/step_trim/step_trim_errors.txt.)

The shapes are the ones where an accumulator set that doubles as an operand, a zeroing that comes later than it used to, or a tile
opened a step early can go wrong: fewer rows than taps (H = 1, 2, 3: idle lanes must keep producing exact zeros), rows that reach lanes 0 and 1 through the
band FIFO with a wrapping lane on EVERY step (W = 16, H = 18 and 34), the bench width (W = 64: a wrap on 16 of 64 steps), masked
channels, the single-wave sector form, the 32-byte and 16-byte forms, and a non-zero accumulator start (premultiplied input, folded
shift).  B = 129 with G = 4 is 516 problems, the smallest count that reaches the helper-wave form.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from helpers import ORIENT_FASTFLOW, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5      # tests/test_gpu_paired_tile.py: TOL
STD = 0.05      # tests/test_gpu_variants.py: bank_std(24, 3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check(dev, B, G, orient, Cq, H, W, seed, sec):
    from fincflow_amd import _lib, ops
    v = _lib.inverse_variant(B, G, Cq, H, W, 3, 3)
    assert v is not None and v["cqp"] == 24 and v["sec"] == sec and v["nw"] == 1, v
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
    print("step_trim B=%d G=%d Cq=%d %dx%d sec=%s err=%.3g" % (B, G, Cq, H, W, v["sec"], e))
    assert e <= TOL, (e, v)
    assert torch.equal(ops.finc_inverse(zt, wc, G, orient, algo="auto"), first)      # two launches, the same bits
    assert _lib.hlp_timeouts() == 0


@pytest.mark.parametrize("H", [1, 2, 3])
def test_fewer_rows_than_taps(H, dev):
    check(dev, 129, 4, ORIENT_FASTFLOW, 24, H, 16, seed=10 + H, sec=3)


@pytest.mark.parametrize("H", [18, 34])
def test_rows_through_the_band_fifo_with_a_wrap_on_every_step(H, dev):
    check(dev, 129, 4, ORIENT_FASTFLOW, 24, H, 16, seed=20 + H, sec=3)


def test_bench_width(dev):
    check(dev, 129, 4, ORIENT_FASTFLOW, 24, 17, 64, seed=64, sec=3)


@pytest.mark.parametrize("Cq", [21, 22, 23])
def test_masked_padding(Cq, dev):
    check(dev, 129, 4, ORIENT_FASTFLOW, Cq, 18, 32, seed=Cq, sec=3)


def test_single_wave_sector_form(dev):
    check(dev, 513, 1, 3, 24, 18, 16, seed=513, sec=2)


@pytest.mark.parametrize("HW,sec", [((18, 24), 1), ((18, 12), 0)])
def test_32_byte_and_16_byte_forms(HW, sec, dev):
    check(dev, 129, 4, ORIENT_FASTFLOW, 24, HW[0], HW[1], seed=30 + sec, sec=sec)


def test_non_zero_accumulator_start(dev):
    """ZPRE (the ring holds the accumulators' start) and a folded shift (a bias in front of the first z-term MFMA) at 34 rows."""
    from fincflow_amd import FastFlowUnit, _lib
    B, C, H, W = 129, 96, 34, 32
    torch.manual_seed(34)
    unit = FastFlowUnit(C, C, 3).to(dev)
    ws = unit._weights()
    assert _lib.inverse_variant(B, 4, C // 4, H, W, 3, 3)["sec"] == 3
    assert _lib.lib().finc_inverse_premultiplied_supported(B, 4, C // 4, H, W, 3, 3) == 1
    wco = oracle.canonicalize(torch.cat(ws).detach().cpu().numpy(), 4, ORIENT_FASTFLOW)
    log_scale = 0.2 * torch.randn(C, device=dev)
    translation = torch.randn(C, device=dev)
    y = torch.randn(B, C, H, W, device=dev)
    z = torch.exp(log_scale).view(1, -1, 1, 1) * y + translation.view(1, -1, 1, 1)
    ref = oracle.inverse_via_f64(z.cpu().numpy(), wco, nthreads=min(oracle.max_threads(), 16))
    with torch.no_grad():
        fused = unit.reverse_affine(y, log_scale, translation)
        assert fused is not None
        e_aff = rel_err(fused.cpu().numpy(), ref)
        lead = unit._cache.lead_inverse(ws, 4, ORIENT_FASTFLOW)
        zp = torch.einsum("gok,bgkhw->bgohw", lead.double(), z.view(B, 4, C // 4, H, W).double()).float().reshape(B, C, H, W).contiguous()
        x_pre = unit._cache.inverse_premultiplied(zp, ws, 4, ORIENT_FASTFLOW)
        assert x_pre is not None
        e_pre = rel_err(x_pre.cpu().numpy(), ref)
        print("step_trim C=%d %dx%d affine err=%.3g premultiplied err=%.3g" % (C, H, W, e_aff, e_pre))
        assert e_aff <= TOL and e_pre <= TOL
        assert torch.equal(unit._cache.inverse_premultiplied(zp, ws, 4, ORIENT_FASTFLOW), x_pre)
        assert torch.equal(unit.reverse_affine(y, log_scale, translation), fused)
    assert _lib.hlp_timeouts() == 0
