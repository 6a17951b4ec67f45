"""Row shifts read from LDS in the helper-wave paired forms of the c3 inverse (finc_mfma.hip): S_1 and S_2 of the
solved pixel are one LDS read per operand register -- the x-ring cell of lane p - a, or for the lanes p < a the hand-over FIFO word of
the band above -- instead of a DPP move merged with a FIFO pop.  Every case is held to the bound of tests/test_gpu_step_trim.py
(1e-5 against oracle.inverse_via_f64, max-normalised), two launches must give the same bits, and no helper wave may time out.
B = 129 with G = 4 is 516 problems, the smallest count that reaches the helper-wave form (sec == 3).

The shapes are the smallest at which a shift that comes from memory can go wrong:
  H = 1, 2, 3 at W = 16     no band hand-over: what stands for the rows above the image must read as zeros;
  H = 18, 34 at W = 16      D = 1: lanes 0 and 1 take the pixel lanes 14 and 15 solved in the SAME step (no FIFO: the ring cell 16 lanes
                            up), across one and two hand-overs, with a wrapping lane on every step;
  H = 33 at W = 32          D = 17: a FIFO ring of 16 slots that wraps inside the run;
  H = 17 at W = 64          the bench width, D = 49: the deepest FIFO ring the k-step block holds;
  Cq = 21, 22, 23           masked channels at 18 x 32;
  premultiplied input (ZPRE) and a folded shift at 18 x 32.
ORIENT_FASTFLOW throughout, so all four flips run.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from helpers import ORIENT_FASTFLOW, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5      # tests/test_gpu_step_trim.py: TOL
STD = 0.05      # tests/test_gpu_variants.py: bank_std(24, 3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check(dev, Cq, H, W, seed):
    from fincflow_amd import _lib, ops
    B, G, orient = 129, 4, ORIENT_FASTFLOW
    v = _lib.inverse_variant(B, G, Cq, H, W, 3, 3)
    assert v is not None and v["cqp"] == 24 and v["sec"] == 3 and v["nw"] == 1, v
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
    print("lds_shifts B=%d G=%d Cq=%d %dx%d sec=%s err=%.3g" % (B, G, Cq, H, W, v["sec"], e))
    assert e <= TOL, (e, v)
    assert torch.equal(ops.finc_inverse(zt, wc, G, orient, algo="auto"), first)      # two launches, the same bits
    assert _lib.hlp_timeouts() == 0


@pytest.mark.parametrize("H", [1, 2, 3])
def test_no_band_above_reads_as_zeros(H, dev):
    check(dev, 24, H, 16, seed=100 + H)


@pytest.mark.parametrize("H", [18, 34])
def test_same_step_hand_over_at_16_columns(H, dev):
    check(dev, 24, H, 16, seed=200 + H)


def test_fifo_ring_wraps_inside_the_run(dev):
    check(dev, 24, 33, 32, seed=233)


def test_bench_width(dev):
    check(dev, 24, 17, 64, seed=264)


@pytest.mark.parametrize("Cq", [21, 22, 23])
def test_masked_padding(Cq, dev):
    check(dev, Cq, 18, 32, seed=300 + Cq)


def test_premultiplied_input_and_folded_shift(dev):
    """ZPRE (the ring holds the accumulators' start) and a folded shift (a bias in front of the first z-term MFMA) at 18 x 32."""
    from fincflow_amd import FastFlowUnit, _lib
    B, C, H, W = 129, 96, 18, 32
    torch.manual_seed(18)
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
        print("lds_shifts C=%d %dx%d affine err=%.3g premultiplied err=%.3g" % (C, H, W, e_aff, e_pre))
        assert e_aff <= TOL and e_pre <= TOL
        assert torch.equal(unit._cache.inverse_premultiplied(zp, ws, 4, ORIENT_FASTFLOW), x_pre)
        assert torch.equal(unit.reverse_affine(y, log_scale, translation), fused)
    assert _lib.hlp_timeouts() == 0
