"""The library calls behind every PackedWeights method (fincflow_amd/ops.py), by name and in order.

A recording proxy stands in for the library object: `_lib.lib()` is what ops.py asks on every call.  What is compared is the list of
entry points that put work on the stream (canonicalise, invariant check, pack, launch); the host-only queries (`*_algo_for`,
`*_supported`, `*_workspace_bytes`) are dropped from it.  The expected lists are written out: pack once per weight version (per
(log_scale, translation) version for the two folds), the invariant check once per version and on the inference path only, one launch
per call.  Every result is also compared with the strict kernel at 1e-5 in helpers.rel_err, the bar of tests/test_gpu_parity.py.
"""
import pytest
import torch

from helpers import ORIENT_FASTFLOW, offset_view, rel_err
from test_gpu_parity import PREMULTIPLIED_CASES

pytestmark = pytest.mark.gpu

TOL = 1e-5

CANON, CHECK = "finc_canonicalize_weights_f32", "finc_check_invariant_f32"
PACK_FWD, PACK_INV = "finc_pack_forward_weights_f32", "finc_pack_inverse_weights_f32"
PACK_FWD_AFFINE, PACK_INV_AFFINE = "finc_pack_forward_weights_affine_f32", "finc_pack_inverse_weights_affine_f32"
FWD_PACKED, INV_PACKED, INV_PREMULTIPLIED = "finc_forward_packed_f32", "finc_inverse_packed_f32", "finc_inverse_packed_premultiplied_f32"
FWD_UNPACKED, INV_UNPACKED = "finc_forward_f32", "finc_inverse_f32"

QUERIES = ("_algo_for", "_supported", "_workspace_bytes")


class Recorder:
    """The library object with every call through it noted by name."""

    def __init__(self, real):
        self._real = real
        self._log = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call

    def take(self):
        """The stream-side calls since the last take()."""
        log, self._log = [n for n in self._log if not n.endswith(QUERIES)], []
        return log


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def rec(dev, monkeypatch):
    from fincflow_amd import _lib
    r = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", r)
    return r


def make_unit(dev, C=16, K=3, seed=0):
    from fincflow_amd import FastFlowUnit
    torch.manual_seed(seed)
    unit = FastFlowUnit(C, C, K).to(dev)
    return unit, unit._cache, (unit._weights(), 4, ORIENT_FASTFLOW)


def acts(dev, shape=(2, 16, 8, 8), seed=1):
    torch.manual_seed(seed)
    return torch.randn(*shape).to(dev)


def close(a, b):
    return rel_err(a.double().cpu().numpy(), b.double().cpu().numpy()) <= TOL


def strict(direction, t, cache, bank):
    """The strict kernel on the cache's canonical bank (call it behind the take() of the calls under test)."""
    from fincflow_amd import ops
    fn = ops.finc_forward if direction > 0 else ops.finc_inverse
    return fn(t.contiguous(), cache.get(*bank), algo="strict")


def bump(unit):
    """An in-place update of one stored bank that leaves every corner tap alone (the centre tap of a 3x3 filter)."""
    with torch.no_grad():
        unit.conv_tr.conv.weight[:, :, 1, 1].mul_(1.5)


def test_build_once_per_weight_version_then_one_launch_per_call(dev, rec):
    unit, cache, bank = make_unit(dev)
    x = acts(dev)
    for _ in range(2):                                # the second round: after an in-place weight update, everything again
        z = cache.forward(x, *bank)
        assert rec.take() == [CANON, CHECK, PACK_FWD, FWD_PACKED]
        z2 = cache.forward(x, *bank)
        assert rec.take() == [FWD_PACKED]
        xr = cache.inverse(z, *bank)
        assert rec.take() == [PACK_INV, INV_PACKED]   # (canonical and checked already: the forward's entry)
        out = torch.empty_like(z)
        assert cache.inverse(z, *bank, out=out) is out
        assert rec.take() == [INV_PACKED]
        assert torch.equal(z, z2) and torch.equal(xr, out)
        assert close(z, strict(+1, x, cache, bank)) and close(xr, strict(-1, z, cache, bank))
        assert rec.take() == [FWD_UNPACKED, INV_UNPACKED]
        bump(unit)


def test_the_training_forward_leaves_the_check_to_the_first_inverse(dev, rec):
    unit, cache, bank = make_unit(dev)
    x = acts(dev)
    z = cache.forward(x, *bank, validate=False)
    assert rec.take() == [CANON, PACK_FWD, FWD_PACKED]
    xr = cache.inverse(z, *bank)
    assert rec.take() == [CHECK, PACK_INV, INV_PACKED]
    cache.forward(x, *bank)
    cache.inverse(z, *bank)
    assert rec.take() == [FWD_PACKED, INV_PACKED]      # checked exactly once
    assert close(z, strict(+1, x, cache, bank)) and close(xr, strict(-1, z, cache, bank))


def test_the_affine_folds_repack_when_their_parameters_change(dev, rec):
    unit, cache, bank = make_unit(dev)
    x = acts(dev)
    torch.manual_seed(2)
    log_scale, translation = (0.2 * torch.randn(16)).to(dev), torch.randn(16).to(dev)

    def affine(t, direction):
        s, tr = log_scale.double().view(1, -1, 1, 1), translation.double().view(1, -1, 1, 1)
        return (t.double() - tr) * torch.exp(-s) if direction > 0 else (t.double() * torch.exp(s) + tr)

    expect_fwd = ([CANON, CHECK, PACK_FWD_AFFINE, FWD_PACKED], [FWD_PACKED], [PACK_FWD_AFFINE, FWD_PACKED], [FWD_PACKED])
    expect_inv = ([PACK_INV_AFFINE, INV_PACKED], [INV_PACKED], [PACK_INV_AFFINE, INV_PACKED], [INV_PACKED])
    for step in range(4):
        if step == 2:                                  # in place: same address, new version
            log_scale.add_(0.1)
            translation.mul_(0.5)
        y = cache.forward_affine(x, *bank, log_scale, translation)
        assert rec.take() == expect_fwd[step]
        xr = cache.inverse_affine(y, *bank, log_scale, translation)
        assert rec.take() == expect_inv[step]
        assert y is not None and xr is not None
        assert close(y, affine(strict(+1, x, cache, bank), +1))
        assert close(xr, strict(-1, affine(y, -1).float(), cache, bank))
        assert rec.take() == [FWD_UNPACKED, INV_UNPACKED]


def test_activations_off_a_16_byte_boundary_leave_the_packed_inverse(dev, rec):
    unit, cache, bank = make_unit(dev)
    z = acts(dev)
    zo = offset_view(z, dev)
    ref = cache.inverse(z, *bank)
    assert rec.take() == [CANON, CHECK, PACK_INV, INV_PACKED]
    xr = cache.inverse(zo, *bank)
    assert rec.take() == [INV_UNPACKED]
    assert close(xr, ref) and close(xr, strict(-1, z, cache, bank))
    rec.take()
    assert cache.inverse(z, *bank, out=offset_view(z, dev)) is not None     # an output off the boundary: the same way out
    assert rec.take() == [INV_UNPACKED]
    zeros = torch.zeros(16, device=dev)
    assert cache.inverse_affine(z, *bank, zeros, zeros) is not None
    assert rec.take() == [PACK_INV_AFFINE, INV_PACKED]
    assert cache.inverse_affine(zo, *bank, zeros, zeros) is None
    assert rec.take() == []


def test_a_filter_without_an_mfma_form_takes_the_unpacked_calls(dev, rec):
    from fincflow_amd import _lib
    assert _lib.lib().finc_inverse_algo_for(4, 8, 8, 9, 9) == _lib.ALGO["strict"]
    assert _lib.lib().finc_forward_algo_for(4, 8, 8, 9, 9) == _lib.ALGO["strict"]
    rec.take()
    unit, cache, bank = make_unit(dev, K=9)
    x = acts(dev)
    z = cache.forward(x, *bank)
    assert rec.take() == [CANON, CHECK, FWD_UNPACKED]
    xr = cache.inverse(z, *bank)
    assert rec.take() == [INV_UNPACKED]
    cache.forward(x, *bank)
    cache.inverse(z, *bank)
    assert rec.take() == [FWD_UNPACKED, INV_UNPACKED]
    zeros = torch.zeros(16, device=dev)
    assert cache.forward_affine(x, *bank, zeros, zeros) is None and cache.inverse_affine(z, *bank, zeros, zeros) is None
    assert rec.take() == []
    assert close(z, strict(+1, x, cache, bank)) and close(xr, strict(-1, z, cache, bank))


def test_the_premultiplied_inverse_shares_the_inverse_bank(dev, rec):
    from fincflow_amd import _lib
    shapes = [c for c in PREMULTIPLIED_CASES if _lib.lib().finc_inverse_premultiplied_supported(c[0], 4, c[1] // 4, c[2], c[3], c[4], c[4])]
    B, C, H, W, K = min(shapes, key=lambda c: c[0] * c[1] * c[2] * c[3])
    rec.take()
    unit, cache, bank = make_unit(dev, C=C, K=K)
    z = acts(dev, (B, C, H, W))
    assert cache.premultiplied_supported((B, C, H, W), *bank)
    assert rec.take() == [CANON, CHECK]
    lead = cache.lead_inverse(*bank)
    assert rec.take() == []
    zp = torch.einsum("gok,bgkhw->bgohw", lead.double(), z.view(B, 4, C // 4, H, W).double()).float().reshape(B, C, H, W).contiguous()
    x_pre = cache.inverse_premultiplied(zp, *bank)
    assert rec.take() == [PACK_INV, INV_PREMULTIPLIED]
    assert cache.inverse_premultiplied(zp, *bank) is not None
    assert rec.take() == [INV_PREMULTIPLIED]
    xr = cache.inverse(z, *bank)
    assert rec.take() == [INV_PACKED]                  # the plain inverse runs on the fragments the premultiplied one packed
    assert cache.inverse_premultiplied(offset_view(zp, dev), *bank) is None
    assert rec.take() == []
    assert x_pre is not None and close(x_pre, strict(-1, z, cache, bank)) and close(xr, x_pre)
    assert _lib.hlp_timeouts() == 0
