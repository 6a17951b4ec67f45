"""Host side of the image boundary (include/finc.h: finc_image_encode_u8_f32, finc_image_encode_f32, finc_image_decode_f32,
finc_image_decode_u8, finc_image_workspace_bytes): the exported symbols and the ABI version gate, the refusal order of the
four entry points with fake pointers, the workspace bound, the constants `FlowSequential.image_boundary_constants` composes, and the
matcher of `FlowSequential.fuse_image_boundary` on CPU tensors, where every layer keeps its PyTorch lines.  No GPU needed, the library
built."""
import math
import os
import re

import pytest
import torch

import flow_twin
from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODES = ("finc_image_encode_u8_f32", "finc_image_encode_f32")
DECODES = ("finc_image_decode_f32", "finc_image_decode_u8")
BIG = 1 << 40
DIMS = (2, 3, 8, 16)
ENC = (1.0 / 256, 1e-6, 256.0, 1e-6, 0.0)            # mult, lo, hi, hi_comp, logdet_const
DEC = (256.0, 0.0, 256.0, 0.0)                       # inv_mult, off, hi, logdet_const
MODEL = dict(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 16, 16), coupling_width=16)


def test_the_five_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in ENCODES + DECODES + ("finc_image_workspace_bytes",):
        assert name in _lib.SYMBOLS and name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.finc_image_encode_u8_f32.argtypes) == len(L.finc_image_encode_f32.argtypes) == 17
    assert len(L.finc_image_decode_f32.argtypes) == len(L.finc_image_decode_u8.argtypes) == 15
    from fincflow_amd import ops
    assert callable(ops.finc_image_encode) and callable(ops.finc_image_decode)


def test_version_is_115_and_a_114_library_is_told_to_rebuild(tmp_path):
    assert _lib.IMAGE_BOUNDARY_ABI_VERSION == 115
    assert _lib.lib().finc_version() >= _lib.IMAGE_BOUNDARY_ABI_VERSION
    out = load_stub_library(tmp_path, 114)
    assert "= 114" in out and "115" in out and "rebuild it" in out and "finc_image_encode_u8_f32" in out, out


@pytest.mark.parametrize("entry", ENCODES)
def test_encode_refusal_order(entry):
    """NULL -> 1, dims (odd sides under squeeze, a squeeze flag that is neither 0 nor 1, out on the image where that permutes) -> 2,
    alignment (fp32 tensors on 4 bytes; a uint8 image has no rule) -> 7, workspace -> 4, in that order."""
    L = _lib.lib()
    u8 = entry == "finc_image_encode_u8_f32"
    fn = getattr(L, entry)
    img, noise, out, ld, ws = _p(0x100000), _p(0x200000), _p(0x300000), _p(0x400000), _p(0x500000)

    def f(img=img, noise=noise, out=out, ld=ld, dims=DIMS, squeeze=1, ws=ws, nbytes=BIG):
        return fn(img, noise, out, ld, *dims, squeeze, *ENC, ws, nbytes, None)
    for name in ("img", "out", "ld"):
        assert f(**{name: None}) == 1, name
    assert f(noise=None, ws=None) == 4                                       # the noise is optional: down to the workspace
    assert f(img=None, dims=(0, 3, 8, 16)) == 1                              # (NULL comes before the dims)
    for dims in ((0, 3, 8, 16), (2, 0, 8, 16), (2, 3, 0, 16), (2, 3, 8, 0), (-1, 3, 8, 16), (2, 3, 7, 16), (2, 3, 8, 15),
                 (1, 1 << 10, 1 << 10, 1 << 10), (1, 1, 1 << 16, 1 << 16)):
        assert f(dims=dims) == 2, dims
    assert f(dims=(2, 3, 7, 15), squeeze=0, ws=None) == 4                    # odd sides are fine without squeeze
    assert f(squeeze=2) == 2 and f(squeeze=-1) == 2
    assert f(out=img) == 2 and f(out=noise) == 2                             # squeeze permutes: no in-place
    assert f(out=img, squeeze=0, ws=None) == (2 if u8 else 4)                # without squeeze an fp32 image may be overwritten
    assert f(out=_p(0x300002), dims=(0, 3, 8, 16)) == 2                      # (dims come before the alignment)
    for name, base in (("noise", 0x200000), ("out", 0x300000), ("ld", 0x400000)):
        assert f(**{name: _p(base + 2)}) == 7, name
        assert f(**{name: _p(base + 4)}, ws=None) == 4, name                 # on 4 bytes: accepted (the dword form)
    assert f(img=_p(0x100001), ws=None) == (4 if u8 else 7)
    assert f(img=_p(0x100002), ws=None) == (4 if u8 else 7)
    assert f(img=_p(0x100004), ws=None) == 4
    assert f(out=_p(0x300002), ws=None) == 7                                 # (alignment comes before the workspace)
    need = L.finc_image_workspace_bytes(*DIMS, 1)
    assert f(ws=None) == 4 and f(nbytes=need - 1) == 4 and f(nbytes=0) == 4 and f(ws=_p(0x500002)) == 4


@pytest.mark.parametrize("entry", DECODES)
def test_decode_refusal_order(entry):
    L = _lib.lib()
    u8 = entry == "finc_image_decode_u8"
    fn = getattr(L, entry)
    z, out, ld, ws = _p(0x100000), _p(0x300000), _p(0x400000), _p(0x500000)

    def f(z=z, out=out, ld=ld, dims=DIMS, unsqueeze=1, consts=DEC, ws=ws, nbytes=BIG):
        return fn(z, out, ld, *dims, unsqueeze, *consts, ws, nbytes, None)
    assert f(z=None) == 1 and f(out=None) == 1
    assert f(z=None, dims=(0, 3, 8, 16)) == 1
    for dims in ((0, 3, 8, 16), (2, 0, 8, 16), (2, 3, 0, 16), (2, 3, 8, 0), (2, 3, 7, 16), (2, 3, 8, 15), (1, 1 << 10, 1 << 10, 1 << 10)):
        assert f(dims=dims) == 2, dims
    assert f(unsqueeze=3) == 2
    assert f(out=z) == 2
    assert f(out=z, unsqueeze=0, ws=None) == (2 if u8 else 4)
    for hi in (0.5, 257.0, float("nan")):                                     # the uint8 clamp's top must fit a byte
        assert f(consts=(256.0, 0.0, hi, 0.0), ws=None) == (2 if u8 else 4), hi
    assert f(z=_p(0x100002), dims=(0, 3, 8, 16)) == 2
    assert f(z=_p(0x100002)) == 7 and f(ld=_p(0x400002)) == 7
    assert f(out=_p(0x300001), ws=None) == (4 if u8 else 7)
    assert f(out=_p(0x300004), ws=None) == 4 and f(z=_p(0x100004), ws=None) == 4
    need = L.finc_image_workspace_bytes(*DIMS, 1)
    assert f(ws=None) == 4 and f(nbytes=need - 1) == 4 and f(ws=_p(0x500002)) == 4
    # without a log-det the ladder never looks at the workspace: every refusal above it still comes, status 4 never
    assert f(ld=None, ws=None, nbytes=0, dims=(2, 3, 7, 16)) == 2
    assert f(ld=None, ws=None, nbytes=0, z=_p(0x100002)) == 7


def launch_constants():
    text = open(os.path.join(REPO, "fincflow_amd", "csrc", "finc_coupling.h")).read()
    threads = int(re.search(r"constexpr int CPL_THREADS = (\d+);", text).group(1))
    wgs = re.search(r"constexpr long long CPL_CHIP_WGS = (\d+) \* (\d+);", text)
    return threads, int(wgs.group(1)) * int(wgs.group(2))


def test_workspace_bytes_follow_cpl_partials_bound():
    """finc_coupling.h: cpl_partials_bound(items, outer) = min(outer * ceil(items / 256), 2048 + outer) floats, for the form with the
    most items (one position per item), padded to 256 bytes; > 0 for any arguments; never shrinks when B, H or W grows."""
    L = _lib.lib()
    threads, chip = launch_constants()

    def bound(B, C, H, W, squeeze):
        items = C * (H // 2) * (W // 2) if squeeze else C * H * W
        n = 4 * min(B * -(-items // threads), chip + B)
        return max(256, -(-n // 256) * 256)
    for dims in ((2, 1, 2, 2), (3, 3, 6, 10), (2, 3, 64, 64), (1024, 3, 64, 64), (64, 3, 256, 256), (5000, 1, 28, 28)):
        for squeeze in (0, 1):
            assert L.finc_image_workspace_bytes(*dims, squeeze) == bound(*dims, squeeze), (dims, squeeze)
    assert L.finc_image_workspace_bytes(0, 3, 8, 8, 1) == 256 and L.finc_image_workspace_bytes(2, 3, -8, 8, 0) == 256
    last = 0
    for B in (1, 2, 7, 64, 1024, 4096):
        got = L.finc_image_workspace_bytes(B, 3, 64, 64, 1)
        assert got >= last
        last = got


# ---------------------------------------------------------------------------------------------------------------------------------
# the model on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def model64(seed=1, **changes):
    import numpy as np
    from fincflow_amd import glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = glow.create_model(**dict(MODEL, **changes))
    flow_twin.randomise(model, seed=seed, actnorm=True)
    return flow_twin.twin_of(model)


@pytest.fixture(scope="module")
def twin():
    return model64()


@pytest.fixture(scope="module")
def pixels():
    return torch.randint(0, 256, (3, 3, 16, 16), generator=torch.Generator().manual_seed(5)).double()


def test_the_flag_is_off_by_default_and_set_per_instance(twin):
    from fincflow_amd import FlowSequential
    assert FlowSequential.fuse_image_boundary is False and twin.fuse_image_boundary is False
    assert "fuse_image_boundary" not in "".join(twin.state_dict().keys())


def test_the_composed_constants_against_a_float64_restatement(twin):
    """create_model's alpha = 1e-6 and 256 levels, from the fp32 values the buffers hold."""
    from fincflow_amd import glow
    k = twin.image_boundary_constants()
    alpha = float(torch.tensor([-1e-6], dtype=torch.float32).double())       # Normalization(-alpha, ...).translation as stored
    s2 = float(torch.tensor([1 / (1 - 2e-6)], dtype=torch.float32).double())
    norms = [m for m in twin if isinstance(m, glow.Normalization)]
    assert [float(n.translation) for n in norms] == [0.0, alpha] and [float(n.scale) for n in norms] == [256.0, s2]
    for v in (0.0, 0.25, 17.5, 255.0, 255.99999994, 256.0):
        y = (v / 256.0 - alpha) / s2
        assert abs(k["mult"] * v + k["lo"] - y) <= 4e-16
        assert abs(k["mult"] * (k["hi"] - v) + k["hi_comp"] - (1.0 - y)) <= 4e-16
        assert abs(k["inv_mult"] * y + k["off"] - v) <= 1e-13
    assert k["hi"] == 256.0
    assert abs(k["mult"] - 1.0 / (256.0 * s2)) <= 1e-18 and abs(k["sum_log_scale"] - (math.log(256.0) + math.log(s2))) <= 1e-15
    assert abs(k["hi_comp"] - (1.0 - k["lo"] - k["mult"] * 256.0)) <= 1e-18 and 0.9e-6 < k["hi_comp"] < 1.1e-6
    assert twin.image_boundary_constants() is k                              # cached per version of the buffers
    with torch.no_grad():
        norms[0].scale.mul_(1.0)
    assert twin.image_boundary_constants() is not k and twin.image_boundary_constants() == k


def test_on_cpu_tensors_the_flag_changes_no_bit(twin, pixels):
    """CPU tensors and fp64 take the layers exactly as with the flag off: forward, sample, encode / decode."""
    outs = []
    for flag in (False, True):
        twin.fuse_image_boundary = flag
        with torch.no_grad():
            torch.manual_seed(3)
            z, lp = twin(pixels)
            torch.manual_seed(3)
            zs, lp2 = twin.encode(pixels)
            back, lq = twin.decode(zs, with_log_prob=True)
            torch.manual_seed(4)
            x, x_true = twin.sample(3, also_true_inverse=True)
            torch.manual_seed(4)
            xq = twin.sample_with_log_prob(3)
        outs.append([z, lp, lp2, back, lq, x, x_true, *xq, *zs])
    twin.fuse_image_boundary = False
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][3], pixels)                                   # decode(encode(x)) is x: the floor undoes the noise


def test_bits_per_dim_is_the_formula(twin, pixels):
    with torch.no_grad():
        torch.manual_seed(8)
        got = twin.bits_per_dim(pixels)
        torch.manual_seed(8)
        want = -twin.log_prob(pixels) / (3 * 16 * 16 * math.log(2.0))
    assert got.shape == (3,) and torch.equal(got, want)


def test_sample_uint8_is_the_clamp_of_sample_and_needs_the_boundary_layers(twin):
    for flag in (False, True):
        twin.fuse_image_boundary = flag
        torch.manual_seed(12)
        u = twin.sample_uint8(4)
        torch.manual_seed(12)
        x = twin.sample(4)[0]
        assert u.dtype == torch.uint8 and u.shape == (4, 3, 16, 16) and torch.equal(u, x.clamp(0, 255).to(torch.uint8))
        torch.manual_seed(12)
        cool = twin.sample_uint8(4, temperature=0.7)
        torch.manual_seed(12)
        assert torch.equal(cool, twin.sample(4, temperature=0.7)[0].clamp(0, 255).to(torch.uint8))
    twin.fuse_image_boundary = False
    bare = model64(preprocess=False)
    assert bare.image_boundary_constants() is None
    with pytest.raises(ValueError, match="image boundary"):
        bare.sample_uint8(2)


def test_the_matcher_and_its_misses():
    """Exactly [Dequantization, Normalization (buffers)+, LogitTransform, (Squeeze)] at the head; anything else is a miss."""
    from fincflow_amd import glow
    from fincflow_amd.layers import _image_boundary_layers
    D, N, L, S = glow.Dequantization, glow.Normalization, glow.LogitTransform, glow.Squeeze
    one, two = N(0, 256), N(-1e-6, 1.0)
    found = _image_boundary_layers([D(), one, two, L(), S(), S()])
    assert found[0] == [one, two] and found[1:] == (5, True)
    assert _image_boundary_layers([D(), one, L(), glow.ActNorm(3)])[1:] == (3, False)
    assert _image_boundary_layers([D(), one, L()])[1:] == (3, False)
    for miss in ([D(), L(), S()], [one, two, L(), S()], [D(), one, S(), L()], [D(), one, glow.ActNorm(3), L(), S()],
                 [D(), one, N(0, 2.0, learnable=True), L(), S()], [D(), N(0, 256, learnable=True), L()], [D(), one], []):
        assert _image_boundary_layers(miss) is None, miss

    class Other(glow.LogitTransform):
        pass
    assert _image_boundary_layers([D(), one, Other(), S()]) is None           # a subclass may compute something else


def test_a_miss_falls_back_to_the_layers(monkeypatch):
    """With the flag on: a learnable Normalization, a layer in between and an input that requires grad never reach the kernels (which
    would raise on these CPU tensors: there is no CPU path)."""
    from fincflow_amd import FlowSequential, glow, ops
    calls = []
    monkeypatch.setattr(ops, "finc_image_encode", lambda *a, **k: calls.append("encode"))
    monkeypatch.setattr(ops, "finc_image_decode", lambda *a, **k: calls.append("decode"))
    base = glow.GaussianPrior((12, 4, 4))
    x = torch.randint(0, 256, (2, 3, 8, 8)).float()
    stacks = {
        "learnable": [glow.Dequantization(), glow.Normalization(0, 256, learnable=True), glow.LogitTransform(), glow.Squeeze()],
        "between": [glow.Dequantization(), glow.Normalization(0, 256), glow.Squeeze(), glow.Normalization(-1e-6, 1.0),
                    glow.LogitTransform()],
        "plain": [glow.Dequantization(), glow.Normalization(0, 256), glow.Normalization(-1e-6, 1.0), glow.LogitTransform(), glow.Squeeze()],
    }
    for name, layers in stacks.items():
        outs = []
        for flag in (False, True):
            model = FlowSequential(base, *layers)
            model.fuse_image_boundary = flag
            torch.manual_seed(2)
            z, lp = model(x.clone().requires_grad_(name == "plain"))
            torch.manual_seed(2)
            back = model.sample(2)[0]
            outs.append((z, lp, back))
        for a, b in zip(*outs):
            assert torch.equal(a, b), name
    assert calls == []
