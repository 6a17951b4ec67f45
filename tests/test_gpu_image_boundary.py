"""The image boundary on the GPU (fincflow_amd/csrc/finc_image.h): `ops.finc_image_encode` / `ops.finc_image_decode`
against float64 on the CPU from the same uint8 pixels and the same fp32 noise, and `FlowSequential.fuse_image_boundary` against the
float64 twin of the model (tests/flow_twin.py).  The bar is TOL = 1e-5 in `helpers.rel_err` for elements and log-dets alike, CHAIN_TOL
for round trips through the model; every case appends what it reached to the parity report (kind `image_boundary`).

Kernel shapes (B, C, H, W), with the launch recomputed here from cpl_parts (finc_coupling.h; CPL_THREADS and CPL_CHIP_WGS read from that
file) and the item definitions of finc_image.h; `reaches` asserts them in front of the kernel:
  (2, 1, 2, 2)          squeeze, dword form, 1 item
  (3, 3, 6, 10)         squeeze, dword, 45 items, odd H/2 and W/2
  (2, 1, 28, 28)        squeeze, dword, 196 items (W % 8 = 4)
  (2, 3, 8, 16)         squeeze, 16-byte form, 24 items
  (2, 3, 32, 32)        squeeze, 16-byte, 192 items, P = 1
  (2, 3, 64, 64)        squeeze, 16-byte, 768 items, P = 3
  (1024, 3, 64, 64)     squeeze, 16-byte, 768 items per image, P = 2: a second trip of the thread loop
  (2, 3, 8, 16) view    one element into its allocation: dword, 96 items
  (2, 3, 5, 7)          no squeeze, <1>, 105 items
  (2, 3, 8, 8)          no squeeze, <4>, 96 items"""
import math
import os
import re

import numpy as np
import pytest
import torch

import flow_twin
from flow_twin import compare, recorded_masks, recorded_noise, replayed_masks, replayed_noise
from helpers import REPO, guarded, guards_intact, isolation_check, nan_filled, offset_view, rel_err, report, same_bits
from test_gpu_inverse_backward import CHAIN_TOL

pytestmark = pytest.mark.gpu

TOL = 1e-5
# the reference model's boundary, as create_model stores it: Normalization(0, 256), Normalization(-alpha, 1 / (1 - 2 alpha)) in fp32
T1, S1 = 0.0, 256.0
T2, S2 = float(np.float32(-1e-6)), float(np.float32(1 / (1 - 2e-6)))
MULT = 1.0 / (S1 * S2)
LO = -T1 / (S1 * S2) - T2 / S2
K = dict(mult=MULT, lo=LO, hi=S1, hi_comp=1.0 - LO - MULT * S1)
KD = dict(inv_mult=S1 * S2, off=T2 * S1 + T1, hi=S1)
SUM_LOG = math.log(S1) + math.log(S2)
MODEL = dict(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 16, 16), coupling_width=16)

SQ1, SQ4, FLAT1, FLAT4 = "squeeze/dword", "squeeze/16-byte", "flat/<1>", "flat/<4>"
# (shape, squeeze, offset view) -> (form, items per image, parts per image, trips of the thread loop)
FORMS = {
    ((2, 1, 2, 2), True, False): (SQ1, 1, 1, 1),
    ((3, 3, 6, 10), True, False): (SQ1, 45, 1, 1),
    ((2, 1, 28, 28), True, False): (SQ1, 196, 1, 1),
    ((2, 3, 8, 16), True, False): (SQ4, 24, 1, 1),
    ((2, 3, 32, 32), True, False): (SQ4, 192, 1, 1),
    ((2, 3, 64, 64), True, False): (SQ4, 768, 3, 1),
    ((1024, 3, 64, 64), True, False): (SQ4, 768, 2, 2),
    ((2, 3, 8, 16), True, True): (SQ1, 96, 1, 1),
    ((2, 3, 5, 7), False, False): (FLAT1, 105, 1, 1),
    ((2, 3, 8, 8), False, False): (FLAT4, 48, 1, 1),
}
BIG = ((1024, 3, 64, 64), True, False)
SMALL = [k for k in FORMS if k != BIG]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def launch_constants():
    text = open(os.path.join(REPO, "fincflow_amd", "csrc", "finc_coupling.h")).read()
    threads = int(re.search(r"constexpr int CPL_THREADS = (\d+);", text).group(1))
    wgs = re.search(r"constexpr long long CPL_CHIP_WGS = (\d+) \* (\d+);", text)
    return threads, int(wgs.group(1)) * int(wgs.group(2))


def launch_form(shape, squeeze, aligned16, u8_aligned=True):
    """finc_image.h's img_plan and cpl_parts, restated: (form, items, P, trips)."""
    B, C, H, W = shape
    threads, chip = launch_constants()
    if squeeze:
        wide = W % 8 == 0 and aligned16 and u8_aligned
        form, items = (SQ4, C * (H // 2) * (W // 8)) if wide else (SQ1, C * (H // 2) * (W // 2))
    else:
        wide = (H * W) % 4 == 0 and aligned16 and u8_aligned
        form, items = (FLAT4, C * H * W // 4) if wide else (FLAT1, C * H * W)
    P = max(1, min(-(-items // threads), -(-chip // B)))
    return form, items, P, -(-items // (P * threads))


def reaches(key, *tensors):
    """The case takes the form the table says, judged on the tensors the kernel is handed."""
    shape, squeeze, off = key
    aligned16 = all(t.data_ptr() % 16 == 0 for t in tensors if t.dtype == torch.float32)
    u8_ok = all(t.data_ptr() % 8 == 0 for t in tensors if t.dtype == torch.uint8)
    assert aligned16 == (not off), (key, [t.data_ptr() % 16 for t in tensors])
    assert launch_form(shape, squeeze, aligned16, u8_ok) == FORMS[key], (key, launch_form(shape, squeeze, aligned16, u8_ok))
    if off:
        assert launch_form(shape, squeeze, True)[0] in (SQ4, FLAT4)             # (aligned, it would be the 16-byte form)


def test_the_table_reaches_every_form_two_parts_and_a_second_trip():
    forms = [v[0] for v in FORMS.values()]
    assert set(forms) == {SQ1, SQ4, FLAT1, FLAT4}
    assert any(v[2] >= 2 for v in FORMS.values()) and any(v[3] >= 2 for v in FORMS.values())
    for (shape, squeeze, off), want in FORMS.items():
        assert launch_form(shape, squeeze, not off) == want, (shape, squeeze, off)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def squeeze64(x):
    b, c, h, w = x.shape
    return x.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(b, c * 4, h // 2, w // 2)


def unsqueeze64(x):
    b, c, h, w = x.shape
    return x.reshape(b, c // 4, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(b, c // 4, h * 2, w * 2)


def encode_ref(pixels, noise, squeeze):
    """The layers' formulas in float64 from the uint8 pixels and the fp32 noise, both converted exactly: (out, logdet)."""
    v = pixels.cpu().double() + (0.0 if noise is None else noise.cpu().double())
    y = ((v - T1) / S1 - T2) / S2
    la, lb = torch.log(y), torch.log1p(-y)
    out = la - lb
    logdet = -(la + lb).flatten(1).sum(1) - v[0].numel() * SUM_LOG
    return (squeeze64(out) if squeeze else out), logdet


def decode_ref(z, unsqueeze):
    """(v in front of the floor, the forward log-det at sigmoid(z)) in float64 from the fp32 z."""
    z = z.cpu().double()
    v = torch.sigmoid(z) * KD["inv_mult"] + KD["off"]
    logdet = (z.abs() + 2.0 * torch.log1p(torch.exp(-z.abs()))).flatten(1).sum(1) - z[0].numel() * SUM_LOG
    return (unsqueeze64(v) if unsqueeze else v), logdet


def case_inputs(key, dev, seed=0, edge_noise=False):
    """uint8 pixels over all levels and fp32 noise on the device; an offset view where the case asks for one."""
    shape, squeeze, off = key
    gen = torch.Generator().manual_seed(seed + sum(shape))
    pixels = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    noise = torch.rand(shape, generator=gen)
    if edge_noise:
        noise = 0.05 + 0.9 * noise
    noise_d = offset_view(noise, dev) if off else noise.to(dev)
    return pixels.to(dev), noise_d


def encode(img, noise, squeeze, out=None):
    from fincflow_amd import ops
    return ops.finc_image_encode(img, noise, logdet_const=-img[0].numel() * SUM_LOG, squeeze=squeeze, out=out, **K)


def decode(z, unsqueeze, dtype=torch.float32, logdet=False, out=None):
    from fincflow_amd import ops
    return ops.finc_image_decode(z, logdet_const=-z[0].numel() * SUM_LOG if logdet else None, unsqueeze=unsqueeze, dtype=dtype, out=out, **KD)


def judge(case, got, want, **fields):
    err = rel_err(got.cpu().numpy(), want.numpy())
    print("image_boundary %s %s: %.3e (bar %.0e)" % (case, fields, err, TOL))
    report("image_boundary", case=case, err=err, bar=TOL, **fields)
    return err


# ---------------------------------------------------------------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_grey_level_at_the_edge_noises(dev):
    """The test that matters: levels 0..255 x noises {0, 2^-24, 0.5, 1 - 2^-24} and twenty random ones, uint8 and fp32 pixels,
    within TOL of float64 -- and the layers' own lines on the same inputs are NOT (their error is on record beside it)."""
    from fincflow_amd import glow
    gen = torch.Generator().manual_seed(1)
    levels = torch.arange(256, dtype=torch.uint8).repeat_interleave(24)
    edge = torch.tensor([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24])
    noise = torch.cat([edge.repeat(256, 1), torch.rand(256, 20, generator=gen)], 1).reshape(-1)
    perm = torch.randperm(levels.numel(), generator=gen)
    pixels, noise = levels[perm].reshape(2, 3, 32, 32).to(dev), noise[perm].reshape(2, 3, 32, 32).to(dev)
    assert float(noise.max()) < 1.0 and int(pixels.max()) == 255 and int(pixels.min()) == 0
    want, want_ld = encode_ref(pixels, noise, True)
    reaches(((2, 3, 32, 32), True, False), pixels, noise)
    outs = []
    for img in (pixels, pixels.float()):
        got, ld = encode(img, noise, True)
        torch.cuda.synchronize()
        tag = "u8" if img.dtype == torch.uint8 else "f32"
        e, el = judge("edge/elements", got, want, pixel=tag), judge("edge/logdet", ld, want_ld, pixel=tag)
        worst = float((got.cpu().double() - want).abs().max())
        print("worst absolute element error %.3e" % worst)
        assert e <= TOL and el <= TOL, (tag, e, el)
        outs.append((got, ld))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    # the layers, flag off, on the same inputs (the noise handed over in the place of Dequantization's draw)
    with torch.no_grad():
        x, total = pixels.float() + noise, 0
        for layer in (glow.Normalization(0, 256).to(dev), glow.Normalization(-1e-6, 1 / (1 - 2e-6)).to(dev), glow.LogitTransform(), glow.Squeeze()):
            x, ld = layer(x)
            total = total + ld
    le, ll = judge("edge/elements", x, want, pixel="layers"), judge("edge/logdet", total, want_ld, pixel="layers")
    print("the PyTorch lines on the same inputs: elements %.3e, log-det %.3e" % (le, ll))
    assert le > TOL, "the layers' lines were expected to miss the bar at saturated pixels"


@pytest.mark.parametrize("key", SMALL, ids=lambda k: "%s-sq%d-off%d" % ("x".join(map(str, k[0])), k[1], k[2]))
def test_encode_against_float64_with_guards_and_repeatable_bits(key, dev):
    shape, squeeze, off = key
    pixels, noise = case_inputs(key, dev)
    want, want_ld = encode_ref(pixels, noise, squeeze)
    results = []
    for u8 in (True, False):
        if u8:
            img = pixels
        else:
            img = offset_view(pixels.float().cpu(), dev) if off else pixels.float()
        out, buf = guarded(torch.zeros(want.shape), dev, lead_floats=1 if off else 0)
        reaches(key, img, noise, out)
        got, ld = encode(img, noise, squeeze, out=out)
        torch.cuda.synchronize()
        assert got is out and guards_intact(buf, out)
        tag = "u8" if u8 else "f32"
        e, el = judge("encode/elements", got, want, shape=shape, squeeze=squeeze, offset=off, pixel=tag), \
            judge("encode/logdet", ld, want_ld, shape=shape, squeeze=squeeze, offset=off, pixel=tag)
        assert e <= TOL and el <= TOL, (key, tag, e, el)
        again, ld2 = encode(img, noise, squeeze)
        assert same_bits(again, got) and same_bits(ld2, ld)                   # a second launch, other output memory: the same bits
        results.append((got.clone(), ld))
    assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1])     # uint8 and fp32 pixels: the same bits
    zero, zld = encode(pixels, torch.zeros_like(noise), squeeze)
    none, nld = encode(pixels, None, squeeze)
    assert same_bits(zero, none) and same_bits(zld, nld)                      # no noise is zero noise


def test_encode_at_a_thousand_images_takes_a_second_trip(dev):
    pixels, noise = case_inputs(BIG, dev, edge_noise=True)
    reaches(BIG, pixels, noise)
    got, ld = encode(pixels, noise, True)
    got32, ld32 = encode(pixels.float(), noise, True)
    assert same_bits(got, got32) and same_bits(ld, ld32)
    pick = [0, 1, 511, 1023]                                                  # the reference for the first, the last and two inner images
    want, want_ld = encode_ref(pixels[pick], noise[pick], True)
    e, el = judge("encode/elements", got[pick], want, shape=BIG[0], images=pick), judge("encode/logdet", ld[pick], want_ld, shape=BIG[0], images=pick)
    assert e <= TOL and el <= TOL
    back = decode(got, True)
    back8 = decode(got, True, torch.uint8)
    assert torch.equal(back, pixels.float()) and torch.equal(back8, pixels)   # every image of the batch, exactly


def test_fp32_pixels_may_be_encoded_in_place_without_squeeze(dev):
    key = ((2, 3, 8, 8), False, False)
    pixels, noise = case_inputs(key, dev)
    want, _ = encode(pixels, noise, False)
    img = pixels.float()
    got, _ = encode(img, noise, False, out=img)
    assert got is img and same_bits(got, want)
    with pytest.raises(ValueError):
        encode(img, noise, True, out=img.view(2, 12, 4, 4))


def test_a_poisoned_neighbour_image_reaches_no_other(dev):
    for key in (((3, 3, 6, 10), True, False), ((2, 3, 64, 64), True, False), ((2, 3, 5, 7), False, False)):
        pixels, noise = case_inputs(key, dev)
        clean, clean_ld = encode(pixels, noise, key[1])
        dirty_noise = noise.clone()
        dirty_noise[0] = float("nan")
        dirty, dirty_ld = encode(pixels, dirty_noise, key[1])
        reach = torch.zeros_like(clean, dtype=torch.bool)
        reach[0] = True
        assert isolation_check(clean, dirty, reach) == (0, True), key
        assert isolation_check(clean_ld, dirty_ld, reach[:, 0, 0, 0]) == (0, True), key
        z = clean.clone()
        z[0] = float("nan")
        back, back_ld = decode(z, key[1], logdet=True)
        good, good_ld = decode(clean, key[1], logdet=True)
        mask = torch.zeros_like(good, dtype=torch.bool)
        mask[0] = True
        assert isolation_check(good, back, mask) == (0, True), key
        assert isolation_check(good_ld, back_ld, mask[:, 0, 0, 0]) == (0, True), key


# ---------------------------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------------------------
def decode_inputs(shape, squeeze, gen):
    """z = float32(logit(mult (k + f) + lo)) computed in float64, k over all of 0..255, f ~ U[0.05, 0.95]: rounding z to fp32 moves v
    by at most about 3e-6 (|z| y (1 - y) <= 0.23 times 2^-24 times 256 / ...), so the float64 decode of the same z sits >= 0.05 - 3e-6
    from any integer and the floor must be k for EVERY element."""
    n = int(np.prod(shape))
    k = torch.arange(256).repeat(-(-n // 256))[:n][torch.randperm(n, generator=gen)].reshape(shape).double()
    f = 0.05 + 0.9 * torch.rand(shape, generator=gen, dtype=torch.float64)
    y = MULT * (k + f) + LO
    z = (torch.log(y) - torch.log1p(-y)).float()
    return k, (squeeze64(z) if squeeze else z)


@pytest.mark.parametrize("key", SMALL, ids=lambda k: "%s-sq%d-off%d" % ("x".join(map(str, k[0])), k[1], k[2]))
def test_decode_floors_to_the_level_for_every_element(key, dev):
    shape, squeeze, off = key
    k, z = decode_inputs(shape, squeeze, torch.Generator().manual_seed(2 + sum(shape)))
    z_d = offset_view(z, dev) if off else z.to(dev)
    v64, want_ld = decode_ref(z_d, squeeze)
    gap = float((v64 - v64.round()).abs().min())
    assert gap >= 0.0499 and torch.equal(v64.floor(), k), gap                 # the reference itself: no element near an integer
    out, buf = guarded(torch.zeros(shape), dev, lead_floats=1 if off else 0)
    reaches(key, z_d, out)
    got, ld = decode(z_d, squeeze, logdet=True, out=out)
    torch.cuda.synchronize()
    assert got is out and guards_intact(buf, out)
    assert torch.equal(got.cpu().double(), k)                                 # every element, no exclusions
    el = judge("decode/logdet", ld, want_ld, shape=shape, squeeze=squeeze, offset=off)
    assert el <= TOL
    plain = decode(z_d, squeeze)
    assert same_bits(plain, got)                                              # with or without the log-det, launch after launch
    # the uint8 output inside byte guards, its payload on 8 bytes (the wide form may take it) and on 1 byte (it may not)
    for lead in (0, 1):
        g = 4096
        raw = torch.full((2 * g + k.numel() + 8,), 0xA5, dtype=torch.uint8, device=dev)
        start = g + (-raw.data_ptr() - g) % 8 + lead
        view = raw[start:start + k.numel()].view(shape)
        assert view.data_ptr() % 8 == lead
        got8 = decode(z_d, squeeze, torch.uint8, out=view)
        torch.cuda.synchronize()
        assert got8 is view and torch.equal(got8.cpu().double(), k)
        assert bool((raw[:start] == 0xA5).all()) and bool((raw[start + k.numel():] == 0xA5).all())
        assert torch.equal(got8, got.to(torch.uint8))                         # the uint8 output is the fp32 output cast


def test_the_clamp_at_the_ends(dev):
    """z = +-40: sigmoid saturates; the fp32 output is what the layers give (256 and -1: Dequantization.reverse does not clamp), the
    uint8 output is clamped to 255 and 0."""
    from fincflow_amd import glow
    z = torch.full((2, 12, 4, 8), 40.0, device=dev)
    z[1] = -40.0
    with torch.no_grad():
        x = glow.Squeeze().reverse(z)
        for layer in (glow.LogitTransform(), glow.Normalization(-1e-6, 1 / (1 - 2e-6)).to(dev), glow.Normalization(0, 256).to(dev),
                      glow.Dequantization()):
            x = layer.reverse(x)
    got, got8 = decode(z, True), decode(z, True, torch.uint8)
    assert torch.equal(got, x) and float(got[0, 0, 0, 0]) == 256.0 and float(got[1, 0, 0, 0]) == -1.0
    assert bool((got8[0] == 255).all()) and bool((got8[1] == 0).all())
    flat8 = decode(z, False, torch.uint8)
    assert flat8.shape == z.shape and bool((flat8[0] == 255).all()) and bool((flat8[1] == 0).all())


@pytest.mark.parametrize("key", SMALL, ids=lambda k: "%s-sq%d-off%d" % ("x".join(map(str, k[0])), k[1], k[2]))
def test_decode_of_encode_is_the_image(key, dev):
    """The un-squeeze against the squeeze: exact for noise in [0.05, 0.95]."""
    pixels, noise = case_inputs(key, dev, seed=9, edge_noise=True)
    y, ld = encode(pixels, noise, key[1])
    back, ld_back = decode(y, key[1], logdet=True)
    assert torch.equal(back, pixels.float()) and torch.equal(decode(y, key[1], torch.uint8), pixels)
    e = judge("round_trip/logdet", ld_back, ld.cpu().double(), shape=key[0], squeeze=key[1])
    assert e <= TOL                                                           # the two directions report the same log-det


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def make_model(dev, seed=0, **changes):
    from fincflow_amd import glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = flow_twin.randomise(glow.create_model(**dict(MODEL, **changes)), seed=seed + 1, actnorm=True).to(dev)
    return model


@pytest.fixture(scope="module")
def models(dev):
    """(the model with the flag on, its flag-off sibling on the same parameters, the float64 twin, uint8 pixels over all levels)."""
    from fincflow_amd import FlowSequential
    model = make_model(dev)
    model.fuse_image_boundary = True
    plain = FlowSequential(model.base_distribution, *list(model))
    assert plain.fuse_image_boundary is False
    twin = flow_twin.twin_of(plain)
    gen = torch.Generator().manual_seed(3)
    pixels = torch.arange(256, dtype=torch.uint8).repeat(12)[torch.randperm(3072, generator=gen)].reshape(4, 3, 16, 16)
    return model, plain, twin, pixels.to(dev)


class replayed_dequantisation:
    """Inside the context the Dequantization layer of `model` adds `noise` (converted exactly) instead of drawing."""

    def __init__(self, model, noise):
        self.layer, self.noise = list(model)[0], noise

    def __enter__(self):
        def forward(input, context=None):
            u = self.noise.to(device=input.device, dtype=torch.float64 if input.dtype == torch.float64 else torch.float32)
            return input + u, input.new_zeros(len(input))
        self.layer.forward = forward

    def __exit__(self, *exc):
        del self.layer.forward


def drawn_noise(seed, shape, dev):
    """What the first `torch.rand` on the device gives after `torch.manual_seed(seed)`: the boundary's draw."""
    torch.manual_seed(seed)
    return torch.rand(shape, dtype=torch.float32, device=dev)


def test_forward_encode_log_prob_and_bits_per_dim_against_the_twin(models, dev):
    model, plain, twin, pixels = models
    noise = drawn_noise(21, pixels.shape, dev)
    x64 = pixels.cpu().double()
    with torch.no_grad():
        torch.manual_seed(21)
        z, lp = model(pixels)
        torch.manual_seed(21)
        zs, lp_e = model.encode(pixels)
        torch.manual_seed(21)
        lp_l = model.log_prob(pixels.float())                                # fp32 pixels: the other entry point, the same bits
        torch.manual_seed(21)
        bpd = model.bits_per_dim(pixels)
        with replayed_dequantisation(twin, noise):
            z_w, lp_w = twin(x64)
            zs_w, _ = twin.encode(x64)
            bpd_w = twin.bits_per_dim(x64)
        with replayed_dequantisation(plain, noise):
            z_p, lp_p = plain(pixels.float())
    assert same_bits(lp, lp_e) and same_bits(lp, lp_l) and same_bits(z, zs[-1])
    compare("model/forward", ["z", "log_prob"], [z, lp], [z_w, lp_w], bar=TOL, kind="image_boundary")
    compare("model/encode", ["z%d" % i for i in range(len(zs))], zs, zs_w, bar=TOL, kind="image_boundary")
    compare("model/bits_per_dim", ["bits_per_dim"], [bpd], [bpd_w], bar=TOL, kind="image_boundary")
    layered = compare("model/forward_layers_flag_off", ["z", "log_prob"], [z_p, lp_p], [z_w, lp_w], kind="image_boundary")
    print("the flag-off model on the same pixels and noise: %s" % layered)


def test_a_training_step_against_the_twin(models, dev):
    model, plain, twin, pixels = models
    noise = drawn_noise(22, pixels.shape, dev)
    flow_twin.sync(twin, plain)
    model.zero_grad(set_to_none=True)
    with recorded_masks(model) as masks:
        torch.manual_seed(22)
        loss = model.bits_per_dim(pixels).mean()
        loss.backward()
    with replayed_dequantisation(twin, noise), replayed_masks(twin, masks):
        want = twin.bits_per_dim(pixels.cpu().double()).mean()
        want.backward()
    flow_twin.mask_unit_grads(twin)
    g, w = {n: p.grad for n, p in model.named_parameters()}, {n: p.grad for n, p in twin.named_parameters()}
    names = [n for n in g if g[n] is not None]
    assert names and names == [n for n in w if w[n] is not None]
    compare("model/train_step/loss", ["loss"], [loss], [want], bar=TOL, kind="image_boundary")
    compare("model/train_step/grads", names, [g[n] for n in names], [w[n] for n in names], bar=TOL, kind="image_boundary")
    model.zero_grad(set_to_none=True)


def test_samplers_against_the_flag_off_model_and_the_twin(models, dev, monkeypatch):
    """From one seed: in front of the floor the flag-on model, the flag-off model and the twin agree to CHAIN_TOL; behind it the two
    models agree wherever the twin's value is at least 1e-3 from an integer (the share left out is printed and under 1 %)."""
    from fincflow_amd import FlowSequential, ops
    model, plain, twin, _ = models
    flow_twin.sync(twin, plain)
    inner = FlowSequential(plain.base_distribution, *list(plain)[1:])            # the flag-off model without the floor
    twin_inner = FlowSequential(twin.base_distribution, *list(twin)[1:])
    twin_inner.fuse_affine = False
    seen = []
    real = ops.finc_image_decode
    monkeypatch.setattr(ops, "finc_image_decode", lambda z, **kw: (seen.append(z.clone()), real(z, **kw))[1])
    n = 16
    for name in ("sample", "decode", "sample_with_log_prob"):
        def run(m):
            if name == "sample":
                return [m.sample(n)[0]]
            if name == "decode":
                return [m.decode(m.draw_latents(n))]
            return list(m.sample_with_log_prob(n))
        del seen[:]
        with torch.no_grad():
            torch.manual_seed(31)
            with recorded_noise(model) as draws:
                on = run(model)
            torch.manual_seed(31)
            off = run(plain)
            torch.manual_seed(31)
            pre_off = run(inner)
            with replayed_noise(twin_inner, draws):
                pre_twin = run(twin_inner)
        assert len(seen) == 1
        pre_on = decode_ref(seen[0], True)[0]
        compare("model/%s/pre_floor" % name, ["fused", "layers"], [pre_on, pre_off[0]], [pre_twin[0], pre_twin[0]], bar=CHAIN_TOL,
                kind="image_boundary")
        safe = (pre_twin[0] - pre_twin[0].round()).abs() >= 1e-3
        left_out = 1.0 - float(safe.double().mean())
        print("model/%s: %.4f %% of the elements lie within 1e-3 of an integer and are left out" % (name, 100 * left_out))
        report("image_boundary", case="model/%s/left_out" % name, share=left_out)
        assert left_out < 0.01
        assert on[0].dtype == torch.float32 and torch.equal(on[0].cpu()[safe], off[0].cpu()[safe])
        if name == "sample_with_log_prob":
            compare("model/sample_with_log_prob/log_q", ["fused", "layers"], [on[1], off[1]], [pre_twin[1], pre_twin[1]], bar=CHAIN_TOL,
                    kind="image_boundary")


def test_sample_uint8_is_the_clamp_of_sample(models, dev):
    model, plain, _, _ = models
    for m in (model, plain):
        torch.manual_seed(41)
        u = m.sample_uint8(8)
        torch.manual_seed(41)
        with torch.no_grad():
            x = m.sample(8)[0]
        assert u.dtype == torch.uint8 and u.shape == (8, 3, 16, 16) and torch.equal(u, x.clamp(0, 255).to(torch.uint8))
        torch.manual_seed(41)
        cool = m.sample_uint8(8, temperature=0.7)
        torch.manual_seed(41)
        with torch.no_grad():
            assert torch.equal(cool, m.sample(8, temperature=0.7)[0].clamp(0, 255).to(torch.uint8))


def test_a_captured_sample_replays_with_the_bits_of_the_eager_call(dev, monkeypatch):
    from fincflow_amd import _lib
    from test_gpu_sample_logdet import fix_latents
    model = make_model(dev, seed=5)
    model.fuse_image_boundary = True
    fix_latents(model, 4, monkeypatch)
    with torch.no_grad():
        x0, _ = model.sample(4)                                              # eager first: the constants' cache, the banks, the workspace
        u0 = model.sample_uint8(4)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                                            # one stream, no parallel branches
            x, _ = model.sample(4)
            u = model.sample_uint8(4)
    for _ in range(2):
        x.zero_(), u.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(x, x0) and torch.equal(u, u0)
    assert not _lib.fault_pending()


class Counter:
    """Counts the calls of `ops` entry points and of Squeeze.forward (the pattern of tests/test_gpu_train_loop.py)."""
    OPS = ("finc_image_encode", "finc_image_decode")

    def __init__(self, monkeypatch):
        from fincflow_amd import glow, ops
        self.n = {}
        for name in self.OPS:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        monkeypatch.setattr(glow.Squeeze, "forward", self._wrap("Squeeze.forward", glow.Squeeze.forward))
        monkeypatch.setattr(glow.Squeeze, "reverse", self._wrap("Squeeze.reverse", glow.Squeeze.reverse))

    def _wrap(self, name, fn):
        def counted(*args, **kwargs):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*args, **kwargs)
        return counted

    def take(self):
        n, self.n = self.n, {}
        return n


def test_prefix_and_tail_are_one_launch_each(models, dev, monkeypatch):
    """Two blocks, so two Squeeze layers: with the flag on the first is the encode's / the decode's, the second stays a layer."""
    model, plain, _, pixels = models
    counter = Counter(monkeypatch)
    with torch.no_grad():
        model.log_prob(pixels)
        assert counter.take() == {"finc_image_encode": 1, "Squeeze.forward": 1}
        model.encode(pixels.float())
        assert counter.take() == {"finc_image_encode": 1, "Squeeze.forward": 1}
        for call in (lambda: model.sample(4), lambda: model.sample_with_log_prob(4), lambda: model.decode(model.draw_latents(4)),
                     lambda: model.sample_uint8(4), lambda: model.reconstruct(pixels)):
            call()
            k = counter.take()
            assert k.get("finc_image_decode") == 1 and k.get("Squeeze.reverse") == 1, k
        model.sample(4, also_true_inverse=True)                               # the layer-by-layer check keeps the layers
        k = counter.take()
        assert k.get("finc_image_decode") == 1 and k.get("Squeeze.reverse") == 3, k
        plain.log_prob(pixels.float())
        plain.sample(4)
        assert counter.take() == {"Squeeze.forward": 2, "Squeeze.reverse": 2}
    model.invertible_backward = True
    try:
        model.log_prob(pixels).sum().backward()                              # the invertible runs: the first Squeeze has left its run
        k = counter.take()
        assert k.get("finc_image_encode") == 1 and k.get("finc_image_decode") is None, k
    finally:
        del model.invertible_backward
        model.zero_grad(set_to_none=True)
    # while autograd records the reverse chain the layers keep their lines
    x = model.rsample(2)
    assert x.requires_grad and counter.take().get("finc_image_decode") is None


def test_misses_on_the_device_fall_back_to_the_layers(dev, monkeypatch):
    """A learnable Normalization, an input that requires grad and fp64 pixels take the layers exactly as with the flag off."""
    from fincflow_amd import FlowSequential, glow
    counter = Counter(monkeypatch)
    base = glow.GaussianPrior((12, 4, 4)).to(dev)
    x = torch.randint(0, 256, (2, 3, 8, 8), device=dev).float()
    for name, norm in (("learnable", glow.Normalization(0, 256, learnable=True)), ("grad", glow.Normalization(0, 256)),
                       ("fp64", glow.Normalization(0, 256))):
        outs = []
        for flag in (False, True):
            m = FlowSequential(base, glow.Dequantization(), norm, glow.Normalization(-1e-6, 1 / (1 - 2e-6)), glow.LogitTransform(),
                               glow.Squeeze()).to(dev)
            if name == "fp64":
                m = m.double()
            m.fuse_image_boundary = flag
            inp = x.double() if name == "fp64" else x.clone().requires_grad_(name == "grad")
            torch.manual_seed(2)
            z, lp = m(inp)
            outs.append((z.detach(), lp.detach()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), name
    assert "finc_image_encode" not in counter.take()


def test_the_flag_off_model_runs_the_layers_by_hand(models, dev):
    """Flag untouched: `forward` and `sample` are the layered calls, bit for bit."""
    _, plain, _, pixels = models
    assert "fuse_image_boundary" not in plain.__dict__
    x = pixels.float()
    with torch.no_grad():
        torch.manual_seed(51)
        plain.fuse_affine = False                                            # (the unit + ActNorm fold is another launch: layer by layer here)
        try:
            z, lp = plain(x)
        finally:
            del plain.fuse_affine
        torch.manual_seed(51)
        h, total = x, 0
        for layer in plain:
            h, ld = layer(h)
            total = total + ld
        assert same_bits(z, h) and same_bits(lp, plain.base_distribution.log_prob(h) + total)
        torch.manual_seed(52)
        s = plain._reverse_chain(plain.base_distribution.sample(4)[0], None, fuse=False)
        torch.manual_seed(52)
        h = plain.base_distribution.sample(4)[0]
        for layer in reversed(list(plain)):
            h = layer.reverse(h)
        assert same_bits(s, h)
        torch.manual_seed(52)
        folded = plain.sample(4)[0]                                          # the folds move a value across an integer now and then
        assert float((folded == h).double().mean()) > 0.99
