"""The layers around the hot path (BASELINE configs[3]) against a trace recorded from the reference's own
layers (tests/golden/make_golden_stack.py).  Host test: topology / parameter names; GPU test: numbers."""
import numpy as np
import pytest
import torch

from helpers import STACK_INPUT, STACK_SPEC, fill_stack_parameters, golden, rel_err


def build_ours():
    from fincflow_amd import FastFlowUnit
    from fincflow_amd import glow
    layers = []
    for s in STACK_SPEC:
        if s[0] == "squeeze":
            layers.append(glow.Squeeze())
        elif s[0] == "ffu":
            layers.append(FastFlowUnit(s[1], s[1], (s[2], s[2])))
        elif s[0] == "actnorm":
            layers.append(glow.ActNorm(s[1]))
        elif s[0] == "conv1x1":
            layers.append(glow.Conv1x1(s[1]))
        elif s[0] == "coupling":
            layers.append(glow.Coupling(s[1], width=s[2]))
    return layers


def test_create_model_topology():
    """fastflow_cifar.py:35-63: 4 preprocessing layers, then per block Squeeze + block_size x [unit, actnorm, 1x1,
    coupling] (+ SplitPrior between blocks); parameter names match the reference's state dict."""
    from fincflow_amd import FastFlowUnit, glow
    m = glow.create_model(num_blocks=3, block_size=2, actnorm=True, split_prior=True, coupling_width=16)
    kinds = [type(l).__name__ for l in m]
    assert kinds[:4] == ["Dequantization", "Normalization", "Normalization", "LogitTransform"]
    assert kinds.count("FastFlowUnit") == 6 and kinds.count("SplitPrior") == 2 and kinds.count("Squeeze") == 3
    units = [l for l in m if isinstance(l, FastFlowUnit)]
    assert [u.conv_tl.conv.weight.shape[0] for u in units] == [3, 3, 6, 6, 12, 12]  # Cq per level (c4)
    keys = set(m.state_dict().keys())
    assert "5.conv_tl.conv.weight" in keys and "6.log_scale" in keys and "7.W" in keys
    assert "8.net.0.weight" in keys and "8.net.4.logs" in keys
    # the preprocessing layers' share of a reference checkpoint: its UniformDistribution's buffer and the two Normalizations' (the
    # complete lists, in order, against the reference's own: tests/test_reference_model_host.py)
    assert [k for k in m.state_dict() if int(k.split(".")[0]) < 4] == ["0.distribution.empty", "1.translation", "1.scale",
                                                                      "2.translation", "2.scale"]
    assert m.base_distribution.size == (48, 4, 4)


def test_squeeze_and_elementwise_layers_host():
    from fincflow_amd import glow
    x = torch.arange(2 * 3 * 4 * 4, dtype=torch.float32).reshape(2, 3, 4, 4)
    sq = glow.Squeeze()
    y, ld = sq(x)
    assert y.shape == (2, 12, 2, 2) and torch.equal(sq.reverse(y), x) and torch.equal(ld, torch.zeros(2))
    assert torch.equal(y[0, :4, 0, 0], torch.tensor([0., 1., 4., 5.]))   # (c, dy, dx) order of layers/squeeze.py
    an = glow.ActNorm(12)
    z, _ = an(y)                                                           # data-dependent init on first call
    assert int(an.initialized) == 1 and torch.allclose(z.mean(dim=(0, 2, 3)), torch.zeros(12), atol=1e-5)
    assert torch.allclose(an.reverse(z), y, atol=1e-4)
    lt = glow.LogitTransform()
    u = torch.rand(2, 3, 4, 4) * 0.9 + 0.05
    assert torch.allclose(lt.reverse(lt(u)[0]), u, atol=1e-6)


@pytest.mark.gpu
def test_stack_matches_reference_trace():
    g = golden("stack_c4_small")
    dev = torch.device("cuda:0")
    layers = build_ours()
    fill_stack_parameters(layers, ffu_weights=g)
    layers = [l.to(dev) for l in layers]
    x = torch.from_numpy(g["x"]).to(dev)
    assert tuple(x.shape) == STACK_INPUT
    with torch.no_grad():
        h, logdet = x, 0
        for m in layers:
            h, ld = m(h, None)
            logdet = logdet + ld
        r = torch.from_numpy(g["z_in"]).to(dev)
        for m in reversed(layers):
            r = m.reverse(r, None)
            r = r[0] if isinstance(r, tuple) else r
    assert rel_err(h.cpu().numpy(), g["z"]) <= 1e-5
    assert np.allclose(logdet.cpu().numpy(), g["logdet"], rtol=1e-5, atol=1e-4)
    assert rel_err(r.cpu().numpy(), g["x_rev"]) <= 1e-5


@pytest.mark.gpu
def test_full_config4_model_samples_and_reconstructs():
    """BASELINE configs[3] topology (num_blocks=3, block_size=32, 96 units), a reduced coupling width to keep the test
    quick: density evaluation, reconstruction through all 96 inverses, and sampling of 128 images run end to end.
    A randomly initialised 96-unit stack is ill-conditioned for ANY fp32 inverse (each unit's inverse amplifies by
    ~1.7 at the init std 0.05: 1.7^32 per level), so the free taps are scaled by 0.2 here; the trace test above
    pins the numbers at the reference's own init scale."""
    from fincflow_amd import FastFlowUnit, glow
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    model = glow.create_model(num_blocks=3, block_size=32, actnorm=True, split_prior=False, preprocess=False,
                              coupling_width=32)
    with torch.no_grad():
        for m in model:
            if isinstance(m, FastFlowUnit):
                for c in (m.conv_tl, m.conv_tr, m.conv_bl, m.conv_br):
                    c.conv.weight.mul_(1 - 0.8 * c.mask)
    model = model.to(dev)
    x = torch.randn(8, 3, 32, 32, device=dev)
    with torch.no_grad():
        z, logp = model(x)                      # also runs ActNorm's data-dependent init
        assert z.shape == (8, 192, 4, 4) and logp.shape == (8,) and torch.isfinite(logp).all()
        xr = model.reconstruct(x)
        assert rel_err(xr.cpu().numpy(), x.cpu().numpy()) <= 1e-4
        s, s_true = model.sample(128)           # (input, input_true): layers/flowsequential.py:89-115
        assert s_true is s
        assert s.shape == (128, 3, 32, 32) and torch.isfinite(s).all()
        # the "true inverse" re-runs the chain from the same z layer by layer (no affine fold): same samples
        torch.manual_seed(5)
        a, a_true = model.sample(16, also_true_inverse=True)
        assert a_true is not a and rel_err(a.cpu().numpy(), a_true.cpu().numpy()) <= 1e-4


@pytest.mark.gpu
def test_config4_exactly_as_benched():
    """The topology `bench.py --workload c4` times, unchanged: create_model(num_blocks=3, block_size=32, actnorm=True,
    split_prior=True), default preprocess and coupling width, 128 samples.  A split prior draws fresh noise at every
    level, so there is no reconstruct identity here; what is checked is the sample contract, that the fused chain
    (ActNorm folded into the inverses' loads/stores) and the layer-by-layer chain produce the same images from the same
    noise (with tamed taps: see below), that every FastFlowUnit in the stack inverts its own forward at the shape it
    sees, and a density pass."""
    from fincflow_amd import FastFlowUnit, glow
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    model = glow.create_model(num_blocks=3, block_size=32, actnorm=True, split_prior=True).to(dev).eval()
    units = [m for m in model if isinstance(m, FastFlowUnit)]
    assert len(units) == 96
    with torch.no_grad():
        for m in model:
            if isinstance(m, glow.ActNorm):
                m.initialized.fill_(1)             # as bench.py does: sampling never runs the data-dependent init
        s, s_true = model.sample(128)
        assert s_true is s and s.shape == (128, 3, 32, 32) and torch.isfinite(s).all()
        torch.manual_seed(11)
        a, a_true = model.sample(128, also_true_inverse=True)
        assert a_true is not a and torch.isfinite(a_true).all() and a_true.shape == a.shape
        shapes = {}
        for u in units:                            # one unit per distinct shape: 12x16x16, 24x8x8, 48x4x4
            shapes.setdefault(u.conv_tl.conv.weight.shape[0] * 4, u)
        assert sorted(shapes) == [12, 24, 48]
        for C, u in shapes.items():
            hw = {12: 16, 24: 8, 48: 4}[C]
            x = torch.randn(128, C, hw, hw, device=dev)
            z, _ = u(x)
            xr = u.reverse(z)
            assert rel_err(xr.cpu().numpy(), x.cpu().numpy()) <= 1e-5
        z, logp = model(torch.rand(16, 3, 32, 32, device=dev))
        assert torch.isfinite(logp).all() and logp.shape == (16,)
        # Fused chain == layer-by-layer chain on this topology.  At the init scale 96 random units amplify any fp32
        # difference by ~1.7 per unit (the images saturate), so this comparison runs with the free taps scaled by 0.2, as in
        # the reconstruction test above; the topology (split priors, widths) stays the benched one.
        for u in units:
            for c in (u.conv_tl, u.conv_tr, u.conv_bl, u.conv_br):
                c.conv.weight.mul_(1 - 0.8 * torch.as_tensor(c.mask).to(c.conv.weight.device))
        z0, _ = model.base_distribution.sample(128, None)
        torch.manual_seed(11)                      # the split priors draw their noise inside the chain: same seed, same draws
        a = model._reverse_chain(z0, None, fuse=True)
        torch.manual_seed(11)
        a_true = model._reverse_chain(z0, None, fuse=False)
        # the chain ends in the dequantisation's floor (layers/dequantize.py): the two evaluations differ by fp32 rounding
        # (the folds change the summation order), which may move a value across an integer -- a handful of pixels of the
        # 393,216 differ by exactly one grey level, everything else is equal
        d = (a - a_true).abs()
        assert float(d.max()) <= 1.0 and float((d > 0).float().mean()) <= 1e-4, (float(d.max()), float((d > 0).float().mean()))
