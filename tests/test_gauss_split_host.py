"""Host side of the Gaussianized split (include/finc.h: finc_gauss_split_f32, finc_gauss_split_merge_f32,
finc_gauss_split_backward_f32): `glow.Gaussianize` / `glow.Split` in float64 on the CPU against a fixture the
reference's own layers/split.py produced (tests/golden/gaussianize_split.npz, scripts/make_golden_gaussianize_split.py), its state
dict, encode / decode through a two-level model, the exported symbols and the ABI version gate, the refusal order of the three
entry points with fake pointers, and the new kernels' register allocation.  No GPU needed, the library built."""
import math
import os

import numpy as np
import pytest
import torch

import flow_twin
from fincflow_amd import _lib
from helpers import fake_ptr as _p, golden, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("finc_gauss_split", "finc_gauss_split_merge", "finc_gauss_split_backward")
BIG = 1 << 40
DIMS = (2, 12, 64)                        # a half tensor: 2 * 6 * 64 * 4 = 3072 bytes, the whole one 6144: the fake pointers lie 64 KiB apart


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer against the reference's fixture
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    g = golden("gaussianize_split")
    return {k: torch.from_numpy(g[k]) for k in g.files}


def _layer(fixture):
    from fincflow_amd import glow
    m = glow.Split((12, 4, 5), glow.GaussianPrior).double()
    state = {k[len("state."):]: v for k, v in fixture.items() if k.startswith("state.")}
    result = m.load_state_dict(state, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return m, state


def test_the_reference_state_dict_loads_with_no_key_left_over(fixture):
    m, state = _layer(fixture)
    assert sorted(state) == sorted(m.state_dict()) == ["gaussianize.log_scale_factor", "gaussianize.net.bias", "gaussianize.net.weight"]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "gaussianize.net.weight": (12, 6, 3, 3), "gaussianize.net.bias": (12,), "gaussianize.log_scale_factor": (12, 1, 1)}


def test_a_fresh_layer_is_the_identity_split():
    from fincflow_amd import glow
    m = glow.Split((4, 3, 3), glow.GaussianPrior)
    assert not any(bool(p.any()) for p in m.parameters())                     # zero-initialised: m = 0, logs = 0
    x = torch.randn(2, 4, 3, 3)
    with torch.no_grad():
        x1, z2, log_p = m.split(x)
    assert torch.equal(x1, x[:, :2]) and torch.equal(z2, x[:, 2:]) and torch.equal(log_p, m.base.log_prob(x[:, 2:]))


def test_the_module_in_float64_reproduces_the_reference(fixture):
    """Pins the roles of the even (mean) and odd (log-scale) output channels and the sign of the log-det."""
    m, _ = _layer(fixture)
    x = fixture["x"]
    with torch.no_grad():
        x1, z2, log_p = m.split(x)
        z2g, logdet = m.gaussianize(x[:, :6], x[:, 6:])
        back = m.merge(x1, z2)
        back2, log_q = m.merge(x1, z2, with_log_prob=True)
        first, log_p_forward = m(x)
    assert float(fixture["logdet"].abs().min()) > 1e-2                         # (not the identity layer)
    assert torch.equal(x1, fixture["x1"]) and torch.equal(first, x1)
    for got, want in ((z2, fixture["z2"]), (z2g, fixture["z2"]), (logdet, fixture["logdet"]), (back, fixture["inverse"]), (back, x),
                      (log_p - m.base.log_prob(z2), fixture["logdet"])):
        assert float((got - want).abs().max()) <= 1e-12, float((got - want).abs().max())
    assert torch.equal(back2, back) and torch.equal(log_p_forward, log_p)
    assert float((log_q - log_p).abs().max()) <= 1e-12 * float(log_p.abs().max())
    # the formula of the C header, written out: even output channels are the mean, odd ones the log-scale
    g = m.gaussianize
    with torch.no_grad():
        a, b = g._scale_shift()
        h = a.view(1, -1, 1, 1) * torch.nn.functional.conv2d(x[:, :6], g.net.weight, None, padding=1) + b.view(1, -1, 1, 1)
        z2_formula = (x[:, 6:] - h[:, 0::2]) * torch.exp(-h[:, 1::2])
        log_p_formula = -h[:, 1::2].flatten(1).sum(1) - 0.5 * z2_formula.square().flatten(1).sum(1) - 0.5 * 6 * 20 * math.log(2 * math.pi)
    assert float((z2 - z2_formula).abs().max()) <= 1e-12 and float((log_p - log_p_formula).abs().max()) <= 1e-12 * float(log_p.abs().max())


def test_reverse_draws_from_the_base_and_merge_scales_the_draw(fixture):
    m, _ = _layer(fixture)
    x1 = fixture["x1"]
    with torch.no_grad():
        torch.manual_seed(9)
        drawn = m.reverse(x1)
        torch.manual_seed(9)
        z2 = m.base.sample(2)[0]
        assert torch.equal(drawn, m.merge(x1, z2)) and torch.equal(drawn[:, :6], x1)
        torch.manual_seed(9)
        cool = m.merge(x1, temperature=0.5)
        assert torch.equal(cool, m.merge(x1, 0.5 * z2))
        torch.manual_seed(9)
        out, log_q = m.reverse_with_logdet(x1)
        assert torch.equal(out, drawn) and float((log_q - m(out)[1]).abs().max()) <= 1e-12 * float(log_q.abs().max())
    # the layer defines no `invertible_backward_supported` of its own: FlowLayer's answer, as for SplitPrior, ends an invertible run
    from fincflow_amd import glow
    assert "invertible_backward_supported" not in vars(glow.Split)
    assert glow.Split.invertible_backward_supported is glow.SplitPrior.invertible_backward_supported
    assert not m.invertible_backward_supported(fixture["x"])


def test_another_base_keeps_its_own_log_prob_and_the_cache_does_not_travel():
    import copy
    from fincflow_amd import glow

    class Wide(glow.GaussianPrior):
        def log_prob(self, input, context=None, sum=True):
            return super().log_prob(input / 2.0, context) - self.dim * math.log(2.0)
    m = glow.Split((4, 3, 3), Wide).double()
    assert not m._hip_latent(torch.zeros(1, 4, 3, 3))
    x = torch.randn(2, 4, 3, 3, dtype=torch.float64)
    with torch.no_grad():
        x1, z2, log_p = m.split(x)
        assert torch.equal(log_p, m.base.log_prob(z2) + m.gaussianize(x[:, :2], x[:, 2:])[1])
    g = glow.Gaussianize(3)
    a, b = g._scale_shift_cached()
    assert g._scale_shift_cached()[0] is a and "_ab" in g.__dict__
    twin = copy.deepcopy(g)
    assert not any(k in twin.__dict__ for k in glow.Gaussianize._derived)      # a deep copy starts empty
    with torch.no_grad():
        g.log_scale_factor.add_(1.0)
    assert g._scale_shift_cached()[0] is not a                                # a new parameter version: rebuilt


# ---------------------------------------------------------------------------------------------------------------------------------
# the model on CPU float64 tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def _randomise_splits(model, seed):
    from fincflow_amd import glow
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, glow.Gaussianize):
                for name, p in m.named_parameters():
                    p.copy_(torch.randn(p.shape, generator=gen) * (0.1 if name.endswith(("bias", "log_scale_factor")) else 0.05))


@pytest.fixture(scope="module")
def twin():
    from fincflow_amd import glow
    torch.manual_seed(1)
    np.random.seed(1)                                                         # (Conv1x1 draws its orthogonal W from numpy)
    kw = dict(num_blocks=2, block_size=1, image_size=(3, 8, 8), split_prior=True, coupling_width=16)
    model = glow.create_model(gaussianize_split=True, preprocess=False, **kw)
    kinds = [type(m).__name__ for m in model.sequence_modules]
    assert kinds.count("Split") == 1 and "SplitPrior" not in kinds
    # the default builds today's model
    assert [type(m).__name__ for m in glow.create_model(preprocess=False, **kw).sequence_modules].count("SplitPrior") == 1
    flow_twin.randomise(model, seed=1)
    _randomise_splits(model, seed=2)
    return flow_twin.twin_of(model)


def test_decode_of_encode_is_the_input_and_encode_has_the_log_prob_of_forward(twin):
    x = torch.randn(3, 3, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        zs, log_prob = twin.encode(x)
        back = twin.decode(zs)
        back_q, log_q = twin.decode(zs, with_log_prob=True)
        want = twin(x)[1]
    assert [tuple(z.shape) for z in zs] == [(3, 6, 4, 4), (3, 24, 2, 2)]
    assert sum(z[0].numel() for z in zs) == x[0].numel()                      # the code is complete
    assert float((back - x).abs().max()) <= 1e-10 and torch.equal(back_q, back)
    assert float((log_prob - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((log_q - log_prob).abs().max()) <= 1e-10 * float(log_prob.abs().max())
    with torch.no_grad():
        torch.manual_seed(5)
        a = twin.sample(2, temperature=0.7)[0]
        torch.manual_seed(5)
        b = twin.decode(twin.draw_latents(2, temperature=0.7))
    assert torch.equal(a, b)


def test_the_encode_loss_reaches_every_parameter_of_the_split(twin):
    x = torch.randn(3, 3, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    names, params = zip(*twin.named_parameters())
    got = torch.autograd.grad(-twin.encode(x)[1].mean(), params)
    want = torch.autograd.grad(-twin.log_prob(x).mean(), params)
    assert any("gaussianize" in n for n in names)
    for name, g, w in zip(names, got, want):
        assert float(w.abs().max()) > 0, name
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max()), name


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for entry, sibling in zip(ENTRIES, ("finc_split_prior", "finc_split_prior_merge", "finc_split_prior_backward")):
        name = entry + "_f32"
        assert name in _lib.SYMBOLS and name + "(" in header, name
        assert getattr(L, name).argtypes == getattr(L, sibling + "_f32").argtypes, name       # the argument lists mirror the siblings'
        assert entry + "_rawbf16_f32" not in _lib.SYMBOLS
    from fincflow_amd import ops
    for name in ENTRIES + ("gauss_split_forward",):
        assert callable(getattr(ops, name)), name


def test_version_is_116_and_a_115_library_is_told_to_rebuild(tmp_path):
    assert _lib.GAUSS_SPLIT_ABI_VERSION == 116
    assert _lib.lib().finc_version() >= _lib.GAUSS_SPLIT_ABI_VERSION
    out = load_stub_library(tmp_path, 115)
    assert "= 115" in out and "116" in out and "rebuild it" in out and "finc_gauss_split_f32" in out, out


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_transform_refusal_order(entry):
    """NULL -> 1, bad dims / an output on raw / overlapping activations -> 2, alignment (4 bytes) -> 7, a channel count without a
    kernel -> 3, workspace -> 4, in that order: the ladder of the split prior."""
    L = _lib.lib()
    merge = entry.endswith("merge")
    fn = getattr(L, entry + "_f32")
    whole, h1, h2 = _p(0x100000), _p(0x200000), _p(0x300000)
    raw, a, b, lp, ws = _p(0x400000), _p(0x500000), _p(0x510000), _p(0x520000), _p(0x600000)

    def f(whole=whole, h1=h1, h2=h2, raw=raw, a=a, b=b, lp=lp, dims=DIMS, ws=ws, nbytes=BIG):
        acts = (h1, h2, raw, a, b, whole) if merge else (whole, raw, a, b, h1, h2)
        return fn(*acts, lp, *dims, ws, nbytes, None)
    for name in ("whole", "h1", "h2", "raw", "a", "b"):
        assert f(**{name: None}) == 1, name
    if not merge:
        assert f(lp=None) == 1                                               # the split always reports log p
    else:
        assert f(lp=None, dims=(2, 13, 64), ws=None, nbytes=0) == 3          # the merge need not: past the NULL rule, down to the channels
        assert f(lp=None, dims=(2, 12, 0), ws=None, nbytes=0) == 2
    assert f(whole=None, dims=(0, 12, 64)) == 1                              # (NULL comes before the dims)
    for dims in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64)):
        assert f(dims=dims) == 2, dims
    for name in (("whole",) if merge else ("h1", "h2")):
        assert f(**{name: raw}) == 2, name                                   # an output on raw
    assert f(h2=h1) == 2 and f(h1=whole) == 2 and f(h2=whole) == 2           # x1, z2 and x may not overlap each other
    # (every call here ends in a refusal: nothing may reach a launch with these addresses)
    assert f(h2=_p(0x200000 + 3068)) == 2 and f(h2=_p(0x200000 + 3072), ws=None) == 4     # the last dword of x1 / the first one behind it
    assert f(h1=_p(0x100000 + 6140)) == 2 and f(h1=_p(0x100000 + 6144), ws=None) == 4     # the same against the whole tensor
    assert f(h1=_p(0x200002), dims=(0, 12, 64)) == 2                         # (dims come before the alignment)
    for name, base in (("whole", 0x100000), ("h1", 0x200000), ("h2", 0x300000), ("a", 0x500000), ("b", 0x510000), ("lp", 0x520000)):
        assert f(**{name: _p(base + 2)}) == 7, name                          # misaligned by 2 bytes
        assert f(**{name: _p(base + 4)}, ws=None) == 4, name                 # on 4 bytes with HW % 4 == 0: accepted (the narrow form)
    assert f(raw=_p(0x400001)) == 7 and f(raw=_p(0x400002)) == 7             # raw is fp32: held to 4 bytes
    assert f(h1=_p(0x200002), dims=(2, 13, 64)) == 7                         # (alignment comes before the channel count)
    for C in (13, 7, 1):
        assert f(dims=(2, C, 64)) == 3, C
        assert f(dims=(2, C, 64), ws=None, nbytes=0) == 3, C                 # (... before the workspace)
    need = L.finc_coupling_workspace_bytes(*DIMS)
    assert f(ws=None) == 4 and f(nbytes=need - 1) == 4 and f(nbytes=0) == 4
    assert f(ws=_p(0x600002)) == 4


def test_backward_refusal_order():
    L = _lib.lib()
    fn = L.finc_gauss_split_backward_f32
    g1, g2, gl, x, raw, a, b = _p(0x100000), _p(0x200000), _p(0x300000), _p(0x400000), _p(0x500000), _p(0x600000), _p(0x610000)
    gx, gr, ga, gb, ws = _p(0x700000), _p(0x800000), _p(0x900000), _p(0x910000), _p(0xa00000)

    def f(g1=g1, g2=g2, gl=gl, x=x, raw=raw, a=a, b=b, gx=gx, gr=gr, ga=ga, gb=gb, dims=DIMS, ws=ws, nbytes=BIG):
        return fn(g1, g2, gl, x, raw, a, b, gx, gr, ga, gb, *dims, ws, nbytes, None)
    for name in ("x", "raw", "a", "b"):
        assert f(**{name: None}) == 1, name
    assert f(g1=None, g2=None, gl=None) == 1                                 # each incoming gradient may be absent, not all three
    for absent in ("g1", "g2", "gl"):
        assert f(**{absent: None}, ws=None) == 4, absent                     # (one absent: past the NULL rule, down to the workspace)
    assert f(gx=None, gr=None, ga=None, gb=None) == 1                        # nothing asked for
    assert f(x=None, dims=(0, 12, 64)) == 1                                  # (NULL comes before the dims)
    for dims in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 1 << 20, 64)):
        assert f(dims=dims) == 2, dims
    for alias in (g1, g2, x, raw):
        assert f(gx=alias) == 2                                              # grad_x on an input
    for alias in (g1, g2, x, raw, gx):
        assert f(gr=alias) == 2                                              # grad_raw on an input or on grad_x
    assert f(g1=_p(0x100002), dims=(0, 12, 64)) == 2                         # (dims come before the alignment)
    for name, base in (("g1", 0x100000), ("g2", 0x200000), ("gl", 0x300000), ("x", 0x400000), ("gx", 0x700000), ("ga", 0x900000)):
        assert f(**{name: _p(base + 2)}) == 7, name
        assert f(**{name: _p(base + 4)}, ws=None) == 4, name                 # on 4 bytes: accepted, the next refusal is the workspace's
    assert f(raw=_p(0x500002)) == 7 and f(gr=_p(0x800002)) == 7
    assert f(g2=_p(0x200002), dims=(2, 13, 64)) == 7                         # (alignment before the channel count)
    for C in (13, 7):
        assert f(dims=(2, C, 64)) == 3
        assert f(dims=(2, C, 64), ws=None, nbytes=0) == 3                    # (... before the workspace)
    need = L.finc_coupling_workspace_bytes(*DIMS)
    assert f(nbytes=need - 1) == 4
    assert f(gx=None, gr=None, gb=None, nbytes=0) == 4 and f(gx=None, gr=None, ga=None, ws=None, nbytes=0) == 4


def test_the_new_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    # transform: V in {4, 1} x (split with log p, merge with, merge without); backward: V in {4, 1}
    want = {"finc_gauss_split_kernel": 6, "finc_gauss_split_bwd_kernel": 2, "finc_coupling_reduce_kernel": 1}
    for name, count in want.items():
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == count, (name, sorted(ks))
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)
    for old in ("finc_coupling_kernel", "finc_coupling_bwd_kernel", "finc_splitprior_kernel", "finc_splitprior_bwd_kernel",
                "finc_coupling_rawbf16_grad_kernel", "finc_coupling_reduce_kernel"):
        assert not any(old in k for k in md if "finc_gauss_split" in k), old          # the counts of the older tests stay theirs
