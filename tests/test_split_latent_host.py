"""Host side of the split prior with its latent (include/finc.h: finc_split_prior_f32, finc_split_prior_merge_f32,
finc_split_prior_backward_f32 and their _rawbf16_f32 siblings): the exported symbols and the ABI version gate, the
refusal order of the six entry points with fake pointers, the new kernels' register allocation, and `SplitPrior.split` / `merge`,
`FlowSequential.encode` / `decode` / `draw_latents` and the samplers' temperature on CPU float64 tensors, where every layer runs its
PyTorch lines.  No GPU needed, the library built."""
import math
import os

import pytest
import torch

import flow_twin
from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSFORMS = ("finc_split_prior", "finc_split_prior_merge")
ENTRIES = TRANSFORMS + ("finc_split_prior_backward",)
SUFFIXES = ("_f32", "_rawbf16_f32")
BIG = 1 << 40
DIMS = (2, 12, 64)                        # a half tensor: 2 * 6 * 64 * 4 = 3072 bytes, the whole one 6144: the fake pointers lie 64 KiB apart


def test_the_six_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for entry in ENTRIES:
        for suffix in SUFFIXES:
            name = entry + suffix
            assert name in _lib.SYMBOLS and name + "(" in header, name
            assert len(getattr(L, name).argtypes) == len(getattr(L, entry + "_f32").argtypes), name
    from fincflow_amd import ops
    for name in ("finc_split_prior", "finc_split_prior_merge", "finc_split_prior_backward", "split_prior_forward"):
        assert callable(getattr(ops, name)), name


def test_version_is_114_and_a_113_library_is_told_to_rebuild(tmp_path):
    assert _lib.SPLIT_LATENT_ABI_VERSION == 114
    assert _lib.lib().finc_version() >= _lib.SPLIT_LATENT_ABI_VERSION
    out = load_stub_library(tmp_path, 113)
    assert "= 113" in out and "114" in out and "rebuild it" in out and "finc_split_prior_f32" in out, out


@pytest.mark.parametrize("suffix", SUFFIXES)
@pytest.mark.parametrize("entry", TRANSFORMS)
def test_transform_refusal_order(entry, suffix):
    """NULL -> 1, bad dims / an output on raw / overlapping activations -> 2, alignment (4 bytes; 2 for a bf16 raw) -> 7, a channel
    count without a kernel -> 3, workspace -> 4, in that order."""
    L = _lib.lib()
    bf16, merge = suffix == "_rawbf16_f32", entry.endswith("merge")
    fn = getattr(L, entry + suffix)
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
    assert f(whole=None, dims=(0, 12, 64)) == 1                              # (NULL comes before the dims)
    for dims in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64)):
        assert f(dims=dims) == 2, dims
    out_names = ("whole",) if merge else ("h1", "h2")
    for name in out_names:
        assert f(**{name: raw}) == 2, name                                   # an output on raw
    # x1, z2 and x may not overlap each other: equal, or one inside the other's bytes
    assert f(h2=h1) == 2 and f(h1=whole) == 2 and f(h2=whole) == 2
    # (every call here ends in a refusal: nothing may reach a launch with these addresses)
    assert f(h2=_p(0x200000 + 3068)) == 2 and f(h2=_p(0x200000 + 3072), ws=None) == 4     # the last dword of x1 / the first one behind it
    assert f(h1=_p(0x100000 + 6140)) == 2 and f(h1=_p(0x100000 + 6144), ws=None) == 4     # the same against the whole tensor
    assert f(whole=_p(0x200000 + 3068)) == 2 and f(whole=_p(0x200000 - 6140)) == 2
    assert f(h1=_p(0x200002), dims=(0, 12, 64)) == 2                         # (dims come before the alignment)
    for name, base in (("whole", 0x100000), ("h1", 0x200000), ("h2", 0x300000), ("a", 0x500000), ("b", 0x510000), ("lp", 0x520000)):
        assert f(**{name: _p(base + 2)}) == 7, name                          # misaligned by 2 bytes
        assert f(**{name: _p(base + 4)}, ws=None) == 4, name                 # on 4 bytes with HW % 4 == 0: accepted (the narrow form)
    assert f(raw=_p(0x400001)) == 7
    assert f(raw=_p(0x400002), ws=None) == (4 if bf16 else 7)                # a bf16 raw is held to 2 bytes, an fp32 one to 4
    assert f(h1=_p(0x200002), dims=(2, 13, 64)) == 7                         # (alignment comes before the channel count)
    for C in (13, 7, 1):
        assert f(dims=(2, C, 64)) == 3, C
        assert f(dims=(2, C, 64), ws=None, nbytes=0) == 3, C                 # (... before the workspace)
    need = L.finc_coupling_workspace_bytes(*DIMS)
    assert f(ws=None) == 4 and f(nbytes=need - 1) == 4 and f(nbytes=0) == 4
    assert f(ws=_p(0x600002)) == 4
    assert f(h1=_p(0x200004), ws=None) == 4                                  # (a half tensor on 4 bytes got past the alignment rule)


@pytest.mark.parametrize("suffix", SUFFIXES)
def test_a_merge_without_log_p_needs_no_workspace_and_refuses_nothing_else(suffix):
    """log_p NULL: the ladder ends at the fault gate / the launch without a look at the workspace (status 4 never appears)."""
    L = _lib.lib()
    fn = getattr(L, "finc_split_prior_merge" + suffix)
    x1, z2, raw, a, b, x = _p(0x200000), _p(0x300000), _p(0x400000), _p(0x500000), _p(0x510000), _p(0x100000)
    assert fn(x1, z2, raw, a, b, x, None, 2, 13, 64, None, 0, None) == 3
    assert fn(x1, z2, raw, a, b, x, _p(0x520000), 2, 12, 64, None, 0, None) == 4
    assert fn(x1, z2, raw, a, b, x, None, 2, 12, 0, None, 0, None) == 2


@pytest.mark.parametrize("suffix", SUFFIXES)
def test_backward_refusal_order(suffix):
    L = _lib.lib()
    bf16 = suffix == "_rawbf16_f32"
    fn = getattr(L, "finc_split_prior_backward" + suffix)
    g1, g2, gl, x, raw, a, b = _p(0x100000), _p(0x200000), _p(0x300000), _p(0x400000), _p(0x500000), _p(0x600000), _p(0x610000)
    gx, gr, ga, gb, ws = _p(0x700000), _p(0x800000), _p(0x900000), _p(0x910000), _p(0xa00000)

    def f(g1=g1, g2=g2, gl=gl, x=x, raw=raw, a=a, b=b, gx=gx, gr=gr, ga=ga, gb=gb, dims=DIMS, ws=ws, nbytes=BIG):
        return fn(g1, g2, gl, x, raw, a, b, gx, gr, ga, gb, *dims, ws, nbytes, None)
    for name in ("x", "raw", "a", "b"):
        assert f(**{name: None}) == 1, name
    assert f(g1=None, g2=None, gl=None) == 1                                 # each incoming gradient may be absent, not all three
    for absent in ("g1", "g2", "gl"):
        assert f(**{absent: None}, ws=None) == 4, absent                     # (one absent: past the NULL rule, down to the workspace)
    assert f(g1=None, g2=None, ws=None) == 4 and f(g2=None, gl=None, ws=None) == 4
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
    assert f(raw=_p(0x500001)) == 7 and f(gr=_p(0x800001)) == 7
    assert f(raw=_p(0x500002), gr=_p(0x800002), ws=None) == (4 if bf16 else 7)
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
    # forward: V in {4, 1} x (split with log p, merge with, merge without) x raw in {fp32, bf16}; backward: V in {4, 1}, the bf16 one
    # is mode 3 of finc_coupling_rawbf16_grad_kernel
    want = {"finc_splitprior_kernel": 12, "finc_splitprior_bwd_kernel": 2}
    for name, count in want.items():
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == count, (name, sorted(ks))
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)
    bf16 = {k: v for k, v in md.items() if "finc_coupling_rawbf16_grad_kernel" in k and "ELi3EE" in k}
    assert len(bf16) == 2, sorted(bf16)
    for k, v in bf16.items():
        assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer on CPU float64 tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def _split_prior(shape=(12, 4, 6), width=16, seed=11):
    from fincflow_amd import glow
    m = glow.SplitPrior(shape, glow.GaussianPrior, width=width)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if name.endswith(("bias", "logs")) else 0.05))
    return m.double()


def test_split_is_the_hand_written_formula_and_merge_undoes_it():
    m = _split_prior()
    torch.manual_seed(4)
    x = torch.randn(3, 12, 4, 6, dtype=torch.float64)
    with torch.no_grad():
        x1, z2, log_p = m.split(x)
        # layers/splitprior.py:7-41 around layers/coupling.py:79-92, written out
        h = m.transform.net(x[:, :6])
        s, t = 2.0 * torch.tanh(h[:, ::2] / 2.0), h[:, 1::2]
        z2_ref = x[:, 6:] * torch.exp(s) + t
        log_p_ref = s.flatten(1).sum(1) - 0.5 * z2_ref.square().flatten(1).sum(1) - 0.5 * 6 * 24 * math.log(2 * math.pi)
        assert torch.equal(x1, x[:, :6])
        assert float((z2 - z2_ref).abs().max()) <= 1e-12 and float((log_p - log_p_ref).abs().max()) <= 1e-12 * float(log_p_ref.abs().max())
        assert float(s.abs().max()) > 0.01                                    # (not the identity coupling)
        assert torch.equal(log_p, m(x)[1]) and torch.equal(x1, m(x)[0])        # what `forward` returns
        back = m.merge(x1, z2)
        assert float((back - x).abs().max()) <= 1e-12
        back2, log_p2 = m.merge(x1, z2, with_log_prob=True)
        assert torch.equal(back2, back) and float((log_p2 - log_p).abs().max()) <= 1e-12 * float(log_p.abs().max())
        # without a latent `merge` draws one, times the temperature, as `reverse` does
        torch.manual_seed(9)
        drawn = m.merge(x1)
        torch.manual_seed(9)
        assert torch.equal(drawn, m.reverse(x1))
        torch.manual_seed(9)
        cool = m.merge(x1, temperature=0.5)
        torch.manual_seed(9)
        assert torch.equal(cool, m.merge(x1, 0.5 * m.base.sample(3)[0]))


def test_a_base_that_is_not_exactly_gaussianprior_keeps_its_own_log_prob():
    from fincflow_amd import glow

    class Wide(glow.GaussianPrior):
        def log_prob(self, input, context=None, sum=True):
            return super().log_prob(input / 2.0, context) - self.dim * math.log(2.0)
    m = glow.SplitPrior((4, 3, 3), Wide, width=8).double()
    assert not m._hip_latent(torch.zeros(1, 4, 3, 3))
    x = torch.randn(2, 4, 3, 3, dtype=torch.float64)
    with torch.no_grad():
        x1, z2, log_p = m.split(x)
        assert torch.equal(log_p, m.base.log_prob(z2) + m.transform(x)[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the model on CPU float64 tensors
# ---------------------------------------------------------------------------------------------------------------------------------
def model64(seed=1):
    """The issue's model as its float64 CPU twin (the units have no CPU path of their own: tests/flow_twin.py), randomised."""
    import numpy as np
    from fincflow_amd import glow
    torch.manual_seed(seed)
    np.random.seed(seed)                                                      # (Conv1x1 draws its orthogonal W from numpy)
    model = glow.create_model(num_blocks=3, block_size=1, split_prior=True, actnorm=True, preprocess=False, image_size=(3, 16, 16),
                              coupling_width=16)
    flow_twin.randomise(model, seed=seed, actnorm=True)
    return flow_twin.twin_of(model)


@pytest.fixture(scope="module")
def twin():
    return model64()


@pytest.fixture(scope="module")
def x():
    return torch.randn(4, 3, 16, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(7))


def test_encode_gives_every_latent_and_the_log_prob_of_forward(twin, x):
    with torch.no_grad():
        zs, log_prob = twin.encode(x)
        want = twin.log_prob(x)
    assert [tuple(z.shape) for z in zs] == [(4, 6, 8, 8), (4, 12, 4, 4), (4, 48, 2, 2)]
    assert sum(z[0].numel() for z in zs) == x[0].numel()                      # the code is complete: as many numbers as the image
    assert float((log_prob - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(zs[-1], twin(x)[0])


def test_decode_of_encode_is_the_input_and_reconstruct_is_not(twin, x):
    """The gap this closes: `reconstruct` resamples the factored-out halves."""
    with torch.no_grad():
        back = twin.decode(twin.encode(x)[0])
        resampled = twin.reconstruct(x)
    assert float((back - x).abs().max()) <= 1e-10
    assert float((resampled - x).abs().max()) > 1e-2


def test_decode_with_log_prob_is_the_log_prob_of_its_result(twin, x):
    with torch.no_grad():
        zs, log_prob = twin.encode(x)
        back, log_q = twin.decode(zs, with_log_prob=True)
    assert torch.equal(back, twin.decode(zs))
    assert float((log_q - log_prob).abs().max()) <= 1e-10 * float(log_prob.abs().max())


def test_draw_latents_draws_in_the_order_of_sample(twin):
    with torch.no_grad():
        torch.manual_seed(5)
        a = twin.decode(twin.draw_latents(3))
        torch.manual_seed(5)
        b, b_true = twin.sample(3)
    assert torch.equal(a, b) and b_true is b


def test_temperature_scales_every_draw(twin):
    T = 0.7
    with torch.no_grad():
        torch.manual_seed(5)
        a, a_true = twin.sample(3, temperature=T)
        torch.manual_seed(5)
        b = twin.decode([T * z for z in twin.draw_latents(3)])
        torch.manual_seed(5)
        c = twin.decode(twin.draw_latents(3, temperature=T))
        torch.manual_seed(5)
        hot = twin.sample(3)[0]
    assert torch.equal(a, b) and torch.equal(a, c) and a_true is a
    assert not torch.equal(a, hot)
    # `also_true_inverse` keeps its meaning at a temperature: the same latents once more, layer by layer without the folds
    with torch.no_grad():
        torch.manual_seed(5)
        d, d_true = twin.sample(3, also_true_inverse=True, temperature=T)
        torch.manual_seed(5)
        e, e_true = twin.sample(3, compute_expensive=True, also_true_inverse=True, temperature=T)
    assert torch.equal(d, a) and d_true is not d and float((d_true - d).abs().max()) <= 1e-12 and e_true is e
    torch.manual_seed(5)
    r = twin.rsample(3, temperature=T)
    assert r.requires_grad and float((r.detach() - a).abs().max()) <= 1e-12


def _method_calls(model, fn):
    """The methods of the model and of its split layers that `fn()` goes through, in order."""
    calls, undo = [], []
    targets = [(model, n) for n in ("decode", "draw_latents", "_reverse_chain")]
    targets += [(m, n) for m in model.sequence_modules if hasattr(m, "split") for n in ("reverse", "merge", "draw")]
    for obj, name in targets:
        def spy(*a, _orig=getattr(obj, name), _name=type(obj).__name__ + "." + name, **k):
            calls.append(_name)
            return _orig(*a, **k)
        setattr(obj, name, spy)
        undo.append((obj, name))
    try:
        fn()
    finally:
        for obj, name in undo:
            delattr(obj, name)
    return calls


def test_temperature_one_leaves_the_call_list_of_sample_as_it_is(twin):
    with torch.no_grad():
        plain = _method_calls(twin, lambda: twin.sample(2))
        one = _method_calls(twin, lambda: twin.sample(2, temperature=1.0))
        cool = _method_calls(twin, lambda: twin.sample(2, temperature=0.7))
    assert plain == ["FlowSequential._reverse_chain", "SplitPrior.reverse", "SplitPrior.reverse"]
    assert one == plain
    assert cool[:2] == ["FlowSequential.draw_latents", "SplitPrior.draw"] and "FlowSequential.decode" in cool
    assert cool.count("SplitPrior.merge") == 2 and "SplitPrior.reverse" not in cool


def test_the_encode_loss_has_the_gradients_of_the_log_prob_loss(x):
    model = model64()
    names, params = zip(*model.named_parameters())
    got = torch.autograd.grad(-model.encode(x)[1].mean(), params)
    want = torch.autograd.grad(-model.log_prob(x).mean(), params)
    for name, g, w in zip(names, got, want):
        assert float(w.abs().max()) > 0, name                                # every parameter is reached
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max()), name


def test_decode_refuses_a_short_list_and_a_wrong_shape(twin, x):
    with torch.no_grad():
        zs = twin.encode(x)[0]
        with pytest.raises(ValueError):
            twin.decode(zs[1:])
        with pytest.raises(ValueError):
            twin.decode(zs + [zs[-1]])
        with pytest.raises(ValueError):
            twin.decode([zs[0][:, :, :4], zs[1], zs[2]])                      # a split layer's latent
        with pytest.raises(ValueError):
            twin.decode([zs[0], zs[1], zs[2][:, :24]])                        # the stack's output
        with pytest.raises(ValueError):
            twin.decode([zs[0][:2], zs[1], zs[2]])                            # another batch


def test_state_dict_keys_did_not_move():
    from fincflow_amd import glow
    keys = list(glow.SplitPrior((12, 4, 4), glow.GaussianPrior, width=8).state_dict())
    assert keys == ["transform." + k for k in ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias",
                                               "net.4.logs")], keys
    kw = dict(num_blocks=2, block_size=1, actnorm=True, preprocess=False, image_size=(3, 8, 8), coupling_width=8)
    model = glow.create_model(split_prior=True, **kw)
    keys = list(model.state_dict())
    splits = [n for n, m in model.named_modules() if isinstance(m, glow.SplitPrior)]
    assert len(splits) == 1
    # a split layer holds its coupling's seven tensors and nothing else; everything else is named as it always was
    mine = [k for k in keys if k.startswith(splits[0] + ".")]
    assert mine == [splits[0] + ".transform." + k for k in ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight",
                                                            "net.4.bias", "net.4.logs")], mine
    plain = list(glow.create_model(split_prior=False, **kw).state_dict())
    assert [k for k in keys if k not in mine][:len(plain) // 2] == plain[:len(plain) // 2]     # the first block: the same names
