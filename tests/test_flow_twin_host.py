"""The float64 twin of tests/flow_twin.py, checked without a GPU: against the trace recorded from the reference's own layers, against
the CPU oracle on one small bank per orientation word, its noise replay -- and that a model with units in it can be copied at all
(copy.deepcopy, pickle, torch.save of the module), which the twin and every EMA copy of a model need."""
import copy
import inspect
import pickle
import threading

import numpy as np
import pytest
import torch

import flow_twin
import inverse_backward_ref as ref
from helpers import ORDER_BITS, ORIENT_FASTFLOW, STACK_INPUT, fill_stack_parameters, golden, rel_err
from oracle import oracle
from test_glow_stack import build_ours


def small_model(preprocess=False):
    from fincflow_amd import glow
    torch.manual_seed(0)
    np.random.seed(0)
    model = glow.create_model(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 8, 8), preprocess=preprocess,
                              coupling_width=8)
    return flow_twin.randomise(model, seed=3, actnorm=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the twin against the reference's own data
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_twin_reproduces_the_reference_trace():
    """tests/golden/stack_c4_small.npz was recorded from the reference's layers in float32: the float64 twin of the same stack gives
    its z, logdet and x_rev to the rounding of that recording."""
    from fincflow_amd import FlowSequential, glow
    g = golden("stack_c4_small")
    layers = build_ours()
    fill_stack_parameters(layers, ffu_weights=g)
    twin = flow_twin.twin_of(FlowSequential(glow.GaussianPrior((48, 4, 4)), *layers))
    assert all(p.dtype == torch.float64 and not p.is_cuda for p in twin.parameters())
    x = torch.from_numpy(g["x"]).double()
    assert tuple(x.shape) == STACK_INPUT
    with torch.no_grad():
        h, logdet = x, 0
        for m in twin:
            h, ld = m(h, None)
            logdet = logdet + ld
        z, logp = twin(x)
        x_rev = twin._reverse_chain(torch.from_numpy(g["z_in"]).double(), None)
    errs = (rel_err(h.numpy(), g["z"]), rel_err(logdet.numpy(), g["logdet"]), rel_err(x_rev.numpy(), g["x_rev"]))
    print("twin against the reference trace: z %.1e, logdet %.1e, x_rev %.1e" % errs)
    assert max(errs) <= 1e-5, errs
    assert torch.equal(z, h) and torch.equal(logp, twin.base_distribution.log_prob(h) + logdet)


CASES = [("unit", 4, 3, ORIENT_FASTFLOW)] + [(o, 1, 5, ORDER_BITS[o]) for o in ("TL", "TR", "BL", "BR")] + [("cinc", 1, 8, 0)]


@pytest.mark.parametrize("kind,G,Cq,orient", CASES, ids=[c[0] for c in CASES])
def test_the_twins_units_against_the_oracle(kind, G, Cq, orient):
    """The replaced `forward` / `reverse` of a unit on the twin, on the stored weights, against oracle.forward_f32 (fp64
    accumulation) and oracle.inverse_via_f64: one small bank per orientation word, an odd map."""
    from fincflow_amd import CINCFlowUnit, FastFlowUnit, FlowSequential, PaddedConv2d, glow
    torch.manual_seed(5)
    if kind == "unit":
        m = FastFlowUnit(G * Cq, G * Cq, 3)
        stored = m._weights()
    elif kind == "cinc":
        m = CINCFlowUnit(Cq, Cq, 3)
        stored = [m.conv_tl.conv.weight]
    else:
        m = PaddedConv2d(Cq, Cq, (3, 3), order=kind)
        stored = [m.conv.weight]
    methods = (type(m).forward, type(m).reverse, PaddedConv2d.forward, PaddedConv2d.reverse)
    twin = flow_twin.twin_of(FlowSequential(glow.GaussianPrior((G * Cq, 7, 6)), m))
    tm = list(twin)[0]
    assert type(tm) is type(m) and tm is not m
    # the instances of the twin are replaced: the class, and with it the model the twin was made from, is untouched
    assert methods == (type(m).forward, type(m).reverse, PaddedConv2d.forward, PaddedConv2d.reverse)
    assert not any("forward" in s.__dict__ or "reverse" in s.__dict__ for s in m.modules())
    wc = oracle.canonicalize(torch.cat([w.detach() for w in stored]).numpy(), G, orient)
    x = np.random.default_rng(6).standard_normal((2, G * Cq, 7, 6)).astype(np.float32)
    with torch.no_grad():
        z, ld = tm(torch.from_numpy(x).double())
        back = tm.reverse(z)
        back = back[0] if isinstance(back, tuple) else back
        out, zeros = tm.reverse_with_logdet(z)
    z_ref = oracle.forward_f32(x, wc, G, orient)
    x_ref = oracle.inverse_via_f64(z_ref, wc, G, orient)
    with torch.no_grad():
        x_twin = tm.reverse(torch.from_numpy(z_ref).double())
        x_twin = x_twin[0] if isinstance(x_twin, tuple) else x_twin
    e_f, e_i, e_rt = rel_err(z.numpy(), z_ref), rel_err(x_twin.numpy(), x_ref), rel_err(back.numpy(), x)
    print("%s: forward %.1e, solve %.1e, round trip %.1e" % (kind, e_f, e_i, e_rt))
    assert ld == 0.0 and e_f <= 1e-6 and e_i <= 1e-6 and e_rt <= 1e-12, (e_f, e_i, e_rt)     # (1e-6: the oracle's float32 outputs)
    assert torch.equal(out, back) and torch.equal(zeros, torch.zeros(2, dtype=torch.float64))


def test_the_masks_are_the_modules_own():
    from fincflow_amd import FastFlowUnit, PaddedConv2d
    unit = FastFlowUnit(12, 12, 3)
    masks = flow_twin.stored_masks(unit)
    assert sorted(masks) == ["conv_%s.conv.weight" % o for o in ("bl", "br", "tl", "tr")]
    for name, mask in masks.items():
        assert torch.equal(mask.float(), getattr(unit, name.split(".")[0]).mask), name
    whole = ref.stored_mask(4, 3, 3, 3, ORIENT_FASTFLOW)
    assert torch.equal(whole, torch.cat([masks["conv_%s.conv.weight" % o] for o in ("tl", "tr", "bl", "br")]))
    assert list(flow_twin.stored_masks(PaddedConv2d(4, 4, (3, 3), bias=True, order="BR"))) == ["conv.weight"]


def test_sync_is_exact_and_the_twin_is_independent():
    from fincflow_amd import glow
    model = small_model()
    twin = flow_twin.twin_of(model)
    assert twin.fuse_affine is False and type(model).fuse_affine is True and "fuse_affine" not in model.__dict__
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.01 * torch.randn_like(p))
        for m in model.modules():
            if isinstance(m, glow.ActNorm):
                m.reset_initialization()
    before = {n: p.clone() for n, p in twin.named_parameters()}
    assert all(not torch.equal(before[n].float(), p) for n, p in model.named_parameters())       # no shared storage
    flow_twin.sync(twin, model)
    for (n, p), (n2, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert n == n2 and q.dtype == torch.float64 and torch.equal(q, p.detach().double()), n
    for (n, p), (n2, q) in zip(model.named_buffers(), twin.named_buffers()):
        assert n == n2 and torch.equal(q, p.to(q.dtype)), n
    acts = [m for m in twin.modules() if isinstance(m, glow.ActNorm)]
    assert acts and all(int(m.initialized) == 0 and not m._is_initialized() for m in acts)


# ---------------------------------------------------------------------------------------------------------------------------------
# noise replay
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_replayed_sample_is_the_recorded_one():
    """A float32 twin samples with its draws recorded (the base and the split prior, in the order the reverse chain asks for them); a
    second float32 twin fed the recording gives the same x bit for bit, log_q is `log_prob(x)` of the float64 twin, and a slice of
    the recording gives those images."""
    model = small_model()
    a, b, t64 = flow_twin.twin_of(model, torch.float32), flow_twin.twin_of(model, torch.float32), flow_twin.twin_of(model)
    torch.manual_seed(9)
    with flow_twin.recorded_noise(a) as draws:
        x, log_q = a.sample_with_log_prob(6)
    assert [tuple(d.shape) for d in draws] == [(6, 24, 2, 2), (6, 6, 4, 4)] and "sample" not in a.base_distribution.__dict__
    with flow_twin.replayed_noise(b, draws):
        x2, log_q2 = b.sample_with_log_prob(6)
    assert x.dtype == torch.float32 and torch.equal(x, x2) and torch.equal(log_q, log_q2)
    with torch.no_grad():
        want = t64.log_prob(x.double())
    e = rel_err(log_q.numpy(), want.numpy())
    print("log_q of the float32 twin against log_prob of the float64 twin: %.1e" % e)
    assert e <= 1e-5, e
    pick = [0, 3, 5]
    with flow_twin.replayed_noise(t64, draws, pick):
        x64, log_q64 = t64.sample_with_log_prob(3)
    assert rel_err(x.numpy()[pick], x64.numpy()) <= 1e-5 and rel_err(log_q.numpy()[pick], log_q64.numpy()) <= 1e-5
    # two chains from one base draw (`also_true_inverse`): the split prior draws again for the second
    with flow_twin.recorded_noise(a) as draws:
        a.sample(2, also_true_inverse=True)
    assert [tuple(d.shape) for d in draws] == [(2, 24, 2, 2), (2, 6, 4, 4), (2, 6, 4, 4)]
    with pytest.raises(AssertionError, match="not consumed"):
        with flow_twin.replayed_noise(b, draws):
            b.sample(2)


def test_the_full_models_sample_is_the_floor_of_the_containers():
    """With preprocessing the chain ends in the dequantisation's floor: the container built from `list(model)[1:]` shares the modules
    and stops in front of it."""
    from fincflow_amd import FlowSequential, glow
    model = small_model(preprocess=True)
    assert isinstance(list(model)[0], glow.Dequantization)
    full = flow_twin.twin_of(model, torch.float32)
    inner = FlowSequential(full.base_distribution, *list(full)[1:])
    assert all(p is q for p, q in zip(full.parameters(), inner.parameters()))
    with flow_twin.recorded_noise(full) as draws:
        x_full, _ = full.sample(4)
    with flow_twin.replayed_noise(inner, draws):
        x_inner, _ = inner.sample(4)
    assert torch.equal(x_full, x_inner.floor()) and not torch.equal(x_full, x_inner)


# ---------------------------------------------------------------------------------------------------------------------------------
# copying a model with units in it
# ---------------------------------------------------------------------------------------------------------------------------------
def _unit(kind):
    from fincflow_amd import CINCFlowUnit, FastFlowUnit, PaddedConv2d, glow
    torch.manual_seed(1)
    np.random.seed(1)
    if kind == "FastFlowUnit":
        return FastFlowUnit(12, 12, 3)
    if kind == "PaddedConv2d":
        return PaddedConv2d(5, 5, (3, 3), bias=True, order="BR")
    if kind == "CINCFlowUnit":
        return CINCFlowUnit(8, 8, 3)
    return glow.create_model(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 8, 8), coupling_width=8)


def _copy(how, m, tmp_path):
    if how == "deepcopy":
        return copy.deepcopy(m)
    if how == "pickle":
        return pickle.loads(pickle.dumps(m))
    path = tmp_path / "module.pt"
    torch.save(m, path)
    return torch.load(path, weights_only=False)


@pytest.mark.parametrize("how", ["deepcopy", "pickle", "torch_save"])
@pytest.mark.parametrize("kind", ["FastFlowUnit", "PaddedConv2d", "CINCFlowUnit", "create_model"])
def test_a_module_with_a_bank_cache_can_be_copied(kind, how, tmp_path):
    """The copy gets a fresh, empty PackedWeights (no shared banks, a lock of its own); parameters, state dict and the layers' plain
    attributes survive."""
    from fincflow_amd import PaddedConv2d, ops
    m = _unit(kind)
    caches = [(n, s._cache) for n, s in m.named_modules() if isinstance(getattr(s, "_cache", None), ops.PackedWeights)]
    assert caches
    for _, c in caches:                                    # as after a call on some device: an entry the copy must not carry
        c._banks["a device"] = ops._DeviceBank(key=(1, 2, 3))
    c = _copy(how, m, tmp_path)
    assert type(c) is type(m) and c is not m
    mods = dict(c.named_modules())
    for name, cache in caches:
        new = mods[name]._cache
        assert type(new) is ops.PackedWeights and new is not cache and new._banks == {} and new.w_canon is None
        assert new._lock is not cache._lock and isinstance(new._lock, type(threading.Lock()))
        with new._lock:
            pass
        assert list(cache._banks) == ["a device"]          # the original keeps what it had
    sd, sd_c = m.state_dict(), c.state_dict()
    assert list(sd) == list(sd_c) and all(torch.equal(sd[k], sd_c[k]) and sd[k].data_ptr() != sd_c[k].data_ptr() for k in sd)
    for (n, p), (n2, q) in zip(m.named_parameters(), c.named_parameters()):
        assert n == n2 and torch.equal(p, q) and p is not q and q.requires_grad == p.requires_grad
    for name, s in m.named_modules():
        if isinstance(s, PaddedConv2d):
            t = mods[name]
            assert torch.equal(t.mask, s.mask) and t.order == s.order and t.pad == s.pad and t.kernel_size == s.kernel_size


def test_the_deep_copy_in_double_is_the_idiom_of_the_other_layers():
    from fincflow_amd import FastFlowUnit
    m = copy.deepcopy(FastFlowUnit(12, 12, 3)).double()
    assert all(w.dtype == torch.float64 for w in m._weights())


# ---------------------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_train_loop.py found: a fused optimiser step does not advance Tensor._version
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda p: torch.optim.Adam(p, lr=0.05, fused=True), lambda p: torch.optim.SGD(p, lr=0.05, fused=True),
                                  lambda p: torch.optim.Adam(p, lr=0.05)], ids=["adam_fused", "sgd_fused", "adam"])
def test_values_cached_per_parameter_version_follow_an_optimiser_step(make):
    """Conv1x1 keeps W^-1 and log|det W| per `ops.version_key(W)`.  PyTorch's fused optimisers write the parameters without advancing
    their version counters (asserted here, so that this test says when that changes): the key carries the process's optimiser steps,
    and the cached inverse follows the step."""
    from fincflow_amd import glow, ops
    if "fused" not in inspect.signature(torch.optim.Adam).parameters:
        pytest.skip("this torch build has no fused optimisers")
    torch.manual_seed(2)
    np.random.seed(2)
    m = glow.Conv1x1(12)
    try:
        opt = make([m.W])
    except RuntimeError as e:                              # (a build whose fused optimisers take device tensors only)
        pytest.skip(str(e))
    z = torch.randn(2, 12, 4, 4)
    with torch.no_grad():
        before, ld_before = m.reverse_with_logdet(z)
    m.W.grad = torch.randn(12, 12)
    key, version = ops.version_key(m.W), m.W._version
    opt.step()
    assert ops.version_key(m.W) != key
    if opt.defaults.get("fused"):
        assert m.W._version == version                     # what made the key on (address, version) alone go stale
    with torch.no_grad():
        after, ld_after = m.reverse_with_logdet(z)
    w64 = m.W.detach().double()
    want = torch.einsum("oc,bchw->bohw", torch.inverse(w64), z.double())
    assert rel_err(after.numpy(), want.numpy()) <= 1e-5 and rel_err(before.numpy(), want.numpy()) > 1e-3
    assert rel_err(ld_after.numpy(), (16 * torch.slogdet(w64)[1]).expand(2).numpy()) <= 1e-5 and not torch.equal(ld_before, ld_after)


def test_a_replayed_activation_pattern_is_the_recorded_one():
    """flow_twin.recorded_masks / replayed_masks: the pattern of every call of every nn.ReLU, in order; replayed, the twin's nets take
    it -- the same branch of the piecewise-linear net on both sides of a gradient comparison -- and an activation that is not within
    rounding of zero may not change sides."""
    model = small_model()
    a, t64 = flow_twin.twin_of(model, torch.float32), flow_twin.twin_of(model)
    x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(2))
    with flow_twin.recorded_masks(a) as masks:
        a.log_prob(x).mean().backward()
        a.log_prob(x[:2])
    assert len(masks) == 6 and all(len(v) == 2 and v[0].dtype == torch.bool and len(v[0]) == 4 and len(v[1]) == 2 for v in masks.values())
    assert not any(m._forward_hooks for m in a.modules())
    with flow_twin.replayed_masks(t64, masks) as flips:
        t64.log_prob(x.double()).mean().backward()
        t64.log_prob(x[:2].double())
        free = t64.log_prob(x.double())                    # nothing recorded is left: the modules run as they are
    assert flips[0] >= 0 and not any(m._forward_hooks for m in t64.modules())
    with torch.no_grad():
        assert torch.equal(free, t64.log_prob(x.double()))
    ga, g64 = dict(a.named_parameters())["4.net.0.weight"].grad, dict(t64.named_parameters())["4.net.0.weight"].grad
    assert rel_err(ga.numpy(), g64.numpy()) <= 1e-5
    wrong = {n: [~m for m in v] for n, v in masks.items()}             # every activation on the other side
    with pytest.raises(AssertionError, match="changed sides"):
        with flow_twin.replayed_masks(t64, wrong):
            t64.log_prob(x.double())
    with pytest.raises(AssertionError, match="not consumed"):
        with flow_twin.replayed_masks(t64, masks):
            t64.log_prob(x.double())
