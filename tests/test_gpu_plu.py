"""glow.Conv1x1LU on the device: the compose kernels against float64 at every width where their indexing takes another
path, the `need_*` subsets, guard bands, a `perm` entry out of range, the recorded op, a stream capture; the layer against its float64
twin (tests/flow_twin.py) alone and in a two-level stack, through every view of a training loop; and no factorisation left on any
path.  Every error is helpers.rel_err against float64 under the project's bar of 1e-5 (plu_cases.BAR; CHAIN_TOL for what runs
through a whole stack, as tests/test_gpu_train_loop.py judges it) and goes to the parity report (kind `plu`)."""
import itertools

import numpy as np
import pytest
import torch

import flow_twin
from helpers import guarded, guards_intact, same_bits
from plu_cases import BAR, factors, judge, leaves64, make_layer, ref64
from test_gpu_inverse_backward import CHAIN_TOL
from test_gpu_train_loop import Twins, clip, every_view, forward_kl, initialise, judge_grads, optimiser, three

pytestmark = pytest.mark.gpu

CAP = 512
# below a wave (1 .. 4, 12), one past the staged block of 16 rows (17), a width without a mix kernel (20), 48, a wave's 64 entries
# and one past (64, 65), the second slot's end and one past (128, 129), the widest mix (192), a workgroup's 256 columns and one
# past (256, 257), the cap
WIDTHS = (1, 2, 3, 4, 12, 17, 20, 48, 64, 65, 128, 129, 192, 256, 257, CAP)
MODEL = dict(num_blocks=2, block_size=2, actnorm=True, split_prior=True, image_size=(3, 8, 8), coupling_width=16, lu_conv1x1=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def on(dev, m):
    return tuple(t.detach().to(dev).contiguous() for t in factors(m))


def reference(m, grad_w, grad_ld):
    """float64: (w, w_inv, logdet) and the gradients of sum(grad_w * w) + grad_ld * logdet."""
    lower, upper, log_s, sign_s, perm = leaves64(m)
    w, w_inv, ld = ref64(lower, upper, log_s, sign_s, perm)
    loss = (w * grad_w.double()).sum() + (0.0 if grad_ld is None else float(grad_ld)) * ld
    return (w, w_inv, ld), torch.autograd.grad(loss, (lower, upper, log_s))


def masked_zeros(gl, gu):
    C = gl.shape[0]
    up, low = torch.ones(C, C, dtype=torch.bool).triu(0), torch.ones(C, C, dtype=torch.bool).tril(0)
    bits = lambda t: t.cpu().view(torch.int32)
    return not bool(bits(gl)[up].any()) and not bool(bits(gu)[low].any())           # +0, bit for bit


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
def test_compose_and_its_backward_against_float64(C, dev):
    from fincflow_amd import ops
    assert ops.plu_supported(C)
    for perturb in (True, False):
        m = make_layer(C, perturb)
        p = on(dev, m)
        g = torch.Generator().manual_seed(C)
        grad_w, grad_ld = torch.randn(C, C, generator=g), torch.randn((), generator=g)
        out = ops.finc_plu_compose(*p)
        (w, w_inv, ld), grads = reference(m, grad_w, grad_ld)
        if perturb:
            judge("compose", ["w", "w_inv", "logdet"], out, [w, w_inv, ld], C=C, perturbed=True)
        else:
            # an orthogonal matrix: the log-det is zero and its float64 reference is that reference's own rounding (5e-17 at C = 2),
            # so the sum is judged against the size of its terms, sum |log_s|
            scale = m.log_s.detach().double().abs().sum().clamp_min(1e-30)
            judge("compose", ["w", "w_inv", "logdet / sum|log_s|"], [out[0], out[1], 1.0 + (out[2].cpu().double() - ld.detach()) / scale],
                  [w, w_inv, torch.ones((), dtype=torch.float64)], C=C, perturbed=False)
        if not perturb:                                       # the drawn orthogonal matrix again
            np.random.seed(1000 + C)
            q = torch.from_numpy(np.linalg.qr(np.random.randn(C, C))[0])
            judge("compose/initialisation", ["w"], out[:1], [q], C=C)
        again = ops.finc_plu_compose(*p)
        assert all(same_bits(a, b) for a, b in zip(out, again))
        got = ops.finc_plu_compose_backward(grad_w.to(dev), grad_ld.to(dev), *p)
        judge("compose_backward", ["grad_lower", "grad_upper", "grad_log_s"], got, grads, C=C, perturbed=perturb, grad_logdet=True)
        assert masked_zeros(got[0], got[1])
        assert all(same_bits(a, b) for a, b in zip(got, ops.finc_plu_compose_backward(grad_w.to(dev), grad_ld.to(dev), *p)))
        got = ops.finc_plu_compose_backward(grad_w.to(dev), None, *p)
        judge("compose_backward", ["grad_lower", "grad_upper", "grad_log_s"], got, reference(m, grad_w, None)[1], C=C,
              perturbed=perturb, grad_logdet=False)
        assert masked_zeros(got[0], got[1])


def test_every_subset_of_the_outputs(dev):
    from fincflow_amd import ops
    C = 12
    p = on(dev, make_layer(C))
    grad_w, grad_ld = torch.randn(C, C, device=dev), torch.randn((), device=dev)
    full, full_b = ops.finc_plu_compose(*p), ops.finc_plu_compose_backward(grad_w, grad_ld, *p)
    for need in itertools.product((False, True), repeat=3):
        for whole, part in ((full, ops.finc_plu_compose(*p, *need)), (full_b, ops.finc_plu_compose_backward(grad_w, grad_ld, *p, *need))):
            assert [t is not None for t in part] == list(need), need
            assert all(same_bits(a, b) for a, b, n in zip(whole, part, need) if n), need


def raw_compose(dev, p, C, lead=0):
    """The entry point itself on guarded outputs: ((view, buffer) of w, w_inv, logdet)."""
    from fincflow_amd import ops
    outs = [guarded(torch.zeros(s), dev, lead) for s in ((C, C), (C, C), (1,))]
    ops._call("finc_plu_compose_f32", dev, *(t.data_ptr() for t in p), *(v.data_ptr() for v, _ in outs), C, ops._stream_ptr(p[0]))
    return outs


def raw_backward(dev, p, C, grad_w, grad_ld, lead=0):
    from fincflow_amd import ops
    outs = [guarded(torch.zeros(s), dev, lead) for s in ((C, C), (C, C), (C,))]
    ops._call("finc_plu_compose_backward_f32", dev, grad_w.data_ptr(), grad_ld.data_ptr(), *(t.data_ptr() for t in p),
              *(v.data_ptr() for v, _ in outs), C, ops._stream_ptr(p[0]))
    return outs


@pytest.mark.parametrize("C", (1, 17, 65, 192, 257))
def test_every_output_stays_inside_its_guard_band(C, dev):
    from fincflow_amd import ops
    p = on(dev, make_layer(C))
    grad_w, grad_ld = torch.randn(C, C, device=dev), torch.randn((), device=dev)
    plain, plain_b = ops.finc_plu_compose(*p), ops.finc_plu_compose_backward(grad_w, grad_ld, *p)
    for lead in (0, 1):
        for outs, want in ((raw_compose(dev, p, C, lead), plain), (raw_backward(dev, p, C, grad_w, grad_ld, lead), plain_b)):
            torch.cuda.synchronize()
            for (view, buf), t in zip(outs, want):
                assert guards_intact(buf, view), (C, lead)
                assert same_bits(view.reshape(t.shape), t), (C, lead)


@pytest.mark.parametrize("C,bad", ((17, 17), (17, -1), (65, 65), (65, -1)))
def test_a_perm_entry_out_of_range_is_never_an_index(C, bad, dev):
    """The kernels are specified never to form an address from an unchecked entry of `perm`: row r of w and column r of w_inv are NaN,
    everything else keeps the bits of the clean call; in the backward the row of G_M that no entry names reads as NaN -- row i of
    grad_lower, rows <= i of grad_upper and grad_log_s -- and the rest keeps its bits.  Guard bands intact."""
    from fincflow_amd import ops
    m = make_layer(C)
    p = on(dev, m)
    r = int((m.perm > 2).nonzero()[0])
    i = int(m.perm[r])
    perm = p[4].clone()
    perm[r] = bad
    q = p[:4] + (perm,)
    grad_w, grad_ld = torch.randn(C, C, device=dev), torch.randn((), device=dev)
    clean, clean_b = ops.finc_plu_compose(*p), ops.finc_plu_compose_backward(grad_w, grad_ld, *p)
    outs, outs_b = raw_compose(dev, q, C), raw_backward(dev, q, C, grad_w, grad_ld)
    torch.cuda.synchronize()
    assert all(guards_intact(buf, view) for view, buf in outs + outs_b)
    w, w_inv, ld = (v for v, _ in outs)
    rows, cols = torch.arange(C, device=dev) != r, torch.arange(C, device=dev) != r
    assert bool(w[r].isnan().all()) and same_bits(w[rows], clean[0][rows])
    assert bool(w_inv[:, r].isnan().all()) and same_bits(w_inv[:, cols], clean[1][:, cols])
    assert same_bits(ld.reshape(()), clean[2])
    gl, gu, gs = (v for v, _ in outs_b)
    other = torch.arange(C, device=dev) != i
    assert bool(gl[i, :i].isnan().all()) and same_bits(gl[other], clean_b[0][other]) and same_bits(gl[i, i:], clean_b[0][i, i:])
    assert same_bits(gu[i + 1:], clean_b[1][i + 1:]) and same_bits(gs[i + 1:], clean_b[2][i + 1:])
    strict = torch.ones(C, C, dtype=torch.bool, device=dev).triu(1)[:i + 1]
    assert bool(gu[:i + 1][strict].isnan().all()) and not bool(gu[:i + 1][~strict].view(torch.int32).any())
    assert bool(gs[:i + 1].isnan().all())


@pytest.mark.parametrize("C", (12, 65, 192))
def test_the_recorded_op_against_float64(C, dev):
    """torch.autograd.gradcheck is not applicable in fp32: `plu_compose` + `.backward()` against the float64 lines for a loss that
    uses w, w_inv and logdet together.  The loss is elementwise in the three outputs: a matrix product of its own, in fp32 at cond(W)
    about 2,000, would put torch's rounding into the gradients that reach the op, and this test is about the op."""
    from fincflow_amd import ops
    m = make_layer(C)
    g = torch.Generator().manual_seed(5 + C)
    a, b = torch.randn(C, C, generator=g), torch.randn(C, C, generator=g)

    def loss_of(w, w_inv, ld, put):
        return (w * put(a)).sum() + (w_inv * put(b)).sum() + 1.5 * ld + (w * w_inv.t()).sum() * ld
    lower, upper, log_s, sign_s, perm = leaves64(m)
    want = loss_of(*ref64(lower, upper, log_s, sign_s, perm), lambda t: t.double())
    want_g = torch.autograd.grad(want, (lower, upper, log_s))
    p = on(dev, m)
    leaves = [t.requires_grad_(True) for t in p[:3]]
    got = loss_of(*ops.plu_compose(*leaves, p[3], p[4]), lambda t: t.to(dev))
    got.backward()
    judge("recorded", ["loss", "grad_lower", "grad_upper", "grad_log_s"], [got] + [t.grad for t in leaves], [want] + list(want_g), C=C)
    assert masked_zeros(leaves[0].grad, leaves[1].grad)
    # only what is asked for is computed: w_inv alone, and a frozen `upper`
    leaves = [t.detach().requires_grad_(i != 1) for i, t in enumerate(p[:3])]
    w, w_inv, ld = ops.plu_compose(*leaves, p[3], p[4], need_w=False, need_logdet=False)
    assert w is None and ld is None
    (w_inv * b.to(dev)).sum().backward()
    lower, upper, log_s, sign_s, perm = leaves64(m)
    want_g = torch.autograd.grad((ref64(lower, upper, log_s, sign_s, perm)[1] * b.double()).sum(), (lower, log_s))
    assert leaves[1].grad is None
    judge("recorded/w_inv_alone", ["grad_lower", "grad_log_s"], [leaves[0].grad, leaves[2].grad], want_g, C=C)


def test_compose_and_backward_in_a_stream_capture(dev):
    """A linear chain of launches on static tensors in one torch.cuda.graph: parameters changed in place, one replay, the results
    of an eager call on the new values."""
    from fincflow_amd import ops
    C = 48
    p = on(dev, make_layer(C))
    leaves = [t.requires_grad_(True) for t in p[:3]]
    a, b = torch.randn(C, C, device=dev), torch.randn(C, C, device=dev)

    def run():
        w, w_inv, ld = ops.plu_compose(*leaves, p[3], p[4])
        loss = (w * a).sum() + (w_inv * b).sum() + 2.0 * ld
        return [w.detach(), w_inv.detach(), ld.detach()] + list(torch.autograd.grad(loss, leaves))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    with torch.no_grad():
        leaves[0].add_(0.01 * torch.randn(C, C, device=dev).tril(-1))
        leaves[1].add_(0.01 * torch.randn(C, C, device=dev).triu(1))
        leaves[2].add_(0.05)
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    assert all(same_bits(s, e) for s, e in zip(static, eager))


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (4, 12, 20, 48))
@pytest.mark.parametrize("hw", ((4, 4), (6, 5)))
def test_the_layer_against_its_float64_twin(C, hw, dev):
    from fincflow_amd import layers, ops
    m = make_layer(C).to(dev)
    twin = flow_twin.twin_of(m)
    g = torch.Generator().manual_seed(C + hw[1])
    x, gz, gld = torch.randn(3, C, *hw, generator=g), torch.randn(3, C, *hw, generator=g), torch.randn(3, generator=g)
    tag = dict(C=C, hw=list(hw))

    def both(fn):
        return fn(m, lambda t: t.to(dev)), fn(twin, lambda t: t.double())

    def grads_of(layer, outs, weights, x_in):
        loss = sum((o * w).sum() for o, w in zip(outs, weights))
        return list(torch.autograd.grad(loss, [x_in] + list(layer.parameters())))

    def fwd(layer, put, grad):
        x_in = put(x).requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            z, ldj = layer(x_in)
        ldj = ldj.expand(3)
        return [z.detach(), ldj.detach()] + (grads_of(layer, (z, ldj), (put(gz), put(gld)), x_in) if grad else [])
    names = ["z", "ldj", "grad_x", "grad_lower", "grad_upper", "grad_log_s"]
    got, want = both(lambda l, put: fwd(l, put, False))
    judge("layer/forward", names[:2], got, want, **tag)
    got_g, want_g = both(lambda l, put: fwd(l, put, True))
    judge("layer/forward_recorded", names, got_g, want_g, **tag)
    assert same_bits(got_g[0], got[0]) and masked_zeros(got_g[3], got_g[4])

    def rev(layer, put, grad, logdet):
        z_in = put(x).requires_grad_(grad)
        with torch.set_grad_enabled(grad), ops.reverse_grad():
            out = layer.reverse_with_logdet(z_in) if logdet else (layer.reverse(z_in),)
        outs = [out[0]] + ([out[1].expand(3)] if logdet else [])
        return [o.detach() for o in outs] + (grads_of(layer, outs, (put(gz), put(gld)), z_in) if grad else [])
    for logdet in (False, True):
        n = ["x"] + (["ldj"] if logdet else [])
        got, want = both(lambda l, put: rev(l, put, False, logdet))
        judge("layer/reverse" + ("_with_logdet" if logdet else ""), n, got, want, **tag)
        got_g, want_g = both(lambda l, put: rev(l, put, True, logdet))
        judge("layer/reverse_recorded" + ("_with_logdet" if logdet else ""), n + names[2:], got_g, want_g, **tag)
        assert same_bits(got_g[0], got[0])
    # under bf16 autocast: fp32 outputs with the bits of the call outside it
    with torch.no_grad():
        plain = list(m(x.to(dev))) + [m.reverse(x.to(dev))]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            cast = list(m(x.to(dev))) + [m.reverse(x.to(dev))]
    assert all(c.dtype == torch.float32 and same_bits(c, q) for c, q in zip(cast, plain))
    x_in = x.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        z, ldj = m(x_in)
    assert z.dtype == ldj.dtype == torch.float32 and same_bits(z.detach(), plain[0]) and same_bits(ldj.detach(), plain[1])
    # from the output, against the stored path
    assert m.invertible_backward_supported(x.to(dev)) == ops.mix_supported(C)
    if ops.mix_supported(C):
        stored = fwd(m, lambda t: t.to(dev), True)
        with torch.no_grad():
            x_back, gx, _, gp = m.backward_from_output(stored[0], gz.to(dev), gld.to(dev), None, layers.BackwardNeeds())
        judge("layer/backward_from_output", ["x"] + names[2:], [x_back, gx] + gp, [x.double()] + fwd(twin, lambda t: t.double(), True)[2:], **tag)
        assert masked_zeros(gp[0], gp[1])
        errs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip([gx] + gp, stored[2:])]
        assert max(errs) <= BAR, errs


# ---------------------------------------------------------------------------------------------------------------------------------
# in a stack
# ---------------------------------------------------------------------------------------------------------------------------------
BATCH = 8                    # (tests/test_gpu_train_loop.py's views draw that many)


def pixel_batch(seed=6):
    """Integer grey levels 16 .. 239 plus the dequantisation noise, drawn once for both sides (test_gpu_train_loop.pixel_batch)."""
    gen = torch.Generator().manual_seed(seed)
    pixels = torch.randint(16, 240, (BATCH,) + MODEL["image_size"], generator=gen)
    return pixels.float() + torch.rand(pixels.shape, generator=gen)


def stack(dev, seed=0, **changes):
    """(the model of the issue, the same modules without the dequantisation layer: what the twins follow)."""
    from fincflow_amd import FlowSequential, glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = flow_twin.randomise(glow.create_model(**dict(MODEL, **changes)), seed=seed + 1).to(dev)
    assert isinstance(list(model)[0], glow.Dequantization)
    want = glow.Conv1x1LU if dict(MODEL, **changes)["lu_conv1x1"] else glow.Conv1x1
    assert sum(type(m) is want for m in model.modules()) == 4 and sum(isinstance(m, glow.Conv1x1) for m in model.modules()) == 4
    return model, FlowSequential(model.base_distribution, *list(model)[1:])


@pytest.mark.parametrize("invertible", (False, True))
def test_a_training_step_of_the_stack_against_its_twin(invertible, dev):
    _, inner = stack(dev)
    x = pixel_batch()
    initialise(inner, x, dev)
    twins = Twins(inner)
    twins.sync(inner)
    inner.invertible_backward = invertible
    got, want, yard, _ = three(inner, twins, lambda m, put: forward_kl(m, [x]))
    flow_twin.compare("plu/forward_kl/loss", ["bits_per_dim", "log_prob"], got[:2], want[:2], yard[:2], bar=BAR, kind="plu",
                      invertible=invertible)
    judge_grads("plu/forward_kl/grads", inner, twins, ["input"], (got[2:], want[2:], yard[2:]), invertible=invertible)
    lu = [n for n, _ in inner.named_parameters() if n.endswith((".lower", ".upper", ".log_s"))]
    assert len(lu) == 12 and all(dict(inner.named_parameters())[n].grad is not None for n in lu)


def test_encode_decode_round_trip_of_the_stack(dev):
    _, inner = stack(dev)
    x = pixel_batch()
    initialise(inner, x, dev)
    twin = flow_twin.twin_of(inner)
    with torch.no_grad():
        zs, lp = inner.encode(x.to(dev))
        back = inner.decode(zs)
        zs64, lp64 = twin.encode(x.double())
    judge("stack/encode", ["log_prob"] + ["z%d" % i for i in range(len(zs))], [lp] + list(zs), [lp64] + list(zs64), bar=CHAIN_TOL)
    judge("stack/decode(encode)", ["x"], [back], [x.double()], bar=CHAIN_TOL)


@pytest.mark.parametrize("opt_name", ("sgd", "adam_fused"))
def test_three_steps_with_every_view_at_each(opt_name, dev):
    """A derived value one step old is seen: every view of the NEW parameters after each optimiser step, SGD (which advances
    Tensor._version) and Adam(fused=True) (which does not)."""
    _, inner = stack(dev)
    x = pixel_batch()
    initialise(inner, x, dev)
    opt = optimiser(opt_name, inner.parameters())
    twins = Twins(inner)
    for step in range(3):
        twins.sync(inner)
        opt.zero_grad(set_to_none=True)
        three(inner, twins, lambda m, put: forward_kl(m, [x]))     # (on the twins too: the clipped norm is compared)
        clip(inner, twins, opt=opt_name, step=step, layer="Conv1x1LU")
        opt.step()
        every_view(inner, twins, x, opt=opt_name, step=step, layer="Conv1x1LU")
        clip(inner, twins, opt=opt_name, step=step, layer="Conv1x1LU")
        opt.step()


def test_the_folds_of_sample_are_those_of_conv1x1(dev, monkeypatch):
    """[FastFlowUnit, ActNorm, mix] -- in the reverse chain the mix applies the unit's lead matrix where the library takes the
    premultiplied form (`reverse_after_mix`), else ActNorm folds into the unit -- and [ActNorm, mix], where no unit follows and the
    mix takes ActNorm's affine map (`reverse_then_affine`): the same counts with either layer as the mix."""
    from fincflow_amd import FastFlowUnit, FlowSequential, _lib, glow
    calls = {}

    def spy(cls, name):
        fn = getattr(cls, name)

        def counted(*args, **kwargs):
            out = fn(*args, **kwargs)
            if out is not None:
                calls[name] = calls.get(name, 0) + 1
            return out
        monkeypatch.setattr(cls, name, counted)
    spy(FastFlowUnit, "reverse_after_mix")
    spy(glow.Conv1x1, "reverse_then_affine")
    C, H, W = 12, 16, 16
    n = next(b for b in range(1, 2049) if _lib.lib().finc_inverse_premultiplied_supported(b, 4, C // 4, H, W, 3, 3))

    def build(mix, with_unit):
        torch.manual_seed(0)
        np.random.seed(0)
        an = glow.ActNorm(C)
        with torch.no_grad():
            an.log_scale.copy_(0.1 * torch.randn(C))
            an.translation.copy_(0.1 * torch.randn(C))
        an.mark_initialized()
        return FlowSequential(glow.GaussianPrior((C, H, W)), *([FastFlowUnit(C, C, (3, 3))] if with_unit else []), an, mix(C)).to(dev)
    counts = {}
    for mix in (glow.Conv1x1LU, glow.Conv1x1):
        for with_unit in (True, False):
            model = build(mix, with_unit)
            for batch in (2, n):
                calls.clear()
                torch.manual_seed(1)
                with torch.no_grad():
                    x = model.sample(batch)[0]
                assert bool(torch.isfinite(x).all())
                counts.setdefault(mix.__name__, []).append(dict(calls))
    assert counts["Conv1x1LU"] == counts["Conv1x1"], counts
    assert counts["Conv1x1LU"] == [{}, {"reverse_after_mix": 1}, {"reverse_then_affine": 1}, {"reverse_then_affine": 1}], counts


def test_no_factorisation_is_left_on_any_path(dev, monkeypatch):
    model, inner = stack(dev)
    x = pixel_batch()
    initialise(inner, x, dev)

    def refuse(*args, **kwargs):
        raise AssertionError("a dense factorisation was called")
    for mod, name in ((torch.linalg, "slogdet"), (torch, "slogdet"), (torch, "inverse"), (torch.linalg, "inv"), (torch.linalg, "inv_ex"),
                      (torch, "logdet"), (torch.linalg, "lu_factor"), (torch.linalg, "solve")):
        monkeypatch.setattr(mod, name, refuse)
    opt = torch.optim.SGD(inner.parameters(), lr=0.01)
    for invertible in (False, True):
        inner.invertible_backward = invertible
        opt.zero_grad(set_to_none=True)
        forward_kl(inner, [x])
        opt.step()
    inner.invertible_backward = False
    with torch.no_grad():
        inner.sample(BATCH)
        inner.sample_with_log_prob(BATCH)
    xs = inner.rsample(BATCH)
    xs.square().mean().backward()
    xs, log_q = inner.rsample_with_log_prob(BATCH)
    (log_q + 0.5 * xs.square().flatten(1).sum(1)).mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in inner.parameters())
