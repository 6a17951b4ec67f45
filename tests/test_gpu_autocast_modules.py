"""glow.Coupling, SplitPrior and whole models under torch.autocast(device_type="cuda", dtype=torch.bfloat16): only the coupling NET
runs in bfloat16; its output goes to the HIP transform as it lies (the _rawbf16_f32 entry points, finc_bias_relu_bf16 on the
inference path), and x, y, the log-det and every gradient outside the net stay fp32.  These tests run bf16 convolutions (tiny ones).

Bars.
  * y and the log-det against helpers.coupling_ref in float64 on the SAME bf16 `raw`: 1e-5 (TOL of tests/test_gpu_coupling.py) -- the
    transform is fp32 arithmetic on values that are exact in both.
  * reverse(forward(x)) under no_grad: TOL as well.  Both directions compute `raw` from the untouched half, so they see the same bits.
  * gradients against the upcasting alternative (the same module under the same autocast with the HIP path off, so that the PyTorch
    lines run on `raw.float()`), and invertible_backward against the stored path: 2^-7, max-normalised (helpers.rel_err).  Both
    pipelines hand the net's backward a bf16 grad_raw rounded from fp32 values that agree to fp32 rounding; where that difference
    straddles a bf16 tie a single element moves by one bf16 ulp, 2^-8 of its own magnitude and at most 2^-8 of the largest; 2^-7
    leaves a factor of two for such elements meeting in one sum.  Derived, not measured; the measured values go to the parity
    report (helpers.report).
  * log_q of sample_with_log_prob against log_prob of the same x: CHAIN_TOL, the bar tests/test_gpu_sample_logdet.py holds the fp32
    model to."""
import pytest
import torch

from helpers import coupling_ref, rel_err, report, same_bits
from test_gpu_coupling import TOL, fill
from test_gpu_inverse_backward import CHAIN_TOL
from test_gpu_sample_logdet import fix_latents

pytestmark = pytest.mark.gpu

GRAD_BAR = 2.0 ** -7
F32_ENTRIES = ("finc_coupling_f32", "finc_coupling_backward_f32", "finc_coupling_reverse_backward_f32", "finc_coupling_reverse_logdet_f32",
               "finc_coupling_reverse_logdet_backward_f32", "finc_coupling_backward_reconstruct_f32", "finc_bias_relu_f32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def autocast():
    return torch.autocast(device_type="cuda", dtype=torch.bfloat16)


def record_entries(monkeypatch):
    """Every entry point of the library that fincflow_amd.ops calls from here on, by name."""
    from fincflow_amd import ops
    names = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *args, **kw: (names.append(name), real(name, *args, **kw))[1])
    return names


def coupling_calls(names):
    return [n for n in names if n.startswith(("finc_coupling", "finc_bias_relu"))]


def make_coupling(n_context, dev):
    from fincflow_amd import glow
    m = fill(glow.Coupling((4, 4, 4), width=8, n_context=n_context)).to(dev)
    torch.manual_seed(7 + (n_context or 0))
    x = torch.randn(2, 4, 4, 4, device=dev)
    ctx = None if n_context is None else torch.randn(2, n_context, 4, 4, device=dev)
    return m, x, ctx


def ref64(m, x, raw, direction):
    a, b = m._scale_shift()
    y, ld = coupling_ref(x.detach().double().cpu(), raw.detach().double().cpu(), a.detach().double().cpu(), b.detach().double().cpu(), direction)
    return y.numpy(), None if ld is None else ld.numpy()


def finite_fp32_grads(m, x):
    assert x.grad is not None and x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all())
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
    m.zero_grad()


@pytest.mark.parametrize("n_context", [None, 3])
def test_a_coupling_under_autocast_on_the_bf16_entry_points(n_context, dev, monkeypatch):
    from fincflow_amd import ops
    m, x, ctx = make_coupling(n_context, dev)
    names = record_entries(monkeypatch)
    gy, gl = torch.randn_like(x), torch.randn(2, device=dev)
    with autocast():
        raw = m._raw_train(x, ctx).detach()
        assert raw.dtype == torch.bfloat16 and raw.shape == x.shape
        # forward, recording
        xg = x.clone().requires_grad_(True)
        y, ld = m(xg, ctx)
        assert y.dtype == torch.float32 and ld.dtype == torch.float32
        assert coupling_calls(names) == ["finc_coupling_rawbf16_f32"], names
    y_ref, ld_ref = ref64(m, x, raw, 1)
    errs = {"y": rel_err(y.detach().cpu().numpy(), y_ref), "logdet": rel_err(ld.detach().cpu().numpy(), ld_ref)}
    ((y * gy).sum() + (ld * gl).sum()).backward()
    assert coupling_calls(names) == ["finc_coupling_rawbf16_f32", "finc_coupling_backward_rawbf16_f32"], names
    finite_fp32_grads(m, xg)
    # reverse and reverse_with_logdet inside reverse_grad(), recording
    r_ref, _ = ref64(m, x, raw, -1)
    rld_ref = ref64(m, torch.from_numpy(r_ref), raw, 1)[1]
    for with_logdet in (False, True):
        del names[:]
        xg = x.clone().requires_grad_(True)
        with autocast(), ops.reverse_grad():
            out = m.reverse_with_logdet(xg, ctx) if with_logdet else (m.reverse(xg, ctx), None)
        r, rld = out
        assert r.dtype == torch.float32 and r.requires_grad
        errs["reverse_grad%d" % with_logdet] = rel_err(r.detach().cpu().numpy(), r_ref)
        loss = (r * gy).sum()
        if with_logdet:
            assert rld.dtype == torch.float32
            errs["reverse_grad_logdet"] = rel_err(rld.detach().cpu().numpy(), rld_ref)
            loss = loss + (rld * gl).sum()
        loss.backward()
        want = (["finc_coupling_reverse_logdet_rawbf16_f32", "finc_coupling_reverse_logdet_backward_rawbf16_f32"] if with_logdet else
                ["finc_coupling_rawbf16_f32", "finc_coupling_reverse_backward_rawbf16_f32"])
        assert coupling_calls(names) == want, names
        finite_fp32_grads(m, xg)
    # the inference path: bias + ReLU in place on bf16, the transform on a bf16 raw
    del names[:]
    with torch.no_grad(), autocast():
        raw_inf = m._raw_inference(x, ctx)
        assert raw_inf.dtype == torch.bfloat16
        assert coupling_calls(names) == ["finc_bias_relu_bf16"] * 2, names
        del names[:]
        y, ld = m(x, ctx)
        r = m.reverse(x, ctx)
        r2, rld = m.reverse_with_logdet(x, ctx)
        back = m.reverse(y, ctx)
    assert coupling_calls(names) == (["finc_bias_relu_bf16"] * 2 + ["finc_coupling_rawbf16_f32"]) * 2 + \
        ["finc_bias_relu_bf16"] * 2 + ["finc_coupling_reverse_logdet_rawbf16_f32"] + ["finc_bias_relu_bf16"] * 2 + ["finc_coupling_rawbf16_f32"], names
    for t in (y, ld, r, r2, rld, back):
        assert t.dtype == torch.float32
    y_ref, ld_ref = ref64(m, x, raw_inf, 1)
    r_ref, _ = ref64(m, x, raw_inf, -1)
    errs.update(inf_y=rel_err(y.cpu().numpy(), y_ref), inf_logdet=rel_err(ld.cpu().numpy(), ld_ref), inf_reverse=rel_err(r.cpu().numpy(), r_ref),
                inf_reverse_logdet=rel_err(rld.cpu().numpy(), ref64(m, torch.from_numpy(r_ref), raw_inf, 1)[1]),
                round_trip=rel_err(back.cpu().numpy(), x.double().cpu().numpy()))
    assert same_bits(r, r2)
    print(n_context, errs)
    report("autocast_coupling", n_context=n_context, **errs)
    for n, e in errs.items():
        assert e <= TOL, (n, e)


def test_no_fp32_entry_point_and_no_cast_of_an_activation_behind_the_net(dev, monkeypatch):
    """One training step and one inference call under autocast, watched on the host side: the entry points by name, and every
    aten::_to_copy by the shape of its input -- none has the shape of `raw` [B,C,H,W] or of the hidden tensor [B,width,H,W]."""
    from torch.profiler import ProfilerActivity, profile
    m, x, ctx = make_coupling(None, dev)
    with autocast():                                                         # once before the watch: whatever the first convolutions set up
        m(x.clone().requires_grad_(True))[1].sum().backward()
    m.zero_grad()
    names = record_entries(monkeypatch)
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
        xg = x.clone().requires_grad_(True)
        with autocast():
            y, ld = m(xg)
        (y.square().sum() + ld.sum()).backward()
        with torch.no_grad(), autocast():
            m(x)
            m.reverse(x)
        torch.cuda.synchronize()
    assert len(coupling_calls(names)) == 8 and not any(n in F32_ENTRIES for n in names), names
    copies = [tuple(e.input_shapes[0]) for e in prof.events() if e.name == "aten::_to_copy" and e.input_shapes and e.input_shapes[0]]
    assert copies, "the watch saw no cast at all (the net's input and weights are cast by autocast)"
    assert (2, 4, 4, 4) not in copies and (2, 8, 4, 4) not in copies, copies


def alternative_off(monkeypatch):
    """The upcasting alternative: the coupling's HIP gate answers False, so the PyTorch formula runs on `raw.float()`."""
    from fincflow_amd import glow
    monkeypatch.setattr(glow.Coupling, "_hip_device", lambda self, x: False)


@pytest.mark.parametrize("n_context", [None, 3])
def test_gradients_against_the_upcasting_alternative(n_context, dev, monkeypatch):
    m, x, ctx = make_coupling(n_context, dev)
    gy, gl = torch.randn_like(x), torch.randn(2, device=dev)
    names = record_entries(monkeypatch)

    def grads():
        m.zero_grad()
        xg = x.clone().requires_grad_(True)
        with autocast():
            y, ld = m(xg, ctx)
        ((y * gy).sum() + (ld * gl).sum()).backward()
        return [("x", xg.grad.clone())] + [(n, p.grad.clone()) for n, p in m.named_parameters()], y.detach(), ld.detach()
    on, y_on, ld_on = grads()
    assert "finc_coupling_backward_rawbf16_f32" in names
    del names[:]
    alternative_off(monkeypatch)
    off, y_off, ld_off = grads()
    assert not coupling_calls(names), names
    errs = {"y": rel_err(y_on.cpu().numpy(), y_off.cpu().numpy()), "logdet": rel_err(ld_on.cpu().numpy(), ld_off.cpu().numpy())}
    for (n, g), (_, w) in zip(on, off):
        assert float(w.abs().max()) > 0, n
        errs["grad_" + n] = rel_err(g.cpu().numpy(), w.cpu().numpy())
    print(n_context, errs)
    report("autocast_against_upcast", n_context=n_context, bar=GRAD_BAR, **errs)
    for n, e in errs.items():
        assert e <= GRAD_BAR, (n, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# whole models
# ---------------------------------------------------------------------------------------------------------------------------------
def build(dev, preprocess, image_size=(3, 8, 8), num_blocks=2, block_size=2, split_prior=True):
    import numpy as np
    from fincflow_amd import glow
    torch.manual_seed(0)
    np.random.seed(0)
    model = glow.create_model(num_blocks=num_blocks, block_size=block_size, actnorm=True, split_prior=split_prior, image_size=image_size,
                              preprocess=preprocess, coupling_width=8)
    gen = torch.Generator().manual_seed(1)
    r = lambda shape, s: s * torch.randn(shape, generator=gen)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, glow.ActNorm):
                m.log_scale.copy_(r(m.log_scale.shape, 0.1))
                m.translation.copy_(r(m.translation.shape, 0.1))
                m.mark_initialized()
            elif isinstance(m, glow.Conv2dZero):
                for p in (m.weight, m.bias, m.logs):
                    p.copy_(r(p.shape, 0.05))
            elif isinstance(m, glow.Conv1x1):
                m.W.mul_(1.1).add_(r(m.W.shape, 0.05))
    return model.to(dev)


def test_one_adam_step_of_the_whole_model_under_autocast(dev, monkeypatch):
    model = build(dev, preprocess=True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    torch.manual_seed(2)
    x = torch.randint(0, 256, (4, 3, 8, 8), device=dev).float()
    before = [p.detach().clone() for p in model.parameters()]
    names = record_entries(monkeypatch)
    with autocast():
        loss = -model.log_prob(x).mean()
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert "finc_coupling_rawbf16_f32" in names and "finc_coupling_backward_rawbf16_f32" in names and not any(n in F32_ENTRIES for n in names)
    for (n, p), b in zip(model.named_parameters(), before):
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b), n


def test_sampling_and_log_prob_of_the_whole_model_under_autocast(dev, monkeypatch):
    model = build(dev, preprocess=False)
    fix_latents(model, 4, monkeypatch)
    names = record_entries(monkeypatch)
    with torch.no_grad(), autocast():
        x, x_true = model.sample(4)
        xs, log_q = model.sample_with_log_prob(4)
        lp = model.log_prob(xs)
    torch.cuda.synchronize()
    for t in (x, xs, log_q, lp):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert same_bits(x, xs)                                                  # the same latents, the same pass
    assert "finc_coupling_reverse_logdet_rawbf16_f32" in names and "finc_bias_relu_bf16" in names and not any(n in F32_ENTRIES for n in names)
    err = rel_err(log_q.cpu().numpy(), lp.cpu().numpy())
    print("log_q against log_prob of the same x under autocast: %.3e (bar %.0e)" % (err, CHAIN_TOL))
    report("autocast_chain", case="log_q_against_log_prob", err=err)
    assert err <= CHAIN_TOL, err
    # a reparameterised sample reaches every parameter
    del names[:]
    with autocast():
        xr, q = model.rsample_with_log_prob(4)
    assert xr.dtype == torch.float32 and q.dtype == torch.float32 and xr.requires_grad and q.requires_grad
    (q - xr.square().flatten(1).sum(1)).mean().backward()
    assert "finc_coupling_reverse_logdet_backward_rawbf16_f32" in names and not any(n in F32_ENTRIES for n in names)
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n


def test_invertible_backward_under_autocast_against_the_stored_path(dev, monkeypatch):
    """The run's backward executes where no autocast context is active; it rebuilds each coupling's input with `raw` from the net,
    which is only right in the forward's dtype.  Without the autocast state kept by the forward and entered again around the
    backward, the net would run in fp32 there and these gradients would be off at the 1e-2 level."""
    model = build(dev, preprocess=False)
    torch.manual_seed(5)
    x = torch.randn(4, 3, 8, 8, device=dev)
    names = record_entries(monkeypatch)

    def grads(invertible):
        model.invertible_backward = invertible
        model.zero_grad()
        with autocast():
            loss = -model.log_prob(x).mean()
        loss.backward()                                                      # outside the context, as a training loop has it
        return loss.detach(), [(n, p.grad.clone()) for n, p in model.named_parameters()]
    loss_s, stored = grads(False)
    assert "finc_coupling_backward_reconstruct_rawbf16_f32" not in names
    loss_i, inv = grads(True)
    assert "finc_coupling_backward_reconstruct_rawbf16_f32" in names and not any(n in F32_ENTRIES for n in names), names
    errs = {"loss": abs(float(loss_i) - float(loss_s)) / abs(float(loss_s))}
    for (n, g), (_, w) in zip(inv, stored):
        assert float(w.abs().max()) > 0, n
        errs[n] = rel_err(g.cpu().numpy(), w.cpu().numpy())
    worst = max(errs, key=errs.get)
    print("invertible_backward under autocast: worst of %d, %s %.3e (bar %.3e)" % (len(errs), worst, errs[worst], GRAD_BAR))
    report("autocast_invertible_backward", worst=worst, err=errs[worst], loss=errs["loss"], bar=GRAD_BAR)
    for n, e in errs.items():
        assert e <= GRAD_BAR, (n, e)


def test_a_channel_count_without_a_mix_kernel_stays_fp32_under_autocast(dev):
    """Conv1x1 at C = 20 has no finc_mix instantiation: its F.conv2d lines run with autocast off, so the next unit gets fp32."""
    from fincflow_amd import glow, ops
    assert not ops.mix_supported(20)
    model = build(dev, preprocess=False, image_size=(5, 4, 4), num_blocks=1, block_size=1, split_prior=False)
    mix = [m for m in model.modules() if isinstance(m, glow.Conv1x1)][0]
    torch.manual_seed(6)
    x = torch.randn(2, 5, 4, 4, device=dev)
    with torch.no_grad(), autocast():
        z, lp = model(x)
        s, _ = model.sample(2)
        h = torch.randn(2, 20, 2, 2, device=dev)
        assert mix(h)[0].dtype == torch.float32 and mix.reverse(h).dtype == torch.float32
    with autocast():
        assert mix(h.requires_grad_(True))[0].dtype == torch.float32
    for t in (z, lp, s):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())


def test_a_captured_sample_under_autocast_replays_with_the_bits_of_the_eager_call(dev, monkeypatch):
    from fincflow_amd import _lib
    model = build(dev, preprocess=False)
    fix_latents(model, 4, monkeypatch)
    # (autocast's weight cache off, as PyTorch's notes on graphs ask: a weight cast that the eager call cached would lie outside the
    # graph's memory pool and be freed when the context ends, under the graph's feet)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16, cache_enabled=False):
        x0, _ = model.sample(4)                                              # eager first: results to compare with, caches and workspace filled
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                                            # one stream, no parallel branches
            x, _ = model.sample(4)
    for _ in range(2):
        x.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(x, x0)
    assert not _lib.fault_pending()


def test_outside_autocast_only_the_fp32_entry_points_run(dev, monkeypatch):
    m, x, ctx = make_coupling(None, dev)
    names = record_entries(monkeypatch)
    xg = x.clone().requires_grad_(True)
    y, ld = m(xg)
    (y.square().sum() + ld.sum()).backward()
    with torch.no_grad():
        m(x)
    assert coupling_calls(names) == ["finc_coupling_f32", "finc_coupling_backward_f32", "finc_bias_relu_f32", "finc_bias_relu_f32", "finc_coupling_f32"]
