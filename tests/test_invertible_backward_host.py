"""Host side of training without stored activations (FlowSequential.invertible_backward; include/finc.h:
finc_actnorm_backward_reconstruct_f32, finc_coupling_backward_reconstruct_f32): the exported symbols and the sixth ABI
version gate, argument refusals before any HIP call, the new kernels' register allocation, the rule that cuts a stack into runs, and
the autograd node of a run on layers that implement the protocol in plain PyTorch -- no GPU needed, the library built."""
import os

import numpy as np
import pytest
import torch

from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library, rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("finc_actnorm_backward_reconstruct_f32", "finc_coupling_backward_reconstruct_f32")
DIMS_BAD = ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64), (1 << 20, 4096, 1 << 20))


def test_new_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
        assert getattr(L, name).argtypes is not None, name
    assert "layers/coupling.py:79-92" in header and "layers/actnorm.py:51" in header      # the reference lines of the two formulas
    from fincflow_amd import ops
    for name in ("finc_actnorm_backward_reconstruct", "finc_coupling_backward_reconstruct"):
        assert callable(getattr(ops, name)), name


def test_version_is_110_and_a_109_library_is_refused_by_name(tmp_path):
    assert _lib.lib().finc_version() >= _lib.INVERTIBLE_BACKWARD_ABI_VERSION == 110
    assert _lib.ABI_VERSION == 104 and _lib.ACTNORM_ABI_VERSION == 105 and _lib.INVERSE_BACKWARD_ABI_VERSION == 107
    assert _lib.REVERSE_BACKWARD_ABI_VERSION == 108 and _lib.SAMPLE_LOGDET_ABI_VERSION == 109
    out = load_stub_library(tmp_path, 109)
    assert "= 109" in out and "110" in out, out
    for name in NEW_SYMBOLS:
        assert name in out, out


def test_actnorm_reconstruct_status_codes_without_touching_the_gpu():
    """NULL -> 1, bad dims / forbidden aliasing -> 2, alignment below 4 bytes -> 7, workspace -> 4, in that order of precedence, with
    fake pointers: nothing is launched.  Allowed aliasing (x_out == y, grad_x == grad_y) passes every check up to the workspace."""
    L = _lib.lib()
    gy, gl, y, ls, tr = _p(0x1000), _p(0x1800), _p(0x2000), _p(0x3000), _p(0x4000)
    xo, gx, gls, gt, ws = _p(0x5000), _p(0x6000), _p(0x7000), _p(0x8000), _p(0x10000)
    big = 1 << 40
    f = L.finc_actnorm_backward_reconstruct_f32
    for k in (0, 2, 3):                                                      # grad_y, y, log_scale are required; grad_logdet is not
        args = [gy, gl, y, ls, tr]
        args[k] = None
        assert f(*args, xo, gx, gls, gt, 2, 12, 64, ws, big, None) == 1, k
    assert f(gy, gl, y, ls, None, xo, gx, gls, gt, 2, 12, 64, ws, big, None) == 1          # x_out reads the translation
    assert f(gy, gl, y, ls, tr, None, None, None, None, 2, 12, 64, ws, big, None) == 1     # nothing asked for
    assert f(None, gl, y, ls, tr, xo, gx, gls, gt, 0, 12, 64, ws, big, None) == 1          # (NULL comes before the dims)
    for B, C, HW in DIMS_BAD:
        assert f(gy, gl, y, ls, tr, xo, gx, gls, gt, B, C, HW, ws, big, None) == 2, (B, C, HW)
        assert f(gy, None, y, ls, tr, xo, None, None, None, B, C, HW, None, 0, None) == 2, (B, C, HW)
    assert f(gy, gl, y, ls, tr, gy, gx, gls, gt, 2, 12, 64, ws, big, None) == 2            # x_out on grad_y
    assert f(gy, gl, y, ls, tr, xo, xo, gls, gt, 2, 12, 64, ws, big, None) == 2            # x_out == grad_x
    assert f(gy, gl, y, ls, tr, xo, y, gls, gt, 2, 12, 64, ws, big, None) == 2             # grad_x on y
    assert f(gy, gl, y, ls, tr, y, y, gls, gt, 2, 12, 64, ws, big, None) == 2
    assert f(_p(0x1002), gl, y, ls, tr, xo, y, gls, gt, 2, 12, 64, ws, big, None) == 2     # (aliasing comes before the alignment)
    assert f(_p(0x1002), gl, y, ls, tr, xo, gx, gls, gt, 0, 12, 64, ws, big, None) == 2    # (dims come before the alignment)
    for k in range(9):
        args = [gy, gl, y, ls, tr, xo, gx, gls, gt]
        args[k] = _p(args[k].value + 2)
        assert f(*args, 2, 12, 64, None, 0, None) == 7, k                                  # (alignment before the workspace)
    need = L.finc_actnorm_workspace_bytes(2, 7, 15)
    assert f(gy, gl, y, ls, tr, xo, gx, gls, gt, 2, 7, 15, None, big, None) == 4           # (any C >= 1: odd is fine)
    assert f(gy, gl, y, ls, tr, xo, gx, gls, gt, 2, 7, 15, ws, need - 1, None) == 4
    assert f(gy, None, y, ls, tr, None, None, None, gt, 2, 7, 15, ws, 0, None) == 4
    assert f(gy, gl, y, ls, tr, xo, gx, gls, gt, 2, 7, 15, _p(0x10002), big, None) == 4
    assert f(gy, gl, y, ls, tr, y, gy, gls, gt, 2, 7, 15, ws, need - 1, None) == 4         # both in-place forms pass the aliasing rule


def test_coupling_reconstruct_status_codes_without_touching_the_gpu():
    """As above, with odd C -> 3 between the alignment and the workspace."""
    L = _lib.lib()
    gy, gl, y, raw, a, b = _p(0x1000), _p(0x1800), _p(0x2000), _p(0x3000), _p(0x4000), _p(0x5000)
    xo, gx, gr, ga, gb, ws = _p(0x5800), _p(0x6000), _p(0x7000), _p(0x8000), _p(0x9000), _p(0x10000)
    big = 1 << 40
    f = L.finc_coupling_backward_reconstruct_f32
    for k in (0, 2, 3, 4, 5):                                                # grad_y, y, raw, a, b are required; grad_logdet is not
        args = [gy, gl, y, raw, a, b]
        args[k] = None
        assert f(*args, xo, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 1, k
    assert f(gy, gl, y, raw, a, b, None, None, None, None, None, 2, 12, 64, ws, big, None) == 1    # nothing asked for
    assert f(None, gl, y, raw, a, b, xo, gx, gr, ga, gb, 0, 12, 64, ws, big, None) == 1            # (NULL comes before the dims)
    for B, C, HW in DIMS_BAD:
        assert f(gy, gl, y, raw, a, b, xo, gx, gr, ga, gb, B, C, HW, ws, big, None) == 2, (B, C, HW)
        assert f(gy, None, y, raw, a, b, xo, None, None, None, None, B, C, HW, None, 0, None) == 2, (B, C, HW)
    for alias in (gy, raw, gx, gr):
        assert f(gy, gl, y, raw, a, b, alias, gx, gr, ga, gb, 2, 12, 64, ws, big, None) == 2       # x_out anywhere but on y
    for alias in (y, raw, xo, gr):
        assert f(gy, gl, y, raw, a, b, xo, alias, gr, ga, gb, 2, 12, 64, ws, big, None) == 2       # grad_x anywhere but on grad_y
    for alias in (gy, y, raw, xo, gx):
        assert f(gy, gl, y, raw, a, b, xo, gx, alias, ga, gb, 2, 12, 64, ws, big, None) == 2       # grad_raw on anything
    assert f(_p(0x1002), gl, y, raw, a, b, xo, y, gr, ga, gb, 2, 12, 64, ws, big, None) == 2       # (aliasing before the alignment)
    assert f(_p(0x1002), gl, y, raw, a, b, xo, gx, gr, ga, gb, 0, 12, 64, ws, big, None) == 2      # (dims before the alignment)
    for k in range(11):
        args = [gy, gl, y, raw, a, b, xo, gx, gr, ga, gb]
        args[k] = _p(args[k].value + 2)
        assert f(*args, 2, 12, 64, None, 0, None) == 7, k                                          # (alignment before the workspace)
    assert f(_p(0x1002), gl, y, raw, a, b, xo, gx, gr, ga, gb, 2, 13, 64, ws, big, None) == 7      # (... and before the channel count)
    for C in (13, 7, 1):
        assert f(gy, gl, y, raw, a, b, xo, gx, gr, ga, gb, 2, C, 64, ws, big, None) == 3, C
        assert f(gy, None, y, raw, a, b, xo, None, None, None, None, 2, C, 64, None, 0, None) == 3, C
    need = L.finc_coupling_workspace_bytes(2, 12, 64)
    assert f(gy, gl, y, raw, a, b, xo, gx, gr, ga, gb, 2, 12, 64, None, big, None) == 4
    assert f(gy, gl, y, raw, a, b, xo, gx, gr, ga, gb, 2, 12, 64, ws, need - 1, None) == 4
    assert f(gy, None, y, raw, a, b, None, None, None, ga, None, 2, 12, 64, ws, 0, None) == 4
    assert f(gy, gl, y, raw, a, b, None, None, None, None, gb, 2, 12, 64, None, 0, None) == 4
    assert f(gy, gl, y, raw, a, b, xo, gx, gr, ga, gb, 2, 12, 64, _p(0x10002), big, None) == 4
    assert f(gy, gl, y, raw, a, b, y, gy, gr, ga, gb, 2, 12, 64, ws, need - 1, None) == 4          # both in-place forms pass


def test_new_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    for name in ("finc_actnorm_recon_kernel", "finc_coupling_recon_kernel"):
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == 2, (name, sorted(ks))                             # the 16-byte and the dword form
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cut rule, on models built on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_counts_as_device(monkeypatch):
    """The layers' own `invertible_backward_supported`, with a float32 4-D CPU tensor standing in for a device tensor (for tests
    that only ask: a forward would take the HIP path)."""
    from fincflow_amd import glow, layers
    stand_in = lambda x: x.dtype == torch.float32 and x.dim() == 4
    monkeypatch.setattr(layers, "_hip_tensor", stand_in)
    monkeypatch.setattr(glow, "_hip_tensor", stand_in)


@pytest.fixture
def supported_patched(monkeypatch):
    """`invertible_backward_supported` of the glow layers replaced by the part of their rule a CPU model can run with: float32,
    4-D, and for ActNorm initialised."""
    from fincflow_amd import glow
    ok = lambda self, x, context=None: x.dtype == torch.float32 and x.dim() == 4
    for cls in (glow.Squeeze, glow.Conv1x1, glow.Coupling):
        monkeypatch.setattr(cls, "invertible_backward_supported", ok)
    monkeypatch.setattr(glow.ActNorm, "invertible_backward_supported", lambda self, x, context=None: self._is_initialized() and ok(self, x))


def _foreign_layer():
    from fincflow_amd.layers import FlowLayer

    class Foreign(FlowLayer):                                   # a layer from elsewhere: the base class's "not supported"
        def forward(self, input, context=None):
            return input * 2.0, input.new_full((len(input),), float(np.log(2.0) * input[0].numel()))

        def reverse(self, input, context=None):
            return input / 2.0

        def logdet(self, input, context=None):
            return self.forward(input, context)[1]
    return Foreign()


def _stack():
    """Squeeze ActNorm Conv1x1 Coupling | SplitPrior | ActNorm(uninitialised) | Conv1x1 Coupling | Foreign | Conv1x1 | Foreign"""
    from fincflow_amd import FlowSequential, glow
    torch.manual_seed(2)
    np.random.seed(2)
    first = glow.ActNorm(16)
    first.mark_initialized()
    mods = [glow.Squeeze(), first, glow.Conv1x1(16), glow.Coupling((16, 4, 4), width=8),
            glow.SplitPrior((16, 4, 4), glow.GaussianPrior, width=8),
            glow.ActNorm(8), glow.Conv1x1(8), glow.Coupling((8, 4, 4), width=8),
            _foreign_layer(), glow.Conv1x1(8), _foreign_layer()]
    return FlowSequential(glow.GaussianPrior((8, 4, 4)), *mods)


def test_a_split_prior_an_uninitialised_actnorm_and_a_foreign_layer_each_end_a_run(cpu_counts_as_device):
    model = _stack()
    mods = list(model.sequence_modules)
    x = torch.randn(3, 4, 8, 8)
    end = lambda i, t: model._invertible_run_end(mods, i, t, None)
    assert end(0, x) == 4                                        # Squeeze .. Coupling, judged at the squeezed shape; SplitPrior ends it
    h = torch.randn(3, 8, 4, 4)
    assert end(4, torch.randn(3, 16, 4, 4)) == 4                 # SplitPrior itself: no run
    assert end(5, h) == 5                                        # the ActNorm that still has to initialise: no run
    assert end(6, h) == 8 and end(8, h) == 8 and end(9, h) == 10 and end(10, h) == 10
    mods[5].mark_initialized()
    assert end(5, h) == 8                                        # initialised: the run starts one layer earlier
    assert end(0, x.double()) == 0 and end(0, x[0]) == 0         # fp64 and 3-D tensors are never supported
    assert end(1, x) == 1                                        # (16 channels expected, 4 given: ActNorm says no)


def test_runs_of_two_or_more_are_wrapped_and_a_run_of_one_is_not(supported_patched, monkeypatch):
    from fincflow_amd import layers
    model = _stack()
    mods = list(model.sequence_modules)
    wrapped = []

    class Recorder:
        @staticmethod
        def apply(seq, run, x, context, *params):
            wrapped.append((run, params))
            pass
            return seq._forward_layers(list(run), x, context, x.new_zeros(len(x)))
    monkeypatch.setattr(layers, "_InvertibleRunFunction", Recorder)
    x = torch.randn(3, 4, 8, 8)
    want = model.log_prob(x)                                     # off: no run is built
    assert not wrapped
    model.invertible_backward = True
    with torch.no_grad():
        assert torch.equal(model.log_prob(x), want) and not wrapped          # nothing is recorded: no run either
    mods[5].reset_initialization()
    got = model.log_prob(x)
    # the first call initialises the second ActNorm on the stored path, so its run starts behind it
    assert [tuple(mods.index(m) for m in run) for run, _ in wrapped] == [(0, 1, 2, 3), (6, 7)]
    assert [len(p) for _, p in wrapped] == [sum(len(list(mods[i].parameters())) for i in r) for r in ((0, 1, 2, 3), (6, 7))]
    assert rel_err(got.detach().numpy(), want.detach().numpy()) <= 1e-6
    del wrapped[:]
    model.log_prob(x)                                            # the next call: the ActNorm is initialised and joins its run
    assert [tuple(mods.index(m) for m in run) for run, _ in wrapped] == [(0, 1, 2, 3), (5, 6, 7)]
    del wrapped[:]
    for p in model.parameters():
        p.requires_grad_(False)
    model.log_prob(x)                                            # grad enabled, nothing to differentiate: no run
    assert not wrapped
    model.log_prob(x.requires_grad_(True))
    assert len(wrapped) == 2


def test_with_the_attribute_off_forward_calls_no_new_code(monkeypatch):
    from fincflow_amd import FastFlowUnit, FlowSequential, PaddedConv2d, glow, layers

    def boom(*a, **k):
        raise AssertionError("new code reached with invertible_backward off")
    assert FlowSequential.invertible_backward is False
    monkeypatch.setattr(FlowSequential, "_forward_invertible", boom)
    monkeypatch.setattr(FlowSequential, "_invertible_run_end", boom)
    monkeypatch.setattr(layers._InvertibleRunFunction, "apply", boom)
    for cls in (layers.FlowLayer, PaddedConv2d, FastFlowUnit, glow.Squeeze, glow.ActNorm, glow.Conv1x1, glow.Coupling):
        monkeypatch.setattr(cls, "invertible_backward_supported", boom)
        monkeypatch.setattr(cls, "backward_from_output", boom)
    model = _stack()
    x = torch.randn(3, 4, 8, 8, requires_grad=True)
    model.log_prob(x).mean().backward()
    assert x.grad is not None and all(p.grad is not None for p in model.parameters())


def test_cpu_and_fp64_tensors_keep_the_stored_path_bit_for_bit():
    model = _stack()
    x = torch.randn(3, 4, 8, 8)
    with torch.no_grad():
        model(x)                                                 # (initialises)
    off = model.log_prob(x)
    off.mean().backward()
    grads = [p.grad.clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)
    model.invertible_backward = True
    on = model.log_prob(x)
    assert "InvertibleRun" not in _graph_names(on)
    on.mean().backward()
    assert torch.equal(on, off) and all(torch.equal(p.grad, g) for p, g in zip(model.parameters(), grads))


def _graph_names(t):
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo += [f for f, _ in fn.next_functions]
    return " ".join(names)


# ---------------------------------------------------------------------------------------------------------------------------------
# the run's autograd node, on layers that implement the protocol in PyTorch
# ---------------------------------------------------------------------------------------------------------------------------------
def _toy_layers():
    from fincflow_amd.layers import FlowLayer, _param_needs

    class Scale(FlowLayer):
        """y = x * exp(s[c]) + t[c] (context: + k * context); log-det = H W sum s."""
        def __init__(self, C, uses_context=False):
            super().__init__()
            self.s = torch.nn.Parameter(0.3 * torch.randn(C))
            self.t = torch.nn.Parameter(torch.randn(C))
            self.k = torch.nn.Parameter(torch.randn(())) if uses_context else None
            self.asked = []

        def forward(self, x, context=None):
            y = x * torch.exp(self.s).view(1, -1, 1, 1) + self.t.view(1, -1, 1, 1)
            if self.k is not None:
                y = y + self.k * context
            return y, (self.s.sum() * x.shape[2] * x.shape[3]).expand(len(x))

        def reverse(self, y, context=None):
            if self.k is not None:
                y = y - self.k * context
            return (y - self.t.view(1, -1, 1, 1)) * torch.exp(-self.s).view(1, -1, 1, 1)

        def logdet(self, x, context=None):
            return self.forward(x, context)[1]

        def invertible_backward_supported(self, x, context=None):
            return x.dim() == 4

        def backward_from_output(self, output, grad_output, grad_logdet, context, needs):
            self.asked.append(needs)
            params, asked = _param_needs(self, needs)
            with torch.no_grad():
                x = self.reverse(output, context)
            with torch.enable_grad():
                xin = x.detach().requires_grad_(True)
                ctx = None if context is None else context.detach().requires_grad_(True)
                y, ld = self.forward(xin, ctx)
                wanted = [xin] + ([ctx] if ctx is not None else []) + [p for p, a in zip(params, asked) if a]
                g = list(torch.autograd.grad([y, ld], wanted, [grad_output, grad_logdet], allow_unused=True))
            gx = g.pop(0)
            gc = g.pop(0) if ctx is not None else None
            return (x if needs.input else None, gx if needs.grad_input else None, gc if needs.grad_context else None,
                    [g.pop(0) if a else None for a in asked])
    return Scale


def test_the_run_node_walks_back_to_front_and_matches_the_stored_path():
    from fincflow_amd import FlowSequential, glow
    torch.manual_seed(5)
    Scale = _toy_layers()
    mods = [Scale(4).double(), Scale(4, True).double(), Scale(4).double()]
    mods[1].t.requires_grad_(False)                              # a frozen parameter in the middle
    model = FlowSequential(glow.GaussianPrior((4, 3, 2)), *mods).double()
    x = torch.randn(5, 4, 3, 2, dtype=torch.float64, requires_grad=True)
    c = torch.randn(5, 4, 3, 2, dtype=torch.float64, requires_grad=True)
    leaves = [x, c] + [p for p in model.parameters() if p.requires_grad]
    want = torch.autograd.grad(model.log_prob(x, c).square().sum(), leaves)
    assert not any(m.asked for m in mods)
    model.invertible_backward = True
    lp = model.log_prob(x, c)
    assert "_InvertibleRunFunction" in _graph_names(lp)
    loss = lp.square().sum()
    got = torch.autograd.grad(loss, leaves, retain_graph=True)
    again = torch.autograd.grad(loss, leaves)                    # the saved output is never written: a second backward is the first
    for g, a, w in zip(got, again, want):
        assert torch.equal(g, a) and rel_err(g.numpy(), w.numpy()) <= 1e-12
    assert [len(m.asked) for m in mods] == [2, 2, 2]
    assert mods[2].asked[0] == (True, True, True, (True, True)) and mods[0].asked[0] == (False, True, True, (True, True))
    assert mods[1].asked[0].params == (True, False, True)        # Scale.parameters(): s, t (frozen), k
    # the frozen parameter got no gradient, and an input that needs none asks the first layer for none
    for m in mods:
        del m.asked[:]
    model.log_prob(x.detach(), c.detach()).sum().backward()
    assert mods[1].t.grad is None and mods[1].s.grad is not None
    assert mods[0].asked[0][:3] == (False, False, False) and mods[1].asked[0][:3] == (True, True, False)
    # only the last layer trainable: the walk stops there
    for m in mods:
        del m.asked[:]
    for p in list(mods[0].parameters()) + list(mods[1].parameters()):
        p.requires_grad_(False)
    model.log_prob(x.detach(), c.detach()).sum().backward()
    assert [len(m.asked) for m in mods] == [0, 0, 1] and mods[2].asked[0][:3] == (False, False, False)
