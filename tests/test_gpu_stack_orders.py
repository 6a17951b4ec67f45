"""`FlowSequential`'s folds and invertible runs over the layer orders of tests/stack_cases.py: the HIP model in every view its users
have -- `log_prob`, a training pass with stored activations and with `invertible_backward`, `sample`, `sample_with_log_prob`,
`rsample_with_log_prob`, `reconstruct` -- against the float64 CPU twin of tests/flow_twin.py (draws and the ReLUs' activation patterns
recorded and replayed as tests/test_gpu_train_loop.py does), and, for the named orders, the number of times every fold fired against
the numbers stated by hand there.  Every other test that drives the matcher builds `create_model`'s one order.

Bars: the project's own -- TOL (1e-5) for loss, log_prob and log_q, CHAIN_TOL (5e-5) for gradients, samples and reconstructions; a
gradient whose float64 reference is identically zero must be exactly zero, a frozen parameter's `.grad` stays None.  Every comparison
appends a line of kind `stack_orders` to the parity report, the float32 twin's own error beside the HIP one.
Worst over a run on an MI355X, HIP / yardstick: log_prob and loss 1.3e-7 / 1.3e-7; gradients 1.1e-6 / 7.6e-7 stored, 1.7e-5 / 7.6e-7
with `invertible_backward` (random_0_4, S S A K M M: a coupling at 192 channels on a 2x2 map; the named orders 1.5e-6); sample 5.1e-7 /
3.6e-7; sample_with_log_prob x 7.9e-6 / 4.4e-6, log_q 3.2e-7 / 1.1e-7; rsample_with_log_prob x 5.8e-7 / 3.5e-7, log_q 9.7e-8 / 9.9e-8,
gradients 1.2e-6 / 7.8e-7; reconstruct 1.2e-5 / 5.5e-6 (random_0_4 again).  The 43 tests take 12.5 s.

What the orders found (tests/test_stack_orders_host.py sees it without a GPU): `_forward_layers` summed the log-dets in place, and
`log_prob` raised on a stack whose first layer is a Conv1x1 (`reversed_block`).  profiles/stack_orders/mutations.txt: eight breaks of
the matcher, each made once and undone, and the tests here that went red.
"""
import pytest
import torch

import flow_twin
import stack_cases
from stack_cases import BATCH, CASES, UNITS, eligible_sites, resolved
from test_gpu_inverse_backward import CHAIN_TOL
from test_gpu_train_loop import TOL, Counter, Twins, on_device, placer, three
from test_stack_orders_host import RANDOM, capabilities, sampling_batch

pytestmark = pytest.mark.gpu

KIND = "stack_orders"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# counting
# ---------------------------------------------------------------------------------------------------------------------------------
class FoldCounter(Counter):
    """tests/test_gpu_train_loop.py's Counter plus spies of the same kind -- only a call that returns a result counts -- on the
    methods the reverse chain's matcher chooses between and on the invertible runs' node.  The twins are instances of the same
    classes: a call on a module (or an activation) that is not on the device is theirs and is not counted."""
    METHODS = (("Conv1x1", "reverse_then_affine"), ("Conv1x1", "reverse_premultiplied"), ("Conv1x1", "reverse"), ("ActNorm", "reverse"))

    def __init__(self, monkeypatch):
        from fincflow_amd import glow, layers
        super().__init__(monkeypatch)
        for cls, name in self.METHODS:
            fn = getattr(getattr(glow, cls), name)
            monkeypatch.setattr(getattr(glow, cls), name,
                                self._wrap_device("%s.%s" % (cls, name), fn, lambda args: next(args[0].parameters())))
        apply = layers._InvertibleRunFunction.apply
        monkeypatch.setattr(layers._InvertibleRunFunction, "apply",
                            staticmethod(self._wrap_device("_InvertibleRunFunction.apply", apply, lambda args: args[2])))

    def _wrap_device(self, name, fn, tensor_of):
        def counted(*args, **kwargs):
            out = fn(*args, **kwargs)
            if out is not None and tensor_of(args).is_cuda:
                self.n[name] = self.n.get(name, 0) + 1
            return out
        return counted


def folds(k):
    """What one pass fired, in the words of tests/stack_cases.py."""
    assert k.get("Conv1x1.reverse_premultiplied", 0) == k.get("cache.inverse_premultiplied", 0), k     # R2 is the two together
    return dict(F=k.get("cache.forward_affine", 0), R1=k.get("cache.inverse_affine", 0), R2=k.get("cache.inverse_premultiplied", 0),
                R3=k.get("Conv1x1.reverse_then_affine", 0), mix_reverse=k.get("Conv1x1.reverse", 0),
                actnorm_reverse=k.get("ActNorm.reverse", 0), inverse=k.get("cache.inverse", 0),
                nodes=k.get("_InvertibleRunFunction.apply", 0))


REVERSE = ("R1", "R2", "R3", "mix_reverse", "actnorm_reverse", "inverse")


def layer_counts(case):
    codes = resolved(case["layers"])
    return dict(mixes=codes.count("M"), actnorms=codes.count("A"), couplings=sum(c in ("K", "Kc", "Z") for c in codes),
                solves=sum(c in UNITS or c == "X" or c.startswith("P:") for c in codes))


def unfolded(case):
    """A reverse pass that folds nothing: every layer's own reverse."""
    c = layer_counts(case)
    return dict(R1=0, R2=0, R3=0, mix_reverse=c["mixes"], actnorm_reverse=c["actnorms"], inverse=c["solves"])


class Run:
    """One case on the device: the model, its twins, its inputs, the counter (None: parity only) and what its passes fired."""

    def __init__(self, name, case, dev, counter):
        self.name, self.case, self.counter = name, case, counter
        model = stack_cases.build(case)
        self.model = model.to(dev)
        self.twins = Twins(self.model)
        self.n = sampling_batch(case)                      # of the reverse passes without a graph; everything else runs BATCH images
        self.pick = None if self.n == BATCH else [0, self.n // 3, 2 * self.n // 3, self.n - 1]
        self.x, self.ctx = stack_cases.inputs(case, self.n)
        self.expect = stack_cases.expected(case, capabilities(case)) if "expect" in case else None
        self.fired = dict(F=0, R1=0, R2=0, R3=0)

    def few(self, t):
        """The images every pass under autograd and every `log_prob` evaluates (the twin: of every pass)."""
        return None if t is None else (t if self.pick is None else t[self.pick])

    def mine(self, m, t):
        """`t` for the HIP model, its picked images for a twin."""
        return t if m is self.model else self.few(t)

    def judge(self, tag, names, got, want, yard, bar):
        return flow_twin.compare("%s/%s" % (self.name, tag), names, got, want, yard, bar=bar, kind=KIND, view=tag,
                                 order=" ".join(self.case["layers"]))

    def take(self, want=None, keys=None):
        """The counts since the last call; with `want`, asserts the entries `keys` of it."""
        if self.counter is None:
            return {}
        k = self.counter.take()
        got = folds(k)
        for kind in self.fired:
            self.fired[kind] += got[kind]
        if want is not None and self.expect is not None:
            assert {n: got[n] for n in keys} == {n: want[n] for n in keys}, (self.name, self.case["layers"], got, k)
        return k

    def fuse(self, on):
        if on:
            self.model.__dict__.pop("fuse_affine", None)
        else:
            self.model.fuse_affine = False


# ---------------------------------------------------------------------------------------------------------------------------------
# the views
# ---------------------------------------------------------------------------------------------------------------------------------
def view_log_prob(r):
    x, ctx = r.few(r.x), r.few(r.ctx)

    def fn(m, put):
        with torch.no_grad():
            return [m.log_prob(put(x), None if ctx is None else put(ctx))]
    for fused in (True, False):
        r.fuse(fused)
        r.take()
        got, want, yard, _ = three(r.model, r.twins, fn)
        r.take(dict(F=r.expect["F"] if fused else 0, nodes=0) if r.expect else None, ("F", "nodes"))
        r.judge("log_prob" if fused else "log_prob_unfused", ["log_prob"], got, want, yard, TOL)
    r.fuse(True)


def training_pass(r, m, invertible, input_grad=True):
    """[loss, log_prob, (x.grad, (context.grad))] of `log_prob(x).mean().backward()`; the parameters' gradients stay in `.grad`."""
    put = placer(m)
    x = put(r.few(r.x)).requires_grad_(input_grad)
    ctx = None if r.ctx is None else put(r.few(r.ctx)).requires_grad_(input_grad)
    m.zero_grad(set_to_none=True)
    if on_device(m):
        m.invertible_backward = invertible
    lp = m.log_prob(x, ctx)
    loss = lp.mean()
    loss.backward()
    if on_device(m):
        del m.invertible_backward
    else:
        flow_twin.mask_unit_grads(m)
    return [loss.detach(), lp.detach()] + ([x.grad] + ([] if ctx is None else [ctx.grad]) if input_grad else [])


def judge_grads(r, tag, extra_names, extra):
    """Every parameter's `.grad` of the three models and the activations' gradients `extra` = (got, want, yard)."""
    named = lambda m: {n: p.grad for n, p in m.named_parameters()}
    g, w, y = named(r.model), named(r.twins.t64), named(r.twins.t32)
    frozen = [n for n, p in r.model.named_parameters() if not p.requires_grad]
    assert [n for n in g if g[n] is None] == [n for n in w if w[n] is None] == frozen, "`.grad is None` differs from the twin's or the frozen set"
    names = [n for n in g if g[n] is not None]
    for n, mask in flow_twin.stored_masks(r.model).items():
        assert g[n] is None or not bool(g[n].cpu()[mask == 0].any()), "%s: a gradient under the corner-tap mask is not zero" % n
    r.judge(tag, names + extra_names, [g[n] for n in names] + extra[0], [w[n] for n in names] + extra[1], [y[n] for n in names] + extra[2],
            CHAIN_TOL)


def view_backward(r, invertible):
    tag = "backward_invertible" if invertible else "backward_stored"
    r.take()
    got, want, yard, _ = three(r.model, r.twins, lambda m, put: training_pass(r, m, invertible))
    k = r.take(dict(F=r.expect["F_runs"] if invertible else 0, nodes=r.expect["nodes"] if invertible else 0) if r.expect else None,
               ("F", "nodes"))
    r.judge(tag + "/loss", ["loss", "log_prob"], got[:2], want[:2], yard[:2], TOL)
    judge_grads(r, tag + "/grads", ["input", "context"][:len(got) - 2], (got[2:], want[2:], yard[2:]))
    return k


def view_sample(r):
    def fn(m, put):
        with torch.no_grad():
            x, x_true = m.sample(r.n if m is r.model else BATCH, None if r.ctx is None else put(r.mine(m, r.ctx)))
            assert x_true is x
            return [x]
    for fused in (True, False):
        r.fuse(fused)
        r.take()
        got, want, yard, _ = three(r.model, r.twins, fn, r.pick)
        r.take(r.expect if fused else unfolded(r.case), REVERSE)
        r.judge("sample" if fused else "sample_unfused", ["x"], [r.few(got[0])], want, yard, CHAIN_TOL)
    r.fuse(True)


def view_sample_with_log_prob(r):
    """x against the twin's reverse on the replayed draws; log_q against the twin's `log_prob` at the HIP model's x and against the
    twin's own log_q."""
    def fn(m, put):
        return list(m.sample_with_log_prob(r.n if m is r.model else BATCH, None if r.ctx is None else put(r.mine(m, r.ctx))))
    r.take()
    got, want, yard, _ = three(r.model, r.twins, fn, r.pick)
    k = r.take(r.expect, REVERSE)
    if r.expect:
        assert k.get("finc_coupling_reverse_logdet", 0) == layer_counts(r.case)["couplings"], k
    assert not got[0].requires_grad and not got[1].requires_grad
    got = [r.few(g) for g in got]
    r.judge("sample_with_log_prob/x", ["x"], got[:1], want[:1], yard[:1], CHAIN_TOL)
    x = got[0].cpu()
    with torch.no_grad():
        lq64, lq32 = (tw.log_prob(placer(tw)(x), None if r.ctx is None else placer(tw)(r.few(r.ctx))) for tw in r.twins)
    r.judge("sample_with_log_prob/log_q", ["log_q", "log_q_replayed"], [got[1], got[1]], [lq64, want[1]], [lq32, yard[1]], TOL)


def view_rsample_with_log_prob(r):
    def fn(m, put):
        m.zero_grad(set_to_none=True)
        x, log_q = m.rsample_with_log_prob(BATCH, None if r.ctx is None else put(r.few(r.ctx)))
        assert x.requires_grad and log_q.requires_grad
        (log_q - x.square().flatten(1).sum(1)).mean().backward()
        if not on_device(m):
            flow_twin.mask_unit_grads(m)
        return [x.detach(), log_q.detach()]
    r.take()
    got, want, yard, _ = three(r.model, r.twins, fn)
    k = r.take(unfolded(r.case), ("R1", "R2", "R3", "mix_reverse", "actnorm_reverse"))       # a recorded chain folds nothing
    if r.expect:
        # (every unit solves once: `ops.inverse_reverse` where the chain is recorded by then, and that one goes through the cache too)
        assert k.get("inverse_reverse", 0) <= k.get("cache.inverse", 0) == layer_counts(r.case)["solves"], k
    r.judge("rsample_with_log_prob/x", ["x"], got[:1], want[:1], yard[:1], CHAIN_TOL)
    r.judge("rsample_with_log_prob/log_q", ["log_q"], got[1:], want[1:], yard[1:], TOL)
    judge_grads(r, "rsample_with_log_prob/grads", [], ([], [], []))


def view_reconstruct(r):
    def fn(m, put):
        with torch.no_grad():
            return [m.reconstruct(put(r.mine(m, r.x)), None if r.ctx is None else put(r.mine(m, r.ctx)))]
    r.take()
    got, want, yard, _ = three(r.model, r.twins, fn, r.pick)
    r.take(r.expect, ("F",) + REVERSE)
    r.judge("reconstruct", ["x"], [r.few(got[0])], want, yard, CHAIN_TOL)


# ---------------------------------------------------------------------------------------------------------------------------------
# the named orders: parity and the hand-stated counts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_a_named_order_against_the_twin_and_its_fold_counts(name, dev, monkeypatch):
    r = Run(name, CASES[name], dev, FoldCounter(monkeypatch))
    view_log_prob(r)
    view_backward(r, invertible=False)
    view_backward(r, invertible=True)
    view_sample(r)
    view_sample_with_log_prob(r)
    view_rsample_with_log_prob(r)
    view_reconstruct(r)


def test_the_walk_stops_in_front_of_a_frozen_prefix(dev, monkeypatch):
    """`frozen_prefix` with an input that wants no gradient: nothing in front of the fifth layer wants one, so the node's backward
    differentiates the four trainable layers and rebuilds nothing further -- one unit solved (the fifth layer's input, for its
    weight gradient), one mix undone (the seventh layer's), the frozen four untouched."""
    r = Run("frozen_prefix", CASES["frozen_prefix"], dev, FoldCounter(monkeypatch))
    calls = []
    for k, m in enumerate(r.model):
        monkeypatch.setattr(m, "backward_from_output", lambda *a, _k=k, _f=m.backward_from_output: (calls.append(_k), _f(*a))[1])
    got, want, yard, _ = three(r.model, r.twins, lambda m, put: training_pass(r, m, True, input_grad=False))
    k = r.counter.take()
    assert calls == [7, 6, 5, 4], calls
    assert k.get("_InvertibleRunFunction.apply") == 1 and k.get("cache.inverse") == 1 and k.get("cache.forward_affine") == 2, k
    assert k.get("finc_mix") == 3, k                                   # both mixes in the run's forward, the seventh layer's on the way back
    r.judge("backward_invertible_no_input_grad/loss", ["loss", "log_prob"], got, want, yard, TOL)
    judge_grads(r, "backward_invertible_no_input_grad/grads", [], ([], [], []))


# ---------------------------------------------------------------------------------------------------------------------------------
# the random orders: parity, and no more folds than sites
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RANDOM))
def test_a_random_order_against_the_twin(name, dev, monkeypatch):
    from helpers import report
    case = RANDOM[name]
    r = Run(name, case, dev, FoldCounter(monkeypatch))
    sites = eligible_sites(case["layers"])
    passes = 0
    for view, n in ((view_log_prob, 1), (lambda r: view_backward(r, False), 0), (lambda r: view_backward(r, True), 1),
                    (view_sample_with_log_prob, 1), (view_reconstruct, 1)):
        before = dict(r.fired)
        view(r)
        r.take()
        assert all(r.fired[k] - before[k] <= n * sites[k] for k in sites), (name, case["layers"], view, before, r.fired, sites)
        passes += n
    print("%s %s: fired %s over %d folding passes, sites per pass %s" % (name, case["layers"], r.fired, passes, sites))
    report(KIND, case=name + "/folds", order=" ".join(case["layers"]), fired=r.fired, eligible=sites, passes=passes)
