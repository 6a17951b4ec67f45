"""The host-side caches of values derived from parameters, built on one stream and used on another (`ops.Ready`).

Every case is the same deterministic construction, no luck and no repetition:

  prime      everything upstream of the cache under test runs on the default stream, then the device is synchronised -- the invariant
             check (a device->host copy) and `torch.inverse` (an info word) synchronise the host and would swallow the delay below, so
             the bank is validated through ANOTHER kind of call and W^-1 is built beforehand; then only what invalidates the one
             cache under test changes (new weights, new ActNorm parameters, new Conv2dZero parameters);
  produce    on a side stream s1: a delay (`torch.cuda._sleep`, or a chain of matrix products), an event `done` right behind it, and
             the call that builds the cache;
  consume    on a side stream s2, at once: the same kind of call on other input -- a cache hit;
  non-vacuity  `done` has not completed when the consumer is queued: the fill launch behind the delay cannot have run, and nothing
             but the token's event can have ordered the consumer behind it.  Asserted in every case;
  judge      both results (a) have the bits of the same two calls made on the default stream alone on a `copy.deepcopy` of the module
             (empty caches), and (b) are within the bar of the matching single-stream test against float64: helpers.rel_err <= 1e-5
             against tests/inverse_backward_ref.py / the oracle for the units and against the float64 formulas for the per-pixel
             layers; the whole model against its float64 twin at the bars of tests/test_gpu_train_loop.py (5e-5 for x, 1e-5 for
             log q).

Without the tokens the consumer's launch reads memory that `torch.empty` handed out and no kernel has written yet: wrong numbers, no
fault (the packed banks are plain floats, there is no control flow on them; tests/test_gpu_bounds.py pushes NaN and Inf through the
same kernels).  What each case gave before the tokens existed is in profiles/cache_streams/parent_outcome.txt.

Measured on an MI355X (neither figure is a pass bar): the delay, timed once per module with events, 49.5 ms of `torch.cuda._sleep`;
the host time from the producer's queue point to behind the consumer's, 0.16 ms (the plain inverse) to 1.1 ms (the premultiplied
chain) for the single layers and 2.9 ms for the whole model.
The spline's knot table and the PLU composition (profiles/cache_streams/spline_plu_cases.jsonl): 0.34 ms (shared table), 0.32 ms
(per-position table) and 0.16 ms; neither `_compose` nor the compose launch synchronises the host.
"""
import copy
import time

import numpy as np
import pytest
import torch

import flow_twin
import inverse_backward_ref as ref
from helpers import ORIENT_FASTFLOW, rel_err, report, same_bits
from oracle import oracle
from test_gpu_parity import PREMULTIPLIED_CASES

pytestmark = pytest.mark.gpu

TOL = 1e-5                   # tests/test_gpu_unit_host.py, test_gpu_inverse_backward.py, test_gpu_coupling.py: helpers.rel_err
CHAIN_TOL = 5e-5             # tests/test_gpu_train_loop.py: a sample through the whole model
DELAY_MS = 50.0
UNIT = (12, 3)               # FastFlowUnit(12, 12, 3) ...
UNIT_ACTS = (2, 12, 8, 16)   # ... at [2, 12, 8, 16]
PIXEL_ACTS = (3, 12, 8, 8)   # Conv1x1 / ActNorm / Coupling
MODEL = dict(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 16, 16), preprocess=False, coupling_width=16)
MODEL_BATCH = 2


# ---------------------------------------------------------------------------------------------------------------------------------
# the rig: two warm side streams and a calibrated delay
# ---------------------------------------------------------------------------------------------------------------------------------
class Rig:
    def __init__(self, dev):
        self.dev = dev
        self.s1, self.s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        self.sleeps = hasattr(torch.cuda, "_sleep")
        self._a = torch.randn(2048, 2048, device=dev)
        self.units = 1_000_000 if self.sleeps else 4          # cycles, or matrix products
        self._delay()                                         # (the first launch loads the kernel)
        ms = self._timed()
        self.units = max(1, int(self.units * DELAY_MS / max(ms, 1e-3)))
        self.delay_ms = self._timed()
        self.gaps = []
        print("cache_streams: a delay of %.1f ms (%s, %d units)" % (self.delay_ms, "torch.cuda._sleep" if self.sleeps else "matmul chain", self.units))

    def _delay(self):
        if self.sleeps:
            torch.cuda._sleep(self.units)
        else:
            for _ in range(self.units):
                self._a @ self._a

    def _timed(self):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(self.dev)
        start.record()
        self._delay()
        stop.record()
        torch.cuda.synchronize(self.dev)
        return start.elapsed_time(stop)

    def warm(self, calls):
        """Every kind of call of this file once on the default stream and on both side streams: kernels loaded, per-stream workspaces
        and allocator pools filled (with a throwaway module's values), so that a case's own calls only queue launches."""
        for s in (torch.cuda.current_stream(self.dev), self.s1, self.s2):
            with torch.cuda.stream(s):
                for call in calls:
                    call()
            torch.cuda.synchronize(self.dev)

    def behind_a_delay(self, stream):
        """Queues the delay on `stream`; returns the event recorded right behind it."""
        with torch.cuda.stream(stream):
            self._delay()
            done = torch.cuda.Event()
            done.record(stream)
        return done

    def cross(self, produce, consume):
        """(s1's result, s2's result, was the delay still running when the consumer had been queued?)"""
        torch.cuda.synchronize(self.dev)
        main = torch.cuda.current_stream(self.dev)
        self.s1.wait_stream(main)
        self.s2.wait_stream(main)
        with torch.cuda.stream(self.s1):
            done = self.behind_a_delay(self.s1)
            t0 = time.perf_counter()
            r1 = produce()
        with torch.cuda.stream(self.s2):
            r2 = consume()
        gap = time.perf_counter() - t0
        pending = not done.query()
        torch.cuda.synchronize(self.dev)
        self.gaps.append(gap)
        return r1, r2, pending, gap


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    dev = torch.device("cuda:0")
    r = Rig(dev)
    unit, x = fresh_unit(dev, 900), acts(dev, UNIT_ACTS, 901)
    ls, tr = affine_params(dev, UNIT[0], 902)
    mix, coupling, xp = fresh_mix(dev, 12, 903), fresh_coupling(dev, 904), acts(dev, PIXEL_ACTS, 905)
    a64 = torch.randn(32, 32, device=dev, dtype=torch.float64)

    def no_grad_calls():
        with torch.no_grad():
            z = unit(x)[0]
            unit.reverse(z)
            unit.reverse_affine(unit.forward_affine(x, ls, tr), ls, tr)
            mix.reverse_with_logdet(mix.reverse_then_affine(xp, ls, tr))
            coupling.reverse(coupling(xp)[0])
            torch.block_diag(a64, a64) @ torch.block_diag(a64, a64)
    r.warm([no_grad_calls, lambda: train(unit, x, x), lambda: reverse_grad(unit, x, x)])
    yield r
    print("cache_streams: delay %.1f ms; host time from the producer's queue point to behind the consumer's: min %.2f ms, max %.2f ms over "
          "%d cases" % (r.delay_ms, 1e3 * min(r.gaps, default=0), 1e3 * max(r.gaps, default=0), len(r.gaps)))


# ---------------------------------------------------------------------------------------------------------------------------------
# modules with fresh values, and the calls
# ---------------------------------------------------------------------------------------------------------------------------------
def fresh_unit(dev, seed, C=UNIT[0], K=UNIT[1]):
    from fincflow_amd import FastFlowUnit
    torch.manual_seed(seed)
    return FastFlowUnit(C, C, K).to(dev)


def new_weights(unit, seed):
    """Other random banks written IN PLACE: same addresses, a new version -- every bank kind of the unit is rebuilt on its next use."""
    other = fresh_unit(unit.conv_tl.conv.weight.device, seed, 4 * unit.conv_tl.conv.weight.shape[0], unit.conv_tl.kernel_size)
    with torch.no_grad():
        for w, v in zip(unit._weights(), other._weights()):
            w.copy_(v)


def acts(dev, shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def affine_params(dev, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.2 * torch.randn(C, generator=g)).to(dev), torch.randn(C, generator=g).to(dev)


def new_affine_params(ls, tr, seed):
    a, b = affine_params(ls.device, ls.numel(), seed)
    with torch.no_grad():
        ls.copy_(a)
        tr.copy_(b)


def fresh_mix(dev, C, seed):
    from fincflow_amd import glow
    np.random.seed(seed)
    return glow.Conv1x1(C).to(dev)


def fresh_coupling(dev, seed):
    from fincflow_amd import glow
    torch.manual_seed(seed)
    return flow_twin.randomise(glow.Coupling(PIXEL_ACTS[1:], width=32), seed=seed).to(dev)


def train(unit, x, g):
    """The training path: forward under autograd (no invariant check) and its backward; [z, grad_x, grad of the four stored banks]."""
    x = x.clone().requires_grad_(True)
    z = unit(x)[0]
    return [z.detach()] + list(torch.autograd.grad(z, [x] + unit._weights(), g))


def reverse_grad(unit, z, g):
    """`reverse` inside `reverse_grad()` and its backward: [x, grad_z, grad of the four stored banks]."""
    from fincflow_amd import ops
    z = z.clone().requires_grad_(True)
    with ops.reverse_grad():
        x = unit.reverse(z)
    return [x.detach()] + list(torch.autograd.grad(x, [z] + unit._weights(), g))


def stored64(unit):
    return torch.cat([w.detach() for w in unit._weights()]).double().cpu()


def mask64(unit):
    w = unit.conv_tl.conv.weight
    return ref.stored_mask(4, w.shape[1], w.shape[2], w.shape[3], ORIENT_FASTFLOW)


def forward64(unit, x):
    return ref.forward(x.double().cpu(), stored64(unit), 4, ORIENT_FASTFLOW)


def solve64(unit, z):
    return ref.solve(z.double().cpu(), stored64(unit), 4, ORIENT_FASTFLOW)


def affine64(t, ls, tr, direction):
    s, b = ls.double().cpu().view(1, -1, 1, 1), tr.double().cpu().view(1, -1, 1, 1)
    t = t.double().cpu()
    return (t - b) * torch.exp(-s) if direction > 0 else t * torch.exp(s) + b


def mix64(mix, t):
    return torch.einsum("oi,bihw->bohw", torch.inverse(mix.W.detach().double().cpu()), t.double().cpu())


def uses_mfma(shape, K, forward=False):
    """The library's own answers: this shape is served from packed fragments."""
    from fincflow_amd import _lib
    B, C, H, W = shape
    q = "finc_forward_algo_for" if forward else "finc_inverse_algo_for"
    assert getattr(_lib.lib(), q)(C // 4, H, W, K, K) == _lib.ALGO["mfma"], (q, shape)
    if not forward:
        assert _lib.inverse_variant(B, 4, C // 4, H, W, K, K) is not None, shape


# ---------------------------------------------------------------------------------------------------------------------------------
# one case
# ---------------------------------------------------------------------------------------------------------------------------------
def run_case(rig, name, module, produce, consume, want, names, bars=None):
    """`produce(m)` / `consume(m)`: lists of tensors from the module (or list of modules) `m`; `want(which)`: the float64 lists
    (which = 0: the producer's, 1: the consumer's); `bars`: one per name, or a dict "s1/<name>", "s2/<name>" -> bar.  Prints and records
    every figure, then asserts non-vacuity, bits and bars."""
    from fincflow_amd import _lib
    alone = copy.deepcopy(module)
    r1, r2, pending, gap = rig.cross(lambda: produce(module), lambda: consume(module))
    b1 = produce(alone)
    torch.cuda.synchronize(rig.dev)
    b2 = consume(alone)
    torch.cuda.synchronize(rig.dev)
    bars = bars or [TOL] * len(names)
    errs, bits = {}, {}
    for which, (got, base) in enumerate(((r1, b1), (r2, b2))):
        wanted = want(which)
        assert len(got) == len(base) == len(wanted) == len(names), (name, len(got), len(base), len(wanted))
        for n, g, b, w in zip(names, got, base, wanted):
            tag = "s%d/%s" % (which + 1, n)
            bits[tag] = same_bits(g, b)
            errs[tag] = rel_err(g.detach().cpu().numpy(), np.asarray(w)) if bool(torch.isfinite(g).all()) else float("inf")
    worst = max(errs, key=errs.get)
    print("cache_streams %s: delay pending %s, host gap %.2f ms, worst error %.3e at %s, bits differ at %s" % (
        name, pending, 1e3 * gap, errs[worst], worst, [t for t, same in bits.items() if not same] or "none"))
    report("cache_streams", case=name, pending=pending, gap_ms=1e3 * gap, worst=errs[worst], worst_at=worst, errors=errs,
           bits_differ=[t for t, same in bits.items() if not same])
    assert pending, "%s: the delay had finished before the consumer was queued (a host synchronisation in the builder?): vacuous" % name
    assert all(bits.values()), (name, "not the bits of the same calls on one stream", [t for t, same in bits.items() if not same])
    over = {t: e for t, e in errs.items() if not e <= (bars[t] if isinstance(bars, dict) else bars[names.index(t.split("/", 1)[1])])}
    assert not over, (name, over)
    assert not _lib.fault_pending()


def unit_case(rig, name, seed, prime, call, want_of, names, forward=False, affine=False):
    """A bank kind of FastFlowUnit(12, 12, 3) at [2, 12, 8, 16]: `prime(unit, x0)` validates the fresh bank through another kind of
    call; with `affine`, the cache is primed whole and the ActNorm parameters change afterwards."""
    dev = rig.dev
    uses_mfma(UNIT_ACTS, UNIT[1], forward)
    unit = fresh_unit(dev, seed)
    x0, x1, x2 = (acts(dev, UNIT_ACTS, seed + k) for k in (1, 2, 3))
    ls, tr = affine_params(dev, UNIT[0], seed + 4)
    with torch.no_grad():
        prime(unit, x0, ls, tr)
        torch.cuda.synchronize(dev)
        if affine:
            new_affine_params(ls, tr, seed + 5)
    run_case(rig, name, unit, lambda m: call(m, x1, ls, tr), lambda m: call(m, x2, ls, tr),
             lambda which: want_of(unit, (x1, x2)[which], ls, tr), names)


def no_grad(fn):
    def wrapped(*args):
        with torch.no_grad():
            out = fn(*args)
        assert out is not None, "the fused path stepped aside: the cache under test is not used"
        return [out]
    return wrapped


def test_forward_fragments(rig):
    unit_case(rig, "fwd", 100, lambda u, x, ls, tr: u.reverse(x), no_grad(lambda u, x, ls, tr: u(x)[0]),
              lambda u, x, ls, tr: [forward64(u, x)], ["z"], forward=True)


def test_inverse_fragments(rig):
    unit_case(rig, "inv", 110, lambda u, x, ls, tr: u(x), no_grad(lambda u, x, ls, tr: u.reverse(x)),
              lambda u, x, ls, tr: [solve64(u, x)], ["x"])


def test_forward_fragments_with_the_folded_actnorm(rig):
    unit_case(rig, "fwd_affine", 120, lambda u, x, ls, tr: u.forward_affine(x, ls, tr), no_grad(lambda u, x, ls, tr: u.forward_affine(x, ls, tr)),
              lambda u, x, ls, tr: [affine64(forward64(u, x), ls, tr, +1)], ["y"], forward=True, affine=True)


def test_inverse_fragments_with_the_folded_actnorm(rig):
    unit_case(rig, "inv_affine", 130, lambda u, x, ls, tr: u.reverse_affine(x, ls, tr), no_grad(lambda u, x, ls, tr: u.reverse_affine(x, ls, tr)),
              lambda u, x, ls, tr: [solve64(u, affine64(x, ls, tr, -1))], ["x"], affine=True)


def test_canonical_bank_on_the_training_path(rig):
    """A fresh weight version met by the training forward (`validate=False`: no check, no synchronisation): the canonical bank and the
    forward fragments are built behind the delay; the consumer's forward reads the fragments, its backward the canonical bank."""
    dev, seed = rig.dev, 140
    uses_mfma(UNIT_ACTS, UNIT[1], forward=True)
    unit = fresh_unit(dev, seed)
    x0, x1, x2, g1, g2 = (acts(dev, UNIT_ACTS, seed + k) for k in (1, 2, 3, 4, 5))
    train(unit, x0, g1)
    torch.cuda.synchronize(dev)
    new_weights(unit, seed + 6)

    def want(which):
        x, g = ((x1, g1), (x2, g2))[which]
        gx, gw = ref.forward_vjp(x.cpu().numpy(), stored64(unit).numpy(), g.cpu().numpy(), 4, ORIENT_FASTFLOW)
        return [forward64(unit, x), gx] + list(np.split(gw * mask64(unit).numpy(), 4))
    run_case(rig, "w_canon", unit, lambda m: train(m, x1, g1), lambda m: train(m, x2, g2), want,
             ["z", "grad_x", "grad_w_tl", "grad_w_tr", "grad_w_bl", "grad_w_br"])


def test_adjoint_bank_and_its_fragments(rig):
    """`unit.reverse` inside `reverse_grad()` followed by the backward: the first backward of a weight version builds (w_adj, lead_t)
    and packs the adjoint bank (kind `inv_adjoint`) behind the delay; the consumer's backward finds both."""
    dev, seed = rig.dev, 150
    uses_mfma(UNIT_ACTS, UNIT[1])
    unit = fresh_unit(dev, seed)
    x0, z1, z2, g1, g2 = (acts(dev, UNIT_ACTS, seed + k) for k in (1, 2, 3, 4, 5))
    with torch.no_grad():
        unit.reverse(unit(x0)[0])                              # validated, canonical, the plain inverse fragments: all but the adjoint
    torch.cuda.synchronize(dev)

    def want(which):
        z, g = ((z1, g1), (z2, g2))[which]
        x, gz, gw = ref.reference_grads(z.cpu().numpy(), stored64(unit).numpy(), g.cpu().numpy(), 4, ORIENT_FASTFLOW)
        return [x, gz] + list(np.split(gw * mask64(unit).numpy(), 4))
    run_case(rig, "adjoint", unit, lambda m: reverse_grad(m, z1, g1), lambda m: reverse_grad(m, z2, g2), want,
             ["x", "grad_z", "grad_w_tl", "grad_w_tr", "grad_w_bl", "grad_w_br"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the premultiplied chain: channel mix -> ActNorm -> unit, the mix applying the unit's Linv
# ---------------------------------------------------------------------------------------------------------------------------------
def premultiplied_shape():
    from fincflow_amd import _lib, ops
    shapes = [c for c in PREMULTIPLIED_CASES if _lib.lib().finc_inverse_premultiplied_supported(c[0], 4, c[1] // 4, c[2], c[3], c[4], c[4]) == 1
              and ops.mix_supported(c[1])]
    return min(shapes, key=lambda c: c[0] * c[1] * c[2] * c[3])


def premultiplied_case(rig, name, seed, new_unit_weights):
    from fincflow_amd import glow
    dev = rig.dev
    B, C, H, W, K = premultiplied_shape()
    shape = (B, C, H, W)
    uses_mfma(shape, K)
    unit, mix, an = fresh_unit(dev, seed, C, K), fresh_mix(dev, C, seed + 1), glow.ActNorm(C).to(dev)
    an.mark_initialized()
    new_affine_params(an.log_scale, an.translation, seed + 2)
    u0, u1, u2 = (acts(dev, shape, seed + k) for k in (3, 4, 5))

    def chain(m, u):
        unit_, mix_, an_ = m
        with torch.no_grad():
            out = unit_.reverse_after_mix(u, mix_, an_.reverse_affine_params())
        assert out is not None, "the premultiplied chain stepped aside"
        return [out]
    modules = torch.nn.ModuleList([unit, mix, an])
    chain(modules, u0)                                         # everything once: W^-1 (torch.inverse synchronises), Linv, the mix's fold
    torch.cuda.synchronize(dev)
    if new_unit_weights:                                       # Linv, then (keyed on it) the mix's fold, then the inverse fragments
        new_weights(unit, seed + 6)
        with torch.no_grad():
            unit(u0)                                           # (the invariant check of the new version, through the forward)
    else:                                                      # the mix's fold alone
        new_affine_params(an.log_scale, an.translation, seed + 7)
    torch.cuda.synchronize(dev)
    pick = sorted({0, B // 2, B - 1})                          # (the oracle on every image takes a while)

    def want(which):
        u = (u1, u2)[which][pick]
        a = affine64(mix64(mix, u), an.log_scale.detach(), an.translation.detach(), -1)
        wco = oracle.canonicalize(stored64(unit).float().numpy(), 4, ORIENT_FASTFLOW)
        return [oracle.inverse_via_f64(a.float().numpy(), wco, 4, ORIENT_FASTFLOW)]

    def picked(results):
        return [results[0][pick]]
    # (bits on the whole batch, the float64 bar on the picked images)
    alone = copy.deepcopy(modules)
    r1, r2, pending, gap = rig.cross(lambda: chain(modules, u1), lambda: chain(modules, u2))
    b1, b2 = chain(alone, u1), chain(alone, u2)
    torch.cuda.synchronize(dev)
    bits = {"s1/x": same_bits(r1[0], b1[0]), "s2/x": same_bits(r2[0], b2[0])}
    errs = {"s%d/x" % (k + 1): rel_err(picked(r)[0].cpu().numpy(), want(k)[0]) if bool(torch.isfinite(r[0]).all()) else float("inf")
            for k, r in enumerate((r1, r2))}
    worst = max(errs, key=errs.get)
    print("cache_streams %s %s: delay pending %s, host gap %.2f ms, worst error %.3e at %s, bits differ at %s" % (
        name, shape, pending, 1e3 * gap, errs[worst], worst, [t for t, same in bits.items() if not same] or "none"))
    report("cache_streams", case=name, pending=pending, gap_ms=1e3 * gap, worst=errs[worst], worst_at=worst, errors=errs,
           bits_differ=[t for t, same in bits.items() if not same])
    from fincflow_amd import _lib
    assert pending, "%s: the delay had finished before the consumer was queued: vacuous" % name
    assert all(bits.values()), (name, bits)
    assert all(e <= TOL for e in errs.values()), (name, errs)
    assert _lib.hlp_timeouts() == 0 and not _lib.fault_pending()


def test_lead_inverse_of_the_premultiplied_chain(rig):
    premultiplied_case(rig, "linv", 200, new_unit_weights=True)


def test_the_mix_matrix_that_carries_the_lead_inverse(rig):
    premultiplied_case(rig, "m_lead", 210, new_unit_weights=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-pixel layers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_mix_matrix_that_carries_the_actnorm(rig):
    dev, seed = rig.dev, 300
    mix = fresh_mix(dev, PIXEL_ACTS[1], seed)
    ls, tr = affine_params(dev, PIXEL_ACTS[1], seed + 1)
    z0, z1, z2 = (acts(dev, PIXEL_ACTS, seed + k) for k in (2, 3, 4))
    call = no_grad(lambda m, z: m.reverse_then_affine(z, ls, tr))
    call(mix, z0)                                              # W^-1 (torch.inverse synchronises) and the fold, once
    torch.cuda.synchronize(dev)
    new_affine_params(ls, tr, seed + 5)
    run_case(rig, "m_aff", mix, lambda m: call(m, z1), lambda m: call(m, z2),
             lambda which: [affine64(mix64(mix, (z1, z2)[which]), ls, tr, -1)], ["x"])


def test_the_cached_log_determinant(rig):
    dev, seed = rig.dev, 310
    mix = fresh_mix(dev, PIXEL_ACTS[1], seed)
    z0, z1, z2 = (acts(dev, PIXEL_ACTS, seed + k) for k in (2, 3, 4))

    def call(m, z):
        with torch.no_grad():
            return list(m.reverse_with_logdet(z))
    with torch.no_grad():
        # (the orthogonal initialisation has log|det W| = 0 up to rounding, and an error relative to that says nothing: rows scaled
        # by 0.6 .. 1.9 put it near 2)
        mix.W.mul_(torch.linspace(0.6, 1.9, PIXEL_ACTS[1], device=dev).view(-1, 1))
        mix.reverse(z0)                                        # W^-1 only: log|det W| is built by the producer
    torch.cuda.synchronize(dev)
    with torch.no_grad():
        assert "_ld" not in mix.__dict__ and mix._hip(z0), "not on the HIP inference path, or log|det W| is there already"

    def want(which):
        z = (z1, z2)[which]
        ld = z.shape[2] * z.shape[3] * torch.slogdet(mix.W.detach().double().cpu())[1]
        return [mix64(mix, z), ld.expand(len(z))]
    run_case(rig, "ld", mix, lambda m: call(m, z1), lambda m: call(m, z2), want, ["x", "logdet"])


def test_the_coupling_scale_and_shift(rig):
    dev, seed = rig.dev, 320
    coupling = fresh_coupling(dev, seed)
    x0, x1, x2 = (acts(dev, PIXEL_ACTS, seed + k) for k in (2, 3, 4))

    def call(m, x):
        with torch.no_grad():
            return list(m(x))
    call(coupling, x0)
    torch.cuda.synchronize(dev)
    with torch.no_grad():
        assert coupling._hip(x0), "the coupling is not on its HIP inference path: the cached scale and shift are not used"
    g = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():                                      # new Conv2dZero scale and bias, in place
        last = coupling.net[4]
        last.logs.copy_((0.05 * torch.randn(last.logs.shape, generator=g)).to(dev))
        last.bias.copy_((0.05 * torch.randn(last.bias.shape, generator=g)).to(dev))

    def want(which):
        twin = copy.deepcopy(coupling).cpu().double()          # (on the host the layer runs the reference's PyTorch formula)
        with torch.no_grad():
            return list(twin((x1, x2)[which].double().cpu()))
    run_case(rig, "ab", coupling, lambda m: call(m, x1), lambda m: call(m, x2), want, ["y", "logdet"])


def fresh_spline(dev, seed, individual):
    import spline_twin
    return spline_twin.unit_scale_layer(PIXEL_ACTS[1:], 5, 3.0, individual, seed).to(dev)


@pytest.mark.parametrize("individual", (False, True), ids=("shared", "individual"))
def test_the_spline_knot_table(rig, individual):
    """`SplineActivation._table`: new parameters in place; the producer's `forward` composes the knot table (parameter-sized PyTorch
    launches) behind the delay, the consumer's `reverse_with_logdet` on other input finds it.  The bar is TOL unless the layer's own
    fp32 PyTorch lines on the CPU are themselves further than half of that from float64 on these inputs: then it is the spline
    judge's max(1e-5, 2 * e_ref) (tests/spline_twin.py) -- the inverse of a unit-scale spline loses digits in any fp32 arithmetic."""
    dev, seed = rig.dev, 500 + int(individual)
    m = fresh_spline(dev, seed, individual)
    x0, x1, x2 = (acts(dev, PIXEL_ACTS, seed + k) for k in (2, 3, 4))

    def forward(mod, x):
        with torch.no_grad():
            return list(mod(x))

    def reverse(mod, x):
        with torch.no_grad():
            return list(mod.reverse_with_logdet(x))
    throwaway = fresh_spline(dev, seed + 9, individual)
    # (the throwaway's table is dropped each time: the composing launches and their allocations happen on every stream)
    rig.warm([lambda: (throwaway.__dict__.pop("_tab_key", None), forward(throwaway, x0), reverse(throwaway, x0))])
    forward(m, x0)
    torch.cuda.synchronize(dev)
    primed = m._tab_key
    fresh = [p.detach().clone() for p in fresh_spline(dev, seed + 5, individual).parameters()]
    with torch.no_grad():
        for p, v in zip(m.parameters(), fresh):                 # in place: same addresses, a new version
            p.copy_(v)
    torch.cuda.synchronize(dev)
    keys = []

    def keyed(call, x):
        def run(mod):
            out = call(mod, x)
            keys.append(mod._tab_key)
            return out
        return run

    def twin_results(dtype):
        twin = copy.deepcopy(m).cpu().to(dtype)                # (on the host the layer runs its PyTorch lines)
        return [forward(twin, x1.cpu().to(dtype)), reverse(twin, x2.cpu().to(dtype))]
    want, lines32 = twin_results(torch.float64), twin_results(torch.float32)
    names = ["out", "logdet"]
    e_ref = {"s%d/%s" % (w + 1, n): rel_err(lines32[w][i].numpy(), want[w][i].numpy()) for w in (0, 1) for i, n in enumerate(names)}
    print("cache_streams spline_table: the fp32 CPU lines against float64: %s" % e_ref)
    name = "spline_table_" + ("individual" if individual else "shared")
    run_case(rig, name, m, keyed(forward, x1), keyed(reverse, x2), lambda which: want[which], names,
             {t: max(TOL, 2 * e) for t, e in e_ref.items()})
    assert keys[0] != primed, "the producer did not rebuild the table"
    assert keys[1] == keys[0], "the consumer rebuilt the table: not a cache hit"


def fresh_plu(dev, seed):
    """Conv1x1LU(12) with perturbed factors: log|det W| near 2.4 (the orthogonal initialisation has 0 up to rounding, and an error
    relative to that says nothing)."""
    from fincflow_amd import glow
    np.random.seed(seed)
    m = glow.Conv1x1LU(PIXEL_ACTS[1])
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.lower.add_(0.1 * torch.randn(m.lower.shape, generator=g).tril(-1))
        m.upper.add_(0.1 * torch.randn(m.upper.shape, generator=g).triu(1))
        m.log_s.add_(torch.linspace(-0.2, 0.6, PIXEL_ACTS[1]))
    return m.to(dev)


def test_the_plu_composition(rig):
    """`Conv1x1LU._values`: new `lower`, `upper` and `log_s` in place; the producer's `reverse_with_logdet` runs the one compose launch
    that fills (W, W^-1, log|det W|) behind the delay, the consumer's `forward` on other input takes W and the log-det from the
    cache."""
    dev, seed = rig.dev, 520
    m = fresh_plu(dev, seed)
    z0, z1, z2 = (acts(dev, PIXEL_ACTS, seed + k) for k in (2, 3, 4))

    def call(mod, z, reverse):
        with torch.no_grad():
            out, ld = mod.reverse_with_logdet(z) if reverse else mod(z)
        return [out, ld.expand(len(z))]                         # (`forward` returns the log-det 0-dim)
    throwaway = fresh_plu(dev, seed + 9)
    # (the throwaway's values are dropped each time: the compose launch and its allocations happen on every stream)
    rig.warm([lambda: (throwaway.__dict__.pop("_plu_key", None), call(throwaway, z0, True), call(throwaway, z0, False))])
    call(m, z0, True)
    torch.cuda.synchronize(dev)
    with torch.no_grad():
        assert m._plu_kernel() and m._hip(z0), "not on the HIP compose and mix kernels: the cache under test is not used"
    primed = m._plu_key
    other = fresh_plu(dev, seed + 5)
    with torch.no_grad():
        for p, v in zip(m._factors(), other._factors()):        # in place: same addresses, a new version
            p.copy_(v.detach())
    torch.cuda.synchronize(dev)
    keys = []

    def keyed(z, reverse):
        def run(mod):
            out = call(mod, z, reverse)
            keys.append(mod._plu_key)
            return out
        return run

    def want(which):
        twin = copy.deepcopy(m).cpu().double()                  # (`_compose_torch` in double)
        return call(twin, (z1, z2)[which].double().cpu(), which == 0)
    run_case(rig, "plu_values", m, keyed(z1, True), keyed(z2, False), want, ["out", "logdet"])
    assert keys[0] != primed, "the producer did not compose anew"
    assert keys[1] == keys[0], "the consumer composed again: not a cache hit"


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sample_on_one_stream_and_sample_with_log_prob_on_another_after_an_optimiser_step(rig):
    """After an optimiser step every derived value of every layer is stale.  The banks are validated and W^-1 / log|det W| rebuilt on
    the default stream (`log_prob`, the two cached [C, C] values: the builders that synchronise); `sample` on s1 then builds every
    fold of the reverse chain behind the delay, and `sample_with_log_prob` on s2 finds them."""
    from fincflow_amd import _lib, glow
    dev, seed = rig.dev, 400
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = flow_twin.randomise(glow.create_model(**MODEL), seed=seed + 1, actnorm=True).to(dev)
    assert _lib.inverse_variant(MODEL_BATCH, 4, 3, 8, 8, 3, 3) is not None       # the first level's unit: 12 channels at 8x8
    x = acts(dev, (8,) + MODEL["image_size"], seed + 2)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    with torch.no_grad():
        model.sample(MODEL_BATCH)
        model.sample_with_log_prob(MODEL_BATCH)
    (-model.log_prob(x).mean() / x[0].numel()).backward()
    opt.step()
    with torch.no_grad():
        model.log_prob(x)
        for m in model.modules():
            if isinstance(m, glow.Conv1x1):
                m._inverse_matrix()
                m._log_abs_det()
    torch.cuda.synchronize(dev)
    alone, twin = copy.deepcopy(model), flow_twin.twin_of(model)
    draws = {}

    def sample(m, key):
        torch.manual_seed(seed + 3)
        with torch.no_grad(), flow_twin.recorded_noise(m) as d:
            out = [m.sample(MODEL_BATCH)[0]]
        draws.setdefault(key, d)
        return out

    def sample_with_log_prob(m, key):
        torch.manual_seed(seed + 4)
        with flow_twin.recorded_noise(m) as d:
            out = list(m.sample_with_log_prob(MODEL_BATCH))
        draws.setdefault(key, d)
        return out
    r1, r2, pending, gap = rig.cross(lambda: sample(model, "s1"), lambda: sample_with_log_prob(model, "s2"))
    b1, b2 = sample(alone, "alone1"), sample_with_log_prob(alone, "alone2")
    torch.cuda.synchronize(dev)
    with torch.no_grad():
        with flow_twin.replayed_noise(twin, draws["s1"]):
            w1 = [twin.sample(MODEL_BATCH)[0]]
        with flow_twin.replayed_noise(twin, draws["s2"]):
            w2 = list(twin.sample_with_log_prob(MODEL_BATCH))
        w2.append(twin.log_prob(r2[0].double().cpu()))
    names, bars = ["s1/x", "s2/x", "s2/log_q", "s2/log_q_at_x"], [CHAIN_TOL, CHAIN_TOL, TOL, TOL]
    got, base, wanted = [r1[0], r2[0], r2[1], r2[1]], [b1[0], b2[0], b2[1], b2[1]], [w1[0], w2[0], w2[1], w2[2]]
    bits = {n: same_bits(g, b) for n, g, b in zip(names, got, base)}
    errs = {n: flow_twin.error(g, w) if bool(torch.isfinite(g).all()) else float("inf") for n, g, w in zip(names, got, wanted)}
    worst = max(errs, key=errs.get)
    print("cache_streams model: delay pending %s, host gap %.2f ms, worst error %.3e at %s, bits differ at %s" % (
        pending, 1e3 * gap, errs[worst], worst, [t for t, same in bits.items() if not same] or "none"))
    report("cache_streams", case="model", pending=pending, gap_ms=1e3 * gap, worst=errs[worst], worst_at=worst, errors=errs,
           bits_differ=[t for t, same in bits.items() if not same])
    assert pending, "model: the delay had finished before the consumer was queued: vacuous"
    assert all(bits.values()), bits
    assert all(errs[n] <= bar for n, bar in zip(names, bars)), errs
    assert not _lib.fault_pending()
