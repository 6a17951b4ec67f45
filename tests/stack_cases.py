"""Layer orders for `FlowSequential`, stated by hand, each with the number of times every fold of its matcher must fire.  A helper in
the style of tests/plan_cases.py, not collected: tests/test_stack_orders_host.py checks the float64 twin on every order without a GPU,
tests/test_gpu_stack_orders.py runs the HIP model on every order against that twin and counts the folds.  Nothing here calls the
library except `build`, which turns a case into modules.

The rules the numbers are written out from (fincflow_amd/layers.py, `FlowSequential`):

  F   `_forward_layers`, no autograd graph: FastFlowUnit -> ActNorm (initialised) is one launch (`cache.forward_affine`).
  R1  `_reverse_chain`, read from the LAST layer: ActNorm -> FastFlowUnit is one launch (`cache.inverse_affine`).
  R2  Conv1x1 -> [ActNorm] -> FastFlowUnit: the premultiplied inverse (`Conv1x1.reverse_premultiplied` + `cache.inverse_premultiplied`),
      full-chip problem sets only.  A mix that R2 declines goes on to R3, then to its plain `reverse`.
  R3  Conv1x1 -> ActNorm with NO FastFlowUnit behind the ActNorm: one mixing launch (`Conv1x1.reverse_then_affine`).
  Every layer no fold takes runs its own `reverse` / `reverse_with_logdet`: `Conv1x1.reverse`, `ActNorm.reverse`, and `cache.inverse`
  for a FastFlowUnit, a CINCFlowUnit and a PaddedConv2d alike.
  With `invertible_backward`, every maximal run of two or more layers that support `backward_from_output` is ONE
  `_InvertibleRunFunction` node; its forward is the no-grad pass, folds of kind F included (`F_runs`).  Squeeze and every layer with
  a HIP path support it, SplitPrior does not, a Conv1x1 without a mix kernel does not.

A fold also depends on what the library can launch for a shape.  Where that is not a given, a count is a function of `can`, the
answers of the library's capability queries (asked by the tests, not here), keyed by the kind of fold and the FORWARD index of its
FastFlowUnit: can["F", i] (the forward's strip kernel exists), can["R1", i] (`finc_inverse_affine_supported` and an MFMA inverse),
can["R2", i] (`finc_inverse_premultiplied_supported` at the sampling batch) -- 0 or 1, so a count reads "fires iff the query says yes".
Channel counts 8, 12 and 16 have a mix kernel and 20 has none (`ops.mix_supported`): a premise, asserted by the host test.

Layer codes: U FastFlowUnit 3x3, U2 / U5 2x2 / 5x5, X CINCFlowUnit 3x3, P:<order>[:bias] PaddedConv2d 3x3, A ActNorm, M Conv1x1,
K Coupling, Kc Coupling with n_context = 3, S Squeeze, Z SplitPrior; "=k" is the module OBJECT of position k again.
"""
import random

WIDTH = 16                       # the coupling nets' width
N_CONTEXT = 3
BATCH = 4
FULL_CHIP = "full_chip"          # batch: the smallest the library takes the premultiplied inverse for (the sampling views only)

UNITS = ("U", "U2", "U5")        # the codes of a FastFlowUnit
KERNEL = {"U": 3, "U2": 2, "U5": 5, "X": 3}

# name -> dict(layers, image=(C, H, W) of the model's input, batch, context: channels of the context or None, frozen: positions with
#              requires_grad_(False), expect)
# expect: F, F_runs -- log_prob without a graph / inside the invertible runs of one training pass; R1, R2, R3, mix_reverse,
#         actnorm_reverse, inverse -- one fused reverse pass (sample, sample_with_log_prob, the second half of reconstruct);
#         nodes -- `_InvertibleRunFunction.apply` calls of one training pass with x.requires_grad.
CASES = {
    "glow_baseline": dict(
        layers=["S", "A", "M", "K", "A", "M", "K"], image=(3, 16, 16), batch=BATCH, context=None,
        expect=dict(F=0,                   # no unit anywhere
                    F_runs=0,
                    R1=0,                  # no unit anywhere
                    R2=0,                  # no unit behind either mix
                    R3=2,                  # M -> A with a Coupling, then the Squeeze behind the ActNorm: both mixes
                    mix_reverse=0,         # both went with R3
                    actnorm_reverse=0,     # both went with R3
                    inverse=0,
                    nodes=1)),             # seven supporting layers, one run
    "cinc_block": dict(
        layers=["X", "A", "M", "K"], image=(8, 8, 8), batch=BATCH, context=None,
        expect=dict(F=0,                   # a CINCFlowUnit is not a FastFlowUnit
                    F_runs=0,
                    R1=0,                  # the same
                    R2=0,                  # the same
                    R3=1,                  # the guard asks for a FastFlowUnit behind the ActNorm: X does not bar it
                    mix_reverse=0, actnorm_reverse=0,
                    inverse=1,             # X solves on its own
                    nodes=1)),
    "mix_actnorm_at_the_end": dict(
        layers=["A", "M"], image=(16, 8, 8), batch=BATCH, context=None,
        expect=dict(F=0, F_runs=0, R1=0, R2=0,
                    R3=1,                  # i + 2 == len(mods): nothing behind the ActNorm at all
                    mix_reverse=0, actnorm_reverse=0, inverse=0,
                    nodes=1)),             # a run of exactly two
    "unit_actnorm_mix_small": dict(
        layers=["U", "A", "M"], image=(12, 8, 8), batch=BATCH, context=None,
        expect=dict(F=1, F_runs=1,         # U -> A
                    R1=lambda can: can["R1", 0],       # A -> U, once the mix has run plain
                    R2=0,                  # four images are no full-chip problem set
                    R3=0,                  # barred: a FastFlowUnit stands behind the ActNorm
                    mix_reverse=1,         # declined by R2, barred from R3
                    actnorm_reverse=lambda can: 1 - can["R1", 0],
                    inverse=lambda can: 1 - can["R1", 0],
                    nodes=1)),
    "unit_actnorm_mix_full_chip": dict(
        layers=["U", "A", "M"], image=(12, 8, 16), batch=FULL_CHIP, context=None,
        expect=dict(F=1, F_runs=1,
                    R1=0,                  # the ActNorm rode in the mix's matrix
                    R2=1,                  # M -> A -> U at a batch the library takes
                    R3=0, mix_reverse=0, actnorm_reverse=0, inverse=0,
                    nodes=1)),
    "unit_mix_full_chip": dict(
        layers=["U", "M"], image=(12, 8, 16), batch=FULL_CHIP, context=None,
        expect=dict(F=0, F_runs=0,         # no ActNorm
                    R1=0,
                    R2=1,                  # M -> U without an affine
                    R3=0, mix_reverse=0, actnorm_reverse=0, inverse=0,
                    nodes=1)),
    "actnorm_first": dict(
        layers=["A", "U", "A"], image=(8, 8, 8), batch=BATCH, context=None,
        expect=dict(F=1, F_runs=1,         # U -> A, the pair that ends the list
                    R1=lambda can: can["R1", 1],       # the last ActNorm and the unit
                    R2=0, R3=0, mix_reverse=0,
                    actnorm_reverse=lambda can: 2 - can["R1", 1],   # the first ActNorm is the last reverse layer: plain
                    inverse=lambda can: 1 - can["R1", 1],
                    nodes=1)),
    "two_actnorms": dict(
        layers=["U", "A", "A"], image=(8, 8, 8), batch=BATCH, context=None,
        expect=dict(F=1, F_runs=1,         # the first ActNorm only: the fold steps over two layers
                    R1=lambda can: can["R1", 0],       # the inner ActNorm
                    R2=0, R3=0, mix_reverse=0,
                    actnorm_reverse=lambda can: 2 - can["R1", 0],   # the outer one has an ActNorm behind it, not a unit
                    inverse=lambda can: 1 - can["R1", 0],
                    nodes=1)),
    "two_mixes": dict(
        layers=["U", "M", "M"], image=(16, 8, 8), batch=BATCH, context=None,
        expect=dict(F=0, F_runs=0, R1=0,
                    R2=lambda can: can["R2", 0],       # the inner mix stands in front of the unit: by batch
                    R3=0,                  # no ActNorm
                    mix_reverse=lambda can: 2 - can["R2", 0],       # the outer mix has a mix behind it: always plain
                    actnorm_reverse=0,
                    inverse=lambda can: 1 - can["R2", 0],
                    nodes=1)),
    "reversed_block": dict(
        layers=["M", "A", "U"], image=(12, 8, 8), batch=BATCH, context=None,
        expect=dict(F=0, F_runs=0,         # the unit is the last layer
                    R1=0,                  # behind the ActNorm stands the mix
                    R2=0,                  # nothing stands behind the mix
                    R3=0,                  # the same
                    mix_reverse=1, actnorm_reverse=1, inverse=1,
                    nodes=1)),
    "squeeze_between": dict(
        layers=["U", "S", "A"], image=(8, 8, 8), batch=BATCH, context=None,
        expect=dict(F=0, F_runs=0,         # the Squeeze stands between them: the ActNorm has 32 channels
                    R1=0,                  # the same
                    R2=0, R3=0, mix_reverse=0, actnorm_reverse=1, inverse=1,
                    nodes=1)),             # the Squeeze supports the walk
    "split_between": dict(
        layers=["S", "U", "A", "M", "K", "Z", "U", "A"], image=(4, 16, 16), batch=BATCH, context=None,
        expect=dict(F=2, F_runs=2,         # 16 channels in front of Z, 8 behind it
                    R1=lambda can: can["R1", 6] + can["R1", 1],
                    R2=0,                  # small set
                    R3=0,                  # barred
                    mix_reverse=1,
                    actnorm_reverse=lambda can: 2 - can["R1", 6] - can["R1", 1],
                    inverse=lambda can: 2 - can["R1", 6] - can["R1", 1],
                    nodes=2)),             # S U A M K | Z | U A: the SplitPrior ends a run and is in none
    "mix_without_a_kernel": dict(
        layers=["U", "A", "M", "K"], image=(20, 8, 8), batch=BATCH, context=None,
        expect=dict(F=1, F_runs=1,
                    R1=lambda can: can["R1", 0],
                    R2=0, R3=0,            # (and at no batch: the mix has no launch to fold into)
                    mix_reverse=1,         # on F.conv2d
                    actnorm_reverse=lambda can: 1 - can["R1", 0],
                    inverse=lambda can: 1 - can["R1", 0],
                    nodes=1)),             # U A | M without backward_from_output | K alone: a run of one is no node
    "kernel_sizes": dict(
        layers=["U2", "A", "U5", "A"], image=(16, 8, 8), batch=BATCH, context=None,
        expect=dict(F=lambda can: can["F", 0] + can["F", 2],
                    F_runs=lambda can: can["F", 0] + can["F", 2],
                    R1=lambda can: can["R1", 0] + can["R1", 2],
                    R2=0, R3=0, mix_reverse=0,
                    actnorm_reverse=lambda can: 2 - can["R1", 0] - can["R1", 2],
                    inverse=lambda can: 2 - can["R1", 0] - can["R1", 2],
                    nodes=1)),
    "padded_convs": dict(
        layers=["P:TL", "A", "P:BR:bias", "A"], image=(8, 8, 8), batch=BATCH, context=None,
        expect=dict(F=0, F_runs=0, R1=0, R2=0, R3=0,  # a PaddedConv2d is not a FastFlowUnit
                    mix_reverse=0, actnorm_reverse=2, inverse=2,
                    nodes=1)),
    "with_context": dict(
        layers=["U", "A", "M", "Kc", "A", "M", "Kc"], image=(12, 8, 8), batch=BATCH, context=N_CONTEXT,
        expect=dict(F=1, F_runs=1,
                    R1=lambda can: can["R1", 0],
                    R2=0,                  # small set
                    R3=1,                  # the second block's M -> A has a Coupling behind it; the first block's is barred
                    mix_reverse=1,         # the first block's
                    actnorm_reverse=lambda can: 1 - can["R1", 0],
                    inverse=lambda can: 1 - can["R1", 0],
                    nodes=1)),
    "tied_modules": dict(
        layers=["U", "A", "M", "=0", "=1", "=2"], image=(12, 8, 8), batch=BATCH, context=None,
        expect=dict(F=2, F_runs=2,
                    R1=lambda can: 2 * can["R1", 0],
                    R2=0, R3=0,
                    mix_reverse=2,
                    actnorm_reverse=lambda can: 2 - 2 * can["R1", 0],
                    inverse=lambda can: 2 - 2 * can["R1", 0],
                    nodes=1)),
    "frozen_prefix": dict(
        layers=["U", "A", "M", "K", "U", "A", "M", "K"], image=(16, 8, 8), batch=BATCH, context=None, frozen=(0, 1, 2, 3),
        expect=dict(F=2, F_runs=2,
                    R1=lambda can: can["R1", 0] + can["R1", 4],
                    R2=0, R3=0,
                    mix_reverse=2,
                    actnorm_reverse=lambda can: 2 - can["R1", 0] - can["R1", 4],
                    inverse=lambda can: 2 - can["R1", 0] - can["R1", 4],
                    nodes=1)),             # one run of eight; its backward stops in front of the frozen four when x wants nothing
}

COUNTED = ("F", "F_runs", "R1", "R2", "R3", "mix_reverse", "actnorm_reverse", "inverse", "nodes")


def expected(case, can):
    """The case's counts with the capability answers `can` put in."""
    return {k: (v(can) if callable(v) else v) for k, v in case["expect"].items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# orders as data
# ---------------------------------------------------------------------------------------------------------------------------------
def resolved(layers):
    """The codes with every "=k" replaced by the code it repeats."""
    out = []
    for code in layers:
        out.append(out[int(code[1:])] if code.startswith("=") else code)
    return out


def shapes(case):
    """[(C, H, W) of the INPUT of every layer] + [(C, H, W) of the stack's output], tracked from the codes; asserts that the order
    is valid (a unit needs C % 4 == 0, a coupling an even C, a Squeeze an even map)."""
    c, h, w = case["image"]
    out = []
    for code in resolved(case["layers"]):
        out.append((c, h, w))
        if code in UNITS:
            assert c % 4 == 0, (code, c)
        elif code in ("K", "Kc", "Z"):
            assert c % 2 == 0, (code, c)
        if code == "S":
            assert h % 2 == 0 and w % 2 == 0, (h, w)
            c, h, w = c * 4, h // 2, w // 2
        elif code == "Z":
            c //= 2
    return out + [(c, h, w)]


def eligible_sites(order):
    """From the order alone (forward order, codes): the number of places where each fold COULD fire, whatever the shapes and the
    batch -- an upper bound of what one pass fires."""
    fwd = resolved(order)
    rev = fwd[::-1]
    at = lambda seq, i: seq[i] if i < len(seq) else None
    n = dict(F=0, R1=0, R2=0, R3=0)
    for i in range(len(fwd)):
        n["F"] += fwd[i] in UNITS and at(fwd, i + 1) == "A"
        n["R1"] += rev[i] == "A" and at(rev, i + 1) in UNITS
        n["R2"] += rev[i] == "M" and (at(rev, i + 1) in UNITS or (at(rev, i + 1) == "A" and at(rev, i + 2) in UNITS))
        n["R3"] += rev[i] == "M" and at(rev, i + 1) == "A" and at(rev, i + 2) not in UNITS
    return n


def random_stacks(seed, n):
    """`n` valid cases of 4 to 9 layers from a seeded generator, named "random_<seed>_<k>".  The map starts at [4, 12, 8, 8]; the
    channel count and the map are tracked: a unit where C % 4 == 0 (the 2x2 and 5x5 ones on the 8x8 map only), a Squeeze while H and W
    are even and at least 4, at most one SplitPrior.  A stack either has a context -- then its couplings are Kc, on the 8x8 map the
    context has, and there is no SplitPrior (its coupling takes no context) -- or has none."""
    rng = random.Random(seed)
    pool = ["U"] * 5 + ["A"] * 6 + ["M"] * 5 + ["K"] * 3 + ["S", "S", "Z", "X", "P:TL", "P:BR:bias", "U2", "U5"]
    out = {}
    for k in range(n):
        context = N_CONTEXT if rng.random() < 0.2 else None
        c, h, w = 12, 8, 8
        layers, split = [], False
        want = rng.randint(4, 9)
        while len(layers) < want:
            code = rng.choice(pool)
            if code in UNITS and (c % 4 or (code != "U" and h != 8)):
                continue
            if code in ("X", "P:TL", "P:BR:bias") and c > 48:
                continue
            if code == "K":
                if c % 2 or (context is not None and h != 8):
                    continue
                code = "K" if context is None else "Kc"
            if code == "Z":
                if split or context is not None or c % 2:
                    continue
                split = True
            if code == "S" and (h % 2 or w % 2 or h < 4 or w < 4):
                continue
            layers.append(code)
            if code == "S":
                c, h, w = c * 4, h // 2, w // 2
            elif code == "Z":
                c //= 2
        out["random_%d_%d" % (seed, k)] = dict(layers=layers, image=(12, 8, 8), batch=BATCH, context=context)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# orders as modules
# ---------------------------------------------------------------------------------------------------------------------------------
def build(case, seed=0):
    """The case as a `FlowSequential` on the CPU under a standard-normal base: coupling nets and ActNorms filled by
    `flow_twin.randomise(actnorm=True)`, every Conv1x1's W moved off its orthogonal start as tests/test_gpu_sample_logdet.py's
    `build_model` does (log|det W| of an orthogonal matrix is 0 and a dropped mix term would not show), a PaddedConv2d's own bias off
    zero; asserts that every ActNorm's and every mix's own log-det is beyond 0.1."""
    import numpy as np
    import torch

    import flow_twin
    from fincflow_amd import CINCFlowUnit, FastFlowUnit, FlowSequential, PaddedConv2d, glow
    torch.manual_seed(seed)
    np.random.seed(seed)
    sizes = shapes(case)
    mods = []
    for code, (c, h, w) in zip(case["layers"], sizes):
        if code.startswith("="):
            m = mods[int(code[1:])]
        elif code in UNITS:
            m = FastFlowUnit(c, c, (KERNEL[code],) * 2)
        elif code == "X":
            m = CINCFlowUnit(c, c, (KERNEL[code],) * 2)
        elif code.startswith("P:"):
            m = PaddedConv2d(c, c, (3, 3), bias=code.endswith(":bias"), order=code.split(":")[1])
        elif code == "A":
            m = glow.ActNorm(c)
        elif code == "M":
            m = glow.Conv1x1(c)
        elif code in ("K", "Kc"):
            m = glow.Coupling((c, h, w), width=WIDTH, n_context=N_CONTEXT if code == "Kc" else None)
        elif code == "S":
            m = glow.Squeeze()
        else:
            assert code == "Z", code
            m = glow.SplitPrior((c, h, w), glow.GaussianPrior, width=WIDTH)
        mods.append(m)
    model = flow_twin.randomise(FlowSequential(glow.GaussianPrior(sizes[-1]), *mods), seed=seed + 1, actnorm=True)
    gen = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        for code, m, (c, h, w) in zip(case["layers"], mods, sizes):
            if code.startswith("="):
                continue
            if isinstance(m, glow.Conv1x1):
                m.W.mul_(1.1).add_(0.05 * torch.randn(m.W.shape, generator=gen))
                assert abs(float(torch.slogdet(m.W)[1])) * h * w > 0.1, code
            elif isinstance(m, glow.ActNorm):
                assert abs(float(m.log_scale.sum())) * h * w > 0.1, code
            elif isinstance(m, PaddedConv2d) and m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
    for k in case.get("frozen", ()):
        mods[k].requires_grad_(False)
    return model


def inputs(case, n=BATCH, seed=4):
    """(x [n, C, H, W], the context [n, 3, H, W] or None): float32 on the CPU, seeded."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, *case["image"], generator=gen)
    ctx = None if case["context"] is None else torch.randn(n, case["context"], *case["image"][1:], generator=gen)
    return x, ctx
