"""tests/stack_cases.py without a GPU: every order builds and its shapes chain, the float64 twin of tests/flow_twin.py -- the reference
tests/test_gpu_stack_orders.py holds the HIP model to -- is consistent with itself on every order (reverse(forward(x)) == x, and the
log-det `_reverse_chain(with_logdet=True)` sums is the one `_forward_layers` sums), the random orders reach every fold, and the
counter of eligible sites bounds the hand-stated counts.

Bar of the twin's self-consistency: 1e-12 in helpers.rel_err (float64 round-off over at most 9 layers; six hand-made orders gave
1.8e-15 at most).

What this found: `_forward_layers` summed the log-dets in place into the first layer's, and a Conv1x1's is 0-dim -- a stack that
STARTS with a mix followed by anything with a per-image log-det (M A U, `reversed_block`) raised in `log_prob` on every device.
"""
import numpy as np
import pytest
import torch

import flow_twin
import stack_cases
from helpers import rel_err
from stack_cases import CASES, COUNTED, FULL_CHIP, KERNEL, UNITS, eligible_sites, random_stacks, resolved, shapes

SELF_TOL = 1e-12
RANDOM = random_stacks(0, 24)
EVERY = dict(CASES, **RANDOM)


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's answers for a case (also used by tests/test_gpu_stack_orders.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def unit_dims(case):
    """forward index -> (Cq, H, W, KH, KW) of every FastFlowUnit of the case."""
    return {i: (c // 4, h, w, KERNEL[code], KERNEL[code]) for i, (code, (c, h, w)) in enumerate(zip(resolved(case["layers"]), shapes(case)))
            if code in UNITS}


def full_chip_batch(case):
    """The smallest batch for which the library takes the premultiplied inverse of the case's first unit, found as
    tests/test_gpu_train_loop.py::test_sampling_on_the_premultiplied_fold finds it."""
    from fincflow_amd import _lib
    dims = unit_dims(case)[0]
    n = next(b for b in range(1, 1025) if _lib.lib().finc_inverse_premultiplied_supported(b, 4, *dims))
    assert n > stack_cases.BATCH and not _lib.lib().finc_inverse_premultiplied_supported(n - 1, 4, *dims)
    return n


def sampling_batch(case):
    return full_chip_batch(case) if case["batch"] == FULL_CHIP else case["batch"]


def capabilities(case):
    """`can` of tests/stack_cases.py: what the library's capability queries answer for every unit of the case, the batch-dependent
    ones at the case's sampling batch."""
    from fincflow_amd import _lib
    L, n, can = _lib.lib(), sampling_batch(case), {}
    for i, dims in unit_dims(case).items():
        can["F", i] = int(L.finc_forward_algo_for(*dims) == _lib.ALGO["mfma"])
        can["R1", i] = int(L.finc_inverse_algo_for(*dims) == _lib.ALGO["mfma"] and bool(L.finc_inverse_affine_supported(n, 4, *dims)))
        can["R2", i] = int(bool(L.finc_inverse_premultiplied_supported(n, 4, *dims)))
    return can


def test_the_premises_about_the_mix_kernel():
    from fincflow_amd import ops
    assert all(ops.mix_supported(c) for c in (8, 12, 16)) and not ops.mix_supported(20)


# ---------------------------------------------------------------------------------------------------------------------------------
# well-formed cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EVERY))
def test_the_case_builds_and_its_shapes_chain(name):
    from fincflow_amd import FastFlowUnit, glow
    case = EVERY[name]
    sizes = shapes(case)
    assert 2 <= len(case["layers"]) <= 9 and len(sizes) == len(case["layers"]) + 1
    model = stack_cases.build(case)
    mods = list(model)
    assert len(mods) == len(case["layers"]) and tuple(model.base_distribution.size) == sizes[-1]
    x, ctx = stack_cases.inputs(case)
    assert tuple(x.shape) == (stack_cases.BATCH,) + tuple(case["image"]) and (ctx is None) == (case["context"] is None)
    for k, (code, m) in enumerate(zip(case["layers"], mods)):
        if code.startswith("="):
            assert m is mods[int(code[1:])]
        else:
            assert all(m is not other for other in mods[:k])
        assert isinstance(m, FastFlowUnit) == (resolved(case["layers"])[k] in UNITS)
        assert all(p.requires_grad == (k not in case.get("frozen", ())) for p in m.parameters()) or code.startswith("=")
        if isinstance(m, glow.ActNorm):
            assert m.n_dims == sizes[k][0] and m._is_initialized()
    if name in CASES:
        assert set(case["expect"]) == set(COUNTED), name
        assert all(c == 20 or c in (8, 12, 16) for code, (c, _, _) in zip(resolved(case["layers"]), sizes) if code == "M"), name
    # the shapes chain: the float32 layers run one after the other on the CPU (the units on the twin's formulas)
    twin = flow_twin.twin_of(model, torch.float32)
    with torch.no_grad():
        h = x
        for m, size in zip(twin, sizes):
            assert tuple(h.shape[1:]) == size, (name, tuple(h.shape), size)
            h = m(h, ctx)[0]
    assert tuple(h.shape[1:]) == sizes[-1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference is sound on every order
# ---------------------------------------------------------------------------------------------------------------------------------
def factored_out(twin):
    """A list that receives what every SplitPrior of `twin` hands to its base in `forward`: the half it factors out."""
    from fincflow_amd import glow
    halves = []
    for m in twin.modules():
        if isinstance(m, glow.SplitPrior):
            def log_prob(x, context=None, _base=m.base):
                halves.append(x.detach().clone())
                return type(_base).log_prob(_base, x, context)
            m.base.log_prob = log_prob
    return halves


def round_trip(case):
    twin = flow_twin.twin_of(stack_cases.build(case))
    x, ctx = stack_cases.inputs(case)
    x, ctx = x.double(), None if ctx is None else ctx.double()
    halves = factored_out(twin)
    with torch.no_grad():
        z, ld_forward = twin._forward_layers(list(twin), x, ctx)
        for m in twin.modules():
            m.__dict__.pop("log_prob", None)
        with flow_twin.replayed_noise(twin, halves[::-1]):          # the reverse chain meets the split priors last to first
            back, ld_reverse = twin._reverse_chain(z, ctx, with_logdet=True)
    ld_forward = torch.as_tensor(ld_forward, dtype=torch.float64).expand(len(x))
    assert ld_reverse.shape == (len(x),) and float(ld_forward.abs().max()) > 0.1
    return rel_err(back.numpy(), x.numpy()), rel_err(ld_reverse.numpy(), ld_forward.numpy())


@pytest.mark.parametrize("name", list(EVERY))
def test_the_float64_twin_is_self_consistent(name):
    e_x, e_ld = round_trip(EVERY[name])
    print("%s %s: reverse(forward(x)) %.1e, log-det of the reverse pass against the forward's %.1e" % (name, EVERY[name]["layers"], e_x, e_ld))
    assert e_x <= SELF_TOL and e_ld <= SELF_TOL, (name, e_x, e_ld)


# ---------------------------------------------------------------------------------------------------------------------------------
# the random orders, and the counter of sites
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_random_orders_are_seeded_and_reach_every_fold():
    again = random_stacks(0, 24)
    assert list(again) == list(RANDOM) and all(again[k] == RANDOM[k] for k in RANDOM) and random_stacks(1, 24) != {
        k.replace("random_0", "random_1"): v for k, v in RANDOM.items()}
    assert len(RANDOM) == 24 and all(4 <= len(c["layers"]) <= 9 and c["layers"].count("Z") <= 1 for c in RANDOM.values())
    total = dict(F=0, R1=0, R2=0, R3=0)
    for case in RANDOM.values():
        for k, v in eligible_sites(case["layers"]).items():
            total[k] += v
    print("sites over the 24 random orders:", total)
    assert total["F"] >= 3 and total["R1"] >= 3 and total["R3"] >= 3 and total["R2"] >= 1, total


def test_eligible_sites_on_orders_counted_by_hand():
    assert eligible_sites(["U", "A", "M", "K"]) == dict(F=1, R1=1, R2=1, R3=0)
    assert eligible_sites(["S", "A", "M", "K", "A", "M", "K"]) == dict(F=0, R1=0, R2=0, R3=2)
    assert eligible_sites(["U", "M"]) == dict(F=0, R1=0, R2=1, R3=0)
    assert eligible_sites(["A", "M"]) == dict(F=0, R1=0, R2=0, R3=1)
    assert eligible_sites(["U5", "A", "A", "X", "A", "M"]) == dict(F=1, R1=1, R2=0, R3=1)
    assert eligible_sites(["U", "A", "M", "=0", "=1", "=2"]) == dict(F=2, R1=2, R2=2, R3=0)


@pytest.mark.parametrize("name", list(CASES))
def test_the_hand_stated_counts_stay_under_the_eligible_sites(name):
    case = CASES[name]
    want, sites = stack_cases.expected(case, capabilities(case)), eligible_sites(case["layers"])
    assert all(isinstance(v, int) and v >= 0 for v in want.values()), want
    assert all(want[k] <= sites[k] for k in sites) and want["F_runs"] <= sites["F"], (name, want, sites)
    # every layer of the reverse chain is taken exactly once: by a fold or by its own reverse
    codes = resolved(case["layers"])
    assert want["R2"] + want["R3"] + want["mix_reverse"] == codes.count("M"), name
    taken = want["R1"] + want["R3"] + want["actnorm_reverse"]                # (R2 takes an ActNorm with it, or none)
    assert taken <= codes.count("A") <= taken + want["R2"], name
    assert want["R1"] + want["R2"] + want["inverse"] == sum(c in UNITS or c == "X" or c.startswith("P:") for c in codes), name
