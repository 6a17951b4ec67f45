"""Whole models against recordings of the reference's own create_model (tests/golden/make_golden_model.py; layout and helpers:
tests/reference_model.py), on the host: the state dict's names, the strict load in both directions, every layer that has a CPU
path on the recorded input of its position, and the recorder's own condition from the stored numbers."""
import json

import numpy as np
import pytest
import torch

import reference_model as rm

NAMES = sorted(rm.MODELS)


# ---------------------------------------------------------------------------------------------------------------------------------
# names
# ---------------------------------------------------------------------------------------------------------------------------------
with open(rm.KEYS_FILE) as _f:
    KEY_LISTS = json.load(_f)


def test_all_twelve_key_lists_are_on_file():
    want = {rm.key_config_name(image, a, s) for image in rm.KEY_IMAGES for a in (False, True) for s in (False, True)}
    assert set(KEY_LISTS) == want and len(want) == 12


@pytest.mark.parametrize("split_prior", [False, True], ids=["nosplit", "split"])
@pytest.mark.parametrize("actnorm", [False, True], ids=["noactnorm", "actnorm"])
@pytest.mark.parametrize("image", rm.KEY_IMAGES, ids=lambda s: "x".join(map(str, s)))
def test_state_dict_names_and_shapes_are_the_references(image, actnorm, split_prior):
    """`create_model` with the reference's arguments (fastflow/fastflow_cifar.py:35-63, its coupling width included): the same
    names with the same shapes in the same order as the reference's own model."""
    from fincflow_amd import glow
    model = glow.create_model(actnorm=actnorm, split_prior=split_prior, image_size=image, **rm.KEY_CONFIG)
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    want = KEY_LISTS[rm.key_config_name(image, actnorm, split_prior)]
    assert [k for k, _ in got] == [k for k, _ in want], sorted({k for k, _ in got} ^ {k for k, _ in want})
    assert got == want


@pytest.mark.parametrize("prefix", ["", "module."], ids=["plain", "data_parallel"])
@pytest.mark.parametrize("name", NAMES)
def test_a_reference_checkpoint_loads_strictly(name, prefix):
    """What the reference's create_model saves -- `0.distribution.empty` of its Dequantization included (layers/distributions/
    uniform.py:14) -- loads with strict=True: nothing missing, nothing unexpected, every tensor where the file has it."""
    from fincflow_amd import load_reference_checkpoint
    model, state = rm.build(name), rm.recorded_state(name, prefix)
    assert any(k.endswith("0.distribution.empty") for k in state)
    result = load_reference_checkpoint(model, {"model_state_dict": state}, strict=True)
    assert list(result.missing_keys) == [] and list(result.unexpected_keys) == []
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[prefix + k]), k


@pytest.mark.parametrize("name", NAMES)
def test_a_checkpoint_saved_here_has_the_references_keys(name):
    """The other direction: the state dict of this project's model has exactly the recorded keys, shapes and dtypes, in order, so
    that the reference's own `load_state_dict(strict=True)` takes a checkpoint written here."""
    model, state = rm.build(name), rm.recorded_state(name)
    ours = model.state_dict()
    assert set(ours) == set(state), sorted(set(ours) ^ set(state))
    assert list(ours) == list(state)
    assert [(tuple(v.shape), v.dtype) for v in ours.values()] == [(tuple(v.shape), v.dtype) for v in state.values()]


# ---------------------------------------------------------------------------------------------------------------------------------
# every layer with a CPU path on the recorded input of its position
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_every_cpu_layer_on_its_recorded_input(name, dtype):
    """Forward (output, log-det, a SplitPrior's factored-out half) and reverse (`SplitPrior.reverse` / `merge` on the recorded
    latent) of every layer but the units, which have no CPU path and are skipped by type.  In float64 against the float64
    recording at 1e-12; in float32 at the recorded bar of the quantity (1e-5 unless the reference's own float32 error asked for
    more, see `test_the_recorders_condition_holds`)."""
    from fincflow_amd import FastFlowUnit, load_reference_checkpoint
    model = rm.build(name)
    load_reference_checkpoint(model, {"model_state_dict": rm.recorded_state(name)}, strict=True)
    if dtype == torch.float64:
        model = model.double()
    errs = rm.layer_walk(model, name, dtype, skip=(FastFlowUnit,))
    n_layers, units = len(model.sequence_modules), sum(isinstance(m, FastFlowUnit) for m in model)
    assert units == 2 and len([q for q in errs if q.endswith(".out") and q.startswith("fwd.")]) == n_layers - units
    assert len([q for q in errs if q.startswith("rev.")]) == n_layers - units
    over = {q: e for q, e in errs.items() if not e <= rm.bar(name, q, dtype == torch.float64)}
    print(name, dtype, "worst", max(errs.items(), key=lambda kv: kv[1]))
    assert not over, over


# ---------------------------------------------------------------------------------------------------------------------------------
# the recorder's condition, from the stored numbers alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_recorders_condition_holds(name):
    """The reference's own float32 result lies within a quarter of the bar every recorded quantity is held to, so that a red test
    is this project's fault.  A bar other than the project's own (1e-5 a layer, 5e-5 through the model) is four times the
    reference's recorded error and only there where that error asked for it.  Where the fixture holds the reference's float32
    tensors (its chain: the log-density, the latents, the gradients, the image in front of the floor, the ActNorm
    initialisation) the stored error is computed again from them."""
    fx, yard = rm.fixture(name), rm.yard(name)
    n_layers = 1 + max(int(k.split(".")[2][1:]) for k in fx if k.startswith("f64.fwd.L"))
    for q, y in yard.items():
        if q == "images":
            continue
        base = rm.base_bar(q)
        assert y["ref32"] <= rm.YARD_SHARE * y["bar"], (q, y)
        assert y["bar"] == base or (y["ref32"] > rm.YARD_SHARE * base and y["bar"] == y["ref32"] / rm.YARD_SHARE), (q, y)
    chain = {"z": "fwd.L%d.out" % (n_layers - 1), "decode.image": "rev.L1.out", "log_prob": "log_prob"}
    chain.update({q: "fwd.L%s.half" % q[len("half.L"):] for q in yard if q.startswith("half.L")})
    chain.update({q: q for q in yard if q.startswith("grad.")})
    for q, src in chain.items():
        assert yard[q]["ref32"] == rm.error(fx["f32." + src], fx["f64." + src]), q
    inits = [q for q in yard if q.startswith("init.")]
    assert inits and all(yard[q]["ref32"] == rm.error(fx["init32." + q[5:]], fx["init64." + q[5:]]) for q in inits)
    # every recorded quantity has its entry
    recorded = {k[len("f64."):] for k in fx if k.startswith("f64.") and k != "f64.rev.L0.out"} | set(inits)
    assert recorded <= set(yard), sorted(recorded - set(yard))
    # the images behind the floor: few pixels left out, and the reference's float32 floor agrees on all the others
    near = rm.near_integer(fx["f64.rev.L1.out"])
    assert near.mean() == yard["images"]["excluded"] <= rm.MAX_EXCLUDED == yard["images"]["bar"]
    assert yard["images"]["ref32_differ"] == 0 and not ((fx["f32.rev.L0.out"] != fx["f64.rev.L0.out"]) & ~near).any()
    assert np.array_equal(fx["f64.rev.L0.out"], np.floor(fx["f64.rev.L1.out"]))


@pytest.mark.parametrize("name", NAMES)
def test_the_recording_is_what_the_issue_asks_for(name):
    """The inputs' range, the tie of Conv2dZero.bias and logs that every reference checkpoint has, parameters away from their
    initial values, the unit-triangular invariant, the latent's temperature."""
    fx = rm.fixture(name)
    assert fx["x"].dtype == np.uint8 and fx["x"].min() == 0 and fx["x"].max() == 255 and len(fx["x"]) == 3 and len(fx["init.x"]) == 8
    assert tuple(fx["x"].shape[1:]) == rm.MODELS[name]["image_size"] == tuple(fx["image"])
    state = rm.recorded_state(name)
    logs = [k for k in state if k.endswith("net.4.logs")]
    assert len(logs) == 3 and all(torch.equal(state[k], state[k[:-4] + "bias"]) and bool(state[k].abs().min() > 0) for k in logs)
    assert all(bool(state[k[:-4] + "weight"].abs().sum() > 0) for k in logs)                  # Conv2dZero is no longer zero
    for k, v in state.items():
        if k.endswith(".W"):
            assert float(torch.linalg.cond(v.double())) < 2.0, k
        if k.endswith("initialized"):
            assert int(v) == 1
    temps = sorted(float(v) for k, v in fx.items() if k.startswith("rev.temperature."))
    assert temps == [0.7]
    for k in fx:
        if k.startswith("rev.eps."):
            assert np.array_equal(fx["rev.z." + k[len("rev.eps."):]], fx[k] * np.float32(0.7))
