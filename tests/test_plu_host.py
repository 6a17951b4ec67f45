"""Host side of the PLU-parametrised 1x1 convolution (include/finc.h: finc_plu_supported_f32, finc_plu_compose_f32,
finc_plu_compose_backward_f32): the exported symbols and the ABI version gate, the refusal order of the two entry points
with fake pointers, and `glow.Conv1x1LU` on CPU tensors in float32 and float64, where it runs its PyTorch lines -- against float64
autograd through the written-out composition, `torch.slogdet` and `torch.inverse` (tests/plu_cases.py).  No GPU needed, the library
built."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library, rel_err
from plu_cases import BAR, factors, judge, leaves64, make_layer, ref64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("finc_plu_supported_f32", "finc_plu_compose_f32", "finc_plu_compose_backward_f32")
CAP = 512
DTYPES = (torch.float32, torch.float64)


def test_the_three_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name, nargs in zip(ENTRIES, (1, 10, 12)):
        assert name in _lib.SYMBOLS and name + "(" in header, name
        assert len(getattr(L, name).argtypes) == nargs, name
    from fincflow_amd import glow, ops
    for name in ("plu_supported", "finc_plu_compose", "finc_plu_compose_backward", "plu_compose"):
        assert callable(getattr(ops, name)), name
    assert issubclass(glow.Conv1x1LU, glow.Conv1x1) and callable(glow.convert_conv1x1)


def test_version_is_118_and_a_117_library_is_told_to_rebuild(tmp_path):
    assert _lib.PLU_ABI_VERSION == 118
    assert _lib.lib().finc_version() >= _lib.PLU_ABI_VERSION
    out = load_stub_library(tmp_path, 117)
    assert "= 117" in out and "118" in out and "rebuild it" in out and "finc_plu_compose_f32" in out, out
    assert "finc_plu_compose_backward_f32" in out, out


def test_the_widths_the_kernels_take():
    L = _lib.lib()
    assert [L.finc_plu_supported_f32(C) for C in (-1, 0, 1, 20, CAP, CAP + 1, 1 << 30)] == [0, 0, 1, 1, 1, 0, 0]
    from fincflow_amd import ops
    assert ops.plu_supported(7) and not ops.plu_supported(CAP + 1)


def test_refusal_order_of_compose():
    """NULL -> 1, C < 1 or an output that shares a byte with an input or another output -> 2, alignment (4 bytes, perm included) -> 7,
    a width without a kernel -> 3; there is no workspace."""
    fn = _lib.lib().finc_plu_compose_f32
    C = 12                                                       # a matrix: 576 bytes, a vector: 48; the fake pointers lie 256 MiB apart
    base = dict(lower=0x10000000, upper=0x20000000, log_s=0x30000000, sign_s=0x40000000, perm=0x50000000, w=0x60000000,
                w_inv=0x70000000, logdet=0x80000000)

    def f(C=C, **kw):
        a = dict(base, **kw)
        return fn(*(None if a[k] is None else _p(a[k]) for k in base), C, None)
    for name in ("lower", "upper", "log_s", "sign_s", "perm"):
        assert f(**{name: None}) == 1, name
    assert f(w=None, w_inv=None, logdet=None) == 1
    assert f(lower=None, C=0) == 1                                # (NULL comes before the dims)
    for bad in (0, -1, -(1 << 31)):
        assert f(C=bad) == 2, bad
    for out, size in (("w", 576), ("w_inv", 576), ("logdet", 4)):
        for name, n in (("lower", 576), ("upper", 576), ("log_s", 48), ("sign_s", 48), ("perm", 48)):
            assert f(**{out: base[name]}) == 2, (out, name)
            assert f(**{out: base[name] + n - 4}) == 2, (out, name)              # the input's last dword
            assert f(**{out: base[name] - size + 4}) == 2, (out, name)           # the output's last dword on the input's first
            assert f(**{out: base[name] + n + 2}) == 7, (out, name)              # (one past: no longer this input, on to the alignment)
    assert f(w_inv=base["w"]) == 2 and f(w_inv=base["w"] + 572) == 2 and f(logdet=base["w_inv"] + 572) == 2
    assert f(w=0x60000002, C=0) == 2                                # (dims come before the alignment)
    for name in base:
        assert f(**{name: base[name] + 2}) == 7, name
        assert f(**{name: base[name] + 1}) == 7, name
        assert f(**{name: base[name] + 4}, C=CAP + 1) == 3, name  # on 4 bytes: accepted, on to the width
    assert f(w=0x60000002, C=CAP + 1) == 7                          # (alignment comes before the width)
    for wide in (CAP + 1, 4096):
        assert f(C=wide) == 3, wide
    for only in ("w", "w_inv", "logdet"):                         # each output alone is a call
        kw = dict(w=None, w_inv=None, logdet=None)
        kw[only] = base[only]
        assert f(C=CAP + 1, **kw) == 3, only


def test_refusal_order_of_the_backward():
    fn = _lib.lib().finc_plu_compose_backward_f32
    C = 12
    base = dict(gw=0x10000000, gld=0x18000000, lower=0x20000000, upper=0x30000000, log_s=0x40000000, sign_s=0x50000000,
                perm=0x60000000, gl=0x70000000, gu=0x80000000, gs=0x90000000)

    def f(C=C, **kw):
        a = dict(base, **kw)
        return fn(*(None if a[k] is None else _p(a[k]) for k in base), C, None)
    for name in ("gw", "lower", "upper", "log_s", "sign_s", "perm"):
        assert f(**{name: None}) == 1, name
    assert f(gl=None, gu=None, gs=None) == 1
    assert f(gw=None, C=0) == 1
    for bad in (0, -3):
        assert f(C=bad) == 2 and f(C=bad, gld=None) == 2, bad
    for out, size in (("gl", 576), ("gu", 576), ("gs", 48)):
        for name, n in (("gw", 576), ("gld", 4), ("lower", 576), ("upper", 576), ("log_s", 48), ("sign_s", 48), ("perm", 48)):
            assert f(**{out: base[name]}) == 2, (out, name)
            assert f(**{out: base[name] + n - 4}) == 2, (out, name)
            assert f(**{out: base[name] - size + 4}) == 2, (out, name)
    assert f(gu=base["gl"]) == 2 and f(gs=base["gu"] + 572) == 2 and f(gs=base["gl"]) == 2
    assert f(gl=0x70000002, C=0) == 2
    for name in base:
        assert f(**{name: base[name] + 2}) == 7, name
        assert f(**{name: base[name] + 4}, C=CAP + 1) == 3, name
    assert f(gs=0x90000002, C=CAP + 1) == 7
    assert f(C=CAP + 1) == 3 and f(C=CAP + 1, gld=None) == 3 and f(C=4096) == 3
    for only in ("gl", "gu", "gs"):
        kw = dict(gl=None, gu=None, gs=None)
        kw[only] = base[only]
        assert f(C=CAP + 1, **kw) == 3, only


def test_the_new_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    for name in ("finc_plu_compose_kernel", "finc_plu_compose_bwd_kernel"):
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == 1, (name, sorted(ks))
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer on CPU tensors: its PyTorch lines
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("float32", "float64"))
@pytest.mark.parametrize("C", (1, 4, 12, 20, 48))
def test_the_layer_on_the_cpu(C, dtype):
    m = make_layer(C).to(dtype)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(3, C, 4, 5, generator=g).to(dtype)
    gz, gld = torch.randn(3, C, 4, 5, generator=g), torch.randn(3, generator=g)
    tag = dict(C=C, dtype=str(dtype), where="cpu")
    with torch.no_grad():
        z, ldj = m(x)
        back = m.reverse(z)
        back2, ldj2 = m.reverse_with_logdet(z)
    assert z.dtype == dtype and ldj.dim() == 0
    lower, upper, log_s, sign_s, perm = leaves64(m)
    w64, w_inv64, ld64 = ref64(lower, upper, log_s, sign_s, perm)
    judge("cpu/forward", ["z", "ldj", "ldj == H W sum(log_s)", "reverse(forward)", "reverse_with_logdet"],
          [z, ldj, ldj, back, ldj2], [torch.einsum("oi,bihw->bohw", w64, x.double()), 20 * ld64, 20 * log_s.sum(), x, (20 * ld64).expand(3)],
          **tag)
    assert torch.equal(back, back2)
    judge("cpu/dense", ["W", "slogdet(dense)", "inverse(dense)"],
          [m.dense(), torch.slogdet(m.dense().double())[1] * 20, m._inverse_matrix()], [w64, ldj.double(), w_inv64], **tag)
    # gradients against autograd through dense()
    x_in = x.clone().requires_grad_(True)
    z, ldj = m(x_in)
    got = torch.autograd.grad((z * gz.to(dtype)).sum() + (ldj.expand(3) * gld.to(dtype)).sum(), [x_in] + list(m.parameters()))
    x64 = x.double().requires_grad_(True)
    z64 = torch.einsum("oi,bihw->bohw", w64, x64)
    want = torch.autograd.grad((z64 * gz.double()).sum() + (20 * ld64 * gld.double()).sum(), [x64, lower, upper, log_s])
    judge("cpu/gradients", ["grad_x", "grad_lower", "grad_upper", "grad_log_s"], got, want, **tag)
    assert not bool(got[1].triu(0).any()) and not bool(got[2].tril(0).any())        # the masked entries: exact zeros
    # a recorded reverse
    z_in = x.clone().requires_grad_(True)
    got = torch.autograd.grad((m.reverse(z_in) * gz.to(dtype)).sum(), [z_in] + list(m.parameters()))
    z64 = x.double().requires_grad_(True)
    want = torch.autograd.grad((torch.einsum("oi,bihw->bohw", ref64(lower, upper, log_s, sign_s, perm)[1], z64) * gz.double()).sum(),
                               [z64, lower, upper, log_s])
    judge("cpu/reverse_gradients", ["grad_z", "grad_lower", "grad_upper", "grad_log_s"], got, want, **tag)


@pytest.mark.parametrize("C", (12, 96, 192))
def test_one_seed_gives_both_layers_the_same_matrix(C):
    from fincflow_amd import glow
    np.random.seed(5)
    a = glow.Conv1x1(C)
    np.random.seed(5)
    b = glow.Conv1x1LU(C)
    assert b.lower.dtype == b.upper.dtype == b.log_s.dtype == b.sign_s.dtype == torch.float32 and b.perm.dtype == torch.int32
    assert set(b.sign_s.tolist()) <= {1.0, -1.0} and sorted(b.perm.tolist()) == list(range(C))
    assert not bool(b.lower.detach().triu(0).any()) and not bool(b.upper.detach().tril(0).any())
    judge("cpu/same_seed", ["W"], [b.dense()], [a.W.detach()], C=C)
    assert [n for n, _ in b.named_parameters()] == ["lower", "upper", "log_s"] and [n for n, _ in b.named_buffers()] == ["sign_s", "perm"]
    with pytest.raises(AttributeError):
        b.W = torch.eye(C)                                                          # read-only


def test_from_dense_reproduces_the_layer_and_keeps_the_dtype():
    from fincflow_amd import glow
    m = make_layer(48)
    again = glow.Conv1x1LU.from_dense(m.dense())
    judge("cpu/from_dense(dense())", ["W", "W^-1"], [again.dense(), again._inverse_matrix()], [m.dense().double(), torch.inverse(m.dense().double())])
    assert again.lower.dtype == torch.float32 and glow.Conv1x1LU.from_dense(m.dense().double()).lower.dtype == torch.float64
    assert glow.Conv1x1LU.from_dense(m.dense().detach().numpy()).n_channels == 48
    with pytest.raises(ValueError):
        glow.Conv1x1LU.from_dense(torch.zeros(4, 4))
    with pytest.raises(ValueError):
        glow.Conv1x1LU.from_dense(torch.zeros(4, 5))


def test_state_dict_round_trip_and_a_bad_permutation():
    from fincflow_amd import glow
    m = make_layer(12)
    sd = m.state_dict()
    assert list(sd) == ["lower", "upper", "log_s", "sign_s", "perm"] and sd["perm"].dtype == torch.int32
    other = make_layer(12, seed=3)
    with torch.no_grad():
        before = other(torch.ones(1, 12, 2, 2))[0]
    other.load_state_dict(sd)
    with torch.no_grad():
        x = torch.randn(2, 12, 3, 3)
        assert torch.equal(other(x)[0], m(x)[0]) and torch.equal(other(x)[1], m(x)[1])       # (and no derived value of the old ones)
        assert not torch.equal(other(torch.ones(1, 12, 2, 2))[0], before)
    for bad in (sd["perm"].clone().fill_(0), torch.cat([sd["perm"][:-1], torch.tensor([12], dtype=torch.int32)]),
                torch.cat([sd["perm"][:-1], torch.tensor([-1], dtype=torch.int32)]), sd["perm"][:-1], sd["perm"].float() + 0.5):
        with pytest.raises(ValueError):
            other.load_state_dict(dict(sd, perm=bad))
        layer = glow.Conv1x1LU(12)
        with pytest.raises(ValueError):
            layer._set_factors((m.lower.detach(), m.upper.detach(), m.log_s.detach(), m.sign_s, bad), torch.float32)
    with torch.no_grad():
        assert torch.equal(other(x)[0], m(x)[0])                                    # a refused load changed nothing


def test_copies_start_without_derived_values():
    m = make_layer(12)
    with torch.no_grad():
        x = torch.randn(2, 12, 3, 3)
        z = m(x)[0]
        m.reverse(z)
    assert "_plu" in m.__dict__ and "_plu_key" in m.__dict__
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert not any(k in clone.__dict__ for k in type(m)._derived)
        with torch.no_grad():
            clone.log_s.add_(0.25)
            assert not torch.equal(clone(x)[0], z) and torch.equal(m(x)[0], z)


def test_convert_conv1x1_both_ways_keeps_log_prob():
    from fincflow_amd import glow
    import flow_twin
    torch.manual_seed(0)
    np.random.seed(0)
    model = flow_twin.randomise(glow.create_model(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 8, 8),
                                                  coupling_width=8, preprocess=False), actnorm=True)
    twin = flow_twin.twin_of(model, torch.float32)             # a CPU model: the units on the reference formulas
    x = torch.randn(3, 3, 8, 8, generator=torch.Generator().manual_seed(2))
    count = lambda cls: sum(type(m) is cls for m in twin.modules())
    with torch.no_grad():
        want = twin.log_prob(x)
        assert (count(glow.Conv1x1), count(glow.Conv1x1LU)) == (2, 0)
        assert glow.convert_conv1x1(twin, "lu") is twin and (count(glow.Conv1x1), count(glow.Conv1x1LU)) == (0, 2)
        assert all(type(m) is not glow.Conv1x1 for m in twin.sequence_modules) and all(m in list(twin.children()) for m in twin.sequence_modules)
        lu = twin.log_prob(x)
        glow.convert_conv1x1(twin, "dense")
        assert (count(glow.Conv1x1), count(glow.Conv1x1LU)) == (2, 0)
        dense = twin.log_prob(x)
    judge("cpu/convert", ["log_prob(lu)", "log_prob(dense again)"], [lu, dense], [want, want])
    names = [n for n, _ in twin.named_parameters()]
    assert names == [n for n, _ in model.named_parameters()]   # the dense model has its old state dict
    with pytest.raises(ValueError):
        glow.convert_conv1x1(twin, "qr")
    default = glow.create_model(num_blocks=1, block_size=1, image_size=(3, 4, 4), coupling_width=8)
    assert not any(isinstance(m, glow.Conv1x1LU) for m in default.modules())
    lu_model = glow.create_model(num_blocks=1, block_size=1, image_size=(3, 4, 4), coupling_width=8, lu_conv1x1=True)
    assert sum(isinstance(m, glow.Conv1x1LU) for m in lu_model.modules()) == 1
