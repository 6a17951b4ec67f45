"""Host side of the merges' backward (include/finc.h: finc_split_prior_merge_backward_f32, its _rawbf16_f32 sibling and
finc_gauss_split_merge_backward_f32): the exported symbols and the ABI version gate, the refusal order of the three entry
points with fake pointers, the new kernels' register allocation, and the `hip_recorded_merge` switch of `glow.SplitPrior` /
`glow.Split` on CPU float64 tensors, where it is inert.  No GPU needed, the library built."""
import os

import pytest
import torch

from fincflow_amd import _lib
from helpers import fake_ptr as _p, load_stub_library

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("finc_split_prior_merge_backward_f32", "finc_split_prior_merge_backward_rawbf16_f32", "finc_gauss_split_merge_backward_f32")
BIG = 1 << 40
DIMS = (2, 12, 64)       # the whole tensor: 2 * 12 * 64 * 4 = 6144 bytes (3072 as bf16), a half one 3072: the fake pointers lie 64 KiB apart


def test_the_three_symbols_are_exported_declared_and_bound():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "finc.h")).read()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and name + "(" in header, name
        assert len(getattr(L, name).argtypes) == 17, name
    from fincflow_amd import ops
    for name in ("finc_split_prior_merge_backward", "finc_gauss_split_merge_backward", "split_prior_merge", "gauss_split_merge"):
        assert callable(getattr(ops, name)), name


def test_version_is_117_and_a_116_library_is_told_to_rebuild(tmp_path):
    assert _lib.MERGE_BACKWARD_ABI_VERSION == 117
    assert _lib.lib().finc_version() >= _lib.MERGE_BACKWARD_ABI_VERSION
    out = load_stub_library(tmp_path, 116)
    assert "= 116" in out and "117" in out and "rebuild it" in out and "finc_split_prior_merge_backward_f32" in out, out
    assert "finc_gauss_split_merge_backward_f32" in out, out


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusal_order(entry):
    """NULL -> 1, bad dims / an output that shares a byte with an input or another output -> 2, alignment (4 bytes; 2 for a bf16 raw
    and grad_raw) -> 7, a channel count without a kernel -> 3, workspace -> 4, in that order."""
    L = _lib.lib()
    bf16 = "rawbf16" in entry
    fn = getattr(L, entry)
    gx, gl, x, raw, a, b = _p(0x100000), _p(0x200000), _p(0x300000), _p(0x400000), _p(0x500000), _p(0x510000)
    g1, gz, gr, ga, gb, ws = _p(0x600000), _p(0x700000), _p(0x800000), _p(0x900000), _p(0x910000), _p(0xa00000)

    def f(gx=gx, gl=gl, x=x, raw=raw, a=a, b=b, g1=g1, gz=gz, gr=gr, ga=ga, gb=gb, dims=DIMS, ws=ws, nbytes=BIG):
        return fn(gx, gl, x, raw, a, b, g1, gz, gr, ga, gb, *dims, ws, nbytes, None)
    for name in ("x", "raw", "a", "b"):
        assert f(**{name: None}) == 1, name
    assert f(gx=None, gl=None) == 1                                          # either incoming gradient may be absent, not both
    assert f(gx=None, ws=None) == 4 and f(gl=None, ws=None) == 4             # (one absent: past the NULL rule, down to the workspace)
    assert f(g1=None, gz=None, gr=None, ga=None, gb=None) == 1               # nothing asked for
    for only in ("g1", "gz", "gr"):                                          # each output alone is a call: without sums, no workspace
        kw = dict(g1=None, gz=None, gr=None, ga=None, gb=None, ws=None, nbytes=0)
        del kw[only]
        assert f(dims=(2, 13, 64), **kw) == 3, only
    assert f(x=None, dims=(0, 12, 64)) == 1                                  # (NULL comes before the dims)
    for dims in ((0, 12, 64), (2, 0, 64), (2, 12, 0), (-1, 12, 64), (2, 12, -3), (2, 1 << 20, 64)):
        assert f(dims=dims) == 2, dims
    # no output on an input or on another output: equal pointers ...
    for out in ("g1", "gz", "gr", "ga", "gb"):
        for alias in (gx, gl, x, raw, a, b):
            assert f(**{out: alias}) == 2, out
    for out, other in (("gz", g1), ("gr", g1), ("gr", gz), ("ga", g1), ("gb", ga), ("gb", gr)):
        assert f(**{out: other}) == 2, (out, other)
    # ... and byte ranges: the last dword of a tensor / the first one behind it (every call here ends in a refusal)
    assert f(g1=_p(0x100000 + 6140)) == 2 and f(g1=_p(0x100000 + 6144), ws=None) == 4         # against grad_x (whole)
    assert f(gz=_p(0x300000 + 6140)) == 2 and f(gz=_p(0x300000 + 6144), ws=None) == 4         # against x (whole)
    assert f(gz=_p(0x600000 + 3068)) == 2 and f(gz=_p(0x600000 + 3072), ws=None) == 4         # against grad_x1 (half)
    assert f(g1=_p(0x100000 - 3068)) == 2 and f(g1=_p(0x100000 - 3072), ws=None) == 4         # a half tensor that runs into grad_x
    raw_bytes = 3072 if bf16 else 6144
    assert f(g1=_p(0x400000 + raw_bytes - 4)) == 2 and f(g1=_p(0x400000 + raw_bytes), ws=None) == 4      # against raw, in ITS bytes
    assert f(gr=_p(0x700000 - raw_bytes + 4)) == 2 and f(gr=_p(0x700000 - raw_bytes), ws=None) == 4      # grad_raw into grad_z2
    assert f(ga=_p(0x500000 + 44)) == 2 and f(ga=_p(0x500000 + 48), ws=None) == 4             # grad_a against a: C floats
    assert f(gb=_p(0x200000 + 4)) == 2 and f(gb=_p(0x200000 + 8), ws=None) == 4               # grad_b against grad_log_p: B floats
    assert f(g1=_p(0x600002), dims=(0, 12, 64)) == 2                         # (dims come before the alignment)
    for name, base in (("gx", 0x100000), ("gl", 0x200000), ("x", 0x300000), ("a", 0x500000), ("b", 0x510000), ("g1", 0x600000),
                       ("gz", 0x700000), ("ga", 0x900000), ("gb", 0x910000)):
        assert f(**{name: _p(base + 2)}) == 7, name                          # misaligned by 2 bytes
        assert f(**{name: _p(base + 4)}, ws=None) == 4, name                 # on 4 bytes: accepted (the narrow form), on to the workspace
    assert f(raw=_p(0x400001)) == 7 and f(gr=_p(0x800001)) == 7
    assert f(raw=_p(0x400002), gr=_p(0x800002), ws=None) == (4 if bf16 else 7)                # a bf16 raw is held to 2 bytes
    assert f(gz=_p(0x700002), dims=(2, 13, 64)) == 7                         # (alignment comes before the channel count)
    for C in (13, 7, 1):
        assert f(dims=(2, C, 64)) == 3, C
        assert f(dims=(2, C, 64), ws=None, nbytes=0) == 3, C                 # (... before the workspace)
    need = L.finc_coupling_workspace_bytes(*DIMS)
    assert f(ws=None) == 4 and f(nbytes=need - 1) == 4 and f(nbytes=0) == 4 and f(ws=_p(0xa00002)) == 4
    assert f(g1=None, gz=None, gr=None, gb=None, nbytes=0) == 4 and f(g1=None, gz=None, gr=None, ga=None, ws=None, nbytes=0) == 4


def test_the_new_kernels_are_in_the_code_objects_without_scratch():
    from test_code_objects import kernel_metadata
    md = kernel_metadata()
    new = ("finc_splitprior_merge_bwd_kernel", "finc_splitprior_merge_rawbf16_bwd_kernel", "finc_gauss_merge_bwd_kernel")
    for name in new:                                                          # V in {4, 1} each
        ks = {k: v for k, v in md.items() if name in k}
        assert len(ks) == 2, (name, sorted(ks))
        for k, v in ks.items():
            assert v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0 and v["scratch"] == 0, (k, v)
    # the counts the older tests pin stay theirs: no new name contains an old one, and the old ones are as many as they were
    old = {"finc_splitprior_kernel": 12, "finc_splitprior_bwd_kernel": 2, "finc_gauss_split_kernel": 6, "finc_gauss_split_bwd_kernel": 2,
           "finc_coupling_reduce_kernel": 1, "finc_coupling_bwd_kernel": 2, "finc_coupling_rev_bwd_kernel": 2,
           "finc_coupling_recon_kernel": 2}
    for name, count in old.items():
        assert len([k for k in md if name in k]) == count, (name, sorted(k for k in md if name in k))
        assert not any(name in n for n in new), name
    bf16 = [k for k in md if "finc_coupling_rawbf16_grad_kernel" in k]
    assert len(bf16) == 8 and not any("ELi4EE" in k for k in bf16), sorted(bf16)             # four modes x V in {4, 1}: no fifth


# ---------------------------------------------------------------------------------------------------------------------------------
# the switch, off the device
# ---------------------------------------------------------------------------------------------------------------------------------
def _randomised(m, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if name.endswith(("bias", "logs", "log_scale_factor")) else 0.05))
    return m.double()


def _layers():
    from fincflow_amd import glow
    return (_randomised(glow.SplitPrior((12, 4, 6), glow.GaussianPrior, width=16)), _randomised(glow.Split((12, 4, 6), glow.GaussianPrior)))


def test_the_switch_is_off_by_default():
    from fincflow_amd import glow
    assert glow.SplitPrior.hip_recorded_merge is False and glow.Split.hip_recorded_merge is False
    kw = dict(num_blocks=2, block_size=1, actnorm=True, preprocess=False, image_size=(3, 8, 8), coupling_width=8, split_prior=True)
    for gauss in (False, True):
        bounds = lambda model: [m for m in model.sequence_modules if isinstance(m, (glow.SplitPrior, glow.Split))]
        default = bounds(glow.create_model(gaussianize_split=gauss, **kw))
        assert len(default) == 1 and default[0].hip_recorded_merge is False and "hip_recorded_merge" not in vars(default[0])
        on = bounds(glow.create_model(gaussianize_split=gauss, hip_recorded_merge=True, **kw))
        assert len(on) == 1 and on[0].hip_recorded_merge is True
        assert type(on[0]) is (glow.Split if gauss else glow.SplitPrior)
        assert list(glow.create_model(gaussianize_split=gauss, hip_recorded_merge=True, **kw).state_dict()) == \
            list(glow.create_model(gaussianize_split=gauss, **kw).state_dict())                # a switch, not a parameter


@pytest.mark.parametrize("which", (0, 1), ids=("SplitPrior", "Split"))
def test_off_the_device_the_switch_is_inert(which):
    """CPU float64 under `reverse_grad()` while a graph is recorded: the bits and the gradients of the flag-off call."""
    from fincflow_amd import ops
    m = _layers()[which]
    g = torch.Generator().manual_seed(3)
    x1 = torch.randn(3, 6, 4, 6, dtype=torch.float64, generator=g)
    z2 = torch.randn(3, 6, 4, 6, dtype=torch.float64, generator=g)
    params = list(m.parameters())

    def run(flag):
        m.hip_recorded_merge = flag
        a, b = x1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        with ops.reverse_grad():
            x, log_p = m.merge(a, b, with_log_prob=True)
            plain = m.merge(a, b)
        loss = (x * x).sum() + (log_p * torch.arange(1.0, 4.0, dtype=torch.float64)).sum()
        return (x.detach(), log_p.detach(), plain.detach()) + torch.autograd.grad(loss, [a, b] + params)
    try:
        off, on = run(False), run(True)
    finally:
        del m.hip_recorded_merge
    assert len(off) == len(on) == 5 + len(params)
    for i, (p, q) in enumerate(zip(off, on)):
        assert torch.equal(p, q), i
    assert all(float(t.abs().max()) > 0 for t in off)
