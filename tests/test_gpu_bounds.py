"""Guard bands and problem isolation for every kernel family, through the C ABI (include/finc.h).

Two properties no parity case can see, both stated as bit equality with a plain call:

  guard bands   every pointer a call receives sits in its own buffer [NaN guard | payload | NaN guard] (helpers.guarded); the
                workspace, sized exactly what the library asks for, and the outputs start out as NaN as well.  Afterwards every
                guard is intact, the outputs hold no NaN and have the bits of the same call on plain tensors: nothing outside the
                documented extents was written, and nothing outside them (or left over in the workspace) reached the arithmetic.
  isolation     one (image, group) slab -- one pixel, one image, one channel for the per-pixel layers -- of an input is NaN or +inf;
                every output element the operation's definition keeps away from it has the bits of the clean run, and the part it
                does reach holds a NaN (so the poison was read).  The +inf run of the same spot asserts the clean part only: what
                +inf turns into is the operation's business (tanh saturates, 0 * inf appears or not).  max(NaN + b, 0) is 0 on the
                hardware, so finc_bias_relu_f32 is poisoned with +inf alone and must show a non-finite value.

Every case asserts which kernel produced its numbers (the library's own answer), checks once per family that the plain call is
within the project's bar of a float64 reference, and appends a line to the parity report (kinds `bounds` / `isolation`).
Recurrence under test: cinc_cuda_kernel_level2.cu:59-72; forward: fastflow.py:31-50; layers: layers/{conv1x1,coupling,actnorm}.py.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from helpers import (ORIENT_FASTFLOW, actnorm_ref, broken_guards, coupling_ref, guarded, guards_intact, isolation_check, nan_filled, offset_view, poison,
                     problem_counts_for_row, rel_err, report, same_bits, split_problems)
from plan_cases import GRADW_WALK_CASES, ROW_CHUNK_CASES

pytestmark = pytest.mark.gpu

TOL = 1e-5
F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from fincflow_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bank_std(Cq, K):
    return (0.05 if K < 5 else 0.02) * min(1.0, (24.0 / Cq) ** 0.5)


def orient_of(G):
    return ORIENT_FASTFLOW if G == 4 else (0x1B & ((1 << (2 * G)) - 1)) if G < 4 else 0x1BE4


# ---------------------------------------------------------------------------------------------------------------------------------
# one call of the library, on plain tensors or with every pointer inside its own guarded buffer
# ---------------------------------------------------------------------------------------------------------------------------------
class Result:
    def __init__(self):
        self.outs, self.bad, self.nguard, self.ptrs = {}, [], 0, {}


def run(dev, sym, argf, ins, outs, ws=None, guard=False, lead=(), alias=None, lead_floats=1):
    """`sym(*argf(pointers, workspace pointer, workspace bytes))`.  `ins`: name -> device tensor (None = a NULL pointer); `outs`:
    name -> (shape, dtype), NaN on entry; `ws`: workspace bytes (None = NULL), NaN on entry; `lead`: the names that start one float
    into their allocation (the dword forms; `lead_floats` = 2: two, the 8-byte class); `alias`: output name -> the input it is written
    over (the in-place forms).  `guard`: every tensor sits between guards; Result.bad names the guards that were written, Result.nguard
    counts the elements checked; Result.ptrs: the addresses the call was handed."""
    from fincflow_amd import _lib
    res, views, bufs = Result(), {}, []

    def place(name, src):
        if guard:
            v, b = guarded(src, dev, lead_floats if name in lead else 0)
            bufs.append((name, b, v))
            res.nguard += b.numel() - v.numel()
            return v
        return offset_view(src, dev, lead_floats) if name in lead else src.clone()

    for name, src in ins.items():
        views[name] = None if src is None else place(name, src)
    for name, (shape, dtype) in outs.items():
        views[name] = views[alias[name]] if alias and name in alias else place(name, nan_filled(shape, dtype, dev))
    wsv = None
    if ws is not None:
        assert ws % 4 == 0, ws
        wsv = place("workspace", nan_filled((ws // 4,), F32, dev))
    ptr = {k: (None if v is None else v.data_ptr()) for k, v in views.items()}
    with torch.cuda.device(dev):
        st = getattr(_lib.lib(), sym)(*argf(ptr, None if wsv is None else wsv.data_ptr(), ws or 0))
    torch.cuda.synchronize(dev)
    _lib.check(st, sym)
    res.ptrs = ptr
    res.outs = {k: views[k].clone() for k in outs}
    res.bad = ["%s: %s guard written" % (name, side) for name, b, v in bufs for side in broken_guards(b, v)]
    assert all(guards_intact(b, v) == (not broken_guards(b, v)) for _, b, v in bufs)
    return res


def check_bounds(tag, call, variant, judge=None, may_keep_nan=("packed",), **fields):
    """Determinism, (a) guards, (b) output, (c) `judge(plain result)` -> the errors it asserted on; one report line."""
    plain, again = call(False), call(False)
    for k in plain.outs:
        assert same_bits(plain.outs[k], again.outs[k]), (tag, k, "not bit-stable from launch to launch")
    g = call(True)
    assert not g.bad, (tag, variant, g.bad)
    for k in plain.outs:
        assert k in may_keep_nan or not bool(torch.isnan(g.outs[k]).any()), (tag, variant, k, "NaN in the output")
        assert same_bits(g.outs[k], plain.outs[k]), (tag, variant, k, "guarded call differs from the plain call")
    errs = judge(plain) if judge else None
    report("bounds", tag=tag, variant=variant, guard_elements=g.nguard, err=errs, **fields)
    return plain


def check_isolation(dev, tag, call, ins, spots, variant, values=(NAN, INF), **fields):
    """`call(ins)` clean, then once per spot and value with `ins[name][index]` poisoned.  A spot: (input name, index, {output name:
    index of the part the poison may reach, or None when it may reach nothing of that output})."""
    clean = call(ins)
    for k, v in clean.outs.items():
        assert k == "packed" or bool(torch.isfinite(v).all()), (tag, k, "clean run is not finite")
    for name, idx, reaches in spots:
        for val in values:
            dirty = call(dict(ins, **{name: poison(ins[name], idx, val)}))
            for out, ridx in reaches.items():
                reach = torch.zeros(clean.outs[out].shape, dtype=torch.bool, device=dev)
                if ridx is not None:
                    reach[ridx] = True
                leaked, reached = isolation_check(clean.outs[out], dirty.outs[out], reach)
                assert leaked == 0, (tag, variant, name, idx, val, out, "%d elements outside the poisoned problem changed" % leaked)
                if ridx is not None and val is values[0]:
                    assert reached, (tag, variant, name, idx, val, out, "the poison never showed: vacuous")
                    if val != val:
                        assert bool(torch.isnan(dirty.outs[out][reach]).any()), (tag, name, idx, out, "NaN in, no NaN out")
            report("isolation", tag=tag, variant=variant, poisoned=[name, repr(idx)], value=repr(val), **fields)


# ---------------------------------------------------------------------------------------------------------------------------------
# the unit: inverse, forward, backward, their packed forms, fp64
# ---------------------------------------------------------------------------------------------------------------------------------
PACKED = {"inverse_packed": ("finc_pack_inverse_weights_f32", "finc_inverse_packed_f32", False),
          "inverse_affine": ("finc_pack_inverse_weights_affine_f32", "finc_inverse_packed_f32", True),
          "inverse_premul": ("finc_pack_inverse_weights_f32", "finc_inverse_packed_premultiplied_f32", False),
          "forward_packed": ("finc_pack_forward_weights_f32", "finc_forward_packed_f32", False),
          "forward_affine": ("finc_pack_forward_weights_affine_f32", "finc_forward_packed_f32", True)}


class Unit:
    """One problem set: the bank (oracle's and the device's canonical form), N(0,1) activations, an affine pair to fold."""

    def __init__(self, dev, dims, seed, orient=None, dtype=F32):
        from fincflow_amd import ops
        B, G, Cq, H, W, KH, KW = self.dims = dims
        self.orient = orient_of(G) if orient is None else orient
        ws = oracle.make_stored_weights(G, Cq, KH, KW, orient=self.orient, seed=seed, std=bank_std(Cq, max(KH, KW)))
        self.wco = oracle.canonicalize(ws, G, self.orient)
        self.wc = ops.canonicalize(t(ws if dtype == F32 else ws.astype(np.float64), dev), G, self.orient)
        rng = np.random.default_rng(seed + 1)
        self.shape = (B, G * Cq, H, W)
        self.x = rng.standard_normal(self.shape).astype(np.float32)
        self.gz = rng.standard_normal(self.shape).astype(np.float32)
        self.scale = np.exp(0.2 * rng.standard_normal(G * Cq)).astype(np.float32)
        self.shift = rng.standard_normal(G * Cq).astype(np.float32)
        self.nthr = min(oracle.max_threads(), 16)

    def pick(self):
        """The images assertion (c) looks at: both ends and the middle of the batch (the problems are independent)."""
        B = self.dims[0]
        return sorted({0, 1 % B, B // 2, B - 2 if B > 1 else 0, B - 1})

    def slab(self, p):
        """Index of problem p = image * G + group in an activation tensor."""
        G, Cq = self.dims[1], self.dims[2]
        return (p // G, slice((p % G) * Cq, (p % G + 1) * Cq))

    def slabs(self):
        """Problems to poison: the second of a packed workgroup in the middle of the batch (4k + 1), the last, the first."""
        n = self.dims[0] * self.dims[1]
        return [self.slab(p) for p in dict.fromkeys((min(4 * (n // 8) + 1, n - 1), n - 1, 0))]


def unit_call(dev, u, kind, ins, guard=False, algo="auto", direct=False):
    """One entry point of the unit on problem set `u`; `ins` holds the activations (`act`; the backward: `gz`, `x`)."""
    from fincflow_amd import _lib
    L = _lib.lib()
    d, o = u.dims, u.orient
    B, G, Cq, H, W, KH, KW = d
    if kind in ("inverse", "forward"):
        ws = L.finc_inverse_workspace_bytes(*d) if kind == "inverse" else L.finc_workspace_bytes(G, Cq, KH, KW)
        return run(dev, "finc_%s_f32" % kind, lambda p, w, n: (p["act"], p["w"], p["out"], *d, o, _lib.ALGO[algo], w, n, None),
                   dict(act=ins["act"], w=u.wc), dict(out=(u.shape, F32)), ws, guard)
    if kind == "inverse_f64":
        if algo == "strict":
            return run(dev, "finc_inverse_f64", lambda p, w, n: (p["act"], p["w"], p["out"], *d, o, None),
                       dict(act=ins["act"], w=u.wc), dict(out=(u.shape, F64)), None, guard)
        return run(dev, "finc_inverse_f64_algo", lambda p, w, n: (p["act"], p["w"], p["out"], *d, o, _lib.ALGO[algo], w, n, None),
                   dict(act=ins["act"], w=u.wc), dict(out=(u.shape, F64)), L.finc_f64_workspace_bytes(G, Cq, KH, KW), guard)
    if kind == "backward":
        ws = None if direct else L.finc_backward_workspace_bytes(*d)
        return run(dev, "finc_backward_f32", lambda p, w, n: (p["gz"], p["x"], p["w"], p["gx"], p["gw"], *d, o, w, n, None),
                   dict(gz=ins["gz"], x=ins["x"], w=u.wc), dict(gx=(u.shape, F32), gw=(tuple(u.wc.shape), F32)), ws, guard)
    pack, launch, affine = PACKED[kind]
    nb = L.finc_workspace_bytes(G, Cq, KH, KW)
    assert nb % 4 == 0
    if affine:
        r1 = run(dev, pack, lambda p, w, n: (p["w"], p["scale"], p["shift"], p["packed"], G, Cq, KH, KW, None),
                 dict(w=u.wc, scale=t(u.scale, dev), shift=t(u.shift, dev)), dict(packed=((nb // 4,), F32)), None, guard)
    else:
        r1 = run(dev, pack, lambda p, w, n: (p["w"], p["packed"], G, Cq, KH, KW, None), dict(w=u.wc), dict(packed=((nb // 4,), F32)),
                 None, guard)
    r2 = run(dev, launch, lambda p, w, n: (p["act"], p["packed"], p["out"], *d, o, None),
             dict(act=ins["act"], packed=r1.outs["packed"]), dict(out=(u.shape, F32)), None, guard)
    r2.outs["packed"] = r1.outs["packed"]
    r2.bad += r1.bad
    r2.nguard += r1.nguard
    return r2


def inverse_reference(u, kind):
    """(input of the call, float64-path reference, tolerance) on the images of u.pick(): max(1e-5, 2 x the oracle's own
    fp32-vs-fp64 gap), as tests/test_gpu_variants.py: run_inverse_case."""
    B, G, Cq, H, W, KH, KW = u.dims
    pick = u.pick()
    z = u.x.copy()                        # (the images nobody judges keep their N(0,1) values: the problems are independent)
    z[pick] = oracle.forward_f32(np.ascontiguousarray(u.x[pick]), u.wco, G, u.orient, nthreads=u.nthr)
    act = z
    if kind == "inverse_affine":          # the call's input is y with z = scale * y + shift
        act = u.x
        z = (u.x * u.scale.reshape(1, -1, 1, 1) + u.shift.reshape(1, -1, 1, 1)).astype(np.float32)
    elif kind == "inverse_premul":        # the call's input is blockdiag(Linv) z
        lead = np.linalg.inv(u.wco.reshape(G, Cq, Cq, KH, KW)[:, :, :, -1, -1].astype(np.float64))
        act = np.einsum("gok,bgkhw->bgohw", lead, z.reshape(B, G, Cq, H, W).astype(np.float64)).astype(np.float32).reshape(z.shape)
    zp = np.ascontiguousarray(z[pick])
    ref = oracle.inverse_via_f64(zp, u.wco, G, u.orient, nthreads=u.nthr)
    ref32 = oracle.inverse_f32(zp, u.wco, G, u.orient, nthreads=u.nthr)
    return act, ref, ref32, max(TOL, 2.0 * rel_err(ref32, ref))


def judge_inverse(u, kind, ref, ref32, tol, algo="auto"):
    def judge(plain):
        got = plain.outs["out"][u.pick()].cpu().numpy()
        if algo == "strict":
            assert np.array_equal(got, ref32), "strict kernel must be bit-exact with the fp32 reference order"
        e = rel_err(got, ref)
        print("inverse vs float64 reference: %.3e (tolerance %.3e)" % (e, tol))
        assert e <= tol, (kind, e, tol)
        return e
    return judge


def inverse_bounds_and_isolation(dev, tag, u, variant, kinds=("inverse",), algo="auto", with_reference=True, extra_spots=()):
    for kind in kinds:
        judge = None
        act = u.x
        if with_reference:
            act, ref, ref32, tol = inverse_reference(u, kind)
            judge = judge_inverse(u, kind, ref, ref32, tol, algo)
        act = t(act, dev)
        check_bounds(tag, lambda guard: unit_call(dev, u, kind, dict(act=act), guard, algo), variant, judge, entry=kind, dims=list(u.dims))
        if u.dims[0] * u.dims[1] < 2:
            continue                          # a single problem has nobody to leak into
        spots = [("act", s, {"out": s}) for s in u.slabs()] + list(extra_spots)
        check_isolation(dev, tag, lambda ins: unit_call(dev, u, kind, ins, False, algo), dict(act=act), spots, variant, entry=kind,
                        dims=list(u.dims))


@pytest.mark.parametrize("row", range(34))
def test_inverse_table_row(row, dev):
    """Every row of the instantiation table (finc_mfma.hip g_insts) at every problem count of problem_counts_for_row, in its 64-byte
    form (with helper waves when the problems come in fours, without otherwise), its 32-byte and its 16-byte form, the last at
    cqp - 1 channels (padded channel lanes) -- the maps of test_every_row_of_the_instantiation_table.  Assertion (c) runs once per
    row (smallest count, 16-byte form); the invariance checks run on every form."""
    from fincflow_amd import _lib
    rows = _lib.inverse_table()
    if row >= len(rows):
        pytest.skip("table has fewer rows")
    assert len(rows) <= 34, "extend the parametrisation: the table grew"
    i = rows[row]
    counts = problem_counts_for_row(rows, row)
    assert counts, (row, i)
    one_wave = i["nw"] == 1 and i["npw"] == 1
    judged = False
    for n in counts:
        B, G, orient = split_problems(n)
        big = n > 64
        s64 = 2 if one_wave else 1
        for sec, (H, W) in ((0, (5, 12) if big else (9, 20)), (1, (5, 24) if big else (19, 24)), (s64, (7, 16) if big else (10, 32))):
            Cq = i["cqp"] if sec else max(i["cqp"] - 1, 1)
            dims = (B, G, Cq, H, W, i["kh"], i["kw"])
            v = _lib.inverse_variant(*dims)
            assert v is not None and v["row"] == row, (v, row)
            assert v["sec"] == sec or (sec == 2 and v["sec"] == 3 and n % 4 == 0), (v, sec)
            u = Unit(dev, dims, seed=1000 * row + n + sec, orient=orient)
            inverse_bounds_and_isolation(dev, "table_row_%d" % row, u, v, with_reference=not judged)
            judged = True
    assert _lib.hlp_timeouts() == 0 and not _lib.fault_pending()


def _sec(sec, **more):
    return dict(sec=sec, **more)


# name -> ((B, G, Cq, H, W, KH, KW), what the library must say about the kernel, entry points); wpp = workgroups per problem
INVERSE_CASES = {
    # role-split (form 4): ragged last band, padded channels, one workgroup per problem -- and its packed / affine entry points
    "role_split": ((3, 1, 19, 21, 36, 3, 3), _sec(4, nw=4, wpp=1), ("inverse", "inverse_packed", "inverse_affine")),
    "role_split_four_flips": ((3, 4, 23, 17, 28, 3, 3), _sec(4, nw=4, wpp=1), ("inverse",)),
    # ... its band-split form (workgroups > problems): the smallest BAND_SPLIT_CASES entry, three images
    "band_split": ((3, 4, 20, 17, 72, 3, 3), _sec(4, nw=4, wpp=2), ("inverse", "inverse_affine")),
    # short-step (form 6), 3x3 (five waves) and a 2x2 bank (three)
    "short_step_one_channel": ((3, 4, 1, 9, 12, 3, 3), _sec(6, nw=5, wpp=1), ("inverse",)),
    "short_step_padded": ((3, 4, 11, 5, 40, 3, 3), _sec(6, nw=5, wpp=1), ("inverse", "inverse_packed")),
    "short_step_ragged": ((3, 4, 7, 17, 28, 3, 3), _sec(6, nw=5, wpp=1), ("inverse",)),
    "short_step_2x2": ((4, 4, 2, 6, 8, 2, 2), _sec(6, nw=3, wpp=1), ("inverse",)),
    # big bank (form 5): one band, and a width that is no multiple of the band's 16 columns
    "big_bank": ((3, 1, 96, 16, 16, 3, 3), _sec(5, nw=8, cqp=96, wpp=1), ("inverse", "inverse_packed")),
    "big_bank_width_20": ((3, 1, 65, 7, 20, 3, 3), _sec(5, nw=8, cqp=96, wpp=1), ("inverse",)),
    # the wide-map hand-over through memory (the smallest WIDE_MAP_CASES entry at half its height, three images)
    "wide_map": ((3, 1, 96, 20, 80, 3, 3), _sec(5, nw=8, cqp=96, wpp=1), ("inverse",)),
    # streaming bank (form 7): four waves, one-wave dword (row -3), one-wave 16-byte (row -4), a single-row map
    "stream_four_waves": ((8, 1, 130, 8, 8, 3, 3), _sec(7, nw=4, row=-3, cqp=192), ("inverse", "inverse_affine")),
    "stream_one_wave_dword": ((160, 4, 12, 8, 8, 4, 4), _sec(7, nw=1, row=-3, cqp=16), ("inverse",)),
    "stream_one_wave_16_byte": ((161, 4, 12, 8, 8, 4, 4), _sec(7, nw=1, row=-4, cqp=16), ("inverse",)),
    "stream_single_row": ((3, 4, 129, 1, 50, 3, 3), _sec(7, nw=4, row=-3, cqp=192), ("inverse",)),
    # the borrowed 28-channel bank on the 32-channel bank's packed two-wave kernel (25 channels: padded lanes as well)
    "borrowed_bank": ((65, 4, 25, 9, 20, 3, 3), dict(cqp=32, nw=2, npw=2), ("inverse",)),
    # a table row (c3's bank, helper waves) through the packed, affine-packed and premultiplied entry points
    "table_row_packed": ((132, 4, 24, 8, 16, 3, 3), _sec(3, cqp=24, nw=1, npw=1), ("inverse_packed", "inverse_affine", "inverse_premul")),
}


@pytest.mark.parametrize("name", sorted(INVERSE_CASES))
def test_inverse_family(name, dev):
    """Guard bands (a)-(c) and slab isolation of one inverse kernel family, on each entry point listed for it.  (The premultiplied
    entry point exists for the helper-wave form only: the role-split kernel has none.)"""
    from fincflow_amd import _lib
    dims, want, kinds = INVERSE_CASES[name]
    v = _lib.inverse_variant(*dims)
    assert v is not None, name
    want = dict(want)
    wpp = want.pop("wpp", None)
    assert all(v[k] == x for k, x in want.items()), (name, v, want)
    if wpp:
        assert v["workgroups"] == wpp * dims[0] * dims[1], (name, v)
    assert _lib.inverse_remainder_images(*dims) == 0
    L = _lib.lib()
    if "inverse_affine" in kinds:
        assert L.finc_inverse_affine_supported(*dims) == 1
    if "inverse_premul" in kinds:
        assert L.finc_inverse_premultiplied_supported(*dims) == 1
    u = Unit(dev, dims, seed=sum(dims))
    inverse_bounds_and_isolation(dev, name, u, v, kinds)
    assert _lib.hlp_timeouts() == 0 and not _lib.fault_pending()


@pytest.mark.parametrize("dims", [(3, 4, 4, 7, 7, 3, 3), (3, 4, 4, 6, 5, 5, 5), (3, 1, 65, 9, 18, 3, 3)], ids=lambda d: "B%d_G%d_Cq%d_%dx%d_k%dx%d" % d)
def test_inverse_odd_width_on_the_padded_workspace_copy(dims, dev):
    """W % 4 != 0: FINC_ALGO_AUTO solves a zero-padded copy of z in the workspace (finc_inverse_workspace_bytes) on the MFMA kernel.
    The workspace is NaN on entry and exactly as large as asked for: every byte of the padding the kernel reads must have been
    written by the call itself.  Kernel named as test_odd_widths_run_on_the_padded_mfma_path does: the plain dispatch is strict, the
    workspace the library asks for has room for both copies.  The third case is a big bank (form 5 on the padded copy: 65 channels,
    W = 18), as test_big_bank_forward_on_an_odd_width runs it."""
    from fincflow_amd import _lib
    L = _lib.lib()
    B, G, Cq, H, W, KH, KW = dims
    assert L.finc_inverse_algo_for(Cq, H, W, KH, KW) == _lib.ALGO["strict"]
    need, base = L.finc_inverse_workspace_bytes(*dims), L.finc_workspace_bytes(G, Cq, KH, KW)
    assert need >= base + 2 * B * G * Cq * H * ((W + 7) // 8 * 8) * 4
    u = Unit(dev, dims, seed=sum(dims))
    inverse_bounds_and_isolation(dev, "odd_width", u, dict(path="padded copy", workspace=need))


def test_inverse_remainder_launch(dev):
    """The smallest REMAINDER_CASES entry that takes a second launch: 1,040 problems = a round of 1,024 on the helper-wave form plus
    4 images on the role-split kernel.  (a)-(c), the images on either side of the seam bit-equal to the plain call, and isolation
    with the last image of the first launch poisoned."""
    from fincflow_amd import _lib
    dims = (260, 4, 24, 8, 16, 3, 3)
    B, G = dims[:2]
    r = _lib.inverse_remainder_images(*dims)
    v = _lib.inverse_variant(*dims)
    assert r == 4 and (v["nw"], v["npw"]) == (1, 1) and v["sec"] == 3, (r, v)
    tail = _lib.inverse_variant(r, *dims[1:])
    assert tail["sec"] == 4, tail
    u = Unit(dev, dims, seed=260)
    act, ref, ref32, tol = inverse_reference(u, "inverse")
    act = t(act, dev)
    seam = [B - r - 1, B - r]
    guarded_seam = {}

    def call(guard):
        res = unit_call(dev, u, "inverse", dict(act=act), guard)
        guarded_seam[guard] = res.outs["out"][seam].clone()
        return res
    check_bounds("remainder", call, dict(main=v, remainder=tail, images=r), judge_inverse(u, "inverse", ref, ref32, tol), dims=list(dims))
    assert same_bits(guarded_seam[True], guarded_seam[False])
    last_of_first = (B - r - 1, slice(None))
    spots = [("act", last_of_first, {"out": last_of_first})] + [("act", s, {"out": s}) for s in u.slabs()]
    check_isolation(dev, "remainder", lambda ins: unit_call(dev, u, "inverse", ins), dict(act=act), spots,
                    dict(main=v, remainder=tail, images=r), dims=list(dims))
    assert _lib.hlp_timeouts() == 0 and not _lib.fault_pending()


def test_inverse_strict(dev):
    """FINC_ALGO_STRICT (the reference-order kernel, named by the algo argument): bit-exact with oracle.inverse_f32."""
    u = Unit(dev, (3, 4, 5, 9, 11, 3, 3), seed=5)
    inverse_bounds_and_isolation(dev, "strict", u, dict(algo="strict"), algo="strict")


# (B, G, Cq, H, W, K, orient or None = FastFlow's): the two smallest F64_CASES the matrix-core form takes
@pytest.mark.parametrize("algo", ["strict", "mfma"])
@pytest.mark.parametrize("case", [(3, 1, 5, 9, 11, 3, 0), (3, 1, 3, 7, 7, 3, 1)], ids=lambda c: "B%d_G%d_Cq%d_%dx%d_k%d_o%d" % c)
def test_inverse_fp64(case, algo, dev):
    """finc_inverse_f64 (reference order: bit-exact with the oracle's fp64 solve) and the matrix-core form (FINC_ALGO_MFMA insists on
    it: FINC_ERR_UNSUPPORTED otherwise; within 1e-12 of the reference-order solve, the bar of tests/test_gpu_round5.py)."""
    B, G, Cq, H, W, K, o = case
    u = Unit(dev, (B, G, Cq, H, W, K, K), seed=sum(case), orient=o, dtype=F64)
    z = np.random.default_rng(3).standard_normal(u.shape)
    wco = u.wco.astype(np.float64)            # (the oracle's own canonical form of the same fp32-representable bank)
    zc = z[:, :, ::-1 if o & 2 else 1, ::-1 if o & 1 else 1]
    ref = oracle.inverse_f64(np.ascontiguousarray(zc), wco, 1)[:, :, ::-1 if o & 2 else 1, ::-1 if o & 1 else 1]
    act = t(z, dev)

    def judge(plain):
        got = plain.outs["out"].cpu().numpy()
        e = rel_err(got, ref)
        assert np.array_equal(got, ref) if algo == "strict" else e <= 1e-12, e
        return e
    call = lambda ins, guard=False: unit_call(dev, u, "inverse_f64", ins, guard, algo)
    check_bounds("fp64_" + algo, lambda guard: call(dict(act=act), guard), dict(algo=algo), judge, dims=list(u.dims))
    check_isolation(dev, "fp64_" + algo, call, dict(act=act), [("act", s, {"out": s}) for s in u.slabs()], dict(algo=algo), dims=list(u.dims))


# ---------------------------------------------------------------------------------------------------------------------------------
# forward, grad-input, grad-weight
# ---------------------------------------------------------------------------------------------------------------------------------
# name -> ((B, G, Cq, H, W, KH, KW), pinned forward form, conv_form, gradw form, grad-input waves per strip): each forward family at
# a width that is a multiple of its tile and at one that is not, padded channel counts among them
CONV_CASES = {
    "strip_dword": ((3, 4, 5, 9, 11, 3, 3), 0, "strip", "dword", 1),
    "strip_dword_pinned_w24": ((3, 4, 23, 9, 24, 3, 3), 1, "strip", "winograd", 1),
    "strip_staged": ((3, 4, 23, 5, 48, 3, 3), 1, "strip16", "winograd", 1),
    "strip_staged_28_channels": ((3, 4, 28, 6, 32, 3, 3), 0, "strip16", "winograd", 1),
    "strip_staged_2x2": ((3, 4, 24, 9, 16, 2, 2), 0, "strip16", "staged", 1),
    "f23": ((3, 4, 23, 5, 64, 3, 3), 2, "winograd", "winograd", 1),
    "f23_partial_strip": ((3, 4, 20, 9, 60, 3, 3), 2, "winograd", "winograd", 1),
    "f23_library_choice": ((3, 4, 12, 9, 20, 3, 3), 0, "winograd", "staged", 1),
    "f43": ((3, 4, 23, 5, 64, 3, 3), 4, "winograd4", "winograd", 1),
    "f43_partial_strip": ((3, 4, 20, 9, 60, 3, 3), 4, "winograd4", "winograd", 1),
    "f43_msplit": ((8, 4, 32, 12, 64, 3, 3), 0, "winograd4m", "winograd", 1),
    "f43_msplit_padded_w48": ((8, 4, 28, 9, 48, 3, 3), 0, "winograd4m", "winograd", 1),
    "f25": ((3, 4, 12, 7, 32, 5, 5), 0, "winograd25", "staged", 1),
    "f25_padded_w20": ((3, 4, 15, 9, 20, 5, 5), 0, "winograd25", "winograd_tiled", 1),
    "big_msplit": ((3, 1, 96, 16, 16, 3, 3), 0, "msplit", "tiled", 8),
    "big_msplit_padded_w20": ((3, 1, 65, 7, 20, 3, 3), 0, "msplit", "tiled", 8),
    "ksplit": ((3, 4, 48, 10, 16, 3, 3), 0, "strip", "tiled", 2),
    "ksplit_padded_w20": ((3, 4, 44, 10, 20, 3, 3), 0, "strip", "tiled", 2),
    "ksplit_wino_tiled_gradw": ((3, 4, 48, 10, 36, 3, 3), 0, "strip", "winograd_tiled", 2),
    "gradw_dword_c3_bank": ((3, 4, 24, 9, 18, 3, 3), 0, "strip", "dword", 1),
    # the staged grad-weight kernel with all three of: a strip wider than the row (pieces past its end, mirrored before its start), a
    # mirrored group, and Cq below the padded bank (tiled, winograd, winograd_tiled have such cases above: *_padded_w20, *_w24)
    "gradw_staged_padded_w4": ((2, 2, 1, 5, 4, 3, 3), 0, "winograd", "staged", 1),
    # a big bank on a width with W % 4 != 0: the 8-wave K-split row of the strip kernel on dword loads, the direct grad-weight
    "big_strip_odd_width": ((3, 1, 65, 9, 18, 3, 3), 0, "strip", "direct", 8),
    # a filter no MFMA kernel takes (a side of 8 .. 15 is legal): the generic forward / grad-input / grad-weight kernels, no packed
    # form (1x8: the generic grad-weight kernel holds at most 49 taps and answers FINC_ERR_UNSUPPORTED beyond)
    "scalar_1x8": ((3, 4, 2, 6, 8, 1, 8), 0, "scalar", "direct", 0),
    "stream": ((8, 1, 130, 8, 8, 3, 3), 0, "stream", "tiled", 4),
    "stream_one_wave_4x4": ((3, 4, 8, 20, 24, 4, 4), 0, "stream", "tiled", 1),
    "stream_odd_width": ((3, 4, 100, 17, 33, 3, 3), 0, "stream", "direct", 4),
    "stream_wino_tiled_gradw": ((3, 4, 104, 8, 32, 3, 3), 0, "stream", "winograd_tiled", 4),
}
# the launch regimes of tests/plan_cases.py: a grad-weight workgroup's second trip through its unit loop (all five forms), and the
# chunk seams of the one-wave-per-SIMD forward kernels (H >= 16); conv_family asserts each case's plan numbers before it runs
CONV_CASES.update({n: (c["dims"], 0, c["conv_form"], c["plan"]["form"], c["gradx_waves"]) for n, c in GRADW_WALK_CASES.items()})
CONV_CASES.update({n: (c["dims"], c["pin"], c["conv_form"], c["gradw"], c["gradx_waves"]) for n, c in ROW_CHUNK_CASES.items()})
AFFINE_FORWARD = ("strip_staged", "f23", "f43_msplit", "stream")      # the affine fold behind the forward, on four kernel families


def conv_reference(u):
    """float64 autograd on the CPU of the unit's forward in canonical coordinates (tests/test_gpu_stream.py): z, grad_x, masked grad_w."""
    import torch.nn.functional as F
    B, G, Cq, H, W, KH, KW = u.dims
    xd = torch.from_numpy(u.x).double().requires_grad_(True)
    wd = torch.from_numpy(u.wco).double().requires_grad_(True)
    outs = []
    for g in range(G):
        o = (u.orient >> (2 * g)) & 3
        flips = [d for d, bit in ((2, 2), (3, 1)) if o & bit]
        xg = xd[:, g * Cq:(g + 1) * Cq]
        xg = torch.flip(xg, flips) if flips else xg
        y = F.conv2d(F.pad(xg, (KW - 1, 0, KH - 1, 0)), wd[g * Cq:(g + 1) * Cq])
        outs.append(torch.flip(y, flips) if flips else y)
    z = torch.cat(outs, 1)
    z.backward(torch.from_numpy(u.gz).double())
    gw = wd.grad.numpy().copy()
    corner = gw[:, :, KH - 1, KW - 1].reshape(G, Cq, Cq)
    corner[:, np.triu_indices(Cq)[0], np.triu_indices(Cq)[1]] = 0.0           # PaddedConv2d.reset_gradients (layers/conv.py:98-99)
    return z.detach().numpy(), xd.grad.numpy(), gw


def judge_outputs(refs):
    def judge(plain):
        errs = {k: rel_err(plain.outs[k].cpu().numpy(), r) for k, r in refs.items()}
        print("against the float64 reference:", errs)
        assert all(e <= TOL for e in errs.values()), errs
        return errs
    return judge


def group_rows(u, g):
    Cq = u.dims[2]
    return slice(g * Cq, (g + 1) * Cq)


def assert_regime(name, dims, u):
    """A case of tests/plan_cases.py really is in its regime (the launch's own plan, under the pinned forward form): its plan numbers
    are the table's; a walk case has more units than workgroups per group, and the batch's last image -- the image of the last
    problem, one of the slabs the isolation runs poison -- consists of units a workgroup reaches on its second trip or later."""
    from fincflow_amd import _lib
    if name in GRADW_WALK_CASES:
        p, want = _lib.gradw_plan(*dims, align=16), GRADW_WALK_CASES[name]["plan"]
        assert p == want, (name, p, want)
        assert p["units"] > p["wpg"], (name, p)
        last = u.slab(dims[0] * dims[1] - 1)
        assert last in u.slabs() and last[0] * p["ns"] >= p["wpg"], (name, last, p)     # (unit = image * ns + strip)
    if name in ROW_CHUNK_CASES:
        c, want = _lib.conv_plan(*dims, align=16), ROW_CHUNK_CASES[name]["plan"]
        assert c == want, (name, c, want)
        assert c["nrc"] >= 2 and dims[3] >= 16 and dims[3] % c["RC"] != 0, (name, c)


def conv_family(dev, name, dims, pin, form, gradw, waves, direct=False):
    from fincflow_amd import _lib
    try:
        _lib.set_forward_form(pin)
        bv = _lib.backward_variant(*dims)
        assert bv["conv_form"] == form and bv["gradw"] == gradw and bv["gradx_waves"] == waves, (name, bv)
        assert (_lib.lib().finc_forward_algo_for(*dims[2:]) == _lib.ALGO["mfma"]) == (form != "scalar")
        if direct:
            bv = dict(gradw="direct", gradx="direct", workspace=None)        # NULL workspace selects the direct kernels (include/finc.h)
        u = Unit(dev, dims, seed=sum(dims) + pin)
        assert_regime(name, dims, u)
        z, gx, gw = conv_reference(u)
        x, gz = t(u.x, dev), t(u.gz, dev)
        slabs = u.slabs()
        if not direct:
            kinds = ["forward"] + (["forward_packed"] if form != "scalar" else []) + (["forward_affine"] if name in AFFINE_FORWARD else [])
            for kind in kinds:
                want = z * u.scale.reshape(1, -1, 1, 1).astype(np.float64) + u.shift.reshape(1, -1, 1, 1) if kind == "forward_affine" else z
                check_bounds(name, lambda guard: unit_call(dev, u, kind, dict(act=x), guard), bv, judge_outputs(dict(out=want)),
                             entry=kind, dims=list(dims))
                check_isolation(dev, name, lambda ins: unit_call(dev, u, kind, ins), dict(act=x), [("act", s, {"out": s}) for s in slabs],
                                bv, entry=kind, dims=list(dims))
        check_bounds(name, lambda guard: unit_call(dev, u, "backward", dict(gz=gz, x=x), guard, direct=direct), bv,
                     judge_outputs(dict(gx=gx, gw=gw)), entry="backward", dims=list(dims))
        # grad-input: a slab of grad_z reaches its own slab of grad_x (and its group's block of grad_w); grad-weight: a slab of x
        # reaches its group's block of grad_w and nothing of grad_x
        G = dims[1]
        spots = [("gz", s, {"gx": s, "gw": group_rows(u, s[1].start // dims[2])}) for s in slabs]
        spots += [("x", s, {"gx": None, "gw": group_rows(u, s[1].start // dims[2])}) for s in slabs[:2]]
        if G == 1:                            # one group: every entry of grad_w is reachable, the other IMAGES' grad_x stay
            spots = [(n, i, {k: v for k, v in r.items() if k != "gw"}) for n, i, r in spots]
        check_isolation(dev, name, lambda ins: unit_call(dev, u, "backward", ins, direct=direct), dict(gz=gz, x=x), spots, bv,
                        entry="backward", dims=list(dims))
    finally:
        _lib.set_forward_form(0)
    assert _lib.runtime_switches() == []
    assert not _lib.fault_pending()


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_forward_and_backward_family(name, dev):
    """Forward (plain, packed, and with the affine fold on four families), grad-input and grad-weight of one kernel family: guard
    bands (a)-(c) against float64 autograd on the CPU, slab isolation of all three."""
    conv_family(dev, name, *CONV_CASES[name])


@pytest.mark.parametrize("name", ["strip_dword", "gradw_dword_c3_bank"])
def test_backward_direct_kernels(name, dev):
    """finc_backward_f32 without a workspace: the direct grad-input and grad-weight kernels (backward_variant's "direct")."""
    conv_family(dev, name + "_direct", *CONV_CASES[name], direct=True)


def test_grad_weight_walk_on_float_aligned_activations(dev):
    """walk_staged's shape with grad_z and x one float into their allocations (4-byte aligned, not 16): the plan for these
    activations is the dword form, 258 units on 256 workgroups per group, so the second trip of THAT kernel runs -- between guards,
    on the exact-size NaN workspace, bit-stable, grad_w and grad_x against the float64 reference of the aligned case at TOL."""
    from fincflow_amd import _lib
    dims = GRADW_WALK_CASES["walk_staged"]["dims"]
    p = _lib.gradw_plan(*dims, align=4)
    assert p["form"] == "dword" and p["units"] > p["wpg"], p
    u = Unit(dev, dims, seed=sum(dims))
    _, gx, gw = conv_reference(u)
    x, gz = t(u.x, dev), t(u.gz, dev)
    ws = _lib.lib().finc_backward_workspace_bytes(*dims)
    assert p["bytes"] <= ws
    call = lambda guard: run(dev, "finc_backward_f32", lambda q, w, n: (q["gz"], q["x"], q["w"], q["gx"], q["gw"], *dims, u.orient, w, n, None),
                             dict(gz=gz, x=x, w=u.wc), dict(gx=(u.shape, F32), gw=(tuple(u.wc.shape), F32)), ws, guard, lead=("gz", "x"))
    check_bounds("walk_staged_float_aligned", call, dict(gradw=p["form"], units=p["units"], wpg=p["wpg"]),
                 judge_outputs(dict(gx=gx, gw=gw)), entry="backward", dims=list(dims))
    assert not _lib.fault_pending()


# ---------------------------------------------------------------------------------------------------------------------------------
# weights: canonicalize (fp32, fp64), the invariant check, every pack call
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_canonicalize_weights(dtype, dev):
    """finc_canonicalize_weights_f32 / _f64 against the oracle's flips (bit-exact: a permutation); a poisoned group's bank stays in
    its own rows."""
    G, Cq, KH, KW = 4, 5, 3, 5
    ws = oracle.make_stored_weights(G, Cq, KH, KW, seed=9)
    want = oracle.canonicalize(ws, G, ORIENT_FASTFLOW)
    w = t(ws if dtype == F32 else ws.astype(np.float64), dev)
    sym = "finc_canonicalize_weights_f32" if dtype == F32 else "finc_canonicalize_weights_f64"
    call = lambda ins, guard=False: run(dev, sym, lambda p, _w, _n: (p["w"], p["out"], G, Cq, KH, KW, ORIENT_FASTFLOW, None), ins,
                                        dict(out=(tuple(w.shape), dtype)), None, guard)

    def judge(plain):
        assert np.array_equal(plain.outs["out"].cpu().numpy(), want.astype(plain.outs["out"].cpu().numpy().dtype))
        return 0.0
    check_bounds(sym, lambda guard: call(dict(w=w), guard), dict(kernel=sym), judge)
    rows = slice(2 * Cq, 3 * Cq)
    check_isolation(dev, sym, call, dict(w=w), [("w", rows, {"out": rows})], dict(kernel=sym))


def test_check_invariant(dev):
    """finc_check_invariant_f32 on a bank between NaN guards: FINC_OK on a valid bank, FINC_ERR_INVARIANT (a FincError) when the last
    diagonal entry of the last group -- the entry next to the back guard -- is wrong; the guards stay as they were."""
    from fincflow_amd import _lib, ops
    G, Cq, K = 4, 7, 3
    wc = ops.canonicalize(t(oracle.make_stored_weights(G, Cq, K, K, seed=2), dev), G, ORIENT_FASTFLOW)
    call = lambda w, guard: run(dev, "finc_check_invariant_f32", lambda p, _w, _n: (p["w"], G, Cq, K, K, None), dict(w=w), {}, None, guard)
    res = call(wc, True)
    assert not res.bad and res.nguard == 2 * 4096
    bad = poison(wc, (G * Cq - 1, Cq - 1, K - 1, K - 1), 0.5)
    with pytest.raises(_lib.FincError):
        call(bad, True)
    report("bounds", tag="check_invariant", variant=dict(kernel="finc_check_invariant_f32"), guard_elements=res.nguard, err=None)


@pytest.mark.parametrize("dims", [(4, 23, 3, 3), (1, 96, 3, 3), (4, 12, 4, 4), (4, 12, 5, 5)], ids=lambda d: "G%d_Cq%d_k%dx%d" % d)
@pytest.mark.parametrize("kind", ["inverse_packed", "inverse_affine", "forward_packed", "forward_affine"])
def test_pack_calls(kind, dims, dev):
    """Every finc_pack_* call writes inside a buffer of exactly finc_workspace_bytes(): the wavefront / role-split banks (23 padded
    channels), the big bank, a streaming bank (4x4) and a 5x5 bank.  What the packed bank computes is the launches' business
    (test_inverse_family, test_forward_and_backward_family run them on guarded packed buffers)."""
    from fincflow_amd import _lib, ops
    G, Cq, KH, KW = dims
    pack, _, affine = PACKED[kind]
    L = _lib.lib()
    nb = L.finc_workspace_bytes(G, Cq, KH, KW)
    wc = ops.canonicalize(t(oracle.make_stored_weights(G, Cq, KH, KW, seed=4, std=bank_std(Cq, KH)), dev), G, ORIENT_FASTFLOW if G == 4 else 0)
    rng = np.random.default_rng(1)
    ins = dict(w=wc)
    if affine:
        ins.update(scale=t(np.exp(0.2 * rng.standard_normal(G * Cq)).astype(np.float32), dev),
                   shift=t(rng.standard_normal(G * Cq).astype(np.float32), dev))
        argf = lambda p, _w, _n: (p["w"], p["scale"], p["shift"], p["packed"], G, Cq, KH, KW, None)
    else:
        argf = lambda p, _w, _n: (p["w"], p["packed"], G, Cq, KH, KW, None)
    if kind == "inverse_affine" and Cq > 64:
        # the big banks refuse a shift (include/finc.h), and a refused pack writes nothing: buffer and guards keep the fill pattern
        pv, pb = guarded(nan_filled((nb // 4,), F32, dev), dev)
        st = getattr(L, pack)(wc.data_ptr(), ins["scale"].data_ptr(), ins["shift"].data_ptr(), pv.data_ptr(), G, Cq, KH, KW, None)
        torch.cuda.synchronize(dev)
        assert st == 3, st
        assert guards_intact(pb, pv) and same_bits(pv, nan_filled((nb // 4,), F32, dev))
        report("bounds", tag=pack, variant=dict(kernel=pack, refused=True), guard_elements=pb.numel() - pv.numel(), err=None, dims=list(dims))
        return
    check_bounds(pack, lambda guard: run(dev, pack, argf, ins, dict(packed=((nb // 4,), F32)), None, guard), dict(kernel=pack, bytes=nb),
                 dims=list(dims))


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-pixel layers: finc_mix, coupling, bias + ReLU, ActNorm -- each in its 16-byte and its dword form
# ---------------------------------------------------------------------------------------------------------------------------------
def pixel_inputs(shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    r = lambda *s: torch.randn(*s, generator=g)
    logs = 0.1 * r(C)
    a = torch.exp(3.0 * logs.double())
    return dict(x=r(*shape), gy=r(*shape), raw=1.5 * r(*shape), gl=r(B), a=a.float(), b=(0.3 * r(C).double() * a).float(),
                ls=0.2 * r(C), tr=r(C), mat=r(C, C) / C ** 0.5, bias=r(C))


def grads(fn, leaves, cot):
    """float64 autograd: d sum(out_i * cot_i) / d leaves."""
    leaves = [v.double().requires_grad_(True) for v in leaves]
    outs = fn(*leaves)
    sum((o * c.double()).sum() for o, c in zip(outs, cot) if o is not None and c is not None).backward()
    return [v.grad.numpy() for v in leaves]


def pixel_op(op, shape, dev):
    """One per-pixel entry point on `shape`: symbol, inputs, outputs, workspace bytes, arguments, the activation pointers (what the
    dword form shifts), the documented in-place form, the float64 references, the isolation spots, the poison values."""
    from fincflow_amd import _lib
    L = _lib.lib()
    B, C, H, W = shape
    HW, half = H * W, C // 2
    T = pixel_inputs(shape)
    D = {k: v.to(dev) for k, v in T.items()}
    d64 = {k: v.double() for k, v in T.items()}
    b1, px, c0 = B // 2, (H // 2, W - 1), C - 1 if C < 3 else C // 2 + 1
    pixel = (b1, slice(None), *px)
    image, chan = (b1,), (slice(None), c0)
    values = (NAN, INF)
    alias = None
    if op == "mix":
        sym, ws = "finc_mix_f32", None
        ins, outs, acts = dict(x=D["x"], mat=D["mat"], bias=D["bias"]), dict(out=(shape, F32)), ("x", "out")
        argf = lambda p, w, n: (p["x"], p["mat"], p["bias"], p["out"], B, C, HW, None)
        alias = dict(out="x")
        refs = dict(out=(torch.einsum("oi,bihw->bohw", d64["mat"], d64["x"]) + d64["bias"].view(1, -1, 1, 1)).numpy())
        spots = [("x", pixel, dict(out=pixel))]
    elif op == "mix_backward":
        sym, ws = "finc_mix_backward_f32", L.finc_mix_backward_workspace_bytes(B, C, HW)
        ins, acts = dict(gy=D["gy"], x=D["x"], mat=D["mat"]), ("gy", "x", "gin")
        outs = dict(gin=(shape, F32), gmat=((C, C), F32), gbias=((C,), F32))
        argf = lambda p, w, n: (p["gy"], p["x"], p["mat"], p["gin"], p["gmat"], p["gbias"], B, C, HW, w, n, None)
        refs = dict(gin=torch.einsum("oi,bohw->bihw", d64["mat"], d64["gy"]).numpy(),
                    gmat=torch.einsum("bohw,bihw->oi", d64["gy"], d64["x"]).numpy(), gbias=d64["gy"].sum((0, 2, 3)).numpy())
        spots = [("gy", pixel, dict(gin=pixel)), ("x", chan, dict(gin=None, gmat=chan, gbias=None))]
    elif op in ("coupling", "coupling_no_logdet", "coupling_reverse"):
        direction = -1 if op == "coupling_reverse" else 1
        logdet = op == "coupling"
        sym, ws = "finc_coupling_f32", L.finc_coupling_workspace_bytes(B, C, HW) if logdet else None
        ins, acts = dict(x=D["x"], raw=D["raw"], a=D["a"], b=D["b"]), ("x", "raw", "y")
        outs = dict(y=(shape, F32), **(dict(logdet=((B,), F32)) if logdet else {}))
        argf = lambda p, w, n: (p["x"], p["raw"], p["a"], p["b"], p["y"], p.get("logdet"), B, C, HW, direction, w, n, None)
        alias = dict(y="x")
        y, ld = coupling_ref(d64["x"], d64["raw"], d64["a"], d64["b"], direction)
        refs = dict(y=y.numpy(), **(dict(logdet=ld.numpy()) if logdet else {}))
        spots = [("raw", image, dict(y=image, **(dict(logdet=image) if logdet else {}))),
                 ("x", image, dict(y=image, **(dict(logdet=None) if logdet else {})))]
    elif op == "coupling_backward":
        sym, ws = "finc_coupling_backward_f32", L.finc_coupling_workspace_bytes(B, C, HW)
        ins = dict(gy=D["gy"], gl=D["gl"], x=D["x"], raw=D["raw"], a=D["a"], b=D["b"])
        acts = ("gy", "x", "raw", "gx", "graw")
        outs = dict(gx=(shape, F32), graw=(shape, F32), ga=((C,), F32), gb=((C,), F32))
        argf = lambda p, w, n: (p["gy"], p["gl"], p["x"], p["raw"], p["a"], p["b"], p["gx"], p["graw"], p["ga"], p["gb"], B, C, HW, w, n, None)
        g = grads(lambda x, raw, a, b: coupling_ref(x, raw, a, b, 1), [T["x"], T["raw"], T["a"], T["b"]], [T["gy"], T["gl"]])
        refs = dict(zip(("gx", "graw", "ga", "gb"), g))
        j = half // 2
        pair = (slice(None), slice(2 * j, 2 * j + 2))
        spots = [("raw", image, dict(gx=image, graw=image)), ("gl", image, dict(gx=None, graw=image)),
                 ("raw", pair, dict(ga=pair[1], gb=pair[1], gx=(slice(None), half + j), graw=pair))]
    elif op == "bias_relu":
        sym, ws = "finc_bias_relu_f32", None
        ins, outs, acts = dict(x=D["x"], bias=D["bias"]), dict(out=(shape, F32)), ("x", "out")
        argf = lambda p, w, n: (p["x"], p["bias"], p["out"], B, C, HW, None)
        alias = dict(out="x")
        refs = dict(out=torch.relu(d64["x"] + d64["bias"].view(1, -1, 1, 1)).numpy())
        spots, values = [("x", image, dict(out=image))], (INF,)
    elif op in ("actnorm", "actnorm_reverse"):
        direction = 1 if op == "actnorm" else -1
        sym, ws = "finc_actnorm_f32", None
        ins, acts = dict(x=D["x"], ls=D["ls"], tr=D["tr"]), ("x", "y")
        outs = dict(y=(shape, F32), **(dict(logdet=((B,), F32)) if direction > 0 else {}))
        argf = lambda p, w, n: (p["x"], p["ls"], p["tr"], p["y"], p.get("logdet"), B, C, HW, direction, None)
        alias = dict(y="x")
        y, ld = actnorm_ref(d64["x"], d64["ls"], d64["tr"], direction)
        refs = dict(y=y.numpy(), **(dict(logdet=ld.numpy()) if direction > 0 else {}))
        spots = [("x", chan, dict(y=chan, **(dict(logdet=None) if direction > 0 else {})))]
    elif op == "actnorm_backward":
        sym, ws = "finc_actnorm_backward_f32", L.finc_actnorm_workspace_bytes(B, C, HW)
        y32 = actnorm_ref(T["x"], T["ls"], T["tr"], 1)[0].contiguous()          # the forward's output, as the kernel is handed it
        ins, acts = dict(gy=D["gy"], gl=D["gl"], y=y32.to(dev), ls=D["ls"]), ("gy", "y", "gx")
        outs = dict(gx=(shape, F32), gls=((C,), F32), gt=((C,), F32))
        argf = lambda p, w, n: (p["gy"], p["gl"], p["y"], p["ls"], p["gx"], p["gls"], p["gt"], B, C, HW, w, n, None)
        alias = dict(gx="gy")
        # y = (x - tr) * exp(-ls) with x = y32 * exp(ls) + tr held fixed: the gradients the ABI documents, from y
        e = torch.exp(-d64["ls"])
        gy, yy = d64["gy"], y32.double()
        refs = dict(gx=(gy * e.view(1, -1, 1, 1)).numpy(), gt=(-e * gy.sum((0, 2, 3))).numpy(),
                    gls=(-(gy * yy).sum((0, 2, 3)) - HW * d64["gl"].sum()).numpy())
        spots = [("y", chan, dict(gx=None, gls=(c0,), gt=None)), ("gy", chan, dict(gx=chan, gls=(c0,), gt=(c0,)))]
    elif op == "actnorm_init":
        sym, ws = "finc_actnorm_init_f32", L.finc_actnorm_workspace_bytes(B, C, HW)
        ins, acts = dict(x=D["x"]), ("x",)
        outs = dict(ls=((C,), F32), tr=((C,), F32))
        argf = lambda p, w, n: (p["x"], p["ls"], p["tr"], B, C, HW, w, n, None)
        xc = d64["x"].transpose(0, 1).reshape(C, -1)
        refs = dict(tr=xc.mean(1).numpy(), ls=torch.log(xc.std(1) + 1e-8).numpy())
        spots = [("x", chan, dict(ls=(c0,), tr=(c0,)))]
    else:
        raise KeyError(op)
    return dict(sym=sym, ins=ins, outs=outs, ws=ws, argf=argf, acts=acts, alias=alias, refs=refs, spots=spots, values=values)


PIXEL_OPS = ["mix", "mix_backward", "coupling", "coupling_no_logdet", "coupling_reverse", "coupling_backward", "bias_relu", "actnorm",
             "actnorm_reverse", "actnorm_backward", "actnorm_init"]
# finc_mix_f32 and the grad-input of finc_mix_backward_f32, shape -> the form the launch takes on 16-byte aligned activations
# (finc_mix.hip: finc_mix_launch): C = 4, 12, 96 on four pixels per lane (16-byte pieces: HW >= 64, HW % 4 == 0), C = 96 and 12 on two
# (8-byte: HW >= 32, HW % 2 == 0), C = 192 -- which has the dword instantiation only --, C = 24 (no multiple of 16) on a 5x3 map
# and C = 4 at HW = 49 on dwords
MIX_SHAPES = {(3, 4, 8, 8): "16-byte", (3, 12, 8, 8): "16-byte", (3, 96, 8, 8): "16-byte", (3, 96, 5, 8): "8-byte", (3, 12, 6, 7): "8-byte",
              (3, 192, 8, 8): "dword", (3, 24, 5, 3): "dword", (3, 4, 7, 7): "dword"}
# the others: C = 12 with HW % 4 == 0, C = 4 with HW = 15, five images of 6 channels
PIXEL_SHAPES = [(3, 12, 8, 8), (3, 4, 5, 3), (5, 6, 9, 8)]


def mix_form(C, HW, align):
    """The pixels per lane finc_mix_launch picks (finc_mix.hip), restated: by HW and the activations' common alignment, then
    narrowed to what make_mix<C> instantiates -- four pixels per lane up to 96 channels, two where LDS or registers leave room."""
    MTN, NK = (C + 15) // 16, C // 4
    big_lds = MTN * (NK + 1) * 256 > 80 * 1024
    kb = NK if NK <= 32 else 24
    have = {0: True, 1: (not big_lds) or 2 * kb + 10 * MTN + 24 <= 128, 2: MTN <= 6}
    pxi = 2 if (HW % 4 == 0 and align % 16 == 0 and HW >= 64) else 1 if (HW % 2 == 0 and align % 8 == 0 and HW >= 32) else 0
    while not have[pxi]:
        pxi -= 1
    return ("dword", "8-byte", "16-byte")[pxi]


def pixel_form(op, shape, align):
    """Which I/O form the entry point takes for activations of this common alignment: the mix by finc_mix_launch's rule (grad_mat:
    16-byte pieces when HW % 4 == 0 on 16-byte aligned activations, finc_gradw.hip), every other layer by the rule include/finc.h
    states (16-byte pieces when HW % 4 == 0 and every activation pointer is 16-byte aligned, dwords otherwise)."""
    C, HW = shape[1], shape[2] * shape[3]
    wide = "16-byte" if HW % 4 == 0 and align % 16 == 0 else "dword"
    if op == "mix":
        return mix_form(C, HW, align)
    if op == "mix_backward":
        return dict(grad_in=mix_form(C, HW, align), grad_mat=wide)
    return wide


def pixel_cases():
    for op in PIXEL_OPS:
        for shape in (MIX_SHAPES if op.startswith("mix") else PIXEL_SHAPES):
            yield pytest.param(op, shape, id="%s-B%d_C%d_%dx%d" % ((op,) + shape))


@pytest.mark.parametrize("op,shape", list(pixel_cases()))
def test_per_pixel_layer(op, shape, dev):
    """One per-pixel entry point on one shape: its form on 16-byte aligned activations (`pixel_form`: the library's rule, its
    premises asserted; for the mix the expected form stands beside the shape), the same call with every activation one float into
    its allocation (the dword form, compared with the plain call on offset_view), the in-place form the ABI allows in both (same
    bits as out of place), each between guards; (c) against float64 on the CPU; isolation per the operation's definition."""
    spec = pixel_op(op, shape, dev)
    call = lambda ins, guard=False, lead=(), alias=None: run(dev, spec["sym"], spec["argf"], ins, spec["outs"], spec["ws"], guard, lead, alias)
    assert all(v.data_ptr() % 16 == 0 for v in spec["ins"].values())
    form, dword = pixel_form(op, shape, 16), pixel_form(op, shape, 4)
    assert dword in ("dword", dict(grad_in="dword", grad_mat="dword"))
    if op.startswith("mix"):
        assert (form["grad_in"] if op == "mix_backward" else form) == MIX_SHAPES[shape], (form, shape)
    plain = check_bounds(op, lambda guard: call(spec["ins"], guard), dict(kernel=spec["sym"], form=form), judge_outputs(spec["refs"]),
                         shape=list(shape))
    # the dword form of the same numbers: bit-equal to itself between guards, and within the bar of the reference
    shifted = check_bounds(op, lambda guard: call(spec["ins"], guard, spec["acts"]), dict(kernel=spec["sym"], form=dword),
                           judge_outputs(spec["refs"]), shape=list(shape), lead_floats=1)
    if form == dword:
        assert all(same_bits(plain.outs[k], shifted.outs[k]) for k in plain.outs)      # one kernel form, one answer
    if spec["alias"]:
        for lead, base, f in (((), plain, form), (spec["acts"], shifted, dword)):
            inplace = check_bounds(op, lambda guard: call(spec["ins"], guard, lead, spec["alias"]), dict(kernel=spec["sym"], form=f, in_place=True),
                                   shape=list(shape), lead_floats=len(lead) and 1)
            assert all(same_bits(base.outs[k], inplace.outs[k]) for k in base.outs), "in place differs from out of place"
    for lead in ((), spec["acts"]):
        check_isolation(dev, op, lambda ins: call(ins, False, lead), spec["ins"], spec["spots"],
                        dict(kernel=spec["sym"], form=dword if lead else form), spec["values"], shape=list(shape))
