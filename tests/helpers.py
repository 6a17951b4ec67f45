"""Shared helpers for the parity tests (numpy only; torch is imported where a helper needs it)."""
import ctypes
import glob
import os
import shutil
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

ORDER_BITS = {"TL": 0, "TR": 1, "BL": 2, "BR": 3}
ORIENT_FASTFLOW = 0 | (1 << 2) | (2 << 4) | (3 << 6)


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def golden_names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def unit_stored_weights(g):
    """The four state-dict tensors conv_{tl,tr,bl,br}.conv.weight, concatenated on dim 0."""
    return np.concatenate([g["w_tl"], g["w_tr"], g["w_bl"], g["w_br"]], axis=0)


def rel_err(a, b):
    """max |a-b| / max |b|  -- the 'relative fp32 error' of BASELINE.json's north_star."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


# ---------------------------------------------------------------------------
# the per-pixel layers' host and GPU tests (mix backward, coupling, ActNorm)
# ---------------------------------------------------------------------------
def fake_ptr(v):
    """An address for a status-code test: the entry points refuse before anything reads it."""
    return ctypes.c_void_p(v)


def offset_view(t, dev, lead=1):
    """A contiguous device copy of `t` that starts `lead` elements into its allocation.  One float: 4-byte aligned, not 8 or 16; two
    floats: 8-byte aligned, not 16 (the alignment class of the mix's two-pixel form and of F(2,5))."""
    import torch
    buf = torch.empty(t.numel() + lead, dtype=t.dtype, device=dev)
    v = buf[lead:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (lead * t.element_size()) % 16
    return v


def load_stub_library(tmp_path, version, mask_path=True):
    """What `fincflow_amd._lib.lib()` says, in a fresh process, to a library that exports finc_version() = `version` and nothing
    else: the text of its FincError (any other outcome fails the calling test).  `mask_path`: the library's path reads `<lib>` in
    that text, for callers that search it for version numbers."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to build the stub library with"
    d = tmp_path / ("stub" + "abcdef"[version % 6])         # (a directory name without digits, one per version)
    d.mkdir()
    src = d / "old.c"
    src.write_text("int finc_version(void) { return %d; }\n" % version)
    so = d / "libold.so"
    subprocess.check_call([cc, "-shared", "-fPIC", "-o", str(so), str(src)])
    code = ("import sys\n"
            "from fincflow_amd import _lib\n"
            "try:\n"
            "    _lib.lib()\n"
            "except _lib.FincError as e:\n"
            "    print('FincError:', e)\n"
            "    sys.exit(0)\n"
            "except BaseException as e:\n"
            "    print(type(e).__name__, e)\n"
            "    sys.exit(3)\n"
            "sys.exit(4)\n")
    env = dict(os.environ, FINCFLOW_LIB=str(so), PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    return r.stdout.replace(str(so), "<lib>") if mask_path else r.stdout


# ---------------------------------------------------------------------------
# config-4 style stack: one spec, built from the reference's classes by make_golden_stack.py and
# from fincflow_amd.glow by the GPU test; big parameters are filled deterministically instead of stored.
# ---------------------------------------------------------------------------
STACK_SPEC = [
    ("squeeze",),
    ("ffu", 12, 3), ("actnorm", 12), ("conv1x1", 12), ("coupling", (12, 8, 8), 32),
    ("ffu", 12, 3), ("actnorm", 12), ("conv1x1", 12), ("coupling", (12, 8, 8), 32),
    ("squeeze",),
    ("ffu", 48, 3), ("actnorm", 48), ("conv1x1", 48), ("coupling", (48, 4, 4), 32),
]
STACK_INPUT = (2, 3, 16, 16)


def det_fill(name, shape, scale):
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def fill_stack_parameters(layers, ffu_weights=None):
    """Deterministic parameters for every non-FInC layer of a stack built from STACK_SPEC (works on the reference's
    modules and on ours: same parameter names).  FastFlowUnit weights come from `ffu_weights` (fixture) if given."""
    import torch
    with torch.no_grad():
        for idx, (spec, m) in enumerate(zip(STACK_SPEC, layers)):
            kind = spec[0]
            if kind == "actnorm":
                m.translation.copy_(torch.from_numpy(det_fill(f"L{idx}.t", m.translation.shape, 0.1)))
                m.log_scale.copy_(torch.from_numpy(det_fill(f"L{idx}.s", m.log_scale.shape, 0.1)))
                m.initialized.fill_(1)
            elif kind == "conv1x1":
                q = np.linalg.qr(det_fill(f"L{idx}.W", tuple(m.W.shape), 1.0).astype(np.float64))[0]
                m.W.copy_(torch.from_numpy(q.astype(np.float32)))
            elif kind == "coupling":
                for pname, prm in m.net.named_parameters():
                    scale = 0.01 if (pname.endswith("bias") or pname.endswith("logs")) else 0.05
                    prm.copy_(torch.from_numpy(det_fill(f"L{idx}.{pname}", tuple(prm.shape), scale)))
                # In the reference Conv2dZero.bias and .logs are two Parameters over ONE tensor
                # (layers/coupling.py:33-39), so whatever is written last (logs) is the value of both.
                m.net[4].bias.copy_(m.net[4].logs)
            elif kind == "ffu" and ffu_weights is not None:
                for o in ("tl", "tr", "bl", "br"):
                    getattr(m, f"conv_{o}").conv.weight.copy_(torch.from_numpy(ffu_weights[f"L{idx}.{o}"]))


# ---------------------------------------------------------------------------
# error yardsticks and the parity report
# ---------------------------------------------------------------------------
def elem_rel_err(a, b, floor=1e-3):
    """Element-wise relative error max |a-b| / max(|b|, floor * max|b|): every element is judged against its own
    magnitude, down to `floor` of the largest one (below that an fp32 result has no relative meaning)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = np.maximum(np.abs(b), floor * max(np.max(np.abs(b)), 1e-30))
    return float(np.max(np.abs(a - b) / scale))


def report(kind, **fields):
    """Append one line to gpurun_out/parity_report.jsonl (merged back from the GPU box): the achieved errors of every
    parity case, so loosened tolerances are on record.  Best effort -- never fails a test."""
    import json
    try:
        d = os.path.join(REPO, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_report.jsonl"), "a") as f:
            f.write(json.dumps(dict(kind=kind, **fields)) + "\n")
    except OSError:
        pass


# ---------------------------------------------------------------------------
# the MFMA inverse's instantiation table (finc_mfma.hip g_insts), walked by tests
# ---------------------------------------------------------------------------
def problem_counts_for_row(rows, r):
    """Problem counts (B*G) that select row r -- the library's own answer on a 10x32 map, a host-only call: the smallest, and the
    ones next to each max_problems edge of the shape (for the banks the role-split kernel serves: counts beyond its 256 problems)."""
    from fincflow_amd import _lib
    i = rows[r]
    shape = (i["cqp"], i["kh"], i["kw"])
    edges = sorted({x["max_problems"] for x in rows if (x["cqp"], x["kh"], x["kw"]) == shape and x["max_problems"] > 0})
    cands = [1, 2, 3, 4, 6, 8, 257, 258, 259, 260, 262, 264, 513, 514, 515, 516, 518, 520]   # (beyond the role-split kernel's 256 and its short-step form's 512)
    for e in edges:
        cands += [e - 2, e - 1, e, e + 1, e + 2, e + 4]

    def row_of(n):
        B, G, _ = split_problems(n)
        v = _lib.inverse_variant(B, G, i["cqp"], 10, 32, i["kh"], i["kw"])
        return v and v["row"]
    hits = [n for n in sorted(set(cands)) if n > 0 and row_of(n) == r]
    if not hits:
        return []
    out = [hits[0]]
    quad = [n for n in hits if n % 4 == 0]          # a FastFlowUnit-grouped count (G = 4) whenever the row admits one
    if quad:
        out.append(quad[0])
    if edges:                                        # and the counts right at the far side of the edges
        out += [n for n in (max((h for h in hits if h % 2 == 1), default=None),
                            max((h for h in hits if h % 2 == 0), default=None)) if n]
    if len(set(out)) < 2 and len(hits) > 1:
        out.append(hits[1])
    return sorted(set(out))


def split_problems(n):
    """problems -> (B, G, orient): FastFlowUnit grouping when the count allows it, else a single-group layer."""
    if n % 4 == 0:
        return n // 4, 4, ORIENT_FASTFLOW
    return n, 1, n % 4


# ---------------------------------------------------------------------------
# random-shape parity sweep (scripts/fuzz_parity.py and tests/test_gpu_variants.py share the generator)
# ---------------------------------------------------------------------------
def fuzz_case(rng, case):
    K = int(rng.choice([2, 3, 3, 3, 5]))
    # (channel counts between the compiled banks -- 22, 36, 44, 50 at 3x3, 20 at 5x5 -- run on the next larger bank)
    # (72, 96: the big banks of finc_big.hip)
    cq_opts = [1, 2, 3, 4, 6, 8, 12, 16, 20, 22, 24, 28, 32, 36, 40, 44, 48, 50, 64, 72, 96] if K == 3 else \
        ([1, 3, 4, 8, 12, 13, 16, 24, 32] if K == 2 else [2, 4, 8, 12, 16, 20, 32, 48])
    Cq = int(rng.choice(cq_opts))
    G = int(rng.choice([1, 4, 4, 4]))
    H = int(rng.integers(1, 41))
    W = int(rng.choice([rng.integers(1, 41), 4 * rng.integers(1, 12), 8 * rng.integers(1, 9), 16 * rng.integers(1, 5)]))   # W % 16 == 0: the staged forward
    B = int(rng.integers(1, 4))
    if case % 5 == 4:          # every fifth case: more problems than compute units on a small map (the full-chip forms of the inverse)
        B = int(rng.integers(65, 90)) * (4 if G == 1 else 1)
        H = int(rng.integers(1, 20))
        W = int(rng.choice([8, 12, 16, 16, 32]))
    orient = ORIENT_FASTFLOW if G == 4 else int(rng.integers(0, 4))
    std = (0.05 if K < 5 else 0.02) * min(1.0, (24.0 / Cq) ** 0.5)   # keep the operator norm of the bank roughly constant
    return dict(case=case, B=B, G=G, Cq=Cq, H=H, W=W, K=K, orient=orient, std=std)


# ---------------------------------------------------------------------------
# guard bands and problem isolation (tests/test_gpu_bounds.py on the GPU, tests/test_bounds_host.py for the helpers themselves)
# ---------------------------------------------------------------------------
GUARD_BITS = {2: 0x7FCB, 4: 0x7FC0BEEF, 8: 0x7FF80000_00C0BEEF}      # one quiet NaN per element size (2: bfloat16), recognisable in a dump


def _as_ints(t):
    import torch
    assert t.dtype in (torch.float32, torch.float64, torch.bfloat16), t.dtype
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def guard_elements(t):
    """Elements of ONE guard of `t`: a 16-channel padded tile of the map for activations (the largest over-reach by one tile), 4096
    for everything else; a multiple of 128 elements (512 bytes), so the payload keeps the alignment class of a fresh allocation."""
    n = max(4096, 16 * t.shape[2] * t.shape[3]) if t.dim() == 4 else 4096
    return (n + 127) // 128 * 128


def nan_filled(shape, dtype, dev):
    """A fresh tensor whose every element is the guards' NaN pattern (outputs and workspaces: whatever is left of it was not written)."""
    import torch
    out = torch.empty(shape, dtype=dtype, device=dev)
    _as_ints(out).fill_(GUARD_BITS[out.element_size()])
    return out


def guarded(t, dev, lead_floats=0):
    """(view, buffer): a contiguous view holding `t`'s values inside one larger buffer laid out [front guard | payload | back guard],
    both guards filled with GUARD_BITS.  `lead_floats` = 1 shifts the payload by one element (4-byte aligned, not 16: the dword
    forms, to be compared with the plain call on `offset_view`)."""
    g, n = guard_elements(t), t.numel()
    buf = nan_filled((2 * g + n + lead_floats,), t.dtype, dev)
    view = buf[g + lead_floats:g + lead_floats + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() - buf.data_ptr()) % 512 == lead_floats * t.element_size()
    return view, buf


def _guard_spans(buffer, view):
    off = (view.data_ptr() - buffer.data_ptr()) // buffer.element_size()
    assert 0 <= off and off + view.numel() <= buffer.numel() and buffer.dtype == view.dtype
    ints = _as_ints(buffer)
    return ints[:off], ints[off + view.numel():]


def guards_intact(buffer, view):
    """Do both guards around `view` still hold the fill pattern, bit for bit?"""
    bits = GUARD_BITS[buffer.element_size()]
    return all(bool((span == bits).all()) for span in _guard_spans(buffer, view))


def broken_guards(buffer, view):
    """Which guards of `buffer` were written: a list out of "front", "back" (what a failing test prints)."""
    bits = GUARD_BITS[buffer.element_size()]
    return [name for name, span in zip(("front", "back"), _guard_spans(buffer, view)) if not bool((span == bits).all())]


def poison(t, index, value=float("nan")):
    """A clone of `t` with t[index] set to NaN."""
    c = t.clone()
    c[index] = value
    return c


def poison_inf(t, index):
    return poison(t, index, float("inf"))


def same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_as_ints(a.contiguous()), _as_ints(b.contiguous()))


def isolation_check(clean, dirty, reach):
    """The isolation comparison: `reach` is a boolean mask of the output elements the poison can reach by the operation's
    definition.  Returns (leaked, reached): the number of elements OUTSIDE the mask whose bits differ from the clean run, and whether
    the part inside holds a non-finite value at all (the poison was read: the comparison is not vacuous)."""
    import torch
    reach = reach.expand_as(clean) if reach.shape != clean.shape else reach
    leaked = int(((_as_ints(clean.contiguous()) != _as_ints(dirty.contiguous())) & ~reach).sum())
    reached = bool((~torch.isfinite(dirty[reach])).any())
    return leaked, reached


# float64 formulas of the per-pixel layers (layers/coupling.py:79-101, layers/actnorm.py:34, :51, :57-65): the references of
# tests/test_gpu_bounds.py, and what tests/test_bounds_host.py shows to be isolated themselves
def coupling_ref(x, raw, a, b, direction):
    """(y, logdet) of the forward direction, (y, None) of the reverse."""
    import torch
    half = x.shape[1] // 2
    h = a.view(1, -1, 1, 1) * raw + b.view(1, -1, 1, 1)
    s = 2.0 * torch.tanh(h[:, ::2] / 2.0)
    sh = h[:, 1::2]
    if direction > 0:
        return torch.cat([x[:, :half], x[:, half:] * torch.exp(s) + sh], 1), s.flatten(1).sum(-1)
    return torch.cat([x[:, :half], (x[:, half:] - sh) * torch.exp(-s)], 1), None


def actnorm_ref(x, ls, tr, direction):
    import torch
    if direction > 0:
        return (x - tr.view(1, -1, 1, 1)) * torch.exp(-ls.view(1, -1, 1, 1)), (-ls.sum() * x.shape[2] * x.shape[3]).expand(x.shape[0])
    return x * torch.exp(ls.view(1, -1, 1, 1)) + tr.view(1, -1, 1, 1), None
