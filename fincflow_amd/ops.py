"""Host-side operators over the C ABI (include/finc.h).

`inverse(input, kernel, output)` mirrors the reference's one native op
(fastflow/utils/fastflow_cuda_inverse/cinc_cuda_level2.cpp:19-32): same name,
same argument meaning, same in-place-and-return-alias behaviour, same
RuntimeError for non-device / non-contiguous tensors.  `finc_inverse` /
`finc_forward` are the orientation-aware calls FastFlowUnit uses (no flips, no
chunk/cat copies: fastflow.py:78-100 collapses into one launch).
"""
import contextlib
import math
import threading

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import _lib

ORDER_BITS = {"TL": 0, "TR": 1, "BL": 2, "BR": 3}
ORIENT_FASTFLOW = 0xE4  # TL,TR,BL,BR (fastflow.py:24-27)

_workspaces = {}
_reverse_grad = threading.local()


@contextlib.contextmanager
def reverse_grad():
    """Inside this context the `reverse` of FastFlowUnit, PaddedConv2d and CINCFlowUnit is differentiable: whenever autograd is
    recording (grad enabled, the input or a weight requires grad) it goes through `inverse_reverse` -- the same cached launch, with a
    backward on the HIP kernels (finc_adjoint_weights_f32, the inverse itself on the adjoint bank, finc_lead_product_f32,
    finc_backward_f32) -- and returns a tensor attached to the graph.  Outside it `reverse` is what it always was: detached.  The flag
    is per thread and nests."""
    depth = getattr(_reverse_grad, "depth", 0)
    _reverse_grad.depth = depth + 1
    try:
        yield
    finally:
        _reverse_grad.depth = depth


def reverse_grad_enabled():
    return getattr(_reverse_grad, "depth", 0) > 0


_recorded_net = threading.local()


@contextlib.contextmanager
def recorded_net():
    """Inside this context a layer whose no-grad path computes its net in another way than its recording path does (glow.Coupling:
    bias + ReLU fused behind bias-free convolutions) uses the recording path's arithmetic, without recording.  What
    `FlowSequential.invertible_backward` enters around a run's forward under autocast: its backward rebuilds each input from the
    output with the RECORDING path's net, and in a 16-bit dtype the two paths round at different points.  Per thread; nests."""
    depth = getattr(_recorded_net, "depth", 0)
    _recorded_net.depth = depth + 1
    try:
        yield
    finally:
        _recorded_net.depth = depth


def recorded_net_enabled():
    return getattr(_recorded_net, "depth", 0) > 0


def _stream_ptr(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _require_device(t, name, dtype=torch.float32):
    # same conditions, same exception type as CHECK_INPUT (cinc_cuda_level2.cpp:15-17)
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (fincflow_amd has no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")


def _float_dtype(t, name):
    """float and double, the reference op's dispatch (AT_DISPATCH_FLOATING_TYPES, cinc_cuda_kernel_level2.cu:117)."""
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {t.dtype}")
    return t.dtype


def _out_like(x, out, dtype=torch.float32):
    if out is None:
        return torch.empty_like(x)
    _require_device(out, "output", dtype)
    if out.shape != x.shape or out.device != x.device:
        raise ValueError("output must match input in shape and device")
    return out


def _per_channel(x, label, *tensors):
    if any(t.numel() != x.shape[1] or t.device != x.device for t in tensors):
        raise ValueError(f"{label} must have one entry per channel, on the activations' device")


def _per_image(t, name, x):
    if t is not None:
        _require_device(t, name)
        if t.numel() != x.shape[0] or t.device != x.device:
            raise ValueError(f"{name} must have one entry per image, on the activations' device")


def _ptr(t):
    return t.data_ptr() if t is not None else None


_steps = [0]


def _after_optimizer_step(optimizer, args, kwargs):
    _steps[0] += 1


# PyTorch's fused optimisers (Adam / AdamW / SGD with fused=True) update the parameters in one kernel that does NOT advance
# Tensor._version: keyed on (address, version counter) alone, every value derived from a parameter would outlive such a step and a
# sample would come from last step's weights.  So the key also carries the number of optimiser steps this process has taken, any
# torch.optim optimiser's: after a step every derived value is rebuilt on its next use -- as it is after a step that does bump the
# counters -- and a process that only samples never takes one.
register_optimizer_step_post_hook(_after_optimizer_step)


def version_key(*tensors):
    """(optimiser steps taken so far, then address and version counter of every tensor), flat: what the caches of values derived from
    parameters are keyed on.  Writes that neither bump `Tensor._version` nor are a torch.optim step (collectives, `.data`) still need
    `PackedWeights.invalidate()`."""
    return (_steps[0],) + tuple(v for t in tensors for v in (t.data_ptr(), t._version))


def _current_stream(device):
    return torch.cuda.current_stream(device)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _current_handle(device):
    """The current stream's handle on `device`: what a token compares on every use until it is done.  torch's raw getter where the
    build has it (a thread-local read: no Stream object is made for the comparison), else the public one."""
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return _current_stream(device).cuda_stream


def _capturing():
    return torch.cuda.is_current_stream_capturing()


CAPTURE_IN_FLIGHT = ("a value derived from the parameters is still being built on another stream: synchronise (or let the capturing stream "
                     "wait for the stream that first used the module) before capturing")


class Ready:
    """The readiness token of ONE cache entry of values derived from parameters (the banks of PackedWeights, the folded matrices of
    glow.Conv1x1, glow.Coupling's scale and shift): made where the entry is built, right behind its last fill launch, it keeps the
    building stream's handle, an event recorded there and a `done` flag.  `wait(*tensors)` in front of every use of the entry:

      * `done`, or the current stream is the building stream: nothing (stream order covers it);
      * the event has completed: `done` for good -- the event is never asked again;
      * otherwise the current stream waits for the event, and the entry's tensors are marked as used on it (`record_stream`: their
        memory is not handed out again while this stream may still read it).  Inside a stream capture that raises instead: an event
        from outside must not enter the graph.

    An entry on the host is born `done`.  An entry built INSIDE a capture has no event (it is filled when the graph replays, in the
    graph's own order); another stream that asks for it is refused."""
    __slots__ = ("stream", "event", "done")

    def __init__(self, device):
        self.stream = self.event = None
        self.done = device.type != "cuda"
        if not self.done:
            stream = _current_stream(device)
            self.stream = stream.cuda_stream
            if not _capturing():
                self.event = stream.record_event()

    def wait(self, *tensors):
        if self.done:
            return
        device = tensors[0].device
        if _current_handle(device) == self.stream:
            return
        stream = _current_stream(device)
        if self.event is None:
            raise RuntimeError("a value derived from the parameters was built inside a stream capture and is asked for on another "
                               "stream: call the module once outside the capture first")
        if self.event.query():
            self.done = True
            return
        if _capturing():
            raise RuntimeError(CAPTURE_IN_FLIGHT)
        stream.wait_event(self.event)
        for t in tensors:
            if t is not None:
                t.record_stream(stream)


def _nothing_to_launch(x, grads, sums):
    """An empty batch (the sums over it are zero) or no gradient asked for: `grads` is the result as it stands."""
    if x.numel() == 0:
        for t in sums:
            if t is not None:
                t.zero_()
        return True
    return all(g is None for g in grads)


def _call(name, device, *args, may_refuse=False):
    """One entry point of the library under the device guard, its status checked under the same name.  `may_refuse`: hand
    FINC_ERR_UNSUPPORTED (3) back to a caller that has another path; every other failure raises here all the same.
    (The symbol is looked up on `_lib.lib()` per call, as every call site did: ctypes keeps a bound symbol in the library object's
    own dict, and bench.py swaps that object for one pass to bracket the launches.)"""
    fn = getattr(_lib.lib(), name)
    with torch.cuda.device(device):
        st = fn(*args)
    if st and not (may_refuse and st == 3):
        _lib.check(st, name)
    return st


def release_workspaces():
    """Drop every cached per-(device, stream) scratch buffer (they are re-created on demand).  For long-lived
    processes that cycle through many streams; call it at a synchronisation point."""
    _workspaces.clear()


def _workspace(device, nbytes):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _ws_args(device, nbytes):
    """(pointer, size) of the stream's scratch buffer grown to `nbytes`; (None, 0) for a call that needs none (`nbytes` None)."""
    if nbytes is None:
        return None, 0
    ws = _workspace(device, nbytes)
    return ws.data_ptr(), ws.numel()


def _dims(act, w, G):
    if act.dim() != 4 or w.dim() != 4:
        raise ValueError("expected activations [B,C,H,W] and weights [G*Cq,Cq,KH,KW]")
    B, C, H, W = act.shape
    if C % G != 0:
        raise ValueError(f"channels {C} not divisible by groups {G}")
    Cq = C // G
    if w.shape[0] != C or w.shape[1] != Cq:
        raise ValueError(f"weights {tuple(w.shape)} do not match C={C}, Cq={Cq}")
    if act.device != w.device:
        raise ValueError("activations and weights on different devices")
    return B, Cq, H, W, w.shape[2], w.shape[3]


def canonicalize(w_stored, G, orient):
    """State-dict form -> TL-canonical (fastflow.py:79-84).  The flip is an involution, so the same call
    maps canonical gradients back to stored form."""
    dt = _float_dtype(w_stored, "weights")
    _require_device(w_stored, "weights", dt)
    out = torch.empty_like(w_stored)
    Cq = w_stored.shape[0] // G
    fn = "finc_canonicalize_weights_f32" if dt == torch.float32 else "finc_canonicalize_weights_f64"
    _call(fn, w_stored.device, w_stored.data_ptr(), out.data_ptr(), G, Cq, w_stored.shape[2], w_stored.shape[3], orient,
          _stream_ptr(w_stored))
    return out


def check_invariant(w_canon, G):
    """Raises if the corner tap is not unit lower triangular (layers/conv.py:63-70).  Synchronises.  float32 or float64."""
    dt = _float_dtype(w_canon, "weights")
    _require_device(w_canon, "weights", dt)
    _call("finc_check_invariant_f32" if dt == torch.float32 else "finc_check_invariant_f64", w_canon.device, w_canon.data_ptr(), G,
          w_canon.shape[0] // G, w_canon.shape[2], w_canon.shape[3], _stream_ptr(w_canon))


def _run(fn_name, act, w_canon, G, orient, algo, out):
    dt = _float_dtype(act, "input")
    _require_device(act, "input", dt)
    _require_device(w_canon, "kernel", dt)
    B, Cq, H, W, KH, KW = _dims(act, w_canon, G)
    out = _out_like(act, out, dt)
    if act.numel() == 0:
        return out
    L = _lib.lib()
    run = (act.data_ptr(), w_canon.data_ptr(), out.data_ptr(), B, G, Cq, H, W, KH, KW, orient)
    if dt == torch.float64:
        # strict: the reference-order fp64 kernels (bit-exact with the reference's Cython solver; no packed form, no workspace);
        # auto / mfma: the matrix-core form where the bank has one (finc_f64.hip: Cq <= 24 at 3x3, <= 32 at 2x2 on one wave per
        # problem, 29 .. 64 at 3x3 and 33 .. 64 at 2x2 split over a workgroup's waves), else strict
        fn64 = fn_name.replace("_f32", "_f64")
        if algo == "strict":
            _call(fn64, act.device, *run, _stream_ptr(act))
        else:
            _call(fn64 + "_algo", act.device, *run, _lib.ALGO[algo], *_ws_args(act.device, L.finc_f64_workspace_bytes(G, Cq, KH, KW)),
                  _stream_ptr(act))
        return out
    if fn_name == "finc_inverse_f32":      # room for the zero-padded copy an odd width is solved on
        nbytes = L.finc_inverse_workspace_bytes(B, G, Cq, H, W, KH, KW)
    else:
        nbytes = L.finc_workspace_bytes(G, Cq, KH, KW)
    _call(fn_name, act.device, *run, _lib.ALGO[algo], *_ws_args(act.device, nbytes), _stream_ptr(act))
    return out


def finc_inverse(z, w_canon, G=4, orient=ORIENT_FASTFLOW, algo="auto", out=None):
    """x = inverse(z) for G groups with per-group orientation; one asynchronous launch on the current stream."""
    return _run("finc_inverse_f32", z, w_canon, G, orient, algo, out)


def finc_forward(x, w_canon, G=4, orient=ORIENT_FASTFLOW, algo="auto", out=None):
    """z = forward(x); the layer's logdet is identically 0 (layers/conv.py:106)."""
    return _run("finc_forward_f32", x, w_canon, G, orient, algo, out)


def finc_backward(grad_z, x, w_canon, G, orient, need_gx=True, need_gw=True):
    """(grad_x, grad_w_canon) of z = forward(x), each computed only if asked for (None otherwise); the corner-tap mask is applied
    in-kernel.  float32 (finc_backward_f32) or float64 (finc_backward_f64), taken from `grad_z`: `x` and `w_canon` must match it."""
    dt = _float_dtype(grad_z, "grad_output")
    _require_device(grad_z, "grad_output", dt)
    _require_device(w_canon, "kernel", dt)
    if x is not None:
        _require_device(x, "input", dt)
    B, Cq, H, W, KH, KW = _dims(grad_z, w_canon, G)
    gx = torch.empty_like(grad_z) if need_gx else None
    gw = torch.empty_like(w_canon) if need_gw else None
    if grad_z.numel() == 0:
        if gw is not None:
            gw.zero_()
        return gx, gw
    if gx is None and gw is None:
        return gx, gw
    fn, ws = ("finc_backward_f32", "finc_backward_workspace_bytes") if dt == torch.float32 else \
        ("finc_backward_f64", "finc_backward_f64_workspace_bytes")
    _call(fn, grad_z.device, grad_z.data_ptr(), _ptr(x), w_canon.data_ptr(), _ptr(gx), _ptr(gw), B, G, Cq, H, W, KH, KW,
          orient, *_ws_args(grad_z.device, getattr(_lib.lib(), ws)(B, G, Cq, H, W, KH, KW)), _stream_ptr(grad_z))
    return gx, gw


def mix_supported(C):
    return bool(_lib.lib().finc_mix_supported_f32(int(C)))


def finc_mix(x, mat, bias=None, out=None):
    """out[b, :, h, w] = mat @ x[b, :, h, w] + bias: the 1x1 convolution of a flow step (layers/conv1x1.py:29-43) with
    whatever per-channel affine neighbour the caller folded into `mat` / `bias`, as one streaming HIP launch.
    x [B,C,H,W] fp32 contiguous on the device, mat [C,C] (out, in), bias [C] or None.  `out` may be `x`."""
    _require_device(x, "input")
    _require_device(mat, "matrix")
    if x.dim() != 4 or mat.shape != (x.shape[1], x.shape[1]) or mat.device != x.device:
        raise ValueError("expected activations [B,C,H,W] and a [C,C] matrix on the same device")
    if bias is not None:
        _require_device(bias, "bias")
        if bias.numel() != x.shape[1]:
            raise ValueError("bias must have one entry per channel")
    out = _out_like(x, out)
    if x.numel() == 0:
        return out
    B, C, H, W = x.shape
    _call("finc_mix_f32", x.device, x.data_ptr(), mat.data_ptr(), _ptr(bias), out.data_ptr(), B, C, H * W, _stream_ptr(x))
    return out


def finc_mix_backward(grad_out, x, mat, need_gx=True, need_gm=True, need_gb=False):
    """Gradients of `finc_mix` (autograd through F.conv2d, layers/conv1x1.py:29-31): grad_x = mat^T @ grad_out per pixel,
    grad_mat[o][i] = sum grad_out[:, o] * x[:, i], grad_bias[o] = sum grad_out[:, o]; each is computed only if asked for (None
    otherwise).  grad_out, x [B,C,H,W] fp32 contiguous on the device (`x` may be None without grad_mat), mat [C,C] the forward
    matrix.  The sums run in a fixed order: the same inputs give the same bits."""
    _require_device(grad_out, "grad_output")
    _require_device(mat, "matrix")
    if grad_out.dim() != 4 or mat.shape != (grad_out.shape[1], grad_out.shape[1]) or mat.device != grad_out.device:
        raise ValueError("expected a gradient [B,C,H,W] and a [C,C] matrix on the same device")
    if need_gm:
        if x is None:
            raise ValueError("grad_mat needs the forward's input")
        _require_device(x, "input")
        if x.shape != grad_out.shape or x.device != grad_out.device:
            raise ValueError("input must match grad_output in shape and device")
    B, C, H, W = grad_out.shape
    gx = torch.empty_like(grad_out) if need_gx else None
    gm = torch.empty_like(mat) if need_gm else None
    gb = torch.empty(C, dtype=torch.float32, device=grad_out.device) if need_gb else None
    if _nothing_to_launch(grad_out, (gx, gm, gb), (gm, gb)):
        return gx, gm, gb
    nbytes = _lib.lib().finc_mix_backward_workspace_bytes(B, C, H * W) if (need_gm or need_gb) else None
    _call("finc_mix_backward_f32", grad_out.device, grad_out.data_ptr(), _ptr(x) if need_gm else None, mat.data_ptr(), _ptr(gx), _ptr(gm),
          _ptr(gb), B, C, H * W, *_ws_args(grad_out.device, nbytes), _stream_ptr(grad_out))
    return gx, gm, gb


class _FincMixFunction(torch.autograd.Function):
    """`finc_mix` under autograd: both directions on the HIP kernels (finc_mix_f32 / finc_mix_backward_f32)."""

    @staticmethod
    def forward(ctx, x, mat, bias):
        x = x.contiguous()
        mat = mat.contiguous()
        out = finc_mix(x, mat, None if bias is None else bias.contiguous())
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, mat)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, mat = ctx.saved_tensors
        gx, gm, gb = finc_mix_backward(grad_out.contiguous(), x, mat, need_gx=ctx.needs_input_grad[0],
                                       need_gm=ctx.needs_input_grad[1], need_gb=ctx.needs_input_grad[2])
        return gx, gm, gb


def mix_forward(x, mat, bias=None):
    """`finc_mix(x, mat, bias)` under autograd: gradients for `x`, `mat` and `bias`, each computed only where needed."""
    return _FincMixFunction.apply(x, mat, bias)


def plu_supported(C):
    """Does the library compose a [C, C] matrix from its PLU parameters (1 <= C <= 512)?"""
    return bool(_lib.lib().finc_plu_supported_f32(int(C)))


def _plu_args(lower, upper, log_s, sign_s, perm):
    for t, name in ((lower, "lower"), (upper, "upper"), (log_s, "log_s"), (sign_s, "sign_s")):
        _require_device(t, name)
    _require_device(perm, "perm", torch.int32)
    C = log_s.numel()
    if C < 1 or lower.shape != (C, C) or upper.shape != (C, C) or sign_s.shape != (C,) or perm.shape != (C,) or log_s.dim() != 1:
        raise ValueError("expected lower, upper [C,C] and log_s, sign_s, perm [C]")
    if any(t.device != lower.device for t in (upper, log_s, sign_s, perm)):
        raise ValueError("the PLU parameters must be on one device")
    return C


def finc_plu_compose(lower, upper, log_s, sign_s, perm, need_w=True, need_winv=True, need_logdet=True):
    """The matrix of a PLU-parametrised 1x1 convolution (glow.Conv1x1LU), its inverse and its log-det in ONE HIP launch:
    W = P L Ut with L = strict_lower(lower) + I, Ut = strict_upper(upper) + diag(sign_s * exp(log_s)), W[r] = (L Ut)[perm[r]];
    W^-1 by two triangular solves per column; log|det W| = sum(log_s), 0-dim.  lower, upper [C,C], log_s, sign_s [C] fp32, perm [C]
    int32 contiguous on the device.  Returns (w, w_inv, logdet), each computed only if asked for (None otherwise).  Computed in
    fp64, rounded to fp32 once, in a fixed order: the same inputs give the same bits.  Nothing is recorded for autograd
    (`plu_compose` does that)."""
    C = _plu_args(lower, upper, log_s, sign_s, perm)
    if not (need_w or need_winv or need_logdet):
        return None, None, None
    w = torch.empty_like(lower) if need_w else None
    w_inv = torch.empty_like(lower) if need_winv else None
    logdet = torch.empty((), dtype=torch.float32, device=lower.device) if need_logdet else None
    _call("finc_plu_compose_f32", lower.device, lower.data_ptr(), upper.data_ptr(), log_s.data_ptr(), sign_s.data_ptr(), perm.data_ptr(),
          _ptr(w), _ptr(w_inv), _ptr(logdet), C, _stream_ptr(lower))
    return w, w_inv, logdet


def finc_plu_compose_backward(grad_w, grad_logdet, lower, upper, log_s, sign_s, perm, need_glower=True, need_gupper=True,
                              need_glog_s=True):
    """Gradients of `finc_plu_compose` (include/finc.h: finc_plu_compose_backward_f32) from grad_w [C,C] = dl/dW and grad_logdet
    (0-dim or None: zero): (grad_lower, grad_upper, grad_log_s), each computed only if asked for (None otherwise), ONE launch.  The
    entries outside the strict triangles are exact zeros, written by the kernel.  (A gradient through W^-1 is folded into grad_w
    first: `plu_compose` does that.)"""
    C = _plu_args(lower, upper, log_s, sign_s, perm)
    _require_device(grad_w, "grad_w")
    if grad_w.shape != (C, C) or grad_w.device != lower.device:
        raise ValueError("grad_w must be [C,C] on the parameters' device")
    if grad_logdet is not None:
        _require_device(grad_logdet, "grad_logdet")
        if grad_logdet.numel() != 1 or grad_logdet.device != lower.device:
            raise ValueError("grad_logdet must hold one value on the parameters' device")
    gl = torch.empty_like(lower) if need_glower else None
    gu = torch.empty_like(upper) if need_gupper else None
    gs = torch.empty_like(log_s) if need_glog_s else None
    if gl is None and gu is None and gs is None:
        return gl, gu, gs
    _call("finc_plu_compose_backward_f32", lower.device, grad_w.data_ptr(), _ptr(grad_logdet), lower.data_ptr(), upper.data_ptr(),
          log_s.data_ptr(), sign_s.data_ptr(), perm.data_ptr(), _ptr(gl), _ptr(gu), _ptr(gs), C, _stream_ptr(lower))
    return gl, gu, gs


class _FincPluComposeFunction(torch.autograd.Function):
    """`finc_plu_compose` under autograd: (w, w_inv, logdet) recorded as one node, its backward one launch.  A gradient that arrives
    through w_inv is folded into the one on w first, dl/dW = grad_w - W^-T grad_winv W^-T (two [C, C] matmuls, in fp64)."""

    @staticmethod
    def forward(ctx, lower, upper, log_s, sign_s, perm, need_w, need_winv, need_logdet):
        lower, upper, log_s = lower.contiguous(), upper.contiguous(), log_s.contiguous()
        w, w_inv, logdet = finc_plu_compose(lower, upper, log_s, sign_s, perm, need_w, need_winv, need_logdet)
        ctx.save_for_backward(lower, upper, log_s, sign_s, perm, w_inv)
        ctx.set_materialize_grads(False)
        return w, w_inv, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_w, grad_winv, grad_logdet):
        lower, upper, log_s, sign_s, perm, w_inv = ctx.saved_tensors
        need = ctx.needs_input_grad[:3]
        if grad_winv is not None:
            wt = w_inv.t().double()              # (in fp64 like the kernels: at cond(W) in the thousands an fp32 product is the error)
            through = wt @ grad_winv.double() @ wt
            grad_w = (-through if grad_w is None else grad_w.double() - through).float()
        if grad_logdet is not None:
            grad_logdet = grad_logdet.contiguous()
        if grad_w is None:                       # the log-det alone: every grad_log_s is grad_logdet, nothing reaches the triangles
            gs = grad_logdet.expand(log_s.shape).clone() if (need[2] and grad_logdet is not None) else None
            return (None, None, gs) + (None,) * 5
        gl, gu, gs = finc_plu_compose_backward(grad_w.contiguous(), grad_logdet, lower, upper, log_s, sign_s, perm, *need)
        return (gl, gu, gs) + (None,) * 5


def plu_compose(lower, upper, log_s, sign_s, perm, need_w=True, need_winv=True, need_logdet=True):
    """`finc_plu_compose` under autograd: gradients for lower, upper and log_s, each computed only where needed, in one launch;
    an output nobody asked for is None and costs nothing."""
    return _FincPluComposeFunction.apply(lower, upper, log_s, sign_s, perm, bool(need_w), bool(need_winv), bool(need_logdet))


def coupling_supported(C):
    return bool(_lib.lib().finc_coupling_supported_f32(int(C)))


#: the element types of `raw` (the coupling net's output) that have kernels, and the suffix of their entry points: fp32, and
#: bfloat16 for a net that ran under torch.autocast(device_type="cuda", dtype=torch.bfloat16).  Everything else stays fp32.
_RAW_ENTRY = {torch.float32: "_f32", torch.bfloat16: "_rawbf16_f32"}


def _coupling_entry(name, raw, family="finc_coupling"):
    """`finc_coupling<name>` (or `<family><name>`: "finc_split_prior") for the element type of `raw`."""
    return family + name + _RAW_ENTRY[raw.dtype]


def _coupling_args(x, raw, a, b, what="input", halves=()):
    """`halves`: the split prior's half tensors [B,C/2,H,W] that the call reads or writes (None: absent); `x` None: a call whose
    whole tensor is its output (`finc_split_prior_merge`)."""
    if x is not None:
        _require_device(x, what)
    _require_device(raw, "raw", raw.dtype if raw.dtype in _RAW_ENTRY else torch.float32)
    _require_device(a, "scale")
    _require_device(b, "shift")
    if raw.dim() != 4 or (x is not None and (raw.shape != x.shape or raw.device != x.device)):
        raise ValueError(f"expected {what} [B,C,H,W] and the coupling net's output of the same shape on the same device")
    C = raw.shape[1]
    for h in halves:
        if h is not None:
            _require_device(h, "half tensor")
            if h.shape != (raw.shape[0], C // 2) + raw.shape[2:] or h.device != raw.device:
                raise ValueError("expected half tensors [B,C/2,H,W] beside the coupling net's output [B,C,H,W], on the same device")
    _per_channel(raw, "scale and shift", a, b)
    if not coupling_supported(C):
        raise _lib.FincError(f"finc_coupling: no kernel for {C} channels (the coupling splits an even channel count)")


def _coupling_transform(entry, x, raw, a, b, direction, want_logdet, out, family="finc_coupling"):
    """`finc_coupling_f32` (which takes the direction) or `finc_coupling_reverse_logdet_f32` behind their wrappers, or their
    `_rawbf16_f32` siblings for a bfloat16 `raw` (`entry`: the name between "finc_coupling" and that suffix): (y, logdet), fp32.
    The split prior's transforms (`family` "finc_split_prior") have two half tensors on one side: `x` or `out` is then the tuple of
    them, in the entry point's order, and the result is (*out, log_p)."""
    entry = _coupling_entry(entry, raw, family)
    ins = x if isinstance(x, tuple) else (x,)
    outs = out if isinstance(out, tuple) else (_out_like(x, out),)
    B, C, H, W = raw.shape
    if raw.numel() == 0:
        return outs + (torch.zeros(B, dtype=torch.float32, device=raw.device) if want_logdet else None,)
    logdet = torch.empty(B, dtype=torch.float32, device=raw.device) if want_logdet else None
    nbytes = _lib.lib().finc_coupling_workspace_bytes(B, C, H * W) if want_logdet else None
    _call(entry, raw.device, *map(_ptr, ins), raw.data_ptr(), a.data_ptr(), b.data_ptr(), *map(_ptr, outs), _ptr(logdet), B, C, H * W,
          *direction, *_ws_args(raw.device, nbytes), _stream_ptr(raw))
    return outs + (logdet,)


def finc_coupling(x, raw, a, b, direction=1, want_logdet=False, out=None):
    """The affine coupling behind its net (layers/coupling.py:79-101) as one streaming HIP launch: with h = a * raw + b per channel,
    s = 2 tanh(h[:, ::2] / 2), t = h[:, 1::2]:  y = cat(x1, x2 * exp(s) + t) (direction +1) or cat(x1, (x2 - t) * exp(-s)) (-1).
    x, raw [B,C,H,W] fp32 contiguous on the device, C even; a, b [C].  Returns (y, logdet): logdet [B] = s summed per image when
    `want_logdet` (forward direction; one more small launch, fixed-order sums), else None.  `out` may be `x`.
    `raw` may also be bfloat16 (a net under bf16 autocast): it is read as it lies by finc_coupling_rawbf16_f32, no cast in front; x, a,
    b, y and logdet stay fp32 and have the bits of the call on `raw.float()`.  The same holds for every coupling call below; the
    backwards then return grad_raw in bfloat16 (the fp32 value rounded to nearest even once).  Any other dtype raises."""
    _coupling_args(x, raw, a, b)
    if direction not in (1, -1):
        raise ValueError("direction must be +1 (forward) or -1 (reverse)")
    return _coupling_transform("", x, raw, a, b, (direction,), bool(want_logdet) and direction == 1, out)


def _coupling_grads(entry, grad_y, grad_logdet, v, raw, a, b, what, whose, need_acts, need_sums, family="finc_coupling",
                    half_outs=False):
    """One backward entry point of the coupling behind its wrapper: the checks, the outputs asked for -- `need_acts`: (x,) grad_x,
    grad_raw; `need_sums`: grad_a, grad_b -- the workspace and the call.  `v`: the activation that entry point reads, "input" or
    "output" (`what`) of `whose` pass; grad_logdet: a tuple, empty for the entry point that takes none.  `entry`: the name between
    "finc_coupling" (or `family`) and the suffix of `raw`'s element type; grad_raw is allocated like `raw` (bfloat16 for a bfloat16
    `raw`).  grad_y as a tuple: the gradients of the split prior's two half tensors, each of which may be None (absent: NULL).
    `half_outs` (the merges' backward): grad_y is the gradient of the whole tensor and may be None (absent: NULL), and the
    activation-like outputs in front of grad_raw are half tensors [B,C/2,H,W]."""
    if isinstance(grad_y, tuple):
        _coupling_args(v, raw, a, b, what, halves=grad_y)
    else:
        _coupling_args(v, raw, a, b, what)
        if grad_y is not None or not half_outs:
            _require_device(grad_y, "grad_output")
            if grad_y.shape != v.shape or grad_y.device != v.device:
                raise ValueError(f"grad_output must match {whose} in shape and device")
        grad_y = (grad_y,)
    entry = _coupling_entry(entry, raw, family)
    B, C, H, W = v.shape
    for g in grad_logdet:
        _per_image(g, "grad_logdet", v)
    sums = tuple(torch.empty(C, dtype=torch.float32, device=v.device) if n else None for n in need_sums)
    if half_outs:
        outs = tuple(torch.empty(B, C // 2, H, W, dtype=v.dtype, device=v.device) if n else None for n in need_acts[:-1])
        outs += (torch.empty_like(raw) if need_acts[-1] else None,) + sums
    else:
        acts = (v,) * (len(need_acts) - 1) + (raw,)               # (x,) grad_x like the activations, grad_raw like raw
        outs = tuple(torch.empty_like(t) if n else None for t, n in zip(acts, need_acts)) + sums
    if _nothing_to_launch(v, outs, sums):
        return outs
    nbytes = _lib.lib().finc_coupling_workspace_bytes(B, C, H * W) if any(need_sums) else None
    _call(entry, v.device, *map(_ptr, grad_y), *map(_ptr, grad_logdet), v.data_ptr(), raw.data_ptr(), a.data_ptr(), b.data_ptr(),
          *map(_ptr, outs), B, C, H * W, *_ws_args(v.device, nbytes), _stream_ptr(v))
    return outs


def finc_coupling_backward(grad_y, grad_logdet, x, raw, a, b, need_gx=True, need_graw=True, need_ga=True, need_gb=True):
    """Gradients of `finc_coupling(..., direction=1, want_logdet=True)` (include/finc.h: finc_coupling_backward_f32), given grad_y
    [B,C,H,W] and grad_logdet [B] or None (zeros): (grad_x, grad_raw, grad_a, grad_b), each computed only if asked for (None
    otherwise).  grad_x[:, :C/2] is grad_y[:, :C/2]: what reaches that half through the net is the caller's (autograd's).  s and exp(s)
    are recomputed from `raw`; the per-channel sums run in a fixed order: the same inputs give the same bits."""
    return _coupling_grads("_backward", grad_y, (grad_logdet,), x, raw, a, b, "input", "input", (need_gx, need_graw),
                           (need_ga, need_gb))


def finc_coupling_reverse_backward(grad_y, y, raw, a, b, need_gx=True, need_graw=True, need_ga=True, need_gb=True):
    """Gradients of `finc_coupling(..., direction=-1)` (include/finc.h: finc_coupling_reverse_backward_f32), given grad_y [B,C,H,W]
    and the reverse's OUTPUT `y`: (grad_x, grad_raw, grad_a, grad_b), each computed only if asked for (None otherwise).
    grad_x[:, :C/2] is grad_y[:, :C/2]: what reaches that half through the net is the caller's (autograd's).  tanh and exp(-s) are
    recomputed from `raw`; the per-channel sums run in a fixed order: the same inputs give the same bits."""
    return _coupling_grads("_reverse_backward", grad_y, (), y, raw, a, b, "output", "the reverse's output",
                           (need_gx, need_graw), (need_ga, need_gb))


def finc_coupling_reverse_logdet(x, raw, a, b, out=None):
    """`finc_coupling(x, raw, a, b, -1)` -- the same y, bit for bit -- with, from the same pass, logdet [B] = s summed per image: the
    log-det of the FORWARD map at the recovered input, what `finc_coupling(y, raw, a, b, 1, True)[1]` would report (include/finc.h:
    finc_coupling_reverse_logdet_f32; the reverse map's own log-Jacobian is its negative).  Returns (y, logdet); `out` may be `x`.
    One more small launch for the fixed-order sums: the same inputs give the same bits."""
    _coupling_args(x, raw, a, b)
    return _coupling_transform("_reverse_logdet", x, raw, a, b, (), True, out)


def finc_coupling_reverse_logdet_backward(grad_y, grad_logdet, y, raw, a, b, need_gx=True, need_graw=True, need_ga=True, need_gb=True):
    """Gradients of `finc_coupling_reverse_logdet` (include/finc.h: finc_coupling_reverse_logdet_backward_f32), given grad_y
    [B,C,H,W], grad_logdet [B] or None (zeros) and the reverse's OUTPUT `y`: (grad_x, grad_raw, grad_a, grad_b), each computed only
    if asked for (None otherwise).  With grad_logdet None every result has the bits of `finc_coupling_reverse_backward`."""
    return _coupling_grads("_reverse_logdet_backward", grad_y, (grad_logdet,), y, raw, a, b, "output",
                           "the reverse's output", (need_gx, need_graw), (need_ga, need_gb))


def finc_coupling_backward_reconstruct(grad_y, grad_logdet, y, raw, a, b, need_x=True, need_gx=True, need_graw=True, need_ga=True,
                                       need_gb=True):
    """Gradients of `finc_coupling(..., direction=1, want_logdet=True)` from the forward's OUTPUT `y`, and the forward's input rebuilt
    in the same launch (include/finc.h: finc_coupling_backward_reconstruct_f32): (x, grad_x, grad_raw, grad_a, grad_b), each computed
    only if asked for (None otherwise).  `x` has the bits of `finc_coupling(y, raw, a, b, -1)`; grad_x[:, :C/2] is grad_y[:, :C/2] (the
    net's share is the caller's).  grad_logdet [B] or None (zeros).  Fixed-order sums: the same inputs give the same bits."""
    return _coupling_grads("_backward_reconstruct", grad_y, (grad_logdet,), y, raw, a, b, "output",
                           "the forward's output", (need_x, need_gx, need_graw), (need_ga, need_gb))


def _incoming_grads(like, grad_y, grad_logdet):
    """What a (y, logdet) Function's backward is handed, as the kernels take it: contiguous, zeros for a `y` nobody used (None)."""
    grad_y = torch.zeros_like(like) if grad_y is None else grad_y
    return grad_y.contiguous(), None if grad_logdet is None else grad_logdet.contiguous()


class _FincCouplingFunction(torch.autograd.Function):
    """`finc_coupling` in the forward direction under autograd: (y, logdet) and their backward on the HIP kernels."""

    @staticmethod
    def forward(ctx, x, raw, a, b):
        x, raw, a, b = x.contiguous(), raw.contiguous(), a.contiguous(), b.contiguous()
        y, logdet = finc_coupling(x, raw, a, b, 1, True)
        ctx.save_for_backward(x, raw, a, b)
        return y, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_logdet):
        x, raw, a, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        return finc_coupling_backward(*_incoming_grads(x, grad_y, grad_logdet), x, raw, a, b,
                                      need_gx=need[0], need_graw=need[1], need_ga=need[2], need_gb=need[3])


def coupling_forward(x, raw, a, b):
    """`finc_coupling(x, raw, a, b, +1, want_logdet=True)` under autograd: returns (y, logdet), gradients for `x`, `raw`, `a` and
    `b`, each computed only where needed."""
    return _FincCouplingFunction.apply(x, raw, a, b)


class _FincCouplingReverseFunction(torch.autograd.Function):
    """`finc_coupling` in the reverse direction under autograd (inside `reverse_grad()`): y and its backward on the HIP kernels.  What
    is saved is the OUTPUT y -- the tensor the next layer of a reverse chain keeps as its input anyway -- with raw, a and b."""

    @staticmethod
    def forward(ctx, x, raw, a, b):
        x, raw, a, b = x.contiguous(), raw.contiguous(), a.contiguous(), b.contiguous()
        y = finc_coupling(x, raw, a, b, -1, False)[0]
        ctx.save_for_backward(y, raw, a, b)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        y, raw, a, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        return finc_coupling_reverse_backward(grad_y.contiguous(), y, raw, a, b,
                                              need_gx=need[0], need_graw=need[1], need_ga=need[2], need_gb=need[3])


def coupling_reverse(x, raw, a, b):
    """`finc_coupling(x, raw, a, b, -1)[0]` under autograd: gradients for `x`, `raw`, `a` and `b`, each computed only where needed."""
    return _FincCouplingReverseFunction.apply(x, raw, a, b)


class _FincCouplingReverseLogdetFunction(torch.autograd.Function):
    """`finc_coupling_reverse_logdet` under autograd (inside `reverse_grad()`): (y, logdet) and their backward on the HIP kernels.
    Saved, as by its sibling without the log-det: the OUTPUT y, raw, a and b."""

    @staticmethod
    def forward(ctx, x, raw, a, b):
        x, raw, a, b = x.contiguous(), raw.contiguous(), a.contiguous(), b.contiguous()
        y, logdet = finc_coupling_reverse_logdet(x, raw, a, b)
        ctx.save_for_backward(y, raw, a, b)
        return y, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_logdet):
        y, raw, a, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        return finc_coupling_reverse_logdet_backward(*_incoming_grads(y, grad_y, grad_logdet), y, raw, a, b,
                                                     need_gx=need[0], need_graw=need[1], need_ga=need[2], need_gb=need[3])


def coupling_reverse_logdet(x, raw, a, b):
    """`finc_coupling_reverse_logdet(x, raw, a, b)` under autograd: returns (y, logdet), gradients for `x`, `raw`, `a` and `b`, each
    computed only where needed."""
    return _FincCouplingReverseLogdetFunction.apply(x, raw, a, b)


def finc_split_prior(x, raw, a, b, out=None):
    """`finc_coupling(x, raw, a, b, +1)` with its two output halves as tensors of their own and the second one scored under a standard
    normal, in one launch (include/finc.h: finc_split_prior_f32): (x1, z2, log_p) with x1 = x[:, :C/2], z2 = x2 * exp(s) + t -- the
    bits of the two halves of `finc_coupling`'s y -- and log_p [B] = sum s - 1/2 sum z2^2 - 1/2 (C/2) H W log 2 pi, what
    `glow.SplitPrior.forward` reports as its second value.  `out`: a pair (x1, z2) of contiguous [B,C/2,H,W] tensors to write into;
    they may overlap neither `x` nor each other.  Fixed-order sums: the same inputs give the same bits."""
    _coupling_args(x, raw, a, b, halves=out or ())
    if out is None:
        B, C, H, W = x.shape
        out = tuple(torch.empty(B, C // 2, H, W, dtype=torch.float32, device=x.device) for _ in range(2))
    elif len(out) != 2 or any(t is None for t in out):
        raise ValueError("out must be the pair (x1, z2)")
    return _coupling_transform("", x, raw, a, b, (), True, tuple(out), family="finc_split_prior")


def finc_split_prior_merge(x1, z2, raw, a, b, want_log_p=False, out=None):
    """The inverse of `finc_split_prior`: x = `finc_coupling(cat(x1, z2), raw, a, b, -1)[0]`, bit for bit, without the `cat`
    (include/finc.h: finc_split_prior_merge_f32).  x1, z2 [B,C/2,H,W] fp32 contiguous, raw [B,C,H,W] the net's output on x1.  Returns
    x, or (x, log_p) with `want_log_p`: log_p [B] is what `finc_split_prior` reports at x, from the same pass.  `out` [B,C,H,W] may
    overlap neither half."""
    if x1 is None or z2 is None:
        raise ValueError("finc_split_prior_merge needs both halves")
    _coupling_args(None, raw, a, b, halves=(x1, z2))
    if out is None:
        out = torch.empty(raw.shape, dtype=torch.float32, device=raw.device)
    else:
        _require_device(out, "output")
        if out.shape != raw.shape or out.device != raw.device:
            raise ValueError("output must be [B,C,H,W] like the coupling net's output, on its device")
    x, log_p = _coupling_transform("_merge", (x1, z2), raw, a, b, (), bool(want_log_p), (out,), family="finc_split_prior")
    return (x, log_p) if want_log_p else x


def finc_split_prior_backward(grad_x1, grad_z2, grad_log_p, x, raw, a, b, need_gx=True, need_graw=True, need_ga=True, need_gb=True):
    """Gradients of `finc_split_prior` (include/finc.h: finc_split_prior_backward_f32), given the gradients of its three results --
    grad_x1, grad_z2 [B,C/2,H,W], grad_log_p [B]; each may be None (absent, handed over as NULL), not all three -- and the forward's
    input `x`: (grad_x, grad_raw, grad_a, grad_b), each computed only if asked for (None otherwise).  grad_x[:, :C/2] is grad_x1: what
    reaches that half through the net is the caller's (autograd's).  z2 and exp(s) are recomputed from `raw`."""
    return _coupling_grads("_backward", (grad_x1, grad_z2), (grad_log_p,), x, raw, a, b, "input", "input", (need_gx, need_graw),
                           (need_ga, need_gb), family="finc_split_prior")


class _FincSplitPriorFunction(torch.autograd.Function):
    """`finc_split_prior` under autograd: (x1, z2, log_p) and their backward on the HIP kernel.  A result nobody used arrives as None
    and goes to the kernel as NULL."""

    @staticmethod
    def forward(ctx, x, raw, a, b):
        x, raw, a, b = x.contiguous(), raw.contiguous(), a.contiguous(), b.contiguous()
        x1, z2, log_p = finc_split_prior(x, raw, a, b)
        ctx.save_for_backward(x, raw, a, b)
        ctx.set_materialize_grads(False)
        return x1, z2, log_p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x1, grad_z2, grad_log_p):
        x, raw, a, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = [None if g is None else g.contiguous() for g in (grad_x1, grad_z2, grad_log_p)]
        if all(g is None for g in grads):
            return None, None, None, None
        return finc_split_prior_backward(*grads, x, raw, a, b, need_gx=need[0], need_graw=need[1], need_ga=need[2], need_gb=need[3])


def split_prior_forward(x, raw, a, b):
    """`finc_split_prior(x, raw, a, b)` under autograd: returns (x1, z2, log_p), gradients for `x`, `raw`, `a` and `b`, each computed
    only where needed."""
    return _FincSplitPriorFunction.apply(x, raw, a, b)


def _gauss_split_raw(raw):
    """The Gaussianized split has fp32 kernels only (no `_rawbf16_f32` siblings): a net under autocast hands `raw.float()` over."""
    _require_device(raw, "raw")


def finc_gauss_split(x, raw, a, b, out=None):
    """The Gaussianized split (layers/split.py:24-52; include/finc.h: finc_gauss_split_f32) in one launch: (x1, z2, log_p) with
    x1 = x[:, :C/2], and, for h = a * raw + b per channel, m = h[:, 0::2], logs = h[:, 1::2]: z2 = (x2 - m) * exp(-logs) and
    log_p [B] = -sum logs - 1/2 sum z2^2 - 1/2 (C/2) H W log 2 pi, the split's log-det plus the standard-normal score of z2.
    x, raw [B,C,H,W] fp32 contiguous on the device, raw the 3x3 convolution of x1 WITHOUT its bias; a, b [C].  `out`: a pair
    (x1, z2) of contiguous [B,C/2,H,W] tensors to write into; they may overlap neither `x` nor each other.  Fixed-order sums: the
    same inputs give the same bits."""
    _gauss_split_raw(raw)
    _coupling_args(x, raw, a, b, halves=out or ())
    if out is None:
        B, C, H, W = x.shape
        out = tuple(torch.empty(B, C // 2, H, W, dtype=torch.float32, device=x.device) for _ in range(2))
    elif len(out) != 2 or any(t is None for t in out):
        raise ValueError("out must be the pair (x1, z2)")
    return _coupling_transform("", x, raw, a, b, (), True, tuple(out), family="finc_gauss_split")


def finc_gauss_split_merge(x1, z2, raw, a, b, want_log_p=False, out=None):
    """The inverse of `finc_gauss_split` (include/finc.h: finc_gauss_split_merge_f32): x[:, :C/2] = x1, x[:, C/2:] = z2 * exp(logs)
    + m, written whole by one launch, without a `cat`.  x1, z2 [B,C/2,H,W] fp32 contiguous, raw [B,C,H,W] the convolution's output on
    x1.  Returns x, or (x, log_p) with `want_log_p`: log_p [B] is what `finc_gauss_split` reports at x, from the same pass.  `out`
    [B,C,H,W] may overlap neither half."""
    if x1 is None or z2 is None:
        raise ValueError("finc_gauss_split_merge needs both halves")
    _gauss_split_raw(raw)
    _coupling_args(None, raw, a, b, halves=(x1, z2))
    if out is None:
        out = torch.empty(raw.shape, dtype=torch.float32, device=raw.device)
    else:
        _require_device(out, "output")
        if out.shape != raw.shape or out.device != raw.device:
            raise ValueError("output must be [B,C,H,W] like the convolution's output, on its device")
    x, log_p = _coupling_transform("_merge", (x1, z2), raw, a, b, (), bool(want_log_p), (out,), family="finc_gauss_split")
    return (x, log_p) if want_log_p else x


def finc_gauss_split_backward(grad_x1, grad_z2, grad_log_p, x, raw, a, b, need_gx=True, need_graw=True, need_ga=True, need_gb=True):
    """Gradients of `finc_gauss_split` (include/finc.h: finc_gauss_split_backward_f32), given the gradients of its three results --
    grad_x1, grad_z2 [B,C/2,H,W], grad_log_p [B]; each may be None (absent, handed over as NULL), not all three -- and the forward's
    input `x`: (grad_x, grad_raw, grad_a, grad_b), each computed only if asked for (None otherwise).  grad_x[:, :C/2] is grad_x1: what
    reaches that half through the convolution is the caller's (autograd's).  z2 and exp(-logs) are recomputed from `raw`."""
    _gauss_split_raw(raw)
    return _coupling_grads("_backward", (grad_x1, grad_z2), (grad_log_p,), x, raw, a, b, "input", "input", (need_gx, need_graw),
                           (need_ga, need_gb), family="finc_gauss_split")


class _FincGaussSplitFunction(torch.autograd.Function):
    """`finc_gauss_split` under autograd: (x1, z2, log_p) and their backward on the HIP kernel.  A result nobody used arrives as None
    and goes to the kernel as NULL."""

    @staticmethod
    def forward(ctx, x, raw, a, b):
        x, raw, a, b = x.contiguous(), raw.contiguous(), a.contiguous(), b.contiguous()
        x1, z2, log_p = finc_gauss_split(x, raw, a, b)
        ctx.save_for_backward(x, raw, a, b)
        ctx.set_materialize_grads(False)
        return x1, z2, log_p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x1, grad_z2, grad_log_p):
        x, raw, a, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = [None if g is None else g.contiguous() for g in (grad_x1, grad_z2, grad_log_p)]
        if all(g is None for g in grads):
            return None, None, None, None
        return finc_gauss_split_backward(*grads, x, raw, a, b, need_gx=need[0], need_graw=need[1], need_ga=need[2], need_gb=need[3])


def gauss_split_forward(x, raw, a, b):
    """`finc_gauss_split(x, raw, a, b)` under autograd: returns (x1, z2, log_p), gradients for `x`, `raw`, `a` and `b`, each computed
    only where needed."""
    return _FincGaussSplitFunction.apply(x, raw, a, b)


def _merge_backward(family, grad_x, grad_log_p, x, raw, a, b, needs):
    if grad_x is None and grad_log_p is None:
        raise ValueError(f"{family}_merge_backward needs grad_x or grad_log_p")
    return _coupling_grads("_merge_backward", grad_x, (grad_log_p,), x, raw, a, b, "output", "the merge's output", needs[:3], needs[3:],
                           family=family, half_outs=True)


def finc_split_prior_merge_backward(grad_x, grad_log_p, x, raw, a, b, need_gx1=True, need_gz2=True, need_graw=True, need_ga=True,
                                    need_gb=True):
    """Gradients of `finc_split_prior_merge(..., want_log_p=True)` (include/finc.h: finc_split_prior_merge_backward_f32), given
    grad_x [B,C,H,W] and grad_log_p [B] -- either may be None (absent, handed over as NULL), not both -- and the merge's OUTPUT `x`:
    (grad_x1, grad_z2, grad_raw, grad_a, grad_b), each computed only if asked for (None otherwise).  grad_x1, grad_z2 [B,C/2,H,W];
    grad_x1 is grad_x[:, :C/2]: what reaches x1 through the net is the caller's (autograd's).  z2, tanh and exp(-s) are recomputed
    from `raw`; a bfloat16 `raw` gives a bfloat16 grad_raw.  With grad_log_p None, grad_z2, grad_raw, grad_a and grad_b have the bits
    of `finc_coupling_reverse_backward` on the same arguments.  Fixed-order sums: the same inputs give the same bits."""
    return _merge_backward("finc_split_prior", grad_x, grad_log_p, x, raw, a, b, (need_gx1, need_gz2, need_graw, need_ga, need_gb))


def finc_gauss_split_merge_backward(grad_x, grad_log_p, x, raw, a, b, need_gx1=True, need_gz2=True, need_graw=True, need_ga=True,
                                    need_gb=True):
    """Gradients of `finc_gauss_split_merge(..., want_log_p=True)` (include/finc.h: finc_gauss_split_merge_backward_f32), given
    grad_x [B,C,H,W] and grad_log_p [B] -- either may be None (absent, handed over as NULL), not both -- and the merge's OUTPUT `x`:
    (grad_x1, grad_z2, grad_raw, grad_a, grad_b), each computed only if asked for (None otherwise).  grad_x1 is grad_x[:, :C/2]: what
    reaches x1 through the convolution is the caller's (autograd's).  z2 and exp(logs) are recomputed from `raw` (fp32 only)."""
    _gauss_split_raw(raw)
    return _merge_backward("finc_gauss_split", grad_x, grad_log_p, x, raw, a, b, (need_gx1, need_gz2, need_graw, need_ga, need_gb))


def _merge_record(ctx, merge, x1, z2, raw, a, b, want_log_p):
    """The forward of a merge's Function.  Saved: the OUTPUT x -- the tensor the next layer of a reverse chain keeps anyway -- with
    raw, a and b."""
    x1, z2, raw, a, b = x1.contiguous(), z2.contiguous(), raw.contiguous(), a.contiguous(), b.contiguous()
    out = merge(x1, z2, raw, a, b, want_log_p=want_log_p)
    ctx.save_for_backward(out[0] if want_log_p else out, raw, a, b)
    ctx.set_materialize_grads(False)
    return out


def _merge_differentiate(ctx, merge_backward, grad_x, grad_log_p):
    """The backward of a merge's Function: ONE launch, only what `needs_input_grad` asks for.  A result nobody used arrives as None
    and goes to the kernel as NULL."""
    x, raw, a, b = ctx.saved_tensors
    need = ctx.needs_input_grad
    grads = [None if g is None else g.contiguous() for g in (grad_x, grad_log_p)]
    if all(g is None for g in grads):
        return (None,) * 6
    return merge_backward(*grads, x, raw, a, b, need_gx1=need[0], need_gz2=need[1], need_graw=need[2], need_ga=need[3],
                          need_gb=need[4]) + (None,)


class _FincSplitPriorMergeFunction(torch.autograd.Function):
    """`finc_split_prior_merge` under autograd (inside `reverse_grad()`): x, or (x, log_p), and their backward on the HIP kernel
    (finc_split_prior_merge_backward_f32 / _rawbf16_f32)."""

    @staticmethod
    def forward(ctx, x1, z2, raw, a, b, want_log_p):
        return _merge_record(ctx, finc_split_prior_merge, x1, z2, raw, a, b, want_log_p)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x, grad_log_p=None):
        return _merge_differentiate(ctx, finc_split_prior_merge_backward, grad_x, grad_log_p)


class _FincGaussSplitMergeFunction(torch.autograd.Function):
    """`finc_gauss_split_merge` under autograd (inside `reverse_grad()`): x, or (x, log_p), and their backward on the HIP kernel
    (finc_gauss_split_merge_backward_f32)."""

    @staticmethod
    def forward(ctx, x1, z2, raw, a, b, want_log_p):
        return _merge_record(ctx, finc_gauss_split_merge, x1, z2, raw, a, b, want_log_p)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x, grad_log_p=None):
        return _merge_differentiate(ctx, finc_gauss_split_merge_backward, grad_x, grad_log_p)


def split_prior_merge(x1, z2, raw, a, b, want_log_p=False):
    """`finc_split_prior_merge(x1, z2, raw, a, b, want_log_p)` under autograd: x, or (x, log_p), with gradients for `x1` (the direct
    share), `z2`, `raw`, `a` and `b`, each computed only where needed, from ONE backward launch."""
    return _FincSplitPriorMergeFunction.apply(x1, z2, raw, a, b, bool(want_log_p))


def gauss_split_merge(x1, z2, raw, a, b, want_log_p=False):
    """`finc_gauss_split_merge(x1, z2, raw, a, b, want_log_p)` under autograd: x, or (x, log_p), with gradients for `x1` (the direct
    share), `z2`, `raw`, `a` and `b`, each computed only where needed, from ONE backward launch."""
    return _FincGaussSplitMergeFunction.apply(x1, z2, raw, a, b, bool(want_log_p))


def finc_bias_relu(x, bias, out=None):
    """max(x + bias[c], 0) in one pass: the bias and the ReLU behind a convolution of the coupling net (layers/coupling.py:58-63).
    x [B,C,H,W] fp32 contiguous on the device, bias [C]; `out` may be `x`.  Inference only: no autograd graph is recorded.
    `x` may also be bfloat16 (the output of a convolution under bf16 autocast; finc_bias_relu_bf16): `out` is bfloat16 then, the bias
    stays fp32, the add and the max run in fp32 and are rounded once."""
    bf16 = x.dtype == torch.bfloat16
    _require_device(x, "input", x.dtype if bf16 else torch.float32)
    _require_device(bias, "bias")
    if x.dim() != 4 or bias.numel() != x.shape[1] or bias.device != x.device:
        raise ValueError("expected activations [B,C,H,W] and one bias entry per channel on the same device")
    out = _out_like(x, out, x.dtype)
    if x.numel() == 0:
        return out
    B, C, H, W = x.shape
    _call("finc_bias_relu_bf16" if bf16 else "finc_bias_relu_f32", x.device, x.data_ptr(), bias.data_ptr(), out.data_ptr(), B, C, H * W, _stream_ptr(x))
    return out


def _image_sides(t, squeeze, squeezed_side):
    """((B, C, H, W) of the image, the other side's shape) from a tensor of either side of the image boundary."""
    if t.dim() != 4:
        raise ValueError("expected a tensor [B,C,H,W]")
    B, C, H, W = t.shape
    if not squeeze:
        return (B, C, H, W), (B, C, H, W)
    if squeezed_side:
        if C % 4:
            raise ValueError("a squeezed tensor has 4 channels per image channel")
        return (B, C // 4, 2 * H, 2 * W), (B, C, H, W)
    if H % 2 or W % 2:
        raise ValueError("squeeze needs an even height and width")
    return (B, C, H, W), (B, 4 * C, H // 2, W // 2)


def _image_out(t, shape, out, dtype):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=t.device)
    return _out_like(t.new_empty((), dtype=dtype).expand(shape), out, dtype)


def _image_call(name, t, ptrs, dims, flag, consts, logdet, needs_ws):
    nbytes = _lib.lib().finc_image_workspace_bytes(*dims, flag) if needs_ws else None
    _call(name, t.device, *ptrs, _ptr(logdet), *dims, flag, *(float(v) for v in consts), *_ws_args(t.device, nbytes), _stream_ptr(t))


def finc_image_encode(img, noise=None, *, mult, lo, hi, hi_comp, logdet_const, squeeze=True, out=None):
    """The image boundary in one HIP launch (include/finc.h: finc_image_encode_u8_f32 / finc_image_encode_f32): what Dequantization,
    the Normalization layers, LogitTransform and the first Squeeze compute.  img [B,C,H,W] uint8 or fp32 (whole numbers), contiguous on
    the device; noise fp32 of the same shape or None (zero).  Per element y = mult * (img + noise) + lo and 1 - y = mult * ((hi - img) -
    noise) + hi_comp -- the caller composes the four numbers in double precision, hi_comp = 1 - lo - mult * hi -- and the result is
    log y - log(1 - y), [B,4C,H/2,W/2] in the reference's squeeze order (`squeeze`) or [B,C,H,W].  Returns (y, logdet): logdet [B] =
    logdet_const - sum(log y + log(1 - y)) per image, fixed-order sums.  `out` may be `img` for fp32 pixels without squeeze."""
    u8 = img.dtype == torch.uint8
    _require_device(img, "image", torch.uint8 if u8 else torch.float32)
    dims, shape = _image_sides(img, squeeze, False)
    if noise is not None:
        _require_device(noise, "noise")
        if noise.shape != img.shape or noise.device != img.device:
            raise ValueError("noise must match the image in shape and device")
    out = _image_out(img, shape, out, torch.float32)
    logdet = torch.empty(dims[0], dtype=torch.float32, device=img.device)
    if _nothing_to_launch(img, (out,), (logdet,)):
        return out, logdet
    _image_call("finc_image_encode_u8_f32" if u8 else "finc_image_encode_f32", img, (img.data_ptr(), _ptr(noise), out.data_ptr()), dims,
                int(bool(squeeze)), (mult, lo, hi, hi_comp, logdet_const), logdet, True)
    return out, logdet


def finc_image_decode(z, *, inv_mult, off, hi, logdet_const=None, unsqueeze=True, dtype=torch.float32, out=None):
    """The inverse of `finc_image_encode` up to the floor, in one HIP launch (finc_image_decode_f32 / finc_image_decode_u8): z fp32
    [B,4C,h,w] (`unsqueeze`: the image is [B,C,2h,2w]) or [B,C,H,W]; v = sigmoid(z) * inv_mult + off.  `dtype` torch.float32: floor(v),
    not clamped (what Dequantization.reverse returns); torch.uint8: floor(v) clamped to [0, hi - 1].  With `logdet_const`: (x, logdet),
    logdet [B] = logdet_const + sum(|z| + 2 log(1 + exp(-|z|))) per image -- the log-det `finc_image_encode` reports at the value in
    front of the floor; without: x alone.  `out`: a contiguous image-shaped tensor of `dtype` to write into; an fp32 one may be `z`
    without `unsqueeze`."""
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError("finc_image_decode writes float32 or uint8")
    _require_device(z, "input")
    dims, _ = _image_sides(z, unsqueeze, True)
    out = _image_out(z, dims, out, dtype)
    want = logdet_const is not None
    logdet = torch.empty(dims[0], dtype=torch.float32, device=z.device) if want else None
    if not _nothing_to_launch(z, (out,), (logdet,)):
        _image_call("finc_image_decode_u8" if dtype == torch.uint8 else "finc_image_decode_f32", z, (z.data_ptr(), out.data_ptr()), dims,
                    int(bool(unsqueeze)), (inv_mult, off, hi, logdet_const if want else 0.0), logdet, want)
    return (out, logdet) if want else out


def actnorm_supported():
    """ActNorm's kernels take any channel count, and a library without them does not load (fincflow_amd._lib: ACTNORM_ABI_VERSION):
    True once the library is loaded, no call into it per layer and pass."""
    _lib.lib()
    return True


def _actnorm_args(x, log_scale, translation, what="input"):
    _require_device(x, what)
    _require_device(log_scale, "log_scale")
    if x.dim() != 4:
        raise ValueError(f"expected {what} [B,C,H,W]")
    _per_channel(x, "log_scale", log_scale)
    if translation is not None:
        _require_device(translation, "translation")
        _per_channel(x, "translation", translation)


def finc_actnorm(x, log_scale, translation, direction=1, want_logdet=False, out=None):
    """ActNorm (layers/actnorm.py:34, :51) as one streaming HIP launch: y = (x - translation) * exp(-log_scale) per channel
    (direction +1) or y = x * exp(log_scale) + translation (-1).  x [B,C,H,W] fp32 contiguous on the device; log_scale, translation
    [C].  Returns (y, logdet): logdet [B] = -sum(log_scale) * H * W when `want_logdet` (forward direction; written by the same
    launch), else None.  `out` may be `x`.  Nothing is recorded for autograd (`actnorm_forward` does that)."""
    _actnorm_args(x, log_scale, translation)
    if direction not in (1, -1):
        raise ValueError("direction must be +1 (forward) or -1 (reverse)")
    out = _out_like(x, out)
    B, C, H, W = x.shape
    want_logdet = bool(want_logdet) and direction == 1
    if x.numel() == 0:
        return out, (torch.zeros(B, dtype=torch.float32, device=x.device) if want_logdet else None)
    logdet = torch.empty(B, dtype=torch.float32, device=x.device) if want_logdet else None
    _call("finc_actnorm_f32", x.device, x.data_ptr(), log_scale.data_ptr(), translation.data_ptr(), out.data_ptr(), _ptr(logdet), B, C,
          H * W, direction, _stream_ptr(x))
    return out, logdet


def _actnorm_grads(entry, grad_y, grad_logdet, v, log_scale, translation, what, whose, need_acts, need_sums):
    """One backward entry point of ActNorm behind its wrapper: the checks, the outputs asked for -- `need_acts`: (x,) grad_x;
    `need_sums`: grad_log_scale, grad_translation -- the workspace and the call.  `v`: the activation that entry point reads,
    "input" or "output" (`what`) of `whose` pass; grad_logdet, translation: tuples, empty for an entry point that takes none."""
    _actnorm_args(v, log_scale, translation[0] if translation else None, what)
    _require_device(grad_y, "grad_output")
    if grad_y.shape != v.shape or grad_y.device != v.device:
        raise ValueError(f"grad_output must match {whose} in shape and device")
    B, C, H, W = v.shape
    for g in grad_logdet:
        _per_image(g, "grad_logdet", v)
    sums = tuple(torch.empty(C, dtype=torch.float32, device=v.device) if n else None for n in need_sums)
    outs = tuple(torch.empty_like(v) if n else None for n in need_acts) + sums
    if _nothing_to_launch(v, outs, sums):
        return outs
    nbytes = _lib.lib().finc_actnorm_workspace_bytes(B, C, H * W) if any(need_sums) else None
    _call(entry, v.device, grad_y.data_ptr(), *map(_ptr, grad_logdet), v.data_ptr(), log_scale.data_ptr(),
          *(t.data_ptr() for t in translation), *map(_ptr, outs), B, C, H * W, *_ws_args(v.device, nbytes), _stream_ptr(v))
    return outs


def finc_actnorm_backward(grad_y, grad_logdet, y, log_scale, need_gx=True, need_gls=True, need_gt=True):
    """Gradients of `finc_actnorm(..., direction=1, want_logdet=True)` (include/finc.h: finc_actnorm_backward_f32), given grad_y
    [B,C,H,W], grad_logdet [B] or None (zeros), the forward's OUTPUT `y` and log_scale: (grad_x, grad_log_scale, grad_translation),
    each computed only if asked for (None otherwise).  The per-channel sums run in a fixed order: the same inputs give the same bits."""
    return _actnorm_grads("finc_actnorm_backward_f32", grad_y, (grad_logdet,), y, log_scale, (), "output", "the forward's output",
                          (need_gx,), (need_gls, need_gt))


def finc_actnorm_backward_reconstruct(grad_y, grad_logdet, y, log_scale, translation, need_x=True, need_gx=True, need_gls=True,
                                      need_gt=True):
    """`finc_actnorm_backward` that rebuilds the forward's input from the same read of `y` (include/finc.h:
    finc_actnorm_backward_reconstruct_f32): (x, grad_x, grad_log_scale, grad_translation), each computed only if asked for (None
    otherwise).  `x` has the bits of `finc_actnorm(y, log_scale, translation, -1)`.  One launch (plus the small fixed-order reduce
    with a per-channel gradient): the same inputs give the same bits."""
    return _actnorm_grads("finc_actnorm_backward_reconstruct_f32", grad_y, (grad_logdet,), y, log_scale, (translation,), "output",
                          "the forward's output", (need_x, need_gx), (need_gls, need_gt))


def finc_actnorm_reverse_backward(grad_y, x, log_scale, need_gx=True, need_gls=True, need_gt=True):
    """Gradients of `finc_actnorm(..., direction=-1)` (include/finc.h: finc_actnorm_reverse_backward_f32), given grad_y [B,C,H,W],
    the reverse's INPUT `x` and log_scale: (grad_x, grad_log_scale, grad_translation), each computed only if asked for (None
    otherwise).  The per-channel sums run in a fixed order: the same inputs give the same bits."""
    return _actnorm_grads("finc_actnorm_reverse_backward_f32", grad_y, (), x, log_scale, (), "input", "the reverse's input",
                          (need_gx,), (need_gls, need_gt))


def finc_actnorm_init(x, log_scale, translation):
    """ActNorm's data-dependent initialisation (layers/actnorm.py:17-23) on the device, written IN PLACE into the two parameters:
    translation = per-channel mean of x, log_scale = log(unbiased std + 1e-8).  x [B,C,H,W] fp32 contiguous with B * H * W >= 2.
    No host round trip, capturable; fixed-order merges: the same input gives the same bits."""
    _actnorm_args(x, log_scale, translation)
    B, C, H, W = x.shape
    if B * H * W < 2:
        raise ValueError("the unbiased standard deviation needs at least two values per channel")
    _call("finc_actnorm_init_f32", x.device, x.data_ptr(), log_scale.data_ptr(), translation.data_ptr(), B, C, H * W,
          *_ws_args(x.device, _lib.lib().finc_actnorm_workspace_bytes(B, C, H * W)), _stream_ptr(x))
    # the kernel wrote behind PyTorch's back: the caches keyed on (address, version) of the parameters (FlowSequential's folds) must see it
    torch.autograd.graph.increment_version(log_scale)
    torch.autograd.graph.increment_version(translation)
    return log_scale, translation


class _FincActNormFunction(torch.autograd.Function):
    """`finc_actnorm` in the forward direction under autograd: (y, logdet) and their backward on the HIP kernels.  What is saved is
    the OUTPUT y -- the tensor the next layer keeps as its input anyway -- and log_scale; the input is not kept."""

    @staticmethod
    def forward(ctx, x, log_scale, translation):
        x, log_scale, translation = x.contiguous(), log_scale.contiguous(), translation.contiguous()
        y, logdet = finc_actnorm(x, log_scale, translation, 1, True)
        ctx.save_for_backward(y, log_scale)
        return y, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_logdet):
        y, log_scale = ctx.saved_tensors
        need = ctx.needs_input_grad
        return finc_actnorm_backward(*_incoming_grads(y, grad_y, grad_logdet), y, log_scale,
                                     need_gx=need[0], need_gls=need[1], need_gt=need[2])


def actnorm_forward(x, log_scale, translation):
    """`finc_actnorm(x, log_scale, translation, +1, want_logdet=True)` under autograd: returns (y, logdet), gradients for `x`,
    `log_scale` and `translation`, each computed only where needed."""
    return _FincActNormFunction.apply(x, log_scale, translation)


class _FincActNormReverseFunction(torch.autograd.Function):
    """`finc_actnorm` in the reverse direction under autograd (inside `reverse_grad()`): y and its backward on the HIP kernels.  What
    is saved is the INPUT x and log_scale: grad_log_scale from the output would be a sum over grad_y * (y - translation), which
    cancels on a channel whose translation dwarfs its spread."""

    @staticmethod
    def forward(ctx, x, log_scale, translation):
        x, log_scale, translation = x.contiguous(), log_scale.contiguous(), translation.contiguous()
        y = finc_actnorm(x, log_scale, translation, -1)[0]
        ctx.save_for_backward(x, log_scale)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, log_scale = ctx.saved_tensors
        need = ctx.needs_input_grad
        return finc_actnorm_reverse_backward(grad_y.contiguous(), x, log_scale, need_gx=need[0], need_gls=need[1], need_gt=need[2])


def actnorm_reverse(x, log_scale, translation):
    """`finc_actnorm(x, log_scale, translation, -1)[0]` under autograd: gradients for `x`, `log_scale` and `translation`, each
    computed only where needed."""
    return _FincActNormReverseFunction.apply(x, log_scale, translation)


def spline_supported(K):
    """Bin counts the spline kernels take (include/finc.h: finc_spline_supported_f32): 2 .. 16."""
    return bool(_lib.lib().finc_spline_supported_f32(int(K)))


def _spline_args(x, table, what="input"):
    """The checks of every spline wrapper; returns (B, C, HW, K, P) as the entry points take them."""
    _require_device(x, what)
    _require_device(table, "table")
    if x.dim() != 4:
        raise ValueError(f"expected {what} [B,C,H,W]")
    if table.dim() != 2 or table.shape[0] % 3 or table.device != x.device:
        raise ValueError("table must be [3 * (K + 1), P] (cumwidths, cumheights, derivatives; knot-major) on the activations' device")
    B, C, H, W = x.shape
    K, P = table.shape[0] // 3 - 1, table.shape[1]
    if not spline_supported(K) or P not in (1, C * H * W):
        raise ValueError(f"no spline kernel for K = {K} bins with P = {P} table rows on {C} x {H} x {W} positions (2 <= K <= 16; P = 1 or C*H*W)")
    return B, C, H * W, K, P


def finc_spline(x, table, tail_bound, direction=1, want_logdet=False, out=None):
    """The rational-quadratic spline with linear tails (layers/splines/rational_quadratic.py) as one streaming HIP launch, from its
    knot table [3 * (K + 1), P] (include/finc.h: finc_spline_f32): direction +1 the map, -1 its inverse.  Returns (y, logdet): logdet
    [B], when `want_logdet`, is the FORWARD map's log-det in either direction (in direction -1 at the recovered input), summed in a
    fixed order by a second small launch.  `out` may be `x`.  Nothing is recorded for autograd."""
    B, C, HW, K, P = _spline_args(x, table)
    if direction not in (1, -1):
        raise ValueError("direction must be +1 (forward) or -1 (reverse)")
    out = _out_like(x, out)
    want_logdet = bool(want_logdet)
    if x.numel() == 0:
        return out, (torch.zeros(B, dtype=torch.float32, device=x.device) if want_logdet else None)
    logdet = torch.empty(B, dtype=torch.float32, device=x.device) if want_logdet else None
    nbytes = _lib.lib().finc_spline_workspace_bytes(B, C, HW, K, P) if want_logdet else None
    _call("finc_spline_f32", x.device, x.data_ptr(), table.data_ptr(), P, K, float(tail_bound), direction, out.data_ptr(), _ptr(logdet),
          B, C, HW, *_ws_args(x.device, nbytes), _stream_ptr(x))
    return out, logdet


def _spline_grads(entry, grad_y, grad_logdet, x, table, tail_bound, what, whose, need_gx, need_gt):
    """One backward entry point of the spline behind its wrapper: the checks, the outputs asked for, the workspace and the call.
    grad_y or grad_logdet may be None (zeros), not both."""
    B, C, HW, K, P = _spline_args(x, table, what)
    if grad_y is None and grad_logdet is None:
        raise ValueError("grad_output and grad_logdet are both absent")
    if grad_y is not None:
        _require_device(grad_y, "grad_output")
        if grad_y.shape != x.shape or grad_y.device != x.device:
            raise ValueError(f"grad_output must match {whose} in shape and device")
    _per_image(grad_logdet, "grad_logdet", x)
    gt = torch.empty_like(table) if need_gt else None
    outs = (torch.empty_like(x) if need_gx else None, gt)
    if _nothing_to_launch(x, outs, (gt,)):
        return outs
    nbytes = _lib.lib().finc_spline_workspace_bytes(B, C, HW, K, P) if need_gt else None
    _call(entry, x.device, _ptr(grad_y), _ptr(grad_logdet), x.data_ptr(), table.data_ptr(), P, K, float(tail_bound), *map(_ptr, outs),
          B, C, HW, *_ws_args(x.device, nbytes), _stream_ptr(x))
    return outs


def finc_spline_backward(grad_y, grad_logdet, x, table, tail_bound, need_gx=True, need_gt=True):
    """Gradients of `finc_spline(..., direction=1, want_logdet=True)` (include/finc.h: finc_spline_backward_f32) from the forward's
    INPUT `x`: (grad_x, grad_table), each computed only if asked for (None otherwise).  grad_table is the gradient of the knot table
    as laid out; the chain to the unnormalised parameters is PyTorch's.  Fixed-order sums: the same inputs give the same bits."""
    return _spline_grads("finc_spline_backward_f32", grad_y, grad_logdet, x, table, tail_bound, "input", "the forward's input", need_gx,
                         need_gt)


def finc_spline_reverse_backward(grad_x, grad_logdet, y, table, tail_bound, need_gx=True, need_gt=True):
    """Gradients of `finc_spline(y, ..., direction=-1)` (include/finc.h: finc_spline_reverse_backward_f32) from the reverse's INPUT `y`
    (the position in the bin is the quadratic's root again: taken from the stored output it cancels in a narrow bin), grad_x the
    gradient of its output, grad_logdet that of the log-det it returned (None: it returned none): (grad_y, grad_table), as above."""
    return _spline_grads("finc_spline_reverse_backward_f32", grad_x, grad_logdet, y, table, tail_bound, "input", "the reverse's input",
                         need_gx, need_gt)


class _FincSplineFunction(torch.autograd.Function):
    """`finc_spline` in the forward direction under autograd: (y, logdet) and their backward on the HIP kernels, from the saved input."""

    @staticmethod
    def forward(ctx, x, table, tail_bound):
        x, table = x.contiguous(), table.contiguous()
        y, logdet = finc_spline(x, table, tail_bound, 1, True)
        ctx.save_for_backward(x, table)
        ctx.tail_bound = tail_bound
        return y, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_logdet):
        x, table = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (*finc_spline_backward(*_incoming_grads(x, grad_y, grad_logdet), x, table, ctx.tail_bound, need_gx=need[0], need_gt=need[1]),
                None)


class _FincSplineReverseFunction(torch.autograd.Function):
    """`finc_spline` in the reverse direction under autograd (inside `reverse_grad()`), saved: its INPUT."""

    @staticmethod
    def forward(ctx, y, table, tail_bound):
        y, table = y.contiguous(), table.contiguous()
        x = finc_spline(y, table, tail_bound, -1)[0]
        ctx.save_for_backward(y, table)
        ctx.tail_bound = tail_bound
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x):
        y, table = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (*finc_spline_reverse_backward(grad_x.contiguous(), None, y, table, ctx.tail_bound, need_gx=need[0], need_gt=need[1]), None)


class _FincSplineReverseLogdetFunction(torch.autograd.Function):
    """The reverse with the forward log-det at its result, one pass; saved: its input y."""

    @staticmethod
    def forward(ctx, y, table, tail_bound):
        y, table = y.contiguous(), table.contiguous()
        x, logdet = finc_spline(y, table, tail_bound, -1, True)
        ctx.save_for_backward(y, table)
        ctx.tail_bound = tail_bound
        return x, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x, grad_logdet):
        y, table = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (*finc_spline_reverse_backward(*_incoming_grads(y, grad_x, grad_logdet), y, table, ctx.tail_bound, need_gx=need[0],
                                              need_gt=need[1]), None)


def spline_forward(x, table, tail_bound):
    """`finc_spline(x, table, tail_bound, +1, want_logdet=True)` under autograd: (y, logdet), gradients for `x` and `table`."""
    return _FincSplineFunction.apply(x, table, tail_bound)


def spline_reverse(y, table, tail_bound):
    """`finc_spline(y, table, tail_bound, -1)[0]` under autograd: gradients for `y` and `table`."""
    return _FincSplineReverseFunction.apply(y, table, tail_bound)


def spline_reverse_logdet(y, table, tail_bound):
    """`finc_spline(y, table, tail_bound, -1, want_logdet=True)` under autograd: (x, forward log-det at x)."""
    return _FincSplineReverseLogdetFunction.apply(y, table, tail_bound)


#: include/finc.h FincActivationKind
ACTIVATION_KINDS = {"smooth_leaky_relu": 0, "leaky_relu": 1, "learnable_leaky_relu": 2, "smooth_tanh": 3}
#: include/finc.h finc_activation_backward_f32's `mode`
ACTIVATION_MODES = {"forward": 0, "reverse": 1, "rebuild": 2}


def activation_supported(kind):
    """Does the library have the kernels of this kind (a name of ACTIVATION_KINDS)?"""
    return kind in ACTIVATION_KINDS and bool(_lib.lib().finc_activation_supported_f32(ACTIVATION_KINDS[kind]))


def activation_inverse_trips(kind):
    """The fixed trip count of the kind's inverse on the device (0: the leaky kinds' select and division)."""
    return int(_lib.lib().finc_debug_activation_trips(ACTIVATION_KINDS[kind]))


def _activation_args(x, kind, p0, p1, slope, what="input"):
    """The checks of every activation wrapper; returns (kind code, p0, p1, slope pointer, B, C, HW) as the entry points take them: a
    tensor of two or more dimensions is [B, C, everything else], which the kernels walk as [B, C * HW]."""
    _require_device(x, what)
    if x.dim() < 2:
        raise ValueError(f"expected {what} with a batch dimension and at least one more")
    if kind not in ACTIVATION_KINDS:
        raise ValueError(f"unknown activation kind {kind!r} (one of {sorted(ACTIVATION_KINDS)})")
    if kind == "learnable_leaky_relu":
        if slope is None:
            raise ValueError("the learnable kind reads its slope from a device tensor of one element")
        _require_device(slope, "slope")
        if slope.numel() != 1 or slope.device != x.device:
            raise ValueError("slope must hold one element, on the activations' device")
    else:
        if slope is not None:
            raise ValueError(f"{kind} takes its parameters as numbers, not a slope tensor")
        bad = [p for p in ((p0, p1) if kind == "smooth_tanh" else (p0,)) if not (0.0 < float(p) < math.inf)]
        if bad:
            raise ValueError(f"{kind}: parameters must be positive and finite, got {bad}")
    hw = 1
    for d in x.shape[2:]:
        hw *= d
    return ACTIVATION_KINDS[kind], float(p0), float(p1), _ptr(slope), x.shape[0], x.shape[1], hw


def finc_activation(x, kind, p0=0.0, p1=0.0, slope=None, direction=1, want_logdet=False, out=None):
    """One of the smooth invertible activations (layers/activations.py SmoothLeakyRelu, LeakyRelu, LearnableLeakyRelu, SmoothTanh) as one
    streaming HIP launch (include/finc.h: finc_activation_f32): direction +1 the map, -1 its inverse -- for the two smooth kinds a
    bracketed Newton iteration with a fixed trip count, in registers.  `kind`: a name of ACTIVATION_KINDS; `p0`, `p1`: its parameters
    (alpha; alpha, beta); `slope`: the learnable kind's slope as a device tensor of one element (no host synchronisation).  Returns
    (y, logdet): logdet [B], when `want_logdet`, is the FORWARD map's log-det in either direction (in direction -1 at the recovered
    input), summed in a fixed order by a second small launch.  `out` may be `x`.  Nothing is recorded for autograd."""
    code, p0, p1, sp, B, C, HW = _activation_args(x, kind, p0, p1, slope)
    if direction not in (1, -1):
        raise ValueError("direction must be +1 (forward) or -1 (reverse)")
    out = _out_like(x, out)
    want_logdet = bool(want_logdet)
    if x.numel() == 0:
        return out, (torch.zeros(B, dtype=torch.float32, device=x.device) if want_logdet else None)
    logdet = torch.empty(B, dtype=torch.float32, device=x.device) if want_logdet else None
    nbytes = _lib.lib().finc_activation_workspace_bytes(B, C, HW) if want_logdet else None
    _call("finc_activation_f32", x.device, code, p0, p1, sp, direction, x.data_ptr(), out.data_ptr(), _ptr(logdet), B, C, HW,
          *_ws_args(x.device, nbytes), _stream_ptr(x))
    return out, logdet


def finc_activation_backward(grad_y, grad_logdet, v, kind, p0=0.0, p1=0.0, slope=None, mode="forward", need_x=False, need_gx=True,
                             need_gs=False, out=None):
    """Every backward of the activations (include/finc.h: finc_activation_backward_f32), by `mode`: "forward" from the forward's INPUT,
    "reverse" of direction -1 from its OUTPUT (grad_y: the gradient that reaches that output), "rebuild" from the forward's OUTPUT,
    which also returns the rebuilt input (`need_x`) with the bits direction -1 gives.  Returns (x, grad_input, grad_slope), each
    computed only if asked for (None otherwise); grad_slope [1] belongs to the learnable kind.  grad_y or grad_logdet may be None
    (zeros), not both.  `out`: where grad_input goes (it may be `grad_y`).  Fixed-order sums: the same inputs give the same bits."""
    code, p0, p1, sp, B, C, HW = _activation_args(v, kind, p0, p1, slope, "activation")
    if mode not in ACTIVATION_MODES:
        raise ValueError(f"mode must be one of {sorted(ACTIVATION_MODES)}")
    if need_x and mode != "rebuild":
        raise ValueError("only the rebuild mode returns the input")
    if need_gs and kind != "learnable_leaky_relu":
        raise ValueError("only the learnable kind has a slope gradient")
    if grad_y is None and grad_logdet is None:
        raise ValueError("grad_output and grad_logdet are both absent")
    if grad_y is not None:
        _require_device(grad_y, "grad_output")
        if grad_y.shape != v.shape or grad_y.device != v.device:
            raise ValueError("grad_output must match the activation in shape and device")
    _per_image(grad_logdet, "grad_logdet", v)
    gs = torch.empty(1, dtype=torch.float32, device=v.device) if need_gs else None
    outs = (torch.empty_like(v) if need_x else None, _out_like(v, out) if need_gx else None, gs)
    if _nothing_to_launch(v, outs, (gs,)):
        return outs
    nbytes = _lib.lib().finc_activation_workspace_bytes(B, C, HW) if need_gs else None
    _call("finc_activation_backward_f32", v.device, code, p0, p1, sp, ACTIVATION_MODES[mode], _ptr(grad_y), _ptr(grad_logdet), v.data_ptr(),
          *map(_ptr, outs), B, C, HW, *_ws_args(v.device, nbytes), _stream_ptr(v))
    return outs


def _activation_backward(ctx, mode, grad_y, grad_logdet):
    v, slope = ctx.saved_tensors if ctx.has_slope else (*ctx.saved_tensors, None)
    need = ctx.needs_input_grad
    _, gx, gs = finc_activation_backward(grad_y, grad_logdet, v, ctx.kind, ctx.p0, ctx.p1, slope, mode, need_gx=need[0],
                                         need_gs=ctx.has_slope and need[1])
    return gx, (gs.view(ctx.slope_shape) if gs is not None else None), None, None, None


def _activation_record(ctx, saved, slope, kind, p0, p1):
    ctx.has_slope = slope is not None
    ctx.slope_shape = slope.shape if slope is not None else None
    ctx.save_for_backward(*((saved, slope) if slope is not None else (saved,)))
    ctx.kind, ctx.p0, ctx.p1 = kind, p0, p1


class _FincActivationFunction(torch.autograd.Function):
    """`finc_activation` in the forward direction under autograd: (y, logdet) and their backward on the HIP kernel, from the saved input."""

    @staticmethod
    def forward(ctx, x, slope, kind, p0, p1):
        x = x.contiguous()
        slope = slope.contiguous() if slope is not None else None
        y, logdet = finc_activation(x, kind, p0, p1, slope, 1, True)
        _activation_record(ctx, x, slope, kind, p0, p1)
        return y, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_logdet):
        return _activation_backward(ctx, "forward", *_incoming_grads(ctx.saved_tensors[0], grad_y, grad_logdet))


class _FincActivationReverseFunction(torch.autograd.Function):
    """`finc_activation` in the reverse direction under autograd (inside `reverse_grad()`), saved: its OUTPUT."""

    @staticmethod
    def forward(ctx, y, slope, kind, p0, p1):
        slope = slope.contiguous() if slope is not None else None
        x = finc_activation(y.contiguous(), kind, p0, p1, slope, -1)[0]
        _activation_record(ctx, x, slope, kind, p0, p1)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x):
        return _activation_backward(ctx, "reverse", grad_x.contiguous(), None)


class _FincActivationReverseLogdetFunction(torch.autograd.Function):
    """The reverse with the forward log-det at its result, one pass; saved: its output x."""

    @staticmethod
    def forward(ctx, y, slope, kind, p0, p1):
        slope = slope.contiguous() if slope is not None else None
        x, logdet = finc_activation(y.contiguous(), kind, p0, p1, slope, -1, True)
        _activation_record(ctx, x, slope, kind, p0, p1)
        return x, logdet

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x, grad_logdet):
        return _activation_backward(ctx, "reverse", *_incoming_grads(ctx.saved_tensors[0], grad_x, grad_logdet))


def activation_forward(x, kind, p0=0.0, p1=0.0, slope=None):
    """`finc_activation(x, ..., +1, want_logdet=True)` under autograd: (y, logdet), gradients for `x` and `slope`."""
    return _FincActivationFunction.apply(x, slope, kind, p0, p1)


def activation_reverse(y, kind, p0=0.0, p1=0.0, slope=None):
    """`finc_activation(y, ..., -1)[0]` under autograd: gradients for `y` and `slope`."""
    return _FincActivationReverseFunction.apply(y, slope, kind, p0, p1)


def activation_reverse_logdet(y, kind, p0=0.0, p1=0.0, slope=None):
    """`finc_activation(y, ..., -1, want_logdet=True)` under autograd: (x, forward log-det at x)."""
    return _FincActivationReverseLogdetFunction.apply(y, slope, kind, p0, p1)


def inverse(input, kernel, output):
    """Drop-in for the reference extension's `inverse` (cinc_cuda_level2.cpp:19-32).

    input  [B,C,H,W]        already flipped to TL-canonical per group by the caller (fastflow.py:85-90)
    kernel [G*Cq,Cq,KH,KW]  TL-canonical (fastflow.py:79-84); G = kernel.shape[0] // kernel.shape[1]
    output [B,C,H,W]        written in place; a one-element list aliasing it is returned.
    """
    dt = _float_dtype(input, "input")
    for t, n in ((input, "input"), (kernel, "kernel"), (output, "output")):
        _require_device(t, n, dt)
    G = kernel.shape[0] // kernel.shape[1]
    finc_inverse(input, kernel, G=G, orient=0, out=output)
    return [output]


class _DeviceBank:
    """What PackedWeights holds for ONE device and ONE weight version: a new version starts from a fresh object."""
    __slots__ = ("key", "keep", "validated", "w_canon", "ready", "linv", "linv_ready", "packed", "adjoint", "adjoint_ready")

    def __init__(self, key=None, keep=None, w_canon=None):
        self.key = key
        self.keep = keep          # the source tensors' storages, kept alive while the entry is (see PackedWeights._get)
        self.validated = False    # check_invariant has run on THIS weight version
        self.w_canon = w_canon
        # (every derived tensor below has its `Ready` token: the stream it was built on, and the event behind its fill)
        self.ready = Ready(w_canon.device) if w_canon is not None else None
        self.linv = self.linv_ready = None
        self.packed = {}          # bank kind -> (key of the folded affine parameters or None, packed fragments, their token)
        self.adjoint = None       # (w_adj, lead_t) of the backward through the inverse (finc_adjoint_weights_f32), built by the first one
        self.adjoint_ready = None


def _fold_forward(log_scale, translation):
    """(y - translation) * exp(-log_scale) behind the forward, as the (scale, shift) its bank carries."""
    scale = torch.exp(-log_scale.detach().float()).contiguous()
    return scale, (-translation.detach().float() * scale).contiguous()


def _fold_inverse(log_scale, translation):
    """exp(log_scale) * y + translation in front of the inverse, as the (scale, shift) its bank carries."""
    return torch.exp(log_scale.detach().float()).contiguous(), translation.detach().float().contiguous()


def _packed(bank, kind, pack, t, G, dims, fold=None, params=(), may_refuse=False, src=None):
    """The bank's packed fragments of one kind, allocated and packed by the entry point `pack` on `t`'s stream the first time a
    weight version asks for them -- and, for a kind that carries `fold(*params)` = (scale, shift), again when (address, version) of
    the parameters change.  `may_refuse`: None, and nothing cached, when the pack answers FINC_ERR_UNSUPPORTED.  `src`: the canonical
    bank to pack when it is not the entry's own (the adjoint bank)."""
    key = version_key(*params) if fold is not None else None
    hit = bank.packed.get(kind)
    if hit is not None and hit[0] == key:
        hit[2].wait(hit[1])
        return hit[1]
    B, Cq, H, W, KH, KW = dims
    affine = ()
    if fold is not None:
        scale, shift = fold(*params)
        if scale.numel() != G * Cq or shift.numel() != G * Cq:
            raise ValueError("affine parameters must have one entry per channel")
        affine = (scale.data_ptr(), shift.data_ptr())
    packed = torch.empty(_lib.lib().finc_workspace_bytes(G, Cq, KH, KW), dtype=torch.uint8, device=t.device)
    if _call(pack, t.device, (bank.w_canon if src is None else src).data_ptr(), *affine, packed.data_ptr(), G, Cq, KH, KW, _stream_ptr(t),
             may_refuse=may_refuse):
        return None
    bank.packed[kind] = (key, packed, Ready(t.device))
    return packed


def _launch_packed(name, t, packed, out, G, dims, orient, may_refuse=False):
    """One launch on packed fragments: finc_forward_packed_f32, finc_inverse_packed_f32 or finc_inverse_packed_premultiplied_f32."""
    B, Cq, H, W, KH, KW = dims
    return _call(name, t.device, t.data_ptr(), packed.data_ptr(), out.data_ptr(), B, G, Cq, H, W, KH, KW, orient, _stream_ptr(t),
                 may_refuse=may_refuse)


def _has_mfma(query, t, dims):
    """Does `query` (finc_forward_algo_for / finc_inverse_algo_for) name an MFMA instantiation for these (non-empty) activations?"""
    return t.numel() != 0 and getattr(_lib.lib(), query)(*dims[1:]) == _lib.ALGO["mfma"]


def _f64(bank):
    """A float64 entry: the canonical bank and its check, no packed fragments of any kind."""
    return bank.w_canon.dtype == torch.float64


def _aligned16(t, out):
    """The packed inverse streams 16-byte pieces (a view into a larger allocation may be only 4-byte aligned; INTEGRATION.md: such
    calls fall back)."""
    return not (t.data_ptr() | (out.data_ptr() if out is not None else 0)) & 15


class PackedWeights:
    """Sampling-time cache for one weight version: the TL-canonical bank (fastflow.py:79-84, done once instead of
    every call), its invariant check, and the packed MFMA fragments (finc_pack_inverse_weights_f32), so that a
    sampling step is exactly one kernel launch (finc_inverse_packed_f32).  Rebuilt when a source tensor changes.

    State is kept PER DEVICE: the reference wraps its models in nn.DataParallel (fastflow_cifar_multi_gpu.py:439-440),
    whose replicas are shallow copies that share this object while their weights live on different devices and their
    forwards run on different threads."""

    def __init__(self):
        self._banks = {}
        self._lock = threading.Lock()

    # A copy of the owning module (copy.deepcopy for an EMA model, pickle, torch.save of the module) starts from an empty cache with a
    # lock of its own: the banks are derived from the weights -- the copy's first call rebuilds them from ITS weights -- and a lock
    # cannot be pickled.
    def __deepcopy__(self, memo):
        return type(self)()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()

    def _bank(self, device):
        b = self._banks.get(device)
        if b is None:
            with self._lock:
                b = self._banks.setdefault(device, _DeviceBank())
        return b

    def invalidate(self):
        """Force a rebuild on the next call.  Needed after writes that do not bump Tensor._version
        (torch.distributed collectives, writes through `.data`)."""
        with self._lock:
            self._banks = {}

    # what single-device callers and tests read
    @property
    def w_canon(self):
        banks = list(self._banks.values())
        return banks[0].w_canon if len(banks) == 1 else None

    def get(self, weights, G, orient):
        return self._get(weights, G, orient).w_canon

    def _get(self, weights, G, orient, validate=True):
        """`validate=False`: the training path -- the gradient mask keeps the corner tap unit triangular (layers/conv.py:98-99,
        applied inside the HIP backward), and the check is a device->host synchronisation per layer and step."""
        device = weights[0].device
        bank = self._bank(device)
        # The entry is keyed on (address, version counter) of every source tensor AND holds their storages alive: a weight
        # rebound through `.data` to a fresh tensor keeps its version counter, and the address of a freed tensor is the first
        # one the allocator hands out again -- with the old storage still referenced here the new one cannot land on it.
        key = version_key(*weights) + (orient,)
        if key != bank.key:
            ws = torch.cat([w.detach() for w in weights], dim=0).contiguous() if len(weights) > 1 else weights[0].detach().contiguous()
            # (a fresh entry: not validated, no packed fragments of any kind, no Linv)
            bank = self._banks[device] = _DeviceBank(key, tuple(w.untyped_storage() for w in weights), canonicalize(ws, G, orient))
        else:
            bank.ready.wait(bank.w_canon)
        # An entry the training path created (validate=False) is NOT validated: the first inference call on the same weight
        # version runs the check, so an optimiser effect outside the in-kernel gradient mask (weight decay on the diagonal,
        # a manual edit followed by a forward under grad) cannot reach the inverse unnoticed.
        if validate and not bank.validated:
            check_invariant(bank.w_canon, G)
            bank.validated = True
        return bank

    def _enter(self, t, weights, G, orient, validate=True):
        """What every launch starts with: the device's entry for this weight version, and (B, Cq, H, W, KH, KW) of activations `t`."""
        bank = self._get(weights, G, orient, validate)
        _require_device(t, "input", bank.w_canon.dtype)
        return bank, _dims(t, bank.w_canon, G)

    def forward(self, x, weights, G, orient, out=None, validate=True):
        """Forward on the cached canonical bank + cached strip-kernel fragments (also the forward of the autograd path: a
        weight version that has not changed since the last call -- evaluation under grad, several micro-batches per
        optimiser step -- costs no cat / canonicalise / pack launch)."""
        bank, dims = self._enter(x, weights, G, orient, validate)
        # (float64: finc_forward_f64_algo packs into the workspace per launch -- there are no cached fp64 fragments)
        if _f64(bank) or not _has_mfma("finc_forward_algo_for", x, dims):
            return finc_forward(x, bank.w_canon, G, orient, out=out)
        packed = _packed(bank, "fwd", "finc_pack_forward_weights_f32", x, G, dims)
        if out is None:
            out = torch.empty_like(x)
        _launch_packed("finc_forward_packed_f32", x, packed, out, G, dims, orient)
        return out

    def forward_affine(self, x, weights, G, orient, log_scale, translation, out=None):
        """(forward(x) - translation) * exp(-log_scale) in ONE launch: the per-channel affine layer BEHIND the unit in the
        model (ActNorm.forward, layers/actnorm.py:39-46) folded into the forward bank -- filter rows scaled, accumulators
        started from the shift.  Returns None when the shape has no MFMA strip kernel (the caller runs the two layers)."""
        if weights[0].dtype != torch.float32:        # (fp32 only: the caller runs the two layers)
            return None
        bank, dims = self._enter(x, weights, G, orient)
        if not _has_mfma("finc_forward_algo_for", x, dims):
            return None
        packed = _packed(bank, "fwd_affine", "finc_pack_forward_weights_affine_f32", x, G, dims, _fold_forward, (log_scale, translation))
        if out is None:
            out = torch.empty_like(x)
        _launch_packed("finc_forward_packed_f32", x, packed, out, G, dims, orient)
        return out

    def _inverse_packed(self, name, t, bank, out, G, dims, orient):
        """`name` (a packed inverse launch) on the plain inverse fragments."""
        _launch_packed(name, t, _packed(bank, "inv", "finc_pack_inverse_weights_f32", t, G, dims), out, G, dims, orient)
        return out

    def inverse(self, z, weights, G, orient, out=None, validate=True):
        """`validate=False`: the training path's inverse (the backward that rebuilds a unit's input from its output), as in `_get`."""
        bank, dims = self._enter(z, weights, G, orient, validate)
        if out is None and z.numel():
            out = torch.empty_like(z)
        # the packed launch needs fp32, an MFMA instantiation AND 16-byte aligned activations
        if _f64(bank) or not (_has_mfma("finc_inverse_algo_for", z, dims) and _aligned16(z, out)):
            return finc_inverse(z, bank.w_canon, G, orient, out=out)
        return self._inverse_packed("finc_inverse_packed_f32", z, bank, out, G, dims, orient)

    @staticmethod
    def inverse_backward(bank, grad_x, x, G, orient, need_gz=True, need_gw=True):
        """Gradients of x = inverse(z) on the entry `bank` of the weight version the forward ran on, given grad_x and the
        inverse's OUTPUT x: (grad_z, grad_w_canon), each computed only if asked for.  grad_z = blockdiag(L^-T) inverse(grad_x) on the
        adjoint bank with every group's orientation complemented; grad_w_canon = -(the forward's weight gradient at (x, grad_z)), masked
        in-kernel.  The adjoint bank (w_adj, lead_t) and its packed fragments are a bank kind of the entry: built by the first backward
        of a weight version, dropped with it.  The solve takes `inverse`'s route: the packed launch when there is an MFMA instantiation
        and the activations are 16-byte aligned, otherwise finc_inverse."""
        _require_device(grad_x, "grad_output")
        w_canon = bank.w_canon
        _require_device(w_canon, "kernel")        # (fp32 only: ops.inverse_reverse refuses float64 before it gets here)
        dims = _dims(grad_x, w_canon, G)
        B, Cq, H, W, KH, KW = dims
        gw = torch.empty_like(w_canon) if need_gw else None
        if grad_x.numel() == 0:
            if gw is not None:
                gw.zero_()
            return (torch.empty_like(grad_x) if need_gz else None), gw
        if bank.adjoint is None:
            w_adj = torch.empty_like(w_canon)
            lead_t = torch.empty(G * Cq, G * Cq, dtype=torch.float32, device=w_canon.device)
            _call("finc_adjoint_weights_f32", w_canon.device, w_canon.data_ptr(), w_adj.data_ptr(), lead_t.data_ptr(), G, Cq, KH, KW,
                  _stream_ptr(grad_x))
            bank.adjoint, bank.adjoint_ready = (w_adj, lead_t), Ready(w_canon.device)
        else:
            bank.adjoint_ready.wait(*bank.adjoint)
        w_adj, lead_t = bank.adjoint
        adj_orient = orient ^ ((1 << (2 * G)) - 1)            # the transposed operator reads the opposite corner
        y = torch.empty_like(grad_x)
        if _has_mfma("finc_inverse_algo_for", grad_x, dims) and _aligned16(grad_x, y):
            packed = _packed(bank, "inv_adjoint", "finc_pack_inverse_weights_f32", grad_x, G, dims, src=w_adj)
            _launch_packed("finc_inverse_packed_f32", grad_x, packed, y, G, dims, adj_orient)
        else:
            finc_inverse(grad_x, w_adj, G, adj_orient, out=y)
        _call("finc_lead_product_f32", y.device, y.data_ptr(), lead_t.data_ptr(), B, G, Cq, H * W, _stream_ptr(y))
        if need_gw:
            _call("finc_backward_f32", y.device, y.data_ptr(), x.data_ptr(), w_canon.data_ptr(), None, gw.data_ptr(), B, G, Cq, H, W, KH, KW,
                  orient, *_ws_args(y.device, _lib.lib().finc_backward_workspace_bytes(B, G, Cq, H, W, KH, KW)), _stream_ptr(y))
            _call("finc_negate_f32", gw.device, gw.data_ptr(), gw.numel(), _stream_ptr(y))
        return (y if need_gz else None), gw

    def lead_inverse(self, weights, G, orient):
        """Linv_g = inverse of the unit lower triangular tap of the pixel itself (canonical tap [KH-1, KW-1],
        layers/conv.py:63-70), [G, Cq, Cq] fp32 (solved in fp64), cached per weight version: what a channel mix in front of
        the unit multiplies into its matrix so that `inverse_premultiplied` can skip the z-term."""
        if weights[0].dtype != torch.float32:
            raise ValueError(f"lead_inverse serves the fp32 premultiplied inverse only, got {weights[0].dtype} weights")
        bank = self._get(weights, G, orient)
        if bank.linv is None:
            wc = bank.w_canon
            Cq = wc.shape[1]
            lead = wc.view(G, Cq, Cq, wc.shape[2], wc.shape[3])[:, :, :, -1, -1].double()
            eye = torch.eye(Cq, dtype=torch.float64, device=wc.device).expand(G, Cq, Cq)
            bank.linv = torch.linalg.solve_triangular(lead, eye, upper=False, unitriangular=True).float().contiguous()
            bank.linv_ready = Ready(wc.device)
        else:
            bank.linv_ready.wait(bank.linv)
        return bank.linv

    def premultiplied_supported(self, shape, weights, G, orient):
        """Does `inverse_premultiplied` exist for activations of this shape (the helper-wave form of the inverse: a problem
        set that fills the chip, W % 16 == 0)?  fp32 only."""
        if weights[0].dtype != torch.float32:
            return False
        w_canon = self._get(weights, G, orient).w_canon
        B, C, H, W = shape
        Cq, KH, KW = w_canon.shape[1], w_canon.shape[2], w_canon.shape[3]
        return C == G * Cq and bool(_lib.lib().finc_inverse_premultiplied_supported(B, G, Cq, H, W, KH, KW))

    def inverse_premultiplied(self, zp, weights, G, orient, out=None):
        """inverse(z) given zp = blockdiag(Linv) z (the channel mix in front of the unit applied Linv for free),
        ONE launch without the z-term's MFMAs.  None when the shape has no such kernel or the activations are not 16-byte
        aligned (the caller runs the plain chain), and for anything but fp32."""
        if weights[0].dtype != torch.float32:
            return None
        bank, dims = self._enter(zp, weights, G, orient)
        if zp.numel() == 0 or not _lib.lib().finc_inverse_premultiplied_supported(dims[0], G, *dims[1:]):
            return None
        if out is None:
            out = torch.empty_like(zp)
        if not _aligned16(zp, out):
            return None
        return self._inverse_packed("finc_inverse_packed_premultiplied_f32", zp, bank, out, G, dims, orient)

    def inverse_affine(self, y, weights, G, orient, log_scale, translation, out=None):
        """inverse(exp(log_scale) * y + translation) in ONE launch: the per-channel affine layer in front
        of the unit in the reverse chain (ActNorm.reverse, layers/actnorm.py:39-52) is folded into the packed bank.
        Returns None when the shape has no MFMA instantiation or the activations are not 16-byte aligned (the caller
        then runs the two layers one after the other), and for anything but fp32."""
        if weights[0].dtype != torch.float32:
            return None
        bank, dims = self._enter(y, weights, G, orient)
        if out is None and y.numel():
            out = torch.empty_like(y)
        if not (_has_mfma("finc_inverse_algo_for", y, dims) and _aligned16(y, out)):
            return None
        # the shift rides on the wavefront / role-split kernels only: the big banks and the wide maps that finc_big.hip takes
        # over from the 33..64-channel banks (Cq = 50 at 256 columns) carry a scale and nothing else -> two launches there
        if not _lib.lib().finc_inverse_affine_supported(dims[0], G, *dims[1:]):
            return None
        # FINC_ERR_UNSUPPORTED from the pack: a bank whose kernel cannot carry the shift (the big banks, finc_big.hip)
        packed = _packed(bank, "inv_affine", "finc_pack_inverse_weights_affine_f32", y, G, dims, _fold_inverse, (log_scale, translation),
                         may_refuse=True)
        # (the launch itself refuses a shift-carrying bank on a map it cannot serve)
        if packed is None or _launch_packed("finc_inverse_packed_f32", y, packed, out, G, dims, orient, may_refuse=True):
            return None
        return out


class _FincConvFunction(torch.autograd.Function):
    """The autograd.Function underneath FastFlowUnit / PaddedConv2d.forward.  Backward applies the
    corner-tap mask in-kernel, so `model.apply(clear_grad)` (train/experiment.py:16-18) is a no-op on it.
    The stored weights are inputs (one per group, so every parameter gets its own gradient without a cat node in the
    graph); the canonical bank and the forward fragments come from the layer's PackedWeights cache."""

    @staticmethod
    def forward(ctx, x, cache, G, orient, *weights):
        x = x.contiguous()
        out = cache.forward(x, list(weights), G, orient, validate=False)
        ctx.save_for_backward(x, cache._get(list(weights), G, orient, validate=False).w_canon)   # (same entry: no check, no synchronisation)
        ctx.G, ctx.orient, ctx.nw = G, orient, len(weights)
        return out

    @staticmethod
    def backward(ctx, grad_z):
        x, w_canon = ctx.saved_tensors
        need_gw = any(ctx.needs_input_grad[4:])
        gx, gw = finc_backward(grad_z.contiguous(), x, w_canon, ctx.G, ctx.orient,
                               need_gx=ctx.needs_input_grad[0], need_gw=need_gw)
        gws = (None,) * ctx.nw
        if gw is not None:
            gw = canonicalize(gw, ctx.G, ctx.orient)  # canonical -> stored orientation
            gws = tuple(gw.chunk(ctx.nw, dim=0)) if ctx.nw > 1 else (gw,)
        return (gx, None, None, None) + gws


def conv_forward(x, weights, G, orient, cache):
    """z = forward(x) under autograd.  `weights`: the stored (state-dict form) banks of the G groups, one tensor per group or
    one tensor for all; `cache`: the layer's PackedWeights."""
    return _FincConvFunction.apply(x, cache, G, orient, *weights)


class _FincInverseFunction(torch.autograd.Function):
    """The autograd.Function underneath the units' `reverse` inside `reverse_grad()`.  Forward: the cached launch of
    `PackedWeights.inverse`, invariant check included.  Saved: the OUTPUT and the canonical bank (with the cache entry of this weight
    version, which holds the adjoint bank).  Backward: `PackedWeights.inverse_backward`, then canonical -> stored per group as
    `_FincConvFunction.backward` does; only what `needs_input_grad` asks for is computed."""

    @staticmethod
    def forward(ctx, z, cache, G, orient, *weights):
        z = z.contiguous()
        out = cache.inverse(z, list(weights), G, orient)
        bank = cache._get(list(weights), G, orient)             # (same entry: canonical and checked already)
        ctx.save_for_backward(out, bank.w_canon)
        ctx.bank, ctx.G, ctx.orient, ctx.nw = bank, G, orient, len(weights)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x):
        x, _ = ctx.saved_tensors
        need_gw = any(ctx.needs_input_grad[4:])
        gz, gw = PackedWeights.inverse_backward(ctx.bank, grad_x.contiguous(), x, ctx.G, ctx.orient,
                                                need_gz=ctx.needs_input_grad[0], need_gw=need_gw)
        gws = (None,) * ctx.nw
        if gw is not None:
            gw = canonicalize(gw, ctx.G, ctx.orient)  # canonical -> stored orientation
            gws = tuple(gw.chunk(ctx.nw, dim=0)) if ctx.nw > 1 else (gw,)
        return (gz, None, None, None) + gws


def inverse_reverse(z, weights, G, orient, cache):
    """x = inverse(z) under autograd (see `reverse_grad`): gradients for `z` and for every stored bank in `weights`.  fp32 tensors on
    the device only: anything else raises instead of returning a detached result."""
    if not z.is_cuda or z.dtype != torch.float32 or z.dim() != 4:
        raise _lib.FincError("reverse_grad(): the differentiable inverse takes fp32 [B,C,H,W] tensors on the device, got "
                             f"{z.dtype} on {z.device} with {z.dim()} dimensions (there is no fp64 and no CPU backward)")
    return _FincInverseFunction.apply(z, cache, G, orient, *weights)
