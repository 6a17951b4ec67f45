"""GPU helper: the mixing kernel (ops.finc_mix) against F.conv2d / torch.matmul at the bench shapes.

`backward`: glow.Conv1x1 forward + backward on the HIP kernels (ops.mix_forward) against the F.conv2d autograd path (the same module
with ops.mix_supported patched to False), alternately in this one process, plus the legs of finc_mix_backward_f32 on their own.
`backward trace`: a few calls per shape and nothing else, for a `rocprofv3 --kernel-trace --stats` run."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "2")
import torch
from fincflow_amd import ops
dev = torch.device("cuda:0")
def timeit(fn, n=50):
    t_end = time.perf_counter() + 0.3        # clocks ramp up over the first tenths of a second of load
    while time.perf_counter() < t_end:
        for _ in range(5): fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3
def backward_leg(trace):
    import statistics
    import numpy as np
    from fincflow_amd import glow
    supported = ops.mix_supported
    for (B, C, H, W) in ((256, 96, 64, 64), (64, 192, 128, 128), (64, 48, 32, 32)):
        np.random.seed(C); torch.manual_seed(C)
        c = glow.Conv1x1(C).to(dev)
        x = torch.randn(B, C, H, W, device=dev).requires_grad_(True); g = torch.randn(B, C, H, W, device=dev)
        M = c.W.detach().contiguous(); xd = x.detach(); o = torch.empty_like(xd)
        def step():
            x.grad = None; c.W.grad = None
            z, _ = c(x)
            z.backward(g)
        def path(hip):
            ops.mix_supported = supported if hip else (lambda C: False)
        if trace:
            for hip in (True, False):
                path(hip)
                for _ in range(5): step()
            path(True)
            for _ in range(5): ops.finc_mix(xd, M, out=o)
            torch.cuda.synchronize()
            continue
        new, old = [], []
        for r in range(7):                       # alternately, so that clocks and neighbours on the box hit both alike
            path(True); new.append(timeit(step, 20))
            path(False); old.append(timeit(step, 20))
        path(True)
        gw_new, gx_new = c.W.grad.clone(), x.grad.clone()
        path(False); step(); path(True)
        err = max(float((gw_new - c.W.grad).abs().max() / c.W.grad.abs().max()), float((gx_new - x.grad).abs().max() / x.grad.abs().max()))
        med = statistics.median
        spread = lambda v: (max(v) - min(v)) / med(v) * 100
        print(f"B{B} C{C} {H}x{W}: Conv1x1 fwd+bwd HIP {med(new):.1f} us (min {min(new):.1f} max {max(new):.1f}, spread {spread(new):.1f} %) | "
              f"F.conv2d autograd {med(old):.1f} us (min {min(old):.1f} max {max(old):.1f}, spread {spread(old):.1f} %) | ratio {med(old) / med(new):.2f} | "
              f"max rel diff of the gradients {err:.1e}", flush=True)
        tf = timeit(lambda: ops.finc_mix(xd, M, out=o))
        tx = timeit(lambda: ops.finc_mix_backward(g, None, M, True, False, False))
        tm = timeit(lambda: ops.finc_mix_backward(g, xd, M, False, True, False))
        ta = timeit(lambda: ops.finc_mix_backward(g, xd, M, True, True, True))
        gbs = 8 * xd.numel() / 1e3
        print(f"    legs: forward mix {tf:.1f} us ({gbs / tf:.0f} GB/s) | grad_in {tx:.1f} | grad_mat (kernel + reduce) {tm:.1f} ({gbs / tm:.0f} GB/s, "
              f"{2 * xd.numel() * C / tm / 1e6:.1f} TF) | all three {ta:.1f}", flush=True)
if len(sys.argv) > 1 and sys.argv[1] == "backward":
    backward_leg(len(sys.argv) > 2 and sys.argv[2] == "trace")
    sys.exit(0)
SHAPES = ((256, 96, 64, 64), (64, 48, 32, 32), (64, 192, 128, 128), (128, 12, 16, 16), (256, 96, 63, 63))
if len(sys.argv) > 1 and sys.argv[1] == "sweep":   # every channel count of the kernel's table at a chip-filling size
    SHAPES = tuple((max(8, 4096 // C) * 8, C, 64, 64) for C in (4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192))
for (B, C, H, W) in SHAPES:
    x = torch.randn(B, C, H, W, device=dev); M = torch.randn(C, C, device=dev) / C ** 0.5; b = torch.randn(C, device=dev)
    o = torch.empty_like(x)
    t = timeit(lambda: ops.finc_mix(x, M, b, out=o))
    ref = torch.nn.functional.conv2d(x, M.view(C, C, 1, 1), b)
    err = float((o - ref).abs().max() / ref.abs().max())
    tm = timeit(lambda: torch.matmul(M, x.view(B, C, H * W)), 20)
    tc = timeit(lambda: torch.nn.functional.conv2d(x, M.view(C, C, 1, 1), b), 20)
    gb = 8 * x.numel() / t / 1e3
    print(f"B{B} C{C} {H}x{W}: mix {t:.1f} us ({gb:.0f} GB/s, {2*x.numel()*C/t/1e6:.1f} TF) | torch.matmul {tm:.1f} | F.conv2d {tc:.1f} | rel err vs conv2d {err:.1e}", flush=True)
