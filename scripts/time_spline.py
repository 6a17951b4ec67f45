"""GPU helper: the spline kernels (ops.finc_spline, ops.finc_spline_backward, ops.finc_spline_reverse_backward) at
[256, 96, 64, 64], shared and individual weights, 5 bins, tail_bound 10, beside two references timed alternately in this one process
(HIP events, 7 rounds per leg, median and min..max):
  (a) ops.finc_actnorm / ops.finc_actnorm_backward, which move the same activation bytes (the ratio is reported);
  (b) the layer's own PyTorch lines (glow.rq_spline_lines) on the same build, forward and, for the backwards, under autograd.
Legs: the transform each way with and without the log-det, and both backwards (grad_x and grad_table).  There was no earlier
spline kernel: nothing here is a speed-up of one.  `time_spline.py B C H W` times another shape."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fincflow_amd import glow, ops
dev = torch.device("cuda:0")
med = statistics.median
def timeit(fn, n):
    t_end = time.perf_counter() + 0.2        # clocks ramp up over the first tenths of a second of load
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3
def legs(name, fns, n):
    """fns: label -> (callable, launches per measurement); alternately, so that clocks and neighbours on the box hit all alike"""
    times = {k: [] for k in fns}
    for _ in range(7):
        for k, (fn, reps) in fns.items():
            times[k].append(timeit(fn, max(1, n // reps)))
    line = " | ".join(f"{k} {med(v):.1f} us ({min(v):.1f}..{max(v):.1f})" for k, v in times.items())
    s, a = times["spline"], times.get("actnorm")
    verdict = ""
    if a:
        within = min(s) <= max(a) and min(a) <= max(s)
        verdict = f" | spline / actnorm {med(s) / med(a):.2f}, {'within' if within else 'NOT within'} the alternated spread"
    print(f"  {name}: {line}{verdict} | lines / spline {med(times['lines']) / med(s):.1f}", flush=True)
B, C, H, W = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (256, 96, 64, 64)
K, TB = 5, 10.0
torch.manual_seed(0)
x = 4.0 * torch.randn(B, C, H, W, device=dev)                      # about 1 % of the elements in the tails
gy = torch.randn(B, C, H, W, device=dev); gl = torch.randn(B, device=dev)
y = torch.empty_like(x)
ls = 0.3 * torch.randn(C, device=dev); t = torch.randn(C, device=dev)
print(f"B{B} C{C} {H}x{W}, {K} bins, tail_bound {TB}; HIP events, legs alternated, 7 rounds, median (min..max)", flush=True)
for individual in (False, True):
    m = glow.SplineActivation((C, H, W), n_bins=K, tail_bound=TB, individual_weights=individual).to(dev)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p))
        table = m._compose()
        knots = [k.reshape((1, C, H, W, K + 1) if individual else (K + 1,)) for k in m._knots()]
    print(f"individual_weights={individual} (P = {table.shape[1]}):", flush=True)
    def lines(inverse, want_logdet):
        out, lad = glow.rq_spline_lines(x, *knots, TB, inverse)
        return (out, lad.flatten(1).sum(-1)) if want_logdet else out
    def lines_backward(inverse):
        a = x.detach().requires_grad_(True)
        ks = [k.detach().requires_grad_(True) for k in knots]
        out, lad = glow.rq_spline_lines(a, *ks, TB, inverse)
        torch.autograd.backward([out, lad.flatten(1).sum(-1)], [gy, gl])
    with torch.no_grad():
        for direction, tag in ((1, "forward"), (-1, "reverse")):
            for want in (True, False):
                fns = {"spline": (lambda: ops.finc_spline(x, table, TB, direction, want, out=y), 1),
                       "actnorm": (lambda: ops.finc_actnorm(x, ls, t, direction, want, out=y), 1),
                       "lines": (lambda: lines(direction < 0, want), 10)}
                legs(f"{tag}{' + logdet' if want else ''}", fns, 20)
    fns = {"spline": (lambda: ops.finc_spline_backward(gy, gl, x, table, TB), 1),
           "actnorm": (lambda: ops.finc_actnorm_backward(gy, gl, x, ls), 1),
           "lines": (lambda: lines_backward(False), 10)}
    legs("backward (grad_x, grad_table) [lines: forward + autograd backward]", fns, 20)
    fns = {"spline": (lambda: ops.finc_spline_reverse_backward(gy, gl, x, table, TB), 1),
           "actnorm": (lambda: ops.finc_actnorm_reverse_backward(gy, x, ls), 1),
           "lines": (lambda: lines_backward(True), 10)}
    legs("reverse backward (grad_y, grad_table) [lines: forward + autograd backward]", fns, 20)
    del m, table, knots
