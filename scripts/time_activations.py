"""GPU helper: the smooth invertible activations' kernels (ops.finc_activation, ops.finc_activation_backward) at [256, 96, 64, 64],
each kind beside two references timed alternately in this one process (HIP events, 7 rounds per leg, median and min..max):
  (a) ops.finc_actnorm / ops.finc_actnorm_backward, the memory-bound siblings that move the same activation bytes (the ratio is
      reported, whatever it is: the smooth kinds' inverses run nine Newton trips in registers and are expected to be instruction-bound);
  (b) the layer's own PyTorch lines on the same build, forward and, for the backwards, under autograd.
Legs: forward with the log-det, reverse, reverse with the log-det, and the three backward modes.  Then one training step and
`sample(256)` of the tests' stack ([Squeeze, FastFlowUnit, activation, ActNorm, Conv1x1, Coupling] x 2 around a SplitPrior, 3 x 8 x 8).
There was no earlier kernel for these layers: nothing here is a speed-up of one.  `time_activations.py B C H W` times another shape."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fincflow_amd import FastFlowUnit, FlowSequential, glow, ops
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
    tail = ""
    if "actnorm" in times:
        tail += f" | hip / actnorm {med(times['hip']) / med(times['actnorm']):.2f}"
    if "lines" in times:
        tail += f" | lines / hip {med(times['lines']) / med(times['hip']):.1f}"
    print(f"  {name}: {line}{tail}", flush=True)
B, C, H, W = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (256, 96, 64, 64)
torch.manual_seed(0)
x = 4.0 * torch.randn(B, C, H, W, device=dev)
gy = torch.randn(B, C, H, W, device=dev); gl = torch.randn(B, device=dev)
y = torch.empty_like(x); gx = torch.empty_like(x)
ls = 0.3 * torch.randn(C, device=dev); t = torch.randn(C, device=dev)
print(f"B{B} C{C} {H}x{W}; HIP events, legs alternated, 7 rounds, median (min..max); inverse trips {glow.ACTIVATION_TRIPS}", flush=True)
for m in (glow.SmoothLeakyRelu(0.3), glow.LeakyRelu(0.1), glow.LearnableLeakyRelu(), glow.SmoothTanh(1.0, 0.1)):
    m = m.to(dev)
    with torch.no_grad():
        if m.kind == "learnable_leaky_relu":
            m.alpha_logit.fill_(0.4)
        slope = m._slope()
    args = (m.kind, *m._numbers(), slope)
    learnable = slope is not None
    print(f"{type(m).__name__}{m._numbers() if not learnable else ''}:", flush=True)
    def lines(inverse, want_logdet):
        out, lad = m._lines(x, inverse)
        return (out, lad.flatten(1).sum(-1)) if want_logdet else out
    def lines_backward(inverse):
        m.zero_grad(set_to_none=True)
        a = x.detach().requires_grad_(True)
        out, lad = m._lines(a, inverse)
        ld = lad.flatten(1).sum(-1)
        if ld.requires_grad:
            torch.autograd.backward([out, ld], [gy, gl])
        else:                                    # (the fixed leaky ReLU: its log-derivative is piecewise constant)
            out.backward(gy)
    with torch.no_grad():
        for direction, want, tag in ((1, True, "forward + logdet"), (-1, False, "reverse"), (-1, True, "reverse + logdet")):
            fns = {"hip": (lambda: ops.finc_activation(x, *args, direction, want, out=y), 1),
                   "actnorm": (lambda: ops.finc_actnorm(x, ls, t, direction, want, out=y), 1),
                   "lines": (lambda: lines(direction < 0, want), 10)}
            legs(tag, fns, 20)
        xr = ops.finc_activation(x, *args, -1)[0]
        yf = ops.finc_activation(x, *args, 1)[0]
    fns = {"hip": (lambda: ops.finc_activation_backward(gy, gl, x, *args, mode="forward", need_gs=learnable, out=gx), 1),
           "actnorm": (lambda: ops.finc_actnorm_backward(gy, gl, x, ls), 1),
           "lines": (lambda: lines_backward(False), 10)}
    legs("backward, forward mode [lines: forward + autograd backward]", fns, 20)
    fns = {"hip": (lambda: ops.finc_activation_backward(gy, gl, xr, *args, mode="reverse", need_gs=learnable, out=gx), 1),
           "actnorm": (lambda: ops.finc_actnorm_reverse_backward(gy, x, ls), 1),
           "lines": (lambda: lines_backward(True), 10)}
    legs("backward, reverse mode [lines: reverse + autograd backward]", fns, 20)
    fns = {"hip": (lambda: ops.finc_activation_backward(gy, gl, yf, *args, mode="rebuild", need_x=True, need_gs=learnable, out=gx), 1),
           "actnorm": (lambda: ops.finc_actnorm_backward_reconstruct(gy, gl, x, ls, t), 1)}
    legs("backward, rebuild mode (x and grad_x in one launch)", fns, 20)
    del m, xr, yf
del x, gy, y, gx
torch.cuda.empty_cache()
def stack(kinds):
    layers, size = [], (3, 8, 8)
    for level, make in enumerate(kinds):
        layers.append(glow.Squeeze())
        size = (size[0] * 4, size[1] // 2, size[2] // 2)
        layers += [FastFlowUnit(size[0], size[0], (3, 3)), make(), glow.ActNorm(size[0]), glow.Conv1x1(size[0]), glow.Coupling(size, width=16)]
        if level == 0:
            layers.append(glow.SplitPrior(size, glow.GaussianPrior, width=16))
            size = (size[0] // 2, size[1], size[2])
    return FlowSequential(glow.GaussianPrior(size), *layers)
print("the stack on 3 x 8 x 8, batch 256: one training step (log_prob, backward, Adam) and sample(256)", flush=True)
for name, kinds in (("SmoothLeakyRelu x 2", (glow.SmoothLeakyRelu, glow.SmoothLeakyRelu)), ("SmoothTanh + LearnableLeakyRelu", (glow.SmoothTanh, glow.LearnableLeakyRelu))):
    torch.manual_seed(1)
    model = stack(kinds).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    batch = torch.randn(256, 3, 8, 8, device=dev)
    def step():
        opt.zero_grad(set_to_none=True)
        (-model.log_prob(batch).mean()).backward()
        opt.step()
    def sample():
        with torch.no_grad():
            model.sample(256)
    step()
    legs(name, {"hip": (step, 1)}, 10)
    legs(name + ", sample(256)", {"hip": (sample, 1)}, 10)
