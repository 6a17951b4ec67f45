"""GPU helper: the ActNorm kernels (ops.finc_actnorm, ops.actnorm_forward, ops.finc_actnorm_init) against the PyTorch formula they
replace (layers/actnorm.py:17-65), alternately in this one process: medians and spread of 7 rounds per path.  Legs: forward +
log-det, reverse, forward + backward (all three gradients), the data-dependent initialisation.  Shapes: the three levels of the c4
stack and one chip-filling map; there also the bytes per second of the forward (one tensor read, one written) beside ops.finc_mix,
which moves the same two tensors.  `time_actnorm.py json PATH` also writes the figures.  `time_actnorm.py flowstep` runs nothing but
five training steps of [FastFlowUnit, ActNorm, Conv1x1] at c3's shape, for a kernel trace; the timing of that step against the
parent commit, builds side by side, is scripts/time_actnorm_flowstep.py."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
med = statistics.median
def ab(name, hip, torch_fn, n, out):
    new, old = [], []
    for _ in range(7):                           # alternately, so that clocks and neighbours on the box hit both alike
        new.append(timeit(hip, n)); old.append(timeit(torch_fn, n))
    spread = lambda v: (max(v) - min(v)) / med(v) * 100
    gap = min(old) - max(new)                    # > 0: every HIP round beat every PyTorch round
    pairs = sum(a < b for a, b in zip(new, old))  # rounds in which HIP beat the PyTorch leg timed right after it
    print(f"  {name}: HIP {med(new):.1f} us (min {min(new):.1f} max {max(new):.1f}, spread {spread(new):.1f} %) | PyTorch {med(old):.1f} us "
          f"(min {min(old):.1f} max {max(old):.1f}, spread {spread(old):.1f} %) | ratio {med(old) / med(new):.2f} | "
          f"{'faster by more than the spread' if gap > 0 else 'NOT separated from the spread'}, {pairs} of {len(new)} adjacent pairs", flush=True)
    out[name] = {"hip_us": new, "torch_us": old, "ratio_of_medians": med(old) / med(new), "separated": gap > 0, "pairs_won": pairs}
    return med(new)
def torch_fwd(x, ls, t):
    return (x - t.view(1, -1, 1, 1)) * torch.exp(-ls.view(1, -1, 1, 1)), -ls.sum().expand(x.size(0)) * (x.shape[2] * x.shape[3])
def torch_rev(x, ls, t):
    return x * torch.exp(ls.view(1, -1, 1, 1)) + t.view(1, -1, 1, 1)
def torch_init(x, ls, t):
    t.copy_(x.mean(dim=(0, 2, 3))); ls.copy_(torch.log(x.std(dim=(0, 2, 3)) + 1e-8))
results = {}
only_flowstep = len(sys.argv) > 1 and sys.argv[1] == "flowstep"
for (B, C, H, W) in (() if only_flowstep else ((128, 12, 16, 16), (128, 24, 8, 8), (128, 48, 4, 4), (256, 96, 64, 64))):
    torch.manual_seed(C)
    x = torch.randn(B, C, H, W, device=dev) * 1.7 + 0.3
    ls = 0.3 * torch.randn(C, device=dev); t = torch.randn(C, device=dev)
    gy = torch.randn(B, C, H, W, device=dev); gl = torch.randn(B, device=dev)
    y = torch.empty_like(x); pl, pt = torch.zeros_like(ls), torch.zeros_like(t)
    n = 20 if x.numel() > (1 << 24) else 200     # the small maps are bound by the host's launches: long legs, or its jitter is the result
    print(f"B{B} C{C} {H}x{W}:", flush=True)
    r = results[f"{B}x{C}x{H}x{W}"] = {}
    with torch.no_grad():
        ab("forward + logdet", lambda: ops.finc_actnorm(x, ls, t, 1, True, out=y), lambda: torch_fwd(x, ls, t), n, r)
        ab("reverse", lambda: ops.finc_actnorm(x, ls, t, -1, out=y), lambda: torch_rev(x, ls, t), n, r)
        ab("data-dependent init", lambda: ops.finc_actnorm_init(x, pl, pt), lambda: torch_init(x, pl, pt), n, r)
    leaves = [v.clone().requires_grad_(True) for v in (x, ls, t)]
    def step(hip):
        for v in leaves: v.grad = None
        yy, ld = ops.actnorm_forward(*leaves) if hip else torch_fwd(*leaves)
        torch.autograd.backward([yy, ld], [gy, gl])
    ab("forward + backward", lambda: step(True), lambda: step(False), n, r)
    step(True); g_new = [v.grad.clone() for v in leaves]
    step(False)
    r["max_rel_diff_of_the_gradients"] = max(float((g - v.grad).abs().max() / v.grad.abs().max()) for g, v in zip(g_new, leaves))
    print(f"  max rel diff of the gradients, HIP against PyTorch: {r['max_rel_diff_of_the_gradients']:.1e}", flush=True)
    del leaves, g_new
    if ops.mix_supported(C) and x.numel() > (1 << 24):
        M = torch.randn(C, C, device=dev) / C ** 0.5
        with torch.no_grad():
            tfs, tms = [], []
            for _ in range(5):
                tfs.append(timeit(lambda: ops.finc_actnorm(x, ls, t, 1, True, out=y), n)); tms.append(timeit(lambda: ops.finc_mix(x, M, out=y), n))
        gbf, gbm = 8 * x.numel() / med(tfs) / 1e3, 8 * x.numel() / med(tms) / 1e3
        print(f"  bytes moved: ActNorm forward {gbf:.0f} GB/s ({med(tfs):.1f} us) | finc_mix {gbm:.0f} GB/s ({med(tms):.1f} us), two tensors each | "
              f"ratio {gbf / gbm:.2f}", flush=True)
        r["forward_GBps"], r["finc_mix_GBps"] = gbf, gbm
    del x, y, gy
# the flow step users train (trace mode only)
if not only_flowstep:
    if len(sys.argv) > 2 and sys.argv[1] == "json":
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump(results, f, indent=1)
    sys.exit(0)
import numpy as np
from fincflow_amd import FastFlowUnit, FlowSequential, glow
from fincflow_amd.layers import StandardNormal
B, C, H, W = 256, 96, 64, 64
torch.manual_seed(4); np.random.seed(4)
an = glow.ActNorm(C)
seq = FlowSequential(StandardNormal((C, H, W)), FastFlowUnit(C, C, 3), an, glow.Conv1x1(C)).to(dev)
with torch.no_grad():
    an.log_scale.copy_(0.2 * torch.randn(C, device=dev)); an.translation.copy_(torch.randn(C, device=dev)); an.mark_initialized()
x = torch.randn(B, C, H, W, device=dev)
for _ in range(5):
    seq.zero_grad(set_to_none=True)
    seq.log_prob(x).mean().backward()
torch.cuda.synchronize()
