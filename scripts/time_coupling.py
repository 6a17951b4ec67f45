"""GPU helper: the coupling kernels (ops.finc_coupling, ops.coupling_forward, ops.finc_bias_relu) against the PyTorch formula they
replace (layers/coupling.py:38-40, 79-101: everything behind the coupling net's last convolution), alternately in this one process:
medians and spread of 7 rounds per path.  Shapes: the three levels of the c4 stack, one chip-filling map, and the 512-wide
activation of the c4 coupling nets for bias + ReLU.  Also the bytes per second of the forward transform (x and raw read, y written)
beside ops.finc_mix (one tensor read, one written) at the chip-filling shape.  `time_coupling.py json PATH` also writes the figures."""
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
def torch_tail(x, raw, logs, bias, direction):
    half = x.shape[1] // 2
    h = (raw + bias.view(1, -1, 1, 1)) * torch.exp(logs * 3).view(1, -1, 1, 1)
    log_s = 2.0 * torch.tanh(h[:, ::2] / 2.0)
    t = h[:, 1::2]
    x1, x2 = x[:, :half], x[:, half:]
    if direction > 0:
        return torch.cat([x1, x2 * torch.exp(log_s) + t], dim=1), log_s.flatten(start_dim=1).sum(-1)
    return torch.cat([x1, (x2 - t) * torch.exp(-log_s)], dim=1)
results = {}
for (B, C, H, W) in ((128, 12, 16, 16), (128, 24, 8, 8), (128, 48, 4, 4), (256, 96, 64, 64)):
    torch.manual_seed(C)
    x = torch.randn(B, C, H, W, device=dev); raw = 1.5 * torch.randn(B, C, H, W, device=dev)
    logs = 0.1 * torch.randn(C, device=dev); bias = 0.3 * torch.randn(C, device=dev)
    gy = torch.randn(B, C, H, W, device=dev); gl = torch.randn(B, device=dev)
    a = torch.exp(3 * logs); b = bias * a; y = torch.empty_like(x)
    n = 20 if x.numel() > (1 << 24) else 200     # the small maps are bound by the host's launches: long legs, or its jitter is the result
    print(f"B{B} C{C} {H}x{W}:", flush=True)
    r = results[f"{B}x{C}x{H}x{W}"] = {}
    with torch.no_grad():
        tf = ab("transform forward + logdet", lambda: ops.finc_coupling(x, raw, a, b, 1, True, out=y), lambda: torch_tail(x, raw, logs, bias, 1), n, r)
        ab("transform reverse", lambda: ops.finc_coupling(x, raw, a, b, -1, False, out=y), lambda: torch_tail(x, raw, logs, bias, -1), n, r)
    leaves = [t.clone().requires_grad_(True) for t in (x, raw, logs, bias)]
    def step(hip):
        for t in leaves: t.grad = None
        xl, rl, ll, bl = leaves
        if hip:
            al = torch.exp(ll * 3)
            yy, ld = ops.coupling_forward(xl, rl, al, bl * al)
        else:
            yy, ld = torch_tail(xl, rl, ll, bl, 1)
        torch.autograd.backward([yy, ld], [gy, gl])
    ab("forward + backward", lambda: step(True), lambda: step(False), n, r)
    step(True); g_new = [t.grad.clone() for t in leaves]
    step(False)
    r["max_rel_diff_of_the_gradients"] = max(float((g - t.grad).abs().max() / t.grad.abs().max()) for g, t in zip(g_new, leaves))
    print(f"  max rel diff of the gradients, HIP against PyTorch: {r['max_rel_diff_of_the_gradients']:.1e}", flush=True)
    del leaves, g_new
    if ops.mix_supported(C) and x.numel() > (1 << 24):
        M = torch.randn(C, C, device=dev) / C ** 0.5
        with torch.no_grad():
            tfs, tms = [], []
            for _ in range(5):
                tfs.append(timeit(lambda: ops.finc_coupling(x, raw, a, b, 1, True, out=y), n)); tms.append(timeit(lambda: ops.finc_mix(x, M, out=y), n))
        gbf, gbm = 12 * x.numel() / med(tfs) / 1e3, 8 * x.numel() / med(tms) / 1e3
        print(f"  bytes moved: forward transform {gbf:.0f} GB/s ({med(tfs):.1f} us, three tensors) | finc_mix {gbm:.0f} GB/s ({med(tms):.1f} us, two tensors) | "
              f"ratio {gbf / gbm:.2f}", flush=True)
        r["forward_GBps"], r["finc_mix_GBps"] = gbf, gbm
B, C, H, W = 128, 512, 16, 16
x = torch.randn(B, C, H, W, device=dev); bias = 0.3 * torch.randn(C, device=dev); buf = x.clone()
print(f"B{B} C{C} {H}x{W}:", flush=True)
r = results[f"{B}x{C}x{H}x{W}"] = {}
with torch.no_grad():
    ab("bias + ReLU", lambda: ops.finc_bias_relu(x, bias, out=buf), lambda: torch.relu(x + bias.view(1, -1, 1, 1)), 50, r)
if len(sys.argv) > 2 and sys.argv[1] == "json":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(results, f, indent=1)
