"""GPU helper: what bf16 autocast costs and saves around the coupling, HIP events, the legs of a comparison alternated in
this one process, 7 rounds, medians and spread.  At [256, 96, 64, 64]:
  (a) every finc_coupling_*_rawbf16_f32 entry point (through its ops wrapper) against its _f32 sibling on the same values;
  (b) the same against that sibling WITH the casts the bf16 entry point makes unnecessary: raw.float() in front, and
      grad_raw.bfloat16() behind a backward;
  (c) ops.finc_bias_relu on bf16 against fp32 at [256, 512, 64, 64], in place;
  (d) one training step (forward, backward; no optimiser) and one sample(256) of [FastFlowUnit, ActNorm, Conv1x1, Coupling] x 4 in fp32
      and under torch.autocast(device_type="cuda", dtype=torch.bfloat16) -- both legs are THIS build (the fp32 leg is what the package
      ran before it could run under autocast at all).
`time_autocast.py json PATH` also writes the figures; `time_autocast.py ... small` shrinks every shape (a dry run of the script)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fincflow_amd import FastFlowUnit, glow, ops
from fincflow_amd.layers import FlowSequential
dev = torch.device("cuda:0")
small = "small" in sys.argv
med = statistics.median
def timeit(fn, n, warm_s=0.3):
    t_end = time.perf_counter() + warm_s         # clocks ramp up over the first tenths of a second of load
    while True:
        fn(); torch.cuda.synchronize()
        if time.perf_counter() >= t_end: break
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3
def legs(name, fns, n, out, unit="us", warm_s=0.3):
    """`fns`: {leg: callable}, timed alternately for 7 rounds.  Prints and keeps every round; returns the medians."""
    t = {k: [] for k in fns}
    for _ in range(7):
        for k, fn in fns.items(): t[k].append(timeit(fn, n, warm_s))
    scale = 1e-3 if unit == "ms" else 1.0
    spread = lambda v: (max(v) - min(v)) / med(v) * 100
    print(f"  {name}: " + " | ".join(f"{k} {med(v) * scale:.1f} {unit} (min {min(v) * scale:.1f} max {max(v) * scale:.1f}, spread {spread(v):.1f} %)"
                                     for k, v in t.items()), flush=True)
    out[name] = {k: {"us": v, "median_us": med(v), "spread_pct": spread(v)} for k, v in t.items()}
    return {k: med(v) for k, v in t.items()}
def verdict(name, m, t, out):
    """bf16 against its sibling (a) and against sibling + casts (b): the ratio of the medians, and whether the difference exceeds the
    sibling's own run-to-run spread (max - min over its 7 rounds)."""
    sib = t[name]["fp32"]["us"]
    noise = max(sib) - min(sib)
    a, b = m["fp32"] / m["bf16"], m["fp32+casts"] / m["bf16"]
    slower = m["bf16"] - m["fp32"] > noise
    print(f"    (a) fp32 / bf16 {a:.2f}{'  SLOWER than the sibling by more than its spread' if slower else ''}   (b) (fp32 + casts) / bf16 {b:.2f}", flush=True)
    out[name]["fp32_over_bf16"], out[name]["fp32_casts_over_bf16"], out[name]["bf16_slower_than_sibling_beyond_its_spread"] = a, b, slower
results = {}
B, C, H, W = (8, 96, 16, 16) if small else (256, 96, 64, 64)
torch.manual_seed(C)
x = torch.randn(B, C, H, W, device=dev); raw16 = (1.5 * torch.randn(B, C, H, W, device=dev)).bfloat16(); raw32 = raw16.float()
a = torch.exp(0.3 * torch.randn(C, device=dev)); b = 0.3 * torch.randn(C, device=dev) * a
gy = torch.randn(B, C, H, W, device=dev); gl = torch.randn(B, device=dev); y = torch.empty_like(x)
n = 20
print(f"(a), (b) B{B} C{C} {H}x{W}:", flush=True)
r = results[f"{B}x{C}x{H}x{W}"] = {}
with torch.no_grad():
    yf = ops.finc_coupling(x, raw16, a, b, 1, True)[0]; yr = ops.finc_coupling(x, raw16, a, b, -1)[0]
    transforms = {
        "forward + logdet": lambda raw: ops.finc_coupling(x, raw, a, b, 1, True, out=y),
        "reverse": lambda raw: ops.finc_coupling(x, raw, a, b, -1, False, out=y),
        "reverse + logdet": lambda raw: ops.finc_coupling_reverse_logdet(x, raw, a, b, out=y)}
    backwards = {
        "backward": lambda raw: ops.finc_coupling_backward(gy, gl, x, raw, a, b),
        "reverse backward": lambda raw: ops.finc_coupling_reverse_backward(gy, yr, raw, a, b),
        "reverse + logdet backward": lambda raw: ops.finc_coupling_reverse_logdet_backward(gy, gl, yr, raw, a, b),
        "backward + reconstruct": lambda raw: ops.finc_coupling_backward_reconstruct(gy, gl, yf, raw, a, b)}
    for name, fn in transforms.items():
        m = legs(name, {"bf16": lambda: fn(raw16), "fp32": lambda: fn(raw32), "fp32+casts": lambda: fn(raw16.float())}, n, r)
        verdict(name, m, r, r)
    for name, fn in backwards.items():
        m = legs(name, {"bf16": lambda: fn(raw16), "fp32": lambda: fn(raw32), "fp32+casts": lambda: fn(raw16.float())[-3].bfloat16()}, n, r)
        verdict(name, m, r, r)
    del yf, yr, y, gy, raw32
    Bc, Cc = (8, 512) if small else (256, 512)
    print(f"(c) B{Bc} C{Cc} {H}x{W}:", flush=True)
    r = results[f"{Bc}x{Cc}x{H}x{W}"] = {}
    h16 = torch.randn(Bc, Cc, H, W, device=dev).bfloat16(); bias = 0.3 * torch.randn(Cc, device=dev)
    m = legs("bias + ReLU in place", {"bf16": lambda: ops.finc_bias_relu(h16, bias, out=h16)}, n, r)
    del h16
    h32 = torch.randn(Bc, Cc, H, W, device=dev)
    m.update(legs("bias + ReLU in place (fp32)", {"fp32": lambda: ops.finc_bias_relu(h32, bias, out=h32)}, n, r))
    r["fp32_over_bf16"] = m["fp32"] / m["bf16"]
    print(f"    fp32 / bf16 {r['fp32_over_bf16']:.2f}  (read + written: {4 * Bc * Cc * H * W / 1e9:.2f} GB at {4 * Bc * Cc * H * W / m['bf16'] / 1e3:.0f} GB/s in bf16, "
          f"{8 * Bc * Cc * H * W / 1e9:.2f} GB at {8 * Bc * Cc * H * W / m['fp32'] / 1e3:.0f} GB/s in fp32)", flush=True)
    r["bf16_GBps"], r["fp32_GBps"] = 4 * Bc * Cc * H * W / m["bf16"] / 1e3, 8 * Bc * Cc * H * W / m["fp32"] / 1e3
    del h32
# (d) the flagship stack
width = 32 if small else 512
print(f"(d) [FastFlowUnit, ActNorm, Conv1x1, Coupling] x 4 at B{B} C{C} {H}x{W}, coupling width {width}:", flush=True)
r = results["stack"] = {}
torch.manual_seed(0)
layers = []
for _ in range(4):
    layers += [FastFlowUnit(C, C, (3, 3)), glow.ActNorm(C), glow.Conv1x1(C), glow.Coupling((C, H, W), width=width)]
model = FlowSequential(glow.GaussianPrior((C, H, W)), *layers).to(dev)
with torch.no_grad():
    for mod in model.modules():
        if isinstance(mod, glow.Conv2dZero):
            for p in (mod.weight, mod.bias, mod.logs): p.copy_(0.02 * torch.randn_like(p))
    model.log_prob(x)                            # ActNorm's data-dependent initialisation
def train_step(cast):
    model.zero_grad(set_to_none=True)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=cast):
        loss = -model.log_prob(x).mean()
    loss.backward()
def sample(cast):
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=cast):
        model.sample(B)
m = legs("training step", {"fp32": lambda: train_step(False), "autocast": lambda: train_step(True)}, 3, r, "ms", warm_s=1.0)
r["training step"]["fp32_over_autocast"] = m["fp32"] / m["autocast"]
print(f"    fp32 / autocast {m['fp32'] / m['autocast']:.2f} (both legs are this build)", flush=True)
m = legs("sample", {"fp32": lambda: sample(False), "autocast": lambda: sample(True)}, 3, r, "ms", warm_s=1.0)
r["sample"]["fp32_over_autocast"] = m["fp32"] / m["autocast"]
print(f"    fp32 / autocast {m['fp32'] / m['autocast']:.2f} (both legs are this build)", flush=True)
if len(sys.argv) > 2 and sys.argv[1] == "json":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(results, f, indent=1)
