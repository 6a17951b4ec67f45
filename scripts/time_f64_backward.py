"""GPU helper: what the double-precision backward costs, at c3 ([256, 96, 64, 64], 3x3, G = 4) and c2 (C = 48, 32x32,
B = 64), in this one process by HIP events: the fp64 forward (the yardstick: the grad-input is the same kernel on another bank, the
grad-weight issues 9 MT MT MFMAs per four pixels against the forward's 9 NK MT per sixteen), grad_x, grad_w and the whole
finc_backward_f64 on the matrix cores, then the same three on the templated direct kernels (a NULL workspace selects them).  Legs are
timed alternately, 7 rounds each (3 for the direct kernels, which take tens of milliseconds): medians and the spread of the rounds.
There is no earlier fp64 backward: no ratio is a speed-up.

    time_f64_backward.py [OUT_DIR]     writes OUT_DIR/time_f64_backward.{txt,json} (default profiles/f64_backward)
"""
import json, os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from fincflow_amd import _lib, ops
dev = torch.device("cuda:0")
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "f64_backward")
med = statistics.median
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
def timeit(fn, n, warm=0.3):
    t_end = time.perf_counter() + warm       # clocks ramp up over the first tenths of a second of load
    while True:
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end: break
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3
def rounds(legs, n, reps):
    got = {k: [] for k in legs}
    for _ in range(reps):                        # alternately, so that clocks and neighbours on the box hit every leg alike
        for k, fn in legs.items(): got[k].append(timeit(fn, n))
    return got
def show(name, v):
    say(f"  {name}: {med(v):.1f} us (min {min(v):.1f} max {max(v):.1f}, spread {(max(v) - min(v)) / med(v) * 100:.1f} %)")

results = {}
G, K, orient = 4, 3, ops.ORIENT_FASTFLOW
for tag, (B, C, H, W) in (("c3", (256, 96, 64, 64)), ("c2", (64, 48, 32, 32))):
    Cq = C // G
    torch.manual_seed(0)
    w = 0.05 * torch.randn(C, Cq, K, K, dtype=torch.float64)
    for g in range(G):
        blk = w[g * Cq:(g + 1) * Cq, :, -1, -1]
        blk.copy_(torch.tril(blk, -1) + torch.eye(Cq, dtype=torch.float64))
    wc = w.to(dev)
    x = torch.randn(B, C, H, W, dtype=torch.float64, device=dev)
    gz = torch.randn(B, C, H, W, dtype=torch.float64, device=dev)
    z, gx, gw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(wc)
    L = _lib.lib()
    ws_f, ws_b = L.finc_f64_workspace_bytes(G, Cq, K, K), L.finc_backward_f64_workspace_bytes(B, G, Cq, H, W, K, K)
    dims = (B, G, Cq, H, W, K, K)
    def forward():
        ops._call("finc_forward_f64_algo", dev, x.data_ptr(), wc.data_ptr(), z.data_ptr(), *dims, orient, _lib.ALGO["mfma"],
                  *ops._ws_args(dev, ws_f), ops._stream_ptr(x))
    def backward(want_gx, want_gw, workspace=True):
        ops._call("finc_backward_f64", dev, gz.data_ptr(), x.data_ptr(), wc.data_ptr(), gx.data_ptr() if want_gx else None,
                  gw.data_ptr() if want_gw else None, *dims, orient, *(ops._ws_args(dev, ws_b) if workspace else (None, 0)), ops._stream_ptr(x))
    say(f"{tag}: B{B} C{C} {H}x{W} k{K} G{G} float64, backward workspace {ws_b / 2**20:.1f} MiB")
    legs = {"fp64 forward": forward, "grad_x": lambda: backward(True, False), "grad_w": lambda: backward(False, True),
            "whole backward": lambda: backward(True, True)}
    got = rounds(legs, 10 if tag == "c3" else 50, 7)
    for k, t in got.items(): show(k, t)
    f, a, b = got["fp64 forward"], got["grad_x"], got["grad_w"]
    say(f"  grad_x - forward: {med(a) - med(f):+.1f} us (the forward's own run-to-run spread {max(f) - min(f):.1f} us); "
        f"grad_w / forward: {med(b) / med(f):.2f} (MFMA issues per sixteen pixels: {9 * ((Cq + 15) // 16) ** 2 * 4} against "
        f"{9 * ((Cq + 3) // 4) * ((Cq + 15) // 16)})")
    plain = {"direct grad_x": lambda: backward(True, False, False), "direct grad_w": lambda: backward(False, True, False),
             "direct whole backward": lambda: backward(True, True, False)}
    got_plain = rounds(plain, 1, 3)
    for k, t in got_plain.items(): show(k, t)
    results[tag] = {"shape": [B, C, H, W, K, G], "workspace_bytes": ws_b, "legs_us": got, "direct_legs_us": got_plain,
                    "gradw_over_forward": med(b) / med(f), "gradx_minus_forward_us": med(a) - med(f)}
    del x, gz, z, gx
    ops.release_workspaces()
    torch.cuda.empty_cache()
_lib.raise_if_faulted("time_f64_backward")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_f64_backward.json"), "w") as f:
    json.dump(results, f, indent=1)
with open(os.path.join(out_dir, "time_f64_backward.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
