"""GPU helper: what float64 costs on the banks of 29 .. 64 channels, in this one process by HIP events.  Per shape the
five legs -- inverse, forward, grad_x, grad_w, the whole backward -- on the M-split matrix-core kernels, alternated with the path the
commit before these kernels took for the same call: `algo="strict"` (the reference-order kernels) for the inverse and the forward,
finc_backward_f64 with a NULL workspace (the templated direct kernels) for the backward.  Seven rounds each, medians and the spread of
the rounds.  c3 ([256, 96, 64, 64], Cq = 24) runs on the one-wave kernels as the yardstick.

Beside each matrix-core time: the fraction of the fp64 MFMA peak (1,024 SIMDs x one v_mfma_f64_16x16x4_f64 of 2,048 flops per 64
cycles at CLOCK_MHZ, the MFMAs the kernel issues counted, padded channels included) and the ratio to the MFMA-count model: the waves
of a launch in rounds of 1,024 (one per SIMD), each wave its MFMAs back to back.

    time_f64_wide_banks.py [OUT_DIR] [--old-paths-only]
writes OUT_DIR/time.{txt,json} (default profiles/f64_wide_banks).  --old-paths-only times the strict / NULL-workspace legs alone and
writes OUT_DIR/time_old_paths.{txt,json}: run from a checkout of the commit before, it shows whether those legs cost the same there.
Not measured: hardware counters, and shapes other than these.
"""
import json, os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from fincflow_amd import _lib, ops
dev = torch.device("cuda:0")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
old_only = "--old-paths-only" in sys.argv
out_dir = args[0] if args else os.path.join(REPO, "profiles", "f64_wide_banks")
med = statistics.median
CLOCK_MHZ = 2400.0
SIMDS = 1024
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
def spread(v):
    return (max(v) - min(v)) / med(v) * 100

def mfma_model(leg, B, G, Cq, H, W, K, family):
    """(MFMAs of the launch, model microseconds): waves in rounds of SIMDS, a wave's MFMAs back to back at 64 cycles each."""
    cqp = (Cq + 3) // 4 * 4 if family == 1 else 32 if Cq <= 32 else 48 if Cq <= 48 else 64
    NK, MT, taps, nprob = cqp // 4, (cqp + 15) // 16, K * K, B * G
    split = MT if family == 2 else 1
    tiles = MT // split                                  # row tiles a wave accumulates
    if leg == "inverse":
        P = min(W, 16)
        steps = (H + P - 1) // P * W + P - 1
        per_wave, waves = steps * taps * NK * tiles, nprob * split       # (the z-term's triangle counted as a full tap)
    elif leg in ("forward", "grad_x"):
        per_wave, waves = H * taps * NK * tiles, nprob * split * ((W + 15) // 16)
    else:
        per_wave, waves = H * ((W + 3) // 4) * taps * MT * tiles, nprob * split
    return per_wave * waves, max(1.0, waves / SIMDS) * per_wave * 64 / CLOCK_MHZ

results = {}
G, K, orient = 4, 3, ops.ORIENT_FASTFLOW
SHAPES = (("cq48", (256, 192, 32, 32)), ("cq64", (128, 256, 32, 32)), ("cq32", (256, 128, 64, 64)), ("c3_yardstick", (256, 96, 64, 64)))
for tag, (B, C, H, W) in SHAPES:
    Cq = C // G
    torch.manual_seed(0)
    w = 0.05 * min(1.0, (24.0 / Cq) ** 0.5) * torch.randn(C, Cq, K, K, dtype=torch.float64)
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
    family = 0 if old_only else _lib.f64_plan(*dims)["family"]
    def unit(name, algo):
        if algo == "strict":
            ops._call(name, dev, x.data_ptr(), wc.data_ptr(), z.data_ptr(), *dims, orient, ops._stream_ptr(x))
        else:
            ops._call(name + "_algo", dev, x.data_ptr(), wc.data_ptr(), z.data_ptr(), *dims, orient, _lib.ALGO[algo], *ops._ws_args(dev, ws_f),
                      ops._stream_ptr(x))
    def backward(want_gx, want_gw, workspace=True):
        ops._call("finc_backward_f64", dev, gz.data_ptr(), x.data_ptr(), wc.data_ptr(), gx.data_ptr() if want_gx else None,
                  gw.data_ptr() if want_gw else None, *dims, orient, *(ops._ws_args(dev, ws_b) if workspace else (None, 0)), ops._stream_ptr(x))
    new = {"inverse": lambda: unit("finc_inverse_f64", "mfma"), "forward": lambda: unit("finc_forward_f64", "mfma"),
           "grad_x": lambda: backward(True, False), "grad_w": lambda: backward(False, True), "whole backward": lambda: backward(True, True)}
    old = {"inverse": lambda: unit("finc_inverse_f64", "strict"), "forward": lambda: unit("finc_forward_f64", "strict"),
           "grad_x": lambda: backward(True, False, False), "grad_w": lambda: backward(False, True, False),
           "whole backward": lambda: backward(True, True, False)}
    say(f"{tag}: B{B} C{C} {H}x{W} k{K} G{G} (Cq {Cq}) float64, family {family}, backward workspace {ws_b / 2**20:.1f} MiB")
    got_new, got_old = {k: [] for k in new}, {k: [] for k in old}
    for _ in range(7):                               # alternately, so that clocks and neighbours on the box hit every leg alike
        for k in new:
            if not old_only: got_new[k].append(timeit(new[k], 5))
            if tag != "c3_yardstick": got_old[k].append(timeit(old[k], 1, warm=0.0))
    entry = {"shape": [B, C, H, W, K, G], "family": family, "legs_us": got_new, "old_path_legs_us": got_old, "derived": {}}
    for k in new:
        s = f"  {k}:"
        if got_new[k]:
            mfmas, model_us = mfma_model(k if k != "whole backward" else "grad_x", B, G, Cq, H, W, K, family)
            if k == "whole backward":
                m2, u2 = mfma_model("grad_w", B, G, Cq, H, W, K, family)
                mfmas, model_us = mfmas + m2, model_us + u2
            t_us = med(got_new[k])
            peak = mfmas * 2048 / (t_us * 1e-6) / (SIMDS * 2048 / 64 * CLOCK_MHZ * 1e6)
            s += f" {t_us:.1f} us (spread {spread(got_new[k]):.1f} %), {peak * 100:.1f} % of the fp64 MFMA peak, {t_us / model_us:.2f} x the MFMA-count model"
            entry["derived"][k] = {"median_us": t_us, "spread_pct": spread(got_new[k]), "peak_fraction": peak, "over_model": t_us / model_us}
        if got_old[k]:
            o = got_old[k]
            s += f" | the path before: {med(o):.1f} us (min {min(o):.1f} max {max(o):.1f}, spread {spread(o):.1f} %)"
            if got_new[k]:
                faster = max(got_new[k]) < min(o)
                s += f", {med(o) / med(got_new[k]):.1f} x; slowest new round {'<' if faster else '>='} fastest old round"
                entry["derived"][k].update(old_median_us=med(o), old_spread_pct=spread(o), speedup=med(o) / med(got_new[k]), faster_beyond_spread=faster)
        say(s)
    results[tag] = entry
    del x, gz, z, gx
    ops.release_workspaces()
    torch.cuda.empty_cache()
_lib.raise_if_faulted("time_f64_wide_banks")
os.makedirs(out_dir, exist_ok=True)
stem = "time_old_paths" if old_only else "time"
with open(os.path.join(out_dir, stem + ".json"), "w") as f:
    json.dump(results, f, indent=1)
with open(os.path.join(out_dir, stem + ".txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
