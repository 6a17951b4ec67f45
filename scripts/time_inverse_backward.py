"""GPU helper: what the backward through the unit's inverse costs, part by part, in this one process by HIP events:
the plain inverse, the adjoint solve (the same kernel on the adjoint bank, orientation complemented), the lead product, the
grad-weight (finc_backward_f32 without grad_x, its sign, canonical -> stored), and the whole backward as autograd runs it
(`PackedWeights.inverse_backward` + the canonicalise).  Legs are timed alternately, 7 rounds each: medians and the spread of the
rounds.  The adjoint solve is also timed against the plain bank ON THE SAME DATA (the upstream gradient): the chip's clock under load
depends on the data, so a difference between "plain inverse on z" and "adjoint solve on grad_x" is first a difference of data.
There is no earlier implementation: no ratio is a speed-up.  The grouped lead kernel (channel counts without a finc_mix
instantiation) is timed at 80 channels on the same map, for the record.

    time_inverse_backward.py [OUT_DIR [B C H W K]]     writes OUT_DIR/time_inverse_backward.{txt,json} (default profiles/inverse_backward)
"""
import json, os, statistics, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from fincflow_amd import FastFlowUnit, _lib, ops
dev = torch.device("cuda:0")
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "inverse_backward")
B, C, H, W, K = (int(a) for a in sys.argv[2:7]) if len(sys.argv) > 6 else (256, 96, 64, 64, 3)
G = 4
med = statistics.median
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
def timeit(fn, n):
    t_end = time.perf_counter() + 0.3        # clocks ramp up over the first tenths of a second of load
    while time.perf_counter() < t_end:
        for _ in range(3): fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3
def rounds(legs, n, reps=7):
    got = {k: [] for k in legs}
    for _ in range(reps):                        # alternately, so that clocks and neighbours on the box hit every leg alike
        for k, fn in legs.items(): got[k].append(timeit(fn, n))
    return got
def show(name, v):
    say(f"  {name}: {med(v):.1f} us (min {min(v):.1f} max {max(v):.1f}, spread {(max(v) - min(v)) / med(v) * 100:.1f} %)")

torch.manual_seed(0)
unit = FastFlowUnit(C, C, K).to(dev)
cache, bank_args = unit._cache, unit._cache_args()
Cq = C // G
x0 = torch.randn(B, C, H, W, device=dev)
with torch.no_grad():
    z = unit(x0)[0].contiguous()
    x = cache.inverse(z, *bank_args)
gx = torch.randn(B, C, H, W, device=dev)
bank = cache._get(*bank_args)
dims = (B, Cq, H, W, K, K)
ops.PackedWeights.inverse_backward(bank, gx, x, G, bank_args[2])                 # builds the adjoint bank and its fragments
w_adj, lead_t = bank.adjoint
adj_orient = bank_args[2] ^ ((1 << (2 * G)) - 1)
packed_inv, packed_adj = bank.packed["inv"][1], bank.packed["inv_adjoint"][1]
out = torch.empty_like(gx)
y = gx.clone()
ws_bytes = _lib.lib().finc_backward_workspace_bytes(B, G, Cq, H, W, K, K)
gw = torch.empty_like(bank.w_canon)
# The lead product works in place: timed over and over on one buffer it would raise a unit triangular matrix to the power of the call
# count.  Calls alternate between the matrix and its inverse (unit upper triangular as well: the same kernel, the same cost).
lead_back = torch.linalg.inv(lead_t.double()).float().contiguous()
turn = [0]
def lead_in_place(v, mats, groups, cq):
    turn[0] ^= 1
    ops._call("finc_lead_product_f32", dev, v.data_ptr(), mats[turn[0]].data_ptr(), v.shape[0], groups, cq, H * W, ops._stream_ptr(v))
def gradw():
    ops._call("finc_backward_f32", dev, y.data_ptr(), x.data_ptr(), bank.w_canon.data_ptr(), None, gw.data_ptr(), B, G, Cq, H, W, K, K,
              bank_args[2], *ops._ws_args(dev, ws_bytes), ops._stream_ptr(y))
    ops._call("finc_negate_f32", dev, gw.data_ptr(), gw.numel(), ops._stream_ptr(y))
    return ops.canonicalize(gw, G, bank_args[2])
def whole():
    gz, g = ops.PackedWeights.inverse_backward(bank, gx, x, G, bank_args[2])
    return gz, ops.canonicalize(g, G, bank_args[2])
legs = {
    "plain inverse (on z)": lambda: ops._launch_packed("finc_inverse_packed_f32", z, packed_inv, out, G, dims, bank_args[2]),
    "plain inverse (on grad_x)": lambda: ops._launch_packed("finc_inverse_packed_f32", gx, packed_inv, out, G, dims, bank_args[2]),
    "adjoint solve (on grad_x)": lambda: ops._launch_packed("finc_inverse_packed_f32", gx, packed_adj, out, G, dims, adj_orient),
    "lead product": lambda: lead_in_place(y, (lead_t, lead_back), G, Cq),
    "grad-weight": gradw,
    "whole backward": whole,
}
v = _lib.inverse_variant(B, G, Cq, H, W, K, K)
say(f"B{B} C{C} {H}x{W} k{K} G{G}: inverse kernel {v}, grad-weight form {_lib.backward_variant(B, G, Cq, H, W, K, K)['gradw']}, "
    f"lead product on {'finc_mix' if ops.mix_supported(C) else 'the grouped kernel'}")
with torch.no_grad():
    got = rounds(legs, 10 if x.numel() > (1 << 24) else 100)
for k, t in got.items(): show(k, t)
parts = med(got["adjoint solve (on grad_x)"]) + med(got["lead product"]) + med(got["grad-weight"])
say(f"  whole backward {med(got['whole backward']):.1f} us beside the sum of its parts {parts:.1f} us (solve + lead product + grad-weight)")
p, a, d = got["plain inverse (on z)"], got["adjoint solve (on grad_x)"], got["plain inverse (on grad_x)"]
say(f"  adjoint solve - plain inverse on z: {med(a) - med(p):+.1f} us; the plain inverse's own run-to-run spread {max(p) - min(p):.1f} us; "
    f"adjoint solve - plain inverse on the same data: {med(a) - med(d):+.1f} us (spread there {max(d) - min(d):.1f} us)")
results = {"shape": [B, C, H, W, K, G], "inverse_variant": v, "legs_us": got, "whole_us": med(got["whole backward"]), "sum_of_parts_us": parts}

# the grouped lead kernel, for the record (no bar): a channel count finc_mix has no instantiation for, same map
Cg = 80
assert not ops.mix_supported(Cg)
Bg = max(1, B // 4)
torch.manual_seed(1)
lt = torch.block_diag(*[torch.triu(0.05 * torch.randn(Cg // G, Cg // G), 1) + torch.eye(Cg // G) for _ in range(G)]).to(dev).contiguous()
vg = torch.randn(Bg, Cg, H, W, device=dev)
lt_back = torch.triu(torch.linalg.inv(lt.double())).float().contiguous()
g_legs = {"grouped lead product": lambda: lead_in_place(vg, (lt, lt_back), G, Cg // G)}
with torch.no_grad():
    gg = rounds(g_legs, 10, reps=5)["grouped lead product"]
say(f"B{Bg} C{Cg} {H}x{W} G{G} (no finc_mix instantiation):")
show("grouped lead product", gg)
say(f"  {8 * vg.numel() / med(gg) / 1e3:.0f} GB/s of the two tensor passes a streaming kernel would make")
results["grouped_lead"] = {"shape": [Bg, Cg, H, W, G], "us": gg}
_lib.raise_if_faulted("time_inverse_backward")
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "time_inverse_backward.json"), "w") as f:
    json.dump(results, f, indent=1)
with open(os.path.join(out_dir, "time_inverse_backward.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
