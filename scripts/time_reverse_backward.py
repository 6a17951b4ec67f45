"""GPU helper: `reverse` + its backward of glow.Coupling, ActNorm and Conv1x1 inside `reverse_grad()` (HIP: ops.coupling_reverse,
ops.actnorm_reverse, ops.mix_forward on W^-1) against the same module outside the context (the PyTorch lines, unchanged), alternately
in this one process at [256, 96, 64, 64]: medians and spread of 7 rounds per path, HIP events around each leg.  The coupling is timed
twice: the module (its PyTorch net is in both legs) and the transform alone behind a given `raw`.  Then the two new kernels alone
beside their forward-direction siblings, which move the same bytes: microseconds and TB/s of the algorithmic traffic.

    python scripts/time_reverse_backward.py [DIR]                      # writes DIR/time_reverse_backward.{txt,json}
    python scripts/time_reverse_backward.py step OTHER_TREE [json PATH]  # the whole step: rsample(256) + x.square().mean().backward() on
                                                                       # [FastFlowUnit, ActNorm, Conv1x1, Coupling], this tree against
                                                                       # another tree of the project (the parent commit, built side by
                                                                       # side), fresh child processes, runs alternated
    python scripts/time_reverse_backward.py child TREE                   # one run, one JSON line (what the driver starts)
"""
import contextlib, json, os, statistics, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (256, 96, 64, 64)
med = statistics.median
def timeit(torch, fn, n):
    t_end = time.perf_counter() + 0.3        # clocks ramp up over the first tenths of a second of load
    while time.perf_counter() < t_end:
        fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3
def layers(out_dir):
    sys.path.insert(0, HERE)
    import numpy as np, torch
    import fincflow_amd
    from fincflow_amd import glow, ops
    dev = torch.device("cuda:0")
    lines, results = [], {"shape": list(SHAPE)}
    def say(s):
        print(s, flush=True); lines.append(s)
    def ab(name, new_fn, old_fn, n, out, labels=("HIP", "PyTorch")):
        new, old = [], []
        for _ in range(7):                       # alternately, so that clocks and neighbours on the box hit both alike
            new.append(timeit(torch, new_fn, n)); old.append(timeit(torch, old_fn, n))
        gap = min(old) - max(new)                # > 0: every round of the first leg beat every round of the second
        pairs = sum(a < b for a, b in zip(new, old))
        say(f"  {name}: {labels[0]} {med(new):.1f} us (min {min(new):.1f} max {max(new):.1f}) | {labels[1]} {med(old):.1f} us "
            f"(min {min(old):.1f} max {max(old):.1f}) | ratio {med(old) / med(new):.2f} | "
            f"{'the first faster by more than the spread' if gap > 0 else 'NOT separated from the spread'}, {pairs} of {len(new)} adjacent pairs")
        out[name] = {labels[0] + "_us": new, labels[1] + "_us": old, "ratio_of_medians": med(old) / med(new), "separated": gap > 0, "pairs_won": pairs}
        return med(new), med(old)
    B, C, H, W = SHAPE
    torch.manual_seed(4); np.random.seed(4)
    x = torch.randn(SHAPE, device=dev); g = torch.randn(SHAPE, device=dev)
    an = glow.ActNorm(C).to(dev)
    with torch.no_grad():
        an.log_scale.copy_(0.2 * torch.randn(C, device=dev)); an.translation.copy_(torch.randn(C, device=dev))
    an.mark_initialized()
    cp = glow.Coupling((C, H, W)).to(dev)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        last = cp.net[4]
        last.weight.copy_(0.02 * torch.randn(last.weight.shape, generator=gen)); last.bias.copy_(0.01 * torch.randn(last.bias.shape, generator=gen))
        last.logs.copy_(0.01 * torch.randn(last.logs.shape, generator=gen))
    say(f"B{B} C{C} {H}x{W}, reverse + backward of that reverse (input and every parameter require grad):")
    r = results["layers"] = {}
    for name, m, n in (("ActNorm", an, 20), ("Conv1x1", glow.Conv1x1(C).to(dev), 20), ("Coupling (module, PyTorch net in both legs)", cp, 3)):
        xa = x.clone().requires_grad_(True)
        def leg(inside):
            m.zero_grad(set_to_none=True); xa.grad = None
            with (fincflow_amd.reverse_grad() if inside else contextlib.nullcontext()):
                y = m.reverse(xa)
            y.backward(g)
            return y
        assert "Finc" in type(leg(True).grad_fn).__name__ and "Finc" not in type(leg(False).grad_fn).__name__
        ab(name, lambda: leg(True), lambda: leg(False), n, r)
        leg(True); new = [xa.grad.clone()] + [p.grad.clone() for p in m.parameters()]
        leg(False); old = [xa.grad] + [p.grad for p in m.parameters()]
        r[name]["max_rel_diff_of_the_gradients"] = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(new, old))
        say(f"    max rel diff of the gradients, HIP against PyTorch: {r[name]['max_rel_diff_of_the_gradients']:.1e}")
        del xa, new, old
    # the coupling's transform alone: everything behind the net's last convolution, `raw` a leaf
    raw = 1.5 * torch.randn(SHAPE, device=dev); logs = 0.1 * torch.randn(C, device=dev); bias = 0.3 * torch.randn(C, device=dev)
    leaves = [t.clone().requires_grad_(True) for t in (x, raw, logs, bias)]
    def tail(hip):
        for t in leaves: t.grad = None
        xl, rl, ll, bl = leaves
        if hip:
            al = torch.exp(ll * 3)
            y = ops.coupling_reverse(xl, rl, al, bl * al)
        else:
            h = (rl + bl.view(1, -1, 1, 1)) * torch.exp(ll * 3).view(1, -1, 1, 1)
            log_s = 2.0 * torch.tanh(h[:, ::2] / 2.0)
            y = torch.cat([xl[:, :C // 2], (xl[:, C // 2:] - h[:, 1::2]) * torch.exp(-log_s)], dim=1)
        y.backward(g)
    ab("Coupling (transform alone, raw a leaf)", lambda: tail(True), lambda: tail(False), 20, r)
    del leaves
    # the two new kernels beside their forward-direction siblings
    say("kernels alone (all outputs asked for), algorithmic traffic: coupling 4.5 tensors (grad_y, half of y or x, raw read; grad_x, grad_raw "
        "written), ActNorm 3 tensors (grad_y, x or y read; grad_x written):")
    k = results["kernels"] = {}
    ls = an.log_scale.detach(); a = torch.exp(3 * logs); b = bias * a; gl = torch.randn(B, device=dev)
    with torch.no_grad():
        y = ops.finc_coupling(x, raw, a, b, -1)[0]
        yn = ops.finc_actnorm(x, ls, an.translation.detach(), 1)[0]
        cr, cf = ab("coupling backward", lambda: ops.finc_coupling_reverse_backward(g, y, raw, a, b), lambda: ops.finc_coupling_backward(g, gl, x, raw, a, b),
                    20, k, ("reverse direction (new)", "forward direction"))
        ar, af = ab("ActNorm backward", lambda: ops.finc_actnorm_reverse_backward(g, x, ls), lambda: ops.finc_actnorm_backward(g, gl, yn, ls),
                    20, k, ("reverse direction (new)", "forward direction"))
    nbytes = 4 * x.numel()
    for name, tensors, new, old in (("coupling backward", 4.5, cr, cf), ("ActNorm backward", 3, ar, af)):
        k[name]["TBps"] = {"reverse": tensors * nbytes / new / 1e6, "forward": tensors * nbytes / old / 1e6}
        say(f"  {name}: reverse direction {new:.1f} us = {k[name]['TBps']['reverse']:.2f} TB/s | forward direction {old:.1f} us = "
            f"{k[name]['TBps']['forward']:.2f} TB/s | time ratio reverse / forward {new / old:.2f}")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_reverse_backward.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_reverse_backward.json"), "w") as f:
        json.dump(results, f, indent=1)
def child(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np, torch
    import fincflow_amd
    from fincflow_amd import FastFlowUnit, FlowSequential, _lib, glow, ops
    from fincflow_amd.layers import StandardNormal
    assert os.path.abspath(fincflow_amd.__file__).startswith(os.path.abspath(tree) + os.sep), fincflow_amd.__file__
    dev = torch.device("cuda:0")
    B, C, H, W = SHAPE
    torch.manual_seed(4); np.random.seed(4)
    an, cp = glow.ActNorm(C), glow.Coupling((C, H, W))
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        an.log_scale.copy_(0.2 * torch.randn(C, generator=gen)); an.translation.copy_(torch.randn(C, generator=gen)); an.mark_initialized()
        last = cp.net[4]
        last.weight.copy_(0.02 * torch.randn(last.weight.shape, generator=gen)); last.bias.copy_(0.01 * torch.randn(last.bias.shape, generator=gen))
        last.logs.copy_(0.01 * torch.randn(last.logs.shape, generator=gen))
    seq = FlowSequential(StandardNormal((C, H, W)), FastFlowUnit(C, C, 3), an, glow.Conv1x1(C), cp).to(dev)
    def step():
        seq.zero_grad(set_to_none=True)
        x = seq.rsample(B)
        x.square().mean().backward()
        return x
    torch.manual_seed(5)
    x = step(); torch.cuda.synchronize()
    # the same seed, the same z: what the step computes, for the comparison between the trees
    check = {"x_abs_mean": float(x.detach().abs().mean()), "grad_abs_sum": {n: float(p.grad.abs().sum()) for n, p in seq.named_parameters()
                                                                            if n.split(".")[-1] in ("log_scale", "translation", "W", "logs")}}
    fn = x.grad_fn
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:
        step(); torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(3): step()
        b.record(); torch.cuda.synchronize()
        rounds.append(a.elapsed_time(b) / 3)
    print(json.dumps({"ms_per_step": med(rounds), "rounds_ms": rounds, "finc_version": int(_lib.lib().finc_version()),
                      "last_node": type(fn).__name__, "hip_reverse_backward": hasattr(ops, "coupling_reverse"), "check": check,
                      "fault_pending": bool(_lib.fault_pending())}))
def driver(other, path):
    runs = []
    for r in range(1, 5):
        for name, tree in (("parent commit", other), ("this commit", HERE)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", tree], capture_output=True, text=True, timeout=240,
                               env={k: v for k, v in os.environ.items() if k not in ("FINCFLOW_LIB", "PYTHONPATH")})
            if p.returncode != 0:            # nothing more is started on the GPU after a failure
                sys.exit(f"{name} run {r} failed ({p.returncode}): {p.stderr[-800:]}")
            runs.append(dict(build=name, run=r, **json.loads(p.stdout.strip().splitlines()[-1])))
            print(runs[-1], flush=True)
    out = {"what": "rsample(256) + x.square().mean().backward() on [FastFlowUnit(96), ActNorm(96), Conv1x1(96), Coupling((96, 64, 64))]: parent "
                   "commit and this commit built side by side on one MI355X, fresh processes, runs alternated (parent, this, parent, this, ...)",
           "runs": runs}
    for name in ("parent commit", "this commit"):
        v = [q["ms_per_step"] for q in runs if q["build"] == name]
        out[name] = {"median_ms": med(v), "min_ms": min(v), "max_ms": max(v)}
    old, new = ([q["ms_per_step"] for q in runs if q["build"] == n] for n in ("parent commit", "this commit"))
    out["separated"] = max(new) < min(old)
    out["pairs_won"] = sum(a < b for a, b in zip(new, old))
    print(json.dumps({k: out[k] for k in ("parent commit", "this commit", "separated", "pairs_won")}), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "child":
        child(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "step":
        driver(sys.argv[2], sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "json" else None)
    else:
        layers(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "reverse_backward"))
