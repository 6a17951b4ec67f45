"""GPU helper: what the log-density of a sample costs, HIP events, legs alternated, at [256, 96, 64, 64].

    python scripts/time_sample_log_prob.py [DIR]        # the kernel pairs, in this one process, 7 rounds each, alternated: writes
                                                        # DIR/time_sample_log_prob.{txt,json}
                                                        #   finc_coupling_reverse_logdet beside finc_coupling direction -1
                                                        #   finc_coupling_reverse_logdet_backward (with grad_logdet) beside
                                                        #   finc_coupling_reverse_backward
                                                        #   and, for scale, the forward direction with and without its log-det (the
                                                        #   partials + the reduce launch)
    python scripts/time_sample_log_prob.py step OTHER_TREE [json PATH]
                                                        # the model: [FastFlowUnit, ActNorm, Conv1x1, Coupling], fresh child processes,
                                                        # runs alternated: OTHER_TREE (the parent commit, built side by side) on the only
                                                        # way it has -- x = rsample(256); log_q = log_prob(x) -- this tree on the same two
                                                        # passes, and this tree on rsample_with_log_prob(256); each with the backward of
                                                        # (log_q - |x|^2).mean(), and without a graph (sample + log_prob against
                                                        # sample_with_log_prob)
    python scripts/time_sample_log_prob.py child TREE WAY   # one run, one JSON line (WAY: two_pass | one_pass)
"""
import json, os, statistics, subprocess, sys, time
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
def kernels(out_dir):
    sys.path.insert(0, HERE)
    import torch
    from fincflow_amd import ops
    dev = torch.device("cuda:0")
    lines, results = [], {"shape": list(SHAPE)}
    def say(s):
        print(s, flush=True); lines.append(s)
    def ab(name, new_fn, old_fn, labels, n=20):
        new, old = [], []
        for _ in range(7):                       # alternately, so that clocks and neighbours on the box hit both alike
            new.append(timeit(torch, new_fn, n)); old.append(timeit(torch, old_fn, n))
        spread = max(old) - min(old)
        say(f"  {name}: {labels[0]} {med(new):.1f} us (min {min(new):.1f} max {max(new):.1f}) | {labels[1]} {med(old):.1f} us "
            f"(min {min(old):.1f} max {max(old):.1f}) | ratio {med(new) / med(old):.3f} | difference of the medians {med(new) - med(old):+.1f} us, "
            f"the sibling's own spread {spread:.1f} us")
        results[name] = {labels[0] + "_us": new, labels[1] + "_us": old, "ratio_of_medians": med(new) / med(old),
                         "difference_us": med(new) - med(old), "sibling_spread_us": spread}
        return med(new), med(old)
    B, C, H, W = SHAPE
    torch.manual_seed(4)
    x = torch.randn(SHAPE, device=dev); g = torch.randn(SHAPE, device=dev); raw = 1.5 * torch.randn(SHAPE, device=dev)
    a = torch.exp(0.3 * torch.randn(C, device=dev)); b = 0.3 * torch.randn(C, device=dev) * a; gl = torch.randn(B, device=dev)
    out = torch.empty_like(x)
    say(f"B{B} C{C} {H}x{W}, kernels alone, 7 rounds of 20 launches each, alternated:")
    with torch.no_grad():
        y = ops.finc_coupling(x, raw, a, b, -1)[0]
        assert torch.equal(ops.finc_coupling_reverse_logdet(x, raw, a, b)[0], y)
        rn, ro = ab("reverse", lambda: ops.finc_coupling_reverse_logdet(x, raw, a, b, out=out), lambda: ops.finc_coupling(x, raw, a, b, -1, out=out),
                    ("with log-det (new, 2 launches)", "without (1 launch)"))
        fn_, fo = ab("forward (for scale)", lambda: ops.finc_coupling(x, raw, a, b, 1, True, out=out), lambda: ops.finc_coupling(x, raw, a, b, 1, False, out=out),
                     ("with log-det (2 launches)", "without (1 launch)"))
        bn, bo = ab("reverse backward", lambda: ops.finc_coupling_reverse_logdet_backward(g, gl, y, raw, a, b),
                    lambda: ops.finc_coupling_reverse_backward(g, y, raw, a, b), ("with grad_logdet (new)", "without"))
    nbytes = 4 * x.numel()
    results["TBps"] = {"reverse_with_logdet": 3 * nbytes / rn / 1e6, "reverse": 3 * nbytes / ro / 1e6,
                       "backward_with_grad_logdet": 4.5 * nbytes / bn / 1e6, "backward": 4.5 * nbytes / bo / 1e6}
    say("  algorithmic traffic (reverse: x, raw read, y written = 3 tensors; backward: 4.5 tensors): " +
        ", ".join(f"{k} {v:.2f} TB/s" for k, v in results["TBps"].items()))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_sample_log_prob.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_sample_log_prob.json"), "w") as f:
        json.dump(results, f, indent=1)
def child(tree, way):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np, torch
    import fincflow_amd
    from fincflow_amd import FastFlowUnit, FlowSequential, _lib, glow
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
    seq = FlowSequential(glow.GaussianPrior((C, H, W)), FastFlowUnit(C, C, 3), an, glow.Conv1x1(C), cp).to(dev)
    def draw():
        if way == "one_pass":
            return seq.rsample_with_log_prob(B)
        x = seq.rsample(B)
        return x, seq.log_prob(x)
    def step():
        seq.zero_grad(set_to_none=True)
        x, log_q = draw()
        (log_q - x.square().flatten(1).sum(1)).mean().backward()
        return x, log_q
    def nograd():
        with torch.no_grad():
            if way == "one_pass":
                return seq.sample_with_log_prob(B)
            x, _ = seq.sample(B)
            return x, seq.log_prob(x)
    def measure(fn, reps):
        t_end = time.perf_counter() + 1.0
        while time.perf_counter() < t_end:
            fn(); torch.cuda.synchronize()
        rounds = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps): fn()
            b.record(); torch.cuda.synchronize()
            rounds.append(a.elapsed_time(b) / reps)
        return rounds
    torch.manual_seed(5)
    x, log_q = step(); torch.cuda.synchronize()
    # the same seed, the same z: what the step computes, for the comparison between the legs
    check = {"x_abs_mean": float(x.detach().abs().mean()), "log_q_mean": float(log_q.detach().mean()),
             "grad_abs_sum": {n: float(p.grad.abs().sum()) for n, p in seq.named_parameters() if n.split(".")[-1] in ("log_scale", "translation", "W", "logs")}}
    train, infer = measure(step, 3), measure(nograd, 5)
    print(json.dumps({"step_ms": med(train), "step_rounds_ms": train, "nograd_ms": med(infer), "nograd_rounds_ms": infer,
                      "finc_version": int(_lib.lib().finc_version()), "check": check, "fault_pending": bool(_lib.fault_pending())}))
def driver(other, path):
    legs = (("parent commit, rsample + log_prob", other, "two_pass"), ("this commit, rsample + log_prob", HERE, "two_pass"),
            ("this commit, rsample_with_log_prob", HERE, "one_pass"))
    runs = []
    for r in range(1, 4):
        for name, tree, way in legs:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", tree, way], capture_output=True, text=True, timeout=240,
                               env={k: v for k, v in os.environ.items() if k not in ("FINCFLOW_LIB", "PYTHONPATH")})
            if p.returncode != 0:            # nothing more is started on the GPU after a failure
                sys.exit(f"{name} run {r} failed ({p.returncode}): {p.stderr[-800:]}")
            runs.append(dict(leg=name, run=r, **json.loads(p.stdout.strip().splitlines()[-1])))
            print(runs[-1], flush=True)
    out = {"what": "[FastFlowUnit(96), ActNorm(96), Conv1x1(96), Coupling((96, 64, 64))] at B = 256 on one MI355X, fresh processes, legs "
                   "alternated; step = draw + backward of (log_q - |x|^2).mean(), nograd = the draw and its log-density without a graph",
           "runs": runs}
    for name, _, _ in legs:
        for key in ("step_ms", "nograd_ms"):
            v = [q[key] for q in runs if q["leg"] == name]
            out.setdefault(name, {})[key] = {"median": med(v), "min": min(v), "max": max(v)}
    print(json.dumps({k: out[k] for k, _, _ in legs}), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3])
    elif len(sys.argv) > 2 and sys.argv[1] == "step":
        driver(sys.argv[2], sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "json" else None)
    else:
        kernels(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "sample_log_prob"))
