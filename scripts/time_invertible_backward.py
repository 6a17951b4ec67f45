"""GPU helper: training without stored activations (FlowSequential.invertible_backward) at [256, 96, 64, 64], HIP events,
legs alternated in this one process, medians and spread of the rounds per leg.

  1. the training step -- log_prob(x).mean().backward() -- on [FastFlowUnit, ActNorm, Conv1x1, Coupling] x 4, stored against
     invertible, with torch.cuda.max_memory_allocated of each;
  2. each new kernel against the two-launch sequence it replaces, on the same build (those kernels are unchanged by this feature, so
     the same build is the parent):
       finc_actnorm_backward_reconstruct_f32   against  finc_actnorm_f32(direction -1)  + finc_actnorm_backward_f32
       finc_coupling_backward_reconstruct_f32  against  finc_coupling_f32(direction -1) + finc_coupling_backward_f32

    python scripts/time_invertible_backward.py [DIR]         # writes DIR/time_invertible_backward.{txt,json}
"""
import json, os, statistics, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MIOPEN_FIND_MODE", "2")       # the coupling nets' convolutions: immediate-mode heuristics, both legs alike
SHAPE = (256, 96, 64, 64)
BLOCKS = 4
med = statistics.median
def timeit(torch, fn, n, warm=0.3):
    t_end = time.perf_counter() + warm       # clocks ramp up over the first tenths of a second of load
    while time.perf_counter() < t_end:
        fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3
def main(out_dir):
    sys.path.insert(0, HERE)
    import numpy as np, torch
    from fincflow_amd import FastFlowUnit, FlowSequential, _lib, glow, ops
    dev = torch.device("cuda:0")
    lines, results = [], {"shape": list(SHAPE), "blocks": BLOCKS, "finc_version": int(_lib.lib().finc_version())}
    def say(s):
        print(s, flush=True); lines.append(s)
    def ab(name, new_fn, old_fn, n, out, labels, rounds=7, unit="us"):
        new, old = [], []
        for _ in range(rounds):                  # alternately, so that clocks and neighbours on the box hit both alike
            new.append(timeit(torch, new_fn, n)); old.append(timeit(torch, old_fn, n))
        scale = 1.0 if unit == "us" else 1e-3
        new, old = [v * scale for v in new], [v * scale for v in old]
        gap = min(old) - max(new)                # > 0: every round of the first leg beat every round of the second
        verdict = ("the first faster by more than the spread" if gap > 0 else
                   "the second faster by more than the spread" if min(new) - max(old) > 0 else "NOT separated from the spread")
        say(f"  {name}: {labels[0]} {med(new):.1f} {unit} (min {min(new):.1f} max {max(new):.1f}) | {labels[1]} {med(old):.1f} {unit} "
            f"(min {min(old):.1f} max {max(old):.1f}) | {labels[1]} / {labels[0]} = {med(old) / med(new):.3f} | {verdict}")
        out[name] = {labels[0]: new, labels[1]: old, "unit": unit, "ratio_of_medians": med(old) / med(new), "verdict": verdict}
        return med(new), med(old)
    B, C, H, W = SHAPE
    nbytes = 4 * B * C * H * W
    torch.manual_seed(4); np.random.seed(4)
    # ---- 2. the kernels (first: the step below leaves the allocator full)
    x = torch.randn(SHAPE, device=dev); g = torch.randn(SHAPE, device=dev); gl = torch.randn(B, device=dev)
    raw = 1.5 * torch.randn(SHAPE, device=dev); logs = 0.1 * torch.randn(C, device=dev)
    a = torch.exp(3 * logs); b = 0.3 * torch.randn(C, device=dev) * a
    ls = 0.2 * torch.randn(C, device=dev); tr = torch.randn(C, device=dev)
    k = results["kernels"] = {}
    say(f"B{B} C{C} {H}x{W}: each new kernel (every output asked for) against the two launches it replaces")
    with torch.no_grad():
        yn = ops.finc_actnorm(x, ls, tr, 1)[0]
        yc = ops.finc_coupling(x, raw, a, b, 1)[0]
        def act_pair():
            xr = ops.finc_actnorm(yn, ls, tr, -1)[0]
            return xr, ops.finc_actnorm_backward(g, gl, yn, ls)
        def cpl_pair():
            xr = ops.finc_coupling(yc, raw, a, b, -1)[0]
            return xr, ops.finc_coupling_backward(g, gl, xr, raw, a, b)
        fa, pa = ab("ActNorm", lambda: ops.finc_actnorm_backward_reconstruct(g, gl, yn, ls, tr), act_pair, 20, k, ("fused", "pair"))
        fc, pc = ab("Coupling", lambda: ops.finc_coupling_backward_reconstruct(g, gl, yc, raw, a, b), cpl_pair, 20, k, ("fused", "pair"))
    # tensor passes by the kernels' loads and stores: ActNorm fused reads grad_y, y and writes x, grad_x (4), the pair 2 + 3; the coupling
    # fused reads grad_y, y, raw and writes x, grad_x, grad_raw (6), the pair 3 (reverse) + 4.5 (its backward reads only the second half of x)
    for name, tf, tp, f, p in (("ActNorm", 4, 5, fa, pa), ("Coupling", 6, 7.5, fc, pc)):
        k[name]["tensor_passes"] = {"fused": tf, "pair": tp}
        k[name]["TBps"] = {"fused": tf * nbytes / f / 1e6, "pair": tp * nbytes / p / 1e6}
        say(f"  {name}: fused {tf} tensor passes = {k[name]['TBps']['fused']:.2f} TB/s | pair {tp} = {k[name]['TBps']['pair']:.2f} TB/s | "
            f"by byte count the pair would take {tp / tf:.2f} x the fused time, measured {p / f:.2f} x")
    del x, g, raw, yn, yc
    torch.cuda.empty_cache()
    # ---- 1. the training step
    mods = []
    gen = torch.Generator().manual_seed(1)
    for _ in range(BLOCKS):
        an, cp = glow.ActNorm(C), glow.Coupling((C, H, W))
        with torch.no_grad():
            an.log_scale.copy_(0.2 * torch.randn(C, generator=gen)); an.translation.copy_(torch.randn(C, generator=gen)); an.mark_initialized()
            last = cp.net[4]
            last.weight.copy_(0.02 * torch.randn(last.weight.shape, generator=gen)); last.bias.copy_(0.01 * torch.randn(last.bias.shape, generator=gen))
            last.logs.copy_(0.01 * torch.randn(last.logs.shape, generator=gen))
        mods += [FastFlowUnit(C, C, 3), an, glow.Conv1x1(C), cp]
    model = FlowSequential(glow.GaussianPrior((C, H, W)), *mods).to(dev)
    xin = torch.randn(SHAPE, device=dev)
    def step(mode):
        model.invertible_backward = mode
        model.zero_grad(set_to_none=True)
        lp = model.log_prob(xin)
        lp.mean().backward()
        return lp
    s = results["step"] = {}
    peaks, grads = {}, {}
    for mode, name in ((False, "stored"), (True, "invertible")):
        step(mode); torch.cuda.synchronize()             # warm-up: workspaces, bank caches, MIOpen's choices
        torch.cuda.reset_peak_memory_stats()
        lp = step(mode); torch.cuda.synchronize()
        peaks[name] = int(torch.cuda.max_memory_allocated())
        grads[name] = [lp.detach().clone()] + [p.grad.clone() for p in model.parameters()]
    say(f"training step, log_prob(x).mean().backward() on [FastFlowUnit, ActNorm, Conv1x1, Coupling] x {BLOCKS} (coupling width 512):")
    ab("step", lambda: step(True), lambda: step(False), 2, s, ("invertible", "stored"), rounds=5, unit="ms")
    s["max_memory_allocated_bytes"] = peaks
    s["activation_bytes"] = nbytes
    names = ["log_prob"] + [n for n, _ in model.named_parameters()]
    lp = step(False); torch.cuda.synchronize()           # the stored path once more: its own run-to-run difference, the yardstick
    grads["stored again"] = [lp.detach().clone()] + [p.grad.clone() for p in model.parameters()]
    def worst(a, b):
        d = {n: float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for n, p, q in zip(names, grads[a], grads[b])}
        n = max(d, key=d.get)
        s["largest_rel_diffs " + a + " / " + b] = dict(sorted(d.items(), key=lambda kv: -kv[1])[:8])
        return d[n], n
    s["max_rel_diff_of_log_prob_and_gradients"], s["max_rel_diff_at"] = worst("invertible", "stored")
    s["stored_run_to_run_max_rel_diff"], s["stored_run_to_run_at"] = worst("stored again", "stored")
    s["log_prob_rel_diff"] = float((grads["invertible"][0] - grads["stored"][0]).abs().max() / grads["stored"][0].abs().max())
    say(f"  max_memory_allocated: stored {peaks['stored'] / 2**30:.2f} GiB | invertible {peaks['invertible'] / 2**30:.2f} GiB "
        f"(one activation is {nbytes / 2**30:.2f} GiB) | ratio {peaks['stored'] / peaks['invertible']:.2f}")
    say(f"  max rel diff of log_prob and every gradient (per tensor, max-norm), invertible against stored: "
        f"{s['max_rel_diff_of_log_prob_and_gradients']:.1e} ({s['max_rel_diff_at']}); log_prob alone {s['log_prob_rel_diff']:.1e}; "
        f"the stored path against itself, run to run: {s['stored_run_to_run_max_rel_diff']:.1e} ({s['stored_run_to_run_at']})")
    # ---- 3. how far the rebuilt activations drift from the stored ones, layer by layer from the back (limit (a))
    from fincflow_amd.layers import BackwardNeeds
    model.zero_grad(set_to_none=True)
    d = results["rebuilt_activation_rel_err"] = {}
    with torch.no_grad():
        acts = [xin]
        for m in mods:
            acts.append(m(acts[-1])[0])
        y, gy = acts[-1], torch.randn(SHAPE, device=dev)
        for i in reversed(range(len(mods))):
            y, gy, _, _ = mods[i].backward_from_output(y, gy, None, None, BackwardNeeds(True, True, False, False))
            d[f"{i} {type(mods[i]).__name__}"] = float((y - acts[i]).abs().max() / acts[i].abs().max())
    say("  input of each layer as rebuilt by the walk against the stored one, max |diff| / max |stored| (last layer first): "
        + ", ".join(f"{k.split()[0]}:{v:.1e}" for k, v in d.items()))
    del acts
    results["fault_pending"] = bool(_lib.fault_pending())
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_invertible_backward.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_invertible_backward.json"), "w") as f:
        json.dump(results, f, indent=1)
if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "invertible_backward"))
