"""GPU helper: what the merges' backward costs, HIP events, legs alternated in this one process, 7 rounds.

    python scripts/time_merge_backward.py [DIR]       # writes DIR/time_merge_backward.{txt,json}

At [256, 96, 64, 64], each new launch beside (a) its forward-direction sibling, which moves the same five tensors, and (b) autograd's
backward of the recorded lines it replaces (graph kept), on this same build:
    finc_split_prior_merge_backward   | finc_split_prior_backward   | backward of cat + ops.coupling_reverse_logdet + base.log_prob
    finc_gauss_split_merge_backward   | finc_gauss_split_backward   | backward of h = a raw + b, slices, m + z2 exp(logs), cat, base.log_prob
then the modules at that shape inside ops.reverse_grad(), one recorded merge(with_log_prob=True) and its backward to x1, z2 and every
parameter, `hip_recorded_merge` on beside off: Split (one 48 -> 96 3x3 convolution) and SplitPrior (coupling_width=512).  There was no
earlier kernel for these backwards: nothing here is a speed-up of one.  Every comparison prints both legs' min .. max over the rounds
and whether the ranges overlap: overlapping ranges are not a difference.
"""
import json, os, statistics, sys, time
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
def main(out_dir):
    sys.path.insert(0, HERE)
    import torch
    from fincflow_amd import glow, ops
    dev = torch.device("cuda:0")
    lines, results = [], {"shape": list(SHAPE)}
    def say(s):
        print(s, flush=True); lines.append(s)
    def legs(name, fns, labels, n=20):
        """fns[0]: the new path, fns[1:]: what it is set beside; alternated per round."""
        t = [[] for _ in fns]
        for _ in range(7):                       # alternately, so that clocks and neighbours on the box hit every leg alike
            for k, fn in enumerate(fns):
                t[k].append(timeit(torch, fn, n))
        say(f"  {name}:")
        results[name] = {}
        for k, label in enumerate(labels):
            overlap = k > 0 and min(t[0]) <= max(t[k]) and min(t[k]) <= max(t[0])
            say(f"    {label}: {med(t[k]):.1f} us (min {min(t[k]):.1f} max {max(t[k]):.1f})" +
                ("" if k == 0 else f" | new / this {med(t[0]) / med(t[k]):.3f}, difference of the medians {med(t[0]) - med(t[k]):+.1f} us, "
                                   f"the two min..max ranges {'OVERLAP' if overlap else 'do not overlap'}"))
            results[name][label] = dict(us=t[k], median_us=med(t[k]), **({} if k == 0 else dict(new_over_this=med(t[0]) / med(t[k]), ranges_overlap=overlap)))
        return [med(v) for v in t]
    B, C, H, W = SHAPE
    half = C // 2
    torch.manual_seed(4)
    x = torch.randn(SHAPE, device=dev); gx = torch.randn(SHAPE, device=dev); raw = 0.5 * torch.randn(SHAPE, device=dev)
    a = torch.exp(0.1 * torch.randn(C, device=dev)); b = 0.1 * torch.randn(C, device=dev) * a; gl = torch.randn(B, device=dev)
    x1, z2 = x[:, :half].contiguous(), x[:, half:].contiguous()
    g1, g2 = gx[:, :half].contiguous(), gx[:, half:].contiguous()
    base = glow.GaussianPrior((half, H, W)).to(dev)
    a4, b4 = a.view(1, -1, 1, 1), b.view(1, -1, 1, 1)
    def lines_prior(x1, z2, raw, a, b):          # what SplitPrior.merge records today inside reverse_grad()
        out, ldj = ops.coupling_reverse_logdet(torch.cat([x1, z2], dim=1), raw, a, b)
        return out, base.log_prob(z2) + ldj
    def lines_gauss(x1, z2, raw, a, b):          # what Split.merge records today: the PyTorch lines behind the convolution
        h = raw * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
        m, logs = h[:, 0::2], h[:, 1::2]
        return torch.cat([x1, m + z2 * torch.exp(logs)], dim=1), base.log_prob(z2) - logs.flatten(start_dim=1).sum(-1)
    say(f"B{B} C{C} {H}x{W}, kernels alone, 7 rounds of 20 launches each, alternated:")
    times = {}
    for law, new, sibling, recorded, merge in (
            ("split prior", ops.finc_split_prior_merge_backward, ops.finc_split_prior_backward, lines_prior, ops.finc_split_prior_merge),
            ("Gaussianized split", ops.finc_gauss_split_merge_backward, ops.finc_gauss_split_backward, lines_gauss, ops.finc_gauss_split_merge)):
        leaves = [v.clone().requires_grad_(True) for v in (x1, z2, raw, a, b)]
        with ops.reverse_grad():
            outs = recorded(*leaves)
        def lines_backward(outs=outs, leaves=leaves):
            return torch.autograd.grad(outs, leaves, (gx, gl), retain_graph=True)
        with torch.no_grad():
            xm = merge(x1, z2, raw, a, b)
            got, ref = new(gx, gl, xm, raw, a, b), lines_backward()
            for k, (u, v) in enumerate(zip(got, ref)):
                assert float((u - v.reshape(u.shape)).abs().max() / v.abs().max()) <= 1e-4, (law, k)   # (fp32 against fp32 here; the bar is the tests')
            del got, ref
            times[law] = legs(f"{law}: merge backward",
                              (lambda: new(gx, gl, xm, raw, a, b), lambda: sibling(g1, g2, gl, x, raw, a, b), lines_backward),
                              (f"{new.__name__} (new)", f"{sibling.__name__} (the forward direction's, same five tensors)",
                               "autograd's backward of the recorded lines it replaces (graph kept)"))
        del outs, leaves, lines_backward, xm
        torch.cuda.empty_cache()
    nbytes = 4 * x.numel()
    results["TBps"] = {law: {"new": 5 * nbytes / t[0] / 1e6, "sibling": 5 * nbytes / t[1] / 1e6} for law, t in times.items()}
    say("  algorithmic traffic (grad_x, x, raw read, the two half gradients and grad_raw written = 5 tensors): " +
        ", ".join(f"{law}: new {v['new']:.2f} TB/s, sibling {v['sibling']:.2f} TB/s" for law, v in results["TBps"].items()))
    del raw, gx, g1, g2, x
    torch.cuda.empty_cache()

    gen = torch.Generator().manual_seed(1)
    def filled(mod):
        with torch.no_grad():
            for name, p in mod.named_parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * (0.1 if name.endswith(("bias", "logs", "log_scale_factor")) else 0.02))
        return mod.to(dev)
    say(f"modules at B{B} C{C} {H}x{W} inside reverse_grad(): merge(x1, z2, with_log_prob=True) recorded, then its backward to x1, z2 and every "
        "parameter; 7 rounds of 3 calls each, alternated:")
    gxm = torch.randn(SHAPE, device=dev)
    for label, mod in (("Split", filled(glow.Split((C, H, W), glow.GaussianPrior))),
                       ("SplitPrior", filled(glow.SplitPrior((C, H, W), glow.GaussianPrior, width=512)))):
        params = list(mod.parameters())
        def step(flag, mod=mod, params=params):
            mod.hip_recorded_merge = flag
            u, v = x1.detach().requires_grad_(True), z2.detach().requires_grad_(True)
            with ops.reverse_grad():
                out, lp = mod.merge(u, v, with_log_prob=True)
            return torch.autograd.grad((out, lp), [u, v] + params, (gxm, gl))
        on, off = step(True), step(False)
        worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(on, off))
        say(f"  {label}: largest difference between the two paths' gradients (max-normalised, fp32 against fp32): {worst:.1e}")
        del on, off
        legs(f"{label}.merge + backward", (lambda: step(True), lambda: step(False)),
             ("hip_recorded_merge on (one merge launch, one backward launch)", "hip_recorded_merge off (the recorded lines of today)"), n=3)
        del mod.hip_recorded_merge
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_merge_backward.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_merge_backward.json"), "w") as f:
        json.dump(results, f, indent=1)
if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "merge_backward"))
