"""GPU helper: what the Gaussianized split's launches cost, HIP events, legs alternated in this one process, 7 rounds.

    python scripts/time_gauss_split.py [DIR]       # writes DIR/time_gauss_split.{txt,json}

At [256, 96, 64, 64], each new launch beside (a) its sibling of the split prior, which moves the same bytes and does one tanh more,
and (b) the launch sequence of the module's PyTorch lines behind the convolution, on this same build:
    finc_gauss_split              | finc_split_prior              | h = a raw + b, slices, (x2 - m) exp(-logs), -sum logs, base.log_prob
    finc_gauss_split_merge        | finc_split_prior_merge        | h, slices, m + z2 exp(logs), torch.cat
    ... with log p                | ... with log p                | that + -sum logs + base.log_prob
    finc_gauss_split_backward     | finc_split_prior_backward     | autograd's backward of the PyTorch lines (graph kept)
then the modules at that shape, without a graph: Split.split / merge (one 48 -> 96 3x3 convolution) beside SplitPrior.split / merge
(coupling_width=512: the three-convolution net).  There is no earlier implementation of this layer: nothing here is a speed-up of
one.  The difference to the sibling is printed beside the sibling's own spread over the rounds (max - min): a difference inside that
spread is not a difference.
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
        """fns[0]: the new launch, fns[1]: its sibling, fns[2:]: the PyTorch lines; alternated per round."""
        t = [[] for _ in fns]
        for _ in range(7):                       # alternately, so that clocks and neighbours on the box hit every leg alike
            for k, fn in enumerate(fns):
                t[k].append(timeit(torch, fn, n))
        spread = max(t[1]) - min(t[1])
        inside = min(t[1]) <= med(t[0]) <= max(t[1])
        say(f"  {name}:")
        for k, label in enumerate(labels):
            say(f"    {label}: {med(t[k]):.1f} us (min {min(t[k]):.1f} max {max(t[k]):.1f})" +
                ("" if k == 0 else f" | new / this {med(t[0]) / med(t[k]):.3f}, difference of the medians {med(t[0]) - med(t[k]):+.1f} us") +
                (f", the sibling's own spread {spread:.1f} us: the new median lies {'inside' if inside else 'OUTSIDE'} the sibling's min..max" if k == 1 else ""))
        results[name] = {label + "_us": v for label, v in zip(labels, t)}
        results[name].update(ratio_to_sibling=med(t[0]) / med(t[1]), difference_to_sibling_us=med(t[0]) - med(t[1]), sibling_spread_us=spread,
                             inside_sibling_range=inside)
        return [med(v) for v in t]
    B, C, H, W = SHAPE
    half = C // 2
    torch.manual_seed(4)
    x = torch.randn(SHAPE, device=dev); g = torch.randn(SHAPE, device=dev); raw = 0.5 * torch.randn(SHAPE, device=dev)
    a = torch.exp(0.1 * torch.randn(C, device=dev)); b = 0.1 * torch.randn(C, device=dev) * a; gl = torch.randn(B, device=dev)
    g1, g2 = g[:, :half].contiguous(), g[:, half:].contiguous()
    del g
    out, halves = torch.empty_like(x), (torch.empty(B, half, H, W, device=dev), torch.empty(B, half, H, W, device=dev))
    base = glow.GaussianPrior((half, H, W)).to(dev)
    a4, b4 = a.view(1, -1, 1, 1), b.view(1, -1, 1, 1)
    def lines_split(x, raw, a4, b4):
        h = raw * a4 + b4
        m, logs = h[:, 0::2], h[:, 1::2]
        z2 = (x[:, half:] - m) * torch.exp(-logs)
        return x[:, :half], z2, base.log_prob(z2) - logs.flatten(start_dim=1).sum(-1)
    def lines_merge(x1, z2, with_log_p):
        h = raw * a4 + b4
        m, logs = h[:, 0::2], h[:, 1::2]
        xx = torch.cat([x1, m + z2 * torch.exp(logs)], dim=1)
        return (xx, base.log_prob(z2) - logs.flatten(start_dim=1).sum(-1)) if with_log_p else xx
    say(f"B{B} C{C} {H}x{W}, kernels alone, 7 rounds of 20 launches each, alternated:")
    with torch.no_grad():
        x1, z2, lp = ops.finc_gauss_split(x, raw, a, b)
        want = lines_split(x, raw, a4, b4)
        assert torch.equal(x1, want[0]) and float((z2 - want[1]).abs().max() / want[1].abs().max()) <= 1e-5
        assert float((lp - want[2]).abs().max() / want[2].abs().max()) <= 1e-5
        assert float((ops.finc_gauss_split_merge(x1, z2, raw, a, b) - x).abs().max() / x.abs().max()) <= 5e-5
        s1, s2, _ = ops.finc_split_prior(x, raw, a, b)
        s = legs("split", (lambda: ops.finc_gauss_split(x, raw, a, b, out=halves), lambda: ops.finc_split_prior(x, raw, a, b, out=halves),
                           lambda: lines_split(x, raw, a4, b4)),
                 ("finc_gauss_split (new, 2 launches)", "finc_split_prior (sibling, 2 launches)", "the module's PyTorch lines behind the convolution"))
        m = legs("merge", (lambda: ops.finc_gauss_split_merge(x1, z2, raw, a, b, out=out), lambda: ops.finc_split_prior_merge(s1, s2, raw, a, b, out=out),
                           lambda: lines_merge(x1, z2, False)),
                 ("finc_gauss_split_merge (new, 1 launch)", "finc_split_prior_merge (sibling, 1 launch)", "the module's PyTorch lines behind the convolution"))
        ml = legs("merge with log p", (lambda: ops.finc_gauss_split_merge(x1, z2, raw, a, b, True, out=out),
                                       lambda: ops.finc_split_prior_merge(s1, s2, raw, a, b, True, out=out), lambda: lines_merge(x1, z2, True)),
                  ("finc_gauss_split_merge with log p (new, 2 launches)", "finc_split_prior_merge with log p (sibling, 2 launches)",
                   "the module's PyTorch lines behind the convolution"))
    del s1, s2, want
    leaves = [v.clone().requires_grad_(True) for v in (x, raw, a4, b4)]
    outs = lines_split(*leaves)
    def lines_backward():
        return torch.autograd.grad(outs, leaves, (g1, g2, gl), retain_graph=True)
    with torch.no_grad():
        got, ref = ops.finc_gauss_split_backward(g1, g2, gl, x, raw, a, b), lines_backward()
        for k, (u, v) in enumerate(zip(got, ref)):
            assert float((u - v.reshape(u.shape)).abs().max() / v.abs().max()) <= 1e-4, k     # (fp32 against fp32 here; the bar is the tests')
        del got, ref
        bw = legs("split backward", (lambda: ops.finc_gauss_split_backward(g1, g2, gl, x, raw, a, b),
                                     lambda: ops.finc_split_prior_backward(g1, g2, gl, x, raw, a, b), lines_backward),
                  ("finc_gauss_split_backward (new)", "finc_split_prior_backward (sibling)", "autograd's backward of the PyTorch lines (graph kept)"))
    del outs, leaves
    nbytes = 4 * x.numel()
    results["TBps"] = {"split": 3 * nbytes / s[0] / 1e6, "split_prior": 3 * nbytes / s[1] / 1e6, "merge": 3 * nbytes / m[0] / 1e6,
                       "split_prior_merge": 3 * nbytes / m[1] / 1e6, "split_backward": 5 * nbytes / bw[0] / 1e6,
                       "split_prior_backward": 5 * nbytes / bw[1] / 1e6}
    say("  algorithmic traffic (transforms: x, raw read, halves written = 3 tensors; backwards: grads, x, raw read, grad_x, grad_raw written = 5): " +
        ", ".join(f"{k} {v:.2f} TB/s" for k, v in results["TBps"].items()))
    del raw, out, halves, x1, z2, g1, g2
    torch.cuda.empty_cache()

    gen = torch.Generator().manual_seed(1)
    def filled(mod):
        with torch.no_grad():
            for name, p in mod.named_parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * (0.1 if name.endswith(("bias", "logs", "log_scale_factor")) else 0.02))
        return mod.to(dev)
    new, old = filled(glow.Split((C, H, W), glow.GaussianPrior)), filled(glow.SplitPrior((C, H, W), glow.GaussianPrior, width=512))
    with torch.no_grad():
        n1, n2, _ = new.split(x)
        o1, o2, _ = old.split(x)
        say(f"modules at B{B} C{C} {H}x{W}, no graph, 7 rounds of 3 calls each, alternated (Split: one 48 -> 96 3x3 convolution; SplitPrior: "
            "the 512-wide three-convolution net):")
        legs("module split", (lambda: new.split(x), lambda: old.split(x)), ("Split.split (new)", "SplitPrior.split (the boundary offered so far)"), n=3)
        # what Split.split runs besides its launch: the convolution, and the copy of the channel slice x[:, :half] that the convolution
        # makes of its strided input (SplitPrior's net pays the same copy)
        w = new.gaussianize.net.weight
        x1c = x[:, :half].contiguous()
        parts = [[], [], []]
        for _ in range(7):
            for k, fn in enumerate((lambda: x[:, :half].contiguous(), lambda: torch.nn.functional.conv2d(x1c, w, None, padding=1),
                                    lambda: torch.nn.functional.conv2d(x[:, :half], w, None, padding=1))):
                parts[k].append(timeit(torch, fn, 3))
        for label, v in zip(("copy of the slice x[:, :half]", "the 48 -> 96 3x3 convolution on a contiguous x1", "the same convolution on the slice"), parts):
            say(f"    {label}: {med(v):.1f} us (min {min(v):.1f} max {max(v):.1f})")
        results["module split parts_us"] = parts
        del x1c
        legs("module merge",(lambda: new.merge(n1, n2), lambda: old.merge(o1, o2)), ("Split.merge (new)", "SplitPrior.merge (the boundary offered so far)"), n=3)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_gauss_split.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_gauss_split.json"), "w") as f:
        json.dump(results, f, indent=1)
if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "gauss_split"))
