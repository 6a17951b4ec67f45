"""GPU helper: what the split prior's own launches cost, HIP events, legs alternated in this one process, 7 rounds.

    python scripts/time_split_latent.py [DIR]       # writes DIR/time_split_latent.{txt,json}

At [256, 96, 64, 64], each new launch beside the sibling that moves the same bytes (3 tensors of B C HW floats), and beside what it
replaces on this same build:
    finc_split_prior            | finc_coupling direction +1 with its log-det            | that launch + the slices + base.log_prob
    finc_split_prior_merge      | finc_coupling direction -1                             | torch.cat + that launch
    finc_split_prior_merge with log p | finc_coupling_reverse_logdet                     | torch.cat + that launch + base.log_prob
    finc_split_prior_backward   | finc_coupling_backward (with grad_logdet)
then the split, the merge and their siblings again on four fresh sets of output allocations (what the placement of the tensors alone
is worth),
and, on create_model(num_blocks=3, block_size=4, split_prior=True, actnorm=True, preprocess=False) at 64x64, B = 64, without a graph:
    encode | forward            decode | _reverse_chain on the same latents (the split layers' draws recorded and handed back)
There is no earlier implementation of the latents: nothing here is a speed-up of one.  The ratio to the sibling is printed beside the
sibling's own spread over the rounds (max - min): a difference inside that spread is not a difference.
"""
import json, os, statistics, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (256, 96, 64, 64)
MODEL_BATCH = 64
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
    import numpy as np, torch
    from fincflow_amd import glow, ops
    dev = torch.device("cuda:0")
    lines, results = [], {"shape": list(SHAPE), "model_batch": MODEL_BATCH}
    def say(s):
        print(s, flush=True); lines.append(s)
    def legs(name, fns, labels, n=20):
        """fns[0]: the new launch, fns[1]: its sibling, fns[2:]: what the new launch replaces; alternated per round."""
        t = [[] for _ in fns]
        for _ in range(7):                       # alternately, so that clocks and neighbours on the box hit every leg alike
            for k, fn in enumerate(fns):
                t[k].append(timeit(torch, fn, n))
        spread = max(t[1]) - min(t[1])
        say(f"  {name}:")
        for k, label in enumerate(labels):
            say(f"    {label}: {med(t[k]):.1f} us (min {min(t[k]):.1f} max {max(t[k]):.1f})" +
                ("" if k == 0 else f" | new / this {med(t[0]) / med(t[k]):.3f}, difference of the medians {med(t[0]) - med(t[k]):+.1f} us") +
                (f", the sibling's own spread {spread:.1f} us" if k == 1 else ""))
        results[name] = {label + "_us": v for label, v in zip(labels, t)}
        results[name].update(ratio_to_sibling=med(t[0]) / med(t[1]), difference_to_sibling_us=med(t[0]) - med(t[1]), sibling_spread_us=spread)
        return [med(v) for v in t]
    B, C, H, W = SHAPE
    half = C // 2
    torch.manual_seed(4)
    x = torch.randn(SHAPE, device=dev); g = torch.randn(SHAPE, device=dev); raw = 1.5 * torch.randn(SHAPE, device=dev)
    a = torch.exp(0.3 * torch.randn(C, device=dev)); b = 0.3 * torch.randn(C, device=dev) * a; gl = torch.randn(B, device=dev)
    g1, g2 = g[:, :half].contiguous(), g[:, half:].contiguous()
    out, halves = torch.empty_like(x), (torch.empty(B, half, H, W, device=dev), torch.empty(B, half, H, W, device=dev))
    base = glow.GaussianPrior((half, H, W)).to(dev)
    say(f"B{B} C{C} {H}x{W}, kernels alone, 7 rounds of 20 launches each, alternated:")
    with torch.no_grad():
        y = ops.finc_coupling(x, raw, a, b, 1)[0]
        x1, z2, _ = ops.finc_split_prior(x, raw, a, b)
        assert torch.equal(x1, y[:, :half]) and torch.equal(z2, y[:, half:])
        assert torch.equal(ops.finc_split_prior_merge(x1, z2, raw, a, b), ops.finc_coupling(y, raw, a, b, -1)[0])
        def old_split():
            yy, ld = ops.finc_coupling(x, raw, a, b, 1, True, out=out)
            return yy[:, :half], base.log_prob(yy[:, half:]) + ld
        def old_merge():
            return ops.finc_coupling(torch.cat([x1, z2], dim=1), raw, a, b, -1, out=out)[0]
        def old_merge_lp():
            yy, ld = ops.finc_coupling_reverse_logdet(torch.cat([x1, z2], dim=1), raw, a, b, out=out)
            return yy, base.log_prob(z2) + ld
        s = legs("split", (lambda: ops.finc_split_prior(x, raw, a, b, out=halves), lambda: ops.finc_coupling(x, raw, a, b, 1, True, out=out), old_split),
                 ("finc_split_prior (new, 2 launches)", "finc_coupling +1 with log-det (sibling, 2 launches)",
                  "that + slices + base.log_prob (what SplitPrior.forward runs)"))
        m = legs("merge", (lambda: ops.finc_split_prior_merge(x1, z2, raw, a, b, out=out), lambda: ops.finc_coupling(y, raw, a, b, -1, out=out), old_merge),
                 ("finc_split_prior_merge (new, 1 launch)", "finc_coupling -1 (sibling, 1 launch)", "torch.cat + that (what SplitPrior.reverse runs)"))
        ml = legs("merge with log p", (lambda: ops.finc_split_prior_merge(x1, z2, raw, a, b, True, out=out),
                                       lambda: ops.finc_coupling_reverse_logdet(y, raw, a, b, out=out), old_merge_lp),
                  ("finc_split_prior_merge with log p (new, 2 launches)", "finc_coupling_reverse_logdet (sibling, 2 launches)",
                   "torch.cat + that + base.log_prob (what SplitPrior.reverse_with_logdet runs)"))
        bw = legs("split backward", (lambda: ops.finc_split_prior_backward(g1, g2, gl, x, raw, a, b), lambda: ops.finc_coupling_backward(g, gl, x, raw, a, b)),
                  ("finc_split_prior_backward (new)", "finc_coupling_backward with grad_logdet (sibling)"))
        # Where the outputs lie: the same two launches on four fresh sets of output allocations each (the earlier ones kept alive, so
        # that every set has addresses of its own), 3 rounds per set, alternated.  The range of a kernel's medians over the sets is
        # what the placement of its tensors alone is worth: a gap to the sibling inside that range is not the kernel's.
        say("  placement: the same launches on 4 fresh sets of output allocations, median of 3 rounds of 20 per set:")
        keep, placed = [], {"split": [], "coupling +1": [], "merge": [], "coupling -1": []}
        for _ in range(4):
            o, h = torch.empty_like(x), (torch.empty(B, half, H, W, device=dev), torch.empty(B, half, H, W, device=dev))
            keep.append((o, h))
            fns = {"split": lambda: ops.finc_split_prior(x, raw, a, b, out=h), "coupling +1": lambda: ops.finc_coupling(x, raw, a, b, 1, True, out=o),
                   "merge": lambda: ops.finc_split_prior_merge(x1, z2, raw, a, b, out=o), "coupling -1": lambda: ops.finc_coupling(y, raw, a, b, -1, out=o)}
            t = {k: [] for k in fns}
            for _ in range(3):
                for k, fn in fns.items():
                    t[k].append(timeit(torch, fn, 20))
            for k in fns:
                placed[k].append(med(t[k]))
        for k, v in placed.items():
            say(f"    {k}: " + ", ".join(f"{u:.1f}" for u in v) + f" us (range {max(v) - min(v):.1f} us)")
        results["placement_us"] = placed
        del keep
    nbytes = 4 * x.numel()
    results["TBps"] = {"split": 3 * nbytes / s[0] / 1e6, "coupling_forward_logdet": 3 * nbytes / s[1] / 1e6, "merge": 3 * nbytes / m[0] / 1e6,
                       "coupling_reverse": 3 * nbytes / m[1] / 1e6, "split_backward": 5 * nbytes / bw[0] / 1e6, "coupling_backward": 5 * nbytes / bw[1] / 1e6}
    say("  algorithmic traffic (transforms: x, raw read, y written = 3 tensors; backwards: grad_y, x, raw read, grad_x, grad_raw written = 5): " +
        ", ".join(f"{k} {v:.2f} TB/s" for k, v in results["TBps"].items()))
    del x, g, raw, out, halves, y, x1, z2, g1, g2
    torch.cuda.empty_cache()

    torch.manual_seed(1); np.random.seed(1)
    model = glow.create_model(num_blocks=3, block_size=4, split_prior=True, actnorm=True, preprocess=False, image_size=(3, 64, 64))
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, glow.Conv2dZero):
                mod.weight.copy_(0.02 * torch.randn(mod.weight.shape, generator=gen)); mod.bias.copy_(0.01 * torch.randn(mod.bias.shape, generator=gen))
                mod.logs.copy_(0.01 * torch.randn(mod.logs.shape, generator=gen))
    model = model.to(dev)
    xm = torch.randn(MODEL_BATCH, 3, 64, 64, device=dev)
    with torch.no_grad():
        model(xm)                                # (ActNorm's data-dependent initialisation)
        zs, lp = model.encode(xm)
        back = model.decode(zs)
        err = float((back - xm).abs().max() / xm.abs().max())
        splits = [mod for mod in model.sequence_modules if hasattr(mod, "split")]
        for mod, z in zip(splits, zs):           # the reverse chain consumes the recorded draws: the same latents on both legs
            mod.base.sample = (lambda n, context=None, _z=z: (_z, None))
        # (the two legs hand the split layers' nets the same values -- x1 as a tensor of its own, or as a slice of the cat --
        # and a convolution on other strides may round differently: the same x to fp32 rounding, not to the bit)
        chain = model._reverse_chain(zs[-1], None)
        gap = float((chain - back).abs().max() / back.abs().max())
        assert gap <= 1e-5, gap
        say(f"model: 3 blocks of 4 steps, split priors, 3x64x64, B{MODEL_BATCH}, no graph; decode(encode(x)) - x: {err:.2e} of max |x|, "
            f"decode against _reverse_chain on the same draws: {gap:.2e}; 7 rounds of 5 passes each, alternated:")
        legs("encode", (lambda: model.encode(xm), lambda: model(xm)), ("encode (new)", "forward (sibling: the same walk, latents dropped)"), n=5)
        legs("decode", (lambda: model.decode(zs), lambda: model._reverse_chain(zs[-1], None)),
             ("decode (new)", "_reverse_chain with the recorded draws (sibling)"), n=5)
    results["round_trip_rel_err"], results["decode_against_reverse_chain"] = err, gap
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_split_latent.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_split_latent.json"), "w") as f:
        json.dump(results, f, indent=1)
if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "split_latent"))
