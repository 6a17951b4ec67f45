"""GPU helper: what the image boundary's launches cost, HIP events, legs alternated in this one process, 7 rounds.

    python scripts/time_image_boundary.py [DIR]       # writes DIR/time_image_boundary.{txt,json}

At [256,3,32,32], [256,3,64,64] and [64,3,256,256], each fused launch beside the layered sequence it replaces ON THIS SAME BUILD (the
parent commit runs those same PyTorch lines):
    finc_image_encode (uint8 pixels) | finc_image_encode (fp32 pixels) | rand + Dequantization, 2 x Normalization, LogitTransform, Squeeze
    finc_image_decode (fp32) | finc_image_decode (uint8) | the five reverses, floor last | the same + clamp + cast to uint8
Both encode legs include the draw of the noise (`torch.rand`), as the layers' sequence does.  Then the share of the prefix and the tail
in one `log_prob` and one `sample(256)` of create_model(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3,16,16),
coupling_width=16), flag on and off.  There was no earlier kernel for any of this: nothing here is a speed-up of one.
"""
import json, os, statistics, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((256, 3, 32, 32), (256, 3, 64, 64), (64, 3, 256, 256))
med = statistics.median
def timeit(torch, fn, n):
    t_end = time.perf_counter() + 0.2        # clocks ramp up over the first tenths of a second of load
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
    from fincflow_amd import FlowSequential, glow, ops
    dev = torch.device("cuda:0")
    lines, results = [], {}
    def say(s):
        print(s, flush=True); lines.append(s)
    def legs(name, fns, labels, n=20):
        t = [[] for _ in fns]
        for _ in range(7):                       # alternately, so that clocks and neighbours on the box hit every leg alike
            for k, fn in enumerate(fns):
                t[k].append(timeit(torch, fn, n))
        say(f"  {name}:")
        for k, label in enumerate(labels):
            say(f"    {label}: {med(t[k]):.1f} us (min {min(t[k]):.1f} max {max(t[k]):.1f})")
        results[name] = {label + "_us": v for label, v in zip(labels, t)}
        return [med(v) for v in t]
    boundary = FlowSequential(glow.GaussianPrior((12, 1, 1)), glow.Dequantization(), glow.Normalization(0, 256),
                              glow.Normalization(-1e-6, 1 / (1 - 2e-6)), glow.LogitTransform(), glow.Squeeze()).to(dev)
    k = boundary.image_boundary_constants()
    layers = list(boundary)
    enc = dict(mult=k["mult"], lo=k["lo"], hi=k["hi"], hi_comp=k["hi_comp"])
    dec = dict(inv_mult=k["inv_mult"], off=k["off"], hi=k["hi"])
    with torch.no_grad():
        for shape in SHAPES:
            B, C, H, W = shape
            torch.manual_seed(sum(shape))
            px8 = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
            px = px8.float()
            ldc = -C * H * W * k["sum_log_scale"]
            def layered_encode():
                x, total = px, 0
                for m in layers:
                    x, ld = m(x)
                    total = total + ld
                return x, total
            def fused(img):
                return ops.finc_image_encode(img, torch.rand(shape, dtype=torch.float32, device=dev), logdet_const=ldc, **enc)
            z = fused(px8)[0]
            def layered_decode():
                x = z
                for m in reversed(layers):
                    x = m.reverse(x)
                return x
            assert ops.finc_image_decode(z, **dec).shape == layered_decode().shape == px.shape
            say(f"B{B} C{C} {H}x{W}, 7 rounds of 20 calls each, alternated:")
            e = legs(f"encode {shape}", (lambda: fused(px8), lambda: fused(px), layered_encode),
                     ("finc_image_encode uint8 + rand (2 launches + reduce)", "finc_image_encode fp32 + rand", "the layers' sequence (what the flag-off model runs)"))
            d = legs(f"decode {shape}", (lambda: ops.finc_image_decode(z, **dec), lambda: ops.finc_image_decode(z, dtype=torch.uint8, **dec),
                                         layered_decode, lambda: layered_decode().clamp(0, 255).to(torch.uint8)),
                     ("finc_image_decode fp32 (1 launch)", "finc_image_decode uint8 (1 launch)", "the layers' reverses", "the layers' reverses + clamp + cast"))
            say(f"    encode: fused / layers {e[0] / e[2]:.3f} (uint8), {e[1] / e[2]:.3f} (fp32); decode: fused / layers {d[0] / d[2]:.3f} (fp32), "
                f"{d[1] / d[3]:.3f} (uint8)")
            del px8, px, z
            torch.cuda.empty_cache()
        torch.manual_seed(1); np.random.seed(1)
        model = glow.create_model(num_blocks=2, block_size=1, actnorm=True, split_prior=True, image_size=(3, 16, 16), coupling_width=16).to(dev)
        pixels = torch.randint(0, 256, (256, 3, 16, 16), dtype=torch.uint8, device=dev)
        model(pixels.float())                        # (ActNorm's data-dependent initialisation)
        def flagged(flag, fn):
            def run():
                model.fuse_image_boundary = flag
                return fn()
            return run
        say("model: 2 blocks of 1 step, split prior, 3x16x16, B256, no graph; 7 rounds of 10 passes each, alternated:")
        lp = legs("log_prob", (flagged(True, lambda: model.log_prob(pixels)), flagged(False, lambda: model.log_prob(pixels.float()))),
                  ("flag on (uint8 in)", "flag off (fp32 in)"), n=10)
        sm = legs("sample(256)", (flagged(True, lambda: model.sample(256)), flagged(False, lambda: model.sample(256))), ("flag on", "flag off"), n=10)
        say(f"    the prefix's share of a flag-off log_prob: {(lp[1] - lp[0]) / lp[1]:.3f} of it goes with the flag; "
            f"the tail's share of a flag-off sample: {(sm[1] - sm[0]) / sm[1]:.3f}")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_image_boundary.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(out_dir, "time_image_boundary.json"), "w") as f:
        json.dump(results, f, indent=1)
if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "image_boundary"))
