"""GPU helper: the PLU-parametrised 1x1 convolution (glow.Conv1x1LU).  HIP events, the legs of a comparison alternated in
this one process, seven rounds each: median and min .. max.  `time_plu.py [json PATH]`.

Compose, at C in {12, 48, 96, 192}: the compose launch writing W, W^-1 and the log-det (ops.finc_plu_compose); compose + backward
(ops.plu_compose under autograd, a loss on all three); each against the layer's own PyTorch lines on the same build
(Conv1x1LU._compose_torch), and beside what Conv1x1 spends on the same matrix: torch.slogdet recorded + its backward, and
torch.inverse.

Training step, [FastFlowUnit, ActNorm, mix, Coupling(width 128)] x 4 at [256, 96, 64, 64] and at [128, 12, 16, 16]: a training step
(log_prob, backward) and rsample(256) + backward with Conv1x1LU and with Conv1x1 as the mix -- two different models, a comparison of
two layers."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from fincflow_amd import FastFlowUnit, FlowSequential, glow, ops
dev = torch.device("cuda:0")
med = statistics.median
ROUNDS = 7


def timeit(fn, n):
    t_end = time.perf_counter() + 0.2        # clocks ramp up over the first tenths of a second of load
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def legs(title, named, n, out):
    """Every leg once per round, in turn, ROUNDS rounds."""
    times = {name: [] for name, _ in named}
    for _ in range(ROUNDS):
        for name, fn in named:
            times[name].append(timeit(fn, n))
    print(title, flush=True)
    for name, v in times.items():
        print(f"  {name:58s} {med(v):10.1f} us   (min {min(v):.1f} .. max {max(v):.1f})", flush=True)
    out[title] = {name: {"us": v, "median_us": med(v)} for name, v in times.items()}


results = {}
for C in (12, 48, 96, 192):
    np.random.seed(C); torch.manual_seed(C)
    lu = glow.Conv1x1LU(C).to(dev)
    with torch.no_grad():
        lu.lower.add_(0.05 * torch.randn(C, C, device=dev).tril(-1)); lu.upper.add_(0.05 * torch.randn(C, C, device=dev).triu(1))
        lu.log_s.add_(0.1 * torch.randn(C, device=dev))
        W = lu.dense().detach().clone().requires_grad_(True)
    a, b = torch.randn(C, C, device=dev), torch.randn(C, C, device=dev)
    frozen = [p.detach() for p in (lu.lower, lu.upper, lu.log_s)]

    def kernel_fwd():
        ops.finc_plu_compose(*frozen, lu.sign_s, lu.perm)

    def torch_fwd():
        with torch.no_grad():
            lu._compose_torch()

    def both(compose):
        for p in lu.parameters(): p.grad = None
        w, w_inv, ld = compose()
        ((w * a).sum() + (w_inv * b).sum() + 3.0 * ld).backward()

    def dense_slogdet():
        W.grad = None
        torch.slogdet(W)[1].backward()

    def dense_inverse():
        with torch.no_grad():
            torch.inverse(W)
    legs(f"compose C={C}", [
        ("HIP: compose (W, W^-1, log-det), one launch", kernel_fwd),
        ("PyTorch lines: the same three", torch_fwd),
        ("HIP: compose + backward (ops.plu_compose)", lambda: both(lambda: ops.plu_compose(lu.lower, lu.upper, lu.log_s, lu.sign_s, lu.perm))),
        ("PyTorch lines: compose + backward", lambda: both(lu._compose_torch)),
        ("Conv1x1: torch.slogdet recorded + backward", dense_slogdet),
        ("Conv1x1: torch.inverse", dense_inverse),
    ], 50, results)


def stack(C, H, W, lu_mix):
    np.random.seed(3); torch.manual_seed(3)
    layers = []
    for _ in range(4):
        an = glow.ActNorm(C)
        with torch.no_grad():
            an.log_scale.copy_(0.1 * torch.randn(C)); an.translation.copy_(0.1 * torch.randn(C))
        an.mark_initialized()
        layers += [FastFlowUnit(C, C, (3, 3)), an, glow.Conv1x1LU(C) if lu_mix else glow.Conv1x1(C), glow.Coupling((C, H, W), width=128)]
    return FlowSequential(glow.GaussianPrior((C, H, W)), *layers).to(dev)


for (B, C, H, W) in ((128, 12, 16, 16), (256, 96, 64, 64)):
    models = {"Conv1x1LU": stack(C, H, W, True), "Conv1x1": stack(C, H, W, False)}
    x = torch.randn(B, C, H, W, device=dev)

    def train(m):
        m.zero_grad(set_to_none=True)
        (-m.log_prob(x).mean()).backward()

    def rsample(m):
        m.zero_grad(set_to_none=True)
        m.rsample(256).square().mean().backward()
    named = [(f"{kind}: {name}", (lambda m=m, fn=fn: fn(m))) for name, fn in (("training step", train), ("rsample(256) + backward", rsample))
             for kind, m in models.items()]
    legs(f"[FastFlowUnit, ActNorm, mix, Coupling] x 4 at [{B}, {C}, {H}, {W}]", named, 3 if C == 96 else 20, results)
    del models, x
    torch.cuda.empty_cache()

if len(sys.argv) > 2 and sys.argv[1] == "json":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(results, f, indent=1)
