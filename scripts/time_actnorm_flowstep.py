"""GPU helper: one training step of the flow step users run -- [FastFlowUnit, ActNorm, Conv1x1] at c3's shape (C = 96, 64x64,
B = 256), log_prob(x).mean().backward() -- on THIS tree against another tree of the project (the parent commit, checked out and built
side by side), each run in a fresh child process that imports the package and loads the library of its own tree, runs alternated
(other, this, other, this, ...), as profiles/coupling/bench_c4_alternated.json was made.

    python scripts/time_actnorm_flowstep.py OTHER_TREE [json PATH]     # four runs of each
    python scripts/time_actnorm_flowstep.py child TREE                  # one run, one JSON line (what the driver starts)
"""
import json, os, statistics, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def child(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np, torch
    import fincflow_amd
    from fincflow_amd import FastFlowUnit, FlowSequential, _lib, glow, ops
    from fincflow_amd.layers import StandardNormal
    assert os.path.abspath(fincflow_amd.__file__).startswith(os.path.abspath(tree) + os.sep), fincflow_amd.__file__
    dev = torch.device("cuda:0")
    B, C, H, W = 256, 96, 64, 64
    torch.manual_seed(4); np.random.seed(4)
    an = glow.ActNorm(C)
    seq = FlowSequential(StandardNormal((C, H, W)), FastFlowUnit(C, C, 3), an, glow.Conv1x1(C)).to(dev)
    with torch.no_grad():
        an.log_scale.copy_(0.2 * torch.randn(C, device=dev)); an.translation.copy_(torch.randn(C, device=dev)); an.mark_initialized()
    x = torch.randn(B, C, H, W, device=dev)
    def step():
        seq.zero_grad(set_to_none=True)
        seq.log_prob(x).mean().backward()
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:
        step(); torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10): step()
        b.record(); torch.cuda.synchronize()
        rounds.append(a.elapsed_time(b) / 10)
    print(json.dumps({"ms_per_step": statistics.median(rounds), "rounds_ms": rounds, "finc_version": int(_lib.lib().finc_version()),
                      "hip_actnorm": hasattr(ops, "finc_actnorm"), "fault_pending": bool(_lib.fault_pending())}))
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
    out = {"what": "[FastFlowUnit, ActNorm, Conv1x1] B256 C96 64x64, log_prob(x).mean().backward(): parent commit and this commit built "
                   "side by side on one MI355X, fresh processes, runs alternated (parent, this, parent, this, ...)", "runs": runs}
    for name in ("parent commit", "this commit"):
        v = [q["ms_per_step"] for q in runs if q["build"] == name]
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
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
    else:
        driver(sys.argv[1], sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "json" else None)
