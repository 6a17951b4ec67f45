"""GPU helper: the bits of the float64 matrix-core entry points, for a comparison between two builds of the library.

    python scripts/f64_bits.py OUT.json [NAME]                 # one run, against the library FINCFLOW_LIB names (or the tree's own)
    python scripts/f64_bits.py compare DIR NAME=LIB NAME=LIB   # one fresh process per library (`_lib` keeps one handle per process):
                                                               # DIR/bits_NAME.json each and DIR/bits_compare.txt

A run calls finc_inverse_f64_algo and finc_forward_f64_algo under "mfma" and finc_backward_f64 (both outputs, the workspace given) on
seeded finite inputs and writes a sha256 per output tensor (its first 16 hex digits, as the ISA records under profiles/ do).  Cases:
every one of MFMA_CASES (tests/test_gpu_f64_backward.py) and CASES (tests/test_gpu_f64_wide_banks.py), imported, and the four shapes
of scripts/time_f64_wide_banks.py, read from its SHAPES line (that script measures when it is imported)."""
import ast, hashlib, json, os, re, subprocess, sys
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    """{name: ((B, G, Cq, H, W, KH, KW), orient)}"""
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from fincflow_amd import ops
    from test_gpu_f64_backward import MFMA_CASES
    from test_gpu_f64_wide_banks import CASES
    out = {**MFMA_CASES, **CASES}
    src = open(os.path.join(HERE, "scripts", "time_f64_wide_banks.py")).read()
    for tag, (B, C, H, W) in ast.literal_eval(re.search(r"^SHAPES = (.*)$", src, re.M).group(1)):
        out["time_" + tag] = ((B, 4, C // 4, H, W, 3, 3), ops.ORIENT_FASTFLOW)     # (G, K and the orientation of that script)
    return out


def run(path, name):
    sys.path.insert(0, HERE)
    import torch
    from fincflow_amd import _lib, ops
    dev = torch.device("cuda:0")
    L = _lib.lib()
    digests = {}
    for tag, (dims, orient) in cases().items():
        B, G, Cq, H, W, KH, KW = dims
        assert _lib.f64_plan(*dims)["family"] in (1, 2), tag
        g = torch.Generator().manual_seed(1000 + sum(dims) + orient)
        w = 0.05 * min(1.0, (24.0 / Cq) ** 0.5) * torch.randn(G * Cq, Cq, KH, KW, dtype=torch.float64, generator=g)
        for k in range(G):
            blk = w[k * Cq:(k + 1) * Cq, :, -1, -1]
            blk.copy_(torch.tril(blk, -1) + torch.eye(Cq, dtype=torch.float64))
        wc = w.to(dev)
        x = torch.randn(B, G * Cq, H, W, dtype=torch.float64, generator=g).to(dev)
        gz = torch.randn(B, G * Cq, H, W, dtype=torch.float64, generator=g).to(dev)
        z = ops.finc_forward(x, wc, G, orient, algo="mfma")
        back = ops.finc_inverse(x, wc, G, orient, algo="mfma")
        gx, gw = ops.finc_backward(gz, x, wc, G, orient)
        torch.cuda.synchronize()
        for n, v in (("forward", z), ("inverse", back), ("grad_x", gx), ("grad_w", gw)):
            assert bool(torch.isfinite(v).all()), (tag, n)
            digests.setdefault(tag, {})[n] = hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
        del x, gz, z, back, gx
        ops.release_workspaces()
        torch.cuda.empty_cache()
    assert not _lib.fault_pending()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"library": name, "finc_version": int(L.finc_version()), "digests": digests}, f, indent=0, sort_keys=True)
    print(f"{sum(len(c) for c in digests.values())} digests -> {path}")


def compare(out_dir, libs):
    runs = []
    libs = [l.split("=", 1) for l in libs]
    for name, lib in libs:
        path = os.path.join(out_dir, f"bits_{name}.json")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path, name], env=dict(os.environ, FINCFLOW_LIB=os.path.abspath(lib)),
                           timeout=300)
        if p.returncode != 0:                    # nothing more is started on the GPU after a failure
            sys.exit(f"{name}: exit status {p.returncode}")
        with open(path) as f:
            runs.append({f"{c}/{n}": h for c, ts in json.load(f)["digests"].items() for n, h in ts.items()})
    first, lines = runs[0], []
    for (name, _), d in zip(libs[1:], runs[1:]):
        differ = sorted(k for k in set(first) | set(d) if first.get(k) != d.get(k))
        lines.append(f"{libs[0][0]} against {name}: {len(first)} and {len(d)} digests, {len(differ)} differ")
        lines += [f"  DIFFERS {k}" for k in differ]
    with open(os.path.join(out_dir, "bits_compare.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if any("DIFFERS" in l for l in lines) else 0)


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3:])
    else:
        run(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "FINCFLOW_LIB or the tree's own")
