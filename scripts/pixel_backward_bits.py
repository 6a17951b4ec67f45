"""GPU helper: the bits of the per-pixel layers' backward entry points, for a comparison between two builds of the library.

    python scripts/pixel_backward_bits.py OUT.json [NAME]                 # one run, against the library FINCFLOW_LIB names (or the tree's own)
    python scripts/pixel_backward_bits.py compare DIR NAME=LIB NAME=LIB   # one fresh process per library (`_lib` keeps one handle per
                                                                          # process): DIR/bits_NAME.json each and DIR/bits_compare.txt

A run calls every one of the seven backward entry points, finc_coupling_f32 in both directions and finc_coupling_reverse_logdet_f32 on
seeded finite inputs and writes a sha256 per output tensor (its first 16 hex digits, as the ISA records under profiles/ do).  Cases: both vector forms (16-byte pieces, dwords -- by shape, and by a
view offset by one float) with one partial per sum and with two, the shapes of scripts/time_{coupling,actnorm,reverse_backward,
invertible_backward}.py, each with grad_logdet given and None, with every output asked for, and in the
in-place forms the entry points allow (x_out == y, grad_x == grad_y)."""
import hashlib, json, os, subprocess, sys
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, C, H, W), offset view.  One partial: 2x4x4x4 (ActNorm also C = 3); dwords by shape: 3x5; Q = 2: 3x{4,3}x20x20 (16-byte), 3x9x11
# (dwords); dwords by alignment: HW % 4 == 0 behind one float; then the timing scripts' shapes.
CASES = [((2, 4, 4, 4), False), ((2, 3, 4, 4), False), ((2, 4, 3, 5), False), ((2, 3, 3, 5), False), ((3, 4, 20, 20), False),
         ((3, 3, 20, 20), False), ((3, 4, 9, 11), False), ((3, 3, 9, 11), False), ((2, 4, 4, 4), True), ((3, 4, 20, 20), True),
         ((128, 12, 16, 16), False), ((128, 24, 8, 8), False), ((128, 48, 4, 4), False), ((256, 96, 64, 64), False)]


def run(path, name):
    sys.path.insert(0, HERE)
    import torch
    from fincflow_amd import _lib, ops
    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    digests = {}

    def put(key, names, tensors):
        torch.cuda.synchronize()
        for n, t in zip(names, tensors):
            if t is not None:
                assert bool(torch.isfinite(t).all()), (key, n)
                digests.setdefault(tag, {}).setdefault(key, {})[n] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

    def place(t, offset):
        """`t` on the device: its own allocation (256-byte aligned), or a contiguous view one float into a larger one."""
        if not offset:
            return t.to(dev)
        buf = torch.zeros(t.numel() + 1, device=dev)
        buf[1:].copy_(t.flatten())
        return buf[1:].view(t.shape)

    for shape, offset in CASES:
        B, C, H, W = shape
        tag = "x".join(map(str, shape)) + ("+1float" if offset else "")
        g = torch.Generator().manual_seed(1000 + sum(shape) + offset)
        rnd = lambda *s: torch.randn(*s, generator=g)
        x, gy, raw = place(rnd(*shape), offset), place(rnd(*shape), offset), place(1.5 * rnd(*shape), offset)
        gl = rnd(B).to(dev)
        a, b = torch.exp(0.3 * rnd(C)).to(dev), (0.3 * rnd(C)).to(dev)
        ls, tr = (0.2 * rnd(C)).to(dev), rnd(C).to(dev)
        if C % 2 == 0:
            y, ld = ops.finc_coupling(x, raw, a, b, 1, True, out=place(torch.zeros(shape), offset))
            put(f"coupling_f32/+1", ("y", "logdet"), (y, ld))
            r = ops.finc_coupling(x, raw, a, b, -1, False, out=place(torch.zeros(shape), offset))[0]
            put(f"coupling_f32/-1", ("y",), (r,))
            put(f"coupling_reverse_logdet_f32", ("y", "logdet"),
                ops.finc_coupling_reverse_logdet(x, raw, a, b, out=place(torch.zeros(shape), offset)))
            names = ("grad_x", "grad_raw", "grad_a", "grad_b")
            for glv, k in ((gl, "gld"), (None, "nogld")):
                put(f"coupling_backward_f32/{k}", names, ops.finc_coupling_backward(gy, glv, x, raw, a, b))
                put(f"coupling_reverse_logdet_backward_f32/{k}", names, ops.finc_coupling_reverse_logdet_backward(gy, glv, r, raw, a, b))
                put(f"coupling_backward_reconstruct_f32/{k}", ("x",) + names, ops.finc_coupling_backward_reconstruct(gy, glv, y, raw, a, b))
            put("coupling_reverse_backward_f32", names, ops.finc_coupling_reverse_backward(gy, r, raw, a, b))
            # in place: x_out == y and grad_x == grad_y, straight at the entry point (the wrapper allocates its outputs)
            for glv, gtag in ((gl, "gld"), (None, "nogld")):
                yb, gyb, graw, ga, gb = y.clone(), gy.clone(), torch.empty_like(raw), torch.empty(C, device=dev), torch.empty(C, device=dev)
                nbytes = L.finc_coupling_workspace_bytes(B, C, H * W)
                st = L.finc_coupling_backward_reconstruct_f32(gyb.data_ptr(), ops._ptr(glv), yb.data_ptr(), raw.data_ptr(), a.data_ptr(),
                                                              b.data_ptr(), yb.data_ptr(), gyb.data_ptr(), graw.data_ptr(), ga.data_ptr(),
                                                              gb.data_ptr(), B, C, H * W, *ops._ws_args(dev, nbytes), stream())
                assert st == 0, st
                put(f"coupling_backward_reconstruct_f32/{gtag}/in_place", ("x",) + names, (yb, gyb, graw, ga, gb))
        yn = ops.finc_actnorm(x, ls, tr, 1, True, out=place(torch.zeros(shape), offset))[0]
        names = ("grad_x", "grad_log_scale", "grad_translation")
        for glv, k in ((gl, "gld"), (None, "nogld")):
            put(f"actnorm_backward_f32/{k}", names, ops.finc_actnorm_backward(gy, glv, yn, ls))
            put(f"actnorm_backward_reconstruct_f32/{k}", ("x",) + names, ops.finc_actnorm_backward_reconstruct(gy, glv, yn, ls, tr))
        put("actnorm_reverse_backward_f32", names, ops.finc_actnorm_reverse_backward(gy, x, ls))
        nbytes = L.finc_actnorm_workspace_bytes(B, C, H * W)
        for glv, gtag in ((gl, "gld"), (None, "nogld")):
            yb, gyb, gls, gt = yn.clone(), gy.clone(), torch.empty(C, device=dev), torch.empty(C, device=dev)
            st = L.finc_actnorm_backward_reconstruct_f32(gyb.data_ptr(), ops._ptr(glv), yb.data_ptr(), ls.data_ptr(), tr.data_ptr(), yb.data_ptr(),
                                                         gyb.data_ptr(), gls.data_ptr(), gt.data_ptr(), B, C, H * W, *ops._ws_args(dev, nbytes),
                                                         stream())
            assert st == 0, st
            put(f"actnorm_backward_reconstruct_f32/{gtag}/in_place", ("x",) + names, (yb, gyb, gls, gt))
            gyb, gls, gt = gy.clone(), torch.empty(C, device=dev), torch.empty(C, device=dev)
            st = L.finc_actnorm_backward_f32(gyb.data_ptr(), ops._ptr(glv), yn.data_ptr(), ls.data_ptr(), gyb.data_ptr(), gls.data_ptr(),
                                             gt.data_ptr(), B, C, H * W, *ops._ws_args(dev, nbytes), stream())
            assert st == 0, st
            put(f"actnorm_backward_f32/{gtag}/in_place", names, (gyb, gls, gt))
        gyb, gls, gt = gy.clone(), torch.empty(C, device=dev), torch.empty(C, device=dev)
        st = L.finc_actnorm_reverse_backward_f32(gyb.data_ptr(), x.data_ptr(), ls.data_ptr(), gyb.data_ptr(), gls.data_ptr(), gt.data_ptr(), B, C,
                                                 H * W, *ops._ws_args(dev, nbytes), stream())
        assert st == 0, st
        put(f"actnorm_reverse_backward_f32/in_place", names, (gyb, gls, gt))
    assert not _lib.fault_pending()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"library": name, "finc_version": int(L.finc_version()), "digests": digests}, f, separators=(",", ":"), sort_keys=True)
    print(f"{sum(len(t) for c in digests.values() for t in c.values())} digests -> {path}")


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
            runs.append({f"{c}/{k}/{n}": h for c, ks in json.load(f)["digests"].items() for k, ts in ks.items() for n, h in ts.items()})
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
