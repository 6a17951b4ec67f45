#!/usr/bin/env python3
"""Per-step instruction mix of the compute role's loop, and per-kernel identity of two builds, from device assembly (no GPU).

    hipcc -O3 -fPIC --offload-arch=gfx950 -std=c++20 -mllvm -amdgpu-mfma-vgpr-form -DFINC_EXPERIMENT -DFINC_ONLY_C3 \
          --cuda-device-only -S fincflow_amd/csrc/finc_mfma.hip -o new.s            (the flags of scripts/build_variant.sh)
    scripts/step_isa.py mix new.s [kernel-substring]     the loop that holds the kernel's MFMAs (8 steps), hot path only:
                                                         basic blocks that carry the "cold path" marker (FINC_COLD) are left out
    scripts/step_isa.py same parent.s new.s              every finc_wave_kernel / pack_kernel: identical body or not, registers
"""
import collections
import re
import subprocess
import sys

HEADLINE = "finc_wave_kernelILi24ELi3ELi3ELb1ELi1ELi1ELi3ELi1ELb0EE"     # <24,3,3,true,1,1,3,1,false>: bench.py's c3


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is not None:
            out[cur].append(line.rstrip("\n"))
            if line.strip().startswith(".Lfunc_end"):
                cur = None
    return out


def klass(op):
    if op.startswith("v_mfma_f32_16x16x4"): return "v_mfma_f32_16x16x4"
    if op.startswith("v_mfma_f32_4x4x1"): return "v_mfma_f32_4x4x1_16b"
    if op.startswith("v_permlane"): return "v_permlane*_swap"
    if op.startswith("v_"): return "VALU without the lane swaps"
    if op == "s_nop": return "s_nop"
    if op.startswith("s_waitcnt"): return "s_waitcnt"
    if op.startswith("s_cbranch") or op.startswith("s_branch"): return "branches"
    if op.startswith("ds_"): return "LDS"
    if op.startswith("s_"): return "SALU"
    return "other"


def mix(path, key):
    body = next(v for k, v in functions(path).items() if key in k)
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    # a cold block laid out behind the loop ends in a branch back into it: that is no loop latch
    cold_line, start = [False] * len(body), 0
    for i, l in enumerate(body + [".LBB0_0:"]):
        if re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %bb\.", l):
            if any("cold path" in x for x in body[start:i]):
                cold_line[start:i] = [True] * (i - start)
            start = i
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(?:\S+,\s*)?(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i and not cold_line[i]:
            a = labels[m.group(1)]
            loops.append((sum("v_mfma" in x for x in body[a:i]), a, i))
    most = max(n for n, _, _ in loops)
    n, a, b = min((c for c in loops if c[0] >= 0.9 * most), key=lambda c: c[2] - c[1])   # the innermost loop with (nearly) all MFMAs
    blocks = [[]]
    for l in body[a:b + 1]:
        if re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %bb\.", l):
            blocks.append([])
        blocks[-1].append(l)
    hot = [l for blk in blocks if not any("cold path" in x for x in blk) for l in blk]
    cls, ops = collections.Counter(), collections.Counter()
    for l in hot:
        m = re.match(r"^\s+([a-z_0-9]+)", l)
        if not m or l.strip()[0] in ".;":
            continue
        op = m.group(1)
        cls[klass(op)] += 1
        if op.startswith("v_") and not op.startswith("v_mfma"):
            ops[re.sub(r"_e(32|64)$", "", op) + (" row_shr" if "row_shr" in l else "")] += 1
    print(f"{n} MFMAs in the loop, {len(blocks)} basic blocks, {sum(any('cold path' in x for x in blk) for blk in blocks)} cold; per step (/8):")
    for k in sorted(cls):
        print(f"  {k:30s} {cls[k] / 8:7.2f}")
    print(f"  {'all instructions':30s} {sum(cls.values()) / 8:7.2f}")
    print("VALU by opcode:")
    for k, v in ops.most_common():
        print(f"  {k:30s} {v / 8:7.2f}")


def same(pa, pb):
    ta, tb = open(pa).read(), open(pb).read()
    fa, fb = functions(pa), functions(pb)

    def regs(t, name):
        blk = t[t.find("; Kernel info:", t.find(name + ":")):][:1500]
        g = lambda k: int(re.search(r"; %s: (\d+)" % k, blk).group(1))
        return "vgpr %3d agpr %3d total %3d scratch %d" % (g("NumVgprs"), g("NumAgprs"), g("TotalNumVgprs"), g("ScratchSize"))
    for k in fa:
        if "finc_wave_kernel" not in k and "pack_kernel" not in k:
            continue
        dem = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        dem = dem.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{dem:56s} {'identical' if fa[k] == fb.get(k) else 'DIFFERS  '} | {regs(ta, k)} | {regs(tb, k) if k in fb else 'missing'}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "mix":
        mix(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else HEADLINE)
    elif len(sys.argv) == 4 and sys.argv[1] == "same":
        same(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
