#!/usr/bin/env python3
"""Compare the kernels of two gfx950 code objects (no GPU): `isa_compare.py OLD.co NEW.co [--rename PATTERN=REPLACEMENT ...]`, each made
from a source file with the Makefile's flags plus `--cuda-device-only -c`.  Per kernel: the instruction count, a sha256 over the instruction text of
llvm-objdump -d with addresses and branch targets' addresses removed, and the metadata note (registers, LDS, scratch, spills).  A
kernel whose text or metadata differs is listed with both sides and its opcode histogram difference.  Kernels pair by their demangled
name without the parameter list (`(anonymous namespace)::` first where there is one); a --rename is a regular expression and its
replacement (re.sub) for an OLD name, and the first one that matches a name is the one applied to it."""
import collections, hashlib, re, subprocess, sys
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(path):
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = dict(
            vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), sgpr=g("sgpr_count"), lds=g("group_segment_fixed_size"),
            scratch=g("private_segment_fixed_size"), spills=(g("sgpr_spill_count"), g("vgpr_spill_count")))
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    code, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            name = m.group(1)
            code[name] = []
        elif name and line.startswith("\t"):
            ins = re.sub(r"\s*//.*$", "", line.strip())            # drop the address comment
            code[name].append(re.sub(r"<[^>]*>", "<L>", ins))      # and the label offsets of branches
    return meta, code


def demangled(symbols, renames=()):
    """{name without the parameter list (and the return type c++filt puts before a template's): symbol}"""
    out = {}
    for k in symbols:
        dem = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^void ", "", dem[:dem.rindex("(")] if dem.endswith(")") else dem)
        for pat, rep in renames:
            if re.search(pat, name):
                name = re.sub(pat, rep, name)
                break
        out[name] = k
    return out


def main(old, new, renames=()):
    (ma, ca), (mb, cb) = kernels(old), kernels(new)
    na, nb = demangled(ma, renames), demangled(mb)
    print(f"kernel symbols: old {len(ma)}, new {len(mb)}, only in old {sorted(set(na) - set(nb))}, only in new {sorted(set(nb) - set(na))}")
    for pat, rep in renames:
        print(f"renamed: {pat} -> {rep}")
    differ = 0
    for dem in sorted(set(na) & set(nb)):
        ka, kb = na[dem], nb[dem]
        ha, hb = (hashlib.sha256("\n".join(c[k]).encode()).hexdigest()[:16] for c, k in ((ca, ka), (cb, kb)))
        same = ha == hb and ma[ka] == mb[kb]
        differ += not same
        if same:                                                     # one line: the name without its parameter list
            m = ma[ka]
            print(f"SAME  {dem[:90]}  instructions {len(ca[ka])} sha256 {ha} vgpr {m['vgpr']} sgpr {m['sgpr']} "
                  f"lds {m['lds']} scratch {m['scratch']} spills {m['spills'][0]}+{m['spills'][1]}")
            continue
        print(f"DIFF  {dem}")
        for tag, m, c, h in (("old", ma[ka], ca[ka], ha), ("new", mb[kb], cb[kb], hb)):
            print(f"      {tag:4s} instructions {len(c):4d} sha256 {h} vgpr {m['vgpr']} agpr {m['agpr']} sgpr {m['sgpr']} lds {m['lds']} "
                  f"scratch {m['scratch']} spills {m['spills'][0]}+{m['spills'][1]}")
        oa, ob = (collections.Counter(i.split()[0] for i in c[k]) for c, k in ((ca, ka), (cb, kb)))
        d = {o: ob[o] - oa[o] for o in sorted(set(oa) | set(ob)) if ob[o] != oa[o]}
        print("      opcode histogram, new - old: " + (", ".join(f"{o} {n:+d}" for o, n in d.items()) or "none (order / registers only)"))
    print(f"VERDICT: {differ} of {len(set(na) & set(nb))} common kernels differ in disassembly or metadata")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="PATTERN=REPLACEMENT")
    a = ap.parse_args()
    main(a.old, a.new, [tuple(r.split("=", 1)) for r in a.rename])
