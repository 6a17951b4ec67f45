"""Register metadata of the built library's finc_wave_kernel instantiations (scripts/kernel_regs.py; no GPU): none may spill or use
scratch, and a helper-wave form (512 threads per workgroup: two roles share a wave's 256 + 256 registers, hipcc splits them 128 : 128
per role pair) must stay within 128 architectural VGPRs.  In those forms a spilled in-flight load destination is a wrong result, not
a slow one (finc_mfma.hip, hlp_fits), and stage 2 of the paired tile (finc_pair2_form) spends 4 VGPRs of that budget that no
compile-time formula covers."""
import os
import re
import subprocess
import sys

import pytest

from helpers import REPO

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def rows():
    lib = os.path.join(REPO, "fincflow_amd", "libfinc_hip.so")
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(lib)):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "kernel_regs.py"), "finc_wave_kernel", lib],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    got = []
    for line in out.splitlines():
        m = re.search(r"agpr\s+(\d+) total\s+(\d+) spill (\d+) scratch (\d+) maxflat (\d+)", line)
        assert m, line
        got.append((line.split(" agpr")[0].strip(),) + tuple(int(v) for v in m.groups()))
    assert len(got) > 50, len(got)
    return got


def test_no_wave_kernel_spills_or_uses_scratch(rows):
    bad = [r for r in rows if r[3] or r[4]]
    assert not bad, bad


def test_helper_wave_forms_stay_within_the_128_vgpr_role_budget(rows):
    hlp = [r for r in rows if r[5] == 512]
    assert hlp, "no helper-wave form in the library"
    for name, agpr, total, _, _, _ in hlp:
        assert total - agpr <= 128 and agpr <= 128, (name, total - agpr, agpr)
