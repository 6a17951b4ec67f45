"""The row shifts read from LDS (finc_mfma.hip, the helper-wave paired forms): finc_tile.h's finc_ls_* functions are the
one statement of where a lane writes its solved pixel behind the x-ring write (FIFO word or its own ring cell again), where it reads
S_a from (ring cell of lane p - a, or the FIFO word of the band above), and of the per-lane constants that move the kernel's ONE
pointer per a from step to step.  A small host program prints them; numpy then runs the kernel's pointer schedule over 300 steps --
x-ring write, reads, push, advance, rewinds -- on one k-step's block of LDS and compares what the reads return with the plain
statement:

    lane (q, p), p >= a sees lane (q, p - a)'s pixel of this step;
    lane (q, p), p <  a sees lane (q, P - a + p)'s pixel of D - 1 steps ago (zeros before the first band got there), P = 16.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import REPO

CSRC = os.path.join(REPO, "fincflow_amd", "csrc")
KH, P, STEPS = 3, 16, 300

SHIM = r"""
#include <cstdio>
#include <cstdlib>
#include "finc_tile.h"
int main(int argc, char **argv)
{
    const int KH = atoi(argv[1]), P = atoi(argv[2]), D = atoi(argv[3]);
    printf("J %d %d %d\n", finc_ls_jstride(KH), finc_ls_js(KH), FINC_LS_DMAX);
    for (int lane = 0; lane < 64; ++lane) {
        const bool pu = finc_ls_pushes(KH, P, D, lane);
        printf("P %d %d %d %d %d\n", lane, finc_ls_push(KH, P, D, lane, 4, 0), finc_ls_step(KH, pu), finc_ls_rewind8(pu), finc_ls_rewindR(KH, D, pu));
        for (int a = 1; a < KH; ++a) {
            const bool po = finc_ls_pops(a, D, lane);
            printf("R %d %d %d %d %d %d\n", a, lane, finc_ls_src(KH, a, D, lane, 4, 0), finc_ls_step(KH, po), finc_ls_rewind8(po), finc_ls_rewindR(KH, D, po));
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this box")
    d = tmp_path_factory.mktemp("ls_shim")
    src = d / "ls_shim.hip"
    src.write_text(SHIM)
    exe = d / "ls_shim"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++20", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)

    def run(D):
        out = subprocess.run([str(exe), str(KH), str(P), str(D)], check=True, capture_output=True, text=True, timeout=60).stdout
        rows = [l.split() for l in out.splitlines()]
        head = [[int(v) for v in r[1:]] for r in rows if r[0] == "J"][0]
        push = np.array([[int(v) for v in r[2:]] for r in rows if r[0] == "P"])                       # [lane][addr, step, rew8, rewR]
        read = {a: np.array([[int(v) for v in r[3:]] for r in rows if r[0] == "R" and int(r[1]) == a]) for a in range(1, KH)}
        return head, push, read
    return run


def test_block_layout(shim):
    (jstride, js, dmax), _, _ = shim(49)
    assert js == 4 * (KH - 1)
    assert jstride % 64 == 0                      # two k-steps in one ds_*2st64 instruction
    assert jstride >= 8 * 64 + (dmax - 1) * js    # the x ring's 8 time slots, then the deepest FIFO ring
    assert dmax == 49                             # W = 64, P = 16
    # a wave's LDS at 24 channels: the z ring (6 k-steps x 12 slots x 64) and six such blocks; four waves and their flag words in 160 KB
    assert 4 * 4 * (6 * 12 * 64 + 6 * jstride) + 64 <= 160 * 1024


@pytest.mark.parametrize("D", [1, 17, 49])
def test_reads_return_the_shifted_rows(D, shim):
    (jstride, js, _), push, read = shim(D)
    lanes = np.arange(64)
    q, p = lanes >> 4, lanes & 15
    mem = np.zeros(jstride)                       # the block of one k-step; the kernel zero-fills the FIFO part
    slots = D - 1 if D > 1 else 1 << 30
    push_p = push[:, 0].copy()
    rd_p = {a: read[a][:, 0].copy() for a in read}
    fslot = 0

    def advance(t):
        nonlocal fslot, push_p
        fslot += 1
        push_p = push_p + push[:, 1]
        for a in rd_p:
            rd_p[a] = rd_p[a] + read[a][:, 1]
        if fslot == slots:
            fslot = 0
            push_p = push_p - push[:, 3]
            for a in rd_p:
                rd_p[a] = rd_p[a] - read[a][:, 3]
        if t & 7 == 7:
            push_p = push_p - push[:, 2]
            for a in rd_p:
                rd_p[a] = rd_p[a] - read[a][:, 2]

    for t in range(-4, 0):                        # the prologue only advances
        advance(t)
    pixels = {}
    for t in range(STEPS):
        x = 1.0 + t * 64 + lanes                  # every (step, lane) its own value
        pixels[t] = x
        mem[(t & 7) * 64 + lanes] = x             # the x-ring write of the step
        for a, ptr in rd_p.items():
            assert ptr.min() >= 0 and ptr.max() < jstride
            got = mem[ptr]
            old = pixels.get(t - (D - 1))
            want = np.where(p >= a, x[np.maximum(lanes - a, 0)], 0.0 if old is None else old[np.minimum(16 * q + P - a + p, 63)])
            np.testing.assert_array_equal(got, want, err_msg=f"D={D} t={t} a={a}")
        assert push_p.min() >= 0 and push_p.max() < jstride
        mem[push_p] = x                           # the push (lanes that hand nothing over write their own ring cell again)
        for k in range(min(t + 1, 8)):            # the x ring still holds the pixels of the last 8 steps: what the helper wave stores
            np.testing.assert_array_equal(mem[((t - k) & 7) * 64 + lanes], pixels[t - k])
        advance(t)
