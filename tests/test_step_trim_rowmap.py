"""Stage 2 of the paired remainder tile (finc_mfma.hip): a third pair, taps (2,0)|(2,1) on row_shr:2 of the solved
pixel, whose NKD fragments per group lie behind the 2*NKD of the pairs (0,1)|(0,2) and (1,0)|(1,1).  finc_tile.h's finc_pair_elem
and finc_pair_offset stay the one statement of the map; a small host program prints it for 3*NKD fragments and numpy restates it:

    fragment f = pair * NKD + j; row 4qq + r: r < 2 is channel 16*MTB + 4r + qq of the pair's first tap ((0,1) / (1,0) / (2,0)),
    r >= 2 is channel 16*MTB + 4(r-2) + qq of its partner ((0,2) / (1,1) / (2,1)); lane row q is the column chan_d(MTB, j, q).

The first 2*NKD fragments must be what they were (tests/test_paired_tile_rowmap.py holds them to the same statement with
npair = 2*NKD); the third pair's product must put (2,0) into registers 0,1 -- the pixel the tile is opened for -- and (2,1) into
registers 2,3 -- the pixel after it.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import REPO
from wave_model import chan_d

CSRC = os.path.join(REPO, "fincflow_amd", "csrc")
FIRST, PARTNER = [(0, 1), (1, 0), (2, 0)], [(0, 2), (1, 1), (2, 1)]

SHIM = r"""
#include <cstdio>
#include <cstdlib>
#include "finc_tile.h"
int main(int argc, char **argv)
{
    const int cqp = atoi(argv[1]), G = atoi(argv[2]), npack = atoi(argv[3]);
    const int MTB = cqp / 16, NKD = cqp / 4, npair = 3 * NKD;
    for (int f = 0; f < npair; ++f)
        for (int lane = 0; lane < 64; ++lane) {
            int row, j, q, a, b;
            finc_pair_elem(MTB, NKD, f, lane, &row, &j, &q, &a, &b);
            printf("E %d %d %d %d %d %d %d\n", f, lane, row, j, q, a, b);
        }
    for (int g = 0; g < G; ++g)
        for (int f = 0; f < npair; ++f) printf("O %d %d %zu\n", g, f, finc_pair_offset(G, npack, npair, g, f));
    return 0;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this box")
    d = tmp_path_factory.mktemp("pair2_shim")
    src = d / "pair2_shim.hip"
    src.write_text(SHIM)
    exe = d / "pair2_shim"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++20", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)

    def run(cqp, G, npack):
        out = subprocess.run([str(exe), str(cqp), str(G), str(npack)], check=True, capture_output=True, text=True, timeout=60).stdout
        rows = [l.split() for l in out.splitlines()]
        elems = {(int(r[1]), int(r[2])): tuple(int(v) for v in r[3:]) for r in rows if r[0] == "E"}
        offs = {(int(r[1]), int(r[2])): int(r[3]) for r in rows if r[0] == "O"}
        return elems, offs
    return run


@pytest.mark.parametrize("cqp", [24, 40])
def test_three_pairs_match_the_row_map(cqp, shim):
    MTB, NKD = cqp // 16, cqp // 4
    elems, _ = shim(cqp, 1, 1)
    assert len(elems) == 3 * NKD * 64
    for p in range(3):
        for j in range(NKD):
            for lane in range(64):
                q, qq, r = lane >> 4, (lane & 15) >> 2, lane & 3
                tap = FIRST[p] if r < 2 else PARTNER[p]
                assert elems[(p * NKD + j, lane)] == (16 * MTB + 4 * (r % 2) + qq, j, q) + tap, (p, j, lane)


def test_third_pair_opens_the_tile_of_the_next_pixel(shim):
    """What the kernel relies on, in numbers: with x = row_shr:2 of a solved pixel as the B operand, D = sum_j A_j B_j of the third
    pair is tap (2,0)'s share of the remainder channels in registers 0,1 (operand layout: channel 16 + 4r + qq in lane row qq)
    and tap (2,1)'s in registers 2,3."""
    cqp, MTB, NKD = 24, 1, 6
    elems, _ = shim(cqp, 1, 1)
    rng = np.random.default_rng(2)
    M = {tap: rng.standard_normal((cqp, cqp)) for tap in (FIRST[2], PARTNER[2])}
    x = rng.standard_normal(cqp)
    D = np.zeros(16)
    for j in range(NKD):
        for i in range(16):
            for q in range(4):
                row, jj, qq_, a, b = elems[(2 * NKD + j, 16 * q + i)]
                D[i] += M[(a, b)][row, chan_d(MTB, jj, qq_)] * x[chan_d(MTB, j, q)]
    for qq in range(4):
        for r in range(4):
            tap = FIRST[2] if r < 2 else PARTNER[2]
            np.testing.assert_allclose(D[4 * qq + r], (M[tap] @ x)[16 + 4 * (r % 2) + qq], rtol=1e-12, atol=1e-12)
            if r < 2:       # registers 0,1 are operand registers 4*MTB + r of the pixel: k-slot = lane row qq
                assert 16 + 4 * r + qq == chan_d(MTB, 4 * MTB + r, qq)


@pytest.mark.parametrize("G", [1, 4])
def test_three_pairs_lie_behind_the_banks_of_all_groups(G, shim):
    """G banks of npack fragments first, then 3*NKD paired fragments per group, 64 floats each, none shared; the third pair of a
    group directly behind its first two."""
    npack, npair = 162 + 24, 18                  # Cfg<24,3,3>: NFRAGT = (6 + 8*6) * 3 fragments, 8*MT bias and zero registers
    _, offs = shim(24, G, npack)
    assert len(offs) == G * npair
    for (g, f), o in offs.items():
        assert o == (G * npack + g * npair + f) * 64
    assert sorted(offs.values()) == [(G * npack + k) * 64 for k in range(G * npair)]
