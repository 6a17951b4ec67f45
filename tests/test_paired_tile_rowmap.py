"""The packer's paired remainder fragments (finc_mfma.hip pack_kernel) on the host: finc_tile.h's finc_pair_elem and
finc_pair_offset are the one statement of which (row channel, column channel, tap) element `lane` of paired fragment f holds and
where it lies in the packed buffer -- pack_kernel and the wave kernel call them.  A small host program prints that map for the
24-channel bank (and a 40-channel one: MTB = 2); numpy restates it:

    row 4qq + r of the fragment of pair p, k-step j:  r < 2 is channel 16*MTB + 4r + qq of the pair's first tap ((0,1) / (1,0)),
    r >= 2 is channel 16*MTB + 4(r-2) + qq of its partner ((0,2) / (1,1)); lane row q is the column chan_d(MTB, j, q),

and then uses the printed map as a 16x16x4 MFMA would: registers 0,1 of the product must be the first tap's channels in operand
layout, registers 2,3 the partner's.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import REPO
from wave_model import chan_d

CSRC = os.path.join(REPO, "fincflow_amd", "csrc")
FIRST, PARTNER = [(0, 1), (1, 0)], [(0, 2), (1, 1)]

SHIM = r"""
#include <cstdio>
#include <cstdlib>
#include "finc_tile.h"
int main(int argc, char **argv)
{
    if (argc == 2) {                              // "chan": chan_d over every padded bank of up to 4 tiles + 3 blocks
        for (int cqp = 4; cqp <= 76; cqp += 4)
            for (int j = 0; j < cqp / 4; ++j)
                for (int q = 0; q < 4; ++q) printf("C %d %d %d %d\n", cqp, j, q, chan_d(cqp / 16, j, q));
        return 0;
    }
    const int cqp = atoi(argv[1]), G = atoi(argv[2]), npack = atoi(argv[3]);
    const int MTB = cqp / 16, NKD = cqp / 4, npair = 2 * NKD;
    printf("B %d\n", finc_pair_bank(cqp, 3, 3) ? 1 : 0);
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
    d = tmp_path_factory.mktemp("pair_shim")
    src = d / "pair_shim.hip"
    src.write_text(SHIM)
    exe = d / "pair_shim"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++20", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)

    def run(cqp, G, npack):
        out = subprocess.run([str(exe), str(cqp), str(G), str(npack)], check=True, capture_output=True, text=True, timeout=60).stdout
        rows = [l.split() for l in out.splitlines()]
        bank = [int(r[1]) for r in rows if r[0] == "B"][0]
        elems = {(int(r[1]), int(r[2])): tuple(int(v) for v in r[3:]) for r in rows if r[0] == "E"}
        offs = {(int(r[1]), int(r[2])): int(r[3]) for r in rows if r[0] == "O"}
        return bank, elems, offs

    def chan():
        out = subprocess.run([str(exe), "chan"], check=True, capture_output=True, text=True, timeout=60).stdout
        return {tuple(int(v) for v in l.split()[1:4]): int(l.split()[4]) for l in out.splitlines()}
    run.chan = chan
    return run


@pytest.mark.parametrize("cqp", [24, 40])
def test_paired_fragment_rows_match_the_row_map(cqp, shim):
    MTB, NKD = cqp // 16, cqp // 4
    bank, elems, _ = shim(cqp, 1, 1)
    assert bank == 1
    assert len(elems) == 2 * NKD * 64
    for p in range(2):
        for j in range(NKD):
            for lane in range(64):
                q, qq, r = lane >> 4, (lane & 15) >> 2, lane & 3
                tap = FIRST[p] if r < 2 else PARTNER[p]
                want = (16 * MTB + 4 * (r % 2) + qq, j, q) + tap
                assert elems[(p * NKD + j, lane)] == want, (p, j, lane)
                # registers 0,1 of the product are operand registers 4*MTB + r of the solved pixel, k-slot = lane row qq
                if r < 2:
                    assert want[0] == chan_d(MTB, 4 * MTB + r, qq)


def test_chan_d_matches_the_wave_model_and_is_a_bijection(shim):
    """finc_tile.h's chan_d -- the one definition the packer, the compute waves and the store side of finc_mfma.hip, finc_split.hip and
    finc_chain.hip read -- against its Python twin: MTB = 0 .. 4 tiles, 0 .. 3 blocks behind them, every k-step and k-slot; and over
    those (j, q) it names every channel of the padded bank exactly once."""
    got = shim.chan()
    banks = [16 * mtb + r for mtb in range(5) for r in (0, 4, 8, 12) if 16 * mtb + r]
    assert sorted({c for c, _, _ in got}) == banks
    for cqp in banks:
        MTB, NK = cqp // 16, cqp // 4
        vals = [got[(cqp, j, q)] for j in range(NK) for q in range(4)]
        assert vals == [chan_d(MTB, j, q) for j in range(NK) for q in range(4)], cqp
        assert sorted(vals) == list(range(cqp)), cqp


def test_banks_that_pair(shim):
    assert [c for c in (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64) if shim(c, 1, 1)[0]] == [24, 40, 56]


def test_paired_tile_product_is_first_tap_now_and_partner_next(shim):
    """D = sum_j A_j B_j with A from the printed map and B the operand of a solved pixel (k-slot q of k-step j = channel
    chan_d(MTB, j, q)): D[4qq + r] is the first tap's channel 16 + 4r + qq for r < 2, the partner's channel 16 + 4(r-2) + qq else."""
    cqp, MTB, NKD = 24, 1, 6
    _, elems, _ = shim(cqp, 1, 1)
    rng = np.random.default_rng(0)
    M = {tap: rng.standard_normal((cqp, cqp)) for tap in FIRST + PARTNER}      # the packer's -Linv W_tap, any matrices here
    x = rng.standard_normal(cqp)
    for p in range(2):
        D = np.zeros(16)
        for j in range(NKD):
            for i in range(16):
                for q in range(4):
                    row, jj, qq_, a, b = elems[(p * NKD + j, 16 * q + i)]
                    D[i] += M[(a, b)][row, chan_d(MTB, jj, qq_)] * x[chan_d(MTB, j, q)]
        for qq in range(4):
            for r in range(4):
                tap = FIRST[p] if r < 2 else PARTNER[p]
                np.testing.assert_allclose(D[4 * qq + r], (M[tap] @ x)[16 + 4 * (r % 2) + qq], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("G", [1, 4])
def test_paired_fragments_lie_behind_the_banks_of_all_groups(G, shim):
    """pack_kernel's offset: G banks of npack fragments first, then npair fragments per group, 64 floats each, none shared."""
    npack, npair = 162 + 24, 12                  # Cfg<24,3,3>: NFRAGT = (6 + 8*6) * 3 fragments, 8*MT bias and zero registers
    _, _, offs = shim(24, G, npack)
    assert len(offs) == G * npair
    for (g, f), o in offs.items():
        assert o == (G * npack + g * npair + f) * 64
    assert sorted(offs.values()) == [(G * npack + k) * 64 for k in range(G * npair)]
