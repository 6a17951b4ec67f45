"""The strip-piece map of the grad-weight kernels (finc_gradw.hip: staged, tiled, Winograd, Winograd tile-pair) on the host:
finc_tile.h's finc_strip_piece is the one statement of which 16-byte piece of a channel row load slot t = 64 i + lane fetches, where
it lands in the LDS tile and when the slot is marked OFF_BAD_CHANNEL -- the arithmetic that keeps those kernels inside their slab.
A small host program prints (t, offset, landing address) for every slot of a case; numpy checks them against the plain statement:

    the valid slots name {channels of the window below CQ} x ({row pieces with 0 <= column < W} + {halo piece if 0 <= hm < W}), once each;
    every other slot is OFF_BAD_CHANNEL exactly; a valid piece of any row ends inside the slab;
    pieces land 16-byte aligned, inside the tile, nowhere twice, slots behind the bank in the scratch piece;
    canonical column c of the strip lies at tile column lead + c, mirrored at 4 np - 1 - c with the halo behind it
    (what the kernels' read maps xrd / grd index).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import REPO

CSRC = os.path.join(REPO, "fincflow_amd", "csrc")
BAD = 0x40000000
H = 3

SHIM = r"""
#include <cstdio>
#include "finc_tile.h"
int main()
{
    int id, n, np, rows, c0, CQ, HW, W, ms, hm, mir, pitch, lead, scratch, halo;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &id, &n, &np, &rows, &c0, &CQ, &HW, &W, &ms, &hm, &mir, &pitch, &lead,
                 &scratch, &halo) == 15)
        for (int t = 0; t < n; ++t) {
            const FincStripPiece p = finc_strip_piece(t, np, rows, c0, CQ, HW, W, ms, hm, mir != 0, pitch, lead, scratch, halo != 0);
            printf("%d %d %u %d\n", id, t, p.voff, p.lds);
        }
    return 0;
}
"""


def cases():
    """strip widths x map widths (a strip wider than the row, a ragged last strip, a halo left of column 0), every strip of the row, both
    orientations; the padded bank full and short of 3 channels, and a 16-channel window starting at 16 of a 20-channel bank; an x
    tile (lead 4, halo piece) and a gz tile (lead 0, none)"""
    out = []
    for np_, widths in ((4, (4, 12, 16, 20, 36)), (8, (8, 32, 36, 68))):
        sw = 4 * np_
        for W in widths:
            for strip in range((W + sw - 1) // sw):
                for mir in (0, 1):
                    ms = W - sw - strip * sw if mir else strip * sw
                    hm = ms + sw if mir else ms - 4
                    for rows, c0, CQ in ((24, 0, 24), (24, 0, 21), (16, 16, 20)):
                        for halo, lead in ((1, 4), (0, 0)):
                            pitch = sw + 4
                            n = 64 * (((np_ + halo) * rows + 63) // 64 + 1)          # the bank's slots and at least 64 behind them
                            out.append(dict(n=n, np=np_, rows=rows, c0=c0, CQ=CQ, HW=H * W, W=W, ms=ms, hm=hm, mir=mir, pitch=pitch,
                                            lead=lead, scratch=rows * pitch, halo=halo))
    return out


@pytest.fixture(scope="module")
def pieces(tmp_path_factory):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this box")
    d = tmp_path_factory.mktemp("piece_shim")
    src = d / "piece_shim.hip"
    src.write_text(SHIM)
    exe = d / "piece_shim"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++20", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    cs = cases()
    keys = ("n", "np", "rows", "c0", "CQ", "HW", "W", "ms", "hm", "mir", "pitch", "lead", "scratch", "halo")
    text = "".join(" ".join([str(i)] + [str(c[k]) for k in keys]) + "\n" for i, c in enumerate(cs))
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True, timeout=60).stdout
    a = np.array([[int(v) for v in l.split()] for l in out.splitlines()], dtype=np.int64)
    got = []
    for i, c in enumerate(cs):
        m = a[a[:, 0] == i]
        assert (m[:, 1] == np.arange(c["n"])).all()
        got.append((c, m[:, 2], m[:, 3]))
    return got


def expected_columns(c):
    cols = [c["ms"] + 4 * k for k in range(c["np"]) if 0 <= c["ms"] + 4 * k < c["W"]]
    if c["halo"] and 0 <= c["hm"] < c["W"]:
        cols.append(c["hm"])
    return cols


def test_cases_take_every_branch():
    cs = cases()
    assert any(c["ms"] < 0 for c in cs) and any(c["ms"] + 4 * c["np"] > c["W"] for c in cs)        # mirrored / plain ragged strips
    assert any(c["halo"] and c["hm"] < 0 for c in cs) and any(c["halo"] and c["hm"] >= c["W"] for c in cs)
    assert any(c["halo"] and 0 <= c["hm"] < c["W"] for c in cs)
    assert any(4 * c["np"] > c["W"] for c in cs) and any(c["c0"] + c["rows"] > c["CQ"] for c in cs)


def test_valid_slots_cover_the_window_once_and_the_rest_is_marked(pieces):
    for c, voff, _ in pieces:
        valid = voff != BAD
        plane = c["HW"] * 4
        ch, rest = voff[valid] // plane, voff[valid] % plane
        assert (rest % 16 == 0).all() and (rest < c["W"] * 4).all(), c          # row 0 of the channel: the row offset comes on top
        got = sorted(zip(ch.tolist(), (rest // 4).tolist()))
        want = sorted((ch_, col) for ch_ in range(c["c0"], min(c["c0"] + c["rows"], c["CQ"])) for col in expected_columns(c))
        assert got == want, c                                                    # (sorted lists: each exactly once)
        assert (voff[~valid] == BAD).all()


def test_valid_pieces_of_every_row_end_inside_the_slab(pieces):
    for c, voff, _ in pieces:
        valid = voff[voff != BAD]
        if len(valid):
            assert valid.max() + 16 + (H - 1) * c["W"] * 4 <= c["CQ"] * c["HW"] * 4, c


def test_landing_addresses(pieces):
    for c, voff, lds in pieces:
        nbank = (c["np"] + c["halo"]) * c["rows"]
        assert (lds % 4 == 0).all(), c
        bank = lds[:nbank]
        assert bank.min() >= 0 and bank.max() + 4 <= c["rows"] * c["pitch"], c
        assert len(set(bank.tolist())) == nbank, c
        assert (lds[nbank:] == c["scratch"]).all() and (voff[nbank:] == BAD).all(), c
        # canonical column of the float j of a piece at memory column mc, and the tile column the read maps expect it at
        sw = 4 * c["np"]
        for t in range(nbank):
            if t < c["np"] * c["rows"]:
                row, mc = t // c["np"], c["ms"] + 4 * (t % c["np"])
            else:
                row, mc = t - c["np"] * c["rows"], c["hm"]
            for j in range(4):
                canon = c["ms"] + sw - 1 - (mc + j) if c["mir"] else mc + j - c["ms"]
                assert -4 <= canon < sw
                want = sw - 1 - canon if c["mir"] else c["lead"] + canon
                assert lds[t] + j == row * c["pitch"] + want, (c, t, j)
