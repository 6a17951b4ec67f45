// Output-channel tiling shared by the MFMA kernels (gfx950 only; device code).
//
// The Cq output channels of a group are covered by MTB = Cq/16 full 16-row tiles (v_mfma_f32_16x16x4_f32, 8 passes)
// plus NSM = (Cq%16)/4 four-row blocks (v_mfma_f32_4x4x1_16B_f32, 2 passes): 16 independent 4x4 outer products, used
// as 4 k-slots x 4 pixel quads of ONE 4-channel block.  Both take the SAME B operand (lane (q,p) = channel 4j+q of
// pixel p), so the rest of a group (Cq = 24: 8 channels) costs 2 x 2 passes per k-step instead of 8 for a second,
// half-empty 16-row tile; neither M nor K carries padding.  Layouts pinned on hardware by scripts/micro/mfma4x4.hip.
#pragma once
#include <stddef.h>

#include "finc_device.h"

// Channel held by k-slot q of k-step (= register) j of an operand made from solved pixels: registers of the 16-row tiles first (D
// layout: reg r of tile mt, lane row q = channel 16mt + 4q + r), then one register per 4-row block (channel 16*MTB + 4sb + q after
// the reduce-transpose of finc_block_reduce).  The packer, the compute waves and the store side of every inverse that runs on the
// wavefront kernel's packed bank (finc_mfma.hip, finc_split.hip, finc_chain.hip) read this one definition.
__host__ __device__ constexpr int chan_d(int MTB, int j, int q)
{
    if (j < 4 * MTB) return 16 * (j >> 2) + 4 * q + (j & 3);
    return 16 * MTB + 4 * (j - 4 * MTB) + q;
}

// one accumulator update: tile index mt < MTB is a 16-row tile, otherwise a 4-row block; `a` = the matching fragment
// (16-row tile: lane (q,i) = W[16mt+i][k-slot q]; 4-row block: lane (q,i) = W[16*MTB + 4sb + (i&3)][k-slot q])
template <int MTB>
__device__ inline void finc_mma(v4f &acc, int mt, float a, float b)
{
    if (mt < MTB) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    else acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, acc, 0, 0, 0);
}

// Four 4-row-block fragments share ONE register.  A block fragment repeats its 16 values (4 rows x 4 k-slots) for each of
// the 4 pixel quads; the multi-block MFMAs can broadcast the A operand instead: with CBSZ = 2 the 16 blocks form groups
// of 4 (= the 4 pixel quads of one k-slot) and every block of a group takes A from the group's block ABID.  So lane
// (q, 4a + i) of a packed register holds fragment a's value for (row i, k-slot q), and ABID = a selects it: the 4-row
// blocks of a filter bank cost a quarter of the registers (c3: 108 -> 27), same instruction, same rate.
__device__ inline void finc_mma_small(v4f &acc, float a4, float b, int abid)
{
    switch (abid & 3) {   // (the builtin wants literals; the switch folds once the loops are unrolled)
    case 0: acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4, b, acc, 2, 0, 0); break;
    case 1: acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4, b, acc, 2, 1, 0); break;
    case 2: acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4, b, acc, 2, 2, 0); break;
    default: acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a4, b, acc, 2, 3, 0); break;
    }
}

// A 4-row block's register i holds, in lane row q', the k-slot-q' PARTIAL sum of channel base+i.  Sum over the 4 lane
// rows and leave channel base+q in lane row q: a 4x4 transpose-reduce (rows two apart by v_permlane32_swap + add,
// rows one apart by v_permlane16_swap + add; 6 VALU).
__device__ inline float finc_block_reduce(const v4f &acc)
{
    // NB: __builtin_bit_cast applied directly to an ext-vector ELEMENT silently reads element 0 with this compiler;
    // always go through scalar temporaries.
    const float r0 = acc.x, r1 = acc.y, r2 = acc.z, r3 = acc.w;
    // v_permlane32_swap(v, s): new v = [v.lanes 0-31, s.lanes 0-31], new s = [v.lanes 32-63, s.lanes 32-63]
    const v2u a = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r0), __builtin_bit_cast(unsigned, r2),
                                                        false, false);
    const v2u b = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, r1), __builtin_bit_cast(unsigned, r3),
                                                        false, false);
    const unsigned a0 = a.x, a1 = a.y, b0 = b.x, b1 = b.y;
    const float s02 = __builtin_bit_cast(float, a0) + __builtin_bit_cast(float, a1); // rows 0,1: r0 ; rows 2,3: r2
    const float s13 = __builtin_bit_cast(float, b0) + __builtin_bit_cast(float, b1); // rows 0,1: r1 ; rows 2,3: r3
    // v_permlane16_swap(v, s): new v = [v.row0, s.row0, v.row2, s.row2], new s = [v.row1, s.row1, v.row3, s.row3]
    const v2u c = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, s02), __builtin_bit_cast(unsigned, s13),
                                                        false, false);
    const unsigned c0 = c.x, c1 = c.y;
    return __builtin_bit_cast(float, c0) + __builtin_bit_cast(float, c1);
}

// Linv (the z-term) is lower triangular: its fragment (k-step j, tile mt) is all zero when every column 4j..4j+3 lies
// right of every row of the tile, and the MFMA can be skipped
__host__ __device__ constexpr bool finc_zterm_is_zero(int MTB, int j, int mt)
{
    return mt < MTB ? 4 * j > 16 * mt + 15 : 4 * j > 16 * MTB + 4 * (mt - MTB) + 3;
}

// row of the weight matrix held by lane i (0..15) of fragment tile mt
__host__ __device__ inline int finc_tile_row(int MTB, int mt, int i)
{
    return mt < MTB ? 16 * mt + i : 16 * MTB + 4 * (mt - MTB) + (i & 3);
}

// Paired remainder tile (the inverse's one-wave 3x3 kernels, finc_mfma.hip).  A bank with 8 channels beside its 16-row tiles
// stacks the 4-row blocks of two taps that read the SAME operand into one 16-row fragment: row i = 4*qq + r of the fragment is
//   r = 0, 1: channel 16*MTB + 4r + qq of the pair's first tap ((0,1) resp. (1,0)) -- the pixel being solved;
//   r = 2, 3: channel 16*MTB + 4(r-2) + qq of its partner ((0,2) resp. (1,1)) -- the lane's next pixel.
// So D register r < 2 of lane row qq is channel 16*MTB + 4r + qq: what chan_d gives k-slot qq of operand register 4*MTB + r.
__host__ __device__ constexpr bool finc_pair_bank(int cqp, int KH, int KW) { return KH == 3 && KW == 3 && cqp > 16 && cqp % 16 == 8; }
__host__ __device__ inline int finc_pair_row(int MTB, int i, int *partner)
{
    const int qq = i >> 2, r = i & 3;
    *partner = r >> 1;
    return 16 * MTB + 4 * (r & 1) + qq;
}
// Element `lane` of paired fragment f (0 .. 2*NKD-1) of a group, as the packer writes it and the kernel reads it: pair f / NKD
// (0: taps (0,1)|(0,2), 1: (1,0)|(1,1)), k-step j = f % NKD and k-slot q = lane / 16 of the column (its channel is chan_d(MTB, j, q)),
// row channel and tap (a, b) by finc_pair_row.  The one statement of the map: pack_kernel calls it, and so does the host test.
__host__ __device__ inline void finc_pair_elem(int MTB, int NKD, int f, int lane, int *row, int *j, int *q, int *a, int *b)
{
    int partner;
    const int pr = f / NKD;
    *row = finc_pair_row(MTB, lane & 15, &partner);
    *j = f % NKD;
    *q = lane >> 4;
    *a = pr;                                  // pair 2 (stage 2): taps (2,0)|(2,1)
    *b = (pr == 0 ? 1 : 0) + partner;
}
// float offset of that fragment in the packed buffer: the paired fragments of all groups lie behind the G banks of npack fragments
__host__ __device__ inline size_t finc_pair_offset(int G, int npack, int npair, int g, int f)
{
    return ((size_t)G * npack + (size_t)g * npair + f) * 64;
}

// Row shifts read from LDS (finc_wave_kernel, the helper-wave paired forms: finc_pair2_form; P = 16 there).  S_a(t) of lane (q, p):
// lanes p >= a take the pixel lane p - a wrote to the x ring in this very step, lanes p < a the pixel lane P - a + p of the band
// above solved D - 1 steps ago -- ONE LDS read per operand register with a per-lane address instead of a DPP move merged with a
// FIFO pop.  A k-step's offset is an immediate of the instruction, the same for all 64 lanes, so ring lanes and FIFO lanes must
// share the k-step stride: the FIFO block of a k-step lies right behind its x-ring block (finc_big.hip lays its rings out the
// same way), and the stride is a multiple of 64 floats so that two k-steps still go into one ds_*2st64 instruction:
//   k-step block = [x ring: 8 time slots x 64 lanes][FIFO: FINC_LS_DMAX - 1 slots x JS floats],  JS = 4 k-slots x (KH - 1) rows.
// The FIFO is a ring of D - 1 slots: a step READS its slot (pushed D - 1 steps ago) and then pushes into the same slot, in program
// order -- LDS executes a wave's operations in order.  D = 1 (W = 16) has no FIFO: the pixel lane P - a + p solved in this very step
// is the x-ring cell 16 lanes above the one the shift formula names.  Lanes that push nothing write their own x-ring cell again
// (the value the x-ring write of the same step put there), so no trash words are needed.  The stride is a constant of the build:
// the block holds the deepest FIFO the form runs (W = 64: D = 49), which makes a wave's LDS 39.9 KB at 24 channels whatever the
// width -- less than the 40.6 KB of the plain layout at W = 64, more on narrower maps, where it costs nothing (the z and x rings
// alone let only one 4-problem workgroup onto a compute unit).  All values are float indices relative to the x ring of k-step 0.
constexpr int FINC_LS_DMAX = 49, FINC_LS_XBLOCK = 8 * 64;
__host__ __device__ constexpr int finc_ls_js(int KH) { return 4 * (KH - 1); }
__host__ __device__ constexpr int finc_ls_jstride(int KH) { return FINC_LS_XBLOCK + finc_ls_js(KH) * (FINC_LS_DMAX - 1); }
// x-ring cell of `lane` in time slot t & 7
__host__ __device__ constexpr int finc_ls_xcell(int slot, int lane) { return slot * 64 + lane; }
// FIFO word of slot `fslot` (0 .. D-2), k-slot q, row l (0 .. KH-2) of the band's last KH - 1 rows
__host__ __device__ constexpr int finc_ls_fifo(int KH, int fslot, int q, int l) { return FINC_LS_XBLOCK + fslot * finc_ls_js(KH) + q * (KH - 1) + l; }
// does `lane` push into the FIFO (rows P-(KH-1) .. P-1 of a band) / read S_a from it (rows 0 .. a-1)?
__host__ __device__ constexpr bool finc_ls_pushes(int KH, int P, int D, int lane) { return D > 1 && (lane & 15) >= P - (KH - 1) && (lane & 15) < P; }
__host__ __device__ constexpr bool finc_ls_pops(int a, int D, int lane) { return D > 1 && (lane & 15) < a; }
// where `lane` writes its pixel behind the x-ring write of time slot `slot`, FIFO slot `fslot`
__host__ __device__ constexpr int finc_ls_push(int KH, int P, int D, int lane, int slot, int fslot)
{
    return finc_ls_pushes(KH, P, D, lane) ? finc_ls_fifo(KH, fslot, lane >> 4, (lane & 15) - (P - (KH - 1))) : finc_ls_xcell(slot, lane);
}
// where `lane` reads S_a in the step of time slot `slot`, FIFO slot `fslot`
__host__ __device__ constexpr int finc_ls_src(int KH, int a, int D, int lane, int slot, int fslot)
{
    if (finc_ls_pops(a, D, lane)) return finc_ls_fifo(KH, fslot, lane >> 4, KH - 1 - a + (lane & 15));
    return finc_ls_xcell(slot, (lane & 15) >= a ? lane - a : lane - a + 16);
}
// The kernel keeps ONE pointer per a (and one for the push) and moves it by per-lane constants: `step` after every step, back by
// `rewind8` behind the step of time slot 7 and back by `rewindR` when the FIFO slot wraps (fifo: the lane is on the FIFO side).
__host__ __device__ constexpr int finc_ls_step(int KH, bool fifo) { return fifo ? finc_ls_js(KH) : 64; }
__host__ __device__ constexpr int finc_ls_rewind8(bool fifo) { return fifo ? 0 : FINC_LS_XBLOCK; }
__host__ __device__ constexpr int finc_ls_rewindR(int KH, int D, bool fifo) { return fifo ? (D - 1) * finc_ls_js(KH) : 0; }

// Strip-piece map of the grad-weight kernels (finc_gradw.hip: staged, tiled, Winograd, Winograd tile-pair).  A wave stages a strip
// of 4*np columns of `rows` channel rows (channels c0 .. c0 + rows - 1 of a slab [CQ][H][W]) in an LDS tile [channel][pitch floats],
// one 16-byte piece per load slot t = 64 * i + lane:
//   slots t < np * rows            row piece k = t % np of channel row c = t / np: memory columns ms + 4k .. ms + 4k + 3;
//   then, with `halo`, `rows` more  the halo piece of channel row t - np * rows: memory columns hm .. hm + 3, the four columns to the
//                                  left of the strip in canonical order -- hm = ms - 4, or mirrored hm = ms + 4 * np;
//   every slot behind those        nothing to load: lanes behind the bank park their piece in the scratch piece `scratch`.
// The slot's byte offset in the slab (row offset not included: the kernels add (h * W) * 4 as the load's scalar offset) is that of
// (channel c0 + c, column) -- or OFF_BAD_CHANNEL (finc_device.h) when the channel lies behind the bank (>= CQ: the bank is padded, or
// the 16-channel window of a tile pair reaches past it) or the column outside the row.  W % 4 == 0 and ms % 4 == 0: a piece is inside
// the row or outside, never astride -- outside are the pieces of the last strip of a row whose width is no multiple of the strip's
// (a strip wider than the whole row included) and the halo piece of the first strip.
// The landing address (floats) keeps memory order: row piece k at lead + 4k with the halo piece in front of it at 0 (lead = 4 for an
// x tile, 0 for a gz tile, which has no halo) -- canonical column c of the strip at tile column lead + c -- or, mirrored, row piece k
// at 4k and the halo piece BEHIND the row pieces at 4 * np: canonical column c at tile column 4 * np - 1 - c, and the columns left of
// the strip at 4 * np upwards.  The kernels' read maps (xrd, grd) are written against exactly this.
// Known sibling: the staged forward of finc_conv.hip has the same loop without the column test (its launch rule differs).
// A macro that the kernels expand in place, and a function of it for the host test: a call in the kernels' set-up, a forced inline
// included, moved registers and instructions of the whole kernel (profiles/device_prelude/isa_identity.txt), the expansion moves none.
#define FINC_STRIP_PIECE(voff, lds, t, np, rows, c0, CQ, HW, W, ms, hm, mirrored, pitch, lead, scratch, halo)                    \
    {                                                                                                                            \
        (voff) = OFF_BAD_CHANNEL;                                                                                                \
        (lds) = (scratch);                                                                                                       \
        if ((t) < (np) * (rows)) {                                                                                               \
            const int c_ = (t) / (np), k_ = (t) % (np);                                                                          \
            if ((c0) + c_ < (CQ) && (ms) + 4 * k_ >= 0 && (ms) + 4 * k_ < (W))                                                   \
                (voff) = (unsigned)((c0) + c_) * (HW) * 4u + (unsigned)((ms) + 4 * k_) * 4u;                                     \
            (lds) = c_ * (pitch) + ((mirrored) ? 0 : (lead)) + 4 * k_;                                                           \
        } else if ((halo) && (t) < ((np) + 1) * (rows)) {                                                                        \
            const int c_ = (t) - (np) * (rows);                                                                                  \
            if ((c0) + c_ < (CQ) && (hm) >= 0 && (hm) < (W)) (voff) = (unsigned)((c0) + c_) * (HW) * 4u + (unsigned)(hm) * 4u;   \
            (lds) = c_ * (pitch) + ((mirrored) ? 4 * (np) : 0);                                                                  \
        }                                                                                                                        \
    }
struct FincStripPiece {
    unsigned voff;   // byte offset in the slab, or OFF_BAD_CHANNEL
    int lds;         // landing address in the tile, floats
};
__host__ __device__ constexpr FincStripPiece finc_strip_piece(int t, int np, int rows, int c0, int CQ, int HW, int W, int ms, int hm,
                                                              bool mirrored, int pitch, int lead, int scratch, bool halo)
{
    FincStripPiece p{};
    FINC_STRIP_PIECE(p.voff, p.lds, t, np, rows, c0, CQ, HW, W, ms, hm, mirrored, pitch, lead, scratch, halo)
    return p;
}
