// Double precision on the matrix cores (gfx950 / CDNA4 only): the reference op dispatches over float AND double
// (AT_DISPATCH_FLOATING_TYPES, cinc_cuda_kernel_level2.cu:117) and its CPU solver computes in fp64
// (solve_parallel_mc.pyx:77-126).  finc_inverse_f64 / finc_forward_f64 (finc_generic.hip) keep the reference's term order and
// are bit-exact with that solver; these kernels are the fast form behind FINC_ALGO_AUTO: the same visitation (anti-diagonal
// order band by band, cinc_cuda_kernel_level2.cu:49-56,98-111), the in-pixel substitution folded into the bank (Linv = L^-1, as
// in finc_mfma.hip), every product on v_mfma_f64_16x16x4_f64.
//
// One wavefront owns one (image, group) problem; no barrier, no inter-wave traffic.  Lanes are 4 k-slots q x 16 rows p of a band;
// lane p trails lane p-1 by one step.  The f64 MFMA's result layout (lane (q, n), register r = row q + 4r of column n) is, for
// natural channel order, exactly the B operand of k-step r -- so a solved pixel goes to a ring of cells in LDS as it leaves the
// accumulators and comes back as operands (lane p - a of the slot of step t - a - b) without any shuffling; the rows above a band
// wait in a FIFO in LDS; a wave's LDS operations execute in order, so nothing needs a fence.  The bank -- 9 * NK * MT fragments of
// one double per lane: 216 registers at Cq = 24 -- stays in registers for the whole kernel (one wave per SIMD: 512 registers).
// A step is 9 * NK * MT MFMAs of 64 cycles (Cq = 24: 108 + 12 = 7,680 cycles), so everything else -- 48 LDS reads, the dword-pair
// loads and stores of a lane's own pixel -- runs in their shadow.
//
// That is SPLIT = false: Cq <= 24 at 3x3, <= 32 at 2x2.  Every kernel below is one template with that one parameter: a wave owns the
// 16-row output tiles [m0, m0 + MTW) of the bank -- all MT of them, or (SPLIT = true, "M-split", DESIGN 3.11.2: the banks of 29 .. 64
// channels at 3x3 and 33 .. 64 at 2x2, padded to CQP = 32 / 48 / 64) one, tile m0 = its index among the MT waves of a problem.
// 9 * NK * MT fragments no longer fit one wave there (CQP = 64: 576 doubles), so wave m0 holds the slice [tap][j][m0] (9 * NK
// doubles, 144 at CQP = 64), accumulates tile m0 alone and owns the k-steps 4 m0 .. 4 m0 + 3 of every solved pixel -- its ring and
// FIFO words and its channels in memory.  Linv is folded into the bank, so the tiles of a pixel do not depend on each other within a
// step; what a wave reads of the others is at least one step old, and ONE __syncthreads per step orders it.  Two more things differ
// under SPLIT because the waves of a step are no longer in program order: the FIFO is one slot deeper (the oldest read of a step, age
// KH + KW - 2 of the rows above a band, would share its slot with the push of the same step), and a problem slot of the workgroup
// beyond the last problem runs every step on a zero-length buffer resource (loads give 0, stores are dropped) so that the barrier
// count stays uniform.
#include "finc_common.h"
#include "finc_device.h"

#include <type_traits>
#include <utility>

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));


constexpr int XS = 6;             // x ring slots: taps reach back KH + KW - 2 <= 4 steps
constexpr int WPW = 4;            // inverse, one wave per problem: problems (= waves) per workgroup

template <int CQP, int KH, int KW, bool SPLIT>
struct DCfg {
    static_assert(CQP % 4 == 0 && KH + KW - 2 <= XS - 2, "bank");
    static_assert(!SPLIT || (CQP % 16 == 0 && CQP >= 32 && CQP <= 64), "bank");
    static constexpr int MT = (CQP + 15) / 16, NK = CQP / 4, NTAP = KH * KW;
    static constexpr int MTW = SPLIT ? 1 : MT;                    // row tiles of a wave
    static constexpr int WPP = SPLIT ? MT : 1;                    // waves of a problem
    static constexpr int NKW = SPLIT ? 4 : NK;                    // k-steps of a pixel the wave stores: 4 m0 + r
    static constexpr int PPW = SPLIT ? (CQP == 32 ? 2 : 1) : WPW; // inverse: problems per workgroup at most (as many as the LDS holds)
    static constexpr int NFRAG = NTAP * NK * MT;                 // z-term first, then the taps (a, b) != (0, 0) row-major
    static constexpr int CELL = NK * 8;                           // bytes of a pixel: NK doubles per lane
    static constexpr int HROWS = KH - 1;                          // rows handed over between bands
    // LDS of a problem: ring [slot][lane] | one zero cell | FIFO [slot][q][row]
    static constexpr int RING_B = 0, ZERO_B = XS * 64 * CELL, FIFO_B = ZERO_B + CELL;
    static constexpr int FSLOT = 4 * (HROWS > 0 ? HROWS : 1) * CELL;
    static constexpr int lds_bytes(int DF) { return FIFO_B + DF * FSLOT; }
};

// -----------------------------------------------------------------------------------------------
// Fragment packing in fp64 (one workgroup per group): fragment (tap, j, mt), lane (q, i) = M_tap[16 mt + i][4 j + q], M_z = Linv,
// M_(a,b) = -(Linv * Wc[:, :, KH-1-a, KW-1-b]); forward (1): M_(a,b) = Wc[:, :, KH-1-a, KW-1-b] for all nine taps, (0,0) in the z slot;
// forward transposed (2): M_(a,b)[row][col] = Wc[col][row][KH-1-a][KW-1-b], the grad-input's bank.  (`forward`: a FincF64Mode.)
// -----------------------------------------------------------------------------------------------
__global__ void pack_f64_kernel(const double *__restrict__ wc, double *__restrict__ packed, int Cq, int KH, int KW, int MT, int NK, int forward)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];   // Linv [Cq][Cq]
    const int g = blockIdx.x;
    const double *wg = wc + (size_t)g * Cq * Cq * KH * KW;
    const int KK = KH * KW, nfrag = KK * NK * MT;
    double *Linv = sm;
    if (!forward) {
        for (int j = threadIdx.x; j < Cq; j += blockDim.x)
            for (int r = 0; r < Cq; ++r) {
                double s = (r == j) ? 1.0 : 0.0;
                for (int k = j; k < r; ++k) s -= wg[((size_t)r * Cq + k) * KK + (KK - 1)] * Linv[k * Cq + j];
                Linv[r * Cq + j] = (r < j) ? 0.0 : s;
            }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < nfrag * 64; e += blockDim.x) {
        const int lane = e & 63, f = e >> 6;
        const int q = lane >> 4, i = lane & 15;
        const int mt = f % MT, j = (f / MT) % NK, tap = f / (MT * NK);       // tap 0 = the z-term / the (0,0) tap
        const int row = 16 * mt + i, col = 4 * j + q;
        const int a = tap / KW, b = tap % KW;
        const int widx = (KH - 1 - a) * KW + (KW - 1 - b);
        double v = 0.0;
        if (row < Cq && col < Cq) {
            if (forward == 2) v = wg[((size_t)col * Cq + row) * KK + widx];
            else if (forward) v = wg[((size_t)row * Cq + col) * KK + widx];
            else if (tap == 0) v = Linv[row * Cq + col];
            else {
                double s = 0.0;
                for (int k = 0; k <= row; ++k) s += Linv[row * Cq + k] * wg[((size_t)k * Cq + col) * KK + widx];
                v = -s;
            }
        }
        packed[((size_t)g * nfrag + f) * 64 + lane] = v;
    }
}

// -----------------------------------------------------------------------------------------------
// what the three kernels share
// -----------------------------------------------------------------------------------------------
// slab `bg` of a [B * G][CQ][H][W] tensor as a buffer resource (CQ = 0: zero bytes long -- loads give 0, stores are dropped)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slab_rsrc(const double *t, int bg, int CQ, int HW)
{
    const unsigned slab_bytes = (unsigned)CQ * (unsigned)HW * 8u;
    return FINC_SLAB_RSRC(t, (size_t)bg * CQ * HW, slab_bytes);
}
// byte offset of canonical pixel (r, cc) within a channel; fh, fw: the FINC_FLIP_* bits of the group's orientation
__device__ __forceinline__ unsigned pix_byte_off(bool fh, bool fw, int H, int W, int r, int cc)
{
    return (unsigned)(((fh ? H - 1 - r : r) * W + (fw ? W - 1 - cc : cc)) * 8);
}
// byte offset of channel ch in the slab, or the out-of-range mark
__device__ __forceinline__ unsigned chan_mark(int ch, int CQ, int HW) { return ch < CQ ? (unsigned)(ch * HW * 8) : OFF_BAD_CHANNEL; }
__device__ __forceinline__ double load_f64(const __amdgpu_buffer_rsrc_t &rs, unsigned off)
{
    return __builtin_bit_cast(double, __builtin_bit_cast(v2u, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0)));
}
__device__ __forceinline__ void store_f64(double v, const __amdgpu_buffer_rsrc_t &rs, unsigned off)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), rs, off, 0, 0);
}
__device__ __forceinline__ double pick(v4d v, int r) { return r == 0 ? v.x : r == 1 ? v.y : r == 2 ? v.z : v.w; }
// the wave's slice [tap][j][m0 .. m0 + MTW) of group g's bank, to registers for the whole kernel: put(tap, j, i, value).  (Through `put`
// the array stays the kernel's own; as a reference parameter it changes the schedule of the larger banks.)
template <class C, class F>
__device__ __forceinline__ void load_bank(F &&put, const double *packed, int g, int m0, int lane)
{
    const double *pk = packed + (size_t)g * C::NFRAG * 64 + (size_t)m0 * 64 + lane;
#pragma unroll
    for (int tp = 0; tp < C::NTAP; ++tp)
#pragma unroll
        for (int j = 0; j < C::NK; ++j)
#pragma unroll
            for (int i = 0; i < C::MTW; ++i) put(tp, j, i, pk[(size_t)((tp * C::NK + j) * C::MT + i) * 64]);
}

// -----------------------------------------------------------------------------------------------
// inverse: grid = ceil(B*G / ppw) workgroups of ppw problems, WPP waves each
// -----------------------------------------------------------------------------------------------
template <int CQP, int KH, int KW, bool SPLIT>
__global__ __launch_bounds__((64 * DCfg<CQP, KH, KW, SPLIT>::WPP * DCfg<CQP, KH, KW, SPLIT>::PPW), 1) void finc_f64_inverse_kernel(
    const double *__restrict__ in, const double *__restrict__ packed, double *__restrict__ out, int G, int CQ, int H, int W, int P, int T,
    unsigned orient, int DF, int nprob, int ppw)
{
    using C = DCfg<CQP, KH, KW, SPLIT>;
    constexpr int MTW = C::MTW, WPP = C::WPP, NK = C::NK, NKW = C::NKW, CELL = C::CELL, HROWS = C::HROWS;
    extern __shared__ __attribute__((aligned(16))) double lds_all[];
    // ppw (<= PPW, as many as the LDS holds) independent problems per workgroup: the waves of ONE workgroup go to the four SIMDs in turn, one-wave
    // workgroups do not (two of them on one SIMD halve each other: 2.9 against 2.1 ms at c3)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = wave % WPP, prob = wave / WPP;                 // the wave's first row tile, its problem within the workgroup
    int bg = (int)blockIdx.x * ppw + prob;
    bool live = true;                                             // (the grid has no workgroup without a first problem)
    if constexpr (SPLIT) {                                        // a SPLIT wave never leaves early: the barrier count stays uniform, and
        live = bg < nprob;                                        // a slot beyond the last problem runs on zero-length resources
        bg = live ? bg : 0;
    } else if (bg >= nprob) return;
    double *const ldsd = lds_all + (size_t)prob * (C::lds_bytes(DF) / 8);
    char *const ldsb = reinterpret_cast<char *>(ldsd);
    const int lane = threadIdx.x & 63, q = lane >> 4, p = lane & 15;
    const int g = bg % G;
    const unsigned o = finc_group_orient(orient, g);
    const bool fh = (o & FINC_FLIP_H) != 0, fw = (o & FINC_FLIP_W) != 0;
    auto pix_off = [&](int r, int cc) { return pix_byte_off(fh, fw, H, W, r, cc); };
    const int HW = H * W;
    const __amdgpu_buffer_rsrc_t rin = slab_rsrc(in, bg, live ? CQ : 0, HW), rout = slab_rsrc(out, bg, live ? CQ : 0, HW);

    for (int i = m0 * 64 + lane; i < C::lds_bytes(DF) / 8; i += 64 * WPP) ldsd[i] = 0.0;      // (!SPLIT: the wave's own part, no barrier anywhere)

    double fr[C::NTAP][NK][MTW];
    load_bank<C>([&](int tp, int j, int i, double v) { fr[tp][j][i] = v; }, packed, g, m0, lane);

    auto ld = [&](int byte_off) { return *reinterpret_cast<const double *>(ldsb + byte_off); };
    auto st = [&](int byte_off, double v) { *reinterpret_cast<double *>(ldsb + byte_off) = v; };

    // per-lane constants
    const int jz = 4 * (m0 + MTW);               // Linv is lower triangular: the tiles below m0 + MTW read the k-steps j < jz of z
    unsigned chan_off[NK], own_off[NKW];         // channel 4j + q of the slab; the channels the wave stores: k-steps 4 m0 + r
#pragma unroll
    for (int j = 0; j < NK; ++j) chan_off[j] = chan_mark(4 * j + q, CQ, HW);
#pragma unroll
    for (int r = 0; r < NKW; ++r) own_off[r] = SPLIT ? chan_mark(16 * m0 + 4 * r + q, CQ, HW) : chan_off[r];
    const int wpart = m0 * 32;                   // the wave's doubles within a cell
    int taddr[KH];                               // operand cell of tap row a: lane p - a of the ring slot / the FIFO for the lanes p < a
#pragma unroll
    for (int a = 0; a < KH; ++a) taddr[a] = C::RING_B + (lane - a) * CELL;
    const bool pusher = HROWS > 0 && p >= P - HROWS && p < P;
    const int push_cell = C::FIFO_B + (q * HROWS + (P - 1 - p)) * CELL + wpart;      // row a' = P - p above the next band

    // the lane's walk: position n = t - p, column c = n mod W, band n / W
    int c = -p, row = p;                         // column (negative: not started), image row
    // z of the next step is requested one step ahead
    double zn[NK];
    auto request = [&](int cc, int rr) {
        const bool ok = cc >= 0 && rr < H && p < P;
        const unsigned base = ok ? pix_off(rr, cc) : OFF_INVALID;
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            if constexpr (SPLIT) zn[j] = load_f64(rin, (j < jz ? base : OFF_INVALID) + chan_off[j]);
            else zn[j] = load_f64(rin, base + chan_off[j]);
        }
    };
    request(c, row);
    const bool W4 = (W & 3) == 0;                // rows of whole 32-byte groups
    int slot = 0;                                // t mod XS
    int fpush = 0;                               // t mod DF
    if constexpr (SPLIT) __syncthreads();        // the zero fill
    for (int t = 0; t < T; ++t) {
        double z[NK];
#pragma unroll
        for (int j = 0; j < NK; ++j) z[j] = zn[j];
        const int cn = (c + 1 == W) ? 0 : c + 1, rn = (c + 1 == W) ? row + P : row;
        request(cn, rn);
        // ---- z-term, then the taps by falling age (a + b): the two that need the pixel of the step before come last
        v4d acc[MTW];
#pragma unroll
        for (int i = 0; i < MTW; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < NK; ++j)
#pragma unroll
            for (int i = 0; i < MTW; ++i) {
                if (16 * (m0 + i) + 15 < 4 * j) continue;                    // Linv is lower triangular (SPLIT: uniform in the wave)
                acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[0][j][i], z[j], acc[i], 0, 0, 0);
            }
#pragma unroll
        for (int age = KH + KW - 2; age >= 1; --age)
#pragma unroll
            for (int a = 0; a < KH; ++a) {
                const int b = age - a;
                if (b < 0 || b >= KW) continue;
                // S_a(t - age): ring slot (t - age) mod XS at lane p - a; the lanes p < a read the band above from the FIFO (the push
                // of step t - age - (W - P)); a missing column (c - b < 0) reads the zero cell
                int sl = slot - age; if (sl < 0) sl += XS;
                int fs = fpush - age - (W - P); fs %= DF; if (fs < 0) fs += DF;
                int addr = taddr[a] + sl * (64 * CELL);
                if (a > 0) addr = p >= a ? addr : C::FIFO_B + fs * C::FSLOT + (q * HROWS + (a - 1 - p)) * CELL;
                if (b > 0) addr = c >= b ? addr : C::ZERO_B;
                double x[NK];
#pragma unroll
                for (int j = 0; j < NK; ++j) x[j] = ld(addr + j * 8);
#pragma unroll
                for (int j = 0; j < NK; ++j)
#pragma unroll
                    for (int i = 0; i < MTW; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[a * KW + b][j][i], x[j], acc[i], 0, 0, 0);
            }
        // ---- the solved pixel's k-steps 4 m0 + r: register r & 3 of tile m0 + r / 4, lane row q = channel 16 m0 + 4 r + q
        const bool started = c >= 0 && p < P;
        double xs[NKW];
#pragma unroll
        for (int r = 0; r < NKW; ++r) xs[r] = started ? pick(acc[r >> 2], r & 3) : 0.0;
        const int cell = C::RING_B + slot * (64 * CELL) + lane * CELL + wpart;
#pragma unroll
        for (int r = 0; r < NKW; ++r) st(cell + r * 8, xs[r]);
        if (pusher) {
#pragma unroll
            for (int r = 0; r < NKW; ++r) st(push_cell + fpush * C::FSLOT + r * 8, xs[r]);
        }
        if (W4) {
            // 32-byte pieces: a lane stores a group of four canonical columns when it has solved the last one -- the three before sit
            // in the ring's last slots at its own lane (the wave's own words of them).  (8-byte stores, 100 M of them at c3, bound the
            // kernel at 2.9 ms: every wave keeps 384 partially written lines open, more than the L2s hold.)
            const bool ok = started && row < H && (c & 3) == 3;
            const unsigned base = ok ? pix_off(row, fw ? c : c - 3) : OFF_INVALID;
            int s1 = slot - 1, s2 = slot - 2, s3 = slot - 3;
            s1 = s1 < 0 ? s1 + XS : s1; s2 = s2 < 0 ? s2 + XS : s2; s3 = s3 < 0 ? s3 + XS : s3;
            const int own = C::RING_B + lane * CELL + wpart;
#pragma unroll
            for (int r = 0; r < NKW; ++r) {
                const double x3 = ld(own + s3 * (64 * CELL) + r * 8), x2 = ld(own + s2 * (64 * CELL) + r * 8), x1 = ld(own + s1 * (64 * CELL) + r * 8);
                const double lo0 = fw ? xs[r] : x3, lo1 = fw ? x1 : x2, hi0 = fw ? x2 : x1, hi1 = fw ? x3 : xs[r];
                const v2u a0 = __builtin_bit_cast(v2u, lo0), a1 = __builtin_bit_cast(v2u, lo1), b0 = __builtin_bit_cast(v2u, hi0), b1 = __builtin_bit_cast(v2u, hi1);
                // (s_nop 1: a store of more than 8 bytes reads its data registers a few cycles after issue; scripts/check_store_hazard.py
                // wants two wait states before anything is written to them -- here the allocator reuses them for the next LDS read)
                __builtin_amdgcn_raw_buffer_store_b128((v4u){a0.x, a0.y, a1.x, a1.y}, rout, base + own_off[r], 0, 0);
                asm volatile("s_nop 1");
                __builtin_amdgcn_raw_buffer_store_b128((v4u){b0.x, b0.y, b1.x, b1.y}, rout, base + own_off[r] + 16, 0, 0);
                asm volatile("s_nop 1");
            }
        } else {
            const bool ok = started && row < H;
            const unsigned base = ok ? pix_off(row, c) : OFF_INVALID;
#pragma unroll
            for (int r = 0; r < NKW; ++r) store_f64(xs[r], rout, base + own_off[r]);
        }
        c = cn; row = rn;
        ++slot; if (slot == XS) slot = 0;
        ++fpush; if (fpush == DF) fpush = 0;
        if constexpr (SPLIT) __syncthreads();    // the step's cells are written: the next step's age-1 taps read every wave's words
    }
}

// -----------------------------------------------------------------------------------------------
// forward / grad-input: a workgroup walks a strip of 16 canonical columns of one slab from the top; grid.x = slab * ns + strip.
// SPLIT: the output row tile is one more launch dimension, the waves of a workgroup (which go to the four SIMDs in turn and read the
// same input rows at the same time; one-wave workgroups do neither); wave m0 reads every input channel and stores its 16.
// -----------------------------------------------------------------------------------------------
template <int CQP, int KH, int KW, bool SPLIT>
__global__ __launch_bounds__((64 * DCfg<CQP, KH, KW, SPLIT>::WPP), 1) void finc_f64_forward_kernel(
    const double *__restrict__ in, const double *__restrict__ packed, double *__restrict__ out, int G, int CQ, int H, int W, unsigned orient, int ns)
{
    using C = DCfg<CQP, KH, KW, SPLIT>;
    constexpr int MTW = C::MTW, NK = C::NK, NKW = C::NKW;
    const int lane = threadIdx.x & 63, q = lane >> 4, p = lane & 15;
    const int m0 = SPLIT ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    const unsigned unit = blockIdx.x;
    const int strip = (int)(unit % (unsigned)ns), bg = (int)(unit / (unsigned)ns), g = bg % G;
    const int w0 = strip * 16;
    const unsigned o = finc_group_orient(orient, g);
    const bool fh = (o & FINC_FLIP_H) != 0, fw = (o & FINC_FLIP_W) != 0;
    auto pix_off = [&](int r, int cc) { return pix_byte_off(fh, fw, H, W, r, cc); };
    const int HW = H * W;
    const __amdgpu_buffer_rsrc_t rin = slab_rsrc(in, bg, CQ, HW), rout = slab_rsrc(out, bg, CQ, HW);
    double fr[C::NTAP][NK][MTW];
    load_bank<C>([&](int tp, int j, int i, double v) { fr[tp][j][i] = v; }, packed, g, m0, lane);
    unsigned chan_off[NK], own_off[NKW];
#pragma unroll
    for (int j = 0; j < NK; ++j) chan_off[j] = chan_mark(4 * j + q, CQ, HW);
#pragma unroll
    for (int r = 0; r < NKW; ++r) own_off[r] = SPLIT ? chan_mark(16 * m0 + 4 * r + q, CQ, HW) : chan_off[r];
    const int col = w0 + p;
    for (int h = 0; h < H; ++h) {
        v4d acc[MTW];
#pragma unroll
        for (int i = 0; i < MTW; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < KH; ++a)
#pragma unroll
            for (int b = 0; b < KW; ++b) {
                // x[i, h - a, col - b]: zero outside the image (the padding of layers/conv.py:41-55)
                const bool ok = h - a >= 0 && col - b >= 0 && col - b < W;
                const unsigned base = ok ? pix_off(h - a, col - b) : OFF_INVALID;
                double x[NK];
#pragma unroll
                for (int j = 0; j < NK; ++j) x[j] = load_f64(rin, base + chan_off[j]);
#pragma unroll
                for (int j = 0; j < NK; ++j)
#pragma unroll
                    for (int i = 0; i < MTW; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[a * KW + b][j][i], x[j], acc[i], 0, 0, 0);
            }
        const unsigned base = col < W ? pix_off(h, col) : OFF_INVALID;
#pragma unroll
        for (int r = 0; r < NKW; ++r) store_f64(pick(acc[r >> 2], r & 3), rout, base + own_off[r]);
    }
}

// -----------------------------------------------------------------------------------------------
// weight gradient: grad_w[o][i][tap (a, b)] = sum over the pixels of gz[o, h, w] * x[i, h - a, w - b] (canonical coordinates), the
// pixels on the MFMA K dimension.  One workgroup per (slab, row chunk), grid.x = slab * nrc + chunk, walks its rows in groups of four
// pixels along W; lane (q, m) loads pixel 4 s + q of channel 16 t + m: for gz that is the A operand of output tile t (row m, k-slot q),
// for x shifted by the tap the B operand of input tile t (k-slot q, column m).  KH * KW * MTW * MT accumulators of four doubles (Cq = 24:
// 36, 288 registers; one wave per SIMD): register r of tile (to, ti) at lane (q, n) is grad_w[16 to + 4 r + q][16 ti + n].  SPLIT: the
// output row tile is one more launch dimension, the waves of a workgroup again (they read the same x); wave m0 accumulates its 16
// output channels against every input tile (36 accumulators at CQP = 64).  Orientation, padded channels, the
// image edge and the K remainder (a group that reaches beyond W) are out-of-range buffer offsets, which load zero -- in BOTH
// operands of such a pixel, so that nothing non-finite next to it is multiplied.  The operands of the next group are requested
// before the MFMAs of this one.  Each wave writes its tiles to partials[b * nrc + chunk][g][tap][to][ti][r][lane] with plain stores;
// the reduce adds them in index order and writes the masked bank: the same bits run after run.
// -----------------------------------------------------------------------------------------------
template <int CQP, int KH, int KW, bool SPLIT>
__global__ __launch_bounds__((64 * DCfg<CQP, KH, KW, SPLIT>::WPP), 1) void finc_f64_gradw_kernel(
    const double *__restrict__ gz, const double *__restrict__ x, double *__restrict__ partials, int G, int CQ, int H, int W, unsigned orient,
    int nrc, int RC)
{
    using C = DCfg<CQP, KH, KW, SPLIT>;
    constexpr int MT = C::MT, MTW = C::MTW, NTAP = C::NTAP;
    const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
    const int m0 = SPLIT ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    const unsigned unit = blockIdx.x;
    const int chunk = (int)(unit % (unsigned)nrc), bg = (int)(unit / (unsigned)nrc), g = bg % G;
    const unsigned o = finc_group_orient(orient, g);
    const bool fh = (o & FINC_FLIP_H) != 0, fw = (o & FINC_FLIP_W) != 0;
    auto pix_off = [&](int r, int cc) { return pix_byte_off(fh, fw, H, W, r, cc); };
    const int HW = H * W;
    const __amdgpu_buffer_rsrc_t rgz = slab_rsrc(gz, bg, CQ, HW), rx = slab_rsrc(x, bg, CQ, HW);
    unsigned chan_off[MT], own_off[MTW];          // channel 16 t + m of x; of gz, the wave's output tiles
#pragma unroll
    for (int t = 0; t < MT; ++t) chan_off[t] = chan_mark(16 * t + m, CQ, HW);
#pragma unroll
    for (int i = 0; i < MTW; ++i) own_off[i] = SPLIT ? chan_mark(16 * m0 + m, CQ, HW) : chan_off[i];
    v4d acc[NTAP][MTW][MT];
#pragma unroll
    for (int tp = 0; tp < NTAP; ++tp)
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int ti = 0; ti < MT; ++ti) acc[tp][i][ti] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int r0 = chunk * RC, r1 = r0 + RC < H ? r0 + RC : H;
    double zn[MTW], xn[NTAP][MT];                 // the operands of the next group
    auto request = [&](int h, int c0) {
        const int col = c0 + q;
        const bool okz = h < r1 && col < W;
        const unsigned zb = okz ? pix_off(h, col) : OFF_INVALID;
#pragma unroll
        for (int i = 0; i < MTW; ++i) zn[i] = load_f64(rgz, zb + own_off[i]);
#pragma unroll
        for (int a = 0; a < KH; ++a)
#pragma unroll
            for (int b = 0; b < KW; ++b) {
                const bool ok = okz && h - a >= 0 && col - b >= 0;
                const unsigned xb = ok ? pix_off(h - a, col - b) : OFF_INVALID;
#pragma unroll
                for (int t = 0; t < MT; ++t) xn[a * KW + b][t] = load_f64(rx, xb + chan_off[t]);
            }
    };
    int h = r0, c0 = 0;
    request(h, c0);
    const int steps = (r1 - r0) * ((W + 3) >> 2);
    for (int s = 0; s < steps; ++s) {
        double zc[MTW], xc[NTAP][MT];
#pragma unroll
        for (int i = 0; i < MTW; ++i) zc[i] = zn[i];
#pragma unroll
        for (int tp = 0; tp < NTAP; ++tp)
#pragma unroll
            for (int t = 0; t < MT; ++t) xc[tp][t] = xn[tp][t];
        c0 += 4;
        if (c0 >= W) { c0 = 0; ++h; }
        request(h, c0);                           // (behind the last group: row r1, every offset out of range)
#pragma unroll
        for (int tp = 0; tp < NTAP; ++tp)
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int ti = 0; ti < MT; ++ti)
                    acc[tp][i][ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(zc[i], xc[tp][ti], acc[tp][i][ti], 0, 0, 0);
    }
    constexpr int PER = NTAP * MT * MT * 256;     // doubles of one slab's tiles
    double *out = partials + (((size_t)(bg / G) * nrc + chunk) * G + g) * PER + lane;
#pragma unroll
    for (int tp = 0; tp < NTAP; ++tp)
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
            for (int ti = 0; ti < MT; ++ti) {
                const v4d &am = acc[tp][i][ti];
                double *t = out + (size_t)((tp * MT + m0 + i) * MT + ti) * 256;
                t[0] = am.x; t[64] = am.y; t[128] = am.z; t[192] = am.w;
            }
}

// One thread per element of the padded tiles [g][tap][to][ti][r][lane]: the `parts` partials of its (g, o, i, tap) in index order, then
// the corner-tap mask (+0.0 where i >= o) and the store to grad_w_canon[g * Cq + o][i][KH-1-a][KW-1-b].
__global__ void gradw_f64_reduce_kernel(const double *__restrict__ partials, double *__restrict__ gw, int G, int Cq, int KH, int KW, int MT,
                                        long long parts)
{
    const int KK = KH * KW, per = KK * MT * MT * 256;
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= G * per) return;
    const int lane = e & 63, r = (e >> 6) & 3, f = e >> 8;
    const int ti = f % MT, to = (f / MT) % MT, tap = (f / (MT * MT)) % KK, g = f / (MT * MT * KK);
    const int oc = 16 * to + 4 * r + (lane >> 4), ic = 16 * ti + (lane & 15);
    if (oc >= Cq || ic >= Cq) return;
    const double *p = partials + e;                // (e = g * per + the element's place in a tile set)
    const size_t stride = (size_t)G * per;
    double s = 0.0;
#pragma unroll 8
    for (long long k = 0; k < parts; ++k) s += p[(size_t)k * stride];
    const int a = tap / KW, b = tap % KW;
    const int widx = (KH - 1 - a) * KW + (KW - 1 - b);
    const bool masked = widx == KK - 1 && ic >= oc;
    gw[((size_t)(g * Cq + oc) * Cq + ic) * KK + widx] = masked ? 0.0 : s;
}

typedef void (*f64inv_fn)(const double *, const double *, double *, int, int, int, int, int, int, unsigned, int, int, int);
typedef void (*f64fwd_fn)(const double *, const double *, double *, int, int, int, int, unsigned, int);
typedef void (*f64gw_fn)(const double *, const double *, double *, int, int, int, int, unsigned, int, int);
struct DInst {
    int cqp, kh, kw, mt, nk, nfrag, lds_fixed, fslot;
    bool split;                      // M-split: mt waves per problem instead of one
    int ppw;                         // inverse: problems per workgroup at most
    f64inv_fn inv;
    f64fwd_fn fwd;
    f64gw_fn gradw;
    int waves() const { return split ? mt : 1; }                  // per problem, per strip, per (slab, row chunk)
    size_t gradw_tile_doubles() const { return (size_t)kh * kw * mt * mt * 256; }
};
template <int CQP, int KH, int KW, bool SPLIT>
constexpr DInst make_dinst()
{
    using C = DCfg<CQP, KH, KW, SPLIT>;
    return DInst{CQP, KH, KW, C::MT, C::NK, C::NFRAG, C::lds_bytes(0), C::FSLOT, SPLIT, C::PPW, finc_f64_inverse_kernel<CQP, KH, KW, SPLIT>,
                 finc_f64_forward_kernel<CQP, KH, KW, SPLIT>, finc_f64_gradw_kernel<CQP, KH, KW, SPLIT>};
}
// The M-split banks take what lies beyond the others: 29 .. 64 channels at 3x3 (25 .. 28 stay on the direct kernels), 33 .. 64 at 2x2;
// a count in between runs on the next larger bank with its channels masked
const DInst g_dinsts[] = {
    make_dinst<4, 3, 3, false>(),  make_dinst<8, 3, 3, false>(),  make_dinst<12, 3, 3, false>(), make_dinst<16, 3, 3, false>(),
    make_dinst<20, 3, 3, false>(), make_dinst<24, 3, 3, false>(), make_dinst<4, 2, 2, false>(),  make_dinst<8, 2, 2, false>(),
    make_dinst<12, 2, 2, false>(), make_dinst<16, 2, 2, false>(), make_dinst<24, 2, 2, false>(), make_dinst<32, 2, 2, false>(),
    make_dinst<32, 3, 3, true>(),  make_dinst<48, 3, 3, true>(),  make_dinst<64, 3, 3, true>(),  make_dinst<48, 2, 2, true>(),
    make_dinst<64, 2, 2, true>(),
};
const DInst *find_dinst(int Cq, int KH, int KW)
{
    const int cqp = (Cq + 3) / 4 * 4, cqm = Cq <= 32 ? 32 : Cq <= 48 ? 48 : 64;
    const bool wide = Cq <= 64 && ((KH == 3 && KW == 3 && Cq >= 29) || (KH == 2 && KW == 2 && Cq >= 33));
    for (const DInst &i : g_dinsts)
        if (i.kh == KH && i.kw == KW && (i.split ? wide && i.cqp == cqm : i.cqp == cqp)) return &i;
    return nullptr;
}
// slots of the FIFO of rows above a band.  The M-split kernel's waves are not in program order within a step, so the oldest read of a
// step must not share its slot with the step's push: one slot more.
int f64_fifo_depth(int W, int P, int KH, int KW, bool split) { return W - P + KH + KW - 2 + (split ? 1 : 0); }
constexpr size_t F64_LDS_MAX = 160 * 1024;

} // namespace

FincF64Plan finc_f64_plan(const FincShape &s)
{
    FincF64Plan p;
    const DInst *i = find_dinst(s.Cq, s.KH, s.KW);
    if (!i || s.B < 1 || s.G < 1 || s.H < 1 || s.W < 1) return p;
    const int P = finc_bands(s).P;
    if (P < s.KH - 1) return p;
    if (!finc_slab_in_range(s.Cq, s.H, s.W, 8)) return p;                   // buffer-offset range marks
    const int DF = f64_fifo_depth(s.W, P, s.KH, s.KW, i->split);
    const size_t per = (size_t)i->lds_fixed + (size_t)DF * i->fslot;        // LDS of one problem
    if (per > F64_LDS_MAX) return p;
    const long long nprob = (long long)s.B * s.G;
    const int ns = (s.W + 15) / 16;
    int ppw = i->ppw;
    while (ppw > 1 && per * ppw > F64_LDS_MAX) ppw >>= 1;
    if (i->split && nprob < ppw) ppw = 1;
    if (nprob * ns > 0x7fffffffLL) return p;                                 // (grid.x of the forward)
    p.family = i->split ? 2 : 1;
    p.cqp = i->cqp;
    p.waves = i->waves();
    p.ppw = ppw;
    p.lds = (int)(per * ppw);
    p.P = P;
    p.DF = DF;
    p.inv_grid = (nprob + ppw - 1) / ppw;
    p.fwd_grid_x = nprob * ns;
    p.fwd_grid_y = 1;
    return p;
}

bool finc_f64_supported(const FincShape &s) { return finc_f64_plan(s).family != 0; }

size_t finc_f64_packed_bytes(int G, int Cq, int KH, int KW)
{
    const DInst *i = find_dinst(Cq, KH, KW);
    return i ? (size_t)G * i->nfrag * 64 * sizeof(double) : 0;
}

// Row chunks of the weight gradient: only a launch that leaves SIMDs idle (fewer waves than the 1,024 one-wave slots of the chip) cuts
// its slabs, into as many chunks of at least four rows as fill them.  A slab is one wave, or under the M-split one per row tile.
// B * nrc <= min(B * max(1, H / 4), max(B, 1024 / (G * waves per slab))): the bound.
constexpr long long GW_SLOTS = 1024;
constexpr int GW_MIN_ROWS = 4;

FincF64GradwPlan finc_f64_gradw_plan(const FincShape &s)
{
    FincF64GradwPlan p;
    const DInst *i = find_dinst(s.Cq, s.KH, s.KW);
    if (!i || !finc_f64_supported(s)) return p;
    const long long units = (long long)s.B * s.G;
    const int maxc = s.H / GW_MIN_ROWS > 0 ? s.H / GW_MIN_ROWS : 1;
    long long want = GW_SLOTS / (units * i->waves());
    want = want > maxc ? maxc : want < 1 ? 1 : want;
    const int RC = (s.H + (int)want - 1) / (int)want, nrc = (s.H + RC - 1) / RC;
    if (units * nrc > 0x7fffffffLL) return p;                               // (grid.x: the direct kernel takes such a batch)
    p.nrc = nrc;
    p.RC = RC;
    p.waves = units * nrc * i->waves();
    p.parts = (long long)s.B * nrc;
    p.bytes = (size_t)p.parts * s.G * i->gradw_tile_doubles() * sizeof(double);
    return p;
}

size_t finc_f64_gradw_workspace_bound(int B, int G, int Cq, int H, int KH, int KW)
{
    const DInst *i = find_dinst(Cq, KH, KW);
    if (!i) return 0;
    const long long maxc = H / GW_MIN_ROWS > 0 ? H / GW_MIN_ROWS : 1;
    const long long per_group = (long long)G * i->waves();
    const long long fill = (GW_SLOTS + per_group - 1) / per_group;
    long long parts = B > fill ? B : fill;
    if ((long long)B * maxc < parts) parts = (long long)B * maxc;
    return (size_t)parts * G * i->gradw_tile_doubles() * sizeof(double);
}

int finc_f64_gradw_launch(const double *gz, const double *x, double *gw, void *workspace, const FincShape &s, hipStream_t st)
{
    const DInst *i = find_dinst(s.Cq, s.KH, s.KW);
    const FincF64GradwPlan p = finc_f64_gradw_plan(s);
    if (!i || !p.nrc) return FINC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(i->gradw, dim3((unsigned)(p.waves / i->waves())), dim3(64 * i->waves()), 0, st, gz, x, (double *)workspace, s.G, s.Cq, s.H,
                       s.W, s.orient, p.nrc, p.RC);
    FINC_CHECK_LAUNCH();
    const size_t total = (size_t)s.G * i->gradw_tile_doubles();
    hipLaunchKernelGGL(gradw_f64_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double *)workspace, gw, s.G, s.Cq,
                       s.KH, s.KW, i->mt, p.parts);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

int finc_f64_launch(const double *in, const double *wc, double *out, void *packed, const FincShape &s, FincF64Mode mode, hipStream_t st)
{
    const DInst *i = find_dinst(s.Cq, s.KH, s.KW);
    const FincF64Plan p = finc_f64_plan(s);
    if (!i || !p.family) return FINC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pack_f64_kernel, dim3(s.G), dim3(256), sizeof(double) * s.Cq * s.Cq, st, wc, (double *)packed, s.Cq, s.KH, s.KW, i->mt,
                       i->nk, (int)mode);
    FINC_CHECK_LAUNCH();
    if (mode != FINC_F64_INVERSE) {
        hipLaunchKernelGGL(i->fwd, dim3((unsigned)p.fwd_grid_x), dim3(64 * p.waves), 0, st, in, (const double *)packed, out, s.G, s.Cq, s.H, s.W,
                           s.orient, (s.W + 15) / 16);
    } else {
        const int NB = (s.H + p.P - 1) / p.P;
        if (int e = finc_ensure_dynamic_lds((const void *)i->inv, (size_t)p.lds)) return e;
        hipLaunchKernelGGL(i->inv, dim3((unsigned)p.inv_grid), dim3(64 * p.waves * p.ppw), (size_t)p.lds, st, in, (const double *)packed, out, s.G,
                           s.Cq, s.H, s.W, p.P, NB * s.W + p.P - 1, s.orient, p.DF, s.B * s.G, p.ppw);
    }
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

unsigned finc_build_flags_f64() { return FINC_BUILD_FLAGS; }
