// Shared host/device helpers for libfinc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/finc.h"
#include "finc_experiment.h"   // the measurement knobs: an error if one is set without -DFINC_EXPERIMENT

#define FINC_FLIP_W 1u
#define FINC_FLIP_H 2u

__host__ __device__ inline unsigned finc_group_orient(unsigned orient, int g) { return (orient >> (2 * g)) & 3u; }

// canonical (h,w) of a group -> offset inside one H*W plane
__device__ inline int finc_pix(int H, int W, unsigned o, int h, int w)
{
    int hh = (o & FINC_FLIP_H) ? H - 1 - h : h;
    int ww = (o & FINC_FLIP_W) ? W - 1 - w : w;
    return hh * W + ww;
}

// Recorded by every failing HIP call; read through finc_last_hip_error().
void finc_set_hip_error(hipError_t e);

#define FINC_HIP_TRY(expr)                     \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess) {                \
            finc_set_hip_error(_e);            \
            return FINC_ERR_LAUNCH;            \
        }                                      \
    } while (0)

#define FINC_CHECK_LAUNCH() FINC_HIP_TRY(hipGetLastError())

// hipFuncAttributeMaxDynamicSharedMemorySize = 160 KiB, once per (device, kernel), thread-safe (finc_abi.hip)
int finc_ensure_dynamic_lds(const void *fn, size_t bytes);

// Protocol faults (helper-wave waits that gave up): finc_fault_gate returns FINC_ERR_LAUNCH if the device's fault word is
// set (sticky; no synchronisation -- the word lives in mapped host memory); `arm` allocates and publishes the word on the
// first call per device.  finc_abi.hip owns the per-device table, finc_mfma.hip the device symbol.
int finc_fault_gate(bool arm, hipStream_t st = nullptr);
int finc_mfma_arm_fault_word(unsigned *device_ptr_to_host_word);

// Run-time A/B switches (FINC_NO_HLP, FINC_WINO_FORM, FINC_SPLIT_MAX ...: scripts/ only) are read through finc_env, which
// remembers every switch that was found SET: finc_runtime_switches() reports them, bench.py refuses a judged run with any.
const char *finc_env(const char *name);
int finc_wino_form_override();   // 0 = the library's choice (finc_debug_set_forward_form)

// Row chunks of the forward kernels that run ONE wave per SIMD (F(4,3), its M-split, F(2,5)): a launch of `units` strips (waves or
// workgroups), of which the chip holds `slots` at a time, is cut into row chunks so that every slot has work; a chunk walks its rows
// plus `extra` rows of operands above them.  All units take the same time, so the chip works through units x chunks in ROUNDS of
// `slots`, and the cost of a split is rounds x (rows per chunk + extra).  The count that minimises it is returned (the smallest one
// among equals; chunks of at least `min_rows` rows).  Measured on the F(4,3) forward of c3, 64x64 (profiles/r05/notes/row_chunks.txt):
// B = 96 (384 strips): 3 chunks = 1,152 waves = two rounds of 24 rows 133 us, 5 chunks = two rounds of 15 rows 97 us; B = 160: 2 chunks
// 203 us, 3 chunks 155; B = 384: 1 chunk (two rounds of 66 rows) 395 us, 2 chunks (three rounds of 34) 355.
// `second_tenant`: the kernels that run TWO waves per SIMD (strip kernel, F(2,3)) pass 14 -- once a launch has more waves than SIMDs the
// tenants fill each other's issue gaps, a row costs 14/16 of what it costs a lone wave (F(2,3), c3 shape, B = 24: 5 chunks = 960 lone
// waves 34.5 us, 10 chunks = 1,920 waves in pairs 34.4; 4 against 8 chunks: 39.8 both) -- and count their rounds in SIMDs all the same:
// two tenants share one SIMD's MFMA pipe.  16 = no such effect (one wave per SIMD is all the registers allow).
inline int finc_row_chunks(long long units, long long slots, int H, int min_rows, int extra, int second_tenant = 16)
{
    const int maxc = H / min_rows > 0 ? H / min_rows : 1;
    long long best = -1;
    int nrc = 1;
    for (int c = 1; c <= maxc; ++c) {
        const int rc = (H + c - 1) / c;
        if ((H + rc - 1) / rc != c) continue;                     // (the same split as a smaller count)
        const long long rounds = (units * c + slots - 1) / slots;
        const long long cost = rounds * (rc + extra) * (units * c > slots ? second_tenant : 16);
        if (best < 0 || cost < best) { best = cost; nrc = c; }
    }
    return nrc;
}

// the measurement knobs each kernel translation unit was built with (finc_experiment.h); finc_build_flags() ORs them
unsigned finc_build_flags_mfma();
unsigned finc_build_flags_split();
unsigned finc_build_flags_conv();
unsigned finc_build_flags_gradw();
unsigned finc_build_flags_mix();
unsigned finc_build_flags_generic();
unsigned finc_build_flags_probe();

struct FincShape {
    int B, G, Cq, H, W, KH, KW;
    unsigned orient;
};

// The kernels that mark a lane's buffer offset (OFF_INVALID, OFF_BAD_CHANNEL: finc_device.h) take slabs [Cq][H][W] shorter than 1 GiB
// only: a marked offset must land beyond the slab and below 2^32.  Every launch rule of such a kernel asks this one predicate.
constexpr bool finc_slab_in_range(int Cq, int H, int W, int elem_bytes) { return (size_t)Cq * H * W * elem_bytes < ((size_t)1 << 30); }

// Band geometry of an inverse: lane p of a wave owns rows p, P + p, ... of the map, so the H rows form NB bands of P rows, solved one
// after the other; a band takes W steps and lane p trails lane p - 1 by one step, so the last lane finishes P - 1 steps behind the
// first: T = NB * W + P - 1 dependent steps in all (the reference's anti-diagonal order, band by band).
struct FincBands {
    int P, NB, T;
};
inline FincBands finc_bands(const FincShape &s)
{
    const int P = s.W < 16 ? s.W : 16;
    const int NB = P > 0 ? (s.H + P - 1) / P : 0;   // (callers reject W < 1 themselves, some only after asking)
    return {P, NB, NB * s.W + P - 1};
}

// ---- generic (reference-order) kernels: finc_generic.hip ----
int finc_launch_inverse_strict(const float *z, const float *wc, float *x, const FincShape &s, hipStream_t st);
int finc_launch_forward_generic(const float *x, const float *wc, float *z, const FincShape &s, hipStream_t st);
int finc_launch_inverse_strict_f64(const double *z, const double *wc, double *x, const FincShape &s, hipStream_t st);
int finc_launch_forward_generic_f64(const double *x, const double *wc, double *z, const FincShape &s, hipStream_t st);
int finc_launch_backward_generic(const float *gz, const float *x, const float *wc, float *gx, float *gw,
                                 const FincShape &s, hipStream_t st);
int finc_launch_backward_generic_f64(const double *gz, const double *x, const double *wc, double *gx, double *gw,
                                     const FincShape &s, hipStream_t st);
bool finc_backward_generic_has_gradw(int KH, int KW);   // false: finc_launch_backward_generic answers a grad-weight with FINC_ERR_UNSUPPORTED

// ---- inverse, MFMA wavefront kernel: finc_mfma.hip ----
// rows x Win floats -> rows x Wout floats (Wout > Win: zero fill on the right; Wout < Win: crop)
int finc_launch_repitch(const float *in, float *out, long long rows, int Win, int Wout, hipStream_t st);

bool finc_mfma_supported(int Cq, int H, int W, int KH, int KW);
size_t finc_mfma_packed_bytes(int G, int Cq, int KH, int KW);
// scale / shift [G*Cq] or nullptr: the affine map z = scale*y + shift folded in front of the inverse
int finc_mfma_pack(const float *wc, const float *scale, const float *shift, void *packed, int G, int Cq, int KH, int KW,
                   hipStream_t st);
// zpre: `in` is Linv * z already (the caller's channel mix applied blockdiag(Linv)): the helper-wave form without its z-term
int finc_mfma_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st, bool zpre = false);
bool finc_mfma_zpre_takes(const FincShape &s);
// can an affine map with a SHIFT be folded into the bank this problem set runs on? (not on finc_big.hip's kernels: the big
// banks and the wide-map takeover of the 33..64-channel banks carry a scale only)
bool finc_mfma_affine_takes(const FincShape &s);
bool finc_mfma_needs_align16(const FincShape &s);   // the kernel this problem set runs moves 16-byte pieces
// info[0..7] = {Cq padded, waves per problem, problems per workgroup, 32-byte I/O (1) or 16-byte (0), LDS bytes of a
// workgroup, workgroups, index into the instantiation table, rows of the table}; FINC_ERR_UNSUPPORTED if none applies
int finc_mfma_variant(int B, int G, int Cq, int H, int W, int KH, int KW, int *info);
// info[0..5] = {Cq padded, KH, KW, waves per problem, problems per workgroup, max_problems (0 = no limit)}
int finc_mfma_table_row(int row, int *info);
// waits of the helper-wave protocol that ran out of their spin budget since the library was loaded (synchronous copy)
int finc_mfma_hlp_timeouts(unsigned *count);

// Cq padded as the packed bank of (Cq, KH, KW) has it, or 0 when the shape has no MFMA instantiation
int finc_mfma_packed_cqp(int Cq, int KH, int KW);

// ---- inverse for the under-filled chip, role-split kernel: finc_split.hip (same packed bank as the wavefront kernel) ----
// finc_big.hip: 3x3 banks beyond the wavefront kernel's table (64 < Cq <= 96), 8 waves per problem, each owns 12 output channels
bool finc_big_bank(int Cq, int KH, int KW);
bool finc_big_wide_bank(int Cq, int KH, int KW);   // a bank of the wavefront kernel's table that finc_big.hip takes over on maps too wide for it
bool finc_big_supported(int Cq, int H, int W, int KH, int KW);
size_t finc_big_packed_bytes(int G, int Cq, int KH, int KW);
int finc_big_pack(const float *wc, const float *scale, const float *shift, void *packed, int G, int Cq, int KH, int KW, hipStream_t st);
int finc_big_info(const FincShape &s, int *waves, int *lds_bytes, int *cqp);
int finc_big_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st);
size_t finc_bigfwd_packed_bytes(int G, int Cq, int KH, int KW);         // 0: no big-bank forward for this bank
bool finc_bigfwd_takes(const FincShape &s, int align);
int finc_bigfwd_pack(const float *wc, void *packed, int G, int Cq, int KH, int KW, bool transpose, hipStream_t st, const float *scale,
                     const float *shift);
int finc_bigfwd_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st);
unsigned finc_build_flags_big();
// Which form of the role-split kernel a problem set takes, if any: the one place this is decided (finc_mfma.hip's inverse plan reads it,
// finc_split_launch runs it; only a band split short of progress words falls back to the chained form at launch)
struct FincSplitPlan {
    bool takes = false;            // this problem set runs on the role-split kernel
    bool chain = false;            // ... in its short-step form (finc_chain.hip)
    int row = -1;                  // the role-split kernel's instantiation (-1: the short-step form's)
    int nwg = 1;                   // workgroups per problem (band split)
    int waves = 0, lds = 0, steps = 0;   // of a workgroup
};
FincSplitPlan finc_split_plan(const FincShape &s);
int finc_split_prepare(hipStream_t st);          // allocates the band split's progress words for the current device (not inside a capture)
int finc_split_timeouts_count(unsigned *count);  // progress waits of the band split that gave up (must be 0)
unsigned *finc_fault_device_word();              // device pointer to the current device's (armed) fault word, or nullptr
int finc_split_launch(const float *in, const void *packed, float *out, const FincShape &s, const FincSplitPlan &p, hipStream_t st);
// finc_chain.hip: the short-step form of the same idea for the banks of up to 16 channels (output channels, not taps, shared out
// over the preparing waves); finc_split_plan / finc_split_launch hand over to it
bool finc_chain_takes(const FincShape &s);        // (can run it; finc_split_plan: does run it)
int finc_chain_info(const FincShape &s, int *waves, int *lds_bytes, int *steps);
int finc_chain_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st);
unsigned finc_build_flags_chain();

// ---- banks no register-resident kernel holds: the streaming-bank kernel, inverse and forward forms: finc_stream.hip ----
bool finc_stream_bank_ok(int Cq, int KH, int KW);                      // within its limits (Cq <= 256, KH, KW <= 7)
bool finc_stream_supported(int Cq, int H, int W, int KH, int KW, bool inverse);
size_t finc_stream_packed_bytes(int G, int Cq, int KH, int KW, bool inverse);
int finc_stream_pack(const float *wc, const float *scale, const float *shift, void *packed, int G, int Cq, int KH, int KW, bool inverse,
                     bool transpose, hipStream_t st);
int finc_mfma_remainder_images(const FincShape &s);
int finc_stream_info(const FincShape &s, bool inverse, int *cqp, int *lds, int *steps, int *waves = nullptr, int *one_wave_vec = nullptr);
int finc_stream_launch(const float *in, const void *packed, float *out, const FincShape &s, bool inverse, hipStream_t st);
unsigned finc_build_flags_stream();

// ---- forward / grad-input, MFMA strip kernel: finc_conv.hip ----
// bytes that both activations of a call are aligned to (16, 8 or 4): the `align` input of the forward kernels' *_takes
inline int finc_align(const void *a, const void *b)
{
    const uintptr_t x = (uintptr_t)a | (uintptr_t)b;
    return (x & 15u) == 0 ? 16 : (x & 7u) == 0 ? 8 : 4;
}
bool finc_conv_supported(int Cq, int H, int W, int KH, int KW);
size_t finc_conv_packed_bytes(int G, int Cq, int KH, int KW);
// scale / shift [G*Cq] or nullptr: z' = scale * conv(x) + shift folded into the bank (the affine layer BEHIND the conv)
int finc_conv_pack(const float *wc, void *packed, int G, int Cq, int KH, int KW, bool transpose, hipStream_t st,
                   const float *scale = nullptr, const float *shift = nullptr);
int finc_conv_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st);
// ---- 3x3 forward / grad-input with 1.5x fewer multiplies (Winograd F(2,3) along W): finc_wino.hip; its bank sits behind the
// strip kernels' in the packed buffer
size_t finc_wino_packed_bytes(int G, int Cq, int KH, int KW);          // 0: no Winograd kernel for this bank
bool finc_wino_takes(const FincShape &s, int align);
int finc_wino_pack(const float *wc, void *packed, int G, int Cq, bool transpose, hipStream_t st, const float *scale, const float *shift);
int finc_wino_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st);
bool finc_wino_disabled();                                          // FINC_NO_WINO / finc_debug_set_forward_form(1)
int finc_wino_pack_bank(const float *wc, float *packed, int G, int Cq, int MT, int MTB, int NK, int NF, bool transpose, hipStream_t st,
                        const float *scale, const float *shift);
// 3x3 banks of 28 .. 64 channels: F(4,3) along W, M-split over the waves of a workgroup (finc_wino4m.hip)
size_t finc_wino4m_packed_bytes(int G, int Cq, int KH, int KW);        // 0: no such kernel for this bank
bool finc_wino4m_takes(const FincShape &s, int align);
int finc_wino4m_pack(const float *wc, void *packed, int G, int Cq, bool transpose, hipStream_t st, const float *scale, const float *shift);
int finc_wino4m_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st);
unsigned finc_build_flags_wino4m();
int finc_wino_form(const FincShape &s);                                // 2: F(2,3), 4: F(4,3) -- which of the two a call runs
int finc_wino_set_form(int form);                                      // 0 library's choice, 1 strip kernel, 2 F(2,3), 4 F(4,3)
unsigned finc_build_flags_wino();
// ---- 5x5 forward / grad-input with 0.6 x the multiplies (Winograd F(2,5) along W): finc_wino5.hip; bank behind the strip kernels'
size_t finc_wino5_packed_bytes(int G, int Cq, int KH, int KW);         // 0: no such kernel for this bank
bool finc_wino5_takes(const FincShape &s, int align);
int finc_wino5_pack(const float *wc, void *packed, int G, int Cq, bool transpose, hipStream_t st, const float *scale, const float *shift);
int finc_wino5_launch(const float *in, const void *packed, float *out, const FincShape &s, hipStream_t st);
unsigned finc_build_flags_wino5();
// info[0..2] = {waves per strip (K-split), staged form (1) or dword form (0), strips per slab}; FINC_ERR_UNSUPPORTED: direct kernel
int finc_conv_variant(int B, int G, int Cq, int H, int W, int KH, int KW, int *info);
// The row chunks a forward / grad-input kernel launches with: strips of `strip` columns (`ns` per row), `waves` per workgroup, `nrc`
// chunks of `RC` rows on grid.y (the last one ragged).  One function per kernel decides them -- conv_plan for the strip kernel,
// finc_wino_rows (F(2,3) and F(4,3)), finc_wino4m_rows, finc_wino5_rows -- and both its launch and finc_conv_plan_info read that one.
struct FincRowPlan {
    int strip = 16, ns = 0, waves = 1;
    int nrc = 1, RC = 0;
};
FincRowPlan finc_wino_rows(const FincShape &s);
FincRowPlan finc_wino4m_rows(const FincShape &s);
FincRowPlan finc_wino5_rows(const FincShape &s);
int finc_bigfwd_waves(const FincShape &s);                             // waves of a workgroup of the big banks' M-split (0: no such bank)
// info[0..5] = {form (finc_conv_variant's info[1]; a pinned forward form is honoured), strip, ns, waves, nrc, RC} of a call whose
// activations are `align` bytes aligned; FINC_ERR_UNSUPPORTED: direct kernel
int finc_conv_plan_info(const FincShape &s, int align, int *info);

// ---- weight gradient, MFMA kernels + a reduce: finc_gradw.hip ----
// Which kernel a call runs and on which grid: finc_gradw_plan is the one place this is decided (the run-time switches are read there);
// finc_gradw_launch runs the plan, finc_gradw_variant and finc_gradw_workspace_bytes read it.  `align`: bytes gz and x are both
// aligned to (finc_align).
typedef void (*finc_gradw_fn)(const float *, const float *, float *, int, int, int, int, int, int, int, unsigned);
typedef void (*finc_gradw_pair_fn)(const float *, const float *, float *, int, int, int, int, int, int, int, unsigned, int);
typedef void (*finc_gradw_pair_reduce_fn)(const float *, float *, int, int, int, int);
struct FincGradwPlan {
    int form = 0;         // 0 none (the direct kernel, finc_generic.hip), 1 dword MFMA, 2 staged, 3 tiled, 4 Winograd, 5 Winograd tile-pair
    finc_gradw_fn fn = nullptr;             // main kernel of forms 1, 2, 4 ...
    finc_gradw_pair_fn fn_pair = nullptr;   // ... of forms 3, 5: one (o, i) tile pair per workgroup (takes mtt)
    dim3 grid, block = dim3(64);
    int wpg = 0;                            // workgroups per group: the partials the reduce sums
    int strip = 16, ns = 0;                 // strip width in columns, strips per row
    int mtt = 0;                            // 16-channel tiles on each side of the bank
    int cqp = 0, fs = 1;                    // form 4: the bank, waves per workgroup (frequency split)
    // the reduce: form 4 gradw_wino_reduce_kernel, form 5 this one (gradw_winot_reduce_kernel<KW>), forms 1..3 gradw_reduce_kernel
    finc_gradw_pair_reduce_fn reduce_pair = nullptr;
    dim3 rgrid;                             // the reduce's grid (blocks of 256 threads)
    size_t bytes = 0;                       // partial sums in the workspace
};
FincGradwPlan finc_gradw_plan(const FincShape &s, int align);
int finc_gradw_launch(const float *gz, const float *x, float *gw, void *workspace, const FincShape &s, const FincGradwPlan &p,
                      hipStream_t st);
int finc_gradw_variant(const FincShape &s);             // finc_gradw_plan(s, 16).form
size_t finc_gradw_workspace_bytes(const FincShape &s);  // room for the plans of 16-byte and of float-aligned activations (0: none)
// >= finc_gradw_workspace_bytes of every call on this bank with at most `units` = B * ceil(W / 16) strips; never shrinks when units grows
size_t finc_gradw_workspace_bound(int G, int Cq, int KH, int KW, long long units);

// ---- double precision on the matrix cores: finc_f64.hip.  One body per kernel in two families: one wave per problem (Cq <= 24 at 3x3,
// <= 32 at 2x2) and the M-split over a workgroup's waves (29 .. 64 at 3x3, 33 .. 64 at 2x2); 25 .. 28 at 3x3, wider banks and other
// filters have neither ----
// what a call on this shape launches: the one object the launchers, finc_f64_supported and finc_debug_f64_plan read
struct FincF64Plan {
    int family = 0;           // 0: no matrix-core kernel, 1: one wave per problem, 2: M-split
    int cqp = 0;              // the padded bank
    int waves = 0, ppw = 0;   // waves per problem (and per forward strip); inverse: problems per workgroup
    int lds = 0;              // inverse: bytes of LDS per workgroup
    int P = 0, DF = 0;        // inverse: rows per band, slots of the FIFO of rows above a band
    // forward / grad-input, both families: slab and strip on grid.x (B * G * ceil(W / 16) <= 2^31 - 1), grid.y = 1
    long long inv_grid = 0, fwd_grid_x = 0, fwd_grid_y = 0;
};
FincF64Plan finc_f64_plan(const FincShape &s);
bool finc_f64_supported(const FincShape &s);
size_t finc_f64_packed_bytes(int G, int Cq, int KH, int KW);          // 0: no such kernel for this bank
// what finc_f64_launch packs and runs (the value is the pack kernel's `forward`).  Grad-input: the forward on the bank with in/out
// channels exchanged -- called with every group's orientation complemented
enum FincF64Mode { FINC_F64_INVERSE = 0, FINC_F64_FORWARD = 1, FINC_F64_GRAD_INPUT = 2 };
// packs the bank into `packed` (finc_f64_packed_bytes) and runs the kernel of `mode` on it, all on `st`
int finc_f64_launch(const double *in, const double *wc, double *out, void *packed, const FincShape &s, FincF64Mode mode, hipStream_t st);
// weight gradient: pixels on the MFMA K dimension, one wave per (slab, row chunk), partial tiles in `workspace`, then a fixed-order
// reduce with the corner-tap mask.  The grid is not capped: a wave takes exactly one unit.
struct FincF64GradwPlan {
    int nrc = 0, RC = 0;      // row chunks per slab (0: no kernel for this bank) of RC rows, the last one ragged
    long long waves = 0;      // B * G * nrc waves (M-split family: times the row tiles of the bank, the waves of one workgroup)
    long long parts = 0;      // B * nrc partial tiles per (group, o, i, tap), summed in index order
    size_t bytes = 0;         // of the partials
};
FincF64GradwPlan finc_f64_gradw_plan(const FincShape &s);
// >= finc_f64_gradw_plan(s).bytes for every shape on this bank; never shrinks when B or H grows (0: no kernel for this bank)
size_t finc_f64_gradw_workspace_bound(int B, int G, int Cq, int H, int KH, int KW);
int finc_f64_gradw_launch(const double *gz, const double *x, double *gw, void *workspace, const FincShape &s, hipStream_t st);
unsigned finc_build_flags_f64();

// ---- per-pixel channel mixing (1x1 conv + folded affine): finc_mix.hip ----
bool finc_mix_supported(int C);
// transposed: out = mat^T * in (+ bias), `mat` still the row-major forward matrix (the mix's grad-input)
int finc_mix_launch(const float *in, const float *mat, const float *bias, float *out, int B, int C, int HW, hipStream_t st,
                    bool transposed = false);
// weight and bias gradient of the mix, pixels on the MFMA K dimension + a fixed-order reduce: finc_gradw.hip.  `align`: bytes
// grad_out and in are both aligned to (finc_align); gm or gb may be nullptr (in may be nullptr with gm)
size_t finc_mix_gradw_workspace_bytes(int B, int C, int HW);     // 0: no instantiation for C
int finc_mix_gradw_launch(const float *grad_out, const float *in, float *gm, float *gb, void *workspace, int B, int C, int HW,
                          int align, hipStream_t st);

// ---- the affine coupling's glue (transform + log-det, its backward, bias + ReLU): finc_coupling.h, compiled into finc_mix.o ----
// Which backward of a per-pixel layer (a mode of the family's one kernel body and one launcher): of direction +1, of direction -1,
// of direction +1 from its OUTPUT with the direction's input rebuilt in the same pass (training without stored activations), or (the
// coupling alone) of the split prior's forward: direction +1 with its outputs as two half tensors and a standard-normal score of the
// second one in the per-image sum; or (the coupling alone) of the split prior's merge, direction -1 with its inputs as two half
// tensors and the same score, from its OUTPUT.
enum FincGradMode { FINC_GRAD_FWD = 0, FINC_GRAD_REV = 1, FINC_GRAD_REBUILD = 2, FINC_GRAD_SPLIT = 3, FINC_GRAD_MERGE = 4 };
// C even; `ws` holds finc_coupling_workspace_floats floats (needed with logdet / ga / gb only); direction +1 forward, -1 reverse.
// logdet[b] = sum s in EITHER direction: the FORWARD map's log-det, at the recovered input when direction is -1; nullptr: none.
// `split` (glow.SplitPrior with its latent): the side that is NOT the whole [B][C][HW] tensor is two contiguous halves [B][C/2][HW] --
// direction +1 writes y (the untouched half) and yb (z2) from the whole x, direction -1 reads x (x1) and xb (z2) and writes the whole
// y -- and logdet becomes log p: sum s - 1/2 sum z2^2 - 1/2 (C/2) HW log 2 pi.  xb, yb: nullptr without `split`.
size_t finc_coupling_workspace_floats(int B, int C, int HW);
int finc_coupling_launch(const float *x, const float *xb, const float *raw, const float *a, const float *b, float *y, float *yb,
                         float *logdet, int B, int C, int HW, int direction, bool split, float *ws, hipStream_t st);
// v: the forward's input (FINC_GRAD_FWD, FINC_GRAD_SPLIT), the reverse's OUTPUT (FINC_GRAD_REV) or the forward's OUTPUT
// (FINC_GRAD_REBUILD, which also writes the rebuilt input xo); gld: the gradient of the log-det per image; gld, xo, gx, graw, ga, gb may
// be nullptr.  FINC_GRAD_SPLIT: gy and gz are the gradients of the two half tensors (either may be nullptr: zeros), gld that of log p;
// gz is nullptr in every other mode.  FINC_GRAD_MERGE: gy = grad_x (whole) and gld = grad_log_p, either may be nullptr; v = the
// merge's OUTPUT x; the results for the two half tensors are gx = grad_x1 and xo = grad_z2 [B][C/2][HW].
int finc_coupling_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *gld, const float *v, const float *raw,
                              const float *a, const float *b, float *xo, float *gx, float *graw, float *ga, float *gb, int B, int C, int HW,
                              float *ws, hipStream_t st);
int finc_bias_relu_launch(const float *in, const float *bias, float *out, int B, int C, int HW, hipStream_t st);
// The same three on bf16 tensors, given as their bits: raw and graw of the coupling (everything else stays fp32), in and out of the
// bias + ReLU (the bias stays fp32).  The wide forms want the bf16 pointers on 8 bytes (coupling) or 16 (bias + ReLU).
int finc_coupling_rawbf16_launch(const float *x, const float *xb, const uint16_t *raw, const float *a, const float *b, float *y, float *yb,
                                 float *logdet, int B, int C, int HW, int direction, bool split, float *ws, hipStream_t st);
int finc_coupling_rawbf16_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *gld, const float *v,
                                      const uint16_t *raw, const float *a, const float *b, float *xo, float *gx, uint16_t *graw, float *ga,
                                      float *gb, int B, int C, int HW, float *ws, hipStream_t st);
int finc_bias_relu_bf16_launch(const uint16_t *in, const float *bias, uint16_t *out, int B, int C, int HW, hipStream_t st);
// The Gaussianized split (glow.Split): the two `split` forms of finc_coupling_launch and the FINC_GRAD_SPLIT mode of
// finc_coupling_grad_launch under another arithmetic law -- raw channel 2j is the pre-activation of the mean m, 2j+1 that of the
// log-scale logs; direction +1: y = x1, yb = z2 = (x2 - m) * exp(-logs), direction -1: the whole y from x = x1 and xb = z2 with
// x2 = z2 * exp(logs) + m; log_p = -sum logs - 1/2 sum z2^2 - 1/2 (C/2) HW log 2 pi (nullptr with direction -1: none, `ws` untouched).
// The same geometry, workspace and pointer rules; fp32 raw only.  The backward takes FINC_GRAD_SPLIT or FINC_GRAD_MERGE, with the
// pointers as finc_coupling_grad_launch reads them in that mode.
int finc_gauss_split_launch(const float *x, const float *xb, const float *raw, const float *a, const float *b, float *y, float *yb,
                            float *log_p, int B, int C, int HW, int direction, float *ws, hipStream_t st);
int finc_gauss_split_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *glp, const float *v, const float *raw,
                                 const float *a, const float *b, float *xo, float *gx, float *graw, float *ga, float *gb, int B, int C,
                                 int HW, float *ws, hipStream_t st);
// ---- ActNorm (transform + log-det, its backward from the forward's OUTPUT, the data-dependent initialisation): finc_actnorm.h, same object ----
// `ws` holds finc_actnorm_workspace_floats floats (backward with gls / gt, and the initialisation)
size_t finc_actnorm_workspace_floats(int B, int C, int HW);
int finc_actnorm_launch(const float *x, const float *ls, const float *tr, float *y, float *logdet, int B, int C, int HW, int direction,
                        hipStream_t st);
// v: the forward's OUTPUT (FINC_GRAD_FWD; FINC_GRAD_REBUILD, which also writes the rebuilt input xo = v * exp(ls) + tr) or the
// reverse's INPUT (FINC_GRAD_REV: no gld); gld, tr and xo, gx, gls, gt may be nullptr
int finc_actnorm_grad_launch(FincGradMode mode, const float *gy, const float *gld, const float *v, const float *ls, const float *tr,
                             float *xo, float *gx, float *gls, float *gt, int B, int C, int HW, float *ws, hipStream_t st);
int finc_actnorm_init_launch(const float *x, float *ls, float *tr, int B, int C, int HW, float *ws, hipStream_t st);
// ---- the rational-quadratic spline (element-wise, linear tails): finc_spline.h, same object ----
// table [3 (K + 1)][P] knot-major (cumwidths, cumheights, derivatives), P = 1 or C * HW, 2 <= K <= 16 (the caller's checks); `ws`
// holds finc_spline_workspace_floats floats (needed with logdet / grad_table only).  logdet[b]: the FORWARD map's log-det in either
// direction.  x of the grad launch: the INPUT of the differentiated pass, the forward's (FINC_GRAD_FWD) or the reverse's
// (FINC_GRAD_REV); gy, gld, gx, gt may be nullptr.
size_t finc_spline_workspace_floats(int B, int C, int HW, int K, int P);
int finc_spline_launch(const float *x, const float *table, int P, int K, float tb, int direction, float *y, float *logdet, int B, int C,
                       int HW, float *ws, hipStream_t st);
int finc_spline_grad_launch(FincGradMode mode, const float *gy, const float *gld, const float *x, const float *table, int P, int K, float tb,
                            float *gx, float *gt, int B, int C, int HW, float *ws, hipStream_t st);
// ---- the smooth invertible activations (element-wise on [B][C * HW]): finc_activation.h, same object ----
// kind: FincActivationKind; p0, p1 its parameters (a; a, b), `slope` the learnable kind's device pointer (nullptr otherwise); `ws` holds
// finc_activation_workspace_floats floats (needed with logdet / gs only).  logdet[b]: the FORWARD map's log-det in either direction.
// v of the grad launch: the forward's INPUT (FINC_GRAD_FWD), the reverse's OUTPUT (FINC_GRAD_REV) or the forward's OUTPUT
// (FINC_GRAD_REBUILD, which also writes the rebuilt input xo); gy, gld, xo, gx, gs may be nullptr.
size_t finc_activation_workspace_floats(int B, int C, int HW);
int finc_activation_trips(int kind);
int finc_activation_launch(int kind, float p0, float p1, const float *slope, int direction, const float *x, float *y, float *logdet, int B,
                           int C, int HW, float *ws, hipStream_t st);
int finc_activation_grad_launch(int kind, float p0, float p1, const float *slope, FincGradMode mode, const float *gy, const float *gld,
                                const float *v, float *xo, float *gx, float *gs, int B, int C, int HW, float *ws, hipStream_t st);
// ---- the image boundary (dequantise + normalise + logit + squeeze in one launch, and back): finc_image.h, same object ----
// B, C, H, W: the IMAGE side; with (un)squeeze the other side is [B][4C][H/2][W/2].  `ws` holds finc_image_workspace_floats floats
// (the encode always, the decode with logdet).  noise and the decode's logdet may be nullptr.
size_t finc_image_workspace_floats(int B, int C, int H, int W, int squeeze);
int finc_image_encode_u8_launch(const uint8_t *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                                float m, float c, float hi, float c2, float ldc, float *ws, hipStream_t st);
int finc_image_encode_f32_launch(const float *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                                 float m, float c, float hi, float c2, float ldc, float *ws, hipStream_t st);
int finc_image_decode_f32_launch(const float *z, float *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off,
                                 float hi, float ldc, float *ws, hipStream_t st);
int finc_image_decode_u8_launch(const float *z, uint8_t *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off,
                                float hi, float ldc, float *ws, hipStream_t st);
// ---- backward through the unit's inverse (adjoint bank, lead product, the weight gradient's sign): finc_adjoint.h, same object ----
// w_adj [G*Cq][Cq][KH][KW]: the canonical bank whose inverse (orientation complemented) is the adjoint solve up to the lead product;
// lead_t [C][C]: blockdiag(Linv_g^T), row = output channel
int finc_adjoint_weights_launch(const float *wc, float *w_adj, float *lead_t, int G, int Cq, int KH, int KW, hipStream_t st);
// v <- blockdiag(L^-T) v in place: finc_mix_launch where the channel count has an instantiation, the grouped kernel otherwise
int finc_lead_launch(float *v, const float *lead_t, int B, int G, int Cq, int HW, hipStream_t st);
int finc_negate_launch(float *p, size_t n, hipStream_t st);
// ---- what a per-pixel call would launch, by launch rule (finc_debug_pixel_plan): finc_mix.hip, from the launchers' own functions ----
// rule / family as FincPixelRule / FincPixelFamily of include/finc.h; `groups`: FINC_PIXEL_LEAD's G; `align`: 4, 8 or 16, the common
// alignment of the activation pointers; `elem_bytes`: 4, or 2 for the bf16 raw of the coupling / the bf16 tensors of bias + ReLU.
// info[8] = {io, threads, grid, parts, items, trips, outer, lds}.  Launches nothing.
int finc_pixel_plan_info(int rule, int family, int groups, int B, int C, int HW, int align, int elem_bytes, long long *info);
// ---- the PLU-parametrised 1x1 convolution's parameter work (W, W^-1, log|det W| and their backward): finc_plu.h, same object ----
// the widest matrix the compose kernels take: the staged rows of a workgroup are 88 bytes of LDS per channel
constexpr int FINC_PLU_MAX_C = 512;
bool finc_plu_supported(int C);
// any of w [C][C], w_inv [C][C], logdet (one float), each nullptr when not wanted
int finc_plu_compose_launch(const float *lower, const float *upper, const float *log_s, const float *sign_s, const int *perm, float *w,
                            float *w_inv, float *logdet, int C, hipStream_t st);
// from gw = dl/dW [C][C] and g_ld = dl/dlogdet (one float or nullptr): any of g_lower, g_upper [C][C], g_log_s [C]
int finc_plu_compose_bwd_launch(const float *gw, const float *g_ld, const float *lower, const float *upper, const float *log_s,
                                const float *sign_s, const int *perm, float *g_lower, float *g_upper, float *g_log_s, int C, hipStream_t st);
