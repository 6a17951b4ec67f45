// Device prelude of the kernel files (gfx950 only): the small rules every kernel family shares, each stated once.  Where the other
// shared rules live: chan_d, the tile maps and the grad-weight kernels' strip-piece map in finc_tile.h; the slab limit the range
// marks rest on (finc_slab_in_range) and the band geometry of an inverse (finc_bands) in finc_common.h.
#pragma once
#include <stddef.h>

#include <type_traits>

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Guard-band marks of a buffer access's per-lane byte offset (voffset).  The buffer unit compares offset + access size with the
// descriptor's byte count: beyond it a load returns 0 and a store is dropped, so a lane that has nothing to move needs no branch.
// OFF_INVALID replaces an offset: 2 GiB lies beyond any slab.  OFF_BAD_CHANNEL is ADDED (or OR-ed) to an offset that would be valid
// for another channel or column -- a channel behind the bank, a column outside the row -- and the sum must still land beyond the
// slab and must not wrap: with a slab shorter than 1 GiB the sum lies in [1 GiB, 2 GiB + row offsets), past the slab, below 2^32.
// Every launch rule whose kernel uses the marks therefore refuses slabs of 1 GiB and more: finc_slab_in_range (finc_common.h).
constexpr unsigned OFF_INVALID = 0x80000000u;
constexpr unsigned OFF_BAD_CHANNEL = 0x40000000u;

template <int I>
using IC = std::integral_constant<int, I>;
#define FINC_SB() __builtin_amdgcn_sched_barrier(0)

// `bytes` of a tensor from element `first` on, as a raw buffer resource.  The last word of the descriptor: DATA_FORMAT = 32 bits (bit
// 17) and nothing else -- stride 0, no swizzle, no index: a raw buffer whose range check is offset + size <= bytes.  Build it from
// wave-uniform values only.  _IF, `ok` (wave-uniform) false: zero bytes long, for a row or problem that does not exist -- every
// load through it gives 0 and every store is dropped.
// Macros, not functions: a descriptor built per row or per chunk sits in a lambda that the early simplification passes see before
// any inlining happens, a forced one included; a call there changed the code of 73 kernels (finc_gradw.hip, finc_conv.hip), the
// macro changes none (profiles/device_prelude/isa_identity.txt).
#define FINC_SLAB_RSRC(base, first, bytes) __builtin_amdgcn_make_buffer_rsrc((void *)((base) + (first)), 0, (int)(bytes), 0x00020000)
#define FINC_SLAB_RSRC_IF(base, first, bytes, ok) FINC_SLAB_RSRC(base, first, (ok) ? (int)(bytes) : 0)

// lane i of each 16-lane row <- lane i-N; lanes i < N keep `old`  (the attribute spelled out: the host tests include this file
// without the runtime's header)
template <int N>
__device__ inline __attribute__((always_inline)) float row_shr(float old, float src)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), 0x110 + N,
                                                                 0xf, 0xf, false));
}

// The taps the preparing waves of the role-split and short-step inverses take (a + b >= 2), ordered by a + b (then row-major): the
// taps with a + b == 2 come first -- they are the only ones that need the pixel solved in the step before, so shared out round-robin
// every preparing wave gets one of them.  (The wavefront kernel walks the same taps row-major: finc_mfma.hip RowMajorTaps.)
template <int KH, int KW>
struct BySumTaps {
    static constexpr int count()
    {
        int n = 0;
        for (int a = 0; a < KH; ++a)
            for (int b = 0; b < KW; ++b) n += (a + b >= 2);
        return n;
    }
    static constexpr int find(int i, bool want_a)
    {
        for (int sum = 2; sum <= KH + KW - 2; ++sum)
            for (int a = 0; a < KH; ++a)
                for (int b = 0; b < KW; ++b)
                    if (a + b == sum && i-- == 0) return want_a ? a : b;
        return 0;
    }
    static constexpr int a_of(int i) { return find(i, true); }
    static constexpr int b_of(int i) { return find(i, false); }
};

// Diagnostic builds of the role-split and short-step inverses (-DFINC_SPLIT_STAMP): busy cycles, barrier exit -> next barrier arrival,
// summed into the caller's `st_busy`.  The stamp's lgkmcnt(0) drains the LDS queue: read the SHARES of such a build, never its run time.
#ifdef FINC_SPLIT_STAMP
#define FINC_ST_BEGIN() unsigned long long st_b_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_b_)::"memory")
#define FINC_ST_END()                                                                                                     \
    do {                                                                                                                  \
        unsigned long long st_e_;                                                                                         \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_e_)::"memory");             \
        st_busy += st_e_ - st_b_;                                                                                         \
    } while (0)
#else
#define FINC_ST_BEGIN() do { } while (0)
#define FINC_ST_END() do { } while (0)
#endif
