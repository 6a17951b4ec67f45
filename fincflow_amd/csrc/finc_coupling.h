// The affine coupling's glue for gfx950 (included by finc_mix.hip: same object file, the per-pixel streaming neighbours of the unit).
//
// Reference: layers/coupling.py:44-105 (Coupling) around layers/coupling.py:9-41 (Conv2dZero).  Behind the coupling net's last
// convolution the reference runs twelve elementwise launches -- bias add, logs * 3, exp, broadcast multiply, / 2, tanh, * 2, neg, exp,
// sub, mul, cat -- and two more (bias add, ReLU) behind each of the first two convolutions.  Here:
//   * finc_coupling_kernel      one pass: h = a * raw + b per channel, s = 2 tanh(u / 2), y2 = x2 * exp(s) + t  (forward, + log-det)
//                               or y2 = (x2 - t) * exp(-s) (reverse); the untouched half is copied by the same threads.
//   * cpl_grad<V, MODE>         one pass: every gradient of one direction; s and exp(s) are recomputed from raw (two
//                               transcendentals per element) instead of being saved: saving them would add two tensor writes to the
//                               forward and two reads here, and this body is bound by its memory traffic, not by the VALU.  Its modes
//                               are the kernels finc_coupling_bwd_kernel (forward direction, from its input),
//                               finc_coupling_rev_bwd_kernel (reverse direction, from its OUTPUT: what `reverse` under autograd
//                               records inside ops.reverse_grad()) and finc_coupling_recon_kernel (forward direction from its OUTPUT,
//                               which also writes the rebuilt input: the step of a training backward that stores no activations).
//   * finc_splitprior_kernel    the split prior with its latent (glow.SplitPrior.split / merge): the transform with one side as two
//                               half tensors, and log p = sum s - 1/2 sum z2^2 - c per image from the same pass; its backward,
//                               finc_splitprior_bwd_kernel, is cpl_grad's fourth mode.
//   * finc_gauss_split_kernel   the Gaussianized split (glow.Split: layers/split.py:24-52): the split prior's two bodies under another
//                               arithmetic law (CPL_LAW_GAUSS) -- raw channel 2j = the mean's pre-activation, 2j+1 = the log-scale's,
//                               z2 = (x2 - m) * exp(-logs), log p = -sum logs - 1/2 sum z2^2 - c; its backward is
//                               finc_gauss_split_bwd_kernel.  fp32 raw only.
//   * finc_splitprior_merge_bwd_kernel, finc_gauss_merge_bwd_kernel  the backward of the two merges (the split forms in direction
//                               -1) from the merge's OUTPUT x: cpl_grad's fifth mode under either law -- what a recorded
//                               glow.SplitPrior.merge / glow.Split.merge launches inside ops.reverse_grad().
//   * finc_coupling_rev_logdet_kernel  the reverse pass that also sums s per image: the sample and the forward log-det at the
//                               sample in one pass (FlowSequential.sample_with_log_prob / rsample_with_log_prob).
//   * finc_bias_relu_kernel     out = max(in + bias[c], 0), in place or not.
// Layout: x, y [B][C][HW] fp32, raw [B][C][HW] with channel 2j = u_j (pre-activation of the log-scale) and 2j+1 = t_j (translation).
// A thread owns V consecutive pixels of one channel pair j: V = 4 (16-byte pieces) when HW % 4 == 0 and every pointer is 16-byte
// aligned, else V = 1 (dwords).  Every index is checked against the element count: nothing is read or written beyond a tensor.
// The raw element type R is a parameter of the two bodies, float or __bf16 (a net that ran under bf16 autocast): a bf16 raw is read
// as it lies (bf16 -> fp32 is a 16-bit shift, exact), 8-byte pieces in the wide form -- which then also needs raw and grad_raw on
// 8 bytes -- and 2-byte elements in the narrow one; grad_raw is written in R, rounded to nearest even once, behind the fp32 sums.
// Everything else -- x, y, the gradients of x, a, b, the log-det, the partials -- is fp32 in both, and the arithmetic is the same
// lines: a bf16 raw gives the bits of the fp32 call on the same values.  The *_rawbf16_* kernels and finc_bias_relu_bf16_kernel
// (bf16 in and out, fp32 bias and arithmetic, 16-byte pieces of 8) have names of their own: the fp32 kernels stay the ones they were.
// Sums (log-det per image; grad_a, grad_b per channel) never use atomics: each workgroup reduces its share in a fixed order (wave
// butterflies, then the four waves in LDS) and writes ONE partial to the workspace; finc_coupling_reduce_kernel adds the partials of
// an output in a fixed order.  The same inputs give the same bits.
#ifndef FINC_COUPLING_H
#define FINC_COUPLING_H

namespace {

typedef float cpl_v4f __attribute__((ext_vector_type(4)));
constexpr int CPL_THREADS = 256;
// The arithmetic law of a body: the affine coupling's (s = 2 tanh(h[2j] / 2), t = h[2j+1]: y2 = x2 * exp(s) + t) or the Gaussianized
// split's (m = h[2j], logs = h[2j+1]: z2 = (x2 - m) * exp(-logs)), which exists in the SPLIT forms only.
constexpr int CPL_LAW_COUPLING = 0, CPL_LAW_GAUSS = 1;

template <int V>
__device__ inline void cpl_load(float (&d)[V], const float *p)
{
    if constexpr (V == 4) {
        const cpl_v4f v = *reinterpret_cast<const cpl_v4f *>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
        d[0] = *p;
    }
}
template <int V>
__device__ inline void cpl_store(float *p, const float (&d)[V])
{
    if constexpr (V == 4) {
        cpl_v4f v;
        v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
        *reinterpret_cast<cpl_v4f *>(p) = v;
    } else {
        *p = d[0];
    }
}

// bf16 elements travel as their bits (integer loads and stores of 2, 8 or 16 bytes: no 4-byte access ever touches a 2-byte element
// on its own); up: the bits are the float's high half; down: the compiler's float -> __bf16 conversion, round to nearest even.
typedef float cpl_v2f __attribute__((ext_vector_type(2)));
typedef __bf16 cpl_v2h __attribute__((ext_vector_type(2)));
__device__ inline void cpl_widen(float &lo, float &hi, unsigned w)
{
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xffff0000u);
}
__device__ inline unsigned cpl_narrow(float lo, float hi)
{
    cpl_v2f f;
    f.x = lo; f.y = hi;
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, cpl_v2h));
}
template <int V>
__device__ inline void cpl_load(float (&d)[V], const __bf16 *p)
{
    if constexpr (V == 8) {
        const uint4 w = *reinterpret_cast<const uint4 *>(p);
        cpl_widen(d[0], d[1], w.x); cpl_widen(d[2], d[3], w.y); cpl_widen(d[4], d[5], w.z); cpl_widen(d[6], d[7], w.w);
    } else if constexpr (V == 4) {
        const uint2 w = *reinterpret_cast<const uint2 *>(p);
        cpl_widen(d[0], d[1], w.x); cpl_widen(d[2], d[3], w.y);
    } else {
        d[0] = __uint_as_float((unsigned)*reinterpret_cast<const unsigned short *>(p) << 16);
    }
}
template <int V>
__device__ inline void cpl_store(__bf16 *p, const float (&d)[V])
{
    if constexpr (V == 8) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(cpl_narrow(d[0], d[1]), cpl_narrow(d[2], d[3]), cpl_narrow(d[4], d[5]), cpl_narrow(d[6], d[7]));
    } else if constexpr (V == 4) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(cpl_narrow(d[0], d[1]), cpl_narrow(d[2], d[3]));
    } else {
        *reinterpret_cast<unsigned short *>(p) = __builtin_bit_cast(unsigned short, (__bf16)d[0]);
    }
}

// Sum of N values per thread over the 256 threads of a workgroup, in a fixed order; every thread returns with the totals in v[].
template <int N>
__device__ inline void cpl_block_sum(float (&v)[N], float (*sm)[4])
{
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sm[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (sm[k][0] + sm[k][1]) + (sm[k][2] + sm[k][3]);
}

// Workgroup = (image, part): P parts per image share its half * HW / V thread items.  DIR +1 forward, -1 reverse.
// y == x is allowed (a thread reads its pieces before it writes them, and nobody else touches them).
// LOGDET: the workgroup's partial of sum s goes to part[blockIdx.x], in EITHER direction: what is summed is the FORWARD map's log-det,
// sum_{j,p} s_j -- in the reverse direction that is the log-det of Coupling.forward at the recovered input y (s depends on the
// untouched half only, which both directions share); the reverse map's own Jacobian is its negative.
// SPLIT (glow.SplitPrior with its latent): the side that is not the whole tensor is two contiguous halves [B][half][HW] -- DIR +1
// writes y = the untouched half and yb = z2 (the split), DIR -1 reads x = x1 and xb = z2 (the merge); xb / yb are unused otherwise.
// Nothing may overlap then.  The arithmetic lines are the same, so the halves carry the bits of the whole-tensor call.  With LOGDET
// the partial is sum s - 1/2 sum z2^2, z2 the forward's output (DIR +1) or the reverse's input (DIR -1), and part 0 of every image
// also takes -c (c = 1/2 half HW log 2 pi): the reduce then gives log p = the coupling's log-det + the standard-normal score of z2.
// LAW = CPL_LAW_GAUSS (SPLIT only): u is the pre-activation of the mean and t that of the log-scale, DIR +1 is z2 = (x2 - m) *
// exp(-logs), DIR -1 is x2 = z2 * exp(logs) + m, and the first sum is -sum logs (the split's log-det) in both.
template <int V, int DIR, bool LOGDET, typename R = float, bool SPLIT = false, int LAW = CPL_LAW_COUPLING>
__device__ __forceinline__ void cpl_transform(const float *x, const float *xb, const R *__restrict__ raw, const float *__restrict__ a,
                                              const float *__restrict__ b, float *y, float *yb, float *__restrict__ part, float c, int half,
                                              int HW, int nv, int items, int P)
{
    static_assert(LAW == CPL_LAW_COUPLING || SPLIT, "the Gaussianized law has the split forms only");
    constexpr int NS = SPLIT && LOGDET ? 2 : 1;                            // sums per thread: s, and z2^2 for the split prior
    const int img = (int)blockIdx.x / P, pi = (int)blockIdx.x - img * P;
    const size_t ibase = (size_t)img * (size_t)(2 * half) * (size_t)HW, hbase = (size_t)img * (size_t)half * (size_t)HW;
    float ls[NS] = {};
    for (int idx = pi * CPL_THREADS + (int)threadIdx.x; idx < items; idx += P * CPL_THREADS) {
        const int j = idx / nv, p = (idx - j * nv) * V;
        const size_t o1 = ibase + (size_t)j * HW + p, o2 = o1 + (size_t)half * HW, oh = hbase + (size_t)j * HW + p;
        const size_t ou = ibase + (size_t)(2 * j) * HW + p, ot = ou + HW;
        float x1[V], x2[V], u[V], t[V], y2[V];
        if constexpr (SPLIT && DIR < 0) {
            cpl_load<V>(x1, x + oh);
            cpl_load<V>(x2, xb + oh);
        } else {
            cpl_load<V>(x1, x + o1);
            cpl_load<V>(x2, x + o2);
        }
        cpl_load<V>(u, raw + ou);
        cpl_load<V>(t, raw + ot);
        const float au = a[2 * j], bu = b[2 * j], at = a[2 * j + 1], bt = b[2 * j + 1];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if constexpr (LAW == CPL_LAW_GAUSS) {
                const float m = fmaf(au, u[e], bu), logs = fmaf(at, t[e], bt);
                if constexpr (DIR > 0) y2[e] = (x2[e] - m) * expf(-logs);
                else y2[e] = fmaf(x2[e], expf(logs), m);
                if constexpr (LOGDET) {
                    const float z = DIR > 0 ? y2[e] : x2[e];
                    ls[0] -= logs;
                    ls[NS - 1] = fmaf(z, z, ls[NS - 1]);
                }
            } else {
                const float s = 2.f * tanhf(0.5f * fmaf(au, u[e], bu));
                const float tr = fmaf(at, t[e], bt);
                if constexpr (DIR > 0) {
                    y2[e] = fmaf(x2[e], expf(s), tr);
                    if constexpr (LOGDET) ls[0] += s;
                    if constexpr (NS == 2) ls[NS - 1] = fmaf(y2[e], y2[e], ls[NS - 1]);
                } else {
                    y2[e] = (x2[e] - tr) * expf(-s);
                    if constexpr (LOGDET) ls[0] += s;
                    if constexpr (NS == 2) ls[NS - 1] = fmaf(x2[e], x2[e], ls[NS - 1]);
                }
            }
        }
        if constexpr (SPLIT && DIR > 0) {
            cpl_store<V>(y + oh, x1);
            cpl_store<V>(yb + oh, y2);
        } else {
            cpl_store<V>(y + o1, x1);
            cpl_store<V>(y + o2, y2);
        }
    }
    if constexpr (LOGDET) {
        __shared__ float sm[NS][4];
        cpl_block_sum<NS>(ls, sm);
        if (threadIdx.x == 0) {
            if constexpr (NS == 2) part[blockIdx.x] = fmaf(-0.5f, ls[NS - 1], ls[0]) - (pi == 0 ? c : 0.f);
            else part[blockIdx.x] = ls[0];
        }
    }
}

template <int V, int DIR, bool LOGDET>
__global__ __launch_bounds__(CPL_THREADS) void finc_coupling_kernel(const float *x, const float *__restrict__ raw,
                                                                    const float *__restrict__ a, const float *__restrict__ b, float *y,
                                                                    float *__restrict__ part, int half, int HW, int nv, int items, int P)
{
    cpl_transform<V, DIR, LOGDET>(x, nullptr, raw, a, b, y, nullptr, part, 0.f, half, HW, nv, items, P);
}

// The reverse direction WITH the log-det partials (sampling with its log-density): cpl_transform<V, -1, true> under a name of its
// own, so that the six instantiations of finc_coupling_kernel stay the six they were.
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_coupling_rev_logdet_kernel(const float *x, const float *__restrict__ raw,
                                                                               const float *__restrict__ a, const float *__restrict__ b,
                                                                               float *y, float *__restrict__ part, int half, int HW, int nv,
                                                                               int items, int P)
{
    cpl_transform<V, -1, true>(x, nullptr, raw, a, b, y, nullptr, part, 0.f, half, HW, nv, items, P);
}

// Either direction, with or without the partials, on a bf16 raw: the same body, R = __bf16.
template <int V, int DIR, bool LOGDET>
__global__ __launch_bounds__(CPL_THREADS) void finc_coupling_rawbf16_kernel(const float *x, const __bf16 *__restrict__ raw,
                                                                            const float *__restrict__ a, const float *__restrict__ b,
                                                                            float *y, float *__restrict__ part, int half, int HW, int nv,
                                                                            int items, int P)
{
    cpl_transform<V, DIR, LOGDET, __bf16>(x, nullptr, raw, a, b, y, nullptr, part, 0.f, half, HW, nv, items, P);
}

// The split prior's two transforms (SPLIT): DIR +1 always with log p, DIR -1 with or without it; R = float or __bf16.  Nothing
// overlaps here, so every pointer is __restrict__.
template <int V, int DIR, bool LOGP, typename R>
__global__ __launch_bounds__(CPL_THREADS) void finc_splitprior_kernel(const float *__restrict__ x, const float *__restrict__ xb,
                                                                      const R *__restrict__ raw, const float *__restrict__ a,
                                                                      const float *__restrict__ b, float *__restrict__ y,
                                                                      float *__restrict__ yb, float *__restrict__ part, float c, int half,
                                                                      int HW, int nv, int items, int P)
{
    cpl_transform<V, DIR, LOGP, R, true>(x, xb, raw, a, b, y, yb, part, c, half, HW, nv, items, P);
}

// The Gaussianized split's two transforms: the same forms (DIR +1 always with log p, DIR -1 with or without it) under CPL_LAW_GAUSS.
template <int V, int DIR, bool LOGP>
__global__ __launch_bounds__(CPL_THREADS) void finc_gauss_split_kernel(const float *__restrict__ x, const float *__restrict__ xb,
                                                                       const float *__restrict__ raw, const float *__restrict__ a,
                                                                       const float *__restrict__ b, float *__restrict__ y,
                                                                       float *__restrict__ yb, float *__restrict__ part, float c, int half,
                                                                       int HW, int nv, int items, int P)
{
    cpl_transform<V, DIR, LOGP, float, true, CPL_LAW_GAUSS>(x, xb, raw, a, b, y, yb, part, c, half, HW, nv, items, P);
}

// Every backward of the coupling is ONE body, cpl_grad<V, MODE>; a mode (FincGradMode) is what it reads and the few lines of
// arithmetic behind `if constexpr`:
//   FINC_GRAD_FWD      of y2 = x2 * exp(s) + t, from `v` = the forward's INPUT x (layers/coupling.py:79-93).
//   FINC_GRAD_REV      of y2 = (x2 - t) * exp(-s) (layers/coupling.py:95-101), from `v` = the reverse's OUTPUT y: d y2 / d x2 = E =
//                      exp(-s), d y2 / d t = -E, d y2 / d s = -y2, so the input is not needed (in a recorded reverse chain y is the
//                      tensor the next layer keeps anyway).  gld: the gradient of the log-det finc_coupling_rev_logdet_kernel reports
//                      (sum s, per image), d / d s = gld[img]; nullptr = none, and then every result has the bits of a backward
//                      without that argument: the neutral element is -0 in THIS mode (v + -0 is v for every v, -0 included).
//   FINC_GRAD_REBUILD  of the forward direction from `v` = the forward's OUTPUT y, which also rebuilds the forward's input into xo:
//                      with d = y2 - t, x2 = d * exp(-s) (the arithmetic of finc_coupling_kernel's reverse direction, so the same
//                      bits), and x2 * exp(s) = d: grad_x2 = grad_y2 * exp(s), grad_h[2j+1] = grad_y2, grad_h[2j] = (grad_y2 * d +
//                      gld[img]) * (1 - th^2).  What a training step without stored activations runs per coupling: one launch instead
//                      of a reverse launch plus a backward launch; y and raw are read once.  xo == v and gx == gy are allowed here (a
//                      thread reads its pieces before it writes them, and nobody else touches them).
//   FINC_GRAD_SPLIT    of the split prior's forward (cpl_transform<V, +1, true, R, true>: x1, z2, log p = sum s - 1/2 sum z2^2 - c),
//                      from `v` = the forward's INPUT x.  gy = grad_x1 and gz = grad_z2 are contiguous HALVES [B][half][HW], gld =
//                      grad_log_p; each may be nullptr (zeros).  E = exp(s) and z2 = fma(x2, E, t) are recomputed, G = grad_z2 -
//                      grad_log_p[img] * z2 is what reaches z2 in all, and the FWD mode's lines follow with G in the place of g2.
//                      gz is nullptr in every other mode.  With LAW = CPL_LAW_GAUSS (this mode only) the forward is the Gaussianized
//                      split's: E = exp(-logs) and z2 = (x2 - m) * E are recomputed, G = grad_z2 - grad_log_p[img] * z2,
//                      grad_x2 = G * E, grad_h[2j] (the mean's) = -grad_x2, grad_h[2j+1] (the log-scale's) = -(G * z2 + grad_log_p).
//   FINC_GRAD_MERGE    of the split prior's merge (cpl_transform<V, -1, LOGP, R, true>: x2 = (z2 - t) * exp(-s), log p = sum s -
//                      1/2 sum z2^2 - c), from `v` = the merge's OUTPUT x, the convention of FINC_GRAD_REV.  gy = grad_x [B][C][HW]
//                      and gld = grad_log_p, either may be nullptr (zeros); the two results of the untouched side are contiguous
//                      HALVES [B][half][HW]: gx = grad_x1 (the first half of grad_x, copied: the direct share only) and xo = grad_z2.
//                      With g2 = grad_x's second half and E = exp(-s): grad_z2 = g2 * E - grad_log_p * z2, z2 = fma(x2, exp(s), t)
//                      recomputed only when there is a grad_log_p; grad_t = -(g2 * E), grad_s = -(g2 * x2) + grad_log_p: the REV
//                      mode's expression trees, so that without grad_log_p grad_raw, grad_a, grad_b and grad_z2 carry that mode's
//                      bits.  With LAW = CPL_LAW_GAUSS the merge is the Gaussianized split's, x2 = z2 * exp(logs) + m, log p =
//                      -sum logs - 1/2 sum z2^2 - c: d = x2 - m, z2 = d * exp(-logs), grad_z2 = g2 * exp(logs) - grad_log_p * z2,
//                      grad_h[2j] = g2, grad_h[2j+1] = g2 * d - grad_log_p.
// s and exp(s) are recomputed from raw (two transcendentals per element), not saved by the forward.
// Workgroup = (channel pair j, part): Q parts per pair share its B * HW / V thread items, so the four per-channel sums of a
// workgroup belong to ONE pair.  Partials: part[(4j + k) * Q + q], k = 0 grad_a[2j], 1 grad_b[2j], 2 grad_a[2j+1], 3 grad_b[2j+1].
// gld (grad of the log-det, per image), xo, gx, graw may be nullptr; `sums` = 0 skips the partials.  R: the element type of raw and
// of graw, which is rounded from the fp32 gu, gt behind the sums (the sums never see a rounded value).
template <int V, int MODE, typename R = float, int LAW = CPL_LAW_COUPLING>
__device__ __forceinline__ void cpl_grad(const float *gy, const float *gz, const float *__restrict__ gld, const float *v,
                                         const R *__restrict__ raw,
                                         const float *__restrict__ a, const float *__restrict__ b, float *xo, float *gx,
                                         R *__restrict__ graw, float *__restrict__ part, int half, int HW, int nv, int items, int Q,
                                         int sums)
{
    constexpr bool REBUILD = MODE == FINC_GRAD_REBUILD, SPLIT = MODE == FINC_GRAD_SPLIT, MERGE = MODE == FINC_GRAD_MERGE;
    constexpr bool GAUSS = LAW == CPL_LAW_GAUSS;
    static_assert(!GAUSS || SPLIT || MERGE, "the Gaussianized law has the split and merge modes");
    const int j = (int)blockIdx.x / Q, qi = (int)blockIdx.x - j * Q;
    const float au = a[2 * j], bu = b[2 * j], at = a[2 * j + 1], bt = REBUILD || SPLIT || MERGE ? b[2 * j + 1] : 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int idx = qi * CPL_THREADS + (int)threadIdx.x; idx < items; idx += Q * CPL_THREADS) {
        const int img = idx / nv, p = (idx - img * nv) * V;
        const size_t ibase = (size_t)img * (size_t)(2 * half) * (size_t)HW;
        const size_t o1 = ibase + (size_t)j * HW + p, o2 = o1 + (size_t)half * HW;
        const size_t ou = ibase + (size_t)(2 * j) * HW + p, ot = ou + HW;
        float g1[V], g2[V], v1[V], v2[V], u[V], t[V], x2[V], gx2[V], gu[V], gt[V];
        if constexpr (SPLIT) {
            const size_t oh = (size_t)img * (size_t)half * (size_t)HW + (size_t)j * HW + p;
#pragma unroll
            for (int e = 0; e < V; ++e) g1[e] = g2[e] = 0.f;
            if (gx && gy) cpl_load<V>(g1, gy + oh);
            if (gz) cpl_load<V>(g2, gz + oh);
        } else if constexpr (MERGE) {
#pragma unroll
            for (int e = 0; e < V; ++e) g1[e] = g2[e] = 0.f;
            if (gx && gy) cpl_load<V>(g1, gy + o1);
            if (gy) cpl_load<V>(g2, gy + o2);
        } else {
            if (gx) cpl_load<V>(g1, gy + o1);
            cpl_load<V>(g2, gy + o2);
        }
        if constexpr (REBUILD)
            if (xo) cpl_load<V>(v1, v + o1);
        cpl_load<V>(v2, v + o2);
        cpl_load<V>(u, raw + ou);
        if (REBUILD || SPLIT || (MERGE && (GAUSS || gld)) || sums) cpl_load<V>(t, raw + ot);
        const float gl = gld ? gld[img] : (MODE == FINC_GRAD_REV || (MERGE && !GAUSS) ? -0.f : 0.f);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float ghu, ght;                                        // the gradients of h[2j] and h[2j+1]
            if constexpr (GAUSS && MERGE) {
                const float logs = fmaf(at, t[e], bt), d = v2[e] - fmaf(au, u[e], bu), gE = g2[e] * expf(logs);
                gx2[e] = gld ? fmaf(-gl, d * expf(-logs), gE) : gE;
                ghu = g2[e];
                ght = fmaf(g2[e], d, -gl);
            } else if constexpr (GAUSS) {
                const float m = fmaf(au, u[e], bu), E = expf(-fmaf(at, t[e], bt)), z = (v2[e] - m) * E, G = g2[e] - gl * z;
                gx2[e] = G * E;
                ghu = -gx2[e];
                ght = -fmaf(G, z, gl);
            } else {
                const float th = tanhf(0.5f * fmaf(au, u[e], bu));     // s = 2 th, d s / d h = 1 - s*s/4 = 1 - th*th
                if constexpr (MODE == FINC_GRAD_FWD) {
                    gx2[e] = g2[e] * expf(2.f * th);
                    ghu = fmaf(gx2[e], v2[e], gl) * fmaf(-th, th, 1.f);
                    ght = g2[e];
                } else if constexpr (MODE == FINC_GRAD_REV) {
                    gx2[e] = g2[e] * expf(-2.f * th);
                    ghu = (-(g2[e] * v2[e]) + gl) * fmaf(-th, th, 1.f);
                    ght = -gx2[e];
                } else if constexpr (MERGE) {
                    const float gE = g2[e] * expf(-2.f * th);
                    gx2[e] = gld ? fmaf(-gl, fmaf(v2[e], expf(2.f * th), fmaf(at, t[e], bt)), gE) : gE;
                    ghu = (-(g2[e] * v2[e]) + gl) * fmaf(-th, th, 1.f);
                    ght = -gE;
                } else if constexpr (SPLIT) {
                    const float E = expf(2.f * th), G = g2[e] - gl * fmaf(v2[e], E, fmaf(at, t[e], bt));
                    gx2[e] = G * E;
                    ghu = fmaf(gx2[e], v2[e], gl) * fmaf(-th, th, 1.f);
                    ght = G;
                } else {
                    const float s = 2.f * th, d = v2[e] - fmaf(at, t[e], bt);
                    x2[e] = d * expf(-s);
                    gx2[e] = g2[e] * expf(s);
                    ghu = fmaf(g2[e], d, gl) * fmaf(-th, th, 1.f);
                    ght = g2[e];
                }
            }
            gu[e] = au * ghu;
            gt[e] = at * ght;
            if (sums) {
                acc[0] = fmaf(ghu, u[e], acc[0]);
                acc[1] += ghu;
                acc[2] = fmaf(ght, t[e], acc[2]);
                acc[3] += ght;
            }
        }
        if constexpr (REBUILD) {
            if (xo) {
                cpl_store<V>(xo + o1, v1);
                cpl_store<V>(xo + o2, x2);
            }
        }
        if constexpr (MERGE) {
            const size_t oh = (size_t)img * (size_t)half * (size_t)HW + (size_t)j * HW + p;
            if (gx) cpl_store<V>(gx + oh, g1);
            if (xo) cpl_store<V>(xo + oh, gx2);
        } else if (gx) {
            cpl_store<V>(gx + o1, g1);
            cpl_store<V>(gx + o2, gx2);
        }
        if (graw) {
            cpl_store<V>(graw + ou, gu);
            cpl_store<V>(graw + ot, gt);
        }
    }
    if (sums) {
        __shared__ float sm[4][4];
        cpl_block_sum<4>(acc, sm);
        if (threadIdx.x < 4) part[((size_t)(4 * j) + threadIdx.x) * Q + qi] = acc[threadIdx.x];
    }
}

// The three modes under the names and parameter lists they have always had (the __restrict__ of a kernel's own parameters holds
// inside the body: without the rebuild nothing may overlap).
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_coupling_bwd_kernel(const float *__restrict__ gy, const float *__restrict__ gld,
                                                                        const float *__restrict__ x, const float *__restrict__ raw,
                                                                        const float *__restrict__ a, const float *__restrict__ b,
                                                                        float *__restrict__ gx, float *__restrict__ graw,
                                                                        float *__restrict__ part, int half, int HW, int nv, int items, int Q,
                                                                        int sums)
{
    cpl_grad<V, FINC_GRAD_FWD>(gy, nullptr, gld, x, raw, a, b, nullptr, gx, graw, part, half, HW, nv, items, Q, sums);
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_coupling_rev_bwd_kernel(const float *__restrict__ gy, const float *__restrict__ gld,
                                                                            const float *__restrict__ y, const float *__restrict__ raw,
                                                                            const float *__restrict__ a, const float *__restrict__ b,
                                                                            float *__restrict__ gx, float *__restrict__ graw,
                                                                            float *__restrict__ part, int half, int HW, int nv, int items,
                                                                            int Q, int sums)
{
    cpl_grad<V, FINC_GRAD_REV>(gy, nullptr, gld, y, raw, a, b, nullptr, gx, graw, part, half, HW, nv, items, Q, sums);
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_coupling_recon_kernel(const float *gy, const float *__restrict__ gld, const float *y,
                                                                          const float *__restrict__ raw, const float *__restrict__ a,
                                                                          const float *__restrict__ b, float *xo, float *gx,
                                                                          float *__restrict__ graw, float *__restrict__ part, int half, int HW,
                                                                          int nv, int items, int Q, int sums)
{
    cpl_grad<V, FINC_GRAD_REBUILD>(gy, nullptr, gld, y, raw, a, b, xo, gx, graw, part, half, HW, nv, items, Q, sums);
}

// The split prior's backward (fp32 raw): the fourth mode under a name of its own; nothing may overlap.
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_splitprior_bwd_kernel(const float *__restrict__ gx1, const float *__restrict__ gz2,
                                                                          const float *__restrict__ glp, const float *__restrict__ x,
                                                                          const float *__restrict__ raw, const float *__restrict__ a,
                                                                          const float *__restrict__ b, float *__restrict__ gx,
                                                                          float *__restrict__ graw, float *__restrict__ part, int half, int HW,
                                                                          int nv, int items, int Q, int sums)
{
    cpl_grad<V, FINC_GRAD_SPLIT>(gx1, gz2, glp, x, raw, a, b, nullptr, gx, graw, part, half, HW, nv, items, Q, sums);
}

// The Gaussianized split's backward: the same mode under CPL_LAW_GAUSS; nothing may overlap.
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_gauss_split_bwd_kernel(const float *__restrict__ gx1, const float *__restrict__ gz2,
                                                                           const float *__restrict__ glp, const float *__restrict__ x,
                                                                           const float *__restrict__ raw, const float *__restrict__ a,
                                                                           const float *__restrict__ b, float *__restrict__ gx,
                                                                           float *__restrict__ graw, float *__restrict__ part, int half, int HW,
                                                                           int nv, int items, int Q, int sums)
{
    cpl_grad<V, FINC_GRAD_SPLIT, float, CPL_LAW_GAUSS>(gx1, gz2, glp, x, raw, a, b, nullptr, gx, graw, part, half, HW, nv, items, Q, sums);
}

// The merges' backward, from the merge's OUTPUT x: the fifth mode under names of its own -- the split prior's on an fp32 and on a
// bf16 raw, the Gaussianized split's (fp32 raw).  gx1 and gz2 are the half tensors it writes; nothing may overlap.
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_splitprior_merge_bwd_kernel(const float *__restrict__ gx, const float *__restrict__ glp,
                                                                                const float *__restrict__ x, const float *__restrict__ raw,
                                                                                const float *__restrict__ a, const float *__restrict__ b,
                                                                                float *__restrict__ gx1, float *__restrict__ gz2,
                                                                                float *__restrict__ graw, float *__restrict__ part, int half,
                                                                                int HW, int nv, int items, int Q, int sums)
{
    cpl_grad<V, FINC_GRAD_MERGE>(gx, nullptr, glp, x, raw, a, b, gz2, gx1, graw, part, half, HW, nv, items, Q, sums);
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_splitprior_merge_rawbf16_bwd_kernel(const float *__restrict__ gx, const float *__restrict__ glp,
                                                                                        const float *__restrict__ x, const __bf16 *__restrict__ raw,
                                                                                        const float *__restrict__ a, const float *__restrict__ b,
                                                                                        float *__restrict__ gx1, float *__restrict__ gz2,
                                                                                        __bf16 *__restrict__ graw, float *__restrict__ part,
                                                                                        int half, int HW, int nv, int items, int Q, int sums)
{
    cpl_grad<V, FINC_GRAD_MERGE, __bf16>(gx, nullptr, glp, x, raw, a, b, gz2, gx1, graw, part, half, HW, nv, items, Q, sums);
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_gauss_merge_bwd_kernel(const float *__restrict__ gx, const float *__restrict__ glp,
                                                                           const float *__restrict__ x, const float *__restrict__ raw,
                                                                           const float *__restrict__ a, const float *__restrict__ b,
                                                                           float *__restrict__ gx1, float *__restrict__ gz2,
                                                                           float *__restrict__ graw, float *__restrict__ part, int half, int HW,
                                                                           int nv, int items, int Q, int sums)
{
    cpl_grad<V, FINC_GRAD_MERGE, float, CPL_LAW_GAUSS>(gx, nullptr, glp, x, raw, a, b, gz2, gx1, graw, part, half, HW, nv, items, Q, sums);
}

// The four modes on a bf16 raw (and a bf16 grad_raw): one kernel, the mode its parameter.  xo == v and gx == gy are the rebuild's;
// gz is the split's.
template <int V, int MODE>
__global__ __launch_bounds__(CPL_THREADS) void finc_coupling_rawbf16_grad_kernel(const float *gy, const float *gz,
                                                                                 const float *__restrict__ gld, const float *v,
                                                                                 const __bf16 *__restrict__ raw,
                                                                                 const float *__restrict__ a, const float *__restrict__ b,
                                                                                 float *xo, float *gx, __bf16 *__restrict__ graw,
                                                                                 float *__restrict__ part, int half, int HW, int nv,
                                                                                 int items, int Q, int sums)
{
    cpl_grad<V, MODE, __bf16>(gy, gz, gld, v, raw, a, b, xo, gx, graw, part, half, HW, nv, items, Q, sums);
}

// One wave per output: out = sum of its n consecutive partials, lane l takes l, l + 64, ... and the lanes meet in a butterfly.
// pairs == 0: out_a[o] (the log-det of image o).  pairs == 1: output o = 4j + k goes to out_a / out_b as listed above; a nullptr
// destination is neither summed nor written.
__global__ __launch_bounds__(64) void finc_coupling_reduce_kernel(const float *__restrict__ part, int n, float *__restrict__ out_a,
                                                                  float *__restrict__ out_b, int pairs)
{
    const int o = (int)blockIdx.x;
    float *dst = out_a + o;
    if (pairs) {
        float *base = (o & 1) ? out_b : out_a;
        if (!base) return;
        dst = base + (2 * (o >> 2) + ((o >> 1) & 1));
    }
    const float *p = part + (size_t)o * n;
    float s = 0.f;
    for (int i = (int)threadIdx.x; i < n; i += 64) s += p[i];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
    if (threadIdx.x == 0) *dst = s;
}

// Thread item = V consecutive pixels of one (image, channel) row.  relu as torch.relu has it: a NaN stays a NaN.  T: the element
// type of in and out, float or __bf16 (the add and the max in fp32, rounded once).
template <int V, typename T>
__device__ __forceinline__ void cpl_bias_relu(const T *in, const float *__restrict__ bias, T *out, int C, int HW, int nv, unsigned items)
{
    for (unsigned idx = blockIdx.x * CPL_THREADS + threadIdx.x; idx < items; idx += gridDim.x * CPL_THREADS) {
        const unsigned row = idx / (unsigned)nv, p = (idx - row * (unsigned)nv) * V;
        const float bv = bias[row % (unsigned)C];
        const size_t o = (size_t)row * HW + p;
        float v[V];
        cpl_load<V>(v, in + o);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float w = v[e] + bv;
            v[e] = w != w ? w : fmaxf(w, 0.f);
        }
        cpl_store<V>(out + o, v);
    }
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_bias_relu_kernel(const float *in, const float *__restrict__ bias, float *out, int C,
                                                                     int HW, int nv, unsigned items)
{
    cpl_bias_relu<V, float>(in, bias, out, C, HW, nv, items);
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_bias_relu_bf16_kernel(const __bf16 *in, const float *__restrict__ bias, __bf16 *out,
                                                                          int C, int HW, int nv, unsigned items)
{
    cpl_bias_relu<V, __bf16>(in, bias, out, C, HW, nv, items);
}

// workgroups that fill the chip at eight of these per compute unit
constexpr long long CPL_CHIP_WGS = 256 * 8;

inline int cpl_parts(long long items, long long outer)
{
    long long p = (items + CPL_THREADS - 1) / CPL_THREADS;             // one pass of the loop each ...
    const long long cap = (CPL_CHIP_WGS + outer - 1) / outer;          // ... unless the chip is full already
    if (p > cap) p = cap;
    return p < 1 ? 1 : (int)p;
}
// outer * cpl_parts(items, outer) is at most outer * ceil(items / 256) and below CPL_CHIP_WGS + outer: the smaller of these two bounds,
// for the dword form's item count, is what a workspace reserves per sum.  It never shrinks when B or HW grows.
inline long long cpl_partials_bound(long long items, long long outer)
{
    const long long all = outer * ((items + CPL_THREADS - 1) / CPL_THREADS), cap = CPL_CHIP_WGS + outer;
    return all < cap ? all : cap;
}
// The wide form: HW in whole pieces, every fp32 activation pointer (`ptrs`) on 16 bytes and every bf16 one (`half_ptrs`: a bf16 raw
// and grad_raw, whose piece of four pixels is 8 bytes) on 8.
inline bool cpl_wide(int HW, uintptr_t ptrs, uintptr_t half_ptrs = 0) { return HW % 4 == 0 && (ptrs & 15u) == 0 && (half_ptrs & 7u) == 0; }
inline bool cpl_rows_fit(int B, int C, int HW)          // a channel's B * HW / V items index as int with a full grid's stride beyond them
{
    return (size_t)C * HW * 4 < ((size_t)1 << 31) && (long long)B * HW < (1LL << 31) - (CPL_CHIP_WGS + 1) * CPL_THREADS;
}
template <typename... P>
inline uintptr_t cpl_bits(const P *...p) { return (... | (uintptr_t)p); }     // every pointer's address bits (nullptr adds none)
// A backward launch: `outer` channel units (pairs, channels) share B * HW / V items each in Q parts, a workgroup per (unit, part).
// `ptrs`: cpl_bits of every fp32 activation pointer the launch touches, `half_ptrs`: of every bf16 one.  Q = 0: the rows do not fit
// (cpl_rows_fit).
struct CplGradPlan {
    bool wide;
    int nv, items, Q;
    dim3 grid;
};
inline CplGradPlan cpl_grad_plan(int B, int C, int HW, int outer, uintptr_t ptrs, uintptr_t half_ptrs = 0)
{
    if (!cpl_rows_fit(B, C, HW)) return CplGradPlan{false, 0, 0, 0, dim3(0)};
    const bool wide = cpl_wide(HW, ptrs, half_ptrs);
    const int nv = HW / (wide ? 4 : 1), items = B * nv, Q = cpl_parts(items, outer);
    return CplGradPlan{wide, nv, items, Q, dim3((unsigned)((long long)outer * Q))};
}
// the tail of a backward with per-channel sums: output o of `outputs`, n partials each, to out_a / out_b (finc_coupling_reduce_kernel)
inline int cpl_reduce_pairs(int sums, const float *ws, int outputs, int n, float *out_a, float *out_b, hipStream_t st)
{
    if (sums) {
        hipLaunchKernelGGL(finc_coupling_reduce_kernel, dim3((unsigned)outputs), dim3(64), 0, st, ws, n, out_a, out_b, 1);
        FINC_CHECK_LAUNCH();
    }
    return FINC_OK;
}
inline unsigned cpl_row_grid(long long items)           // grid-stride over rows, up to four chips' worth; 0: they do not index as unsigned
{
    const long long wgs = (items + CPL_THREADS - 1) / CPL_THREADS, most = 4 * CPL_CHIP_WGS;
    return items >= (1LL << 32) - most * CPL_THREADS ? 0u : (unsigned)(wgs > most ? most : wgs);
}
// A grid-stride launch over `rows` rows of HW elements: pieces of V elements (16 bytes) when HW is whole pieces and every pointer of
// `ptrs` is on 16 bytes, single elements otherwise.  wgs = 0: cpl_row_grid's refusal.  What the launchers of ActNorm's transform,
// bias + ReLU and the grouped lead product run, and what finc_pixel_plan_info reports.
struct CplRowPlan {
    bool wide;
    int nv;
    long long items;
    unsigned wgs;
};
inline CplRowPlan cpl_row_plan(long long rows, int HW, int V, uintptr_t ptrs)
{
    const bool wide = HW % V == 0 && (ptrs & 15u) == 0;
    const int nv = HW / (wide ? V : 1);
    const long long items = rows * nv;
    return CplRowPlan{wide, nv, items, cpl_row_grid(items)};
}
// A transform launch: B images share half * HW / V items each in P parts, a workgroup per (image, part).  P = 0: the dimensions do
// not fit (FINC_ERR_BAD_DIMS).  `ptrs` / `half_ptrs` as cpl_wide reads them.
struct CplTransformPlan {
    bool wide;
    int nv, items, P;
};
inline CplTransformPlan cpl_transform_plan(int B, int C, int HW, uintptr_t ptrs, uintptr_t half_ptrs = 0)
{
    if ((size_t)C * HW * 4 >= ((size_t)1 << 31)) return CplTransformPlan{false, 0, 0, 0};
    const bool wide = cpl_wide(HW, ptrs, half_ptrs);
    const int nv = HW / (wide ? 4 : 1), items = (C / 2) * nv, P = cpl_parts(items, B);
    if ((long long)B * P >= (1LL << 31)) return CplTransformPlan{false, 0, 0, 0};
    return CplTransformPlan{wide, nv, items, P};
}

// The kernel of a transform / a backward for a raw element type: the fp32 ones under the names they have always had.
template <typename R, int V, int DIR, bool LOGDET>
constexpr auto cpl_transform_kernel()
{
    if constexpr (sizeof(R) == 2) return finc_coupling_rawbf16_kernel<V, DIR, LOGDET>;
    else if constexpr (DIR < 0 && LOGDET) return finc_coupling_rev_logdet_kernel<V>;
    else return finc_coupling_kernel<V, DIR, LOGDET>;
}
// the address bits of raw-typed pointers that count towards the 16-byte rule (fp32) or the 8-byte rule (bf16)
template <typename R, typename... P>
inline uintptr_t cpl_bits16(const P *...p) { return sizeof(R) == 4 ? cpl_bits(p...) : 0; }
template <typename R, typename... P>
inline uintptr_t cpl_bits8(const P *...p) { return sizeof(R) == 2 ? cpl_bits(p...) : 0; }

// logdet (either direction): the log-det of the FORWARD map, sum s per image -- in the reverse direction at the recovered input y
// (B x P partials in `ws`, then the reduce); nullptr: none, and `ws` is not touched.
// split: the split prior's transforms (cpl_transform's SPLIT) -- xb / yb are the second half tensor of the side that has two, every
// half-tensor pointer counts towards the 16-byte rule, and logdet is log p (direction +1 always has it).  LAW = CPL_LAW_GAUSS (with
// `split` and an fp32 raw): the same geometry in front of finc_gauss_split_kernel.
template <typename R, int LAW = CPL_LAW_COUPLING>
int cpl_launch(const float *x, const float *xb, const R *raw, const float *a, const float *b, float *y, float *yb, float *logdet, int B,
               int C, int HW, int direction, bool split, float *ws, hipStream_t st)
{
    const int half = C / 2;
    const CplTransformPlan tp = cpl_transform_plan(B, C, HW, cpl_bits(x, xb, y, yb) | cpl_bits16<R>(raw), cpl_bits8<R>(raw));
    if (!tp.P) return FINC_ERR_BAD_DIMS;
    const bool wide = tp.wide;
    const int nv = tp.nv, items = tp.items, P = tp.P;
    const dim3 grid((unsigned)((long long)B * P)), block(CPL_THREADS);
    if (split) {
        const float c = (float)(0.5 * (double)half * (double)HW * 1.8378770664093454835606594728112);        // log(2 pi)
        if constexpr (LAW == CPL_LAW_GAUSS) {
            const auto kernel = direction > 0 ? (wide ? finc_gauss_split_kernel<4, 1, true> : finc_gauss_split_kernel<1, 1, true>)
                                : logdet      ? (wide ? finc_gauss_split_kernel<4, -1, true> : finc_gauss_split_kernel<1, -1, true>)
                                              : (wide ? finc_gauss_split_kernel<4, -1, false> : finc_gauss_split_kernel<1, -1, false>);
            hipLaunchKernelGGL(kernel, grid, block, 0, st, x, xb, raw, a, b, y, yb, ws, c, half, HW, nv, items, P);
        } else {
            const auto kernel = direction > 0 ? (wide ? finc_splitprior_kernel<4, 1, true, R> : finc_splitprior_kernel<1, 1, true, R>)
                                : logdet      ? (wide ? finc_splitprior_kernel<4, -1, true, R> : finc_splitprior_kernel<1, -1, true, R>)
                                              : (wide ? finc_splitprior_kernel<4, -1, false, R> : finc_splitprior_kernel<1, -1, false, R>);
            hipLaunchKernelGGL(kernel, grid, block, 0, st, x, xb, raw, a, b, y, yb, ws, c, half, HW, nv, items, P);
        }
    } else {
        const auto kernel = !logdet ? (direction < 0 ? (wide ? cpl_transform_kernel<R, 4, -1, false>() : cpl_transform_kernel<R, 1, -1, false>())
                                                     : (wide ? cpl_transform_kernel<R, 4, 1, false>() : cpl_transform_kernel<R, 1, 1, false>()))
                            : direction < 0 ? (wide ? cpl_transform_kernel<R, 4, -1, true>() : cpl_transform_kernel<R, 1, -1, true>())
                                            : (wide ? cpl_transform_kernel<R, 4, 1, true>() : cpl_transform_kernel<R, 1, 1, true>());
        hipLaunchKernelGGL(kernel, grid, block, 0, st, x, raw, a, b, y, ws, half, HW, nv, items, P);
    }
    FINC_CHECK_LAUNCH();
    if (logdet) {
        hipLaunchKernelGGL(finc_coupling_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float *)ws, P, logdet, (float *)nullptr, 0);
        FINC_CHECK_LAUNCH();
    }
    return FINC_OK;
}

template <int V, int MODE>
void cpl_grad_start(const CplGradPlan &p, hipStream_t st, const float *gy, const float *gz, const float *gld, const float *v,
                    const float *raw, const float *a, const float *b, float *xo, float *gx, float *graw, float *ws, int half, int HW, int sums)
{
    if constexpr (MODE == FINC_GRAD_MERGE)
        hipLaunchKernelGGL(finc_splitprior_merge_bwd_kernel<V>, p.grid, dim3(CPL_THREADS), 0, st, gy, gld, v, raw, a, b, gx, xo, graw, ws, half,
                           HW, p.nv, p.items, p.Q, sums);
    else if constexpr (MODE == FINC_GRAD_SPLIT)
        hipLaunchKernelGGL(finc_splitprior_bwd_kernel<V>, p.grid, dim3(CPL_THREADS), 0, st, gy, gz, gld, v, raw, a, b, gx, graw, ws, half, HW,
                           p.nv, p.items, p.Q, sums);
    else if constexpr (MODE == FINC_GRAD_REBUILD)
        hipLaunchKernelGGL(finc_coupling_recon_kernel<V>, p.grid, dim3(CPL_THREADS), 0, st, gy, gld, v, raw, a, b, xo, gx, graw, ws, half, HW,
                           p.nv, p.items, p.Q, sums);
    else
        hipLaunchKernelGGL(MODE == FINC_GRAD_REV ? finc_coupling_rev_bwd_kernel<V> : finc_coupling_bwd_kernel<V>, p.grid, dim3(CPL_THREADS), 0,
                           st, gy, gld, v, raw, a, b, gx, graw, ws, half, HW, p.nv, p.items, p.Q, sums);
}
template <int V, int MODE>
void cpl_grad_start(const CplGradPlan &p, hipStream_t st, const float *gy, const float *gz, const float *gld, const float *v,
                    const __bf16 *raw, const float *a, const float *b, float *xo, float *gx, __bf16 *graw, float *ws, int half, int HW, int sums)
{
    if constexpr (MODE == FINC_GRAD_MERGE)
        hipLaunchKernelGGL(finc_splitprior_merge_rawbf16_bwd_kernel<V>, p.grid, dim3(CPL_THREADS), 0, st, gy, gld, v, raw, a, b, gx, xo, graw, ws,
                           half, HW, p.nv, p.items, p.Q, sums);
    else
        hipLaunchKernelGGL((finc_coupling_rawbf16_grad_kernel<V, MODE>), p.grid, dim3(CPL_THREADS), 0, st, gy, gz, gld, v, raw, a, b, xo, gx,
                           graw, ws, half, HW, p.nv, p.items, p.Q, sums);
}

template <typename R, int LAW = CPL_LAW_COUPLING>
int cpl_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *gld, const float *v, const R *raw, const float *a,
                    const float *b, float *xo, float *gx, R *graw, float *ga, float *gb, int B, int C, int HW, float *ws, hipStream_t st)
{
    const int half = C / 2, sums = (ga || gb) ? 1 : 0;
    const CplGradPlan p = cpl_grad_plan(B, C, HW, half, cpl_bits(gy, gz, v, xo, gx) | cpl_bits16<R>(raw, graw), cpl_bits8<R>(raw, graw));
    if (!p.Q) return FINC_ERR_BAD_DIMS;
#define CPL_GRAD_START(V, MODE) cpl_grad_start<V, MODE>(p, st, gy, gz, gld, v, raw, a, b, xo, gx, graw, ws, half, HW, sums)
    if constexpr (LAW == CPL_LAW_GAUSS) {                                  // (FINC_GRAD_SPLIT or FINC_GRAD_MERGE, fp32 raw)
        if (mode == FINC_GRAD_MERGE) {
            const auto kernel = p.wide ? finc_gauss_merge_bwd_kernel<4> : finc_gauss_merge_bwd_kernel<1>;
            hipLaunchKernelGGL(kernel, p.grid, dim3(CPL_THREADS), 0, st, gy, gld, v, raw, a, b, gx, xo, graw, ws, half, HW, p.nv, p.items, p.Q,
                               sums);
        } else {
            const auto kernel = p.wide ? finc_gauss_split_bwd_kernel<4> : finc_gauss_split_bwd_kernel<1>;
            hipLaunchKernelGGL(kernel, p.grid, dim3(CPL_THREADS), 0, st, gy, gz, gld, v, raw, a, b, gx, graw, ws, half, HW, p.nv, p.items, p.Q,
                               sums);
        }
    } else if (mode == FINC_GRAD_MERGE) {
        if (p.wide) CPL_GRAD_START(4, FINC_GRAD_MERGE); else CPL_GRAD_START(1, FINC_GRAD_MERGE);
    } else if (mode == FINC_GRAD_SPLIT) {
        if (p.wide) CPL_GRAD_START(4, FINC_GRAD_SPLIT); else CPL_GRAD_START(1, FINC_GRAD_SPLIT);
    } else if (mode == FINC_GRAD_REBUILD) {
        if (p.wide) CPL_GRAD_START(4, FINC_GRAD_REBUILD); else CPL_GRAD_START(1, FINC_GRAD_REBUILD);
    } else if (mode == FINC_GRAD_REV) {
        if (p.wide) CPL_GRAD_START(4, FINC_GRAD_REV); else CPL_GRAD_START(1, FINC_GRAD_REV);
    } else {
        if (p.wide) CPL_GRAD_START(4, FINC_GRAD_FWD); else CPL_GRAD_START(1, FINC_GRAD_FWD);
    }
#undef CPL_GRAD_START
    FINC_CHECK_LAUNCH();
    return cpl_reduce_pairs(sums, ws, 4 * half, p.Q, ga, gb, st);
}

} // namespace

// floats: forward log-det partials (B images x P parts) and backward partials (4 sums x C/2 pairs x Q parts)
size_t finc_coupling_workspace_floats(int B, int C, int HW)
{
    const long long half = C / 2, fwd = cpl_partials_bound(half * HW, B), bwd = 4 * cpl_partials_bound((long long)B * HW, half);
    return (size_t)(fwd > bwd ? fwd : bwd);
}

int finc_coupling_launch(const float *x, const float *xb, const float *raw, const float *a, const float *b, float *y, float *yb,
                         float *logdet, int B, int C, int HW, int direction, bool split, float *ws, hipStream_t st)
{
    return cpl_launch<float>(x, xb, raw, a, b, y, yb, logdet, B, C, HW, direction, split, ws, st);
}
int finc_coupling_rawbf16_launch(const float *x, const float *xb, const uint16_t *raw, const float *a, const float *b, float *y, float *yb,
                                 float *logdet, int B, int C, int HW, int direction, bool split, float *ws, hipStream_t st)
{
    return cpl_launch<__bf16>(x, xb, reinterpret_cast<const __bf16 *>(raw), a, b, y, yb, logdet, B, C, HW, direction, split, ws, st);
}

int finc_gauss_split_launch(const float *x, const float *xb, const float *raw, const float *a, const float *b, float *y, float *yb,
                            float *log_p, int B, int C, int HW, int direction, float *ws, hipStream_t st)
{
    return cpl_launch<float, CPL_LAW_GAUSS>(x, xb, raw, a, b, y, yb, log_p, B, C, HW, direction, true, ws, st);
}

int finc_coupling_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *gld, const float *v, const float *raw,
                              const float *a, const float *b, float *xo, float *gx, float *graw, float *ga, float *gb, int B, int C, int HW,
                              float *ws, hipStream_t st)
{
    return cpl_grad_launch<float>(mode, gy, gz, gld, v, raw, a, b, xo, gx, graw, ga, gb, B, C, HW, ws, st);
}
int finc_gauss_split_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *glp, const float *v, const float *raw,
                                 const float *a, const float *b, float *xo, float *gx, float *graw, float *ga, float *gb, int B, int C,
                                 int HW, float *ws, hipStream_t st)
{
    return cpl_grad_launch<float, CPL_LAW_GAUSS>(mode, gy, gz, glp, v, raw, a, b, xo, gx, graw, ga, gb, B, C, HW, ws, st);
}
int finc_coupling_rawbf16_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *gld, const float *v,
                                      const uint16_t *raw, const float *a, const float *b, float *xo, float *gx, uint16_t *graw, float *ga,
                                      float *gb, int B, int C, int HW, float *ws, hipStream_t st)
{
    return cpl_grad_launch<__bf16>(mode, gy, gz, gld, v, reinterpret_cast<const __bf16 *>(raw), a, b, xo, gx,
                                   reinterpret_cast<__bf16 *>(graw), ga, gb, B, C, HW, ws, st);
}

// fp32: 16-byte pieces of 4; bf16: 16-byte pieces of 8
template <typename T>
static int cpl_bias_relu_launch(const T *in, const float *bias, T *out, int B, int C, int HW, hipStream_t st)
{
    constexpr int V = 16 / (int)sizeof(T);
    const CplRowPlan rp = cpl_row_plan((long long)B * C, HW, V, (uintptr_t)in | (uintptr_t)out);
    if (!rp.wgs) return FINC_ERR_BAD_DIMS;
    const bool wide = rp.wide;
    const int nv = rp.nv;
    const long long items = rp.items;
    const unsigned wgs = rp.wgs;
    if constexpr (sizeof(T) == 2)
        hipLaunchKernelGGL(wide ? finc_bias_relu_bf16_kernel<8> : finc_bias_relu_bf16_kernel<1>, dim3(wgs), dim3(CPL_THREADS), 0, st, in, bias,
                           out, C, HW, nv, (unsigned)items);
    else
        hipLaunchKernelGGL(wide ? finc_bias_relu_kernel<4> : finc_bias_relu_kernel<1>, dim3(wgs), dim3(CPL_THREADS), 0, st, in, bias, out, C, HW,
                           nv, (unsigned)items);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}
int finc_bias_relu_launch(const float *in, const float *bias, float *out, int B, int C, int HW, hipStream_t st)
{
    return cpl_bias_relu_launch<float>(in, bias, out, B, C, HW, st);
}
int finc_bias_relu_bf16_launch(const uint16_t *in, const float *bias, uint16_t *out, int B, int C, int HW, hipStream_t st)
{
    return cpl_bias_relu_launch<__bf16>(reinterpret_cast<const __bf16 *>(in), bias, reinterpret_cast<__bf16 *>(out), B, C, HW, st);
}

#endif /* FINC_COUPLING_H */
