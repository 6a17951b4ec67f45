// The image boundary for gfx950 (included by finc_mix.hip behind finc_coupling.h: same object file, the per-pixel streaming neighbours
// of the unit).
//
// Reference: every model starts with Dequantization, Normalization(0, 256), Normalization(-alpha, 1 / (1 - 2 alpha)), LogitTransform
// and a Squeeze (layers/dequantize.py, layers/normalize.py, layers/transforms.py:6-19, layers/squeeze.py:5-41) and its reverse chain
// ends with them.  Here each direction is one launch:
//   * finc_image_encode_kernel  x (uint8 or fp32 pixels) + u (fp32 noise, optional) -> logit(m (x + u) + c), squeezed or not, and the
//                               per-image log-det of the whole prefix;
//   * finc_image_decode_kernel  z -> floor(sigmoid(z) / m' + off), un-squeezed or not, as fp32 (no clamp: Dequantization.reverse) or
//                               as uint8 (clamped to [0, hi - 1]), optionally with the FORWARD map's log-det at the recovered value.
// The encode never forms 1 - y from a rounded y: with the integer pixel and the noise in hand, 1 - y = m ((hi - x) - u) + c2 with
// c2 = 1 - c - m hi composed on the host in float64.  hi - x is exact, (hi - x) - u is a difference of two numbers of like sign and is
// rounded once, and neither term of the fma cancels against the other: at x = 255, u = 1 - 2^-24 the PyTorch lines' log(1 - y) is
// 7e-2 off, this is at the rounding of the formats.
// Layout: image [B][C][H][W], noise alike (fp32); with squeeze the other side is [B][4C][H/2][W/2] in the reference's channel order,
// out[b][4c + 2dy + dx][h][w] = f(in[b][c][2h + dy][2w + dx]).  Forms (ImgForm):
//   IMG_SQ4    thread item = one input channel, one output row, FOUR output columns: two input rows of 8 pixels (2 x 2 16-byte loads
//              of an fp32 image and of the noise, 2 8-byte loads of a uint8 image), four 16-byte stores (one per output channel).  W %
//              8 == 0, the fp32 pointers on 16 bytes, a uint8 image on 8.
//   IMG_SQ1    thread item = one input channel, one output position: 2 x 2 pixels, four dwords out.  Everything else with squeeze.
//   IMG_FLAT4  no squeeze: 4 consecutive pixels (HW % 4 == 0, fp32 pointers on 16 bytes, a uint8 one on 4);  IMG_FLAT1: one pixel.
// Workgroup = (image, part) as in cpl_transform: P = cpl_parts(items, B) parts share an image's items, the workgroup's log-det partial
// goes to part[blockIdx.x] (part 0 adds the host's per-image constant) and finc_coupling_reduce_kernel adds an image's P partials in
// a fixed order: the same inputs give the same bits.  Every index is below the element count: nothing is read or written beyond a
// tensor.  out == img is allowed in the FLAT forms on fp32 (a thread reads its pieces before it writes them).
#ifndef FINC_IMAGE_H
#define FINC_IMAGE_H

namespace {

enum ImgForm { IMG_FLAT1 = 0, IMG_FLAT4 = 1, IMG_SQ1 = 2, IMG_SQ4 = 3 };

// N consecutive pixels as floats: fp32 in dwords (N = 1, 2: a 2 x 2 patch's row has no 8-byte promise) or 16-byte pieces (N = 4, 8);
// uint8 in bytes (N = 1, 2), one dword (N = 4) or one 8-byte piece (N = 8).  A uint8 -> float conversion is exact.
template <int N>
__device__ inline void img_load(float (&d)[N], const float *p)
{
    if constexpr (N >= 4) {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            const cpl_v4f v = *reinterpret_cast<const cpl_v4f *>(p + k);
            d[k] = v.x; d[k + 1] = v.y; d[k + 2] = v.z; d[k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] = p[k];
    }
}
template <int N>
__device__ inline void img_load(float (&d)[N], const uint8_t *p)
{
    if constexpr (N == 8) {
        const uint2 w = *reinterpret_cast<const uint2 *>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = (float)((w.x >> (8 * k)) & 0xffu);
            d[k + 4] = (float)((w.y >> (8 * k)) & 0xffu);
        }
    } else if constexpr (N == 4) {
        const unsigned w = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = (float)((w >> (8 * k)) & 0xffu);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) d[k] = (float)p[k];
    }
}
template <int N>
__device__ inline void img_store(float *p, const float (&d)[N])
{
    if constexpr (N >= 4) {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            cpl_v4f v;
            v.x = d[k]; v.y = d[k + 1]; v.z = d[k + 2]; v.w = d[k + 3];
            *reinterpret_cast<cpl_v4f *>(p + k) = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = d[k];
    }
}
// (the values are whole numbers in [0, 255] here: the clamp is the caller's)
template <int N>
__device__ inline void img_store(uint8_t *p, const float (&d)[N])
{
    if constexpr (N == 8) {
        uint2 w = make_uint2(0u, 0u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w.x |= (unsigned)d[k] << (8 * k);
            w.y |= (unsigned)d[k + 4] << (8 * k);
        }
        *reinterpret_cast<uint2 *>(p) = w;
    } else if constexpr (N == 4) {
        unsigned w = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) w |= (unsigned)d[k] << (8 * k);
        *reinterpret_cast<unsigned *>(p) = w;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = (uint8_t)d[k];
    }
}

struct ImgEncode {
    float m, c, hi, c2;
    // the logit of y = m (x + u) + c and its log-det term -(log y + log(1 - y)), 1 - y from hi - x (see the head of this file)
    __device__ inline float operator()(float x, float u, float &ld) const
    {
        const float yl = fmaf(m, x + u, c), yr = fmaf(m, (hi - x) - u, c2);
        const float a = logf(yl), b = logf(yr);
        ld += -(a + b);
        return a - b;
    }
};

template <typename T, bool LOGDET>
struct ImgDecode {
    float inv_m, off, top;
    // floor(sigmoid(z) * inv_m + off); uint8: clamped to [0, top].  Log-det of the forward map at the recovered y = sigmoid(z):
    // -log y - log(1 - y) = |z| + 2 log(1 + exp(-|z|)).
    __device__ inline float operator()(float z, float &ld) const
    {
        const float az = fabsf(z), e = expf(-az), s = (z >= 0.f ? 1.f : e) / (1.f + e);
        if constexpr (LOGDET) ld += fmaf(2.f, log1pf(e), az);
        const float v = floorf(fmaf(s, inv_m, off));
        if constexpr (sizeof(T) == 1) return fminf(fmaxf(v, 0.f), top);
        else return v;
    }
};

// The (channel, row, column piece) of squeeze item idx: image-side offset of its first input row's first pixel and squeezed-side
// offset of output channel 4c's piece (channel 4c + k lies k * plane further on), both within the image.
template <int NW>
__device__ inline void img_sq_offsets(int idx, int H, int W, int &oi, int &os, int &plane)
{
    const int h2 = H / 2, w2 = W / 2, nw = w2 / NW, per = h2 * nw;
    const int ch = idx / per, r = idx - ch * per, h = r / nw, wq = r - h * nw;
    oi = (ch * H + 2 * h) * W + 2 * NW * wq;
    plane = h2 * w2;
    os = 4 * ch * plane + h * w2 + NW * wq;
}

template <typename T, int FORM>
__global__ __launch_bounds__(CPL_THREADS) void finc_image_encode_kernel(const T *img, const float *__restrict__ noise, float *out,
                                                                        float *__restrict__ part, ImgEncode f, float ldc, int C, int H,
                                                                        int W, int items, int P)
{
    const int b = (int)blockIdx.x / P, pi = (int)blockIdx.x - b * P;
    const size_t base = (size_t)b * (size_t)C * (size_t)H * (size_t)W;
    float ld = 0.f;
    for (int idx = pi * CPL_THREADS + (int)threadIdx.x; idx < items; idx += P * CPL_THREADS) {
        if constexpr (FORM == IMG_FLAT1 || FORM == IMG_FLAT4) {
            constexpr int V = FORM == IMG_FLAT4 ? 4 : 1;
            const size_t o = base + (size_t)idx * V;
            float x[V], u[V] = {}, y[V];
            img_load<V>(x, img + o);
            if (noise) img_load<V>(u, noise + o);
#pragma unroll
            for (int e = 0; e < V; ++e) y[e] = f(x[e], u[e], ld);
            img_store<V>(out + o, y);
        } else {
            constexpr int NW = FORM == IMG_SQ4 ? 4 : 1;
            int oi, os, plane;
            img_sq_offsets<NW>(idx, H, W, oi, os, plane);
            float x[2][2 * NW], u[2][2 * NW] = {};
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                img_load<2 * NW>(x[dy], img + base + oi + dy * W);
                if (noise) img_load<2 * NW>(u[dy], noise + base + oi + dy * W);
            }
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    float y[NW];
#pragma unroll
                    for (int k = 0; k < NW; ++k) y[k] = f(x[dy][2 * k + dx], u[dy][2 * k + dx], ld);
                    img_store<NW>(out + base + os + (2 * dy + dx) * plane, y);
                }
            }
        }
    }
    __shared__ float sm[1][4];
    float v[1] = {ld};
    cpl_block_sum<1>(v, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = pi == 0 ? v[0] + ldc : v[0];
}

template <typename T, int FORM, bool LOGDET>
__global__ __launch_bounds__(CPL_THREADS) void finc_image_decode_kernel(const float *z, T *out, float *__restrict__ part,
                                                                        ImgDecode<T, LOGDET> f, float ldc, int C, int H, int W, int items,
                                                                        int P)
{
    const int b = (int)blockIdx.x / P, pi = (int)blockIdx.x - b * P;
    const size_t base = (size_t)b * (size_t)C * (size_t)H * (size_t)W;
    float ld = 0.f;
    for (int idx = pi * CPL_THREADS + (int)threadIdx.x; idx < items; idx += P * CPL_THREADS) {
        if constexpr (FORM == IMG_FLAT1 || FORM == IMG_FLAT4) {
            constexpr int V = FORM == IMG_FLAT4 ? 4 : 1;
            const size_t o = base + (size_t)idx * V;
            float v[V], x[V];
            img_load<V>(v, z + o);
#pragma unroll
            for (int e = 0; e < V; ++e) x[e] = f(v[e], ld);
            img_store<V>(out + o, x);
        } else {
            constexpr int NW = FORM == IMG_SQ4 ? 4 : 1;
            int oi, os, plane;
            img_sq_offsets<NW>(idx, H, W, oi, os, plane);
            float x[2][2 * NW];
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    float v[NW];
                    img_load<NW>(v, z + base + os + (2 * dy + dx) * plane);
#pragma unroll
                    for (int k = 0; k < NW; ++k) x[dy][2 * k + dx] = f(v[k], ld);
                }
            }
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) img_store<2 * NW>(out + base + oi + dy * W, x[dy]);
        }
    }
    if constexpr (LOGDET) {
        __shared__ float sm[1][4];
        float v[1] = {ld};
        cpl_block_sum<1>(v, sm);
        if (threadIdx.x == 0) part[blockIdx.x] = pi == 0 ? v[0] + ldc : v[0];
    }
}

// The form and the thread items per image.  `f32_ptrs`: cpl_bits of every fp32 tensor the launch touches; `u8_ptr`: the uint8 one's
// address (0: none), held to 8 bytes by IMG_SQ4 (a row piece of 8 pixels) and to 4 by IMG_FLAT4.
struct ImgPlan {
    int form, items;
};
inline ImgPlan img_plan(int C, int H, int W, int squeeze, uintptr_t f32_ptrs, uintptr_t u8_ptr)
{
    if (squeeze) {
        if (W % 8 == 0 && (f32_ptrs & 15u) == 0 && (u8_ptr & 7u) == 0) return ImgPlan{IMG_SQ4, C * (H / 2) * (W / 8)};
        return ImgPlan{IMG_SQ1, C * (H / 2) * (W / 2)};
    }
    if (cpl_wide(H * W, f32_ptrs) && (u8_ptr & 3u) == 0) return ImgPlan{IMG_FLAT4, C * H * W / 4};
    return ImgPlan{IMG_FLAT1, C * H * W};
}

// index widths as in cpl_launch: an image's offsets are ints, and so is the grid
inline bool img_fits(int B, int C, int H, int W) { return (size_t)C * (size_t)H * (size_t)W * 4 < ((size_t)1 << 31); }

template <typename T>
int img_encode_launch(const T *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze, float m, float c,
                      float hi, float c2, float ldc, float *ws, hipStream_t st)
{
    if (!img_fits(B, C, H, W)) return FINC_ERR_BAD_DIMS;
    const uintptr_t f32 = cpl_bits(noise, out) | (sizeof(T) == 4 ? (uintptr_t)img : 0), u8 = sizeof(T) == 1 ? (uintptr_t)img : 0;
    const ImgPlan p = img_plan(C, H, W, squeeze, f32, u8);
    const int P = cpl_parts(p.items, B);
    if ((long long)B * P >= (1LL << 31)) return FINC_ERR_BAD_DIMS;
    const auto kernel = p.form == IMG_SQ4     ? finc_image_encode_kernel<T, IMG_SQ4>
                        : p.form == IMG_SQ1   ? finc_image_encode_kernel<T, IMG_SQ1>
                        : p.form == IMG_FLAT4 ? finc_image_encode_kernel<T, IMG_FLAT4>
                                              : finc_image_encode_kernel<T, IMG_FLAT1>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)B * P)), dim3(CPL_THREADS), 0, st, img, noise, out, ws, ImgEncode{m, c, hi, c2}, ldc,
                       C, H, W, p.items, P);
    FINC_CHECK_LAUNCH();
    hipLaunchKernelGGL(finc_coupling_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float *)ws, P, logdet, (float *)nullptr, 0);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

template <typename T, bool LOGDET>
int img_decode_start(const float *z, T *out, int B, int C, int H, int W, int unsqueeze, float inv_m, float off, float hi, float ldc, float *ws,
                     hipStream_t st, int &P)
{
    const uintptr_t f32 = (uintptr_t)z | (sizeof(T) == 4 ? (uintptr_t)out : 0), u8 = sizeof(T) == 1 ? (uintptr_t)out : 0;
    const ImgPlan p = img_plan(C, H, W, unsqueeze, f32, u8);
    P = cpl_parts(p.items, B);
    if ((long long)B * P >= (1LL << 31)) return FINC_ERR_BAD_DIMS;
    const auto kernel = p.form == IMG_SQ4     ? finc_image_decode_kernel<T, IMG_SQ4, LOGDET>
                        : p.form == IMG_SQ1   ? finc_image_decode_kernel<T, IMG_SQ1, LOGDET>
                        : p.form == IMG_FLAT4 ? finc_image_decode_kernel<T, IMG_FLAT4, LOGDET>
                                              : finc_image_decode_kernel<T, IMG_FLAT1, LOGDET>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)B * P)), dim3(CPL_THREADS), 0, st, z, out, ws,
                       ImgDecode<T, LOGDET>{inv_m, off, hi - 1.f}, ldc, C, H, W, p.items, P);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

template <typename T>
int img_decode_launch(const float *z, T *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off, float hi,
                      float ldc, float *ws, hipStream_t st)
{
    if (!img_fits(B, C, H, W)) return FINC_ERR_BAD_DIMS;
    int P = 0;
    if (!logdet) return img_decode_start<T, false>(z, out, B, C, H, W, unsqueeze, inv_m, off, hi, ldc, ws, st, P);
    if (int e = img_decode_start<T, true>(z, out, B, C, H, W, unsqueeze, inv_m, off, hi, ldc, ws, st, P)) return e;
    hipLaunchKernelGGL(finc_coupling_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float *)ws, P, logdet, (float *)nullptr, 0);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

} // namespace

// floats: the log-det partials, B images x P parts, for the form with the most items (the one-position / one-pixel one)
size_t finc_image_workspace_floats(int B, int C, int H, int W, int squeeze)
{
    const long long items = squeeze ? (long long)C * (H / 2) * (W / 2) : (long long)C * H * W;
    return (size_t)cpl_partials_bound(items, B);
}

int finc_image_encode_u8_launch(const uint8_t *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                                float m, float c, float hi, float c2, float ldc, float *ws, hipStream_t st)
{
    return img_encode_launch<uint8_t>(img, noise, out, logdet, B, C, H, W, squeeze, m, c, hi, c2, ldc, ws, st);
}
int finc_image_encode_f32_launch(const float *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                                 float m, float c, float hi, float c2, float ldc, float *ws, hipStream_t st)
{
    return img_encode_launch<float>(img, noise, out, logdet, B, C, H, W, squeeze, m, c, hi, c2, ldc, ws, st);
}
int finc_image_decode_f32_launch(const float *z, float *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off,
                                 float hi, float ldc, float *ws, hipStream_t st)
{
    return img_decode_launch<float>(z, out, logdet, B, C, H, W, unsqueeze, inv_m, off, hi, ldc, ws, st);
}
int finc_image_decode_u8_launch(const float *z, uint8_t *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off,
                                float hi, float ldc, float *ws, hipStream_t st)
{
    return img_decode_launch<uint8_t>(z, out, logdet, B, C, H, W, unsqueeze, inv_m, off, hi, ldc, ws, st);
}

#endif /* FINC_IMAGE_H */
