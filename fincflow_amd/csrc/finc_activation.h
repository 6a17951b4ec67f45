// The smooth invertible activations for gfx950 (included by finc_mix.hip behind finc_spline.h: same object file, same helpers).  fp32 only.
//
// Reference: layers/activations.py SmoothLeakyRelu (:36-54), LeakyRelu (:57-79), LearnableLeakyRelu (:82-105), SmoothTanh (:108-123).
// There `forward` is torch.stack + logsumexp and a second pass through act_prime for the log-det, and the `reverse` of the two smooth
// kinds is newton_raphson_inverse (:26-33): 100 unbracketed Newton steps of a handful of launches each, which CYCLES for
// SmoothTanh(3, 0.05) (tanh is not convex: a step from the flat part overshoots).  Here every call is one read, the map in registers
// and one write.  With x the forward's input, f the forward map and L = log f':
//   FINC_ACT_SMOOTH_LEAKY_RELU (a)   f = a x + (1 - a) softplus(x)   f' = a + (1 - a) sigmoid(x)      L' = (1 - a) s (1 - s) / f'
//   FINC_ACT_LEAKY_RELU (a)          f = x < 0 ? a x : x             f' = x < 0 ? a : 1               L' = 0
//   FINC_ACT_LEARNABLE_LEAKY_RELU    the same, a read from a DEVICE pointer (the module's sigmoid(alpha_logit) + 0.5: no host round trip)
//   FINC_ACT_SMOOTH_TANH (a, b)      f = tanh(a x) + b x             f' = b + a sech^2(a x)           L' = -2 a^2 sech^2 tanh / f'
// softplus is max(x, 0) + log1p(exp(-|x|)) and sigmoid comes from the same exponential; sech^2 is 4 e / (1 + e)^2 and tanh
// (1 - e) / (1 + e) with e = exp(-2 |a x|): nothing overflows and nothing cancels.  The comparison is x < 0 strictly, as in the
// reference (-0 and 0 take the identity branch).  A NaN passes through with log-derivative 0, derivative 1 and L' = 0.
//
// The inverse of the two smooth kinds (act_inverse) is solved in registers: ACT_TRIPS Newton trips kept inside an analytic bracket.
//   smooth leaky ReLU: g(x) < f(x) <= g(x) + c (a <= 1; reversed for a > 1) with g the leaky ReLU of slope a and c = (1 - a) ln 2,
//                      so x lies between g^-1(y) and g^-1(y - c); the start is g^-1(y): f is convex (a < 1) or concave (a > 1) and
//                      Newton from that end walks to the root from one side.
//   smooth tanh:       f is odd: the solve runs on t = |y| and the result takes y's sign.  t / (a + b) <= x (f is concave on x >= 0
//                      with slope a + b at 0), (t - 1) / b <= x <= t / b; the start is the larger lower end, from which Newton on a
//                      concave function never overshoots.
// Each trip shrinks the bracket on the sign of f(x) - y and replaces a step that LEAVES [lo, hi] by the midpoint; a step onto an end
// is inside.  The trip count is the same for every lane: no data-dependent exit, the same inputs give the same bits.  ACT_TRIPS = 9:
// over the parameter box of DESIGN 3.26 the worst case (smooth tanh (8, 0.01)) is at its fp32 floor after 7 trips, plus 2 of margin.
// Outside that box the result is still finite and inside the bracket (the ends are clamped to the largest float), no more is claimed.
//
// The walk: the tensor is [B][N], N = C * HW, no channel structure.  Workgroup = (image, part): P = cpl_parts(items, B) parts share an
// image's items = N / V thread items, V = 4 (16-byte pieces) when N % 4 == 0 -- N, not HW -- and every activation pointer is 16-byte
// aligned, else V = 1.  Every index is checked against the item count; y == x is allowed (an item is read before it is written, by
// the same thread).  logdet[b], when asked for, is the FORWARD map's log-det in either direction (in direction -1 at the recovered
// input): a wave sums the 64 items of each chunk of 256 it meets in a butterfly and writes ONE partial per (image, chunk, wave) --
// part[(b * chunks + chunk) * 4 + wave], a layout that does not depend on P, so an image's log-det has the same bits whatever the
// batch around it -- and finc_coupling_reduce_kernel adds an image's partials in a fixed order.  No atomics.  The maps run with
// contraction off: which products fuse would otherwise depend on whether the instantiation also computes the log-det, and y is to
// carry the same bits with and without it.
//
// Every backward is ONE body, act_grad<KIND, V, MODE> (FincGradMode), on the same walk:
//   FINC_GRAD_FWD      from `v` = the forward's INPUT x:  grad_x = grad_y f'(x) + grad_logdet[b] L'(x).
//   FINC_GRAD_REV      of direction -1 from `v` = its OUTPUT x:  grad_y = (grad_x + grad_logdet[b] L'(x)) / f'(x).  No second solve, and
//                      the output is safe to differentiate from: there are no bins whose edges it could miss and f', L' do not
//                      cancel anywhere (the spline's reverse backward reads its INPUT for those two reasons).
//   FINC_GRAD_REBUILD  from `v` = the forward's OUTPUT y: x = act_inverse(y) -- the inverse kernel's own function, so xo (optional)
//                      has the bits `reverse` returns -- and the FINC_GRAD_FWD gradients at that x in the same launch.
// gy, gld, xo, gx may be nullptr; gx == gy and xo == v are allowed.  With a slope pointer and `sums` the body also sums the slope's
// gradient -- x < 0: grad_y x + grad_logdet / a (FWD, REBUILD), (-grad_x x + grad_logdet) / a (REV) -- per workgroup (cpl_block_sum)
// into part[blockIdx.x]; finc_coupling_reduce_kernel adds the B * P partials in a fixed order.
#ifndef FINC_ACTIVATION_H
#define FINC_ACTIVATION_H

namespace {

constexpr int ACT_TRIPS = 9;
constexpr float ACT_FLT_MAX = 3.4028234663852886e38f, ACT_LN2 = 0.6931471805599453f;
// (the learnable kind is the leaky kind with its slope behind a pointer: one set of instantiations)
constexpr int ACT_SLR = FINC_ACT_SMOOTH_LEAKY_RELU, ACT_LEAKY = FINC_ACT_LEAKY_RELU, ACT_STANH = FINC_ACT_SMOOTH_TANH;

// f(x) and f'(x) of the two smooth kinds (x not NaN)
template <int KIND>
__device__ __forceinline__ void act_eval(float x, float a, float b, float &f, float &fp)
{
#pragma clang fp contract(off)
    if constexpr (KIND == ACT_SLR) {
        const float e = expf(-fabsf(x)), sp = fmaxf(x, 0.f) + log1pf(e);
        const float s = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        f = a * x + (1.f - a) * sp;
        fp = a + (1.f - a) * s;
    } else {
        const float u = a * x, e = expf(-2.f * fabsf(u));
        const float t = (1.f - e) / (1.f + e);
        f = (u < 0.f ? -t : t) + b * x;
        fp = b + a * (4.f * e / ((1.f + e) * (1.f + e)));
    }
}

// y = f(x), ld = log f'(x); loga = log a (the leaky kinds)
template <int KIND>
__device__ __forceinline__ void act_forward(float x, float a, float b, float loga, float &y, float &ld)
{
#pragma clang fp contract(off)
    if constexpr (KIND == ACT_LEAKY) {
        const bool neg = x < 0.f;
        y = neg ? a * x : x;
        ld = neg ? loga : 0.f;
    } else {
        float f, fp;
        act_eval<KIND>(x, a, b, f, fp);
        const bool nan = x != x;
        y = nan ? x : f;
        ld = nan ? 0.f : logf(fp);
    }
}

// x = f^-1(y): a select and a division for the leaky kinds, ACT_TRIPS bracketed Newton trips for the smooth ones
template <int KIND>
__device__ __forceinline__ float act_inverse(float y, float a, float b)
{
#pragma clang fp contract(off)
    if constexpr (KIND == ACT_LEAKY) {
        return y < 0.f ? y / a : y;
    } else {
        float t, lo, hi, x;
        if constexpr (KIND == ACT_SLR) {
            const float v = y - (1.f - a) * ACT_LN2;
            const float g1 = fminf(fmaxf(y < 0.f ? y / a : y, -ACT_FLT_MAX), ACT_FLT_MAX);
            const float g2 = fminf(fmaxf(v < 0.f ? v / a : v, -ACT_FLT_MAX), ACT_FLT_MAX);
            t = y;
            lo = fminf(g1, g2);
            hi = fmaxf(g1, g2);
            x = g1;
        } else {
            t = fabsf(y);
            hi = fminf(t / b, ACT_FLT_MAX);
            lo = fminf(fmaxf(t / (a + b), (t - 1.f) / b), hi);
            x = lo;
        }
#pragma unroll 1
        for (int k = 0; k < ACT_TRIPS; ++k) {
            float f, fp;
            act_eval<KIND>(x, a, b, f, fp);
            const float r = f - t;
            hi = r > 0.f ? x : hi;
            lo = r < 0.f ? x : lo;
            const float xn = x - r / fp;
            x = (xn >= lo && xn <= hi) ? xn : lo + 0.5f * (hi - lo);
        }
        if constexpr (KIND == ACT_STANH) x = y < 0.f ? -x : x;
        return y != y ? y : x;
    }
}

// f'(x) and L'(x) = f''(x) / f'(x)
template <int KIND>
__device__ __forceinline__ void act_slopes(float x, float a, float b, float &fp, float &lp)
{
    if constexpr (KIND == ACT_LEAKY) {
        fp = x < 0.f ? a : 1.f;
        lp = 0.f;
    } else if constexpr (KIND == ACT_SLR) {
        const float e = expf(-fabsf(x)), i = 1.f / (1.f + e);
        const float s = x >= 0.f ? i : e * i;
        fp = a + (1.f - a) * s;
        lp = (1.f - a) * (e * i * i) / fp;                           // s (1 - s) = e / (1 + e)^2 on either side
    } else {
        const float u = a * x, e = expf(-2.f * fabsf(u)), i = 1.f / (1.f + e);
        const float t = (1.f - e) * i, S = 4.f * e * i * i;
        fp = b + a * S;
        lp = -2.f * a * a * S * (u < 0.f ? -t : t) / fp;
    }
    if (x != x) {
        fp = 1.f;
        lp = 0.f;
    }
}

template <int KIND, int V, int DIR, bool LOGDET>
__global__ __launch_bounds__(CPL_THREADS) void finc_activation_kernel(const float *x, const float *__restrict__ slope, float *y,
                                                                      float *__restrict__ part, float p0, float p1, int N, int items,
                                                                      int chunks, int P)
{
    const int img = (int)blockIdx.x / P, pi = (int)blockIdx.x - img * P;
    const size_t base = (size_t)img * (size_t)N;
    const float a = slope ? *slope : p0, b = p1, loga = KIND == ACT_LEAKY && LOGDET ? logf(a) : 0.f;
    // (the loop is uniform over the workgroup: every wave meets every chunk of its part, so the butterfly has all 64 lanes)
    for (int first = pi * CPL_THREADS; first < items; first += P * CPL_THREADS) {
        const int idx = first + (int)threadIdx.x;
        float ls = 0.f;
        if (idx < items) {
            const size_t o = base + (size_t)idx * V;
            float v[V], r[V];
            cpl_load<V>(v, x + o);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float ld = 0.f;
                if constexpr (DIR > 0) {
                    act_forward<KIND>(v[e], a, b, loga, r[e], ld);
                } else {
                    r[e] = act_inverse<KIND>(v[e], a, b);
                    if constexpr (LOGDET) {                          // the forward map's, at the recovered input
                        float f;
                        act_forward<KIND>(r[e], a, b, loga, f, ld);
                    }
                }
                if constexpr (LOGDET) ls += ld;
            }
            cpl_store<V>(y + o, r);
            // (s_nop 1: a store of more than 8 bytes reads its data registers a few cycles after issue; scripts/check_store_hazard.py
            // wants two wait states before anything is written to them -- here the butterfly's first shuffle lands in one)
            if constexpr (V == 4) asm volatile("s_nop 1");
        }
        if constexpr (LOGDET) {
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) ls += __shfl_xor(ls, k, 64);
            if ((threadIdx.x & 63) == 0)
                part[((size_t)img * chunks + (size_t)(first / CPL_THREADS)) * 4 + (threadIdx.x >> 6)] = ls;
        }
    }
}

template <int KIND, int V, int MODE>
__device__ __forceinline__ void act_grad(const float *gy, const float *__restrict__ gld, const float *v, const float *__restrict__ slope,
                                         float *xo, float *gx, float *__restrict__ part, float p0, float p1, int N, int items, int P,
                                         int sums)
{
    const int img = (int)blockIdx.x / P, pi = (int)blockIdx.x - img * P;
    const size_t base = (size_t)img * (size_t)N;
    const float a = slope ? *slope : p0, b = p1, ia = 1.f / a, gl = gld ? gld[img] : 0.f;
    float acc[1] = {0.f};
    for (int idx = pi * CPL_THREADS + (int)threadIdx.x; idx < items; idx += P * CPL_THREADS) {
        const size_t o = base + (size_t)idx * V;
        float g[V], w[V], out[V];
#pragma unroll
        for (int e = 0; e < V; ++e) g[e] = 0.f;
        if (gy) cpl_load<V>(g, gy + o);
        cpl_load<V>(w, v + o);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if constexpr (MODE == FINC_GRAD_REBUILD) w[e] = act_inverse<KIND>(w[e], a, b);
            float fp, lp;
            act_slopes<KIND>(w[e], a, b, fp, lp);
            if constexpr (MODE == FINC_GRAD_REV) out[e] = (g[e] + gl * lp) / fp;
            else out[e] = g[e] * fp + gl * lp;
            if constexpr (KIND == ACT_LEAKY) {
                if (sums && w[e] < 0.f) acc[0] += MODE == FINC_GRAD_REV ? (gl - g[e] * w[e]) * ia : g[e] * w[e] + gl * ia;
            }
        }
        if constexpr (MODE == FINC_GRAD_REBUILD)
            if (xo) cpl_store<V>(xo + o, w);
        if (gx) cpl_store<V>(gx + o, out);
        if constexpr (V == 4) asm volatile("s_nop 1");               // (as in finc_activation_kernel)
    }
    if constexpr (KIND == ACT_LEAKY) {
        if (sums) {
            __shared__ float sm[1][4];
            cpl_block_sum<1>(acc, sm);
            if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
        }
    }
}

template <int KIND, int V, int MODE>
__global__ __launch_bounds__(CPL_THREADS) void finc_activation_bwd_kernel(const float *gy, const float *__restrict__ gld, const float *v,
                                                                          const float *__restrict__ slope, float *xo, float *gx,
                                                                          float *__restrict__ part, float p0, float p1, int N, int items,
                                                                          int P, int sums)
{
    act_grad<KIND, V, MODE>(gy, gld, v, slope, xo, gx, part, p0, p1, N, items, P, sums);
}

// A launch: B images share N / V items each in P parts, a workgroup per (image, part); `chunks` blocks of 256 items per image.
// P = 0: the dimensions do not fit (FINC_ERR_BAD_DIMS).  `ptrs`: cpl_bits of every activation pointer the launch touches.
struct ActPlan {
    bool wide;
    int N, items, chunks, P;
};
inline ActPlan act_plan(int B, int C, int HW, uintptr_t ptrs)
{
    if ((size_t)C * HW * 4 >= ((size_t)1 << 31)) return ActPlan{false, 0, 0, 0, 0};
    const int N = C * HW;
    const bool wide = N % 4 == 0 && (ptrs & 15u) == 0;
    const int items = N / (wide ? 4 : 1), chunks = (items + CPL_THREADS - 1) / CPL_THREADS, P = cpl_parts(items, B);
    if ((long long)B * P >= (1LL << 31)) return ActPlan{false, 0, 0, 0, 0};
    return ActPlan{wide, N, items, chunks, P};
}

template <int KIND, int V>
void act_start(const ActPlan &p, int direction, bool logdet, dim3 grid, hipStream_t st, const float *x, const float *slope, float *y,
               float *ws, float p0, float p1)
{
    const auto kernel = direction > 0 ? (logdet ? finc_activation_kernel<KIND, V, 1, true> : finc_activation_kernel<KIND, V, 1, false>)
                                      : (logdet ? finc_activation_kernel<KIND, V, -1, true> : finc_activation_kernel<KIND, V, -1, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(CPL_THREADS), 0, st, x, slope, y, ws, p0, p1, p.N, p.items, p.chunks, p.P);
}

template <int KIND, int V>
void act_grad_start(const ActPlan &p, FincGradMode mode, dim3 grid, hipStream_t st, const float *gy, const float *gld, const float *v,
                    const float *slope, float *xo, float *gx, float *ws, float p0, float p1, int sums)
{
    const auto kernel = mode == FINC_GRAD_REBUILD ? finc_activation_bwd_kernel<KIND, V, FINC_GRAD_REBUILD>
                        : mode == FINC_GRAD_REV   ? finc_activation_bwd_kernel<KIND, V, FINC_GRAD_REV>
                                                  : finc_activation_bwd_kernel<KIND, V, FINC_GRAD_FWD>;
    hipLaunchKernelGGL(kernel, grid, dim3(CPL_THREADS), 0, st, gy, gld, v, slope, xo, gx, ws, p0, p1, p.N, p.items, p.P, sums);
}

inline int act_device_kind(int kind) { return kind == FINC_ACT_LEARNABLE_LEAKY_RELU ? ACT_LEAKY : kind; }

} // namespace

int finc_activation_trips(int kind)
{
    if (kind == FINC_ACT_SMOOTH_LEAKY_RELU || kind == FINC_ACT_SMOOTH_TANH) return ACT_TRIPS;
    return (kind == FINC_ACT_LEAKY_RELU || kind == FINC_ACT_LEARNABLE_LEAKY_RELU) ? 0 : -1;
}

// floats: the log-det's partials (four per image and chunk of 256 items, for the dword form's item count) or the slope gradient's (one
// per workgroup)
size_t finc_activation_workspace_floats(int B, int C, int HW)
{
    const long long N = (long long)C * HW, logdet = 4LL * B * ((N + CPL_THREADS - 1) / CPL_THREADS), grads = cpl_partials_bound(N, B);
    return (size_t)(logdet > grads ? logdet : grads);
}

int finc_activation_launch(int kind, float p0, float p1, const float *slope, int direction, const float *x, float *y, float *logdet, int B,
                           int C, int HW, float *ws, hipStream_t st)
{
    const ActPlan p = act_plan(B, C, HW, cpl_bits(x, y));
    if (!p.P) return FINC_ERR_BAD_DIMS;
    const dim3 grid((unsigned)((long long)B * p.P));
    const bool ld = logdet != nullptr;
#define ACT_START(KIND) (p.wide ? act_start<KIND, 4>(p, direction, ld, grid, st, x, slope, y, ws, p0, p1) \
                                : act_start<KIND, 1>(p, direction, ld, grid, st, x, slope, y, ws, p0, p1))
    switch (act_device_kind(kind)) {
    case ACT_SLR: ACT_START(ACT_SLR); break;
    case ACT_LEAKY: ACT_START(ACT_LEAKY); break;
    case ACT_STANH: ACT_START(ACT_STANH); break;
    default: return FINC_ERR_UNSUPPORTED;
    }
#undef ACT_START
    FINC_CHECK_LAUNCH();
    if (logdet) {
        hipLaunchKernelGGL(finc_coupling_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float *)ws, 4 * p.chunks, logdet,
                           (float *)nullptr, 0);
        FINC_CHECK_LAUNCH();
    }
    return FINC_OK;
}

// v: the forward's INPUT (FINC_GRAD_FWD), the reverse's OUTPUT (FINC_GRAD_REV) or the forward's OUTPUT (FINC_GRAD_REBUILD)
int finc_activation_grad_launch(int kind, float p0, float p1, const float *slope, FincGradMode mode, const float *gy, const float *gld,
                                const float *v, float *xo, float *gx, float *gs, int B, int C, int HW, float *ws, hipStream_t st)
{
    const ActPlan p = act_plan(B, C, HW, cpl_bits(gy, v, xo, gx));
    if (!p.P) return FINC_ERR_BAD_DIMS;
    const dim3 grid((unsigned)((long long)B * p.P));
    const int sums = gs ? 1 : 0;
#define ACT_GRAD_START(KIND) (p.wide ? act_grad_start<KIND, 4>(p, mode, grid, st, gy, gld, v, slope, xo, gx, ws, p0, p1, sums) \
                                     : act_grad_start<KIND, 1>(p, mode, grid, st, gy, gld, v, slope, xo, gx, ws, p0, p1, sums))
    switch (act_device_kind(kind)) {
    case ACT_SLR: ACT_GRAD_START(ACT_SLR); break;
    case ACT_LEAKY: ACT_GRAD_START(ACT_LEAKY); break;
    case ACT_STANH: ACT_GRAD_START(ACT_STANH); break;
    default: return FINC_ERR_UNSUPPORTED;
    }
#undef ACT_GRAD_START
    FINC_CHECK_LAUNCH();
    if (gs) {
        hipLaunchKernelGGL(finc_coupling_reduce_kernel, dim3(1), dim3(64), 0, st, (const float *)ws, (int)((long long)B * p.P), gs,
                           (float *)nullptr, 0);
        FINC_CHECK_LAUNCH();
    }
    return FINC_OK;
}

#endif /* FINC_ACTIVATION_H */
