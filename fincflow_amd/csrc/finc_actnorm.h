// ActNorm for gfx950 (included by finc_mix.hip behind finc_coupling.h: same object file, same helpers).
//
// Reference: layers/actnorm.py:5-66.  Under autograd the reference's layer is about twenty PyTorch launches per step (sub, neg, exp,
// mul; sum, neg, expand, mul for the log-det; autograd's chain behind them) and keeps `x - translation` alive until the backward.  Here:
//   * finc_actnorm_kernel        one pass: y = (x - t[c]) * exp(-ls[c]) (forward, layers/actnorm.py:34) or y = x * exp(ls[c]) + t[c]
//                                (reverse, :51); with a log-det pointer the first wave of the launch also writes
//                                logdet[b] = -(sum_c ls[c]) * HW for every image (:57-65): a training forward is ONE launch.
//   * an_grad<V, MODE>           one pass over grad_y and y (the forward's OUTPUT: x - t = y * exp(ls), so
//                                d loss / d ls[c] = -sum grad_y * y needs nothing the forward's caller does not keep anyway):
//                                grad_x = grad_y * exp(-ls[c]) and the two per-channel sums, then finc_coupling_reduce_kernel.  Its
//                                modes are the kernels finc_actnorm_bwd_kernel (that), finc_actnorm_recon_kernel (that, and the
//                                forward's INPUT rebuilt from the same read of y: the step of a training backward that stores no
//                                activations, FlowSequential.invertible_backward) and finc_actnorm_rev_bwd_kernel (the reverse
//                                direction, from the reverse's INPUT: what `reverse` under autograd records inside
//                                ops.reverse_grad()).
//   * finc_actnorm_stats_kernel  the data-dependent initialisation (:17-23): per-channel mean and unbiased standard deviation in ONE
//                                pass over x.  Every thread folds its pieces into a running (n, mean, M2) triple (Chan et al.'s pairwise
//                                update: the squares are taken of differences from a running mean, never of x itself -- the
//                                sum(x^2) - sum(x)^2 / n form loses everything on a channel with mean 1000 and std 0.01); triples
//                                meet in a fixed order (lanes in a butterfly, the four waves in LDS, the workgroups of a channel in
//                                finc_actnorm_stats_final_kernel), which writes translation[c] and log_scale[c] = log(std + 1e-8).
// Layout [B][C][HW] fp32.  A thread item is V consecutive pixels of one (image, channel) row: V = 4 (16-byte pieces) when HW % 4 == 0
// and every activation pointer is 16-byte aligned, else V = 1 (dwords).  Every index is checked against the item count: nothing is
// read or written beyond a tensor.  No atomics: every sum runs in a fixed order, the same inputs give the same bits.
#ifndef FINC_ACTNORM_H
#define FINC_ACTNORM_H

namespace {

// Grid-stride over the B * C * HW / V items.  y == x is allowed (an item is read before it is written, by the same thread).
template <int V, int DIR>
__global__ __launch_bounds__(CPL_THREADS) void finc_actnorm_kernel(const float *x, const float *__restrict__ ls,
                                                                   const float *__restrict__ tr, float *y, float *__restrict__ logdet,
                                                                   int B, int C, int HW, int nv, unsigned items)
{
    for (unsigned idx = blockIdx.x * CPL_THREADS + threadIdx.x; idx < items; idx += gridDim.x * CPL_THREADS) {
        const unsigned row = idx / (unsigned)nv, p = (idx - row * (unsigned)nv) * V;
        const unsigned c = row % (unsigned)C;
        const float s = expf(DIR > 0 ? -ls[c] : ls[c]), t = tr[c];
        const size_t o = (size_t)row * HW + p;
        float v[V];
        cpl_load<V>(v, x + o);
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = DIR > 0 ? (v[e] - t) * s : fmaf(v[e], s, t);
        cpl_store<V>(y + o, v);
    }
    if constexpr (DIR > 0) {
        if (logdet && blockIdx.x == 0 && threadIdx.x < 64) {       // one wave: lane l takes channels l, l + 64, ...; a butterfly
            float s = 0.f;
            for (int c = (int)threadIdx.x; c < C; c += 64) s += ls[c];
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
            const float v = -s * (float)HW;
            for (int b = (int)threadIdx.x; b < B; b += 64) logdet[b] = v;
        }
    }
}

// Every backward of ActNorm is ONE body, an_grad<V, MODE>; a mode (FincGradMode) is what it reads, its scale and its partials:
//   FINC_GRAD_FWD      of y = (x - t[c]) * exp(-ls[c]), from `v` = the forward's OUTPUT y: grad_x = grad_y * exp(-ls[c]).
//   FINC_GRAD_REBUILD  that backward, and from the same read of y the forward's input: xo = y * exp(ls[c]) + t[c] (the arithmetic of
//                      finc_actnorm_kernel's reverse direction, so the same bits).  What a training step without stored activations
//                      runs per ActNorm: one launch instead of a reverse launch plus a backward launch, y read once.  xo (then tr is
//                      not read) may be nullptr; xo == v is allowed.
//   FINC_GRAD_REV      of y = x * exp(ls[c]) + t[c] (layers/actnorm.py:47-52), from `v` = the reverse's INPUT x: grad_x = grad_y *
//                      exp(ls[c]), grad_ls[c] = exp(ls[c]) * sum grad_y * x, grad_t[c] = sum grad_y.  (The output would do in real
//                      arithmetic -- x * exp(ls) = y - t -- but on a channel with |t| >> |y - t| that difference has lost its digits.)
// Workgroup = (channel c, part q): Q parts share the channel's B * HW / V items, so a workgroup's sums belong to ONE channel.
// Partials, n per output, output 2c = grad_t[c], 2c + 1 = grad_ls[c] (the layout finc_coupling_reduce_kernel's pair mode sends to
// out_a[c] / out_b[c]).  The two forward modes, n = Q + 1:  part[(2c) * n + q] = -exp(-ls[c]) * sum gy,  part[(2c+1) * n + q] =
// -sum gy * y;  slot Q of grad_ls is -HW * sum_b gld[b] (added by the channel's part 0, one wave in a fixed order), slot Q of grad_t is
// zero.  The reverse mode, n = Q:  part[(2c) * Q + q] = sum gy,  part[(2c+1) * Q + q] = exp(ls[c]) * sum gy * x.
// gld, gx may be nullptr; `sums` = 0 skips the partials; `need_v` = 0 (neither xo nor grad_ls) skips the read of v.  gx == gy is allowed
// (an item is read before it is written, by the same thread).
template <int V, int MODE>
__device__ __forceinline__ void an_grad(const float *gy, const float *__restrict__ gld, const float *v, const float *__restrict__ ls,
                                        const float *__restrict__ tr, float *xo, float *gx, float *__restrict__ part, int B, int C, int HW,
                                        int nv, int items, int Q, int sums, int need_v)
{
    constexpr bool REBUILD = MODE == FINC_GRAD_REBUILD, REV = MODE == FINC_GRAD_REV;
    const int c = (int)blockIdx.x / Q, qi = (int)blockIdx.x - c * Q;
    const float l = ls[c], s = expf(REV ? l : -l), si = REBUILD ? expf(l) : 0.f, t = REBUILD && xo ? tr[c] : 0.f;
    float acc[2] = {0.f, 0.f};
    for (int idx = qi * CPL_THREADS + (int)threadIdx.x; idx < items; idx += Q * CPL_THREADS) {
        const int img = idx / nv, p = (idx - img * nv) * V;
        const size_t o = ((size_t)img * C + c) * (size_t)HW + p;
        float g[V], vv[V], d[V], xv[V];
        cpl_load<V>(g, gy + o);
        if (need_v) cpl_load<V>(vv, v + o);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            d[e] = g[e] * s;
            acc[0] += g[e];
            if (need_v) {
                acc[1] = fmaf(g[e], vv[e], acc[1]);
                if constexpr (REBUILD) xv[e] = fmaf(vv[e], si, t);
            }
        }
        if constexpr (REBUILD)
            if (xo) cpl_store<V>(xo + o, xv);
        if (gx) cpl_store<V>(gx + o, d);
    }
    if (sums) {
        __shared__ float sm[2][4];
        cpl_block_sum<2>(acc, sm);
        const int n = REV ? Q : Q + 1;
        float *p0 = part + (size_t)(2 * c) * n, *p1 = p0 + n;
        if (threadIdx.x == 0) {
            p0[qi] = REV ? acc[0] : -s * acc[0];
            p1[qi] = REV ? s * acc[1] : -acc[1];
        }
        if constexpr (!REV) {
            if (qi == 0 && threadIdx.x < 64) {
                float gl = 0.f;
                if (gld)
                    for (int b = (int)threadIdx.x; b < B; b += 64) gl += gld[b];
#pragma unroll
                for (int k = 32; k > 0; k >>= 1) gl += __shfl_xor(gl, k, 64);
                if (threadIdx.x == 0) {
                    p0[Q] = 0.f;
                    p1[Q] = -(float)HW * gl;
                }
            }
        }
    }
}

// The three modes under the names and parameter lists they have always had.  y / x nullptr (the launcher's, without grad_ls): not read.
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_actnorm_bwd_kernel(const float *gy, const float *__restrict__ gld,
                                                                       const float *__restrict__ y, const float *__restrict__ ls, float *gx,
                                                                       float *__restrict__ part, int B, int C, int HW, int nv, int items, int Q,
                                                                       int sums)
{
    an_grad<V, FINC_GRAD_FWD>(gy, gld, y, ls, nullptr, nullptr, gx, part, B, C, HW, nv, items, Q, sums, y != nullptr);
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_actnorm_recon_kernel(const float *gy, const float *__restrict__ gld, const float *y,
                                                                         const float *__restrict__ ls, const float *__restrict__ tr,
                                                                         float *xo, float *gx, float *__restrict__ part, int B, int C, int HW,
                                                                         int nv, int items, int Q, int sums, int need_y)
{
    an_grad<V, FINC_GRAD_REBUILD>(gy, gld, y, ls, tr, xo, gx, part, B, C, HW, nv, items, Q, sums, need_y);
}

template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_actnorm_rev_bwd_kernel(const float *gy, const float *__restrict__ x,
                                                                           const float *__restrict__ ls, float *gx,
                                                                           float *__restrict__ part, int C, int HW, int nv, int items, int Q,
                                                                           int sums)
{
    an_grad<V, FINC_GRAD_REV>(gy, nullptr, x, ls, nullptr, nullptr, gx, part, 0, C, HW, nv, items, Q, sums, x != nullptr);
}

// (count, mean, sum of squared differences from the mean) of a set of values; two disjoint sets merge exactly in real arithmetic
// (Chan, Golub, LeVeque 1979), and in floating point without ever squaring anything larger than a difference of means.  The count is
// carried as a float: it only weighs the merge (b.n / n), so beyond 2^24 values per channel, where it stops being exact, the weights
// are off by 1e-7 relative like every other operand here; the divisor n - 1 of the variance comes from the host's integer.
struct AnStat {
    float n, mean, m2;
};
__device__ inline AnStat an_merge(const AnStat a, const AnStat b)
{
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    const float n = a.n + b.n, d = b.mean - a.mean, w = b.n / n;
    return AnStat{n, fmaf(d, w, a.mean), a.m2 + b.m2 + d * d * a.n * w};
}
__device__ inline AnStat an_shfl_xor(const AnStat a, int k)
{
    return AnStat{__shfl_xor(a.n, k, 64), __shfl_xor(a.mean, k, 64), __shfl_xor(a.m2, k, 64)};
}
// lanes of a wave meet in a butterfly; the lower lane of a pair is always the left operand, so lane 0 ends with a fixed tree
__device__ inline AnStat an_wave_merge(AnStat a)
{
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const AnStat o = an_shfl_xor(a, k);
        a = (threadIdx.x & k) ? an_merge(o, a) : an_merge(a, o);
    }
    return a;
}

// Workgroup = (channel c, part q) as in the backward.  part[(c * Q + q) * 3 + {0, 1, 2}] = the workgroup's (n, mean, M2).
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_actnorm_stats_kernel(const float *__restrict__ x, float *__restrict__ part, int C,
                                                                         int HW, int nv, int items, int Q)
{
    const int c = (int)blockIdx.x / Q, qi = (int)blockIdx.x - c * Q;
    AnStat a{0.f, 0.f, 0.f};
    for (int idx = qi * CPL_THREADS + (int)threadIdx.x; idx < items; idx += Q * CPL_THREADS) {
        const int img = idx / nv, p = (idx - img * nv) * V;
        float v[V];
        cpl_load<V>(v, x + ((size_t)img * C + c) * (size_t)HW + p);
        AnStat b{(float)V, v[0], 0.f};
        if constexpr (V == 4) {
            b.mean = 0.25f * ((v[0] + v[1]) + (v[2] + v[3]));
#pragma unroll
            for (int e = 0; e < 4; ++e) b.m2 = fmaf(v[e] - b.mean, v[e] - b.mean, b.m2);
        }
        a = an_merge(a, b);
    }
    a = an_wave_merge(a);
    __shared__ float sm[3][4];
    if ((threadIdx.x & 63) == 0) {
        sm[0][threadIdx.x >> 6] = a.n;
        sm[1][threadIdx.x >> 6] = a.mean;
        sm[2][threadIdx.x >> 6] = a.m2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const AnStat w0{sm[0][0], sm[1][0], sm[2][0]}, w1{sm[0][1], sm[1][1], sm[2][1]}, w2{sm[0][2], sm[1][2], sm[2][2]},
            w3{sm[0][3], sm[1][3], sm[2][3]};
        const AnStat r = an_merge(an_merge(w0, w1), an_merge(w2, w3));
        float *dst = part + ((size_t)c * Q + qi) * 3;
        dst[0] = r.n;
        dst[1] = r.mean;
        dst[2] = r.m2;
    }
}

// One wave per channel: lane l folds the triples l, l + 64, ... of its channel in order, the lanes meet in the butterfly above.
// n = B * HW >= 2 (the caller's check): translation[c] = mean, log_scale[c] = log(sqrt(M2 / (n - 1)) + 1e-8), torch.std's divisor.
__global__ __launch_bounds__(64) void finc_actnorm_stats_final_kernel(const float *__restrict__ part, int Q, float *__restrict__ ls,
                                                                      float *__restrict__ tr, float nm1)
{
    const int c = (int)blockIdx.x;
    const float *p = part + (size_t)c * Q * 3;
    AnStat a{0.f, 0.f, 0.f};
    for (int i = (int)threadIdx.x; i < Q; i += 64) a = an_merge(a, AnStat{p[3 * i], p[3 * i + 1], p[3 * i + 2]});
    a = an_wave_merge(a);
    if (threadIdx.x == 0) {
        tr[c] = a.mean;
        ls[c] = logf(sqrtf(a.m2 / nm1) + 1e-8f);
    }
}

} // namespace

// floats: backward partials (2 outputs x C channels x (Q + 1)) or the stats' triples (3 x C x Q).  C * Q at its bound
// (cpl_partials_bound) for the dword form's item count is reserved three times over, plus the 2 C extra slots of the backward.
size_t finc_actnorm_workspace_floats(int B, int C, int HW)
{
    return (size_t)(3 * cpl_partials_bound((long long)B * HW, C) + 2LL * C);
}

int finc_actnorm_launch(const float *x, const float *ls, const float *tr, float *y, float *logdet, int B, int C, int HW, int direction,
                        hipStream_t st)
{
    const CplRowPlan rp = cpl_row_plan((long long)B * C, HW, 4, (uintptr_t)x | (uintptr_t)y);
    if (!rp.wgs) return FINC_ERR_BAD_DIMS;
    const bool wide = rp.wide;
    const int nv = rp.nv;
    const long long items = rp.items;
    const unsigned wgs = rp.wgs;
    const auto kernel = direction > 0 ? (wide ? finc_actnorm_kernel<4, 1> : finc_actnorm_kernel<1, 1>)
                                      : (wide ? finc_actnorm_kernel<4, -1> : finc_actnorm_kernel<1, -1>);
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(CPL_THREADS), 0, st, x, ls, tr, y, logdet, B, C, HW, nv, (unsigned)items);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

// v: the forward's OUTPUT (FINC_GRAD_FWD, FINC_GRAD_REBUILD) or the reverse's INPUT (FINC_GRAD_REV, which takes no gld); tr and xo
// with FINC_GRAD_REBUILD only
int finc_actnorm_grad_launch(FincGradMode mode, const float *gy, const float *gld, const float *v, const float *ls, const float *tr,
                             float *xo, float *gx, float *gls, float *gt, int B, int C, int HW, float *ws, hipStream_t st)
{
    const int need_v = (xo || gls) ? 1 : 0, sums = (gls || gt) ? 1 : 0;      // grad_ls and the rebuilt input read v
    if (!need_v) v = nullptr;
    const CplGradPlan p = cpl_grad_plan(B, C, HW, C, cpl_bits(gy, v, xo, gx));
    if (!p.Q) return FINC_ERR_BAD_DIMS;
    const dim3 block(CPL_THREADS);
    if (mode == FINC_GRAD_REBUILD)
        hipLaunchKernelGGL(p.wide ? finc_actnorm_recon_kernel<4> : finc_actnorm_recon_kernel<1>, p.grid, block, 0, st, gy, gld, v, ls, tr, xo,
                           gx, ws, B, C, HW, p.nv, p.items, p.Q, sums, need_v);
    else if (mode == FINC_GRAD_REV)
        hipLaunchKernelGGL(p.wide ? finc_actnorm_rev_bwd_kernel<4> : finc_actnorm_rev_bwd_kernel<1>, p.grid, block, 0, st, gy, v, ls, gx, ws, C,
                           HW, p.nv, p.items, p.Q, sums);
    else
        hipLaunchKernelGGL(p.wide ? finc_actnorm_bwd_kernel<4> : finc_actnorm_bwd_kernel<1>, p.grid, block, 0, st, gy, gld, v, ls, gx, ws, B, C,
                           HW, p.nv, p.items, p.Q, sums);
    FINC_CHECK_LAUNCH();
    return cpl_reduce_pairs(sums, ws, 2 * C, mode == FINC_GRAD_REV ? p.Q : p.Q + 1, gt, gls, st);
}

int finc_actnorm_init_launch(const float *x, float *ls, float *tr, int B, int C, int HW, float *ws, hipStream_t st)
{
    const CplGradPlan p = cpl_grad_plan(B, C, HW, C, cpl_bits(x));
    if (!p.Q) return FINC_ERR_BAD_DIMS;
    hipLaunchKernelGGL(p.wide ? finc_actnorm_stats_kernel<4> : finc_actnorm_stats_kernel<1>, p.grid, dim3(CPL_THREADS), 0, st, x, ws, C, HW,
                       p.nv, p.items, p.Q);
    FINC_CHECK_LAUNCH();
    hipLaunchKernelGGL(finc_actnorm_stats_final_kernel, dim3((unsigned)C), dim3(64), 0, st, (const float *)ws, p.Q, ls, tr,
                       (float)((long long)B * HW - 1));
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

#endif /* FINC_ACTNORM_H */
