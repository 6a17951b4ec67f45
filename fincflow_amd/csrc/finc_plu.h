// The PLU-parametrised 1x1 convolution's parameter work for gfx950 (included by finc_mix.hip behind finc_adjoint.h: same object file,
// same helpers).  glow.Conv1x1LU keeps  W = P L Ut,  L = strict_lower(lower) + I,  Ut = strict_upper(upper) + diag(d),
// d = sign_s * exp(log_s),  W[r, :] = M[perm[r], :] with M = L Ut.  Here:
//   * finc_plu_compose_kernel       any subset of w [C][C], w_inv [C][C] and logdet (one float) from the five inputs, ONE launch.  All
//                                   arithmetic in fp64, every output rounded to fp32 once, every sum in a fixed order, no atomics.
//                                     w      one thread per entry: (r, j) is a dot product of length min(perm[r], j) + 1.
//                                     w_inv  one WAVE per row i of M^-1 = Ut^-1 L^-1 (W^-1[i][c] = M^-1[i][perm[c]]):  z^T Ut = e_i^T, then
//                                            x^T L = z^T.  Both solves in the column-oriented (axpy) form ON ROWS of the stored matrices --
//                                            step k takes the finished z[k] (a v_readlane of the owner lane: k is wave-uniform) and
//                                            subtracts z[k] * Ut[k][j] from every later j, which are consecutive floats of row k -- so
//                                            every global read is coalesced and the chain of a solve is C steps, not the C^2 / 2
//                                            dependent FMAs of one thread per column (finc_adjoint_weights_kernel's form).  The wave keeps
//                                            its row in registers, lane l holding entries l, l + 64, ...; z is zero before entry i, so
//                                            the first solve starts at step i.  A workgroup's four waves share the rows of Ut / L,
//                                            staged PLU_RB at a time in LDS by all 256 threads.
//                                     logdet sum(log_s), one thread, ascending.
//   * finc_plu_compose_bwd_kernel   grad_lower = strict_lower(G_M Ut^T), grad_upper = strict_upper(L^T G_M), grad_log_s[i] =
//                                   (L^T G_M)[i][i] * d[i] + g_ld from G = dl/dW (G_M[perm[r]][:] = G[r][:]), each wanted or not by
//                                   pointer: one thread per entry, one fp64 dot product in ascending order each; the masked entries are
//                                   written as +0 by the kernel.
// `perm` lives in device memory and is never used as an index unchecked: an entry outside [0, C) makes row r of w and column r of w_inv
// NaN; in the backward the row of G_M that no entry names reads as NaN (row i of grad_lower, rows <= i of L^T G_M).  Nothing else is
// touched.  Widths: 1 <= C <= FINC_PLU_MAX_C, bounded by the LDS of the staged rows (88 bytes per channel: 44 KiB at 512).
#ifndef FINC_PLU_H
#define FINC_PLU_H

namespace {

constexpr int PLU_THREADS = 256;
constexpr int PLU_WAVES = PLU_THREADS / 64;             // rows of M^-1 per workgroup
constexpr int PLU_RB = 16;                              // rows of upper / lower staged at a time
constexpr int PLU_SLOTS = FINC_PLU_MAX_C / 64;          // entries of its row a lane holds
constexpr size_t PLU_LDS_PER_CHANNEL = sizeof(double) + (PLU_RB + PLU_WAVES) * sizeof(float);

// `v` of lane `lane` (wave-uniform) in every lane
__device__ inline double plu_readlane(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ inline double plu_diag(const float *__restrict__ log_s, const float *__restrict__ sign_s, int k)
{
    return (double)sign_s[k] * exp((double)log_s[k]);
}

// grid: n_inv workgroups of PLU_WAVES rows of M^-1 (first: the longest), n_w workgroups of 256 entries of one row of w, then one for
// the log-det; each part only where its output is wanted.  LDS (w_inv only): 1 / d [C] doubles, the staged rows [PLU_RB][C] floats,
// the waves' finished rows [PLU_WAVES][C] floats.
__global__ __launch_bounds__(PLU_THREADS) void finc_plu_compose_kernel(const float *__restrict__ lower, const float *__restrict__ upper,
                                                                       const float *__restrict__ log_s, const float *__restrict__ sign_s,
                                                                       const int *__restrict__ perm, float *__restrict__ w,
                                                                       float *__restrict__ w_inv, float *__restrict__ logdet, int C,
                                                                       int n_inv, int n_w)
{
    extern __shared__ __attribute__((aligned(16))) double plu_lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int blk = (int)blockIdx.x;
    if (blk < n_inv) {
        double *dinv = plu_lds;
        float *stage = (float *)(dinv + C);
        float *xrow = stage + PLU_RB * C + wave * C;
        for (int k = tid; k < C; k += PLU_THREADS) dinv[k] = 1.0 / plu_diag(log_s, sign_s, k);
        const int i = blk * PLU_WAVES + wave;                        // (a wave past the last row stages and waits with the others)
        const int nr = (C + 63) >> 6;
        double acc[PLU_SLOTS];
#pragma unroll
        for (int t = 0; t < PLU_SLOTS; ++t) acc[t] = (lane + 64 * t == i) ? 1.0 : 0.0;
        // z^T Ut = e_i^T, ascending: z[k] = acc[k] / d[k], then acc[j] -= z[k] * Ut[k][j] for j > k
        for (int kb = 0; kb < C; kb += PLU_RB) {
            const int rows = min(PLU_RB, C - kb);
            __syncthreads();                                         // (the first pass: dinv; later ones: the last block's readers)
            for (int e = tid; e < rows * C; e += PLU_THREADS) stage[e] = upper[(size_t)kb * C + e];
            __syncthreads();
            if (i < C)
                for (int k = max(kb, i); k < kb + rows; ++k) {
                    const int kt = k >> 6, kl = k & 63;
                    double zk = 0.0;
#pragma unroll
                    for (int t = 0; t < PLU_SLOTS; ++t)
                        if (t == kt) zk = plu_readlane(acc[t], kl);
                    zk *= dinv[k];
                    const float *row = stage + (k - kb) * C;
#pragma unroll
                    for (int t = 0; t < PLU_SLOTS; ++t) {
                        if (t < kt || t >= nr) continue;             // (wave-uniform: a slot that ends at or before k, or past C)
                        const int j = lane + 64 * t;
                        if (j == k) acc[t] = zk;
                        else if (j > k && j < C) acc[t] = fma(-zk, (double)row[j], acc[t]);
                    }
                }
        }
        // x^T L = z^T, descending: x[k] = acc[k] (unit diagonal), then acc[j] -= x[k] * L[k][j] for j < k
        for (int kb = ((C - 1) / PLU_RB) * PLU_RB; kb >= 0; kb -= PLU_RB) {
            const int rows = min(PLU_RB, C - kb);
            __syncthreads();
            for (int e = tid; e < rows * C; e += PLU_THREADS) stage[e] = lower[(size_t)kb * C + e];
            __syncthreads();
            if (i < C)
                for (int k = kb + rows - 1; k >= max(kb, 1); --k) {
                    const int kt = k >> 6, kl = k & 63;
                    double xk = 0.0;
#pragma unroll
                    for (int t = 0; t < PLU_SLOTS; ++t)
                        if (t == kt) xk = plu_readlane(acc[t], kl);
                    const float *row = stage + (k - kb) * C;
#pragma unroll
                    for (int t = 0; t < PLU_SLOTS; ++t) {
                        if (t > kt) continue;
                        const int j = lane + 64 * t;
                        if (j < k) acc[t] = fma(-xk, (double)row[j], acc[t]);
                    }
                }
        }
        if (i < C) {
#pragma unroll
            for (int t = 0; t < PLU_SLOTS; ++t) {
                const int j = lane + 64 * t;
                if (j < C) xrow[j] = (float)acc[t];
            }
        }
        __syncthreads();
        if (i < C)
            for (int c = lane; c < C; c += 64) {
                const int p = perm[c];
                w_inv[(size_t)i * C + c] = (p >= 0 && p < C) ? xrow[p] : __builtin_nanf("");
            }
        return;
    }
    blk -= n_inv;
    if (blk < n_w) {
        const int per_row = (C + PLU_THREADS - 1) / PLU_THREADS;
        const int r = blk / per_row, j = (blk - r * per_row) * PLU_THREADS + tid;
        if (j >= C) return;
        const int p = perm[r];
        if (p < 0 || p >= C) {
            w[(size_t)r * C + j] = __builtin_nanf("");
            return;
        }
        const float *lp = lower + (size_t)p * C;
        const int m = min(p, j);
        double s = 0.0;
        for (int k = 0; k < m; ++k) s = fma((double)lp[k], (double)upper[(size_t)k * C + j], s);
        const double dj = plu_diag(log_s, sign_s, j);
        s += p < j ? (double)upper[(size_t)p * C + j] : p == j ? dj : (double)lp[j] * dj;
        w[(size_t)r * C + j] = (float)s;
        return;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < C; ++k) s += (double)log_s[k];
        *logdet = (float)s;
    }
}

// grid: n_up workgroups of 256 entries of one row of L^T G_M (grad_upper, grad_log_s), then as many of G_M Ut^T (grad_lower) where
// that is wanted.  LDS: the inverse permutation [C] ints, -1 for a row of G_M that no entry of `perm` names.
__global__ __launch_bounds__(PLU_THREADS) void finc_plu_compose_bwd_kernel(const float *__restrict__ gw, const float *__restrict__ g_ld,
                                                                           const float *__restrict__ lower, const float *__restrict__ upper,
                                                                           const float *__restrict__ log_s, const float *__restrict__ sign_s,
                                                                           const int *__restrict__ perm, float *__restrict__ g_lower,
                                                                           float *__restrict__ g_upper, float *__restrict__ g_log_s, int C,
                                                                           int n_up)
{
    extern __shared__ __attribute__((aligned(16))) int plu_iperm[];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < C; i += PLU_THREADS) plu_iperm[i] = -1;
    __syncthreads();
    for (int r = tid; r < C; r += PLU_THREADS) {
        const int p = perm[r];
        if (p >= 0 && p < C) plu_iperm[p] = r;
    }
    __syncthreads();
    const int per_row = (C + PLU_THREADS - 1) / PLU_THREADS;
    int blk = (int)blockIdx.x;
    if (blk < n_up) {
        const int a = blk / per_row, b = (blk - a * per_row) * PLU_THREADS + tid;
        if (b >= C) return;
        double s = 0.0;
        if (b > a ? g_upper != nullptr : b == a)
            for (int i = a; i < C; ++i) {
                const int r = plu_iperm[i];
                const double g = r < 0 ? (double)__builtin_nanf("") : (double)gw[(size_t)r * C + b];
                s = fma(i == a ? 1.0 : (double)lower[(size_t)i * C + a], g, s);
            }
        if (g_upper) g_upper[(size_t)a * C + b] = b > a ? (float)s : 0.f;
        if (b == a && g_log_s) g_log_s[a] = (float)(s * plu_diag(log_s, sign_s, a) + (g_ld ? (double)*g_ld : 0.0));
        return;
    }
    blk -= n_up;
    const int i = blk / per_row, j = (blk - i * per_row) * PLU_THREADS + tid;
    if (j >= C) return;
    float out = 0.f;
    if (j < i) {
        const int r = plu_iperm[i];
        if (r < 0) out = __builtin_nanf("");
        else {
            const float *g = gw + (size_t)r * C, *u = upper + (size_t)j * C;
            double s = (double)g[j] * plu_diag(log_s, sign_s, j);
            for (int k = j + 1; k < C; ++k) s = fma((double)g[k], (double)u[k], s);
            out = (float)s;
        }
    }
    g_lower[(size_t)i * C + j] = out;
}

} // namespace

bool finc_plu_supported(int C) { return C >= 1 && C <= FINC_PLU_MAX_C; }

int finc_plu_compose_launch(const float *lower, const float *upper, const float *log_s, const float *sign_s, const int *perm, float *w,
                            float *w_inv, float *logdet, int C, hipStream_t st)
{
    if (!finc_plu_supported(C)) return FINC_ERR_UNSUPPORTED;
    const int per_row = (C + PLU_THREADS - 1) / PLU_THREADS;
    const int n_inv = w_inv ? (C + PLU_WAVES - 1) / PLU_WAVES : 0, n_w = w ? C * per_row : 0;
    const size_t lds = w_inv ? (size_t)C * PLU_LDS_PER_CHANNEL : 0;
    if (int e = finc_ensure_dynamic_lds((const void *)finc_plu_compose_kernel, lds)) return e;
    hipLaunchKernelGGL(finc_plu_compose_kernel, dim3((unsigned)(n_inv + n_w + (logdet ? 1 : 0))), dim3(PLU_THREADS), lds, st, lower, upper,
                       log_s, sign_s, perm, w, w_inv, logdet, C, n_inv, n_w);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

int finc_plu_compose_bwd_launch(const float *gw, const float *g_ld, const float *lower, const float *upper, const float *log_s,
                                const float *sign_s, const int *perm, float *g_lower, float *g_upper, float *g_log_s, int C, hipStream_t st)
{
    if (!finc_plu_supported(C)) return FINC_ERR_UNSUPPORTED;
    const int per_row = (C + PLU_THREADS - 1) / PLU_THREADS;
    const int n_up = (g_upper || g_log_s) ? C * per_row : 0, n_low = g_lower ? C * per_row : 0;
    hipLaunchKernelGGL(finc_plu_compose_bwd_kernel, dim3((unsigned)(n_up + n_low)), dim3(PLU_THREADS), (size_t)C * sizeof(int), st, gw,
                       g_ld, lower, upper, log_s, sign_s, perm, g_lower, g_upper, g_log_s, C, n_up);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

#endif /* FINC_PLU_H */
