// Backward through the unit's INVERSE for gfx950 (included by finc_mix.hip behind finc_actnorm.h: same object file, same helpers).
//
// x = inverse(z) solves M x = z, M = L_blk + N (L: the unit lower triangular tap of the pixel itself, canonical tap [KH-1][KW-1];
// N: every other tap, on earlier pixels).  For an upstream gradient g_x:  grad_z = y = M^-T g_x,  grad_w = -(the forward's weight
// gradient at input x and grad_output y).  M^T reads the opposite corner (orientation bits complemented) with transposed channel
// matrices; its corner tap L^T is UPPER triangular, which the inverse kernels do not take as their z-term, so it is factored out on the
// right:
//     M^T = (I + sum_t S_t T_t) L_blk^T,   T_t = W_t^T L^-T      =>      v = inverse(g_x; bank w_adj, ~orient),   y = blockdiag(L^-T) v
//     w_adj[g][i][o][kh][kw] = sum_k w_canon[g][k][i][kh][kw] * Linv_g[o][k]   (every tap but the corner),   corner tap = I
// -- a valid canonical bank, solved by every inverse kernel as it stands.  Here:
//   * finc_adjoint_weights_kernel   w_adj and lead_t = blockdiag(Linv_g^T) ([C][C], row = output channel) from w_canon.  All math in
//                                   fp64, rounded to fp32 once.  One thread per COLUMN of the triangular solve L a = b: b = column i
//                                   of tap t (a = w_adj[g][i][:][t]) or a unit vector e_j (a = column j of Linv = row j of lead_t).  A
//                                   workgroup keeps its threads' columns in LDS ([row][thread]: no bank conflicts); the pack kernels
//                                   keep all of Linv there (finc_mfma.hip pack_kernel), which at Cq = 256 would be 512 KB in fp64 --
//                                   a column at a time is Cq * 8 bytes per thread whatever the bank, and nothing else is needed.
//   * finc_lead_grouped_kernel      y = blockdiag(L^-T) v IN PLACE for the channel counts finc_mix_kernel has no instantiation for:
//                                   a thread owns V consecutive pixels of one (image, group) and walks the group's unit upper
//                                   triangular block row by row (row o' reads channels o >= o', so ascending rows never read what
//                                   they wrote).  Coalesced along pixels; V = 4 under the per-pixel layers' rule (cpl_wide), else 1.
//   * finc_negate_kernel            the sign of the weight gradient, on the [C][Cq][KH][KW] result (0 stays +0: the masked entries).
#ifndef FINC_ADJOINT_H
#define FINC_ADJOINT_H

namespace {

constexpr int ADJ_LDS_BYTES = 64 * 1024;

// grid (panels, G), blockDim.x = P threads, LDS Cq * P doubles.  Column ids of a group: [0, Cq * (NT-1)) = (tap t != corner, bank
// column i), then Cq unit vectors.  Panel 0 of a group also writes what no column does: the corner tap of w_adj (the identity) and the
// zeros of lead_t's rows outside the group's diagonal block.
__global__ void finc_adjoint_weights_kernel(const float *__restrict__ wc, float *__restrict__ w_adj, float *__restrict__ lead_t, int G,
                                            int Cq, int KH, int KW)
{
    extern __shared__ __attribute__((aligned(16))) double adj_col[];   // [r * P + p]
    const int P = (int)blockDim.x, p = (int)threadIdx.x, g = (int)blockIdx.y;
    const int NT = KH * KW, corner = NT - 1, C = G * Cq;
    const int ntap = Cq * (NT - 1), ncol = ntap + Cq;
    const float *wg = wc + (size_t)g * Cq * Cq * NT;
    float *ag = w_adj + (size_t)g * Cq * Cq * NT;
    const int col = (int)blockIdx.x * P + p;
    if (col < ncol) {
        const bool unit = col >= ntap;
        const int t = unit ? 0 : col / Cq, i = unit ? col - ntap : col - t * Cq;   // t: index among the taps before the corner
        for (int r = 0; r < Cq; ++r) {
            double v;
            if (unit) v = r == i ? 1.0 : 0.0;
            else v = (double)wg[((size_t)r * Cq + i) * NT + t];
            // (a unit vector's solution is zero above its own row)
            for (int k = unit ? i : 0; k < r; ++k) v -= (double)wg[((size_t)r * Cq + k) * NT + corner] * adj_col[k * P + p];
            adj_col[r * P + p] = v;
            if (unit) lead_t[(size_t)(g * Cq + i) * C + g * Cq + r] = (float)v;      // lead_t[o'][o] = Linv[o][o']
            else ag[((size_t)i * Cq + r) * NT + t] = (float)v;                        // w_adj[i][o][t] = sum_k W_t[k][i] Linv[o][k]
        }
    }
    if (blockIdx.x == 0) {
        for (int e = p; e < Cq * Cq; e += P) ag[(size_t)e * NT + corner] = (e / Cq == e % Cq) ? 1.f : 0.f;
        for (int e = p; e < Cq * (C - Cq); e += P) {
            const int row = e / (C - Cq), c = e - row * (C - Cq);
            lead_t[(size_t)(g * Cq + row) * C + (c < g * Cq ? c : c + Cq)] = 0.f;
        }
    }
}

// Grid-stride over the B * G * HW / V items; item = (image, group, V pixels).  `v` is read and written by its owner alone.
template <int V>
__global__ __launch_bounds__(CPL_THREADS) void finc_lead_grouped_kernel(float *v, const float *__restrict__ lead_t, int G, int Cq, int HW,
                                                                        int nv, unsigned items)
{
    const int C = G * Cq;
    for (unsigned idx = blockIdx.x * CPL_THREADS + threadIdx.x; idx < items; idx += gridDim.x * CPL_THREADS) {
        const unsigned bg = idx / (unsigned)nv, px = (idx - bg * (unsigned)nv) * V;
        const int g = (int)(bg % (unsigned)G);
        float *base = v + (size_t)bg * Cq * HW + px;                 // channel 0 of the group (NCHW: groups are consecutive channels)
        const float *lt = lead_t + (size_t)g * Cq * C + g * Cq;      // the group's diagonal block
        for (int r = 0; r < Cq; ++r) {
            float acc[V], in[V];
            cpl_load<V>(acc, base + (size_t)r * HW);                 // the unit diagonal
            for (int o = r + 1; o < Cq; ++o) {
                const float m = lt[(size_t)r * C + o];
                cpl_load<V>(in, base + (size_t)o * HW);
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] = fmaf(m, in[e], acc[e]);
            }
            cpl_store<V>(base + (size_t)r * HW, acc);
        }
    }
}

__global__ void finc_negate_kernel(float *p, unsigned n)
{
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x) p[idx] = 0.f - p[idx];
}

} // namespace

int finc_adjoint_weights_launch(const float *wc, float *w_adj, float *lead_t, int G, int Cq, int KH, int KW, hipStream_t st)
{
    // as many columns per workgroup as 64 KiB of LDS hold in fp64, at most 64, whole waves' worth where the bank allows it
    int P = ADJ_LDS_BYTES / (Cq * (int)sizeof(double));
    P = P >= 64 ? 64 : P >= 32 ? 32 : P;
    if (P < 1) return FINC_ERR_BAD_DIMS;
    const size_t lds = (size_t)Cq * P * sizeof(double);
    const int ncol = Cq * KH * KW;                                    // Cq * (NT - 1) tap columns + Cq unit vectors
    if (int e = finc_ensure_dynamic_lds((const void *)finc_adjoint_weights_kernel, lds)) return e;
    hipLaunchKernelGGL(finc_adjoint_weights_kernel, dim3((unsigned)((ncol + P - 1) / P), (unsigned)G), dim3((unsigned)P), lds, st, wc, w_adj,
                       lead_t, G, Cq, KH, KW);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

// y = blockdiag(L^-T) v in place: one streaming MFMA pass where the channel count has a mix instantiation, the grouped kernel otherwise
int finc_lead_launch(float *v, const float *lead_t, int B, int G, int Cq, int HW, hipStream_t st)
{
    const int C = G * Cq;
    if (finc_mix_supported(C)) return finc_mix_launch(v, lead_t, nullptr, v, B, C, HW, st);
    const CplRowPlan rp = cpl_row_plan((long long)B * G, HW, 4, (uintptr_t)v);      // a row: the V pixels of one (image, group)
    if (!rp.wgs) return FINC_ERR_BAD_DIMS;
    const bool wide = rp.wide;
    const int nv = rp.nv;
    const long long items = rp.items;
    const unsigned wgs = rp.wgs;
    hipLaunchKernelGGL(wide ? finc_lead_grouped_kernel<4> : finc_lead_grouped_kernel<1>, dim3(wgs), dim3(CPL_THREADS), 0, st, v, lead_t, G, Cq,
                       HW, nv, (unsigned)items);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

// the negate's grid: one pass of 256 threads per workgroup, at most 1024 workgroups, grid-stride beyond (n < 2^31)
static inline unsigned adj_negate_grid(size_t n)
{
    const size_t wgs = (n + 255) / 256;
    return (unsigned)(wgs > 1024 ? 1024 : wgs);
}

int finc_negate_launch(float *p, size_t n, hipStream_t st)
{
    if (n == 0) return FINC_OK;
    if (n >= ((size_t)1 << 31)) return FINC_ERR_BAD_DIMS;
    const unsigned wgs = adj_negate_grid(n);
    hipLaunchKernelGGL(finc_negate_kernel, dim3(wgs), dim3(256), 0, st, p, (unsigned)n);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

#endif /* FINC_ADJOINT_H */
