// The element-wise monotone rational-quadratic spline with linear tails for gfx950 (included by finc_mix.hip behind finc_actnorm.h:
// same object file, same helpers).  fp32 only.
//
// Reference: layers/splines/rational_quadratic.py (Durkan et al. 2019) as layers/activations.py SplineActivation calls it.  There a
// call repeats the parameters to [B, C, H, W, K], gathers the in-range elements with boolean masks (a host synchronisation), asks
// torch.min(inputs) < left (another), asserts (discriminant >= 0).all() (a third) and runs two softmaxes, two cumsums and seven
// gathers over the inflated tensor.  Here the map is one read, a search over at most 17 knots, a few FMAs, divisions and two logs,
// and one write; nothing goes to the host, so the layer can be captured in a HIP graph.
//
// The kernels never see the unnormalised parameters.  They read a KNOT TABLE, knot-major: table[(a * (K + 1) + k) * P + p], a = 0
// cumwidths, 1 cumheights, 2 derivatives -- the three arrays of rational_quadratic.py:97-115, padded end derivatives included -- for
// the K + 1 knots k of table row p.  P = 1: one spline for every element (shared weights).  P = C * HW: one per position
// (individual_weights=True); consecutive lanes sit on consecutive positions, so every table load is coalesced.  Widths, heights and
// delta = heights / widths are differences and quotients of the knots, taken here.  2 <= K <= 16.
//
// The walk (both P): a workgroup is (block of 256 consecutive positions n of the C * HW, part q); a lane loads the 3 (K + 1) knots
// of ITS position once, keeps them in registers, and walks the images b = q, q + Q, ... -- the table is read once per position and
// part, not once per element.  With P = 1 every lane loads row 0 (one address per wave).  Activation accesses are dwords, coalesced
// over the lanes: a lane that kept four positions' tables would need 4 x 51 registers at K = 16.  Every index is checked against
// C * HW; nothing is read or written beyond a tensor.
// The knot arrays live in registers only: every loop over them is unrolled to the instantiation's capacity KB (8 or 16) and every
// index is a constant; the bin is the reference's -- the knots <= x counted, minus one (knot 0 is not counted instead), and the
// count capped at K - 1 so that x == right lands in the last bin -- and its six values are picked with one compare of the bin
// against each constant and six selects.  Slots beyond K hold +inf knots: never counted, never selected.  The ISA shows no scratch.
//
// direction +1 is :161-175.  direction -1 is :135-159 with root = 2c / (-b - sqrt(disc)); disc is CLAMPED at 0 before the square
// root: the reference asserts disc >= 0 on the host and would stop on a rounding-negative value, a kernel has no host round trip.
// The root is a position in the bin: it is CLAMPED to [0, 1] and x to [cw0, cw1] (spl_root; the reverse and the reverse's backward
// both use it).  A root of 1 + 1e-4 makes the log-det's d1 th^2 + 2 delta th (1 - th) + d0 (1 - th)^2 negative -- a NaN log q from a
// finite in-range input -- and puts x outside its bin.  The clamp is a backstop: the quadratic is solved from the NEARER knot (the
// upper half of a bin through the spline's mirror image), where c is small and b^2 - 4ac does not cancel as it does in fp32 one ulp
// from the far knot of a steep bin beside a flat one, and in whichever of 2c / (-b - sqrt) and (-b + sqrt) / 2a adds two numbers of
// one sign, so that x is monotone in y down to consecutive floats.
// Outside [-tail_bound, tail_bound], and for NaN, the output is the input's bits and the log-derivative is 0.
// logdet[b], when asked for, is the FORWARD map's log-det in either direction (in direction -1 at the recovered input: minus what the
// reference's inverse returns), summed in a fixed order: lanes in a butterfly, one partial per wave and image in the workspace,
// finc_coupling_reduce_kernel over an image's partials.  No atomics anywhere: the same inputs give the same bits.
#ifndef FINC_SPLINE_H
#define FINC_SPLINE_H

namespace {

constexpr int SPL_MIN_BINS = 2, SPL_MAX_BINS = 16;

template <int KB>
struct SplTable {
    float cw[KB + 1], ch[KB + 1], d[KB + 1];
};

// the knots of table row `row`; slots beyond K (and a lane beyond the tensor) get +inf knots and unit derivatives
template <int KB>
__device__ __forceinline__ void spl_load_table(SplTable<KB> &t, const float *__restrict__ table, size_t P, size_t row, int K, bool valid)
{
    const size_t a = (size_t)(K + 1) * P;
#pragma unroll
    for (int k = 0; k <= KB; ++k) {
        const bool in = valid && k <= K;
        const size_t o = (size_t)k * P + row;
        t.cw[k] = in ? table[o] : INFINITY;
        t.ch[k] = in ? table[a + o] : INFINITY;
        t.d[k] = in ? table[2 * a + o] : 1.f;
    }
}

struct SplBin {
    float cw0, cw1, ch0, ch1, d0, d1;
    int bin;
};

// the bin of v among the cumwidths (HEIGHTS: the cumheights): selects with constant indices, no indexed register array
template <int KB, bool HEIGHTS>
__device__ __forceinline__ SplBin spl_find(const SplTable<KB> &t, float v, int K)
{
    int count = 0;                                                   // inner knots <= v; knot K counts too and the minimum undoes it
#pragma unroll
    for (int j = 1; j <= KB; ++j) count += (HEIGHTS ? t.ch[j] : t.cw[j]) <= v ? 1 : 0;
    const int bin = min(count, K - 1);
    SplBin s{t.cw[0], t.cw[1], t.ch[0], t.ch[1], t.d[0], t.d[1], bin};
#pragma unroll
    for (int j = 1; j < KB; ++j) {
        const bool m = bin == j;
        s.cw0 = m ? t.cw[j] : s.cw0;
        s.cw1 = m ? t.cw[j + 1] : s.cw1;
        s.ch0 = m ? t.ch[j] : s.ch0;
        s.ch1 = m ? t.ch[j + 1] : s.ch1;
        s.d0 = m ? t.d[j] : s.d0;
        s.d1 = m ? t.d[j + 1] : s.d1;
    }
    return s;
}

// rational_quadratic.py:161-175.  (No contraction in the two maps: which products fuse into an FMA would otherwise depend on whether
// the instantiation also computes the log-det, and `reverse` and `reverse_with_logdet` are to return the same bits.)
__device__ __forceinline__ void spl_forward(const SplBin &s, float x, float &y, float &ld)
{
#pragma clang fp contract(off)
    const float w = s.cw1 - s.cw0, h = s.ch1 - s.ch0, delta = h / w;
    const float th = (x - s.cw0) / w, omt = 1.f - th, tm = th * omt;
    const float sd = s.d0 + s.d1 - 2.f * delta;
    const float num = h * (delta * th * th + s.d0 * tm), den = delta + sd * tm;
    y = s.ch0 + num / den;
    const float dnum = delta * delta * (s.d1 * th * th + 2.f * delta * tm + s.d0 * omt * omt);
    ld = logf(dnum) - 2.f * logf(den);
}

// rational_quadratic.py:135-159; ld is the forward map's log-derivative at the root (the reference returns its negative)
// the position in the bin at which the spline takes the value y (:135-148)
// Solved from the NEARER knot (the spline is its own mirror image under th -> 1 - th, d0 <-> d1, y - ch0 -> ch1 - y): `upper` says
// which, r is the distance from that knot in [0, 1] (clamped: see the header comment), the return value the position th.
__device__ __forceinline__ float spl_root(const SplBin &s, float y, bool &upper, float &r)
{
#pragma clang fp contract(off)
    const float w = s.cw1 - s.cw0, h = s.ch1 - s.ch0, delta = h / w;
    const float sd = s.d0 + s.d1 - 2.f * delta;
    upper = 2.f * (y - s.ch0) > h;
    const float dy = upper ? s.ch1 - y : y - s.ch0, da = upper ? s.d1 : s.d0;
    const float a = dy * sd + h * (delta - da), b = h * da - dy * sd, c = -delta * dy;
    const float disc = fmaxf(b * b - 4.f * a * c, 0.f);              // (the reference asserts disc >= 0 on the host instead)
    // the form that adds two numbers of one sign: the reference's for b >= 0; for b < 0 (a flat bin between large derivatives:
    // -b - sqrt cancels) the other one, and a > 0 there because a + b = h delta > 0
    const float sq = sqrtf(disc), num = b >= 0.f ? 2.f * c : sq - b, den = b >= 0.f ? -b - sq : 2.f * a;
    r = fminf(fmaxf(num / den, 0.f), 1.f);
    return upper ? 1.f - r : r;
}

__device__ __forceinline__ void spl_inverse(const SplBin &s, float y, float &x, float &ld)
{
#pragma clang fp contract(off)
    const float w = s.cw1 - s.cw0, h = s.ch1 - s.ch0, delta = h / w;
    const float sd = s.d0 + s.d1 - 2.f * delta;
    bool upper;
    float r;
    const float root = spl_root(s, y, upper, r);
    x = fminf(fmaxf(upper ? s.cw1 - r * w : r * w + s.cw0, s.cw0), s.cw1);   // (the rounded w + cw0 can pass the knot by half an ulp of w)
    const float omt = 1.f - root, tm = root * omt, den = delta + sd * tm;
    const float dnum = delta * delta * (s.d1 * root * root + 2.f * delta * tm + s.d0 * omt * omt);
    ld = logf(dnum) - 2.f * logf(den);
}

// Workgroup = (position block, part): blockIdx.x = block * Q + q.  part[b * npart + 4 * block + wave] = that wave's share of
// logdet[b] (zero for lanes beyond N).  y == x is allowed (a lane reads an element before it writes it, nobody else touches it).
template <int KB, int DIR, bool LOGDET>
__global__ __launch_bounds__(CPL_THREADS) void finc_spline_kernel(const float *x, const float *__restrict__ table, float *y,
                                                                  float *__restrict__ part, int B, int N, int P, int K, float tb, int Q,
                                                                  int npart)
{
    const int pb = (int)blockIdx.x / Q, q = (int)blockIdx.x - pb * Q;
    const int n = pb * CPL_THREADS + (int)threadIdx.x;
    const bool valid = n < N;
    SplTable<KB> t;
    spl_load_table<KB>(t, table, (size_t)P, P == 1 ? 0 : (size_t)n, K, valid);
    for (int b = q; b < B; b += Q) {
        float ld = 0.f;
        if (valid) {
            const size_t o = (size_t)b * N + n;
            const float v = x[o];
            float r = v;
            if (v >= -tb && v <= tb) {
                const SplBin s = spl_find<KB, (DIR < 0)>(t, v, K);
                if constexpr (DIR > 0) spl_forward(s, v, r, ld);
                else spl_inverse(s, v, r, ld);
            }
            y[o] = r;
        }
        if constexpr (LOGDET) {
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) ld += __shfl_xor(ld, k, 64);
            if ((threadIdx.x & 63) == 0) part[(size_t)b * npart + 4 * pb + (threadIdx.x >> 6)] = ld;
        }
    }
}

// The adjoint of one in-range element.  With w = cw1 - cw0, h = ch1 - ch0, delta = h / w, th = (x - cw0) / w, tm = th (1 - th),
// sd = d0 + d1 - 2 delta, r = delta th^2 + d0 tm, N = h r, D = delta + sd tm, q = d1 th^2 + 2 delta tm + d0 (1 - th)^2,
// dnum = delta^2 q:  y = ch0 + N / D,  f'(x) = dnum / D^2,  L = log f' = log dnum - 2 log D.
// FINC_GRAD_FWD: reverse-mode through those lines from (yb, Lb) = (grad_y, grad_logdet): gk[] = the gradients of cw0, cw1, ch0, ch1,
// d0, d1; returns grad_x = grad_y f'(x) + grad_logdet dL/dx.
// FINC_GRAD_REV: x = f^-1(y) was the OUTPUT, `g` the gradient that reaches it, Lb that of the log-det L(x) the reverse returned.
// dx/dy = 1 / f', dx/dtheta = -(df/dtheta) / f':  with u = (g + Lb dL/dx) / f'(x) the gradient of y is u and the table's is the
// forward adjoint at (yb, Lb) = (-u, Lb).
// `th` is the position in the bin, (x - cw0) / w.  The reverse mode is handed the ROOT the quadratic gives for the reverse's input y,
// not that quotient of the stored output: in a narrow bin x - cw0 cancels, and dL/dx, which jumps from bin to bin and scales with
// 1 / w, loses the digits (measured at 16 bins on [-3, 3]: 1.6e-5 of the largest gradient from the stored x, against 1.7e-7 for
// PyTorch's fp32 lines, which differentiate the root).
template <int MODE>
__device__ __forceinline__ float spl_adjoint(const SplBin &s, float th, float omt, float g, float Lb, float (&gk)[6])
{
    const float w = s.cw1 - s.cw0, h = s.ch1 - s.ch0, iw = 1.f / w, delta = h * iw;
    const float tm = th * omt;
    // 1 - 2 th; the reverse mode is handed 1 - th as the root gave it (solved from the upper knot it IS the root: 1 - (1 - r) would
    // round a root of 1e-7 to a multiple of 6e-8), and takes the difference from that
    const float omtt = MODE == FINC_GRAD_REV ? omt - th : 1.f - 2.f * th;
    const float sd = s.d0 + s.d1 - 2.f * delta;
    const float r = delta * th * th + s.d0 * tm, N = h * r, D = delta + sd * tm;
    const float q = s.d1 * th * th + 2.f * delta * tm + s.d0 * omt * omt, dnum = delta * delta * q;
    const float iD = 1.f / D, idn = 1.f / dnum;
    float yb = g, out = 0.f;
    if constexpr (MODE == FINC_GRAD_REV) {
        const float lth = idn * delta * delta * (2.f * s.d1 * th - 2.f * s.d0 * omt) + (2.f * delta * delta * delta * idn - 2.f * sd * iD) * omtt;
        out = (g + Lb * lth * iw) * (D * D * idn);
        yb = -out;
    }
    const float Nb = yb * iD, Db = -yb * N * iD * iD - 2.f * Lb * iD, dnb = Lb * idn;
    float deltab = dnb * (2.f * delta * q + 2.f * delta * delta * tm) + Db;
    const float qb = dnb * delta * delta;
    float d1b = qb * th * th, d0b = qb * omt * omt;
    float thb = qb * (2.f * s.d1 * th - 2.f * s.d0 * omt), tmb = qb * 2.f * delta + Db * sd;
    const float sb = Db * tm;
    d0b += sb;
    d1b += sb;
    deltab -= 2.f * sb;
    float hb = Nb * r;
    const float rb = Nb * h;
    if constexpr (MODE == FINC_GRAD_REV) {
        // dy/ddelta = h th^2 / D - N (1 - 2 tm) / D^2 = h tm (d1 th^2 - d0 (1 - th)^2) / D^2: the two terms of the left form are equal to
        // tm, and yb = -u is the size of dL/dx (1e3 in a steep bin) -- the log-det's share of Db stays as it was
        const float DbL = -2.f * Lb * iD;
        deltab = dnb * (2.f * delta * q + 2.f * delta * delta * tm) + DbL - 2.f * DbL * tm +
                 yb * h * tm * (s.d1 * th * th - s.d0 * omt * omt) * iD * iD;
    } else {
        deltab += rb * th * th;
    }
    thb += rb * 2.f * delta * th;
    d0b += rb * tm;
    tmb += rb * s.d0;
    thb += tmb * omtt;
    // (yb f' + Lb dL/dx at yb = -u is -g exactly; summed from its terms it carries the rounding of Lb dL/dx)
    if constexpr (MODE == FINC_GRAD_REV) thb = -g * w;
    hb += deltab * iw;
    const float xb = thb * iw, wb = -(deltab * delta + thb * th) * iw;
    // cw0's: -xb - wb = (deltab delta - thb (1 - th)) / w; near the upper knot the two terms of the left form are equal to 1 - th
    gk[0] = MODE == FINC_GRAD_REV ? (deltab * delta - thb * omt) * iw : -xb - wb;
    gk[1] = wb;
    gk[2] = yb - hb;
    gk[3] = hb;
    gk[4] = d0b;
    gk[5] = d1b;
    if constexpr (MODE == FINC_GRAD_FWD) out = xb;
    return out;
}

// Where the sum of table entry t (of T) lands for finc_coupling_reduce_kernel's pair mode (even outputs to out_a, odd ones to
// out_b): the first Ta = ceil(T / 2) entries are the even outputs, the rest the odd ones, with out_a = grad_table, out_b = grad_table + Ta.
__device__ __forceinline__ size_t spl_output(size_t t, size_t Ta) { return t < Ta ? 2 * t : 2 * (t - Ta) + 1; }

// Every backward of the spline is ONE body, spl_grad<KB, MODE> (FincGradMode), on the walk of finc_spline_kernel:
//   FINC_GRAD_FWD  of direction +1 from its saved INPUT x: grad_x = grad_y f'(x) + grad_logdet[b] dL/dx.
//   FINC_GRAD_REV  of direction -1 from its saved INPUT (`x` is then the reverse's input y; the bin is searched among the cumheights
//                  and the position in it is the quadratic's root, see spl_adjoint): the gradient of that input, with grad_logdet when
//                  the reverse was asked for its log-det.
// gy, gld, gx may be nullptr (zeros / not written).  An element contributes to its own bin's two knots per array only; a tail element
// (and a NaN) passes gy through and contributes nothing.  grad_table: a lane sums its position's 3 (K + 1) entries over its images in
// order.  P > 1: the lane's sums go to part[spl_output(t) * Q + q] -- or, with Q == 1 (`direct`), straight to grad_table[t]: they
// are the whole fixed-order sum already.  P == 1: the workgroup's lanes meet (cpl_block_sum) and thread 0 writes
// part[spl_output(t) * gridDim.x + blockIdx.x].  gx == gy is allowed.
template <int KB, int MODE>
__device__ __forceinline__ void spl_grad(const float *gy, const float *__restrict__ gld, const float *x, const float *__restrict__ table,
                                         float *gx, float *__restrict__ part, float *__restrict__ gt, int B, int N, int P, int K, float tb,
                                         int Q, int sums)
{
    const int pb = (int)blockIdx.x / Q, q = (int)blockIdx.x - pb * Q;
    const int n = pb * CPL_THREADS + (int)threadIdx.x;
    const bool valid = n < N;
    SplTable<KB> t;
    spl_load_table<KB>(t, table, (size_t)P, P == 1 ? 0 : (size_t)n, K, valid);
    float acc[3 * (KB + 1)];
#pragma unroll
    for (int k = 0; k < 3 * (KB + 1); ++k) acc[k] = 0.f;
    if (valid) {
        for (int b = q; b < B; b += Q) {
            const size_t o = (size_t)b * N + n;
            const float v = x[o], g = gy ? gy[o] : 0.f, Lb = gld ? gld[b] : 0.f;
            float out = g;
            if (v >= -tb && v <= tb) {
                const SplBin s = spl_find<KB, MODE == FINC_GRAD_REV>(t, v, K);
                float gk[6];
                float th, omt;
                if constexpr (MODE == FINC_GRAD_REV) {
                    bool upper;
                    float r;
                    th = spl_root(s, v, upper, r);
                    omt = upper ? r : 1.f - r;
                } else {
                    th = (v - s.cw0) / (s.cw1 - s.cw0);
                    omt = 1.f - th;
                }
                out = spl_adjoint<MODE>(s, th, omt, g, Lb, gk);
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const bool m = s.bin == j;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        acc[a * (KB + 1) + j] += m ? gk[2 * a] : 0.f;
                        acc[a * (KB + 1) + j + 1] += m ? gk[2 * a + 1] : 0.f;
                    }
                }
            }
            if (gx) gx[o] = out;
        }
    }
    if (!sums) return;
    const size_t T = (size_t)3 * (K + 1) * P, Ta = (T + 1) / 2;
    if (P == 1) {
        __shared__ float sm[3 * (KB + 1)][4];
        cpl_block_sum<3 * (KB + 1)>(acc, sm);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int k = 0; k <= KB; ++k)
                    if (k <= K) part[spl_output((size_t)(a * (K + 1) + k), Ta) * gridDim.x + blockIdx.x] = acc[a * (KB + 1) + k];
        }
    } else if (valid) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k <= KB; ++k)
                if (k <= K) {
                    const size_t e = (size_t)(a * (K + 1) + k) * P + n;
                    if (Q == 1) gt[e] = acc[a * (KB + 1) + k];
                    else part[spl_output(e, Ta) * Q + q] = acc[a * (KB + 1) + k];
                }
    }
}

template <int KB>
__global__ __launch_bounds__(CPL_THREADS) void finc_spline_bwd_kernel(const float *gy, const float *__restrict__ gld,
                                                                      const float *__restrict__ x, const float *__restrict__ table,
                                                                      float *gx, float *__restrict__ part, float *__restrict__ gt, int B,
                                                                      int N, int P, int K, float tb, int Q, int sums)
{
    spl_grad<KB, FINC_GRAD_FWD>(gy, gld, x, table, gx, part, gt, B, N, P, K, tb, Q, sums);
}

template <int KB>
__global__ __launch_bounds__(CPL_THREADS) void finc_spline_rev_bwd_kernel(const float *gy, const float *__restrict__ gld,
                                                                          const float *__restrict__ x, const float *__restrict__ table,
                                                                          float *gx, float *__restrict__ part, float *__restrict__ gt, int B,
                                                                          int N, int P, int K, float tb, int Q, int sums)
{
    spl_grad<KB, FINC_GRAD_REV>(gy, gld, x, table, gx, part, gt, B, N, P, K, tb, Q, sums);
}

} // namespace

// The launch of every spline kernel: `blocks` blocks of 256 positions are the outer units, and a block's 256 * B thread items (one
// per position and image) are shared by Q = cpl_parts parts -- a lane of part q walks the images q, q + Q, ...  Q = 0: the
// dimensions do not fit (FINC_ERR_BAD_DIMS).
struct SplPlan {
    int N, blocks, Q;
};
inline SplPlan spl_plan(int B, int C, int HW)
{
    if ((size_t)C * HW * 4 >= ((size_t)1 << 31)) return SplPlan{0, 0, 0};
    const int N = C * HW, blocks = (N + CPL_THREADS - 1) / CPL_THREADS;
    return SplPlan{N, blocks, cpl_parts((long long)B * CPL_THREADS, blocks)};
}

// floats: the log-det's partials (one per wave and image) or grad_table's (Q per entry; for P == 1 one per workgroup and entry)
size_t finc_spline_workspace_floats(int B, int C, int HW, int K, int P)
{
    const SplPlan p = spl_plan(B, C, HW);
    if (!p.Q) return 0;
    const size_t logdet = (size_t)B * p.blocks * 4, T = (size_t)3 * (K + 1) * (P == 1 ? 1 : (size_t)p.N);
    const size_t grads = T * (P == 1 ? (size_t)p.blocks * p.Q : (size_t)p.Q);
    return logdet > grads ? logdet : grads;
}

int finc_spline_launch(const float *x, const float *table, int P, int K, float tb, int direction, float *y, float *logdet, int B, int C,
                       int HW, float *ws, hipStream_t st)
{
    const SplPlan p = spl_plan(B, C, HW);
    if (!p.Q) return FINC_ERR_BAD_DIMS;
    const int form = (K > 8 ? 4 : 0) + (direction > 0 ? 2 : 0) + (logdet ? 1 : 0);
    using Kernel = void (*)(const float *, const float *, float *, float *, int, int, int, int, float, int, int);
    static const Kernel kernels[8] = {
        finc_spline_kernel<8, -1, false>,  finc_spline_kernel<8, -1, true>,  finc_spline_kernel<8, 1, false>,  finc_spline_kernel<8, 1, true>,
        finc_spline_kernel<16, -1, false>, finc_spline_kernel<16, -1, true>, finc_spline_kernel<16, 1, false>, finc_spline_kernel<16, 1, true>};
    const int npart = 4 * p.blocks;
    hipLaunchKernelGGL(kernels[form], dim3((unsigned)((long long)p.blocks * p.Q)), dim3(CPL_THREADS), 0, st, x, table, y, ws, B, p.N, P, K, tb,
                       p.Q, npart);
    FINC_CHECK_LAUNCH();
    if (logdet) {
        hipLaunchKernelGGL(finc_coupling_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float *)ws, npart, logdet, (float *)nullptr, 0);
        FINC_CHECK_LAUNCH();
    }
    return FINC_OK;
}

// x: the INPUT of the pass that is differentiated, the forward's (FINC_GRAD_FWD) or the reverse's (FINC_GRAD_REV)
int finc_spline_grad_launch(FincGradMode mode, const float *gy, const float *gld, const float *x, const float *table, int P, int K, float tb,
                            float *gx, float *gt, int B, int C, int HW, float *ws, hipStream_t st)
{
    const SplPlan p = spl_plan(B, C, HW);
    if (!p.Q) return FINC_ERR_BAD_DIMS;
    const size_t T = (size_t)3 * (K + 1) * P, Ta = (T + 1) / 2;
    if (gt && T >= ((size_t)1 << 31)) return FINC_ERR_BAD_DIMS;        // (the reduce's grid: one wave per entry)
    const bool rev = mode == FINC_GRAD_REV;
    const auto kernel = K > 8 ? (rev ? finc_spline_rev_bwd_kernel<16> : finc_spline_bwd_kernel<16>)
                              : (rev ? finc_spline_rev_bwd_kernel<8> : finc_spline_bwd_kernel<8>);
    const unsigned grid = (unsigned)((long long)p.blocks * p.Q);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(CPL_THREADS), 0, st, gy, gld, x, table, gx, ws, gt, B, p.N, P, K, tb, p.Q, gt ? 1 : 0);
    FINC_CHECK_LAUNCH();
    if (!gt || (P != 1 && p.Q == 1)) return FINC_OK;
    return cpl_reduce_pairs(1, ws, (int)T, P == 1 ? (int)grid : p.Q, gt, gt + Ta, st);
}

#endif /* FINC_SPLINE_H */
