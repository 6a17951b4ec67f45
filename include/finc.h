/*
 * finc.h -- C ABI of the MI355X-native FInC Flow hot path (libfinc_hip.so).
 *
 * This is the drop-in boundary.  It replaces the reference's one native entry
 * point
 *
 *     m.def("inverse", &cinc_inverse_level2)            cinc_cuda_level2.cpp:30-32
 *     std::vector<Tensor> cinc_inverse_level2(Tensor input  [B,C,H,W],
 *                                             Tensor kernel [G*Cq,Cq,KH,KW],
 *                                             Tensor output [B,C,H,W])   :19-28
 *
 * and the cuDNN convolution behind PaddedConv2d.forward (layers/conv.py:102-107)
 * with plain-pointer functions: no torch types, no global state besides a
 * per-process table of (device, kernel) attributes and one 4-byte flag word per
 * device (finc_check_invariant_f32).  Every function is stream-ordered
 * and asynchronous unless its comment says otherwise; every pointer is a
 * DEVICE pointer unless its name starts with `h_`.
 *
 * Data layout (the reference's own, fastflow.py:78-100):
 *   activations  fp32 NCHW contiguous, C = G*Cq; group g owns channels
 *                [g*Cq, (g+1)*Cq).
 *   w_canon      fp32 [G*Cq][Cq][KH][KW], TL-canonical -- exactly the `kernel`
 *                tensor of the reference op (fastflow.py:79-84).
 *   w_stored     the same shape in state-dict form: each group's bank flipped
 *                per its order (layers/conv.py:72-79).
 *   orient       2 bits per group g at bits [2g, 2g+1]: bit0 = W-flipped (TR),
 *                bit1 = H-flipped (BL), both = BR.  FastFlowUnit = 0xE4
 *                (TL,TR,BL,BR; fastflow.py:24-27).  The reference flips the
 *                activation chunks in PyTorch around the op (fastflow.py:85-100);
 *                here the kernels index the flipped pixel directly, so the
 *                caller passes the un-flipped tensors.
 *
 * Invariant (layers/conv.py:63-70): w_canon[c][c][KH-1][KW-1] == 1 and
 * w_canon[c][kc>c][KH-1][KW-1] == 0.  finc_check_invariant_f32 verifies it.
 */
#ifndef FINC_H
#define FINC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *finc_stream_t; /* a hipStream_t; NULL = the default stream */

enum finc_status {
    FINC_OK = 0,
    FINC_ERR_NULL_POINTER = 1,
    FINC_ERR_BAD_DIMS = 2,     /* non-positive dims, G > 16, Cq > FINC_MAX_CQ ... */
    FINC_ERR_UNSUPPORTED = 3,  /* the requested algo has no instantiation for this shape */
    FINC_ERR_WORKSPACE = 4,    /* workspace NULL or smaller than finc_workspace_bytes() */
    FINC_ERR_LAUNCH = 5,       /* a HIP call failed; see finc_last_hip_error() */
    FINC_ERR_INVARIANT = 6,    /* unit-lower-triangular corner tap violated */
    FINC_ERR_ALIGNMENT = 7     /* a pointer is not aligned to its element: 4 bytes (fp32), 8 (fp64), 2 (bf16 bits) */
};

enum finc_algo {
    FINC_ALGO_AUTO = 0,   /* fastest kernel that supports the shape */
    FINC_ALGO_STRICT = 1, /* reference visitation + term order; inverse is bit-exact with the
                             fp32 CPU restatement (cinc_cuda_kernel_level2.cu:59-72)        */
    FINC_ALGO_MFMA = 2    /* wavefront-per-(image,group) MFMA kernel; FINC_ERR_UNSUPPORTED
                             when the shape has no instantiation                             */
};

#define FINC_MAX_GROUPS 16
#define FINC_MAX_CQ 256
#define FINC_ORIENT_FASTFLOW 0xE4u

int finc_version(void);
/* Bit mask of the measurement knobs (csrc/finc_experiment.h: ablations, stamps, reduced tables ...) the library was built
 * with.  0 for a product build; anything else computes wrong results by design and must never be shipped or benchmarked. */
unsigned finc_build_flags(void);
const char *finc_status_string(int status);
/* hipGetErrorString of the last failing HIP call on this thread (never NULL). */
const char *finc_last_hip_error(void);

/* Replaces fastflow.py:79-84 (four torch.flip + cat).  w_stored -> w_canon; may not alias. */
int finc_canonicalize_weights_f32(const float *w_stored, float *w_canon, int G, int Cq, int KH, int KW,
                                  unsigned orient, finc_stream_t stream);

/* SYNCHRONOUS (one 4-byte D2H copy on `stream`; the device flag word is allocated once per device and kept).
 * Returns FINC_OK or FINC_ERR_INVARIANT.  Call once per weight version, not per step. */
int finc_check_invariant_f32(const float *w_canon, int G, int Cq, int KH, int KW, finc_stream_t stream);

/* Scratch the AUTO/MFMA algos need (packed filter fragments); 0 is never returned. */
size_t finc_workspace_bytes(int G, int Cq, int KH, int KW);

/*
 * Workspace finc_inverse_f32 can use for this problem: finc_workspace_bytes(), plus -- when W is not a multiple
 * of 4, which the MFMA inverse cannot stream -- room for a zero-padded copy of z and of x (row pitch rounded up to
 * 8 floats).  With at least this much workspace FINC_ALGO_AUTO solves the padded copy (exact, two extra copies);
 * with less it falls back to FINC_ALGO_STRICT for such widths.  The reference has no counterpart: its kernel
 * takes any width (cinc_cuda_kernel_level2.cu:49-56).
 */
size_t finc_inverse_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW);

/* Which algo FINC_ALGO_AUTO resolves to for this shape (FINC_ALGO_STRICT or FINC_ALGO_MFMA). */
int finc_inverse_algo_for(int Cq, int H, int W, int KH, int KW);
int finc_forward_algo_for(int Cq, int H, int W, int KH, int KW);

/*
 * x = inverse(z): the reference op `inverse(input=z, kernel=w_canon, output=x)`
 * (cinc_cuda_level2.cpp:19-28 -> cinc_cuda_kernel_level2.cu:77-136) including the
 * chunk flips FastFlowUnit.reverse_level2 wraps around it (fastflow.py:85-100).
 * Unlike the reference: `x` need not be zero-filled, B is not limited to 1024,
 * one launch per call instead of (H+W-1)*Cq launches + device syncs.
 * z and x may not alias.
 */
int finc_inverse_f32(const float *z, const float *w_canon, float *x, int B, int G, int Cq, int H, int W,
                     int KH, int KW, unsigned orient, int algo, void *workspace, size_t workspace_bytes,
                     finc_stream_t stream);

/*
 * z = forward(x): FastFlowUnit.forward (fastflow.py:31-50) = per group
 * F.pad on one corner + bias-free cross-correlation (layers/conv.py:102-107),
 * without the pad/chunk/cat copies.  logdet of this layer is identically 0
 * (layers/conv.py:106,220-221), so nothing is written for it.
 * x and z may not alias.
 */
int finc_forward_f32(const float *x, const float *w_canon, float *z, int B, int G, int Cq, int H, int W,
                     int KH, int KW, unsigned orient, int algo, void *workspace, size_t workspace_bytes,
                     finc_stream_t stream);

/*
 * Split form of the two calls above for callers that run many steps on one
 * weight version (sampling): pack once, then launch with the packed buffer.
 * `packed` must hold finc_workspace_bytes() bytes.
 */
int finc_pack_inverse_weights_f32(const float *w_canon, void *packed, int G, int Cq, int KH, int KW,
                                  finc_stream_t stream);
int finc_pack_forward_weights_f32(const float *w_canon, void *packed, int G, int Cq, int KH, int KW,
                                  finc_stream_t stream);
/*
 * SURVEY 8 f3 -- the per-channel affine layer that precedes the unit in the reverse chain folded into the bank:
 * with fragments packed by this call, finc_inverse_packed_f32(y, ...) returns inverse(scale * y + shift), i.e.
 * FastFlowUnit.reverse(ActNorm.reverse(y)) (layers/actnorm.py:39-52: scale = exp(log_scale), shift = translation;
 * called back to back by FlowSequential.sample, layers/flowsequential.py:89-115) in the one launch and at the
 * per-step cost of the plain inverse: Linv*diag(scale) replaces Linv as the z-term and Linv*shift is the
 * accumulators' initial value.  scale / shift: [G*Cq] device floats, either may be NULL (identity).
 * FINC_ERR_UNSUPPORTED when the shape has no MFMA instantiation (there is no strict twin of this call).
 * A SHIFT cannot ride on every kernel: the big banks (64 < Cq <= 96) refuse it here (FINC_ERR_UNSUPPORTED), and the
 * 33..64-channel banks carry it on every map except those too wide for the wavefront kernel's forms (Cq = 50 at 256
 * columns ...), which run on the big-bank kernel.  Packing does not know the map, so ask first:
 * finc_inverse_affine_supported(B, G, Cq, H, W, KH, KW) == 1 iff finc_inverse_packed_f32 on THIS problem set accepts a
 * bank packed with a shift.  A launch that does not (a wide map on a shift-carrying bank) returns FINC_ERR_UNSUPPORTED --
 * it never computes with a partial bank -- and the caller runs the affine layer as its own launch.
 */
int finc_inverse_affine_supported(int B, int G, int Cq, int H, int W, int KH, int KW);
int finc_pack_inverse_weights_affine_f32(const float *w_canon, const float *scale, const float *shift, void *packed,
                                         int G, int Cq, int KH, int KW, finc_stream_t stream);
/*
 * The same fold for the forward direction: with fragments packed by this call, finc_forward_packed_f32(x, ...) returns
 * scale * forward(x) + shift per output channel, i.e. ActNorm.forward(FastFlowUnit.forward(x)) (layers/actnorm.py:39-46:
 * scale = exp(-log_scale), shift = -translation * exp(-log_scale); FlowSequential.forward calls them back to back,
 * layers/flowsequential.py:21-44) in the one launch: the filter rows carry the scale, the accumulators start from the
 * shift.  The layer's log-determinant is the caller's business (it does not depend on the data).
 */
int finc_pack_forward_weights_affine_f32(const float *w_canon, const float *scale, const float *shift, void *packed,
                                         int G, int Cq, int KH, int KW, finc_stream_t stream);
int finc_inverse_packed_f32(const float *z, const void *packed, float *x, int B, int G, int Cq, int H, int W,
                            int KH, int KW, unsigned orient, finc_stream_t stream);
int finc_forward_packed_f32(const float *x, const void *packed, float *z, int B, int G, int Cq, int H, int W,
                            int KH, int KW, unsigned orient, finc_stream_t stream);
/*
 * SURVEY 8 f3, second half -- the inverse of a unit whose input the caller has ALREADY multiplied by blockdiag(Linv_g),
 * Linv_g = inverse(w_canon[g][:, :, KH-1, KW-1]) (the unit lower triangular tap of the pixel itself, layers/conv.py:63-70):
 * in the reverse chain of a flow step (fastflow/fastflow_cifar.py:46-55: ... Conv1x1.reverse -> [ActNorm.reverse] ->
 * FastFlowUnit.reverse) the channel mix in front of the unit is a dense C x C matrix product per pixel anyway, so
 *     zp = finc_mix_f32(u, blockdiag(Linv) * diag(scale) * inverse(W), blockdiag(Linv) * shift)
 * costs what the plain mix costs, and the unit's inverse starts every pixel from what it reads instead of spending 15 of
 * its 162 MFMAs (c3) on Linv * z.  `packed` is the plain bank of finc_pack_inverse_weights_f32 (its z-term and folded
 * shift are not used).  Exists for the problem sets that run the helper-wave form (a full chip; W % 16 == 0):
 * finc_inverse_premultiplied_supported() == 1, else FINC_ERR_UNSUPPORTED and the caller keeps the two plain calls.
 */
int finc_inverse_premultiplied_supported(int B, int G, int Cq, int H, int W, int KH, int KW);
int finc_inverse_packed_premultiplied_f32(const float *zp, const void *packed, float *x, int B, int G, int Cq, int H,
                                          int W, int KH, int KW, unsigned orient, finc_stream_t stream);

/*
 * Backward of the forward conv (replaces autograd through cuDNN,
 * layers/conv.py:105, plus PaddedConv2d.reset_gradients, layers/conv.py:98-99).
 *   grad_x = conv_transpose(grad_z, w)      (same corner geometry, mirrored)
 *   grad_w_canon[o][i][kh][kw] = sum_{b,h,w} grad_z[b,o,h,w] * x[b,i,h-(KH-1-kh),w-(KW-1-kw)]
 * with the corner-tap mask applied in-kernel (masked entries are written as 0).
 * grad_w is OVERWRITTEN (not accumulated).  Either output may be NULL to skip it.
 * `workspace` of finc_backward_workspace_bytes() bytes lets both gradients run on the MFMA strip kernels (grad_x: the
 * forward kernel on the flipped image with transposed fragments; grad_w: pixels on the MFMA K dimension, partial
 * tiles in the workspace, then a reduce).  NULL or a smaller buffer selects the direct kernels.
 */
size_t finc_backward_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW);
int finc_backward_f32(const float *grad_z, const float *x, const float *w_canon, float *grad_x, float *grad_w_canon,
                      int B, int G, int Cq, int H, int W, int KH, int KW, unsigned orient, void *workspace,
                      size_t workspace_bytes, finc_stream_t stream);

/*
 * Backward through the unit's INVERSE (differentiable sampling: reverse-KL training, latent optimisation; the reference has no
 * counterpart -- its `inverse` op, cinc_cuda_level2.cpp:19-32, records nothing for autograd).  With x = inverse(z), i.e. M x = z for
 * M = L_blk + N (L: the unit lower triangular tap of the pixel itself, w_canon[g][:, :, KH-1, KW-1]; N: every other tap), and an
 * upstream gradient grad_x:
 *     grad_z       = y = transpose(inverse(M)) * grad_x
 *     grad_w_canon = -(finc_backward_f32's grad_w at input x and grad_z := y), the same in-kernel corner mask (masked entries 0)
 * transpose(M) is the same convolution read from the opposite corner (every group's orientation bits complemented) with transposed
 * channel matrices; its corner tap, transpose(L), is UPPER triangular, which no inverse kernel takes, so it is factored out on the
 * right:  transpose(M) = (I + sum_t S_t T_t) * transpose(L_blk),  T_t = transpose(W_t) * transpose(inverse(L)),  and
 *     v = inverse(grad_x; bank w_adj, orientation complemented),      y = blockdiag(transpose(inverse(L_g))) * v   per pixel.
 * finc_adjoint_weights_f32: w_canon -> w_adj [G*Cq][Cq][KH][KW] and lead_t [C][C] (C = G*Cq), all math in fp64, rounded once:
 *     w_adj[g][i][o][kh][kw] = sum_k w_canon[g][k][i][kh][kw] * Linv_g[o][k]  for every tap but the corner, whose tap is the identity
 *     lead_t[g*Cq + a][g*Cq + b] = Linv_g[b][a], zero outside the diagonal blocks (row = output channel: a finc_mix_f32 matrix)
 *   w_adj is a canonical bank like any other (finc_check_invariant_f32 passes): finc_inverse_f32 / finc_pack_inverse_weights_f32 +
 *   finc_inverse_packed_f32 solve it with every kernel and launch rule they have.  Any Cq <= FINC_MAX_CQ, G <= 16, any filter.  The
 *   outputs may alias neither the input nor each other (FINC_ERR_BAD_DIMS).
 * finc_lead_product_f32: v <- blockdiag(transpose(inverse(L_g))) * v IN PLACE, v [B][C][HW]: finc_mix_f32's kernel with lead_t where
 *   finc_mix_supported_f32(C), else a plain grouped kernel on the unit upper triangular block of each group (any C; 16-byte pieces when
 *   HW % 4 == 0 and v is 16-byte aligned, dwords otherwise).
 * finc_negate_f32: p[i] <- -p[i] for n floats (0 stays +0): the sign of grad_w, on the [C][Cq][KH][KW] result -- never a pass over
 *   activations.
 * finc_inverse_backward_f32: the one-call form -- adjoint bank, pack, the inverse's FINC_ALGO_AUTO dispatch on w_adj with the
 *   complemented orientation, the lead product, the grad-weight and its sign, all on `stream`, asynchronously.  `x` is the inverse's
 *   OUTPUT.  Either output may be NULL to skip it, not both; grad_w_canon is OVERWRITTEN; `x` is read for grad_w_canon only and may be
 *   NULL without it; grad_z may alias neither grad_x nor x.  `workspace`: finc_inverse_backward_workspace_bytes() bytes, 16-byte
 *   aligned (it holds w_adj, lead_t, y when grad_z is skipped, and what the solve and the grad-weight take: packed fragments, the
 *   padded copies of a width that is no multiple of 4, partial sums); the bound is > 0 for any arguments and never shrinks when B, H
 *   or W grows.  An image of 2 GiB or more (G*Cq*H*W >= 2^29) is FINC_ERR_BAD_DIMS.  Callers that run many backwards on one weight
 *   version keep w_adj, lead_t and the packed fragments and call the pieces (the Python layer does).
 * Status, checked in this order before any HIP call: a NULL required pointer FINC_ERR_NULL_POINTER; the dims FINC_ERR_BAD_DIMS; a
 * pointer not 4-byte aligned FINC_ERR_ALIGNMENT; forbidden aliasing FINC_ERR_BAD_DIMS; a missing, misaligned or short workspace
 * FINC_ERR_WORKSPACE; grad_w_canon for a filter finc_backward_f32 has no grad-weight kernel for (more than 49 taps: 8x8 and up)
 * FINC_ERR_UNSUPPORTED -- grad_z alone is available for every filter.  The four launching calls take part in the sticky-fault rule below like every other.
 */
int finc_adjoint_weights_f32(const float *w_canon, float *w_adj, float *lead_t, int G, int Cq, int KH, int KW, finc_stream_t stream);
int finc_lead_product_f32(float *v, const float *lead_t, int B, int G, int Cq, int HW, finc_stream_t stream);
int finc_negate_f32(float *p, size_t n, finc_stream_t stream);
size_t finc_inverse_backward_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW);
int finc_inverse_backward_f32(const float *grad_x, const float *x, const float *w_canon, float *grad_z, float *grad_w_canon, int B,
                              int G, int Cq, int H, int W, int KH, int KW, unsigned orient, void *workspace, size_t workspace_bytes,
                              finc_stream_t stream);

/*
 * Double precision: the reference op dispatches over float AND double (AT_DISPATCH_FLOATING_TYPES,
 * cinc_cuda_kernel_level2.cu:117), and its CPU solver computes in fp64 (solve_parallel_mc.pyx:77-126, called from
 * layers/conv.py:113-163).  These entry points run the reference visitation and term order in fp64 (separately
 * rounded multiply and subtract): finc_inverse_f64 is bit-exact with that solver.  Same layout and orientation rules
 * as the f32 calls; no workspace, no packed form, any shape.
 */
int finc_canonicalize_weights_f64(const double *w_stored, double *w_canon, int G, int Cq, int KH, int KW,
                                  unsigned orient, finc_stream_t stream);
int finc_inverse_f64(const double *z, const double *w_canon, double *x, int B, int G, int Cq, int H, int W, int KH,
                     int KW, unsigned orient, finc_stream_t stream);
int finc_forward_f64(const double *x, const double *w_canon, double *z, int B, int G, int Cq, int H, int W, int KH,
                     int KW, unsigned orient, finc_stream_t stream);
/*
 * The same two calls with an algorithm choice (round 5): FINC_ALGO_STRICT = the reference-order kernels above; FINC_ALGO_AUTO /
 * FINC_ALGO_MFMA = the double-precision matrix-core form (finc_f64.hip: v_mfma_f64_16x16x4_f64, one wavefront per (image, group),
 * the reference's anti-diagonal visitation band by band, the in-pixel substitution folded into the bank in fp64) for the banks that
 * have one -- Cq <= 24 at 3x3 (configs[1], configs[2]), Cq <= 32 at 2x2, and since version 112 the wider banks of 29 .. 64 channels
 * at 3x3 and 33 .. 64 at 2x2 on a second family that splits a problem's 16-row output tiles over the waves of a workgroup (one
 * barrier per step; finc_debug_f64_plan says which family a shape takes; 25 .. 28 channels at 3x3, more than 64, 5x5 and non-square
 * filters have none); results within 1e-12 of the reference-order solve, not
 * bit-equal to it (the order in which a pixel's terms are added differs).  AUTO falls back to the reference-order kernel for any
 * other shape or when `workspace` is NULL / smaller than finc_f64_workspace_bytes(); MFMA reports FINC_ERR_UNSUPPORTED /
 * FINC_ERR_WORKSPACE instead.  The workspace (8-byte aligned) holds the packed bank; the call packs and launches on `stream`.
 */
size_t finc_f64_workspace_bytes(int G, int Cq, int KH, int KW);
int finc_inverse_f64_algo(const double *z, const double *w_canon, double *x, int B, int G, int Cq, int H, int W, int KH, int KW,
                          unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_forward_f64_algo(const double *x, const double *w_canon, double *z, int B, int G, int Cq, int H, int W, int KH, int KW,
                          unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream);
/*
 * Backward of the forward conv in double precision: finc_backward_f32's two gradients, argument for argument, on doubles.
 *   grad_x = conv_transpose(grad_z, w)
 *   grad_w_canon[o][i][kh][kw] = sum_{b,h,w} grad_z[b,o,h,w] * x[b,i,h-(KH-1-kh),w-(KW-1-kw)]
 * with the corner-tap mask applied in-kernel: masked entries are written as +0.0.  grad_w_canon is OVERWRITTEN.  Either output may
 * be NULL to skip it, not both; `x` is read for grad_w_canon only and `w_canon` for grad_x only (each may be NULL without its output);
 * grad_x may not be grad_z.
 * With a `workspace` of finc_backward_f64_workspace_bytes() bytes (8-byte aligned) the banks of finc_forward_f64_algo's matrix-core
 * form (Cq <= 24 at 3x3, <= 32 at 2x2, 29 .. 64 at 3x3 and 33 .. 64 at 2x2 on the M-split family, on the maps that form takes) run both gradients on v_mfma_f64_16x16x4_f64: grad_x is the
 * forward kernel on the bank packed transposed, every group's orientation complemented; grad_w has the pixels on the MFMA K dimension,
 * one wavefront per (image, group, row chunk) -- and per 16-row output tile on the M-split family --, partial tiles in the workspace and a reduce that adds them in index order (no atomics:
 * the same inputs give the same bits).  Every other shape, and any call whose workspace is NULL, off an 8-byte boundary or too small,
 * runs the direct kernels (one output per thread; grad_w: filters of at most 49 taps, FINC_ERR_UNSUPPORTED beyond, as in
 * finc_backward_f32 -- grad_x is available for every filter).  Results are within 1e-12 of an fp64 autograd of the same convolution.
 * finc_backward_f64_workspace_bytes is > 0 for any arguments and never shrinks when B, H or W grows.
 * Status, checked in this order before any HIP call: a NULL required pointer (grad_z; both outputs; w_canon with grad_x; x with
 * grad_w_canon) FINC_ERR_NULL_POINTER; the dims FINC_ERR_BAD_DIMS; a tensor pointer off an 8-byte boundary FINC_ERR_ALIGNMENT;
 * grad_x == grad_z FINC_ERR_BAD_DIMS; then the sticky-fault rule below.  All launches are asynchronous on `stream`.
 * finc_check_invariant_f64: finc_check_invariant_f32 on doubles (same conditions, same status; synchronises `stream`).
 */
size_t finc_backward_f64_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW);
int finc_backward_f64(const double *grad_z, const double *x, const double *w_canon, double *grad_x, double *grad_w_canon, int B, int G,
                      int Cq, int H, int W, int KH, int KW, unsigned orient, void *workspace, size_t workspace_bytes,
                      finc_stream_t stream);
int finc_check_invariant_f64(const double *w_canon, int G, int Cq, int KH, int KW, finc_stream_t stream);

/*
 * SURVEY 8 f3, second half -- the 1x1 convolution next to the unit (layers/conv1x1.py:29-43: forward
 * F.conv2d(x, W), reverse F.conv2d(z, inverse(W)); one per flow step, fastflow_cifar_multi_gpu.py:224-256) as one
 * streaming pass:      out[b, :, p] = mat * in[b, :, p] + bias      for every pixel p of every image,
 * mat [C][C] row-major (out channel, in channel), bias [C] or NULL, activations fp32 NCHW with HW = H*W.
 * The per-channel affine neighbour folds into the operands on the host: Conv1x1.reverse followed by ActNorm.reverse
 * (layers/actnorm.py:47-52) is mat = diag(exp(log_scale)) * inverse(W), bias = translation.
 * `in == out` is allowed.  FINC_ERR_UNSUPPORTED for channel counts without an instantiation
 * (finc_mix_supported_f32(C) == 0): the caller keeps its own 1x1 convolution for those.
 */
int finc_mix_supported_f32(int C);
int finc_mix_f32(const float *in, const float *mat, const float *bias, float *out, int B, int C, int HW,
                 finc_stream_t stream);

/*
 * Backward of finc_mix_f32 (replaces autograd through F.conv2d, layers/conv1x1.py:29-31), for out = mat * in + bias:
 *   grad_in[b, :, p]  = transpose(mat) * grad_out[b, :, p]
 *   grad_mat[o][i]    = sum_{b,p} grad_out[b,o,p] * in[b,i,p]
 *   grad_bias[o]      = sum_{b,p} grad_out[b,o,p]
 * Same layout as the forward: activations fp32 NCHW with HW = H*W, `mat` the FORWARD matrix, [C][C] row-major (the call
 * transposes it on the device).  Every output is OVERWRITTEN (not accumulated); any of the three may be NULL to skip it, not
 * all of them.  `in` is read for grad_mat only and may be NULL without it.  grad_in may alias neither grad_out nor in
 * (FINC_ERR_BAD_DIMS).  grad_mat and grad_bias need a `workspace` of finc_mix_backward_workspace_bytes() bytes for their partial
 * sums (FINC_ERR_WORKSPACE when it is NULL or smaller; its content on entry is irrelevant); the partials are summed in a fixed
 * order, without atomics: the same inputs give the same bits.  Channel counts: those of finc_mix_supported_f32.
 */
size_t finc_mix_backward_workspace_bytes(int B, int C, int HW);
int finc_mix_backward_f32(const float *grad_out, const float *in, const float *mat, float *grad_in, float *grad_mat,
                          float *grad_bias, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                          finc_stream_t stream);

/*
 * The affine coupling behind its net (layers/coupling.py:44-105; the net's last layer is Conv2dZero, layers/coupling.py:9-41):
 * everything after the last convolution in ONE launch, instead of the reference's twelve elementwise ones.
 *   x, y [B][C][HW] fp32 NCHW, C even, half = C/2;  raw [B][C][HW] = the last convolution's output WITHOUT its bias;
 *   a, b [C]: h = a[c] * raw[:, c] + b[c]   (Conv2dZero: a = exp(3 * logs), b = bias * a);
 *   u_j = h[:, 2j], t_j = h[:, 2j+1], s_j = 2 * tanh(u_j / 2)   (layers/coupling.py:79-82).
 * finc_coupling_f32:   y[:, :half] = x[:, :half];
 *   direction +1 (Coupling.forward, :86-92):  y[:, half+j] = x[:, half+j] * exp(s_j) + t_j,  logdet[b] = sum_{j,p} s_j[b,p]
 *   direction -1 (Coupling.reverse, :95-101): y[:, half+j] = (x[:, half+j] - t_j) * exp(-s_j).
 *   `logdet` [B] may be NULL (and is ignored in the reverse direction); with it the call needs a `workspace` of
 *   finc_coupling_workspace_bytes() bytes for the workgroups' partial sums, added in a fixed order by a second small launch: no
 *   atomics, the same inputs give the same bits.  y == x is allowed; y == raw is not (FINC_ERR_BAD_DIMS).
 * finc_coupling_backward_f32: the gradients of direction +1 (replaces autograd through :79-92 and :38-40), given grad_y and
 *   grad_logdet [B] (NULL = zeros); s and exp(s) are recomputed from raw, nothing else was saved:
 *     grad_x[:, :half] = grad_y[:, :half]  (what reaches x[:, :half] THROUGH THE NET is the caller's: it owns the net's backward)
 *     grad_x[:, half+j] = grad_y2 * exp(s_j)                    with grad_y2 = grad_y[:, half+j]
 *     grad_h[:, 2j+1] = grad_y2,   grad_h[:, 2j] = (grad_y2 * x[:, half+j] * exp(s_j) + grad_logdet[b]) * (1 - s_j^2 / 4)
 *     grad_raw[:, c] = a[c] * grad_h[:, c],   grad_a[c] = sum_{b,p} grad_h[b,c,p] * raw[b,c,p],   grad_b[c] = sum_{b,p} grad_h[b,c,p]
 *   Every output is OVERWRITTEN; any may be NULL to skip it, not all of them.  grad_a / grad_b need the workspace (same size, same
 *   fixed-order sums).  The outputs may alias no input and not each other (FINC_ERR_BAD_DIMS).
 * finc_coupling_reverse_backward_f32: the gradients of direction -1 (replaces autograd through layers/coupling.py:95-101 and :38-40),
 *   given grad_y and `y`, the reverse's OUTPUT (y2 = (x2 - t) * E with E = exp(-s): d y2 / d s = -y2, so the input is not needed, and
 *   in a recorded reverse chain y is what the next layer keeps anyway); th = tanh(u / 2) and E are recomputed from raw:
 *     grad_x[:, :half] = grad_y[:, :half]  (what reaches x[:, :half] through the net is the caller's, as in the forward direction)
 *     grad_x[:, half+j] = grad_y2 * E_j                         with grad_y2 = grad_y[:, half+j]
 *     grad_h[:, 2j+1] = -grad_y2 * E_j,   grad_h[:, 2j] = -(grad_y2 * y[:, half+j]) * (1 - th_j^2)
 *     grad_raw[:, c] = a[c] * grad_h[:, c],   grad_a[c] = sum_{b,p} grad_h[b,c,p] * raw[b,c,p],   grad_b[c] = sum_{b,p} grad_h[b,c,p]
 *   There is no log-det in this direction.  Outputs, workspace, aliasing and status as for finc_coupling_backward_f32.
 * finc_coupling_reverse_logdet_f32: direction -1 of finc_coupling_f32 -- the same y, bit for bit -- and, from the same pass,
 *     logdet[b] = sum_{j,p} s_j[b,p]:
 *   the log-det of the FORWARD map, i.e. what direction +1 reports at the recovered input y (s depends on the untouched half only,
 *   which x and y share).  The reverse map's own log-Jacobian is its negative.  It is what a sampler adds to the base density:
 *   log q(y) = log p(x) + (the layers in front) + logdet.  `logdet` [B] is required (FINC_ERR_NULL_POINTER), and so is a `workspace`
 *   of finc_coupling_workspace_bytes() bytes: the partials are those of direction +1 (one per workgroup, the same grid), which that
 *   size already covers, summed by the same second launch in a fixed order -- no atomics, the same inputs give the same bits.
 *   y == x is allowed; y == raw is not (FINC_ERR_BAD_DIMS).
 * finc_coupling_reverse_logdet_backward_f32: the gradients of finc_coupling_reverse_logdet_f32, given grad_y, grad_logdet [B]
 *   (NULL = zeros) and the reverse's OUTPUT y: finc_coupling_reverse_backward_f32 with one more term,
 *     grad_h[:, 2j] = (-(grad_y2 * y[:, half+j]) + grad_logdet[b]) * (1 - th_j^2)
 *   and everything else as there.  With grad_logdet NULL every output has the bits finc_coupling_reverse_backward_f32 gives.
 *   Outputs, workspace, aliasing and status as for finc_coupling_reverse_backward_f32.
 * finc_coupling_backward_reconstruct_f32: the gradients of direction +1 (layers/coupling.py:79-92) given grad_y, grad_logdet [B]
 *   (NULL = zeros) and `y`, the forward's OUTPUT, with the forward's input rebuilt in the same pass (:95-101) -- what a training
 *   backward that stores no activations runs per coupling, instead of finc_coupling_f32(direction -1) + finc_coupling_backward_f32.
 *   With th_j = tanh(u_j / 2), s_j = 2 th_j, E_j = exp(s_j) recomputed from raw:
 *     x_out[:, :half] = y[:, :half],   x_out[:, half+j] = (y[:, half+j] - t_j) / E_j    (the bits of finc_coupling_f32, direction -1)
 *     grad_x[:, :half] = grad_y[:, :half]  (what reaches x[:, :half] through the net is the caller's, as above)
 *     grad_x[:, half+j] = grad_y2 * E_j                         with grad_y2 = grad_y[:, half+j]
 *     grad_h[:, 2j+1] = grad_y2,   grad_h[:, 2j] = (grad_y2 * (y[:, half+j] - t_j) + grad_logdet[b]) * (1 - th_j^2)
 *     grad_raw[:, c] = a[c] * grad_h[:, c],   grad_a[c] = sum_{b,p} grad_h[b,c,p] * raw[b,c,p],   grad_b[c] = sum_{b,p} grad_h[b,c,p]
 *   Every output is OVERWRITTEN; x_out and each gradient may be NULL to skip it, not all of them.  Aliasing: x_out == y and
 *   grad_x == grad_y are allowed (in place); any other output on grad_y, y, raw or on another output is FINC_ERR_BAD_DIMS.
 *   Workspace (grad_a / grad_b only) and status as for finc_coupling_backward_f32.  A channel with |t| >> |y - t| loses digits
 *   in y - t: x_out and grad_h[:, 2j] carry that cancellation, which the stored-input form does not have.
 * finc_bias_relu_f32: out = max(in + bias[c], 0) -- the Conv2d bias and the nn.ReLU behind the net's first two convolutions
 *   (layers/coupling.py:58-63) in one pass; in == out allowed.  Inference only (no backward).
 * Rows of HW floats move as 16-byte pieces when HW % 4 == 0 and every activation pointer is 16-byte aligned, as dwords otherwise.
 * The _rawbf16_f32 siblings (version 113): the same six calls for a net that ran under bf16 autocast.  `raw` is bfloat16, given as
 *   its bits (const uint16_t *), and is read as it lies -- bf16 -> fp32 is exact, so every fp32 output (y, logdet, x_out, grad_x,
 *   grad_a, grad_b) has the BITS of the _f32 call on the same values widened; `grad_raw` (uint16_t *) is bfloat16 as well: the fp32
 *   value the _f32 call writes, rounded to nearest even once (grad_a and grad_b are summed before that rounding).  x, y, a, b, every
 *   other gradient, the log-det and the workspace (finc_coupling_workspace_bytes) stay fp32: the flow's own map keeps its
 *   invertibility and its log-det in fp32.  Argument lists, refusals and their order, aliasing rules and status are the sibling's; a
 *   bf16 pointer is held to 2 bytes (FINC_ERR_ALIGNMENT on an odd address), and the 16-byte-piece form additionally wants raw and
 *   grad_raw on 8 bytes (four bf16 pixels), single 2-byte elements otherwise.
 * finc_bias_relu_bf16: finc_bias_relu_f32 on bfloat16 activations (bits), bias fp32: the add and the max in fp32, rounded to nearest
 *   even once; a NaN stays a NaN; in == out allowed.  16-byte pieces of eight when HW % 8 == 0 and both pointers are 16-byte aligned,
 *   single elements otherwise.
 * The split prior with its latent (version 114; layers/splitprior.py:7-41 with the factored-out half handed back): the coupling
 * above whose second output half z2 is scored under a standard normal, with the two halves as tensors of their own.  x1, z2
 * [B][half][HW] fp32 contiguous, x [B][C][HW], D = half * HW, c = D / 2 * log(2 pi).
 * finc_split_prior_f32: direction +1 with two outputs, x1 = x[:, :half] and z2[:, j] = x[:, half+j] * exp(s_j) + t_j -- the bits of
 *   the two halves of finc_coupling_f32(direction +1) -- and log_p[b] = sum_{j,p} s_j - 1/2 sum_{j,p} z2^2 - c: the coupling's
 *   log-det plus the standard-normal log-density of z2, what SplitPrior.forward reports, from the pass that had z2 in registers
 *   (-c is added inside the launch).  x1, z2 and log_p are required, and so is a workspace of finc_coupling_workspace_bytes().
 * finc_split_prior_merge_f32: direction -1 with two inputs: x[:, :half] = x1, x[:, half+j] = (z2[:, j] - t_j) * exp(-s_j): the bits of
 *   finc_coupling_f32(direction -1) on cat(x1, z2), without that cat.  `log_p` [B] is optional: with it (and the workspace) the
 *   call reports the value finc_split_prior_f32 reports at the result x, sum s - 1/2 sum z2^2 - c from the z2 it was handed;
 *   NULL: no partials are written and the workspace is not touched.
 * finc_split_prior_backward_f32: the gradients of finc_split_prior_f32 given grad_x1, grad_z2 [B][half][HW] and grad_log_p [B]
 *   -- each may be NULL (zeros), not all three -- and the forward's INPUT x.  With E = exp(s) and z2 = x2 * E + t recomputed from
 *   raw and G = grad_z2 - grad_log_p[b] * z2:
 *     grad_x[:, :half] = grad_x1,   grad_x[:, half+j] = G * E_j,
 *     grad_h[:, 2j+1] = G,   grad_h[:, 2j] = (G * E_j * x[:, half+j] + grad_log_p[b]) * (1 - s_j^2 / 4),
 *   grad_raw, grad_a and grad_b from grad_h as for finc_coupling_backward_f32; outputs, workspace and status as there.
 * Aliasing: x1, z2 and x may not overlap each other, nor may an output be raw (FINC_ERR_BAD_DIMS); the backward's outputs may
 *   alias no input and not each other.  The sums are fixed-order without atomics: the same inputs give the same bits.  The
 *   16-byte-piece form wants every activation pointer of the call, the half tensors included, on 16 bytes.  Each has its
 *   _rawbf16_f32 sibling, under the rules of the six above.
 * Status: a NULL required pointer FINC_ERR_NULL_POINTER, non-positive dims FINC_ERR_BAD_DIMS, odd C FINC_ERR_UNSUPPORTED
 * (finc_coupling_supported_f32(C) == 0), a missing / short workspace where one is needed FINC_ERR_WORKSPACE.
 */
int finc_coupling_supported_f32(int C);
size_t finc_coupling_workspace_bytes(int B, int C, int HW);
int finc_coupling_f32(const float *x, const float *raw, const float *a, const float *b, float *y, float *logdet, int B, int C,
                      int HW, int direction, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_coupling_backward_f32(const float *grad_y, const float *grad_logdet, const float *x, const float *raw, const float *a,
                               const float *b, float *grad_x, float *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                               void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_coupling_reverse_backward_f32(const float *grad_y, const float *y, const float *raw, const float *a, const float *b,
                                       float *grad_x, float *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                                       void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_coupling_reverse_logdet_f32(const float *x, const float *raw, const float *a, const float *b, float *y, float *logdet,
                                     int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_coupling_reverse_logdet_backward_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *raw,
                                              const float *a, const float *b, float *grad_x, float *grad_raw, float *grad_a,
                                              float *grad_b, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                              finc_stream_t stream);
int finc_coupling_backward_reconstruct_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *raw,
                                           const float *a, const float *b, float *x_out, float *grad_x, float *grad_raw,
                                           float *grad_a, float *grad_b, int B, int C, int HW, void *workspace,
                                           size_t workspace_bytes, finc_stream_t stream);
int finc_bias_relu_f32(const float *in, const float *bias, float *out, int B, int C, int HW, finc_stream_t stream);
int finc_coupling_rawbf16_f32(const float *x, const uint16_t *raw, const float *a, const float *b, float *y, float *logdet, int B, int C,
                              int HW, int direction, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_coupling_backward_rawbf16_f32(const float *grad_y, const float *grad_logdet, const float *x, const uint16_t *raw,
                                       const float *a, const float *b, float *grad_x, uint16_t *grad_raw, float *grad_a, float *grad_b,
                                       int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_coupling_reverse_backward_rawbf16_f32(const float *grad_y, const float *y, const uint16_t *raw, const float *a, const float *b,
                                               float *grad_x, uint16_t *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                                               void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_coupling_reverse_logdet_rawbf16_f32(const float *x, const uint16_t *raw, const float *a, const float *b, float *y,
                                             float *logdet, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                             finc_stream_t stream);
int finc_coupling_reverse_logdet_backward_rawbf16_f32(const float *grad_y, const float *grad_logdet, const float *y, const uint16_t *raw,
                                                      const float *a, const float *b, float *grad_x, uint16_t *grad_raw, float *grad_a,
                                                      float *grad_b, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                                      finc_stream_t stream);
int finc_coupling_backward_reconstruct_rawbf16_f32(const float *grad_y, const float *grad_logdet, const float *y, const uint16_t *raw,
                                                   const float *a, const float *b, float *x_out, float *grad_x, uint16_t *grad_raw,
                                                   float *grad_a, float *grad_b, int B, int C, int HW, void *workspace,
                                                   size_t workspace_bytes, finc_stream_t stream);
int finc_bias_relu_bf16(const uint16_t *in, const float *bias, uint16_t *out, int B, int C, int HW, finc_stream_t stream);
int finc_split_prior_f32(const float *x, const float *raw, const float *a, const float *b, float *x1, float *z2, float *log_p, int B,
                         int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_split_prior_merge_f32(const float *x1, const float *z2, const float *raw, const float *a, const float *b, float *x,
                               float *log_p, int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_split_prior_backward_f32(const float *grad_x1, const float *grad_z2, const float *grad_log_p, const float *x,
                                  const float *raw, const float *a, const float *b, float *grad_x, float *grad_raw, float *grad_a,
                                  float *grad_b, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                  finc_stream_t stream);
int finc_split_prior_rawbf16_f32(const float *x, const uint16_t *raw, const float *a, const float *b, float *x1, float *z2,
                                 float *log_p, int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_split_prior_merge_rawbf16_f32(const float *x1, const float *z2, const uint16_t *raw, const float *a, const float *b, float *x,
                                       float *log_p, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                       finc_stream_t stream);
int finc_split_prior_backward_rawbf16_f32(const float *grad_x1, const float *grad_z2, const float *grad_log_p, const float *x,
                                          const uint16_t *raw, const float *a, const float *b, float *grad_x, uint16_t *grad_raw,
                                          float *grad_a, float *grad_b, int B, int C, int HW, void *workspace,
                                          size_t workspace_bytes, finc_stream_t stream);

/*
 * The Gaussianized split (version 116; layers/split.py:4-52, Glow figure 2 / RealNVP figure 4b): the level boundary that models the
 * second half of the channels as N(m, exp(logs)^2), with (m, logs) from ONE convolution of the first half.  The tensors, the
 * argument lists, the workspace (finc_coupling_workspace_bytes), the 16-byte-piece rule, the aliasing rules and the refusal order are
 * those of finc_split_prior_f32 / _merge_f32 / _backward_f32 above; what differs is the arithmetic.  raw [B][C][HW] fp32 is that
 * convolution's output WITHOUT its bias, h = a[c] * raw + b[c] (a = exp(log_scale_factor), b = bias * a), and per channel j < half
 * and pixel  m = h[:, 2j]  (even channels: the mean),  logs = h[:, 2j+1]  (odd channels: the log-scale);  D = half * HW,
 * c = D / 2 * log(2 pi).
 * finc_gauss_split_f32: x1 = x[:, :half], z2[:, j] = (x[:, half+j] - m_j) * exp(-logs_j), and log_p[b] = -sum_{j,p} logs_j -
 *   1/2 sum_{j,p} z2^2 - c: the split's log-det plus the standard-normal log-density of z2, from the pass that had z2 in registers.
 *   x1, z2, log_p and the workspace are required.
 * finc_gauss_split_merge_f32: x[:, :half] = x1, x[:, half+j] = z2[:, j] * exp(logs_j) + m_j (one fma), without a cat.  `log_p` [B]
 *   is optional: with it (and the workspace) the call reports the value finc_gauss_split_f32 reports at the result x, from the z2
 *   it was handed; NULL: no partials are written and the workspace is not touched.
 * finc_gauss_split_backward_f32: the gradients of finc_gauss_split_f32 given grad_x1, grad_z2 [B][half][HW] and grad_log_p [B] --
 *   each may be NULL (zeros), not all three -- and the forward's INPUT x.  With E = exp(-logs) and z2 = (x2 - m) * E recomputed
 *   from raw and G = grad_z2 - grad_log_p[b] * z2:
 *     grad_x[:, :half] = grad_x1,   grad_x[:, half+j] = G * E_j,
 *     grad_h[:, 2j] = -G * E_j,   grad_h[:, 2j+1] = -(G * z2 + grad_log_p[b]),
 *   grad_raw[c] = a[c] * grad_h[c], grad_a[c] = sum grad_h * raw, grad_b[c] = sum grad_h (fixed-order sums through the workspace, no
 *   atomics: the same inputs give the same bits); each output may be NULL, not all four.  What reaches x[:, :half] through the
 *   convolution is the caller's (autograd's).
 * There are no _rawbf16_f32 siblings: a net under autocast hands its output over upcast.
 */
int finc_gauss_split_f32(const float *x, const float *raw, const float *a, const float *b, float *x1, float *z2, float *log_p, int B,
                         int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_gauss_split_merge_f32(const float *x1, const float *z2, const float *raw, const float *a, const float *b, float *x,
                               float *log_p, int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_gauss_split_backward_f32(const float *grad_x1, const float *grad_z2, const float *grad_log_p, const float *x,
                                  const float *raw, const float *a, const float *b, float *grad_x, float *grad_raw, float *grad_a,
                                  float *grad_b, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                  finc_stream_t stream);

/*
 * The backward of the two merges (version 117): what a recorded glow.SplitPrior.merge / glow.Split.merge launches inside
 * ops.reverse_grad().  Each differentiates its merge from the merge's OUTPUT x [B][C][HW] (the convention of
 * finc_coupling_reverse_backward_f32: the next layer of a reverse chain keeps x anyway), given grad_x [B][C][HW] and grad_log_p [B] --
 * either may be NULL (zeros), not both -- with raw, a, b as the merge had them.  With g2 = grad_x[:, half+j], x2 = x[:, half+j],
 * glp = grad_log_p[b] and h = a * raw + b:
 * finc_split_prior_merge_backward_f32 (of finc_split_prior_merge_f32: x2 = (z2 - t) * exp(-s), log p = sum s - 1/2 sum z2^2 - c):
 *   s = 2 tanh(h[:, 2j] / 2), E = exp(-s), z2 = x2 * exp(s) + t recomputed from raw:
 *     grad_z2 = g2 * E - glp * z2,   grad_t = -g2 * E,   grad_s = -g2 * x2 + glp,
 *     grad_h[:, 2j] = grad_s * (1 - (s/2)^2),   grad_h[:, 2j+1] = grad_t.
 *   With grad_log_p NULL, grad_z2, grad_raw, grad_a and grad_b carry the bits of finc_coupling_reverse_backward_f32 on the same
 *   (grad_x, x, raw, a, b), grad_z2 those of the second half of its grad_x.
 * finc_split_prior_merge_backward_rawbf16_f32: the same on a bf16 raw; grad_raw is written in bf16, rounded once behind the fp32 sums.
 * finc_gauss_split_merge_backward_f32 (of finc_gauss_split_merge_f32: x2 = z2 * exp(logs) + m, log p = -sum logs - 1/2 sum z2^2 - c;
 *   fp32 raw only):  d = x2 - m, z2 = d * exp(-logs):
 *     grad_z2 = g2 * exp(logs) - glp * z2,   grad_h[:, 2j] = g2,   grad_h[:, 2j+1] = g2 * d - glp.
 * All three: grad_x1 [B][half][HW] = grad_x[:, :half], the direct share only, copied by the same threads (what reaches x1 through the
 * net or the convolution is the caller's, autograd's); grad_z2 [B][half][HW]; grad_raw[c] = a[c] * grad_h[c] like raw; grad_a[c] =
 * sum grad_h * raw, grad_b[c] = sum grad_h (fixed-order sums through the workspace, finc_coupling_workspace_bytes, no atomics: the same
 * inputs give the same bits).  Each output may be NULL, not all five.  No output may share a byte with an input or with another
 * output (FINC_ERR_BAD_DIMS).  The 16-byte-piece rule counts every pointer of the call, the half tensors included.  Refusal order:
 * NULL -> dims and overlap -> alignment -> channel count -> workspace.
 */
int finc_split_prior_merge_backward_f32(const float *grad_x, const float *grad_log_p, const float *x, const float *raw, const float *a,
                                        const float *b, float *grad_x1, float *grad_z2, float *grad_raw, float *grad_a, float *grad_b,
                                        int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_split_prior_merge_backward_rawbf16_f32(const float *grad_x, const float *grad_log_p, const float *x, const uint16_t *raw,
                                                const float *a, const float *b, float *grad_x1, float *grad_z2, uint16_t *grad_raw,
                                                float *grad_a, float *grad_b, int B, int C, int HW, void *workspace,
                                                size_t workspace_bytes, finc_stream_t stream);
int finc_gauss_split_merge_backward_f32(const float *grad_x, const float *grad_log_p, const float *x, const float *raw, const float *a,
                                        const float *b, float *grad_x1, float *grad_z2, float *grad_raw, float *grad_a, float *grad_b,
                                        int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);

/*
 * The PLU-parametrised 1x1 convolution's parameter work (version 118; Kingma & Dhariwal 2018, section 3.2): what glow.Conv1x1LU
 * launches.  The layer keeps  W = P L Ut  with  L = strict_lower(lower) + I,  Ut = strict_upper(upper) + diag(sign_s * exp(log_s)),
 * M = L Ut  and  W[r][:] = M[perm[r]][:]:  lower, upper [C][C] row-major fp32 (only the strict triangles are read), log_s, sign_s [C]
 * fp32, perm [C] int32, a permutation of 0 .. C-1.  The per-pixel product with W or W^-1 is finc_mix_f32's.
 * finc_plu_supported_f32: 1 for 1 <= C <= 512, the widths the two entry points take (C is a runtime argument; the bound is the LDS of
 *   the rows a workgroup stages, 88 bytes per channel), else 0.
 * finc_plu_compose_f32: ONE launch that writes any of  w [C][C] = W,  w_inv [C][C] = W^-1 (column r = Ut^-1 L^-1 e_perm[r]: two
 *   triangular solves, no pivoting)  and  logdet (one float) = sum(log_s) = log|det W|;  at least one non-NULL.  All arithmetic in fp64,
 *   every output rounded to fp32 once, every sum in a fixed order, no atomics: the same inputs give the same bits.
 * finc_plu_compose_backward_f32: from grad_w [C][C] = dl/dW and grad_logdet (one float, NULL = 0), with G_M[perm[r]][:] = grad_w[r][:]:
 *     grad_lower = strict_lower(G_M Ut^T),   grad_upper = strict_upper(L^T G_M),
 *     grad_log_s[i] = (L^T G_M)[i][i] * sign_s[i] * exp(log_s[i]) + grad_logdet,
 *   each wanted or not by pointer (not all three NULL): one fp64 dot product in a fixed order per entry, ONE launch.  The entries of
 *   grad_lower on and above the diagonal and of grad_upper on and below it are written as +0 by the kernel.  (A gradient that arrives
 *   through W^-1 is folded into grad_w by the caller: grad_w - W^-T grad_winv W^-T.)
 * `perm` lives in device memory, so neither the host nor the kernels trust it: an entry outside [0, C) is never used as an index.  It
 *   makes row r of w and column r of w_inv NaN; in the backward the row of G_M that no entry names reads as NaN.  Nothing else is touched.
 * No output may share a byte with an input or with another output (FINC_ERR_BAD_DIMS).  No workspace.  Refusal order: NULL -> dims
 * (C < 1, overlap) -> alignment (4 bytes, perm included) -> a width without a kernel (FINC_ERR_UNSUPPORTED) -> the fault gate.
 */
int finc_plu_supported_f32(int C);
int finc_plu_compose_f32(const float *lower, const float *upper, const float *log_s, const float *sign_s, const int *perm, float *w,
                         float *w_inv, float *logdet, int C, finc_stream_t stream);
int finc_plu_compose_backward_f32(const float *grad_w, const float *grad_logdet, const float *lower, const float *upper,
                                  const float *log_s, const float *sign_s, const int *perm, float *grad_lower, float *grad_upper,
                                  float *grad_log_s, int C, finc_stream_t stream);

/*
 * ActNorm (layers/actnorm.py:5-66) on its own kernels: activations [B][C][HW] fp32, log_scale and translation [C], any C >= 1
 * (up to FINC_MAX_CQ * FINC_MAX_GROUPS), HW >= 1.
 * finc_actnorm_f32: direction +1: y = (x - translation[c]) * exp(-log_scale[c]) (layers/actnorm.py:34); direction -1:
 *   y = x * exp(log_scale[c]) + translation[c] (:51).  y == x allowed.  A non-NULL `logdet` (forward direction; ignored in the
 *   reverse) is filled by the SAME launch: logdet[b] = -(sum_c log_scale[c]) * HW for every image (:57-65), the sum over C in a
 *   fixed order by one wave.  No workspace.
 * finc_actnorm_backward_f32: gradients of the forward direction from grad_y, grad_logdet ([B], NULL = zeros), log_scale and `y`,
 *   the forward's OUTPUT (x - translation = y * exp(log_scale): nothing but what the next layer keeps anyway is needed):
 *     grad_x[b,c,p]       = grad_y[b,c,p] * exp(-log_scale[c])
 *     grad_translation[c] = -exp(-log_scale[c]) * sum_{b,p} grad_y[b,c,p]
 *     grad_log_scale[c]   = -sum_{b,p} grad_y[b,c,p] * y[b,c,p]  -  HW * sum_b grad_logdet[b]
 *   Every output is OVERWRITTEN; any may be NULL to skip it, not all of them.  grad_x == grad_y allowed, grad_x == y is not
 *   (FINC_ERR_BAD_DIMS).  The two per-channel outputs need the workspace; their sums run in a fixed order (no atomics).
 * finc_actnorm_backward_reconstruct_f32: finc_actnorm_backward_f32 -- the same three formulas, the same fixed-order sums -- that
 *   from the same read of `y` also rebuilds the forward's input (layers/actnorm.py:51):
 *     x_out[b,c,p] = y[b,c,p] * exp(log_scale[c]) + translation[c]        (the bits of finc_actnorm_f32, direction -1)
 *   What a training backward that stores no activations runs per ActNorm, instead of finc_actnorm_f32(direction -1) +
 *   finc_actnorm_backward_f32.  grad_logdet, x_out and each gradient may be NULL, not every output; `translation` is read for
 *   x_out only (NULL without it).  Aliasing: x_out == y and grad_x == grad_y are allowed (in place); x_out on grad_y or grad_x,
 *   and grad_x on y, are FINC_ERR_BAD_DIMS.  Workspace and status as for finc_actnorm_backward_f32.
 * finc_actnorm_reverse_backward_f32: gradients of the reverse direction (replaces autograd through layers/actnorm.py:47-52) from
 *   grad_y, log_scale and `x`, the reverse's INPUT (the output would do in real arithmetic, x * exp(log_scale) = y - translation, but
 *   that difference cancels on a channel whose translation dwarfs its spread):
 *     grad_x[b,c,p]       = grad_y[b,c,p] * exp(log_scale[c])
 *     grad_log_scale[c]   = exp(log_scale[c]) * sum_{b,p} grad_y[b,c,p] * x[b,c,p]
 *     grad_translation[c] = sum_{b,p} grad_y[b,c,p]
 *   Outputs, workspace and status as for finc_actnorm_backward_f32; grad_x == grad_y allowed, grad_x == x is not.
 * finc_actnorm_init_f32: the data-dependent initialisation (:17-23) written straight into the parameters, no host round trip:
 *   translation[c] = mean over (b, p), log_scale[c] = log(std + 1e-8) with the UNBIASED standard deviation (divisor n - 1,
 *   n = B * HW; torch.std's default), one pass over x on (n, mean, M2) triples merged pairwise in a fixed order.  n < 2 is
 *   FINC_ERR_BAD_DIMS (the reference's result there is NaN).  Needs the workspace.
 * finc_actnorm_workspace_bytes: one bound for the backward and the initialisation; > 0 for any arguments, never shrinks when B or
 *   HW grows.
 * Rows of HW floats move as 16-byte pieces when HW % 4 == 0 and every activation pointer is 16-byte aligned, as dwords otherwise.
 * The _rawbf16_f32 siblings (version 113): the same six calls for a net that ran under bf16 autocast.  `raw` is bfloat16, given as
 *   its bits (const uint16_t *), and is read as it lies -- bf16 -> fp32 is exact, so every fp32 output (y, logdet, x_out, grad_x,
 *   grad_a, grad_b) has the BITS of the _f32 call on the same values widened; `grad_raw` (uint16_t *) is bfloat16 as well: the fp32
 *   value the _f32 call writes, rounded to nearest even once (grad_a and grad_b are summed before that rounding).  x, y, a, b, every
 *   other gradient, the log-det and the workspace (finc_coupling_workspace_bytes) stay fp32: the flow's own map keeps its
 *   invertibility and its log-det in fp32.  Argument lists, refusals and their order, aliasing rules and status are the sibling's; a
 *   bf16 pointer is held to 2 bytes (FINC_ERR_ALIGNMENT on an odd address), and the 16-byte-piece form additionally wants raw and
 *   grad_raw on 8 bytes (four bf16 pixels), single 2-byte elements otherwise.
 * finc_bias_relu_bf16: finc_bias_relu_f32 on bfloat16 activations (bits), bias fp32: the add and the max in fp32, rounded to nearest
 *   even once; a NaN stays a NaN; in == out allowed.  16-byte pieces of eight when HW % 8 == 0 and both pointers are 16-byte aligned,
 *   single elements otherwise.
 * Status: a NULL required pointer FINC_ERR_NULL_POINTER; non-positive / overflowing dims, a direction other than +1 / -1 or
 * forbidden aliasing FINC_ERR_BAD_DIMS; a pointer not 4-byte aligned FINC_ERR_ALIGNMENT; a missing / short workspace where one is
 * needed FINC_ERR_WORKSPACE -- checked in that order, before any HIP call.  The four launching calls take part in the
 * sticky-fault rule below like every other.
 */
size_t finc_actnorm_workspace_bytes(int B, int C, int HW);
int finc_actnorm_f32(const float *x, const float *log_scale, const float *translation, float *y, float *logdet, int B, int C, int HW,
                     int direction, finc_stream_t stream);
int finc_actnorm_backward_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *log_scale, float *grad_x,
                              float *grad_log_scale, float *grad_translation, int B, int C, int HW, void *workspace,
                              size_t workspace_bytes, finc_stream_t stream);
int finc_actnorm_backward_reconstruct_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *log_scale,
                                          const float *translation, float *x_out, float *grad_x, float *grad_log_scale,
                                          float *grad_translation, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                          finc_stream_t stream);
int finc_actnorm_reverse_backward_f32(const float *grad_y, const float *x, const float *log_scale, float *grad_x, float *grad_log_scale,
                                      float *grad_translation, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                      finc_stream_t stream);
int finc_actnorm_init_f32(const float *x, float *log_scale, float *translation, int B, int C, int HW, void *workspace,
                          size_t workspace_bytes, finc_stream_t stream);

/*
 * The element-wise monotone rational-quadratic spline with linear tails (version 120; layers/activations.py SplineActivation,
 * layers/splines/rational_quadratic.py): activations [B][C][HW] fp32.  The calls read a KNOT TABLE, not the unnormalised parameters:
 *   table[(a * (K + 1) + k) * P + p],  a = 0 cumwidths, 1 cumheights, 2 derivatives (rational_quadratic.py:97-115, the padded end
 *   derivatives included), knot k of K + 1, table row p of P.  P = 1: one spline for all elements; P = C * HW: one per position
 *   (individual_weights=True).  2 <= K <= 16 (finc_spline_supported_f32).  Knots must increase; cumwidths[0] = cumheights[0] =
 *   -tail_bound and cumwidths[K] = cumheights[K] = tail_bound as the reference pins them.
 * finc_spline_f32: direction +1 is :161-175, direction -1 is :135-159 with the discriminant clamped at 0 before the square root (the
 *   reference asserts it non-negative on the host; there is no host round trip here).  The bin is the reference's: the knots <= x
 *   counted, minus one, x == tail_bound in the last bin.  Outside [-tail_bound, tail_bound], and for NaN, y is x's bits and the
 *   log-derivative 0.  `logdet` [B] (optional; needs the workspace): in EITHER direction the FORWARD map's log-det per image, in
 *   direction -1 at the recovered input (minus what the reference's inverse returns), summed in a fixed order -- the same inputs give
 *   the same bits.  y == x is allowed.
 * finc_spline_backward_f32: gradients of direction +1 from its saved INPUT x: grad_x = grad_y f'(x) + grad_logdet[b] dlog f'/dx and
 *   grad_table [3 (K + 1)][P], the gradient of the table as laid out above (an element adds to its own bin's two knots per array; a
 *   tail element adds nothing and hands grad_y through), a fixed-order sum over the batch (P > 1) or over everything (P = 1); it needs
 *   the workspace.  grad_y and grad_logdet may be NULL (zeros), not both; grad_x and grad_table may be NULL, not both.
 * finc_spline_reverse_backward_f32: gradients of direction -1 (dx/dy = 1 / f'(x), dx/dtable = -(df/dtable) / f'(x)) from its saved
 *   INPUT, handed over as `x`: the position of the recovered value in its bin is the root of the reverse's quadratic, recomputed
 *   here -- taken as a quotient from the stored output it cancels in a narrow bin, and the log-det's gradient with it.
 *   grad_logdet: of the log-det that call returned, NULL when it returned none.  Otherwise as above.
 *   grad_x == grad_y is allowed in both; grad_x == x is FINC_ERR_BAD_DIMS.
 * Refusal order: NULL -> dims (non-positive or overflowing, a direction other than +1 / -1, a tail_bound that is not positive and
 * finite, forbidden aliasing) FINC_ERR_BAD_DIMS -> a pointer not 4-byte aligned FINC_ERR_ALIGNMENT -> K outside 2..16 or a P that is
 * neither 1 nor C * HW FINC_ERR_UNSUPPORTED -> a missing / short workspace where one is needed FINC_ERR_WORKSPACE -> the sticky-fault
 * rule below.
 */
int finc_spline_supported_f32(int K);
size_t finc_spline_workspace_bytes(int B, int C, int HW, int K, int P);
int finc_spline_f32(const float *x, const float *table, int P, int K, float tail_bound, int direction, float *y, float *logdet, int B,
                    int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_spline_backward_f32(const float *grad_y, const float *grad_logdet, const float *x, const float *table, int P, int K,
                             float tail_bound, float *grad_x, float *grad_table, int B, int C, int HW, void *workspace,
                             size_t workspace_bytes, finc_stream_t stream);
int finc_spline_reverse_backward_f32(const float *grad_y, const float *grad_logdet, const float *x, const float *table, int P, int K,
                                     float tail_bound, float *grad_x, float *grad_table, int B, int C, int HW, void *workspace,
                                     size_t workspace_bytes, finc_stream_t stream);

/*
 * The smooth invertible activations (version 121; layers/activations.py SmoothLeakyRelu :36-54, LeakyRelu :57-79, LearnableLeakyRelu
 * :82-105, SmoothTanh :108-123): element-wise maps on activations [B][C][HW] fp32, which the kernels walk as [B][C * HW].  With x the
 * forward's input, f the forward map and L = log f':
 *   FINC_ACT_SMOOTH_LEAKY_RELU (p0 = a)          f = a x + (1 - a) softplus(x),  f' = a + (1 - a) sigmoid(x)
 *   FINC_ACT_LEAKY_RELU (p0 = a)                 f = x < 0 ? a x : x,            f' = x < 0 ? a : 1   (x < 0 strictly, as the reference)
 *   FINC_ACT_LEARNABLE_LEAKY_RELU                the same with a = *slope_dev, a DEVICE pointer (no host round trip); p0, p1 ignored
 *   FINC_ACT_SMOOTH_TANH (p0 = a, p1 = b)        f = tanh(a x) + b x,            f' = b + a sech^2(a x)
 * A NaN passes through with log-derivative 0.  finc_activation_supported_f32: 1 for these four kinds, 0 otherwise.
 * finc_activation_f32: direction +1 is f, direction -1 its inverse -- a select and a division for the leaky kinds; for the smooth kinds
 *   a Newton iteration inside an analytic bracket with a FIXED trip count (finc_debug_activation_trips; a step that leaves the
 *   bracket is replaced by the midpoint), so every finite y gives a finite x inside the bracket, where the reference's 100 unbracketed
 *   steps cycle for SmoothTanh(3, 0.05).  Accuracy is claimed AT the parameters the sweep of DESIGN 3.26 covers -- a among 0.01, 0.1,
 *   0.3, 0.9, 1.0, 1.5 (smooth leaky ReLU), (a, b) among (1, 0.1), (3, 0.05), (8, 0.01), (0.5, 1), (0.1, 0.01) (smooth tanh) -- and
 *   nowhere between or beyond them: there the result is bracketed and finite, no more.  `logdet` [B]
 *   (optional; needs the workspace): in EITHER direction the FORWARD map's log-det per image, in direction -1 at the recovered input,
 *   summed in a fixed order that does not depend on the batch size -- the same inputs give the same bits, and y has the same bits
 *   with and without it.  y == x is allowed.
 * finc_activation_backward_f32: every backward, by `mode` (0 forward, 1 reverse, 2 rebuild):
 *   0  from v = the forward's INPUT x:   grad_x = grad_y f'(x) + grad_logdet[b] L'(x);
 *   1  of direction -1, from v = its OUTPUT x (grad_y here is the gradient that reaches that output, grad_logdet that of the log-det
 *      the call returned):   grad_x (the gradient of the reverse's input) = (grad_y + grad_logdet[b] L'(x)) / f'(x);
 *   2  from v = the forward's OUTPUT y: x = f^-1(y) with the bits direction -1 returns, written to x_out when given, and the mode-0
 *      gradients at that x in the same launch.
 *   grad_y, grad_logdet may be NULL (zeros), not both; x_out (mode 2 only), grad_x, grad_slope may be NULL, not all.  grad_slope [1]
 *   (the learnable kind only; needs the workspace): the slope's gradient, a fixed-order sum.  grad_x == grad_y and x_out == v are
 *   allowed; grad_x == v, x_out == grad_y and x_out == grad_x are FINC_ERR_BAD_DIMS.
 * Thread items are 16-byte pieces of four when C * HW % 4 == 0 (whatever HW is) and every activation pointer is 16-byte aligned, single
 * elements otherwise.
 * Refusal order: NULL -> dims (non-positive or overflowing, a direction other than +1 / -1, an unknown mode, forbidden aliasing)
 * FINC_ERR_BAD_DIMS -> a pointer not 4-byte aligned FINC_ERR_ALIGNMENT -> an unknown kind, a parameter that is not positive and finite,
 * a slope_dev that is missing for the learnable kind or given for another, x_out outside mode 2, grad_slope for another kind
 * FINC_ERR_UNSUPPORTED -> a missing / short workspace where one is needed FINC_ERR_WORKSPACE -> the sticky-fault rule below.
 */
typedef enum {
    FINC_ACT_SMOOTH_LEAKY_RELU = 0,
    FINC_ACT_LEAKY_RELU = 1,
    FINC_ACT_LEARNABLE_LEAKY_RELU = 2,
    FINC_ACT_SMOOTH_TANH = 3
} FincActivationKind;
int finc_activation_supported_f32(int kind);
/* Introspection (tests; no reference counterpart): the fixed trip count of the kind's inverse as the kernels were compiled, 0 for
 * the leaky kinds, -1 for an unknown kind.  Host-only. */
int finc_debug_activation_trips(int kind);
size_t finc_activation_workspace_bytes(int B, int C, int HW);
int finc_activation_f32(int kind, float p0, float p1, const float *slope_dev, int direction, const float *x, float *y, float *logdet,
                        int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_activation_backward_f32(int kind, float p0, float p1, const float *slope_dev, int mode, const float *grad_y,
                                 const float *grad_logdet, const float *v, float *x_out, float *grad_x, float *grad_slope, int B, int C,
                                 int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream);

/*
 * The image boundary (version 115; layers/dequantize.py, layers/normalize.py, layers/transforms.py:6-19, layers/squeeze.py:5-41): what
 * every model starts with -- Dequantization, Normalization(s), LogitTransform, Squeeze -- as ONE streaming launch per direction.
 * B, C, H, W describe the IMAGE side in every call; with squeeze / unsqueeze = 1 the other side is [B][4C][H/2][W/2] in the
 * reference's channel order, side[b][4c + 2dy + dx][h][w] <-> image[b][c][2h + dy][2w + dx] (odd H or W: FINC_ERR_BAD_DIMS), with 0
 * it is [B][C][H][W].
 * finc_image_encode_u8_f32 / finc_image_encode_f32: per element, x the pixel (uint8, or fp32 holding the same numbers) and u the
 *   noise (fp32, image-shaped; NULL = 0):  yl = fma(mult, x + u, lo);  yr = fma(mult, (hi - x) - u, hi_comp);  out = log yl - log yr;
 *   logdet[b] = logdet_const + sum over the image of -(log yl + log yr).  For y = ((x + u - t1) / s1 - t2) / s2 the caller composes,
 *   in double precision, mult = 1 / (s1 s2), lo = -t1 / (s1 s2) - t2 / s2, hi = s1, hi_comp = 1 - lo - mult hi (so yr = 1 - y without
 *   ever rounding y: hi - x is exact) and logdet_const = -C H W (log s1 + log s2).  The two entry points give the same bits on the
 *   same numbers.  `logdet` [B] and the workspace are required.  out == img: allowed for fp32 pixels without squeeze, refused with
 *   squeeze (it permutes: FINC_ERR_BAD_DIMS), as is out == noise.
 * finc_image_decode_f32 / finc_image_decode_u8: z fp32 on the squeezed side;  v = fma(sigmoid(z), inv_mult, off);  the fp32 output
 *   is floor(v), not clamped (Dequantization.reverse); the uint8 output is floor(v) clamped to [0, hi - 1] (1 <= hi <= 256, else
 *   FINC_ERR_BAD_DIMS; a NaN gives 0).  `logdet` (optional; needs the workspace): logdet_const + sum over the image of |z| + 2
 *   log(1 + exp(-|z|)), the FORWARD map's log-det at the recovered value.  out == z: allowed for the fp32 output without unsqueeze.
 * The per-image sums run in a fixed order (no atomics): the same inputs give the same bits.  With squeeze a thread moves two image
 * rows of 8 pixels and four 16-byte pieces of the other side when W % 8 == 0, every fp32 tensor is 16-byte aligned and a uint8 one
 * 8-byte aligned; one 2 x 2 patch in dwords (bytes) otherwise.  Without squeeze: 16-byte pieces of four when H W % 4 == 0, fp32
 * tensors are 16-byte and a uint8 one 4-byte aligned; single elements otherwise.
 * finc_image_workspace_bytes: > 0 for any arguments, never shrinks when B, H or W grows.
 * Status: a NULL required pointer FINC_ERR_NULL_POINTER; non-positive / odd / overflowing dims (an image of 2 GiB or more as fp32),
 * squeeze other than 0 / 1 or forbidden aliasing FINC_ERR_BAD_DIMS; an fp32 pointer not 4-byte aligned FINC_ERR_ALIGNMENT; a missing
 * / short workspace where one is needed FINC_ERR_WORKSPACE -- in that order, before any HIP call; then the sticky-fault rule below.
 */
size_t finc_image_workspace_bytes(int B, int C, int H, int W, int squeeze);
int finc_image_encode_u8_f32(const uint8_t *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                             float mult, float lo, float hi, float hi_comp, float logdet_const, void *workspace, size_t workspace_bytes,
                             finc_stream_t stream);
int finc_image_encode_f32(const float *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                          float mult, float lo, float hi, float hi_comp, float logdet_const, void *workspace, size_t workspace_bytes,
                          finc_stream_t stream);
int finc_image_decode_f32(const float *z, float *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_mult, float off,
                          float hi, float logdet_const, void *workspace, size_t workspace_bytes, finc_stream_t stream);
int finc_image_decode_u8(const float *z, uint8_t *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_mult, float off,
                         float hi, float logdet_const, void *workspace, size_t workspace_bytes, finc_stream_t stream);

/*
 * Introspection (tests, diagnostics; no reference counterpart).
 * finc_inverse_kernel_variant: which MFMA inverse kernel FINC_ALGO_AUTO / finc_inverse_packed_f32 launches for this
 *   problem.  info[8] = {Cq padded to 4, waves per problem (K-split), problems per workgroup, 3 = sector pairing with
 *   helper waves (8-wave workgroups of 4 problems) / 2 = 64-byte sector pairing / 1 = 32-byte pieces / 0 = 16-byte
 *   groups, LDS bytes per workgroup, workgroups, row of the instantiation table, rows in the table}.
 *   info[3] = 4: the role-split kernel (problem sets that do not outnumber the compute units; row = -1);
 *   info[3] = 6: its short-step form for the banks of up to 16 channels (finc_chain.hip: one wave carries the recurrence on a
 *     16-row tile, one wave per tap with a + b == 2 prepares the rest, one wave owns the HBM side; row = -1);
 *   info[3] = 5: the big-bank kernel (3x3 banks with 64 < Cq <= 96, 8 waves per problem; row = -2).
 *   info[3] = 7: the streaming-bank kernel (finc_stream.hip) of every bank no table holds -- 3x3 above 96 channels per group,
 *     5x5 above 48, 2x2 above 32, 4x4, 6x6, 7x7, non-square filters above 16 channels; Cq <= 256, KH, KW <= 7: the bank
 *     streams from the L2 once per step, the solved pixels of the last KH+KW-2 steps sit in an LDS ring; info[0] = Cq padded
 *     to 16 (one-wave problems, Cq <= 48) or 64 (four waves per problem), info[1] = waves per problem; row = -3.
 *   FINC_ERR_UNSUPPORTED when the shape runs on the strict kernel.
 * finc_debug_attr_table_insert: the (device, kernel) table behind the once-per-device kernel attributes; returns 1 if
 *   the pair was new.  Host-only; exists so the key logic is testable without two GPUs.
 * finc_debug_inverse_table_row: row `row` of the MFMA inverse instantiation table, info[6] = {Cq padded, KH, KW, waves
 *   per problem, problems per workgroup, max_problems (0 = none)}; FINC_ERR_BAD_DIMS past the end.  Lets a test walk
 *   every compiled variant.
 */
int finc_inverse_kernel_variant(int B, int G, int Cq, int H, int W, int KH, int KW, int *info);
/* Which kernels finc_backward_f32 runs for this shape (16-byte aligned activations, full workspace): info[3] =
 * {grad-weight: 0 direct / 1 dword MFMA strip kernel / 2 staged (16-byte pieces through LDS) / 3 tiled (one tile pair per
 * workgroup) / 4 Winograd (3x3 banks of 13..32 channels: F(4,3) transposed, half the multiplies) / 5 Winograd on one tile pair
 * per wave (3x3 above 32 channels: F(4,3) transposed; 5x5 above 12: F(2,5) transposed), grad-input: waves per strip of the MFMA strip kernel (0 = direct kernel; > 1 = K-split), grad-input: staged form
 * (1) or dword form (0); 2 = Winograd F(2,3) along W, 3 = the big banks' M-split, 4 = Winograd F(4,3) along W, 5 = Winograd
 * F(2,5) along W (5x5 banks), 6 = Winograd F(4,3) M-split over a workgroup's waves (3x3 banks of 25 .. 64 channels), 7 = the
 * streaming-bank kernel in its forward form (the banks beyond every table; info[1] = its waves per problem)}.  Lets a parity
 * test assert WHICH kernel its numbers came from. */
int finc_debug_backward_variant(int B, int G, int Cq, int H, int W, int KH, int KW, int *info);
/* Pins the kernel family of the 3x3 forward / grad-input for this process (tests and A/B timing of each form on one shape):
 * 0 = the library's choice (default), 1 = the direct strip kernels (3x3 and 5x5), 2 = Winograd F(2,3), 4 = Winograd F(4,3).  A form a call
 * cannot take (width not a multiple of 4, unaligned activations, bank too large) still falls back to the strip kernel. */
int finc_debug_set_forward_form(int form);
/* How many images of an fp32 inverse call (FINC_ALGO_AUTO / the packed entry points) go to a SECOND launch: a problem set of whole
 * rounds of one-wave problems (1,024: four to a compute unit; 512 for the packed two-wave kernels) plus a remainder of at most 512
 * problems runs the rounds on that kernel and the remainder's images -- the last ones of the batch -- on the kernel the library picks
 * for them alone (`finc_inverse_kernel_variant` of that image count).  0: the call is one launch.  Host-only.  (The reference's
 * counterpart is the host loop of cinc_cuda_level2.cpp:19-32: 3,048 launches whatever the batch.) */
int finc_debug_inverse_remainder_images(int B, int G, int Cq, int H, int W, int KH, int KW);
/* The row-chunk count the one-wave-per-SIMD forward kernels (F(4,3), its M-split, F(2,5)) launch with: `units` strips of which the chip
 * holds `slots` at a time, maps of H rows, chunks of at least `min_rows` rows that each recompute `extra` rows of operands -- the count
 * that minimises rounds x (rows per chunk + extra).  `second_tenant` (1 .. 16): sixteenths a row costs once the launch has more units
 * than slots -- 14 for the kernels that run two waves per SIMD (strip kernel, F(2,3): slots = SIMDs, min_rows 4), 16 otherwise.
 * Host-only; 0 for arguments out of range.  (No reference counterpart: the reference's forward is one cuDNN call,
 * layers/conv.py:98-107.) */
int finc_debug_row_chunks(long long units, long long slots, int H, int min_rows, int extra, int second_tenant);
/* The grad-weight launch plan of finc_backward_f32 for this shape when grad_z and x are both aligned to `align` bytes (4, 8 or 16):
 * the plan object the launch itself runs, not a restatement of its rule.  info[10] = {form (finc_debug_backward_variant's
 * numbering; 0 = direct kernel, everything else 0 too), strip width in columns, strips per row ns, units = B * ns (what the
 * workgroups of a group walk: `for (u = slot; u < units; u += wpg)`), wpg = workgroups per group, grid.x, block.x, 16-channel tiles
 * per side of the bank, waves per workgroup of form 4 (frequency split), bytes of partial sums in the workspace}.  units > wpg: some
 * workgroup takes a second trip through its unit loop.  Host-only.  (No reference counterpart: the reference's weight gradient is
 * autograd through F.conv2d, layers/conv.py:98-107.) */
int finc_debug_gradw_plan(int B, int G, int Cq, int H, int W, int KH, int KW, int align, long long *info);
/* The forward / grad-input launch plan for this shape at that alignment, a form pinned by finc_debug_set_forward_form honoured:
 * info[6] = {form (finc_debug_backward_variant's info[2]), strip width in columns, strips per row, waves per workgroup, row chunks
 * nrc (grid.y), rows per chunk RC}: chunk c owns rows [c * RC, min(H, (c + 1) * RC)) and recomputes the operand rows above them.
 * Forms 3 and 7 have no row chunks and report nrc = 1, RC = H.  Each kernel's chunk arithmetic lives in one host function that its
 * launch and this query both call.  FINC_ERR_UNSUPPORTED: the direct kernel.  Host-only. */
int finc_debug_conv_plan(int B, int G, int Cq, int H, int W, int KH, int KW, int align, int *info);
/* The three launch rules of the per-pixel layers (everything beside the unit), and the entry-point families that fix a rule's
 * outer count (version 119). */
typedef enum {
    FINC_PIXEL_ROWS = 0,   /* grid-stride: at most 8192 workgroups of 256 threads, a thread loops with idx += gridDim.x * 256 */
    FINC_PIXEL_PARTS = 1,  /* (outer, part) workgroups: P parts share an outer unit's items, a thread loops with idx += P * 256 */
    FINC_PIXEL_MIX = 2     /* finc_mix_f32's persistent chunk loop: a wave loops with chunk += waves of the grid */
} FincPixelRule;
typedef enum {
    /* FINC_PIXEL_ROWS */
    FINC_PIXEL_CHANNEL_ROWS = 0,  /* rows of one (image, channel): finc_actnorm_f32, finc_bias_relu_f32, finc_bias_relu_bf16 (elem_bytes 2) */
    FINC_PIXEL_LEAD = 1,          /* the grouped kernel of finc_lead_product_f32: rows of one (image, group), `groups` = G */
    FINC_PIXEL_NEGATE = 2,        /* finc_negate_f32 on n = B * C * HW elements (its own cap: 1024 workgroups) */
    /* FINC_PIXEL_PARTS */
    FINC_PIXEL_TRANSFORM = 0,     /* outer = B: every coupling, split and merge transform, with or without the log-det */
    FINC_PIXEL_COUPLING_GRAD = 1, /* outer = C / 2 channel pairs: every backward of the coupling and the splits */
    FINC_PIXEL_ACTNORM_GRAD = 2,  /* outer = C channels: ActNorm's backwards and finc_actnorm_init_f32 */
    FINC_PIXEL_SPLINE = 4,        /* (version 120; 3 stays FINC_ERR_BAD_DIMS, the unknown family that callers written against 119
                                     probe with) outer = ceil(C * HW / 256) blocks of positions: every spline call, transform and
                                     backward, P = 1 and P = C * HW alike; items = 256 * B (a lane walks the images b = q, q + Q, ...),
                                     io = 1 (dwords) whatever the alignment */
    FINC_PIXEL_ACTIVATION = 5     /* (version 121) outer = B: every call of the smooth invertible activations, transform and backward;
                                     items = C * HW / io, io = 4 when C * HW % 4 == 0 (whatever HW is) and `align` is 16, else 1 */
} FincPixelFamily;
/* What a per-pixel call on [B][C][HW] would launch when every activation pointer it takes is aligned to `align` bytes (4, 8 or 16)
 * and no better, answered by the functions the launchers themselves call; launches nothing.  `elem_bytes`: 4, or 2 for the calls on
 * bf16 tensors (the coupling's raw / grad_raw, bias + ReLU's in / out).  `groups`: G of FINC_PIXEL_LEAD, ignored otherwise.
 * info[8] = {io: elements per thread item (1, 4, 8) -- the mix: pixels per lane (1, 2, 4); threads per workgroup; grid.x; parts:
 * P or Q of FINC_PIXEL_PARTS, the waves of the grid for the mix, 0 for FINC_PIXEL_ROWS; items: thread items (of one outer unit
 * under FINC_PIXEL_PARTS) -- the mix: chunks of 16 * io pixels; trips: passes the busiest thread (wave) makes through its loop;
 * outer; bytes of LDS per workgroup (the mix)}.  trips >= 2: the loop's stride is exercised.  FINC_ERR_UNSUPPORTED: no mix
 * instantiation for C -- or, for FINC_PIXEL_LEAD, there is one and the call runs the mix.  Host-only.  (No reference counterpart:
 * the reference's layers are chains of elementwise PyTorch launches, layers/{coupling,actnorm,conv1x1}.py.) */
int finc_debug_pixel_plan(int rule, int family, int groups, int B, int C, int HW, int align, int elem_bytes, long long *info);
/* What a float64 call on this shape launches, from the plan object the launchers themselves read (finc_f64.hip): info[11] = {family
 * (0: no matrix-core kernel -- the reference-order and direct kernels run, everything else 0 too; 1: one wave per problem, Cq <= 24
 * at 3x3 and <= 32 at 2x2; 2: the M-split over a workgroup's waves, 29 .. 64 channels at 3x3 and 33 .. 64 at 2x2), the padded bank
 * CQP, waves per problem and problems per workgroup of the inverse, its LDS bytes per workgroup (fixed part + FIFO slots x slot bytes)
 * and grid.x, grid.x and grid.y of the forward / grad-input, grid.x of the grad-weight, its row chunks per slab and rows per chunk}.
 * The workgroups of the forward and the grad-weight have one wave in family 1 and one per 16-row output tile (= waves per problem)
 * in family 2.  Both families carry slab and strip of the forward on grid.x (B * G * ceil(W / 16)), so grid.y is 1 wherever there is
 * a kernel -- family 1 had the slabs on grid.y until the two families' kernels became one body each; no symbol, argument list or
 * packed layout changed with that, so finc_version() did not move.  Host-only.  (The reference dispatches double for any shape on one kernel, cinc_cuda_kernel_level2.cu:117.) */
int finc_debug_f64_plan(int B, int G, int Cq, int H, int W, int KH, int KW, int *info);
int finc_debug_inverse_table_row(int row, int *info);
int finc_debug_attr_table_insert(int device, size_t kernel_token);
/* SYNCHRONOUS.  The helper-wave form of the inverse (form 3 of finc_inverse_kernel_variant) pairs each compute wave with a
 * wave that does its HBM traffic; the two meet through progress words in LDS, and every wait is bounded.  *h_count = waits
 * that gave up since the library was loaded on the current device: anything but 0 is a bug. */
int finc_debug_hlp_timeouts(unsigned *h_count);
/* A wait that gives up leaves garbage in that launch's output.  It does not pass silently: the kernel also sets a word in
 * mapped host memory, and every later launching call on that device -- finc_inverse_*, finc_forward_*, finc_mix_f32,
 * finc_backward_f32, finc_check_invariant_f32, the coupling's and ActNorm's calls, the inverse's backward -- returns FINC_ERR_LAUNCH (finc_last_hip_error() names the cause) until
 * finc_clear_fault(); no synchronisation is added to the launch path.  The word is armed by the packing calls (and by the
 * first helper-wave launch outside a stream capture).  The launch that faulted has itself returned FINC_OK (it is
 * asynchronous): callers check finc_fault_pending() at their own synchronisation points -- the Python layer does at the
 * end of FlowSequential.sample and in load_reference_checkpoint, bench.py after every timed leg. */
int finc_clear_fault(void);
/* 1 if the current device's fault word is set (host-side read of mapped memory, no synchronisation), else 0. */
int finc_fault_pending(void);
/* Run-time A/B switches in effect in this process: every FINC_* environment switch the library found SET when it looked
 * (FINC_NO_HLP, FINC_NO_S64, FINC_NO_WINO, FINC_WINO_FORM, FINC_SPLIT_MAX ...: scripts/ only) and a forward form pinned by
 * finc_debug_set_forward_form.  Returns their number and writes a comma-separated list into h_buf (n bytes, may be NULL).
 * 0 = the library's own dispatch; bench.py records the list and refuses to report a judged line otherwise. */
int finc_runtime_switches(char *h_buf, size_t n);
/* Clock probe (bench.py's per-leg `sclk_mhz`).  The chip lowers its shader clock under load by an amount that depends on
 * the data, so one kernel can take different wall times on different inputs with no code difference.  _begin starts ONE
 * wavefront on a stream of its own that samples s_memtime (shader clock) against s_memrealtime (100 MHz) every
 * `period_us` until _end, its sample budget or `max_ms` of wall time, whichever comes first -- nothing is stamped in the
 * measured kernels.  _end (SYNCHRONOUS on the probe's stream only) stops it and returns h_stats[6] = {mean MHz of the
 * window, min and max over the sampling intervals, samples, seconds covered, median MHz}.  One probe per device at a
 * time; the caller must not device-synchronise between _begin and _end (stream synchronisation is fine). */
int finc_debug_clock_probe_begin(int period_us, int max_ms);
int finc_debug_clock_probe_end(double *h_stats);

#ifdef __cplusplus
}
#endif
#endif /* FINC_H */
