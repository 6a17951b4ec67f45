// extern "C" surface of libfinc_hip.so -- see include/finc.h for the contract
// and the reference interfaces each entry point replaces.
#include "finc_common.h"

#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

namespace {

thread_local char g_hip_error[256] = "no error";

// ---- per-process tables (the only global state of the library; include/finc.h) ----
std::mutex g_table_mutex;
std::vector<std::pair<int, const void *>> g_attr_done;   // (device, kernel) pairs whose LDS attribute is set
constexpr int MAX_DEVICES = 64;
int *g_invariant_flag[MAX_DEVICES];                       // one 4-byte device word per device, allocated on first use
volatile unsigned *g_fault_host[MAX_DEVICES];             // one pinned, mapped host word per device: set by a kernel that gave up a wait
unsigned *g_fault_dev[MAX_DEVICES];                       // ... and the device's pointer to it
std::vector<std::pair<int, size_t>> g_debug_tokens;       // finc_debug_attr_table_insert's own table (never the live one)

std::atomic<bool> g_fault_armed_any{false};
std::vector<const char *> g_env_seen;                      // run-time switches found set (finc_env)

// caller holds g_table_mutex
bool attr_table_has(int device, const void *fn)
{
    for (const auto &e : g_attr_done)
        if (e.first == device && e.second == fn) return true;
    return false;
}

template <typename T>
__global__ void canonicalize_kernel(const T *__restrict__ ws, T *__restrict__ wc, int G, int Cq, int KH,
                                    int KW, unsigned orient)
{
    const int total = G * Cq * Cq * KH * KW;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int kw = idx % KW;
        const int kh = (idx / KW) % KH;
        const int rest = idx / (KW * KH); // (g*Cq + oc)*Cq + ic
        const int g = rest / (Cq * Cq);
        const unsigned o = finc_group_orient(orient, g);
        const int sh = (o & FINC_FLIP_H) ? KH - 1 - kh : kh;
        const int sw = (o & FINC_FLIP_W) ? KW - 1 - kw : kw;
        wc[idx] = ws[(rest * KH + sh) * KW + sw];
    }
}

// flag[0] = 0 if the corner tap is unit lower triangular in every group, else 1 + first bad index
template <typename T>
__global__ void invariant_kernel(const T *__restrict__ wc, int G, int Cq, int KH, int KW, int *flag)
{
    const int total = G * Cq * Cq;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int kc = idx % Cq;
        const int c = (idx / Cq) % Cq;
        if (kc < c) continue;
        const T v = wc[((size_t)idx * KH + (KH - 1)) * KW + (KW - 1)];
        const bool ok = (kc == c) ? (v == T(1)) : (v == T(0));
        if (!ok) atomicMax(flag, 1 + idx);
    }
}

int check_shape(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    if (B <= 0 || G <= 0 || Cq <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0) return FINC_ERR_BAD_DIMS;
    if (G > FINC_MAX_GROUPS || Cq > FINC_MAX_CQ || KH > 15 || KW > 15) return FINC_ERR_BAD_DIMS;
    if ((size_t)B * G * Cq * H * W >= ((size_t)1 << 40)) return FINC_ERR_BAD_DIMS;
    if ((size_t)Cq * H * W >= ((size_t)1 << 31)) return FINC_ERR_BAD_DIMS; // per-group offsets are 32-bit in-kernel
    return FINC_OK;
}

// any of the pointers off a boundary of `mask` + 1 bytes?  (nullptr, an output nobody asked for, is aligned)
template <typename... P>
inline bool off_boundary(uintptr_t mask, const P *...p) { return ((... | (uintptr_t)p) & mask) != 0; }
template <typename... P>
inline bool misaligned(const P *...p) { return off_boundary(3u, p...); }

// What the unit's entry points refuse first, in the order tests/test_abi.py pins: NULL, the dims, a pointer off its element size
// (`mask`: 3 for fp32, 7 for fp64; `bank` is held to it as a weight tensor, packed fragments have no rule), then in == out.
int unit_prelude(const void *in, const void *bank, const void *out, int B, int G, int Cq, int H, int W, int KH, int KW, uintptr_t mask,
                 bool bank_is_tensor)
{
    if (!in || !bank || !out) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    if (off_boundary(mask, in, out, bank_is_tensor ? bank : nullptr)) return FINC_ERR_ALIGNMENT;
    return in == out ? FINC_ERR_BAD_DIMS : FINC_OK;
}

} // namespace

void finc_set_hip_error(hipError_t e)
{
    strncpy(g_hip_error, hipGetErrorString(e), sizeof(g_hip_error) - 1);
    g_hip_error[sizeof(g_hip_error) - 1] = 0;
}

// A kernel's dynamic-LDS ceiling is a per-DEVICE property of the loaded code object: set it once per (device, kernel),
// whichever thread launches first (a per-thread cache would skip the second device of a process that drives two).
int finc_ensure_dynamic_lds(const void *fn, size_t bytes)
{
    if (bytes <= 48 * 1024) return FINC_OK;
    int dev = 0;
    FINC_HIP_TRY(hipGetDevice(&dev));
    // one lock over lookup, hipFuncSetAttribute and insert: a second thread on the device must not see the entry before the
    // attribute is set, and a failed call must leave no entry behind (the next launch tries again)
    std::lock_guard<std::mutex> lk(g_table_mutex);
    if (attr_table_has(dev, fn)) return FINC_OK;
    FINC_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    g_attr_done.emplace_back(dev, fn);
    return FINC_OK;
}

unsigned *finc_fault_device_word()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
    return g_fault_host[dev] ? g_fault_dev[dev] : nullptr;
}

const char *finc_env(const char *name)
{
    const char *v = getenv(name);
    if (v) {
        std::lock_guard<std::mutex> lk(g_table_mutex);
        bool seen = false;
        for (const char *n : g_env_seen) seen = seen || strcmp(n, name) == 0;
        if (!seen) g_env_seen.push_back(name);              // (string literals of the callers: they outlive the table)
    }
    return v;
}

// `arm`: publish the device's fault word if that has not happened yet.  Arming is a hipHostMalloc + a synchronous copy to a
// device symbol: both are illegal while `st` is being captured into a graph, so a capture skips it (the packing calls, which
// run before any capture of the launches, arm too); a failed step frees the word and is retried by the next arming call.
int finc_fault_gate(bool arm, hipStream_t st)
{
    if (!arm && !g_fault_armed_any.load(std::memory_order_acquire)) return FINC_OK;   // nothing armed yet: no HIP call at all
    int dev = 0;
    FINC_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return FINC_ERR_BAD_DIMS;
    volatile unsigned *w = g_fault_host[dev];
    if (!w && arm) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs == hipStreamCaptureStatusNone) {
            std::lock_guard<std::mutex> lk(g_table_mutex);
            if (!g_fault_host[dev]) {
                unsigned *h = nullptr, *d = nullptr;
                FINC_HIP_TRY(hipHostMalloc((void **)&h, sizeof(unsigned), hipHostMallocMapped));
                *h = 0;
                int e = FINC_OK;
                if (hipError_t he = hipHostGetDevicePointer((void **)&d, h, 0); he != hipSuccess) { finc_set_hip_error(he); e = FINC_ERR_LAUNCH; }
                if (!e) e = finc_mfma_arm_fault_word(d);
                if (e) { (void)hipHostFree(h); return e; }
                g_fault_dev[dev] = d;
                g_fault_host[dev] = h;
                g_fault_armed_any.store(true, std::memory_order_release);
            }
            w = g_fault_host[dev];
        }
    }
    if (w && *w != 0) {
        strncpy(g_hip_error, "a helper-wave wait of an earlier launch on this device gave up: its output is not valid (finc_clear_fault() resets)",
                sizeof(g_hip_error) - 1);
        return FINC_ERR_LAUNCH;
    }
    return FINC_OK;
}

template <typename T>
static int canonicalize(const T *w_stored, T *w_canon, int G, int Cq, int KH, int KW, unsigned orient, finc_stream_t stream)
{
    if (!w_stored || !w_canon) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(1, G, Cq, 1, 1, KH, KW)) return e;
    if (w_stored == w_canon) return FINC_ERR_BAD_DIMS;
    const int total = G * Cq * Cq * KH * KW;
    int blocks = (total + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(canonicalize_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_stored, w_canon, G,
                       Cq, KH, KW, orient);
    FINC_CHECK_LAUNCH();
    return FINC_OK;
}

extern "C" {

int finc_version(void) { return 121; }

unsigned finc_build_flags(void)
{
    return FINC_BUILD_FLAGS | finc_build_flags_mfma() | finc_build_flags_split() | finc_build_flags_chain() | finc_build_flags_f64() | finc_build_flags_conv() | finc_build_flags_gradw() | finc_build_flags_wino4m() |
           finc_build_flags_mix() | finc_build_flags_generic() | finc_build_flags_wino() | finc_build_flags_big() | finc_build_flags_probe() | finc_build_flags_wino5() | finc_build_flags_stream();
}

int finc_fault_pending(void)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return 0;
    volatile unsigned *w = g_fault_host[dev];
    return (w && *w != 0) ? 1 : 0;
}

int finc_runtime_switches(char *h_buf, size_t n)
{
    std::lock_guard<std::mutex> lk(g_table_mutex);
    size_t used = 0;
    int count = 0;
    auto put = [&](const char *t) {
        const size_t l = strlen(t);
        if (h_buf && used + l + 2 < n) {
            if (used) h_buf[used++] = ',';
            memcpy(h_buf + used, t, l);
            used += l;
        }
        ++count;
    };
    for (const char *name : g_env_seen) put(name);
    if (finc_wino_form_override() != 0) put("forward_form_override");
    if (h_buf && n) h_buf[used < n ? used : n - 1] = 0;
    return count;
}

int finc_clear_fault(void)
{
    int dev = 0;
    FINC_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return FINC_ERR_BAD_DIMS;
    if (g_fault_host[dev]) *g_fault_host[dev] = 0;
    return FINC_OK;
}

const char *finc_status_string(int status)
{
    switch (status) {
    case FINC_OK: return "ok";
    case FINC_ERR_NULL_POINTER: return "null pointer argument";
    case FINC_ERR_BAD_DIMS: return "bad dimensions";
    case FINC_ERR_UNSUPPORTED: return "requested algorithm does not support this shape";
    case FINC_ERR_WORKSPACE: return "workspace missing or too small";
    case FINC_ERR_LAUNCH: return "HIP call failed";
    case FINC_ERR_INVARIANT: return "corner tap is not unit lower triangular (layers/conv.py:63-70 invariant)";
    case FINC_ERR_ALIGNMENT: return "pointer not aligned for fp32";
    default: return "unknown status";
    }
}

const char *finc_last_hip_error(void) { return g_hip_error; }

int finc_canonicalize_weights_f32(const float *w_stored, float *w_canon, int G, int Cq, int KH, int KW,
                                  unsigned orient, finc_stream_t stream)
{
    return canonicalize<float>(w_stored, w_canon, G, Cq, KH, KW, orient, stream);
}

int finc_canonicalize_weights_f64(const double *w_stored, double *w_canon, int G, int Cq, int KH, int KW,
                                  unsigned orient, finc_stream_t stream)
{
    return canonicalize<double>(w_stored, w_canon, G, Cq, KH, KW, orient, stream);
}

extern "C++" template <typename T>
static int check_invariant(const T *w_canon, int G, int Cq, int KH, int KW, finc_stream_t stream)
{
    if (!w_canon) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(1, G, Cq, 1, 1, KH, KW)) return e;
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    FINC_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return FINC_ERR_BAD_DIMS;
    if (int e = finc_fault_gate(false)) return e;          // (a synchronous call is a natural place to report a protocol fault)
    // the call is synchronous anyway: one lock covers the lazily allocated per-device flag word and its use, so
    // concurrent checks (DataParallel replica threads) neither allocate twice nor share the word
    std::lock_guard<std::mutex> lk(g_table_mutex);
    if (!g_invariant_flag[dev]) FINC_HIP_TRY(hipMalloc(&g_invariant_flag[dev], sizeof(int)));
    int *d_flag = g_invariant_flag[dev];
    int h_flag = 0;
    FINC_HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    const int blocks = (G * Cq * Cq + 255) / 256;
    hipLaunchKernelGGL(invariant_kernel<T>, dim3(blocks), dim3(256), 0, st, w_canon, G, Cq, KH, KW, d_flag);
    FINC_CHECK_LAUNCH();
    FINC_HIP_TRY(hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    FINC_HIP_TRY(hipStreamSynchronize(st));
    return h_flag == 0 ? FINC_OK : FINC_ERR_INVARIANT;
}

int finc_check_invariant_f32(const float *w_canon, int G, int Cq, int KH, int KW, finc_stream_t stream)
{
    return check_invariant<float>(w_canon, G, Cq, KH, KW, stream);
}

int finc_check_invariant_f64(const double *w_canon, int G, int Cq, int KH, int KW, finc_stream_t stream)
{
    return check_invariant<double>(w_canon, G, Cq, KH, KW, stream);
}

int finc_debug_attr_table_insert(int device, size_t kernel_token)
{
    // the key logic of the (device, kernel) table on a table of its OWN: a test token must never land in the live table
    // (a token equal to a real kernel address would make the next launch skip its attribute)
    std::lock_guard<std::mutex> lk(g_table_mutex);
    for (const auto &e : g_debug_tokens)
        if (e.first == device && e.second == kernel_token) return 0;
    g_debug_tokens.emplace_back(device, kernel_token);
    return 1;
}

size_t finc_workspace_bytes(int G, int Cq, int KH, int KW)
{
    if (G <= 0 || Cq <= 0 || KH <= 0 || KW <= 0) return 256;
    size_t n = finc_mfma_packed_bytes(G, Cq, KH, KW);
    const size_t c = finc_conv_packed_bytes(G, Cq, KH, KW);
    if (c > n) n = c;
    return n < 256 ? 256 : n;
}

// The MFMA inverse streams rows in 16-byte pieces (W % 4 == 0).  Any other width runs on a copy whose rows are padded
// with zeros to a multiple of 8 floats -- exact (finc_generic.hip, repitch_kernel) and two cheap copies instead of the
// strict kernel's serial chain (W = 66: 0.4 ms instead of 133 ms at B=64, C=96).
static int padded_width(int Cq, int H, int W, int KH, int KW)
{
    if (W % 4 == 0 || finc_mfma_supported(Cq, H, W, KH, KW)) return 0;
    const int Wp = (W + 7) / 8 * 8;
    return finc_mfma_supported(Cq, H, Wp, KH, KW) ? Wp : 0;
}
static size_t align256(size_t n) { return (n + 255) / 256 * 256; }

size_t finc_inverse_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    size_t n = finc_workspace_bytes(G, Cq, KH, KW);
    if (B <= 0 || G <= 0 || Cq <= 0 || H <= 0 || W <= 0) return n;
    if (const int Wp = padded_width(Cq, H, W, KH, KW))
        n = align256(n) + 2 * align256((size_t)B * G * Cq * H * Wp * sizeof(float));
    return n;
}

int finc_inverse_algo_for(int Cq, int H, int W, int KH, int KW)
{
    return finc_mfma_supported(Cq, H, W, KH, KW) ? FINC_ALGO_MFMA : FINC_ALGO_STRICT;
}

int finc_forward_algo_for(int Cq, int H, int W, int KH, int KW)
{
    return finc_conv_supported(Cq, H, W, KH, KW) ? FINC_ALGO_MFMA : FINC_ALGO_STRICT;
}

static int run(const float *in, const float *w_canon, float *out, int B, int G, int Cq, int H, int W, int KH,
               int KW, unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream,
               bool forward)
{
    if (int e = unit_prelude(in, w_canon, out, B, G, Cq, H, W, KH, KW, 3, true)) return e;
    if (int e = finc_fault_gate(false)) return e;          // an earlier launch on this device gave up a protocol wait
    FincShape s{B, G, Cq, H, W, KH, KW, orient};
    hipStream_t st = (hipStream_t)stream;
    if (algo == FINC_ALGO_AUTO && !forward) {
        // a width the MFMA kernel cannot stream: solve a zero-padded copy when the caller's workspace has room for it
        const int Wp = padded_width(Cq, H, W, KH, KW);
        if (Wp && workspace && workspace_bytes >= finc_inverse_workspace_bytes(B, G, Cq, H, W, KH, KW)) {
            const size_t pk = align256(finc_workspace_bytes(G, Cq, KH, KW));
            const size_t act = align256((size_t)B * G * Cq * H * Wp * sizeof(float));
            float *zp = (float *)((char *)workspace + pk), *xp = (float *)((char *)workspace + pk + act);
            const long long rows = (long long)B * G * Cq * H;
            if (int e = finc_launch_repitch(in, zp, rows, W, Wp, st)) return e;
            if (int e = finc_mfma_pack(w_canon, nullptr, nullptr, workspace, G, Cq, KH, KW, st)) return e;
            FincShape sp{B, G, Cq, H, Wp, KH, KW, orient};
            if (int e = finc_mfma_launch(zp, workspace, xp, sp, st)) return e;
            return finc_launch_repitch(xp, out, rows, Wp, W, st);
        }
    }
    if (algo == FINC_ALGO_AUTO) {
        algo = forward ? finc_forward_algo_for(Cq, H, W, KH, KW) : finc_inverse_algo_for(Cq, H, W, KH, KW);
        // the wavefront kernel moves aligned 16-byte pieces: activations that are only 4-byte aligned take the strict kernel
        // (the role-split kernel of small problem sets has no alignment rule: the inverse plan says which kernel needs one)
        if (!forward && algo == FINC_ALGO_MFMA && ((((uintptr_t)in) | ((uintptr_t)out)) & 15u) && finc_mfma_needs_align16(s)) algo = FINC_ALGO_STRICT;
    }
    if (algo == FINC_ALGO_STRICT)
        return forward ? finc_launch_forward_generic(in, w_canon, out, s, st)
                       : finc_launch_inverse_strict(in, w_canon, out, s, st);
    if (algo != FINC_ALGO_MFMA) return FINC_ERR_UNSUPPORTED;
    if (forward) {
        if (!finc_conv_supported(Cq, H, W, KH, KW)) return FINC_ERR_UNSUPPORTED;
        if (!workspace || workspace_bytes < finc_conv_packed_bytes(G, Cq, KH, KW)) return FINC_ERR_WORKSPACE;
        if (int e = finc_conv_pack(w_canon, workspace, G, Cq, KH, KW, false, st)) return e;
        return finc_conv_launch(in, workspace, out, s, st);
    }
    if (!finc_mfma_supported(Cq, H, W, KH, KW)) return FINC_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < finc_mfma_packed_bytes(G, Cq, KH, KW)) return FINC_ERR_WORKSPACE;
    if (int e = finc_mfma_pack(w_canon, nullptr, nullptr, workspace, G, Cq, KH, KW, st)) return e;
    return finc_mfma_launch(in, workspace, out, s, st);
}

int finc_inverse_f32(const float *z, const float *w_canon, float *x, int B, int G, int Cq, int H, int W, int KH,
                     int KW, unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return run(z, w_canon, x, B, G, Cq, H, W, KH, KW, orient, algo, workspace, workspace_bytes, stream, false);
}

int finc_forward_f32(const float *x, const float *w_canon, float *z, int B, int G, int Cq, int H, int W, int KH,
                     int KW, unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return run(x, w_canon, z, B, G, Cq, H, W, KH, KW, orient, algo, workspace, workspace_bytes, stream, true);
}

// `scale`, `shift`: the per-channel affine neighbour folded into the fragments, or nullptr (the plain banks)
static int pack(const float *w_canon, const float *scale, const float *shift, void *packed, int G, int Cq, int KH, int KW,
                finc_stream_t stream, bool forward)
{
    if (!w_canon || !packed) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(1, G, Cq, 1, 1, KH, KW)) return e;
    if (forward) {
        if (finc_conv_packed_bytes(G, Cq, KH, KW) == 0) return FINC_ERR_UNSUPPORTED;
        return finc_conv_pack(w_canon, packed, G, Cq, KH, KW, false, (hipStream_t)stream, scale, shift);
    }
    if (finc_mfma_packed_bytes(G, Cq, KH, KW) == 0) return FINC_ERR_UNSUPPORTED;
    return finc_mfma_pack(w_canon, scale, shift, packed, G, Cq, KH, KW, (hipStream_t)stream);
}

int finc_pack_inverse_weights_f32(const float *w_canon, void *packed, int G, int Cq, int KH, int KW,
                                  finc_stream_t stream)
{
    return pack(w_canon, nullptr, nullptr, packed, G, Cq, KH, KW, stream, false);
}

int finc_pack_inverse_weights_affine_f32(const float *w_canon, const float *scale, const float *shift, void *packed,
                                         int G, int Cq, int KH, int KW, finc_stream_t stream)
{
    return pack(w_canon, scale, shift, packed, G, Cq, KH, KW, stream, false);
}

int finc_pack_forward_weights_f32(const float *w_canon, void *packed, int G, int Cq, int KH, int KW,
                                  finc_stream_t stream)
{
    return pack(w_canon, nullptr, nullptr, packed, G, Cq, KH, KW, stream, true);
}

int finc_pack_forward_weights_affine_f32(const float *w_canon, const float *scale, const float *shift, void *packed,
                                         int G, int Cq, int KH, int KW, finc_stream_t stream)
{
    return pack(w_canon, scale, shift, packed, G, Cq, KH, KW, stream, true);
}

static int run_packed(const float *in, const void *packed, float *out, int B, int G, int Cq, int H, int W, int KH,
                      int KW, unsigned orient, finc_stream_t stream, bool forward)
{
    if (int e = unit_prelude(in, packed, out, B, G, Cq, H, W, KH, KW, 3, false)) return e;
    if (int e = finc_fault_gate(false)) return e;
    FincShape s{B, G, Cq, H, W, KH, KW, orient};
    if (forward) {
        if (!finc_conv_supported(Cq, H, W, KH, KW)) return FINC_ERR_UNSUPPORTED;
        return finc_conv_launch(in, packed, out, s, (hipStream_t)stream);
    }
    if (!finc_mfma_supported(Cq, H, W, KH, KW)) return FINC_ERR_UNSUPPORTED;
    return finc_mfma_launch(in, packed, out, s, (hipStream_t)stream);
}

int finc_inverse_packed_f32(const float *z, const void *packed, float *x, int B, int G, int Cq, int H, int W, int KH,
                            int KW, unsigned orient, finc_stream_t stream)
{
    return run_packed(z, packed, x, B, G, Cq, H, W, KH, KW, orient, stream, false);
}

int finc_forward_packed_f32(const float *x, const void *packed, float *z, int B, int G, int Cq, int H, int W, int KH,
                            int KW, unsigned orient, finc_stream_t stream)
{
    return run_packed(x, packed, z, B, G, Cq, H, W, KH, KW, orient, stream, true);
}

int finc_inverse_affine_supported(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    if (check_shape(B, G, Cq, H, W, KH, KW)) return 0;
    return finc_mfma_affine_takes(FincShape{B, G, Cq, H, W, KH, KW, 0}) ? 1 : 0;
}

int finc_inverse_premultiplied_supported(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    if (check_shape(B, G, Cq, H, W, KH, KW)) return 0;
    return finc_mfma_zpre_takes(FincShape{B, G, Cq, H, W, KH, KW, 0}) ? 1 : 0;
}

int finc_inverse_packed_premultiplied_f32(const float *zp, const void *packed, float *x, int B, int G, int Cq, int H, int W,
                                          int KH, int KW, unsigned orient, finc_stream_t stream)
{
    if (int e = unit_prelude(zp, packed, x, B, G, Cq, H, W, KH, KW, 3, false)) return e;
    // (unlike run_packed: neither the fault gate nor finc_mfma_supported is consulted here -- a known difference)
    FincShape s{B, G, Cq, H, W, KH, KW, orient};
    return finc_mfma_launch(zp, packed, x, s, (hipStream_t)stream, true);
}

size_t finc_f64_workspace_bytes(int G, int Cq, int KH, int KW)
{
    if (G <= 0 || Cq <= 0 || KH <= 0 || KW <= 0) return 0;
    return finc_f64_packed_bytes(G, Cq, KH, KW);
}

static int run_f64_algo(const double *in, const double *w_canon, double *out, int B, int G, int Cq, int H, int W, int KH, int KW,
                        unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream, bool forward)
{
    if (int e = unit_prelude(in, w_canon, out, B, G, Cq, H, W, KH, KW, 7, true)) return e;
    if (algo != FINC_ALGO_AUTO && algo != FINC_ALGO_STRICT && algo != FINC_ALGO_MFMA) return FINC_ERR_BAD_DIMS;
    FincShape s{B, G, Cq, H, W, KH, KW, orient};
    const bool can = algo != FINC_ALGO_STRICT && finc_f64_supported(s) && workspace && ((uintptr_t)workspace & 7u) == 0 &&
                     workspace_bytes >= finc_f64_packed_bytes(G, Cq, KH, KW);
    if (!can) {
        if (algo == FINC_ALGO_MFMA) return finc_f64_supported(s) ? FINC_ERR_WORKSPACE : FINC_ERR_UNSUPPORTED;
        return forward ? finc_launch_forward_generic_f64(in, w_canon, out, s, (hipStream_t)stream)
                       : finc_launch_inverse_strict_f64(in, w_canon, out, s, (hipStream_t)stream);
    }
    if (int e = finc_fault_gate(false)) return e;
    return finc_f64_launch(in, w_canon, out, workspace, s, forward ? FINC_F64_FORWARD : FINC_F64_INVERSE, (hipStream_t)stream);
}

// the reference-order kernels: the strict path, which needs no workspace
int finc_inverse_f64(const double *z, const double *w_canon, double *x, int B, int G, int Cq, int H, int W, int KH,
                     int KW, unsigned orient, finc_stream_t stream)
{
    return run_f64_algo(z, w_canon, x, B, G, Cq, H, W, KH, KW, orient, FINC_ALGO_STRICT, nullptr, 0, stream, false);
}

int finc_forward_f64(const double *x, const double *w_canon, double *z, int B, int G, int Cq, int H, int W, int KH,
                     int KW, unsigned orient, finc_stream_t stream)
{
    return run_f64_algo(x, w_canon, z, B, G, Cq, H, W, KH, KW, orient, FINC_ALGO_STRICT, nullptr, 0, stream, true);
}

int finc_inverse_f64_algo(const double *z, const double *w_canon, double *x, int B, int G, int Cq, int H, int W, int KH, int KW,
                          unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return run_f64_algo(z, w_canon, x, B, G, Cq, H, W, KH, KW, orient, algo, workspace, workspace_bytes, stream, false);
}

int finc_forward_f64_algo(const double *x, const double *w_canon, double *z, int B, int G, int Cq, int H, int W, int KH, int KW,
                          unsigned orient, int algo, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return run_f64_algo(x, w_canon, z, B, G, Cq, H, W, KH, KW, orient, algo, workspace, workspace_bytes, stream, true);
}

int finc_inverse_kernel_variant(int B, int G, int Cq, int H, int W, int KH, int KW, int *info)
{
    if (!info) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    return finc_mfma_variant(B, G, Cq, H, W, KH, KW, info);
}

// ---- the per-pixel neighbours of the unit (finc_mix.hip, finc_coupling.h, finc_actnorm.h) ----
// Every entry point refuses in one order, which tests/test_*_host.py pin with fake pointers: NULL, then the dims (with the direction
// and the aliasing rules), then the alignment, then a channel count without a kernel, then the workspace, then the fault gate.

// counts below one; with `cap_channels`, more channels than the unit's widest layer (finc_bias_relu_f32 runs on the coupling net's
// width, which has no such cap)
static bool pixel_counts_bad(int B, int C, int HW, bool cap_channels)
{
    return B <= 0 || C <= 0 || HW <= 0 || (cap_channels && C > FINC_MAX_CQ * FINC_MAX_GROUPS);
}
static bool pixel_total_bad(int B, int C, int HW) { return (size_t)B * C * HW >= ((size_t)1 << 40); }
static int pixel_dims(int B, int C, int HW, bool cap_channels)
{
    return (pixel_counts_bad(B, C, HW, cap_channels) || pixel_total_bad(B, C, HW)) ? FINC_ERR_BAD_DIMS : FINC_OK;
}
static bool workspace_short(const void *workspace, size_t bytes, size_t need) { return !workspace || misaligned(workspace) || bytes < need; }
static size_t padded_ws_bytes(size_t n) { return n < 256 ? 256 : align256(n); }

int finc_mix_supported_f32(int C) { return (C > 0 && finc_mix_supported(C)) ? 1 : 0; }

int finc_mix_f32(const float *in, const float *mat, const float *bias, float *out, int B, int C, int HW, finc_stream_t stream)
{
    if (!in || !mat || !out) return FINC_ERR_NULL_POINTER;
    if (pixel_counts_bad(B, C, HW, true)) return FINC_ERR_BAD_DIMS;
    if (misaligned(in, mat, out, bias)) return FINC_ERR_ALIGNMENT;
    if (pixel_total_bad(B, C, HW)) return FINC_ERR_BAD_DIMS;         // (this entry point alone judges the total behind the alignment)
    if (int e = finc_fault_gate(false)) return e;
    return finc_mix_launch(in, mat, bias, out, B, C, HW, (hipStream_t)stream);
}

size_t finc_mix_backward_workspace_bytes(int B, int C, int HW)
{
    return pixel_counts_bad(B, C, HW, false) ? 256 : padded_ws_bytes(finc_mix_gradw_workspace_bytes(B, C, HW));
}

int finc_mix_backward_f32(const float *grad_out, const float *in, const float *mat, float *grad_in, float *grad_mat, float *grad_bias,
                          int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if (!grad_out || !mat || (!grad_in && !grad_mat && !grad_bias) || (grad_mat && !in)) return FINC_ERR_NULL_POINTER;
    if (int e = pixel_dims(B, C, HW, true)) return e;
    if (grad_in && (grad_in == grad_out || grad_in == in)) return FINC_ERR_BAD_DIMS;
    if (misaligned(grad_out, mat, in, grad_in, grad_mat, grad_bias)) return FINC_ERR_ALIGNMENT;
    if (!finc_mix_supported(C)) return FINC_ERR_UNSUPPORTED;
    if ((grad_mat || grad_bias) && workspace_short(workspace, workspace_bytes, finc_mix_backward_workspace_bytes(B, C, HW)))
        return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    hipStream_t st = (hipStream_t)stream;
    // grad_in = mat^T * grad_out: the forward kernel, its fragments read transposed from the same matrix
    if (grad_in)
        if (int e = finc_mix_launch(grad_out, mat, nullptr, grad_in, B, C, HW, st, true)) return e;
    // grad_mat, grad_bias: pixels on the MFMA K dimension, partial tiles in the workspace, then a fixed-order reduce (finc_gradw.hip)
    if (grad_mat || grad_bias)
        return finc_mix_gradw_launch(grad_out, in, grad_mat, grad_bias, workspace, B, C, HW, finc_align(grad_out, grad_mat ? in : grad_out),
                                     st);
    return FINC_OK;
}

int finc_coupling_supported_f32(int C) { return (C >= 2 && C % 2 == 0 && C <= FINC_MAX_CQ * FINC_MAX_GROUPS) ? 1 : 0; }

size_t finc_coupling_workspace_bytes(int B, int C, int HW)
{
    if (B <= 0 || C < 2 || HW <= 0) return 256;
    return padded_ws_bytes(finc_coupling_workspace_floats(B, C, HW) * sizeof(float));
}

// The coupling's entry points come in two families of one ladder each, and each ladder in two raw element types: float (the _f32
// names) and bf16 given as its bits (the _rawbf16_f32 names: what a net under bf16 autocast hands over).  A bf16 pointer is held to
// its 2 bytes, every other pointer to 4 as always.
static int coupling_launch(const float *x, const float *xb, const float *raw, const float *a, const float *b, float *y, float *yb,
                           float *logdet, int B, int C, int HW, int direction, bool split, float *ws, hipStream_t st)
{
    return finc_coupling_launch(x, xb, raw, a, b, y, yb, logdet, B, C, HW, direction, split, ws, st);
}
static int coupling_launch(const float *x, const float *xb, const uint16_t *raw, const float *a, const float *b, float *y, float *yb,
                           float *logdet, int B, int C, int HW, int direction, bool split, float *ws, hipStream_t st)
{
    return finc_coupling_rawbf16_launch(x, xb, raw, a, b, y, yb, logdet, B, C, HW, direction, split, ws, st);
}
static int coupling_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *gld, const float *v, const float *raw,
                                const float *a, const float *b, float *xo, float *gx, float *graw, float *ga, float *gb, int B, int C, int HW,
                                float *ws, hipStream_t st)
{
    return finc_coupling_grad_launch(mode, gy, gz, gld, v, raw, a, b, xo, gx, graw, ga, gb, B, C, HW, ws, st);
}
static int coupling_grad_launch(FincGradMode mode, const float *gy, const float *gz, const float *gld, const float *v, const uint16_t *raw,
                                const float *a, const float *b, float *xo, float *gx, uint16_t *graw, float *ga, float *gb, int B, int C,
                                int HW, float *ws, hipStream_t st)
{
    return finc_coupling_rawbf16_grad_launch(mode, gy, gz, gld, v, raw, a, b, xo, gx, graw, ga, gb, B, C, HW, ws, st);
}
// do [p, p + n) and [q, q + m) share a byte?  (nullptr shares none)
static bool bytes_overlap(const void *p, size_t n, const void *q, size_t m)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + m && b < a + n;
}
extern "C++" {
template <typename R, typename... P>
static bool raw_misaligned(const P *...p) { return off_boundary(sizeof(R) - 1, p...); }

// The transform in either direction, in one of four forms (one ladder):
//   CPL_PLAIN    logdet is optional and belongs to direction +1;
//   CPL_LOGDET   the entry point that always reports the log-det (logdet must be there, and so must the workspace);
//   CPL_SPLIT    direction +1 with two half-tensor outputs y (x1) and yb (z2) and log p, all required (finc_split_prior_f32);
//   CPL_MERGE    direction -1 with two half-tensor inputs x (x1) and xb (z2); log p optional (finc_split_prior_merge_f32).
// xb and yb are nullptr in the first two.  In the last two the whole tensor and the two halves may not overlap each other.
// `gauss` (the last two forms, fp32 raw): the Gaussianized split's arithmetic behind the same ladder (finc_gauss_split_f32,
// finc_gauss_split_merge_f32).
enum CplForm { CPL_PLAIN, CPL_LOGDET, CPL_SPLIT, CPL_MERGE };
template <typename R>
static int coupling_transform(CplForm form, const float *x, const float *xb, const R *raw, const float *a, const float *b, float *y,
                              float *yb, float *logdet, int B, int C, int HW, int direction, void *workspace, size_t workspace_bytes,
                              finc_stream_t stream, bool gauss = false)
{
    const bool split = form == CPL_SPLIT || form == CPL_MERGE;
    if (!x || !raw || !a || !b || !y || ((form == CPL_LOGDET || form == CPL_SPLIT) && !logdet) || (form == CPL_SPLIT && !yb) ||
        (form == CPL_MERGE && !xb))
        return FINC_ERR_NULL_POINTER;
    if (int e = pixel_dims(B, C, HW, true)) return e;
    if (direction != 1 && direction != -1) return FINC_ERR_BAD_DIMS;
    if ((const void *)y == (const void *)raw || (yb && (const void *)yb == (const void *)raw)) return FINC_ERR_BAD_DIMS;
    if (split) {
        const size_t hb = (size_t)B * (size_t)(C / 2) * (size_t)HW * sizeof(float), wb = (size_t)B * (size_t)C * (size_t)HW * sizeof(float);
        const void *h1 = form == CPL_SPLIT ? (const void *)y : x, *h2 = form == CPL_SPLIT ? (const void *)yb : xb;
        const void *whole = form == CPL_SPLIT ? (const void *)x : y;
        if (bytes_overlap(h1, hb, h2, hb) || bytes_overlap(h1, hb, whole, wb) || bytes_overlap(h2, hb, whole, wb)) return FINC_ERR_BAD_DIMS;
    }
    if (misaligned(x, xb, a, b, y, yb, logdet) || raw_misaligned<R>(raw)) return FINC_ERR_ALIGNMENT;
    if (!finc_coupling_supported_f32(C)) return FINC_ERR_UNSUPPORTED;
    const bool sums = form == CPL_LOGDET || form == CPL_SPLIT || (form == CPL_PLAIN ? direction > 0 && logdet : logdet != nullptr);
    if (sums && workspace_short(workspace, workspace_bytes, finc_coupling_workspace_bytes(B, C, HW))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    if constexpr (sizeof(R) == 4)
        if (gauss)
            return finc_gauss_split_launch(x, xb, raw, a, b, y, yb, sums ? logdet : nullptr, B, C, HW, direction, (float *)workspace,
                                           (hipStream_t)stream);
    return coupling_launch(x, xb, raw, a, b, y, yb, sums ? logdet : nullptr, B, C, HW, direction, split, (float *)workspace,
                           (hipStream_t)stream);
}

} // extern "C++"

int finc_coupling_f32(const float *x, const float *raw, const float *a, const float *b, float *y, float *logdet, int B, int C, int HW,
                      int direction, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_PLAIN, x, nullptr, raw, a, b, y, nullptr, logdet, B, C, HW, direction, workspace, workspace_bytes, stream);
}

int finc_coupling_rawbf16_f32(const float *x, const uint16_t *raw, const float *a, const float *b, float *y, float *logdet, int B, int C,
                              int HW, int direction, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_PLAIN, x, nullptr, raw, a, b, y, nullptr, logdet, B, C, HW, direction, workspace, workspace_bytes, stream);
}

// Every backward of the coupling: `v` is the activation the mode reads (FincGradMode), x_out the rebuilt input of FINC_GRAD_REBUILD
// alone, which also allows grad_x == grad_y (and x_out == v); no other output may be an input or another output.  grad_z belongs to
// FINC_GRAD_SPLIT (nullptr in every other mode): there grad_y and grad_z are the gradients of the two half tensors, and they and
// grad_logdet (that of log p) may each be absent, not all three.  FINC_GRAD_MERGE: grad_y is the gradient of the WHOLE tensor and v
// the merge's output; it or grad_logdet may be absent, not both; grad_x (grad_x1) and x_out (grad_z2) are HALF tensors, and no output
// may share a byte with an input or with another output.
extern "C++" {
template <typename R>
static int coupling_grad(FincGradMode mode, const float *grad_y, const float *grad_z, const float *grad_logdet, const float *v,
                         const R *raw, const float *a, const float *b, float *x_out, float *grad_x, R *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                         void *workspace, size_t workspace_bytes, finc_stream_t stream, bool gauss = false)
{
    const void *r = raw, *gr = grad_raw;
    if ((mode == FINC_GRAD_SPLIT   ? !grad_y && !grad_z && !grad_logdet
         : mode == FINC_GRAD_MERGE ? !grad_y && !grad_logdet
                                   : !grad_y) ||
        !v || !raw || !a || !b || (!x_out && !grad_x && !grad_raw && !grad_a && !grad_b))
        return FINC_ERR_NULL_POINTER;
    if (int e = pixel_dims(B, C, HW, true)) return e;
    if (mode == FINC_GRAD_MERGE) {
        const size_t n = (size_t)B * (size_t)C * (size_t)HW, wb = n * sizeof(float), hb = wb / 2, cb = (size_t)C * sizeof(float);
        const void *in[] = {grad_y, grad_logdet, v, r, a, b}, *out[] = {grad_x, x_out, gr, grad_a, grad_b};
        const size_t in_bytes[] = {wb, (size_t)B * sizeof(float), wb, n * sizeof(R), cb, cb}, out_bytes[] = {hb, hb, n * sizeof(R), cb, cb};
        for (int o = 0; o < 5; ++o) {
            for (int i = 0; i < 6; ++i)
                if (bytes_overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return FINC_ERR_BAD_DIMS;
            for (int q = 0; q < o; ++q)
                if (bytes_overlap(out[o], out_bytes[o], out[q], out_bytes[q])) return FINC_ERR_BAD_DIMS;
        }
    }
    if (x_out && (x_out == grad_y || x_out == r || x_out == grad_x || x_out == gr)) return FINC_ERR_BAD_DIMS;
    if (grad_x && ((grad_x == grad_y && mode != FINC_GRAD_REBUILD) || grad_x == grad_z || grad_x == v || grad_x == r)) return FINC_ERR_BAD_DIMS;
    if (grad_raw && (gr == grad_y || gr == grad_z || gr == v || gr == r || gr == grad_x)) return FINC_ERR_BAD_DIMS;
    if (misaligned(grad_y, grad_z, grad_logdet, v, a, b, x_out, grad_x, grad_a, grad_b) || raw_misaligned<R>(raw, grad_raw)) return FINC_ERR_ALIGNMENT;
    if (!finc_coupling_supported_f32(C)) return FINC_ERR_UNSUPPORTED;
    if ((grad_a || grad_b) && workspace_short(workspace, workspace_bytes, finc_coupling_workspace_bytes(B, C, HW)))
        return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    if constexpr (sizeof(R) == 4)
        if (gauss)                                       // (FINC_GRAD_SPLIT or FINC_GRAD_MERGE under the Gaussianized split's law)
            return finc_gauss_split_grad_launch(mode, grad_y, grad_z, grad_logdet, v, raw, a, b, x_out, grad_x, grad_raw, grad_a, grad_b, B,
                                                C, HW, (float *)workspace, (hipStream_t)stream);
    return coupling_grad_launch(mode, grad_y, grad_z, grad_logdet, v, raw, a, b, x_out, grad_x, grad_raw, grad_a, grad_b, B, C, HW,
                                (float *)workspace, (hipStream_t)stream);
}

} // extern "C++"

int finc_coupling_backward_f32(const float *grad_y, const float *grad_logdet, const float *x, const float *raw, const float *a,
                               const float *b, float *grad_x, float *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                               void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_FWD, grad_y, nullptr, grad_logdet, x, raw, a, b, nullptr, grad_x, grad_raw, grad_a, grad_b, B, C, HW, workspace,
                         workspace_bytes, stream);
}

int finc_coupling_reverse_backward_f32(const float *grad_y, const float *y, const float *raw, const float *a, const float *b,
                                       float *grad_x, float *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                                       void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return finc_coupling_reverse_logdet_backward_f32(grad_y, nullptr, y, raw, a, b, grad_x, grad_raw, grad_a, grad_b, B, C, HW, workspace,
                                                     workspace_bytes, stream);
}

int finc_coupling_reverse_logdet_f32(const float *x, const float *raw, const float *a, const float *b, float *y, float *logdet, int B,
                                     int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_LOGDET, x, nullptr, raw, a, b, y, nullptr, logdet, B, C, HW, -1, workspace, workspace_bytes, stream);
}

int finc_coupling_reverse_logdet_backward_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *raw,
                                              const float *a, const float *b, float *grad_x, float *grad_raw, float *grad_a,
                                              float *grad_b, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                              finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_REV, grad_y, nullptr, grad_logdet, y, raw, a, b, nullptr, grad_x, grad_raw, grad_a, grad_b, B, C, HW, workspace,
                         workspace_bytes, stream);
}

int finc_coupling_backward_reconstruct_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *raw, const float *a,
                                           const float *b, float *x_out, float *grad_x, float *grad_raw, float *grad_a, float *grad_b,
                                           int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_REBUILD, grad_y, nullptr, grad_logdet, y, raw, a, b, x_out, grad_x, grad_raw, grad_a, grad_b, B, C, HW, workspace,
                         workspace_bytes, stream);
}

int finc_coupling_backward_rawbf16_f32(const float *grad_y, const float *grad_logdet, const float *x, const uint16_t *raw, const float *a,
                                       const float *b, float *grad_x, uint16_t *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                                       void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_FWD, grad_y, nullptr, grad_logdet, x, raw, a, b, nullptr, grad_x, grad_raw, grad_a, grad_b, B, C, HW, workspace,
                         workspace_bytes, stream);
}

int finc_coupling_reverse_backward_rawbf16_f32(const float *grad_y, const float *y, const uint16_t *raw, const float *a, const float *b,
                                               float *grad_x, uint16_t *grad_raw, float *grad_a, float *grad_b, int B, int C, int HW,
                                               void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return finc_coupling_reverse_logdet_backward_rawbf16_f32(grad_y, nullptr, y, raw, a, b, grad_x, grad_raw, grad_a, grad_b, B, C, HW,
                                                             workspace, workspace_bytes, stream);
}

int finc_coupling_reverse_logdet_rawbf16_f32(const float *x, const uint16_t *raw, const float *a, const float *b, float *y, float *logdet,
                                             int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_LOGDET, x, nullptr, raw, a, b, y, nullptr, logdet, B, C, HW, -1, workspace, workspace_bytes, stream);
}

int finc_coupling_reverse_logdet_backward_rawbf16_f32(const float *grad_y, const float *grad_logdet, const float *y, const uint16_t *raw,
                                                      const float *a, const float *b, float *grad_x, uint16_t *grad_raw, float *grad_a,
                                                      float *grad_b, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                                      finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_REV, grad_y, nullptr, grad_logdet, y, raw, a, b, nullptr, grad_x, grad_raw, grad_a, grad_b, B, C, HW, workspace,
                         workspace_bytes, stream);
}

int finc_coupling_backward_reconstruct_rawbf16_f32(const float *grad_y, const float *grad_logdet, const float *y, const uint16_t *raw,
                                                   const float *a, const float *b, float *x_out, float *grad_x, uint16_t *grad_raw,
                                                   float *grad_a, float *grad_b, int B, int C, int HW, void *workspace,
                                                   size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_REBUILD, grad_y, nullptr, grad_logdet, y, raw, a, b, x_out, grad_x, grad_raw, grad_a, grad_b, B, C, HW, workspace,
                         workspace_bytes, stream);
}

// The split prior with its latent: the transform's ladder in its two split forms, the backward's ladder in its fourth mode.
int finc_split_prior_f32(const float *x, const float *raw, const float *a, const float *b, float *x1, float *z2, float *log_p, int B, int C,
                         int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_SPLIT, x, nullptr, raw, a, b, x1, z2, log_p, B, C, HW, 1, workspace, workspace_bytes, stream);
}

int finc_split_prior_rawbf16_f32(const float *x, const uint16_t *raw, const float *a, const float *b, float *x1, float *z2, float *log_p,
                                 int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_SPLIT, x, nullptr, raw, a, b, x1, z2, log_p, B, C, HW, 1, workspace, workspace_bytes, stream);
}

int finc_split_prior_merge_f32(const float *x1, const float *z2, const float *raw, const float *a, const float *b, float *x, float *log_p,
                               int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_MERGE, x1, z2, raw, a, b, x, nullptr, log_p, B, C, HW, -1, workspace, workspace_bytes, stream);
}

int finc_split_prior_merge_rawbf16_f32(const float *x1, const float *z2, const uint16_t *raw, const float *a, const float *b, float *x,
                                       float *log_p, int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_MERGE, x1, z2, raw, a, b, x, nullptr, log_p, B, C, HW, -1, workspace, workspace_bytes, stream);
}

int finc_split_prior_backward_f32(const float *grad_x1, const float *grad_z2, const float *grad_log_p, const float *x, const float *raw,
                                  const float *a, const float *b, float *grad_x, float *grad_raw, float *grad_a, float *grad_b, int B,
                                  int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_SPLIT, grad_x1, grad_z2, grad_log_p, x, raw, a, b, nullptr, grad_x, grad_raw, grad_a, grad_b, B, C, HW,
                         workspace, workspace_bytes, stream);
}

int finc_split_prior_backward_rawbf16_f32(const float *grad_x1, const float *grad_z2, const float *grad_log_p, const float *x,
                                          const uint16_t *raw, const float *a, const float *b, float *grad_x, uint16_t *grad_raw,
                                          float *grad_a, float *grad_b, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                          finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_SPLIT, grad_x1, grad_z2, grad_log_p, x, raw, a, b, nullptr, grad_x, grad_raw, grad_a, grad_b, B, C, HW,
                         workspace, workspace_bytes, stream);
}

// The Gaussianized split (glow.Split): the split prior's two ladders, in front of the kernels of the other arithmetic law.
int finc_gauss_split_f32(const float *x, const float *raw, const float *a, const float *b, float *x1, float *z2, float *log_p, int B, int C,
                         int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_SPLIT, x, nullptr, raw, a, b, x1, z2, log_p, B, C, HW, 1, workspace, workspace_bytes, stream, true);
}

int finc_gauss_split_merge_f32(const float *x1, const float *z2, const float *raw, const float *a, const float *b, float *x, float *log_p,
                               int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_transform(CPL_MERGE, x1, z2, raw, a, b, x, nullptr, log_p, B, C, HW, -1, workspace, workspace_bytes, stream, true);
}

int finc_gauss_split_backward_f32(const float *grad_x1, const float *grad_z2, const float *grad_log_p, const float *x, const float *raw,
                                  const float *a, const float *b, float *grad_x, float *grad_raw, float *grad_a, float *grad_b, int B,
                                  int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_SPLIT, grad_x1, grad_z2, grad_log_p, x, raw, a, b, nullptr, grad_x, grad_raw, grad_a, grad_b, B, C, HW,
                         workspace, workspace_bytes, stream, true);
}

// The backward of the two merges, from the merge's OUTPUT: the backward's ladder in its fifth mode, under either law.
int finc_split_prior_merge_backward_f32(const float *grad_x, const float *grad_log_p, const float *x, const float *raw, const float *a,
                                        const float *b, float *grad_x1, float *grad_z2, float *grad_raw, float *grad_a, float *grad_b,
                                        int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_MERGE, grad_x, nullptr, grad_log_p, x, raw, a, b, grad_z2, grad_x1, grad_raw, grad_a, grad_b, B, C, HW,
                         workspace, workspace_bytes, stream);
}

int finc_split_prior_merge_backward_rawbf16_f32(const float *grad_x, const float *grad_log_p, const float *x, const uint16_t *raw,
                                                const float *a, const float *b, float *grad_x1, float *grad_z2, uint16_t *grad_raw,
                                                float *grad_a, float *grad_b, int B, int C, int HW, void *workspace,
                                                size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_MERGE, grad_x, nullptr, grad_log_p, x, raw, a, b, grad_z2, grad_x1, grad_raw, grad_a, grad_b, B, C, HW,
                         workspace, workspace_bytes, stream);
}

int finc_gauss_split_merge_backward_f32(const float *grad_x, const float *grad_log_p, const float *x, const float *raw, const float *a,
                                        const float *b, float *grad_x1, float *grad_z2, float *grad_raw, float *grad_a, float *grad_b,
                                        int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return coupling_grad(FINC_GRAD_MERGE, grad_x, nullptr, grad_log_p, x, raw, a, b, grad_z2, grad_x1, grad_raw, grad_a, grad_b, B, C, HW,
                         workspace, workspace_bytes, stream, true);
}

// bias + ReLU on fp32 or on bf16 bits (the bias is fp32 in both): one ladder
extern "C++" {
template <typename T>
static int bias_relu(const T *in, const float *bias, T *out, int B, int C, int HW, finc_stream_t stream)
{
    if (!in || !bias || !out) return FINC_ERR_NULL_POINTER;
    if (int e = pixel_dims(B, C, HW, false)) return e;
    if (misaligned(bias) || raw_misaligned<T>(in, out)) return FINC_ERR_ALIGNMENT;
    if (int e = finc_fault_gate(false)) return e;
    if constexpr (sizeof(T) == 2)
        return finc_bias_relu_bf16_launch(in, bias, out, B, C, HW, (hipStream_t)stream);
    else
        return finc_bias_relu_launch(in, bias, out, B, C, HW, (hipStream_t)stream);
}

} // extern "C++"

int finc_bias_relu_f32(const float *in, const float *bias, float *out, int B, int C, int HW, finc_stream_t stream)
{
    return bias_relu(in, bias, out, B, C, HW, stream);
}

int finc_bias_relu_bf16(const uint16_t *in, const float *bias, uint16_t *out, int B, int C, int HW, finc_stream_t stream)
{
    return bias_relu(in, bias, out, B, C, HW, stream);
}

// ---- the image boundary (finc_image.h): B, C, H, W are the image's; `squeeze` 1: the other side is [B][4C][H/2][W/2] ----
static int image_dims(int B, int C, int H, int W, int squeeze)
{
    if (H <= 0 || W <= 0 || (long long)H * W >= (1LL << 31)) return FINC_ERR_BAD_DIMS;
    if (int e = pixel_dims(B, C, H * W, false)) return e;
    if ((squeeze != 0 && squeeze != 1) || (squeeze && (H % 2 || W % 2))) return FINC_ERR_BAD_DIMS;
    return (size_t)C * H * W * 4 >= ((size_t)1 << 31) ? FINC_ERR_BAD_DIMS : FINC_OK;           // (cpl_launch's limit: int offsets per image)
}

size_t finc_image_workspace_bytes(int B, int C, int H, int W, int squeeze)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 256;
    return padded_ws_bytes(finc_image_workspace_floats(B, C, H, W, squeeze) * sizeof(float));
}

extern "C++" {
static int image_encode_launch(const uint8_t *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                               float m, float c, float hi, float c2, float ldc, float *ws, hipStream_t st)
{
    return finc_image_encode_u8_launch(img, noise, out, logdet, B, C, H, W, squeeze, m, c, hi, c2, ldc, ws, st);
}
static int image_encode_launch(const float *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                               float m, float c, float hi, float c2, float ldc, float *ws, hipStream_t st)
{
    return finc_image_encode_f32_launch(img, noise, out, logdet, B, C, H, W, squeeze, m, c, hi, c2, ldc, ws, st);
}
static int image_decode_launch(const float *z, uint8_t *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off,
                               float hi, float ldc, float *ws, hipStream_t st)
{
    return finc_image_decode_u8_launch(z, out, logdet, B, C, H, W, unsqueeze, inv_m, off, hi, ldc, ws, st);
}
static int image_decode_launch(const float *z, float *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off,
                               float hi, float ldc, float *ws, hipStream_t st)
{
    return finc_image_decode_f32_launch(z, out, logdet, B, C, H, W, unsqueeze, inv_m, off, hi, ldc, ws, st);
}

// One ladder per direction, T the pixel type (uint8_t, float).  In place (out on the input) only where nothing is permuted and both
// sides are fp32; a uint8 tensor has no alignment rule.
template <typename T>
static int image_encode(const T *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze, float m,
                        float c, float hi, float c2, float ldc, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if (!img || !out || !logdet) return FINC_ERR_NULL_POINTER;
    if (int e = image_dims(B, C, H, W, squeeze)) return e;
    if ((squeeze || sizeof(T) != 4) && ((const void *)out == (const void *)img)) return FINC_ERR_BAD_DIMS;
    if (squeeze && out == noise) return FINC_ERR_BAD_DIMS;
    if (misaligned(noise, out, logdet) || (sizeof(T) == 4 && misaligned(img))) return FINC_ERR_ALIGNMENT;
    if (workspace_short(workspace, workspace_bytes, finc_image_workspace_bytes(B, C, H, W, squeeze))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return image_encode_launch(img, noise, out, logdet, B, C, H, W, squeeze, m, c, hi, c2, ldc, (float *)workspace, (hipStream_t)stream);
}

template <typename T>
static int image_decode(const float *z, T *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_m, float off, float hi,
                        float ldc, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if (!z || !out) return FINC_ERR_NULL_POINTER;
    if (int e = image_dims(B, C, H, W, unsqueeze)) return e;
    if (sizeof(T) == 1 && !(hi >= 1.f && hi <= 256.f)) return FINC_ERR_BAD_DIMS;                 // the clamp's top must fit a byte
    if ((unsqueeze || sizeof(T) != 4) && ((const void *)out == (const void *)z)) return FINC_ERR_BAD_DIMS;
    if (misaligned(z, logdet) || (sizeof(T) == 4 && misaligned(out))) return FINC_ERR_ALIGNMENT;
    if (logdet && workspace_short(workspace, workspace_bytes, finc_image_workspace_bytes(B, C, H, W, unsqueeze))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return image_decode_launch(z, out, logdet, B, C, H, W, unsqueeze, inv_m, off, hi, ldc, (float *)workspace, (hipStream_t)stream);
}
} // extern "C++"

int finc_image_encode_u8_f32(const uint8_t *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze,
                             float mult, float lo, float hi, float hi_comp, float logdet_const, void *workspace, size_t workspace_bytes,
                             finc_stream_t stream)
{
    return image_encode(img, noise, out, logdet, B, C, H, W, squeeze, mult, lo, hi, hi_comp, logdet_const, workspace, workspace_bytes, stream);
}

int finc_image_encode_f32(const float *img, const float *noise, float *out, float *logdet, int B, int C, int H, int W, int squeeze, float mult,
                          float lo, float hi, float hi_comp, float logdet_const, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return image_encode(img, noise, out, logdet, B, C, H, W, squeeze, mult, lo, hi, hi_comp, logdet_const, workspace, workspace_bytes, stream);
}

int finc_image_decode_f32(const float *z, float *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_mult, float off,
                          float hi, float logdet_const, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return image_decode(z, out, logdet, B, C, H, W, unsqueeze, inv_mult, off, hi, logdet_const, workspace, workspace_bytes, stream);
}

int finc_image_decode_u8(const float *z, uint8_t *out, float *logdet, int B, int C, int H, int W, int unsqueeze, float inv_mult, float off,
                         float hi, float logdet_const, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    return image_decode(z, out, logdet, B, C, H, W, unsqueeze, inv_mult, off, hi, logdet_const, workspace, workspace_bytes, stream);
}

size_t finc_actnorm_workspace_bytes(int B, int C, int HW)
{
    return pixel_counts_bad(B, C, HW, false) ? 256 : padded_ws_bytes(finc_actnorm_workspace_floats(B, C, HW) * sizeof(float));
}

int finc_actnorm_f32(const float *x, const float *log_scale, const float *translation, float *y, float *logdet, int B, int C, int HW,
                     int direction, finc_stream_t stream)
{
    if (!x || !log_scale || !translation || !y) return FINC_ERR_NULL_POINTER;
    if (int e = pixel_dims(B, C, HW, true)) return e;
    if (direction != 1 && direction != -1) return FINC_ERR_BAD_DIMS;
    if (misaligned(x, log_scale, translation, y, logdet)) return FINC_ERR_ALIGNMENT;
    if (int e = finc_fault_gate(false)) return e;
    return finc_actnorm_launch(x, log_scale, translation, y, direction > 0 ? logdet : nullptr, B, C, HW, direction, (hipStream_t)stream);
}

// Every backward of ActNorm: `v` is the activation the mode reads (FincGradMode), translation and x_out belong to FINC_GRAD_REBUILD
// alone.  grad_x == grad_y and x_out == v are the two allowed overlaps.
static int actnorm_grad(FincGradMode mode, const float *grad_y, const float *grad_logdet, const float *v, const float *log_scale,
                        const float *translation, float *x_out, float *grad_x, float *grad_log_scale, float *grad_translation, int B, int C,
                        int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if (!grad_y || !v || !log_scale || (x_out && !translation) || (!x_out && !grad_x && !grad_log_scale && !grad_translation))
        return FINC_ERR_NULL_POINTER;
    if (int e = pixel_dims(B, C, HW, true)) return e;
    if (x_out && (x_out == grad_y || x_out == grad_x)) return FINC_ERR_BAD_DIMS;
    if (grad_x && grad_x == v) return FINC_ERR_BAD_DIMS;
    if (misaligned(grad_y, grad_logdet, v, log_scale, translation, x_out, grad_x, grad_log_scale, grad_translation)) return FINC_ERR_ALIGNMENT;
    if ((grad_log_scale || grad_translation) && workspace_short(workspace, workspace_bytes, finc_actnorm_workspace_bytes(B, C, HW)))
        return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return finc_actnorm_grad_launch(mode, grad_y, grad_logdet, v, log_scale, translation, x_out, grad_x, grad_log_scale, grad_translation, B,
                                    C, HW, (float *)workspace, (hipStream_t)stream);
}

int finc_actnorm_backward_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *log_scale, float *grad_x,
                              float *grad_log_scale, float *grad_translation, int B, int C, int HW, void *workspace,
                              size_t workspace_bytes, finc_stream_t stream)
{
    return actnorm_grad(FINC_GRAD_FWD, grad_y, grad_logdet, y, log_scale, nullptr, nullptr, grad_x, grad_log_scale, grad_translation, B, C, HW,
                        workspace, workspace_bytes, stream);
}

int finc_actnorm_backward_reconstruct_f32(const float *grad_y, const float *grad_logdet, const float *y, const float *log_scale,
                                          const float *translation, float *x_out, float *grad_x, float *grad_log_scale,
                                          float *grad_translation, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                          finc_stream_t stream)
{
    return actnorm_grad(FINC_GRAD_REBUILD, grad_y, grad_logdet, y, log_scale, translation, x_out, grad_x, grad_log_scale, grad_translation, B,
                        C, HW, workspace, workspace_bytes, stream);
}

int finc_actnorm_reverse_backward_f32(const float *grad_y, const float *x, const float *log_scale, float *grad_x, float *grad_log_scale,
                                      float *grad_translation, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                                      finc_stream_t stream)
{
    return actnorm_grad(FINC_GRAD_REV, grad_y, nullptr, x, log_scale, nullptr, nullptr, grad_x, grad_log_scale, grad_translation, B, C, HW,
                        workspace, workspace_bytes, stream);
}

int finc_actnorm_init_f32(const float *x, float *log_scale, float *translation, int B, int C, int HW, void *workspace,
                          size_t workspace_bytes, finc_stream_t stream)
{
    if (!x || !log_scale || !translation) return FINC_ERR_NULL_POINTER;
    if (int e = pixel_dims(B, C, HW, true)) return e;
    if ((long long)B * HW < 2) return FINC_ERR_BAD_DIMS;             // the unbiased deviation of one value (torch.std: NaN)
    if (log_scale == translation) return FINC_ERR_BAD_DIMS;
    if (misaligned(x, log_scale, translation)) return FINC_ERR_ALIGNMENT;
    if (workspace_short(workspace, workspace_bytes, finc_actnorm_workspace_bytes(B, C, HW))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return finc_actnorm_init_launch(x, log_scale, translation, B, C, HW, (float *)workspace, (hipStream_t)stream);
}

// ---- the rational-quadratic spline (finc_spline.h) ----
int finc_spline_supported_f32(int K) { return (K >= 2 && K <= 16) ? 1 : 0; }

static bool spline_table_bad(int C, int HW, int K, int P) { return !finc_spline_supported_f32(K) || (P != 1 && (long long)P != (long long)C * HW); }

size_t finc_spline_workspace_bytes(int B, int C, int HW, int K, int P)
{
    if (pixel_counts_bad(B, C, HW, false) || spline_table_bad(C, HW, K, P)) return 256;
    return padded_ws_bytes(finc_spline_workspace_floats(B, C, HW, K, P) * sizeof(float));
}

// (C * HW * 4 >= 2^31 is the launcher's FINC_ERR_BAD_DIMS; judged here so that it comes before the alignment)
static int spline_dims(int B, int C, int HW, float tail_bound)
{
    if (int e = pixel_dims(B, C, HW, false)) return e;
    if ((size_t)C * HW * 4 >= ((size_t)1 << 31)) return FINC_ERR_BAD_DIMS;
    return (tail_bound > 0.f && tail_bound < INFINITY) ? FINC_OK : FINC_ERR_BAD_DIMS;
}

int finc_spline_f32(const float *x, const float *table, int P, int K, float tail_bound, int direction, float *y, float *logdet, int B,
                    int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if (!x || !table || !y) return FINC_ERR_NULL_POINTER;
    if (int e = spline_dims(B, C, HW, tail_bound)) return e;
    if (direction != 1 && direction != -1) return FINC_ERR_BAD_DIMS;
    if (misaligned(x, table, y, logdet)) return FINC_ERR_ALIGNMENT;
    if (spline_table_bad(C, HW, K, P)) return FINC_ERR_UNSUPPORTED;
    if (logdet && workspace_short(workspace, workspace_bytes, finc_spline_workspace_bytes(B, C, HW, K, P))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return finc_spline_launch(x, table, P, K, tail_bound, direction, y, logdet, B, C, HW, (float *)workspace, (hipStream_t)stream);
}

// Both backwards of the spline: `x` is the input of the pass the mode differentiates (FincGradMode).  grad_x == grad_y is the one
// allowed overlap.
static int spline_grad(FincGradMode mode, const float *grad_y, const float *grad_logdet, const float *x, const float *table, int P, int K,
                       float tail_bound, float *grad_x, float *grad_table, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                       finc_stream_t stream)
{
    if ((!grad_y && !grad_logdet) || !x || !table || (!grad_x && !grad_table)) return FINC_ERR_NULL_POINTER;
    if (int e = spline_dims(B, C, HW, tail_bound)) return e;
    if (grad_x && grad_x == x) return FINC_ERR_BAD_DIMS;
    if (misaligned(grad_y, grad_logdet, x, table, grad_x, grad_table)) return FINC_ERR_ALIGNMENT;
    if (spline_table_bad(C, HW, K, P)) return FINC_ERR_UNSUPPORTED;
    if (grad_table && workspace_short(workspace, workspace_bytes, finc_spline_workspace_bytes(B, C, HW, K, P))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return finc_spline_grad_launch(mode, grad_y, grad_logdet, x, table, P, K, tail_bound, grad_x, grad_table, B, C, HW, (float *)workspace,
                                   (hipStream_t)stream);
}

int finc_spline_backward_f32(const float *grad_y, const float *grad_logdet, const float *x, const float *table, int P, int K,
                             float tail_bound, float *grad_x, float *grad_table, int B, int C, int HW, void *workspace,
                             size_t workspace_bytes, finc_stream_t stream)
{
    return spline_grad(FINC_GRAD_FWD, grad_y, grad_logdet, x, table, P, K, tail_bound, grad_x, grad_table, B, C, HW, workspace, workspace_bytes,
                       stream);
}

int finc_spline_reverse_backward_f32(const float *grad_y, const float *grad_logdet, const float *x, const float *table, int P, int K,
                                     float tail_bound, float *grad_x, float *grad_table, int B, int C, int HW, void *workspace,
                                     size_t workspace_bytes, finc_stream_t stream)
{
    return spline_grad(FINC_GRAD_REV, grad_y, grad_logdet, x, table, P, K, tail_bound, grad_x, grad_table, B, C, HW, workspace, workspace_bytes,
                       stream);
}

// ---- the smooth invertible activations (finc_activation.h) ----
int finc_activation_supported_f32(int kind) { return finc_activation_trips(kind) >= 0 ? 1 : 0; }
int finc_debug_activation_trips(int kind) { return finc_activation_trips(kind); }

size_t finc_activation_workspace_bytes(int B, int C, int HW)
{
    return pixel_counts_bad(B, C, HW, false) ? 256 : padded_ws_bytes(finc_activation_workspace_floats(B, C, HW) * sizeof(float));
}

// (C * HW * 4 >= 2^31 is the launcher's FINC_ERR_BAD_DIMS; judged here so that it comes before the alignment)
static int activation_dims(int B, int C, int HW)
{
    if (int e = pixel_dims(B, C, HW, false)) return e;
    return (size_t)C * HW * 4 >= ((size_t)1 << 31) ? FINC_ERR_BAD_DIMS : FINC_OK;
}

// the host's parameter checks: a > 0 (and b > 0 for the smooth tanh), finite; the slope pointer for the learnable kind and no other
static bool activation_kind_bad(int kind, float p0, float p1, const float *slope_dev)
{
    if (!finc_activation_supported_f32(kind)) return true;
    if (kind == FINC_ACT_LEARNABLE_LEAKY_RELU) return !slope_dev;
    if (slope_dev || !(p0 > 0.f && p0 < INFINITY)) return true;
    return kind == FINC_ACT_SMOOTH_TANH && !(p1 > 0.f && p1 < INFINITY);
}

int finc_activation_f32(int kind, float p0, float p1, const float *slope_dev, int direction, const float *x, float *y, float *logdet,
                        int B, int C, int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if (!x || !y) return FINC_ERR_NULL_POINTER;
    if (int e = activation_dims(B, C, HW)) return e;
    if (direction != 1 && direction != -1) return FINC_ERR_BAD_DIMS;
    if (misaligned(x, y, logdet, slope_dev)) return FINC_ERR_ALIGNMENT;
    if (activation_kind_bad(kind, p0, p1, slope_dev)) return FINC_ERR_UNSUPPORTED;
    if (logdet && workspace_short(workspace, workspace_bytes, finc_activation_workspace_bytes(B, C, HW))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return finc_activation_launch(kind, p0, p1, slope_dev, direction, x, y, logdet, B, C, HW, (float *)workspace, (hipStream_t)stream);
}

// Every backward of the activations: `v` is the activation the mode reads (FincGradMode).  grad_x == grad_y and x_out == v are the two
// allowed overlaps.
int finc_activation_backward_f32(int kind, float p0, float p1, const float *slope_dev, int mode, const float *grad_y,
                                 const float *grad_logdet, const float *v, float *x_out, float *grad_x, float *grad_slope, int B, int C,
                                 int HW, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if ((!grad_y && !grad_logdet) || !v || (!x_out && !grad_x && !grad_slope)) return FINC_ERR_NULL_POINTER;
    if (int e = activation_dims(B, C, HW)) return e;
    if (mode != FINC_GRAD_FWD && mode != FINC_GRAD_REV && mode != FINC_GRAD_REBUILD) return FINC_ERR_BAD_DIMS;
    if (grad_x && grad_x == v) return FINC_ERR_BAD_DIMS;
    if (x_out && (x_out == grad_y || x_out == grad_x)) return FINC_ERR_BAD_DIMS;
    if (misaligned(grad_y, grad_logdet, v, x_out, grad_x, grad_slope, slope_dev)) return FINC_ERR_ALIGNMENT;
    if (activation_kind_bad(kind, p0, p1, slope_dev)) return FINC_ERR_UNSUPPORTED;
    if ((x_out && mode != FINC_GRAD_REBUILD) || (grad_slope && kind != FINC_ACT_LEARNABLE_LEAKY_RELU)) return FINC_ERR_UNSUPPORTED;
    if (grad_slope && workspace_short(workspace, workspace_bytes, finc_activation_workspace_bytes(B, C, HW))) return FINC_ERR_WORKSPACE;
    if (int e = finc_fault_gate(false)) return e;
    return finc_activation_grad_launch(kind, p0, p1, slope_dev, (FincGradMode)mode, grad_y, grad_logdet, v, x_out, grad_x, grad_slope, B, C,
                                       HW, (float *)workspace, (hipStream_t)stream);
}

int finc_debug_backward_variant(int B, int G, int Cq, int H, int W, int KH, int KW, int *info)
{
    if (!info) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    FincShape s{B, G, Cq, H, W, KH, KW, 0};
    info[0] = finc_gradw_variant(s);
    int c[3] = {0, 0, 0};
    const bool mfma = finc_conv_variant(B, G, Cq, H, W, KH, KW, c) == FINC_OK;
    info[1] = mfma ? c[0] : 0;
    info[2] = mfma ? c[1] : 0;
    return FINC_OK;
}

// (both plan queries answer from the object the launch runs: finc_gradw_plan, conv_plan and the kernels' FincRowPlan functions)
int finc_debug_gradw_plan(int B, int G, int Cq, int H, int W, int KH, int KW, int align, long long *info)
{
    if (!info) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    if (align != 4 && align != 8 && align != 16) return FINC_ERR_BAD_DIMS;
    const FincGradwPlan p = finc_gradw_plan(FincShape{B, G, Cq, H, W, KH, KW, 0}, align);
    const long long v[10] = {p.form, p.strip, p.ns, (long long)B * p.ns, p.wpg, (long long)p.grid.x, (long long)p.block.x, p.mtt, p.fs,
                             (long long)p.bytes};
    for (int k = 0; k < 10; ++k) info[k] = p.form ? v[k] : 0;
    return FINC_OK;
}

int finc_debug_conv_plan(int B, int G, int Cq, int H, int W, int KH, int KW, int align, int *info)
{
    if (!info) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    if (align != 4 && align != 8 && align != 16) return FINC_ERR_BAD_DIMS;
    return finc_conv_plan_info(FincShape{B, G, Cq, H, W, KH, KW, 0}, align, info);
}

// (answers from the functions the per-pixel launchers call: finc_mix.hip finc_pixel_plan_info)
int finc_debug_pixel_plan(int rule, int family, int groups, int B, int C, int HW, int align, int elem_bytes, long long *info)
{
    if (!info) return FINC_ERR_NULL_POINTER;
    if (B < 1 || C < 1 || HW < 1) return FINC_ERR_BAD_DIMS;
    if (align != 4 && align != 8 && align != 16) return FINC_ERR_BAD_DIMS;
    if (elem_bytes != 4 && elem_bytes != 2) return FINC_ERR_BAD_DIMS;
    return finc_pixel_plan_info(rule, family, groups, B, C, HW, align, elem_bytes, info);
}

int finc_debug_f64_plan(int B, int G, int Cq, int H, int W, int KH, int KW, int *info)
{
    if (!info) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    const FincShape s{B, G, Cq, H, W, KH, KW, 0};
    const FincF64Plan p = finc_f64_plan(s);
    const FincF64GradwPlan gw = finc_f64_gradw_plan(s);
    const long long v[11] = {p.family, p.cqp, p.waves, p.ppw, p.lds, p.inv_grid, p.fwd_grid_x, p.fwd_grid_y, p.waves ? gw.waves / p.waves : 0, gw.nrc, gw.RC};
    for (int k = 0; k < 11; ++k) info[k] = p.family ? (int)v[k] : 0;
    return FINC_OK;
}

int finc_debug_set_forward_form(int form) { return finc_wino_set_form(form); }

int finc_debug_inverse_remainder_images(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    if (B < 1 || G < 1 || Cq < 1 || H < 1 || W < 1 || KH < 1 || KW < 1) return 0;
    return finc_mfma_remainder_images(FincShape{B, G, Cq, H, W, KH, KW, 0});
}

int finc_debug_row_chunks(long long units, long long slots, int H, int min_rows, int extra, int second_tenant)
{
    if (units < 1 || slots < 1 || H < 1 || min_rows < 1 || extra < 0 || second_tenant < 1 || second_tenant > 16) return 0;
    return finc_row_chunks(units, slots, H, min_rows, extra, second_tenant);
}

int finc_debug_hlp_timeouts(unsigned *h_count)
{
    if (!h_count) return FINC_ERR_NULL_POINTER;
    unsigned a = 0, b = 0;
    if (int e = finc_mfma_hlp_timeouts(&a)) return e;          // helper-wave protocol (finc_mfma.hip)
    if (int e = finc_split_timeouts_count(&b)) return e;       // band split's progress words (finc_split.hip)
    *h_count = a + b;
    return FINC_OK;
}

int finc_debug_inverse_table_row(int row, int *info)
{
    if (!info) return FINC_ERR_NULL_POINTER;
    return finc_mfma_table_row(row, info);
}

// the backward's workspace: the grad-input bank (finc_conv_pack), then the grad-weight partials from the next 256-byte boundary
struct BackwardWorkspace { size_t bank, partials; };
static BackwardWorkspace backward_workspace(const FincShape &s)
{
    return {align256(finc_conv_packed_bytes(s.G, s.Cq, s.KH, s.KW)), finc_gradw_workspace_bytes(s)};
}

size_t finc_backward_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    if (B <= 0 || G <= 0 || Cq <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0) return 256;
    const BackwardWorkspace ws = backward_workspace(FincShape{B, G, Cq, H, W, KH, KW, 0});
    const size_t n = ws.bank + ws.partials;
    return n < 256 ? 256 : n;
}

int finc_backward_f32(const float *grad_z, const float *x, const float *w_canon, float *grad_x, float *grad_w_canon,
                      int B, int G, int Cq, int H, int W, int KH, int KW, unsigned orient, void *workspace,
                      size_t workspace_bytes, finc_stream_t stream)
{
    // (its own prelude: every output is optional, what must be there depends on which is asked for, and no pointer has an alignment rule)
    if (!grad_z) return FINC_ERR_NULL_POINTER;
    if (grad_x && !w_canon) return FINC_ERR_NULL_POINTER;
    if (grad_w_canon && !x) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    if (grad_x == grad_z) return FINC_ERR_BAD_DIMS;
    if (int e = finc_fault_gate(false)) return e;
    FincShape s{B, G, Cq, H, W, KH, KW, orient};
    hipStream_t st = (hipStream_t)stream;
    const BackwardWorkspace ws = backward_workspace(s);
    // grad_x: the same conv on the H- and W-flipped image with in/out channels transposed (finc_conv.hip)
    if (grad_x && workspace && finc_conv_supported(Cq, H, W, KH, KW) && ws.bank > 0 && workspace_bytes >= ws.bank) {
        if (int e = finc_conv_pack(w_canon, workspace, G, Cq, KH, KW, true, st)) return e;
        FincShape sb = s;
        sb.orient = orient ^ ((G >= 16) ? 0xFFFFFFFFu : ((1u << (2 * G)) - 1u));
        if (int e = finc_conv_launch(grad_z, workspace, grad_x, sb, st)) return e;
        grad_x = nullptr;
    }
    // grad_w: an MFMA kernel with the pixels on K + reduce (+ corner-tap mask), where the plan for these activations has one
    if (grad_w_canon && workspace && workspace_bytes >= ws.bank + ws.partials) {
        const FincGradwPlan p = finc_gradw_plan(s, finc_align(grad_z, x));
        if (p.form) {
            if (int e = finc_gradw_launch(grad_z, x, grad_w_canon, (char *)workspace + ws.bank, s, p, st)) return e;
            grad_w_canon = nullptr;
        }
    }
    if (!grad_x && !grad_w_canon) return FINC_OK;
    return finc_launch_backward_generic(grad_z, x, w_canon, grad_x, grad_w_canon, s, st);
}

// the fp64 backward's workspace: the transposed bank of the grad-input (finc_f64_packed_bytes), then the grad-weight partials from the
// next 256-byte boundary.  The bound is a function of the bank, B and H alone, so it never shrinks when B, H or W grows.
size_t finc_backward_f64_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    if (B <= 0 || G <= 0 || Cq <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0) return 256;
    const size_t n = align256(finc_f64_packed_bytes(G, Cq, KH, KW)) + finc_f64_gradw_workspace_bound(B, G, Cq, H, KH, KW);
    return n < 256 ? 256 : n;
}

int finc_backward_f64(const double *grad_z, const double *x, const double *w_canon, double *grad_x, double *grad_w_canon, int B, int G,
                      int Cq, int H, int W, int KH, int KW, unsigned orient, void *workspace, size_t workspace_bytes, finc_stream_t stream)
{
    if (!grad_z || (!grad_x && !grad_w_canon)) return FINC_ERR_NULL_POINTER;
    if (grad_x && !w_canon) return FINC_ERR_NULL_POINTER;
    if (grad_w_canon && !x) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    if (off_boundary(7u, grad_z, x, w_canon, grad_x, grad_w_canon)) return FINC_ERR_ALIGNMENT;
    if (grad_x == grad_z) return FINC_ERR_BAD_DIMS;
    if (int e = finc_fault_gate(false)) return e;
    FincShape s{B, G, Cq, H, W, KH, KW, orient};
    hipStream_t st = (hipStream_t)stream;
    // (a workspace off an 8-byte boundary counts as none, as in the finc_*_f64_algo calls)
    const bool mfma = workspace && ((uintptr_t)workspace & 7u) == 0 && finc_f64_supported(s);
    const size_t bank = align256(finc_f64_packed_bytes(G, Cq, KH, KW));
    // grad_x: the forward kernel on the transposed bank, every group's orientation complemented
    if (grad_x && mfma && workspace_bytes >= bank) {
        FincShape sb = s;
        sb.orient = orient ^ ((G >= 16) ? 0xFFFFFFFFu : ((1u << (2 * G)) - 1u));
        if (int e = finc_f64_launch(grad_z, w_canon, grad_x, workspace, sb, FINC_F64_GRAD_INPUT, st)) return e;
        grad_x = nullptr;
    }
    // grad_w: the pixels on the MFMA K dimension, partial tiles behind the bank, a fixed-order reduce with the corner-tap mask
    if (grad_w_canon && mfma) {
        const FincF64GradwPlan p = finc_f64_gradw_plan(s);
        if (p.nrc && workspace_bytes >= bank + p.bytes) {
            if (int e = finc_f64_gradw_launch(grad_z, x, grad_w_canon, (char *)workspace + bank, s, st)) return e;
            grad_w_canon = nullptr;
        }
    }
    if (!grad_x && !grad_w_canon) return FINC_OK;
    return finc_launch_backward_generic_f64(grad_z, x, w_canon, grad_x, grad_w_canon, s, st);
}

// ---- backward through the inverse (finc_adjoint.h) ----
int finc_adjoint_weights_f32(const float *w_canon, float *w_adj, float *lead_t, int G, int Cq, int KH, int KW, finc_stream_t stream)
{
    if (!w_canon || !w_adj || !lead_t) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(1, G, Cq, 1, 1, KH, KW)) return e;
    if (misaligned(w_canon, w_adj, lead_t)) return FINC_ERR_ALIGNMENT;
    if (w_adj == w_canon || lead_t == w_canon || (const float *)lead_t == w_adj) return FINC_ERR_BAD_DIMS;
    if (int e = finc_fault_gate(false)) return e;
    return finc_adjoint_weights_launch(w_canon, w_adj, lead_t, G, Cq, KH, KW, (hipStream_t)stream);
}

int finc_lead_product_f32(float *v, const float *lead_t, int B, int G, int Cq, int HW, finc_stream_t stream)
{
    if (!v || !lead_t) return FINC_ERR_NULL_POINTER;
    if (G <= 0 || Cq <= 0 || G > FINC_MAX_GROUPS || Cq > FINC_MAX_CQ) return FINC_ERR_BAD_DIMS;
    if (int e = pixel_dims(B, G * Cq, HW, true)) return e;
    if ((size_t)G * Cq * HW >= ((size_t)1 << 29)) return FINC_ERR_BAD_DIMS;      // an image's bytes index as int (finc_mix_launch)
    if (misaligned(v, lead_t)) return FINC_ERR_ALIGNMENT;
    if ((const float *)v == lead_t) return FINC_ERR_BAD_DIMS;
    if (int e = finc_fault_gate(false)) return e;
    return finc_lead_launch(v, lead_t, B, G, Cq, HW, (hipStream_t)stream);
}

int finc_negate_f32(float *p, size_t n, finc_stream_t stream)
{
    if (!p) return FINC_ERR_NULL_POINTER;
    if (n == 0 || n >= ((size_t)1 << 31)) return FINC_ERR_BAD_DIMS;
    if (misaligned(p)) return FINC_ERR_ALIGNMENT;
    if (int e = finc_fault_gate(false)) return e;
    return finc_negate_launch(p, n, (hipStream_t)stream);
}

// ---- the PLU-parametrised 1x1 convolution's parameter work (finc_plu.h) ----
int finc_plu_supported_f32(int C) { return finc_plu_supported(C) ? 1 : 0; }

// does an output share a byte with one of the five inputs, with `extra` (the incoming gradients) or with an earlier output?
// sizes in floats: [C][C] matrices, [C] vectors, one-float scalars
struct PluSpan { const void *p; size_t n; };
static bool plu_overlap(const PluSpan *in, int n_in, const PluSpan *out, int n_out)
{
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (bytes_overlap(out[o].p, out[o].n * 4, in[i].p, in[i].n * 4)) return true;
        for (int q = 0; q < o; ++q)
            if (bytes_overlap(out[o].p, out[o].n * 4, out[q].p, out[q].n * 4)) return true;
    }
    return false;
}

int finc_plu_compose_f32(const float *lower, const float *upper, const float *log_s, const float *sign_s, const int *perm, float *w,
                         float *w_inv, float *logdet, int C, finc_stream_t stream)
{
    if (!lower || !upper || !log_s || !sign_s || !perm || (!w && !w_inv && !logdet)) return FINC_ERR_NULL_POINTER;
    if (C < 1) return FINC_ERR_BAD_DIMS;
    const size_t cc = (size_t)C * C, c = (size_t)C;
    const PluSpan in[] = {{lower, cc}, {upper, cc}, {log_s, c}, {sign_s, c}, {perm, c}}, out[] = {{w, cc}, {w_inv, cc}, {logdet, 1}};
    if (plu_overlap(in, 5, out, 3)) return FINC_ERR_BAD_DIMS;
    if (misaligned(lower, upper, log_s, sign_s, w, w_inv, logdet) || misaligned(perm)) return FINC_ERR_ALIGNMENT;
    if (!finc_plu_supported(C)) return FINC_ERR_UNSUPPORTED;
    if (int e = finc_fault_gate(false)) return e;
    return finc_plu_compose_launch(lower, upper, log_s, sign_s, perm, w, w_inv, logdet, C, (hipStream_t)stream);
}

int finc_plu_compose_backward_f32(const float *grad_w, const float *grad_logdet, const float *lower, const float *upper,
                                  const float *log_s, const float *sign_s, const int *perm, float *grad_lower, float *grad_upper,
                                  float *grad_log_s, int C, finc_stream_t stream)
{
    if (!grad_w || !lower || !upper || !log_s || !sign_s || !perm || (!grad_lower && !grad_upper && !grad_log_s)) return FINC_ERR_NULL_POINTER;
    if (C < 1) return FINC_ERR_BAD_DIMS;
    const size_t cc = (size_t)C * C, c = (size_t)C;
    const PluSpan in[] = {{grad_w, cc}, {grad_logdet, 1}, {lower, cc}, {upper, cc}, {log_s, c}, {sign_s, c}, {perm, c}},
                  out[] = {{grad_lower, cc}, {grad_upper, cc}, {grad_log_s, c}};
    if (plu_overlap(in, 7, out, 3)) return FINC_ERR_BAD_DIMS;
    if (misaligned(grad_w, grad_logdet, lower, upper, log_s, sign_s, grad_lower, grad_upper, grad_log_s) || misaligned(perm))
        return FINC_ERR_ALIGNMENT;
    if (!finc_plu_supported(C)) return FINC_ERR_UNSUPPORTED;
    if (int e = finc_fault_gate(false)) return e;
    return finc_plu_compose_bwd_launch(grad_w, grad_logdet, lower, upper, log_s, sign_s, perm, grad_lower, grad_upper, grad_log_s, C,
                                       (hipStream_t)stream);
}

// the one-call form's workspace: the adjoint bank, lead_t, one activation-sized buffer (y, when the caller skips grad_z), then what the
// solve (finc_inverse_f32, AUTO) and the grad-weight (finc_backward_f32) take, one after the other on the same bytes.  The activation
// parts are sized for rows padded to 8 floats whatever the width, so that the bound never shrinks when B, H or W grows.
struct InverseBackwardWorkspace { size_t w_adj, lead_t, y, calls, total; };
static InverseBackwardWorkspace inverse_backward_workspace(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    InverseBackwardWorkspace ws;
    const size_t act = align256((size_t)B * G * Cq * H * ((W + 7) / 8 * 8) * sizeof(float));
    ws.w_adj = 0;
    ws.lead_t = align256((size_t)G * Cq * Cq * KH * KW * sizeof(float));
    ws.y = ws.lead_t + align256((size_t)G * Cq * G * Cq * sizeof(float));
    ws.calls = ws.y + act;
    const size_t inv = align256(finc_workspace_bytes(G, Cq, KH, KW)) + 2 * act;
    // (the grad-weight plan's own bytes change form with the width: its bound over all maps of no more strips does not)
    const size_t bwd = align256(finc_conv_packed_bytes(G, Cq, KH, KW)) + finc_gradw_workspace_bound(G, Cq, KH, KW, (long long)B * ((W + 15) / 16));
    ws.total = ws.calls + align256(inv > bwd ? inv : bwd);
    return ws;
}

size_t finc_inverse_backward_workspace_bytes(int B, int G, int Cq, int H, int W, int KH, int KW)
{
    if (B <= 0 || G <= 0 || Cq <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0) return 256;
    return inverse_backward_workspace(B, G, Cq, H, W, KH, KW).total;
}

int finc_inverse_backward_f32(const float *grad_x, const float *x, const float *w_canon, float *grad_z, float *grad_w_canon, int B, int G,
                              int Cq, int H, int W, int KH, int KW, unsigned orient, void *workspace, size_t workspace_bytes,
                              finc_stream_t stream)
{
    if (!grad_x || !w_canon || (!grad_z && !grad_w_canon) || (grad_w_canon && !x)) return FINC_ERR_NULL_POINTER;
    if (int e = check_shape(B, G, Cq, H, W, KH, KW)) return e;
    if ((size_t)G * Cq * H * W >= ((size_t)1 << 29)) return FINC_ERR_BAD_DIMS;   // an image's bytes index as int in the lead product
    if (misaligned(grad_x, x, w_canon, grad_z, grad_w_canon)) return FINC_ERR_ALIGNMENT;
    if (grad_z && (grad_z == grad_x || grad_z == x)) return FINC_ERR_BAD_DIMS;
    const InverseBackwardWorkspace ws = inverse_backward_workspace(B, G, Cq, H, W, KH, KW);
    // (the parts start on 256-byte boundaries of a 16-byte aligned buffer: the packed launch and the 16-byte forms stay available)
    if (!workspace || off_boundary(15u, workspace) || workspace_bytes < ws.total) return FINC_ERR_WORKSPACE;
    float *y = grad_z ? grad_z : (float *)((char *)workspace + ws.y);
    // the forward's weight gradient has no kernel for this filter (finc_backward_f32 says the same): refuse before anything is launched
    if (grad_w_canon && !finc_backward_generic_has_gradw(KH, KW) && !finc_gradw_plan(FincShape{B, G, Cq, H, W, KH, KW, orient}, finc_align(y, x)).form)
        return FINC_ERR_UNSUPPORTED;
    if (int e = finc_fault_gate(false)) return e;
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)workspace;
    float *w_adj = (float *)(base + ws.w_adj), *lead_t = (float *)(base + ws.lead_t);
    void *calls = base + ws.calls;
    const size_t calls_bytes = ws.total - ws.calls;
    if (int e = finc_adjoint_weights_launch(w_canon, w_adj, lead_t, G, Cq, KH, KW, st)) return e;
    // M^T reads the opposite corner: every group's orientation bits complemented
    const unsigned adj_orient = orient ^ ((G >= 16) ? 0xFFFFFFFFu : ((1u << (2 * G)) - 1u));
    if (int e = run(grad_x, w_adj, y, B, G, Cq, H, W, KH, KW, adj_orient, FINC_ALGO_AUTO, calls, calls_bytes, stream, false)) return e;
    if (int e = finc_lead_launch(y, lead_t, B, G, Cq, H * W, st)) return e;
    if (!grad_w_canon) return FINC_OK;
    if (int e = finc_backward_f32(y, x, w_canon, nullptr, grad_w_canon, B, G, Cq, H, W, KH, KW, orient, calls, calls_bytes, stream)) return e;
    return finc_negate_launch(grad_w_canon, (size_t)G * Cq * Cq * KH * KW, st);
}

} // extern "C"
