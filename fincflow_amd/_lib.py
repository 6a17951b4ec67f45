"""ctypes binding of the C ABI declared in include/finc.h (libfinc_hip.so).

Fails loudly: a missing library is an ImportError-like RuntimeError at first use,
never a silent fallback.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
#: FINCFLOW_LIB selects another build of the library (scripts/: A/B timing of experiment builds).  It is never silent: the
#: override is announced on stderr with the library's build flags, `library_info()` reports it, and bench.py refuses to print a
#: judged line from an overridden library unless its build flags are 0 and the line says which file ran.
LIB_OVERRIDE = os.environ.get("FINCFLOW_LIB") or None
LIB_PATH = LIB_OVERRIDE or os.path.join(HERE, "libfinc_hip.so")

OK = 0
ALGO = {"auto": 0, "strict": 1, "mfma": 2}

# every symbol include/finc.h declares (tests/test_abi.py checks the list against the header)
SYMBOLS = [
    "finc_version", "finc_status_string", "finc_last_hip_error", "finc_canonicalize_weights_f32",
    "finc_check_invariant_f32", "finc_workspace_bytes", "finc_inverse_algo_for", "finc_forward_algo_for",
    "finc_inverse_f32", "finc_forward_f32", "finc_pack_inverse_weights_f32", "finc_pack_forward_weights_f32",
    "finc_inverse_packed_f32", "finc_forward_packed_f32", "finc_backward_f32", "finc_backward_workspace_bytes",
    "finc_inverse_workspace_bytes", "finc_pack_inverse_weights_affine_f32",
    "finc_canonicalize_weights_f64", "finc_inverse_f64", "finc_forward_f64",
    "finc_f64_workspace_bytes", "finc_inverse_f64_algo", "finc_forward_f64_algo",
    "finc_inverse_kernel_variant", "finc_debug_attr_table_insert", "finc_debug_inverse_table_row",
    "finc_mix_supported_f32", "finc_mix_f32", "finc_pack_forward_weights_affine_f32", "finc_debug_hlp_timeouts",
    "finc_build_flags", "finc_inverse_packed_premultiplied_f32", "finc_inverse_premultiplied_supported", "finc_clear_fault", "finc_debug_backward_variant", "finc_debug_set_forward_form",
    "finc_debug_row_chunks", "finc_debug_inverse_remainder_images", "finc_debug_gradw_plan", "finc_debug_conv_plan",
    "finc_inverse_affine_supported", "finc_fault_pending", "finc_runtime_switches",
    "finc_debug_clock_probe_begin", "finc_debug_clock_probe_end",
    "finc_mix_backward_workspace_bytes", "finc_mix_backward_f32",
    "finc_coupling_supported_f32", "finc_coupling_workspace_bytes", "finc_coupling_f32", "finc_coupling_backward_f32",
    "finc_bias_relu_f32",
    "finc_actnorm_workspace_bytes", "finc_actnorm_f32", "finc_actnorm_backward_f32", "finc_actnorm_init_f32",
    "finc_adjoint_weights_f32", "finc_lead_product_f32", "finc_negate_f32", "finc_inverse_backward_workspace_bytes",
    "finc_inverse_backward_f32",
    "finc_coupling_reverse_backward_f32", "finc_actnorm_reverse_backward_f32",
    "finc_coupling_reverse_logdet_f32", "finc_coupling_reverse_logdet_backward_f32",
    "finc_actnorm_backward_reconstruct_f32", "finc_coupling_backward_reconstruct_f32",
    "finc_backward_f64_workspace_bytes", "finc_backward_f64", "finc_check_invariant_f64",
    "finc_debug_f64_plan",
    "finc_coupling_rawbf16_f32", "finc_coupling_backward_rawbf16_f32", "finc_coupling_reverse_backward_rawbf16_f32",
    "finc_coupling_reverse_logdet_rawbf16_f32", "finc_coupling_reverse_logdet_backward_rawbf16_f32",
    "finc_coupling_backward_reconstruct_rawbf16_f32", "finc_bias_relu_bf16",
    "finc_split_prior_f32", "finc_split_prior_merge_f32", "finc_split_prior_backward_f32",
    "finc_split_prior_rawbf16_f32", "finc_split_prior_merge_rawbf16_f32", "finc_split_prior_backward_rawbf16_f32",
    "finc_image_workspace_bytes", "finc_image_encode_u8_f32", "finc_image_encode_f32", "finc_image_decode_f32", "finc_image_decode_u8",
    "finc_gauss_split_f32", "finc_gauss_split_merge_f32", "finc_gauss_split_backward_f32",
    "finc_split_prior_merge_backward_f32", "finc_split_prior_merge_backward_rawbf16_f32", "finc_gauss_split_merge_backward_f32",
    "finc_plu_supported_f32", "finc_plu_compose_f32", "finc_plu_compose_backward_f32",
    "finc_debug_pixel_plan",
    "finc_spline_supported_f32", "finc_spline_workspace_bytes", "finc_spline_f32", "finc_spline_backward_f32",
    "finc_spline_reverse_backward_f32",
    "finc_activation_supported_f32", "finc_debug_activation_trips", "finc_activation_workspace_bytes", "finc_activation_f32",
    "finc_activation_backward_f32",
]

#: the ABI version this binding is written against (include/finc.h: finc_version)
ABI_VERSION = 104
#: the version that added the ActNorm entry points (finc_actnorm_f32, finc_actnorm_backward_f32, finc_actnorm_init_f32); a second,
#: named floor behind the first so that each refusal says what the library lacks
ACTNORM_ABI_VERSION = 105
#: the version that added the backward through the inverse (finc_adjoint_weights_f32, finc_lead_product_f32, finc_negate_f32,
#: finc_inverse_backward_f32)
INVERSE_BACKWARD_ABI_VERSION = 107
#: the version that added the backwards of the per-pixel layers' reverse direction (finc_coupling_reverse_backward_f32,
#: finc_actnorm_reverse_backward_f32)
REVERSE_BACKWARD_ABI_VERSION = 108
#: the version that added the coupling's reverse with its log-det and the backward of that (finc_coupling_reverse_logdet_f32,
#: finc_coupling_reverse_logdet_backward_f32): what sample_with_log_prob / rsample_with_log_prob launch
SAMPLE_LOGDET_ABI_VERSION = 109
#: the version that added the forward-direction backwards that rebuild the layer's input from its output
#: (finc_actnorm_backward_reconstruct_f32, finc_coupling_backward_reconstruct_f32): what FlowSequential.invertible_backward launches
INVERTIBLE_BACKWARD_ABI_VERSION = 110
#: the version that added the double-precision backward of the forward conv and the invariant check on doubles (finc_backward_f64,
#: finc_check_invariant_f64): what a float64 unit on the device trains and validates with
F64_BACKWARD_ABI_VERSION = 111
#: the version that added the float64 matrix-core kernels of the wider banks (29 .. 64 channels at 3x3, 33 .. 64 at 2x2: the M-split
#: family of finc_f64.hip) and the plan query that says which family a shape takes (finc_debug_f64_plan)
F64_WIDE_BANKS_ABI_VERSION = 112
#: the version that added the coupling's entry points on a bfloat16 `raw` / `grad_raw` (the six finc_coupling_*_rawbf16_f32) and
#: finc_bias_relu_bf16: what a Coupling launches under torch.autocast(device_type="cuda", dtype=torch.bfloat16)
AUTOCAST_ABI_VERSION = 113
#: the version that added the split prior with its latent (finc_split_prior_f32, finc_split_prior_merge_f32,
#: finc_split_prior_backward_f32 and their _rawbf16_f32 siblings): what SplitPrior.split / merge and FlowSequential.encode / decode launch
SPLIT_LATENT_ABI_VERSION = 114
#: the version that added the image boundary (finc_image_encode_u8_f32, finc_image_encode_f32, finc_image_decode_f32,
#: finc_image_decode_u8): what FlowSequential.fuse_image_boundary and sample_uint8 launch
IMAGE_BOUNDARY_ABI_VERSION = 115
#: the version that added the Gaussianized split (finc_gauss_split_f32, finc_gauss_split_merge_f32, finc_gauss_split_backward_f32):
#: what glow.Split.split / merge launch
GAUSS_SPLIT_ABI_VERSION = 116
#: the version that added the backward of the two merges (finc_split_prior_merge_backward_f32, its _rawbf16_f32 sibling,
#: finc_gauss_split_merge_backward_f32): what a recorded SplitPrior.merge / Split.merge with `hip_recorded_merge` launches
MERGE_BACKWARD_ABI_VERSION = 117
#: the version that added the PLU-parametrised 1x1 convolution's parameter work (finc_plu_supported_f32, finc_plu_compose_f32,
#: finc_plu_compose_backward_f32): what glow.Conv1x1LU launches
PLU_ABI_VERSION = 118
#: the version that added the host-only plan query of the per-pixel layers' three launch rules (finc_debug_pixel_plan): what
#: `pixel_plan` and the launch-regime tests of the coupling, ActNorm, bias + ReLU, the lead product and the mix read
PIXEL_PLAN_ABI_VERSION = 119
#: the version that added the rational-quadratic spline (finc_spline_f32, finc_spline_backward_f32,
#: finc_spline_reverse_backward_f32) and its family of the plan query: what glow.SplineActivation launches
SPLINE_ABI_VERSION = 120
#: the version that added the smooth invertible activations (finc_activation_f32, finc_activation_backward_f32) and their family of
#: the plan query: what glow.SmoothLeakyRelu, LeakyRelu, LearnableLeakyRelu and SmoothTanh launch
ACTIVATION_ABI_VERSION = 121

_lib = None


class FincError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FincError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C fincflow_amd/csrc`).  fincflow_amd has no CPU / PyTorch fallback.")
    L = ctypes.CDLL(LIB_PATH)
    vp, i, u, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
    # the version first: an older build (FINCFLOW_LIB) lacks symbols bound below, and an AttributeError from ctypes would not say why
    try:
        L.finc_version.restype = i
        have = int(L.finc_version())
    except AttributeError:
        raise FincError(f"{LIB_PATH} does not export finc_version: not a build of libfinc_hip.so") from None
    if have < ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, this package needs at least {ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < ACTNORM_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the ActNorm entry points (finc_actnorm_f32, "
                        f"finc_actnorm_backward_f32, finc_actnorm_init_f32) came with {ACTNORM_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < INVERSE_BACKWARD_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the backward through the inverse (finc_adjoint_weights_f32, "
                        f"finc_inverse_backward_f32) came with {INVERSE_BACKWARD_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < REVERSE_BACKWARD_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the backwards of the reverse direction "
                        f"(finc_coupling_reverse_backward_f32, finc_actnorm_reverse_backward_f32) came with "
                        f"{REVERSE_BACKWARD_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < SAMPLE_LOGDET_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the coupling's reverse with its log-det "
                        f"(finc_coupling_reverse_logdet_f32, finc_coupling_reverse_logdet_backward_f32) came with "
                        f"{SAMPLE_LOGDET_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < INVERTIBLE_BACKWARD_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the backwards that rebuild a layer's input from its output "
                        f"(finc_actnorm_backward_reconstruct_f32, finc_coupling_backward_reconstruct_f32) came with "
                        f"{INVERTIBLE_BACKWARD_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < F64_BACKWARD_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the double-precision backward (finc_backward_f64, "
                        f"finc_check_invariant_f64) came with {F64_BACKWARD_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < F64_WIDE_BANKS_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the float64 matrix-core kernels of the 29 .. 64 channel banks "
                        f"and their plan query (finc_debug_f64_plan) came with {F64_WIDE_BANKS_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < AUTOCAST_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the coupling's bfloat16 entry points (finc_coupling_rawbf16_f32 "
                        f"and its five siblings, finc_bias_relu_bf16) came with {AUTOCAST_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < SPLIT_LATENT_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the split prior's entry points (finc_split_prior_f32, "
                        f"finc_split_prior_merge_f32, finc_split_prior_backward_f32 and their bfloat16 siblings) came with "
                        f"{SPLIT_LATENT_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < IMAGE_BOUNDARY_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the image boundary's entry points (finc_image_encode_u8_f32, "
                        f"finc_image_encode_f32, finc_image_decode_f32, finc_image_decode_u8) came with "
                        f"{IMAGE_BOUNDARY_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < GAUSS_SPLIT_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the Gaussianized split's entry points (finc_gauss_split_f32, "
                        f"finc_gauss_split_merge_f32, finc_gauss_split_backward_f32) came with "
                        f"{GAUSS_SPLIT_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < MERGE_BACKWARD_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the backward of the merges "
                        f"(finc_split_prior_merge_backward_f32, its bfloat16 sibling, finc_gauss_split_merge_backward_f32) came with "
                        f"{MERGE_BACKWARD_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < PLU_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the PLU-parametrised 1x1 convolution's entry points "
                        f"(finc_plu_compose_f32, finc_plu_compose_backward_f32) came with {PLU_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < PIXEL_PLAN_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the per-pixel layers' launch-plan query "
                        f"(finc_debug_pixel_plan) came with {PIXEL_PLAN_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < SPLINE_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the rational-quadratic spline's entry points "
                        f"(finc_spline_f32, finc_spline_backward_f32, finc_spline_reverse_backward_f32) came with "
                        f"{SPLINE_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    if have < ACTIVATION_ABI_VERSION:
        raise FincError(f"{LIB_PATH} reports finc_version() = {have}, the smooth invertible activations' entry points "
                        f"(finc_activation_f32, finc_activation_backward_f32) came with {ACTIVATION_ABI_VERSION}: rebuild it "
                        "(`make -C fincflow_amd/csrc`)" + (" or unset FINCFLOW_LIB" if LIB_OVERRIDE else ""))
    L.finc_build_flags.restype = u
    L.finc_clear_fault.restype = i
    L.finc_status_string.restype = ctypes.c_char_p
    L.finc_status_string.argtypes = [i]
    L.finc_last_hip_error.restype = ctypes.c_char_p
    L.finc_canonicalize_weights_f32.argtypes = [vp, vp, i, i, i, i, u, vp]
    L.finc_check_invariant_f32.argtypes = [vp, i, i, i, i, vp]
    L.finc_workspace_bytes.restype = sz
    L.finc_workspace_bytes.argtypes = [i, i, i, i]
    L.finc_inverse_algo_for.argtypes = [i, i, i, i, i]
    L.finc_forward_algo_for.argtypes = [i, i, i, i, i]
    run = [vp, vp, vp, i, i, i, i, i, i, i, u, i, vp, sz, vp]
    L.finc_inverse_f32.argtypes = run
    L.finc_forward_f32.argtypes = run
    L.finc_pack_inverse_weights_f32.argtypes = [vp, vp, i, i, i, i, vp]
    L.finc_pack_inverse_weights_affine_f32.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
    L.finc_pack_forward_weights_f32.argtypes = [vp, vp, i, i, i, i, vp]
    L.finc_pack_forward_weights_affine_f32.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
    runp = [vp, vp, vp, i, i, i, i, i, i, i, u, vp]
    L.finc_inverse_packed_f32.argtypes = runp
    L.finc_inverse_packed_premultiplied_f32.argtypes = runp
    L.finc_inverse_premultiplied_supported.argtypes = [i, i, i, i, i, i, i]
    L.finc_inverse_affine_supported.argtypes = [i, i, i, i, i, i, i]
    L.finc_fault_pending.restype = i
    L.finc_runtime_switches.argtypes = [ctypes.c_char_p, sz]
    L.finc_debug_clock_probe_begin.argtypes = [i, i]
    L.finc_debug_clock_probe_end.argtypes = [ctypes.POINTER(ctypes.c_double)]
    L.finc_forward_packed_f32.argtypes = runp
    L.finc_backward_workspace_bytes.restype = sz
    L.finc_inverse_workspace_bytes.restype = sz
    L.finc_inverse_workspace_bytes.argtypes = [i, i, i, i, i, i, i]
    L.finc_backward_workspace_bytes.argtypes = [i, i, i, i, i, i, i]
    L.finc_backward_f32.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, u, vp, sz, vp]
    L.finc_canonicalize_weights_f64.argtypes = [vp, vp, i, i, i, i, u, vp]
    run64 = [vp, vp, vp, i, i, i, i, i, i, i, u, vp]
    L.finc_inverse_f64.argtypes = run64
    L.finc_forward_f64.argtypes = run64
    L.finc_f64_workspace_bytes.restype = sz
    L.finc_f64_workspace_bytes.argtypes = [i, i, i, i]
    L.finc_inverse_f64_algo.argtypes = run
    L.finc_forward_f64_algo.argtypes = run
    L.finc_backward_f64_workspace_bytes.restype = sz
    L.finc_backward_f64_workspace_bytes.argtypes = [i, i, i, i, i, i, i]
    L.finc_backward_f64.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, u, vp, sz, vp]
    L.finc_check_invariant_f64.argtypes = [vp, i, i, i, i, vp]
    L.finc_inverse_kernel_variant.argtypes = [i, i, i, i, i, i, i, ctypes.POINTER(ctypes.c_int)]
    L.finc_debug_attr_table_insert.argtypes = [i, sz]
    L.finc_debug_inverse_table_row.argtypes = [i, ctypes.POINTER(ctypes.c_int)]
    L.finc_debug_hlp_timeouts.argtypes = [ctypes.POINTER(ctypes.c_uint)]
    L.finc_debug_backward_variant.argtypes = [i, i, i, i, i, i, i, ctypes.POINTER(ctypes.c_int)]
    L.finc_debug_inverse_remainder_images.argtypes = [i, i, i, i, i, i, i]
    L.finc_debug_row_chunks.argtypes = [ctypes.c_longlong, ctypes.c_longlong, i, i, i, i]
    L.finc_debug_set_forward_form.argtypes = [i]
    L.finc_debug_gradw_plan.argtypes = [i, i, i, i, i, i, i, i, ctypes.POINTER(ctypes.c_longlong)]
    L.finc_debug_conv_plan.argtypes = [i, i, i, i, i, i, i, i, ctypes.POINTER(ctypes.c_int)]
    L.finc_debug_f64_plan.argtypes = [i, i, i, i, i, i, i, ctypes.POINTER(ctypes.c_int)]
    L.finc_debug_pixel_plan.argtypes = [i, i, i, i, i, i, i, i, ctypes.POINTER(ctypes.c_longlong)]
    L.finc_mix_supported_f32.argtypes = [i]
    L.finc_mix_f32.argtypes = [vp, vp, vp, vp, i, i, i, vp]
    L.finc_mix_backward_workspace_bytes.restype = sz
    L.finc_mix_backward_workspace_bytes.argtypes = [i, i, i]
    L.finc_mix_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_coupling_supported_f32.argtypes = [i]
    L.finc_coupling_workspace_bytes.restype = sz
    L.finc_coupling_workspace_bytes.argtypes = [i, i, i]
    L.finc_coupling_f32.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, vp, sz, vp]
    L.finc_coupling_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_bias_relu_f32.argtypes = [vp, vp, vp, i, i, i, vp]
    L.finc_actnorm_workspace_bytes.restype = sz
    L.finc_actnorm_workspace_bytes.argtypes = [i, i, i]
    L.finc_actnorm_f32.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp]
    L.finc_actnorm_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_actnorm_init_f32.argtypes = [vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_adjoint_weights_f32.argtypes = [vp, vp, vp, i, i, i, i, vp]
    L.finc_lead_product_f32.argtypes = [vp, vp, i, i, i, i, vp]
    L.finc_negate_f32.argtypes = [vp, sz, vp]
    L.finc_inverse_backward_workspace_bytes.restype = sz
    L.finc_inverse_backward_workspace_bytes.argtypes = [i, i, i, i, i, i, i]
    L.finc_inverse_backward_f32.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, u, vp, sz, vp]
    L.finc_coupling_reverse_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_actnorm_reverse_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_coupling_reverse_logdet_f32.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_coupling_reverse_logdet_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_actnorm_backward_reconstruct_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_coupling_backward_reconstruct_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    for name in ("finc_coupling", "finc_coupling_backward", "finc_coupling_reverse_backward", "finc_coupling_reverse_logdet",
                 "finc_coupling_reverse_logdet_backward", "finc_coupling_backward_reconstruct"):
        getattr(L, name + "_rawbf16_f32").argtypes = getattr(L, name + "_f32").argtypes       # (pointers are void * here)
    L.finc_bias_relu_bf16.argtypes = L.finc_bias_relu_f32.argtypes
    L.finc_split_prior_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_split_prior_merge_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_split_prior_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    for name in ("finc_split_prior", "finc_split_prior_merge", "finc_split_prior_backward"):
        getattr(L, name + "_rawbf16_f32").argtypes = getattr(L, name + "_f32").argtypes
    fl = ctypes.c_float
    L.finc_image_workspace_bytes.restype = sz
    L.finc_image_workspace_bytes.argtypes = [i, i, i, i, i]
    L.finc_image_encode_u8_f32.argtypes = [vp, vp, vp, vp, i, i, i, i, i, fl, fl, fl, fl, fl, vp, sz, vp]
    L.finc_image_encode_f32.argtypes = L.finc_image_encode_u8_f32.argtypes
    L.finc_image_decode_f32.argtypes = [vp, vp, vp, i, i, i, i, i, fl, fl, fl, fl, vp, sz, vp]
    L.finc_image_decode_u8.argtypes = L.finc_image_decode_f32.argtypes
    for name in ("finc_split_prior", "finc_split_prior_merge", "finc_split_prior_backward"):    # (the same argument lists)
        getattr(L, name.replace("split_prior", "gauss_split") + "_f32").argtypes = getattr(L, name + "_f32").argtypes
    L.finc_split_prior_merge_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_split_prior_merge_backward_rawbf16_f32.argtypes = L.finc_split_prior_merge_backward_f32.argtypes
    L.finc_gauss_split_merge_backward_f32.argtypes = L.finc_split_prior_merge_backward_f32.argtypes
    L.finc_plu_supported_f32.argtypes = [i]
    L.finc_plu_compose_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, vp]
    L.finc_plu_compose_backward_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp]
    L.finc_spline_supported_f32.argtypes = [i]
    L.finc_spline_workspace_bytes.restype = sz
    L.finc_spline_workspace_bytes.argtypes = [i, i, i, i, i]
    L.finc_spline_f32.argtypes = [vp, vp, i, i, fl, i, vp, vp, i, i, i, vp, sz, vp]
    L.finc_spline_backward_f32.argtypes = [vp, vp, vp, vp, i, i, fl, vp, vp, i, i, i, vp, sz, vp]
    L.finc_spline_reverse_backward_f32.argtypes = L.finc_spline_backward_f32.argtypes
    L.finc_activation_supported_f32.argtypes = [i]
    L.finc_debug_activation_trips.argtypes = [i]
    L.finc_activation_workspace_bytes.restype = sz
    L.finc_activation_workspace_bytes.argtypes = [i, i, i]
    L.finc_activation_f32.argtypes = [i, fl, fl, vp, i, vp, vp, vp, i, i, i, vp, sz, vp]
    L.finc_activation_backward_f32.argtypes = [i, fl, fl, vp, i, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp]
    for name in SYMBOLS:
        getattr(L, name)  # AttributeError here = header and library out of sync
    _lib = L
    if LIB_OVERRIDE:
        import sys
        print(f"fincflow_amd: FINCFLOW_LIB override -> {LIB_PATH} (finc_build_flags = {int(L.finc_build_flags()):#x})", file=sys.stderr)
    return L


def library_info():
    """Which library file is loaded, whether the environment chose it, and the measurement knobs it was built with."""
    return {"path": os.path.relpath(LIB_PATH, os.path.dirname(HERE)) if not LIB_OVERRIDE else LIB_PATH,
            "env_override": bool(LIB_OVERRIDE), "build_flags": int(lib().finc_build_flags()), "version": int(lib().finc_version())}


def inverse_variant(B, G, Cq, H, W, KH, KW):
    """The MFMA inverse kernel variant the library launches for this problem, or None (strict kernel)."""
    info = (ctypes.c_int * 8)()
    st = lib().finc_inverse_kernel_variant(B, G, Cq, H, W, KH, KW, info)
    if st == 3:
        return None
    check(st, "finc_inverse_kernel_variant")
    keys = ("cqp", "nw", "npw", "sec", "lds_bytes", "workgroups", "row", "rows")
    return dict(zip(keys, list(info)))


def inverse_remainder_images(B, G, Cq, H, W, KH, KW):
    """Images of an inverse call that go to a second launch on the remainder's own kernel (0: one launch)."""
    return int(lib().finc_debug_inverse_remainder_images(B, G, Cq, H, W, KH, KW))


def backward_variant(B, G, Cq, H, W, KH, KW):
    """Kernels finc_backward_f32 runs for this shape, given 16-byte aligned activations: `gradw`, the grad-weight form ("direct" =
    no MFMA kernel, "dword" = MFMA kernel on dword loads, "staged" = its 16-byte pieces through LDS, "tiled" = one (o, i) tile pair
    per workgroup, "winograd" = F(4,3) transposed, "winograd_tiled" = the same (5x5: F(2,5)) on one tile pair per wave), `gradx_waves`,
    the grad-input's waves per strip (0 = direct kernel, > 1 = K-split), and `conv_form`: the kernel the forward and grad-input run
    ("scalar", "strip", "strip16" = its 16-byte-piece form, "winograd" = F(2,3) along W, "msplit" = the big banks' M-split over eight waves,
    "winograd4" = F(4,3) along W, "winograd25" = F(2,5) along W for the 5x5 banks, "winograd4m" = F(4,3) M-split over a workgroup's
    waves for the 3x3 banks of 28 .. 64 channels, "stream" = the streaming-bank kernel of the banks beyond every table, finc_stream.hip)."""
    info = (ctypes.c_int * 3)()
    check(lib().finc_debug_backward_variant(B, G, Cq, H, W, KH, KW, info), "finc_debug_backward_variant")
    form = "scalar" if info[1] == 0 else ("strip", "strip16", "winograd", "msplit", "winograd4", "winograd25", "winograd4m", "stream")[info[2]]
    return {"gradw": ("direct", "dword", "staged", "tiled", "winograd", "winograd_tiled")[info[0]], "gradx_waves": info[1],
            "conv_form": form}


GRADW_FORMS = ("direct", "dword", "staged", "tiled", "winograd", "winograd_tiled")
CONV_FORMS = ("strip", "strip16", "winograd", "msplit", "winograd4", "winograd25", "winograd4m", "stream")


def gradw_plan(B, G, Cq, H, W, KH, KW, align=16):
    """The grad-weight launch plan finc_backward_f32 runs for this shape when grad_z and x are `align` bytes aligned (host-only; the
    launch's own plan object): `form` (backward_variant's names), `strip` columns per strip, `ns` strips per row, `units` = B * ns that
    the `wpg` workgroups of a group walk (units > wpg: a second trip through a workgroup's unit loop), `grid` and `block` (x),
    `mtt` 16-channel tiles per side, `fs` waves per workgroup of the winograd form, `bytes` of partial sums in the workspace."""
    info = (ctypes.c_longlong * 10)()
    check(lib().finc_debug_gradw_plan(B, G, Cq, H, W, KH, KW, int(align), info), "finc_debug_gradw_plan")
    d = dict(zip(("form", "strip", "ns", "units", "wpg", "grid", "block", "mtt", "fs", "bytes"), (int(v) for v in info)))
    d["form"] = GRADW_FORMS[d["form"]]
    return d


def conv_plan(B, G, Cq, H, W, KH, KW, align=16):
    """The forward / grad-input launch plan for this shape and alignment, a form pinned by set_forward_form honoured (host-only):
    `form` (backward_variant's conv_form names), `strip` columns per strip, `ns` strips per row, `waves` per workgroup, `nrc` row
    chunks of `RC` rows (the last one ragged).  None: the direct kernel."""
    info = (ctypes.c_int * 6)()
    st = lib().finc_debug_conv_plan(B, G, Cq, H, W, KH, KW, int(align), info)
    if st == 3:
        return None
    check(st, "finc_debug_conv_plan")
    d = dict(zip(("form", "strip", "ns", "waves", "nrc", "RC"), (int(v) for v in info)))
    d["form"] = CONV_FORMS[d["form"]]
    return d


#: finc_debug_pixel_plan's launch rules and, per rule, the entry-point families (include/finc.h FincPixelRule / FincPixelFamily)
PIXEL_RULES = {"rows": 0, "parts": 1, "mix": 2}
PIXEL_FAMILIES = {"rows": {"channel_rows": 0, "lead": 1, "negate": 2},
                  "parts": {"transform": 0, "coupling_grad": 1, "actnorm_grad": 2, "spline": 4, "activation": 5},
                  "mix": {"mix": 0}}


def pixel_plan(rule, family, B, C, HW, align=16, elem_bytes=4, groups=0):
    """What a per-pixel call on [B][C][HW] launches when its activation pointers are `align` bytes aligned (host-only; answered by
    the functions the launchers call).  `rule`: "rows" (grid-stride; families "channel_rows": ActNorm's transform and bias + ReLU --
    `elem_bytes` 2 is finc_bias_relu_bf16 --, "lead": the grouped lead product with `groups` = G, "negate": finc_negate_f32 on
    B * C * HW elements), "parts" ((outer, part) workgroups; "transform": outer = B, "coupling_grad": outer = C / 2, "actnorm_grad":
    outer = C; `elem_bytes` 2: a bf16 raw; "spline": every spline call, outer = ceil(C * HW / 256) blocks of positions, items =
    256 * B, io 1 whatever the alignment; "activation": every call of the smooth invertible activations, outer = B, items = C * HW / io
    with io 4 when C * HW % 4 == 0 at `align` 16), "mix" (family "mix").  Returns `io` (elements per thread item; the mix: pixels per lane),
    `threads` per workgroup, `grid`, `parts` (P or Q; the mix: waves of the grid; rows: 0), `items` (of one outer unit; the mix:
    chunks), `trips` of the busiest thread or wave, `outer`, `lds` bytes.  None: FINC_ERR_UNSUPPORTED (no mix instantiation for C; a
    "lead" whose channel count has one and runs the mix)."""
    info = (ctypes.c_longlong * 8)()
    st = lib().finc_debug_pixel_plan(PIXEL_RULES[rule], PIXEL_FAMILIES[rule][family], int(groups), B, C, HW, int(align), int(elem_bytes), info)
    if st == 3:
        return None
    check(st, "finc_debug_pixel_plan")
    return dict(zip(("io", "threads", "grid", "parts", "items", "trips", "outer", "lds"), (int(v) for v in info)))


F64_FAMILIES = ("none", "one_wave", "msplit")


def f64_plan(B, G, Cq, H, W, KH, KW):
    """What a float64 call on this shape launches (host-only; the launchers' own plan object): `family` 0 none (the reference-order and
    direct kernels), 1 one wave per problem, 2 the M-split over a workgroup's waves; `cqp` the padded bank; the inverse's `waves` per
    problem, `ppw` problems per workgroup, `lds` bytes per workgroup and `inv_grid`; `fwd_grid` (x, y) of the forward / grad-input -- slab and
    strip on x, B * G * ceil(W / 16), and y = 1 in both families (0, 0 without a kernel);
    the grad-weight's `gw_grid`, its `nrc` row chunks per slab of `RC` rows.  The forward's and the grad-weight's workgroups have one
    wave in family 1 and `waves` (one per 16-row output tile) in family 2."""
    info = (ctypes.c_int * 11)()
    check(lib().finc_debug_f64_plan(B, G, Cq, H, W, KH, KW, info), "finc_debug_f64_plan")
    v = [int(x) for x in info]
    return dict(family=v[0], cqp=v[1], waves=v[2], ppw=v[3], lds=v[4], inv_grid=v[5], fwd_grid=(v[6], v[7]), gw_grid=v[8], nrc=v[9], RC=v[10])


def set_forward_form(form):
    """Pin the 3x3 forward / grad-input kernel family for this process: 0 library's choice, 1 strip kernel, 2 Winograd F(2,3),
    4 Winograd F(4,3) (tests, A/B timing)."""
    check(lib().finc_debug_set_forward_form(int(form)), "finc_debug_set_forward_form")


def build_flags():
    """Measurement knobs the library was built with (0 = product build)."""
    return int(lib().finc_build_flags())


def runtime_switches():
    """FINC_* environment switches the library found set, plus a pinned forward form: [] = the library's own dispatch."""
    buf = ctypes.create_string_buffer(1024)
    n = lib().finc_runtime_switches(buf, len(buf))
    return [t for t in buf.value.decode().split(",") if t] if n else []


def clock_probe_begin(period_us=250, max_ms=3000):
    """Start the one-wave shader-clock probe on the current device (include/finc.h).  No device-wide synchronisation until
    clock_probe_end()."""
    check(lib().finc_debug_clock_probe_begin(int(period_us), int(max_ms)), "finc_debug_clock_probe_begin")


def clock_probe_end():
    st = (ctypes.c_double * 6)()
    check(lib().finc_debug_clock_probe_end(st), "finc_debug_clock_probe_end")
    return {"mean_mhz": st[0], "min_mhz": st[1], "max_mhz": st[2], "samples": int(st[3]), "seconds": st[4], "median_mhz": st[5]}


def fault_pending():
    """Has a helper-wave wait of an earlier launch on the current device given up (its output is garbage)?  Host-side read."""
    return bool(lib().finc_fault_pending())


def raise_if_faulted(where):
    if fault_pending():
        raise FincError(f"{where}: a helper-wave wait of an earlier launch on this device gave up -- its output is not valid "
                        "(fincflow_amd._lib.clear_fault() resets)")


def clear_fault():
    check(lib().finc_clear_fault(), "finc_clear_fault")


def hlp_timeouts():
    """Waits of the helper-wave inverse that gave up (must be 0)."""
    n = ctypes.c_uint(0)
    check(lib().finc_debug_hlp_timeouts(ctypes.byref(n)), "finc_debug_hlp_timeouts")
    return int(n.value)


def inverse_table():
    """Every row of the MFMA inverse instantiation table (host-only call)."""
    rows, r = [], 0
    info = (ctypes.c_int * 6)()
    while lib().finc_debug_inverse_table_row(r, info) == OK:
        rows.append(dict(zip(("cqp", "kh", "kw", "nw", "npw", "max_problems"), list(info))))
        r += 1
    return rows


def check(status, what):
    if status != OK:
        L = lib()
        msg = L.finc_status_string(status).decode()
        if status == 5:
            msg += ": " + L.finc_last_hip_error().decode()
        if status in (1, 2, 7):
            raise ValueError(f"{what}: {msg}")
        raise FincError(f"{what}: {msg}")
