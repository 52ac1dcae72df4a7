"""ctypes signature table of the C ABI declared in include/var_hip.h.

One table, two consumers: var_amd/hip.py binds `varhip_<name>(..., stream)` in libvar_hip.so (the product),
the CPU checker under oracle/ binds `varref_<name>(...)` in its own shared library.  Keeping the argument
lists in one place is what lets the parity tests drive both libraries with identical arguments.
"""
import ctypes as C

P = C.c_void_p
I = C.c_int
L = C.c_int64
F = C.c_float
D = C.c_double

# name -> argument ctypes (without the trailing stream of the HIP flavour); all return int
SIGNATURES = {
    'gemm_nt_f32':       [P, L, P, L, P, P, L, I, I, I, I, P, L, P, L, I, I, I, L, L, L],
    'silu_f32':          [P, P, L],
    'add_bcast_f32':     [P, P, P, I, I],
    'ln_modulate_f32':   [P, P, L, P, L, P, I, I, I, F],
    'qkv_prep_f32':      [P, P, F, I, P, P, P, I, I, I, I, I],
    'attn_cached_f32':   [P, P, P, P, I, I, I, I, I],
    'cfg_sample_f32':    [P, P, P, P, I, I, I, D, I, D],
    'quant_accum_f32':   [P, P, P, P, P, P, F, P, P, I, I, I, I],
    'next_map_f32':      [P, P, P, P, P, P, I, I, I, I, I],
    'lvl_pos_f32':       [P, P, P, P, I, I],
    'first_map_f32':     [P, P, I, P, P, P, P, I, I, I],
    'conv3x3_nhwc_f32':  [P, P, P, P, P, I, I, I, I, I, I, I],
    'gn_stats_f32':      [P, P, P, I, I, I, I, F],
    'gn_apply_f32':      [P, P, P, P, P, I, I, I, I, I],
    'softmax_rows_f32':  [P, P, L, I, F],
    'nchw_to_nhwc_f32':  [P, P, I, I, I],
    'nhwc_to_nchw_f32':  [P, P, I, I, I],
    'nearest_code_f32':  [P, P, P, I, I, I],
    'nearest_code_cos_f32': [P, P, P, I, I, I],
    'token_select_i64':  [P, P, P, P, L],
    'conv3x3_s2_nhwc_f32': [P, P, P, P, I, I, I, I, I],
    'nchw_to_nhwc_pad_f32': [P, P, I, I, I, I],
    'area_pool_f32':     [P, P, I, I, I, I],
    'word_embed_f32':    [P, P, P, P, P, I, I, I, I],
    'quant_residual_f32': [P, P, P, P, P, P, F, P, P, P, I, I, I, I],
    'upconv_pack_f32':   [P, P, I, I],
    'upconv_phase_f32':  [P, P, P, P, I, I, I, I, I],
    'quant_accum_h_f32': [P, P, P, P, P, F, P, P, I, I, I, I],
    'gumbel_softmax_f32': [P, P, P, L, I, F, F],
    'gemm_qkv_f32':      [P, L, P, L, P, I, I, I, P, F, I, P, P, P, I, I, I, I, I],
    'conv3x3_gn_nhwc_f32': [P, P, P, P, P, P, I, I, I, I, I, I],
    'upconv_phase_gn_f32': [P, P, P, P, P, I, I, I, I, I],
    'gn_stats_part_f32': [P, P, I, I, I, I, I, F],
    'adaln_block_f32':   [P, P, P, P, P, P, P, L, P, P, P, F, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, F],
    'neighbor_table_f32': [P, I, I, I, P, P],
    'smooth_select_f32': [P, P, P, P, I, I, I, F, F, I, I, I, D, P, P, P, P],
}

# the 16-bit throughput mode: HIP library only (its CPU twin is oracle/var_oracle.py with f16=True: the fp32 functions + rounding points)
SIGNATURES_F16 = {
    'gemm_nt_f16':       [P, L, P, L, P, P, L, I, I, I, I, I, P, L, I, P, L, I, I, L, L, L],
    'gemm_qkv_f16':      [P, L, P, L, P, I, I, I, P, F, I, P, P, P, I, I, I, I, I],
    'attn_cached_f16':   [P, P, P, P, I, I, I, I, I],
    'ln_modulate_f16out': [P, P, L, P, L, P, I, I, I, F],
    'adaln_block_f16':   [P, P, P, P, P, P, P, L, P, P, P, F, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, F],
    'conv3x3_nhwc_f16':  [P, P, P, P, P, P, I, I, I, I, I, I],
    'upconv_phase_f16':  [P, P, P, P, P, I, I, I, I, I],
    'gnconv3x3_nhwc_f16': [P, P, I, P, P, P, P, P, I, I, I, I, I],
    'gn_stats_f16':      [P, P, P, I, I, I, I, F],
    'gn_apply_f16':      [P, P, P, P, P, I, I, I, I, I],
    'gn_silu_conv_out_f16': [P, P, P, P, P, P, P, I, I, I, I, I, I, I],
    'cast_f32_to_f16':   [P, P, L],
    'cast_f16_to_f32':   [P, P, L],
}

# entry points of the HIP library that have no oracle twin of their own (they are pinned against other entry points bit for bit)
SIGNATURES_HIP_ONLY = {
    'gn_scale_shift_f32': [P, P, P, P, I, I, I],
    'gn_silu_conv_out_f32': [P, P, P, P, P, P, P, I, I, I, I, I, I, I],
    'token_loglik_f32':  [P, P, L, I, I, I, I, I, F, F, P, L, L],       # pinned against float64 log_softmax (tests/test_likelihood_gpu.py)
    'code_dist_f32':     [P, I, I, P],                                  # pinned against neighbor_table_f32 (tests/test_token_scores_gpu.py)
    'token_score_f32':   [P, P, L, I, I, I, I, I, F, F, I, I, F, P, L, P, L, L],   # pinned against float64 (tests/test_token_scores_gpu.py)
    'dist_profile_f32':  [P, P, L, I, I, I, I, I, F, F, P, L, P, I, F, P, P, L, L],   # pinned against float64 (tests/test_distance_profile_gpu.py)
    'class_mix_f32':     [P, P, L, I, I, I, I, I, F, F, P, L, P, L, L, P, P, P, L, P, P, P, P, L],   # pinned bit for bit against its host twin (tests/test_class_information_gpu.py)
    'class_mix_finish_f32': [P, P, P, L, P, L, I, I, I, P, P, P, P, L],
    'conv3x3_wino_nhwc_f32': [P, P, P, P, P, P, I, I, I, I, I],      # pinned against float64 and the direct conv (tests/test_winograd_gpu.py)
    'class_select_f32':  [P, L, L, I, I, I, I, P, I, P],             # pinned against a numpy lexsort of the rule (tests/test_classify_gpu.py)
    'cfg_argmax_f32':    [P, P, P, L, P, I, I, I, D],                # pinned against cfg_sample_f32(top_k=1) (tests/test_generative_gpu.py)
    'conv3x3_s2_nhwc_f16': [P, P, P, P, I, I, I, I, I],            # pinned against a CPU twin (tests/test_generative_gpu.py)
    'conv3x3_s2_nhwc_bf16': [P, P, P, P, I, I, I, I, I],
    'feature_l1_f32':    [P, P, P, L, L, P],                         # pinned against the torch L1 (tests/test_generative_gpu.py)
    'edit_keep_u8':      [P, I, I, I, P, I, I, P],                   # pinned against F.interpolate > 0.5 and the reference's maps (tests/test_edit_gpu.py)
    'quant_accum_edit_f32': [P, P, P, L, P, P, P, P, P, F, P, P, I, I, I, I],     # pinned against token_select_i64 + quant_accum_f32 (tests/test_edit_gpu.py)
    'quant_accum_h_edit_f32': [P, P, P, L, P, P, P, P, P, F, P, P, I, I, I, I],   # pinned against an overwrite of h + quant_accum_h_f32
    'cfg_sample_rows_f32': [P, P, P, P, I, I, I, P, P, P, I],         # pinned against cfg_sample_f32 per image (tests/test_per_image_gpu.py)
    'exp1_philox_f32':   [P, I, I, I, I, I, P],                      # pinned against its host twin below (tests/test_per_image_gpu.py)
    'vq_scale_stats_f32': [P, P, L, P, L, I, P, P, P, P, P],          # pinned against torch.bincount and a numpy float64 sum (tests/test_vae_forward_gpu.py)
    'vq_loss_combine_f32': [P, I, F, P],                             # pinned against the fp32 sequence in torch
    'vq_straight_through_f32': [P, P, P, P, I, I, I],                # pinned against (f_hat - f) + f in torch, bit for bit
    'token_eval_f32':    [P, P, L, I, I, I, P, P, P, P, L],             # pinned against float64, torch.argmax and the rank's definition (tests/test_evaluate_gpu.py)
    'eval_reduce_f32':   [P, P, P, P, L, I, P, I, I, P, P, P, P],       # pinned against numpy float64 sums and torch.bincount; begin_S1 is a host array
    'sample_stats_f32':  [P, P, P, I, I, I, D, P, P, P, P, P, P, L],    # pinned against its host twin, token_loglik_f32 and float64 (tests/test_sample_stats_gpu.py)
    'attn_profile_f32':  [P, P, I, I, I, I, I, P, I, I, I, P, L, L, P, P, L, L],      # pinned bit for bit against its host twin (tests/test_attention_profile_gpu.py); ends is a host array
    'evidence_reduce_f32': [P, L, L, I, I, I, P, P, P, P, P, I, P, P, P, P, P, P],   # pinned bit for bit against evidence_maps_torch (tests/test_evidence_gpu.py); pn, begin, w are host arrays
    'evidence_overlay_u8': [P, L, L, I, I, I, P, P, P, P, P, I, P, P, P, I, D, P],   # pinned byte for byte against evidence_maps_torch
    'kv_compact':        [P, P, I, P, I, I, I, I, I, I, I],             # pinned byte for byte against numpy's gather (tests/test_kv_compact_gpu.py); src, dst are host arrays of pointers
    'kv_resample':       [P, I, P, I, I, I, I, I, P],                   # pinned byte for byte against numpy's gather on a copy (tests/test_smc_kernels_gpu.py); bufs is a host array of pointers
    'smc_resample_f32':  [P, L, L, I, I, I, I, D, P, P, I, D, P, P, P, P],   # pinned bit for bit against its host twin (tests/test_smc_kernels_gpu.py)
}

# plain host functions of the HIP library (no stream argument, no device pointer, no GPU needed); bound by var_amd/hip.py
SIGNATURES_HOST = {
    'exp1_philox_host_f32': [P, I, I, I, I, I, P],                   # pinned against a numpy Philox4x32-10 (tests/test_per_image_cpu.py)
    'philox4x32_host':   [P, P, P],                                  # pinned against the Random123 known answers
    'exp1_from_bits_host_f32': [P, L, P],
    'sample_stats_host_f32': [P, P, P, I, I, I, D, P, P, P, P, P, P, L],   # pinned against float64 (tests/test_sample_stats_cpu.py)
    'class_mix_host_f32': [P, P, L, I, I, I, I, I, F, F, P, L, P, L, L, P, P, P, L, P, P, P, P, L],   # pinned against float64 (tests/test_class_information_cpu.py)
    'class_mix_finish_host_f32': [P, P, P, L, P, L, I, I, I, P, P, P, P, L],
    'attn_profile_host_f32': [P, P, I, I, I, I, I, P, I, I, I, P, L, L, P, P, L, L],   # pinned against float64 (tests/test_attention_profile_cpu.py)
    'smc_resample_host_f32': [P, L, L, I, I, I, I, D, P, P, I, D, P, P, P, P],   # pinned against a numpy restatement of the contract (tests/test_smc_resample_cpu.py)
    'evidence_jet_host': [P],                                       # pinned against matplotlib's 'jet' (tests/test_evidence_cpu.py)
}

# ... and with bfloat16 storage: one entry point per _f16 entry point, same arguments (include/var_hip.h, "bf16")
SIGNATURES_BF16 = {k.replace('_f16out', '_bf16out').replace('_to_f16', '_to_bf16').replace('cast_f16_', 'cast_bf16_').replace('_f16', '_bf16'): v
                   for k, v in SIGNATURES_F16.items()}

EPI_NONE, EPI_GELU, EPI_RESID = 0, 1, 2
EINVAL = -1


def bind(lib, prefix: str, with_stream: bool):
    """Attach argtypes/restype to every ABI function of `lib`; raises AttributeError naming a missing symbol."""
    fns = {}
    table = dict(SIGNATURES)
    if with_stream:                      # the HIP library also carries the 16-bit mode
        table.update(SIGNATURES_F16)
        table.update(SIGNATURES_BF16)
        table.update(SIGNATURES_HIP_ONLY)
    for name, args in table.items():
        fn = getattr(lib, prefix + name)
        fn.argtypes = list(args) + ([P] if with_stream else [])
        fn.restype = I
        fns[name] = fn
    gs = getattr(lib, prefix + 'gn_scratch_elems')
    gs.argtypes = [I, I, I, I]
    gs.restype = L
    fns['gn_scratch_elems'] = gs
    cb = getattr(lib, prefix + 'conv_gn_blocks')
    cb.argtypes = [I, I, I, I]
    cb.restype = I
    fns['conv_gn_blocks'] = cb
    if with_stream:
        cf = getattr(lib, prefix + 'conv16_gn_fusable')
        cf.argtypes = [I, I, I, I, I]
        cf.restype = I
        fns['conv16_gn_fusable'] = cf
    ver = getattr(lib, prefix + 'version')
    ver.argtypes = []
    ver.restype = C.c_char_p
    fns['version'] = ver
    return fns
