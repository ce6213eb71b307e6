"""ctypes binding of ``libfishvoc_hip.so`` (include/fishvoc.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises
``ImportError`` loudly, and every op requires CUDA(HIP) tensors.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# FV_LIB_PATH points the loader at an experimental build (A/B kernel variants); default = the in-tree library
LIB_PATH = os.environ.get("FV_LIB_PATH") or os.path.join(CSRC, "libfishvoc_hip.so")

FV_ABI_VERSION = 5
FV_OK, FV_ERR_INVALID, FV_ERR_UNSUPPORTED, FV_ERR_STATE = 0, -1, -2, -6
FV_MAX_STAGES = 8
FV_MAX_KERNELS = 8
FV_MAX_DILATIONS = 3

FV_MODEL_HIFIGAN, FV_MODEL_BIGVGAN, FV_MODEL_VOCOS, FV_MODEL_FIREFLY, FV_MODEL_CONVNEXT, FV_MODEL_ISTFT_HEAD = 1, 2, 3, 4, 5, 6
FV_MODEL_LOGMEL = 7
FV_MODEL_REFINEGAN = 8
FV_PRECISION_F32, FV_PRECISION_F16X3 = 0, 1
PRECISIONS = {"f32": FV_PRECISION_F32, "f16x3": FV_PRECISION_F16X3}
FV_CONV_ALGO_AUTO, FV_CONV_ALGO_DIRECT, FV_CONV_ALGO_WINOGRAD = 0, 1, 2
CONV_ALGOS = {"auto": FV_CONV_ALGO_AUTO, "direct": FV_CONV_ALGO_DIRECT, "winograd": FV_CONV_ALGO_WINOGRAD}
FV_ISTFT_SAME, FV_ISTFT_CENTER = 0, 1
FV_ACT_NONE, FV_ACT_SILU, FV_ACT_LEAKY_RELU, FV_ACT_GELU, FV_ACT_TANH, FV_ACT_LOG_CLAMP = 0, 1, 2, 3, 4, 5
FV_RESAMPLE_SINC_HANN, FV_RESAMPLE_SINC_KAISER = 0, 1
RESAMPLE_METHODS = {"sinc_interp_hann": FV_RESAMPLE_SINC_HANN, "sinc_interp_kaiser": FV_RESAMPLE_SINC_KAISER}
FV_SPEC_DISTANCE_LOG = 1     # fv_spec_distance flags: also form S_log = sum |log ref - log est|
FV_TEMPLATE_SINE, FV_TEMPLATE_SAWTOOTH = 0, 1
TEMPLATE_KINDS = {"sine": FV_TEMPLATE_SINE, "sawtooth": FV_TEMPLATE_SAWTOOTH}
FV_POST_ACT_DEFAULT, FV_POST_ACT_IDENTITY = 0, -1   # fv_upsampler_config.post_activation (ABI 5): 0 = reference default SiLU, -1 = nn.Identity

EXPORTS = (
    "fv_create", "fv_load_weight", "fv_finalize", "fv_destroy", "fv_output_length", "fv_output_channels",
    "fv_input_channels", "fv_workspace_bytes", "fv_forward", "fv_conv_create", "fv_conv_output_length",
    "fv_conv_forward", "fv_conv_destroy", "fv_last_error", "fv_abi_version", "fv_last_kernel",
    "fv_profile_begin", "fv_profile_end", "fv_conv_pair_forward", "fv_forward_template",
    "fv_set_precision", "fv_conv_set_precision", "fv_refinegan_noise_elems", "fv_forward_refinegan",
    "fv_refinegan_set_noise_seed", "fv_refinegan_clear_noise_seed", "fv_forward_refinegan_seeded", "fv_refinegan_fill_noise",
    "fv_set_graph_replay", "fv_get_graph_replay", "fv_reload_env", "fv_set_conv_algorithm", "fv_set_batch_invariant", "fv_conv_set_algorithm",
    "fv_reach_frames", "fv_stream_create", "fv_stream_workspace_bytes", "fv_stream_pending_frames", "fv_stream_push", "fv_stream_flush",
    "fv_stream_reset", "fv_stream_destroy",
    "fv_ragged_plan", "fv_ragged_create", "fv_ragged_workspace_bytes", "fv_ragged_num_groups", "fv_ragged_group", "fv_ragged_windows",
    "fv_ragged_forward", "fv_ragged_destroy",
    "fv_pool_plan", "fv_pool_create", "fv_pool_workspace_bytes", "fv_pool_pending_frames", "fv_pool_step", "fv_pool_reset", "fv_pool_destroy",
    "fv_resample_design", "fv_resample_input_tile", "fv_resample_create", "fv_resample_destroy", "fv_resample_output_length",
    "fv_resample_forward", "fv_resample_check_lengths", "fv_resample_stream_create", "fv_resample_stream_pending", "fv_resample_stream_push",
    "fv_resample_stream_flush", "fv_resample_stream_reset", "fv_resample_stream_destroy",
    "fv_logmel_frames", "fv_logmel_frames_ready", "fv_logmel_ragged_forward", "fv_logmel_stream_create", "fv_logmel_stream_workspace_bytes",
    "fv_logmel_stream_pending_samples", "fv_logmel_stream_push", "fv_logmel_stream_flush", "fv_logmel_stream_reset", "fv_logmel_stream_destroy",
    "fv_wavpool_create", "fv_wavpool_workspace_bytes", "fv_wavpool_max_frames", "fv_wavpool_received_samples", "fv_wavpool_emitted_frames",
    "fv_wavpool_pending_samples", "fv_wavpool_plan", "fv_wavpool_step", "fv_wavpool_reset", "fv_wavpool_destroy",
    "fv_global_resample_create",
    "fv_respool_create", "fv_respool_max_outputs", "fv_respool_received", "fv_respool_emitted", "fv_respool_pending", "fv_respool_plan",
    "fv_respool_step", "fv_respool_reset", "fv_respool_destroy",
    "fv_pitch_shift_plan", "fv_pitch_shift_lengths", "fv_pitch_shift_create", "fv_pitch_shift_destroy", "fv_pitch_shift_workspace_bytes",
    "fv_pitch_shift_stretch", "fv_pitch_shift_forward",
    "fv_pv_stream_ready", "fv_pv_set_batch_invariant", "fv_pv_stream_create", "fv_pv_stream_workspace_bytes", "fv_pv_stream_pending",
    "fv_pv_stream_push", "fv_pv_stream_flush", "fv_pv_stream_reset", "fv_pv_stream_destroy",
    "fv_pvpool_create", "fv_pvpool_workspace_bytes", "fv_pvpool_max_outputs", "fv_pvpool_received", "fv_pvpool_emitted", "fv_pvpool_pending",
    "fv_pvpool_bounds", "fv_pvpool_plan", "fv_pvpool_step", "fv_pvpool_reset", "fv_pvpool_destroy",
    "fv_spec_distance_tile", "fv_spec_distance_workspace_bytes", "fv_spec_distance",
    "fv_f0_plan", "fv_f0_create", "fv_f0_destroy", "fv_f0_workspace_bytes", "fv_f0_forward",
    "fv_template_create", "fv_template_destroy", "fv_template_workspace_bytes", "fv_template_forward",
    "fv_yin_frames_ready", "fv_yin_stream_create", "fv_yin_stream_pending_samples", "fv_yin_stream_push", "fv_yin_stream_flush",
    "fv_yin_stream_reset", "fv_yin_stream_destroy",
    "fv_osc_stream_create", "fv_osc_stream_pending_frames", "fv_osc_stream_push", "fv_osc_stream_flush", "fv_osc_stream_reset",
    "fv_osc_stream_destroy",
    "fv_yinpool_create", "fv_yinpool_max_frames", "fv_yinpool_received", "fv_yinpool_emitted", "fv_yinpool_pending", "fv_yinpool_plan",
    "fv_yinpool_step", "fv_yinpool_reset", "fv_yinpool_destroy",
    "fv_oscpool_create", "fv_oscpool_max_frames", "fv_oscpool_received", "fv_oscpool_emitted", "fv_oscpool_pending", "fv_oscpool_plan",
    "fv_oscpool_step", "fv_oscpool_reset", "fv_oscpool_destroy",
    "fv_pair_wino4_tile", "fv_pair_wino4_pack",
    "fv_vq_create", "fv_vq_destroy", "fv_vq_load_codebook", "fv_vq_set_slices", "fv_vq_workspace_bytes", "fv_vq_encode", "fv_vq_decode",
    "fv_stream_create_codes", "fv_stream_push_codes", "fv_codepool_create", "fv_codepool_step", "fv_stream_ring_bytes", "fv_codepool_ring_bytes",
    "fv_posterior_create", "fv_posterior_load_weight", "fv_posterior_finalize", "fv_posterior_reach_frames", "fv_posterior_output_channels",
    "fv_posterior_workspace_bytes", "fv_posterior_forward", "fv_posterior_destroy",
    "fv_wnstream_create", "fv_wnstream_push", "fv_wnstream_flush", "fv_wnstream_reset", "fv_wnstream_pending", "fv_wnstream_lookahead",
    "fv_wnstream_destroy",
    "fv_wnpool_create", "fv_wnpool_plan", "fv_wnpool_step", "fv_wnpool_reset", "fv_wnpool_received", "fv_wnpool_emitted", "fv_wnpool_pending",
    "fv_wnpool_lookahead", "fv_wnpool_max_frames", "fv_wnpool_launches", "fv_wnpool_destroy",
    "fv_w2v_create", "fv_w2v_load_weight", "fv_w2v_finalize", "fv_w2v_frames", "fv_w2v_workspace_bytes", "fv_w2v_forward", "fv_w2v_destroy",
    "fv_mms_normalize_workspace_bytes", "fv_mms_normalize", "fv_mms_interpolate", "fv_mms_nearest_index",
    "fv_cnxstream_create", "fv_cnxstream_push", "fv_cnxstream_flush", "fv_cnxstream_reset", "fv_cnxstream_pending", "fv_cnxstream_lookahead",
    "fv_cnxstream_state_bytes", "fv_cnxstream_destroy", "fv_cnxstream_plan",
    "fv_cnxpool_create", "fv_cnxpool_plan", "fv_cnxpool_step", "fv_cnxpool_reset", "fv_cnxpool_received", "fv_cnxpool_emitted",
    "fv_cnxpool_pending", "fv_cnxpool_lookahead", "fv_cnxpool_max_frames", "fv_cnxpool_launches", "fv_cnxpool_state_bytes",
    "fv_cnxpool_table_size", "fv_cnxpool_destroy",
    "fv_aa_snake_forward", "fv_dwconv_ln_forward",
    "fv_disc_create", "fv_disc_load_weight", "fv_disc_finalize", "fv_disc_destroy", "fv_disc_layout", "fv_disc_workspace_bytes",
    "fv_disc_forward", "fv_disc_distance",
)

_i32 = ctypes.c_int32


class UpsamplerConfig(ctypes.Structure):
    _fields_ = [
        ("hop_length", _i32), ("num_upsamples", _i32),
        ("upsample_rates", _i32 * FV_MAX_STAGES), ("upsample_kernel_sizes", _i32 * FV_MAX_STAGES),
        ("num_kernels", _i32), ("resblock_kernel_sizes", _i32 * FV_MAX_KERNELS),
        ("resblock_dilation_sizes", (_i32 * FV_MAX_DILATIONS) * FV_MAX_KERNELS),
        ("num_mels", _i32), ("upsample_initial_channel", _i32), ("use_template", _i32),
        ("pre_conv_kernel_size", _i32), ("post_conv_kernel_size", _i32),
        ("post_activation", _i32), ("post_activation_slope", ctypes.c_float),
    ]


class ConvNeXtConfig(ctypes.Structure):
    _fields_ = [("input_channels", _i32), ("num_stages", _i32), ("depths", _i32 * FV_MAX_STAGES),
                ("dims", _i32 * FV_MAX_STAGES), ("kernel_size", _i32)]


class IstftHeadConfig(ctypes.Structure):
    _fields_ = [("dim", _i32), ("n_fft", _i32), ("hop_length", _i32), ("win_length", _i32), ("padding", _i32)]


class LogMelConfig(ctypes.Structure):
    _fields_ = [("sample_rate", _i32), ("n_fft", _i32), ("win_length", _i32), ("hop_length", _i32), ("n_mels", _i32),
                ("f_min", ctypes.c_float), ("f_max", ctypes.c_float)]


class RefineGANConfig(ctypes.Structure):
    _fields_ = [("hop_length", _i32), ("num_stages", _i32), ("downsample_rates", _i32 * FV_MAX_STAGES),
                ("upsample_rates", _i32 * FV_MAX_STAGES), ("num_mels", _i32), ("start_channels", _i32),
                ("leaky_relu_slope", ctypes.c_float)]


class Config(ctypes.Structure):
    _fields_ = [("abi_version", _i32), ("model", _i32), ("ups", UpsamplerConfig), ("backbone", ConvNeXtConfig),
                ("head", IstftHeadConfig), ("mel", LogMelConfig), ("refine", RefineGANConfig)]


class ConvDesc(ctypes.Structure):
    _fields_ = [("transposed", _i32), ("c_in", _i32), ("c_out", _i32), ("kernel_size", _i32), ("dilation", _i32),
                ("padding", _i32), ("stride", _i32), ("pre_act", _i32), ("post_act", _i32),
                ("act_slope", ctypes.c_float)]


class StreamConfig(ctypes.Structure):
    _fields_ = [("batch", _i32), ("max_chunk_frames", _i32), ("context_frames", _i32), ("lookahead_frames", _i32)]


class RaggedWindow(ctypes.Structure):
    _fields_ = [("clip", _i32), ("start", _i32), ("frames", _i32), ("keep_lo", _i32), ("keep_hi", _i32), ("group", _i32)]


class PoolConfig(ctypes.Structure):
    _fields_ = [("sessions", _i32), ("max_chunk_frames", _i32), ("context_frames", _i32), ("lookahead_frames", _i32)]


class PoolItem(ctypes.Structure):
    _fields_ = [("session", _i32), ("frames", _i32), ("flush", _i32)]


class WavPoolItem(ctypes.Structure):
    _fields_ = [("session", _i32), ("samples", _i32), ("flush", _i32)]


class PoolRow(ctypes.Structure):
    _fields_ = [("item", _i32), ("group", _i32), ("col0", _i32), ("frames", _i32), ("w", ctypes.c_int64), ("emit_lo", ctypes.c_int64),
                ("emit_hi", ctypes.c_int64)]


class ResampleConfig(ctypes.Structure):
    _fields_ = [("orig_freq", _i32), ("new_freq", _i32), ("lowpass_filter_width", _i32), ("rolloff", ctypes.c_double), ("method", _i32),
                ("beta", ctypes.c_double)]


class PitchShiftConfig(ctypes.Structure):
    _fields_ = [("sample_rate", _i32), ("n_steps", ctypes.c_double), ("bins_per_octave", _i32), ("n_fft", _i32), ("hop_length", _i32),
                ("freq_granularity", _i32), ("lowpass_filter_width", _i32), ("rolloff", ctypes.c_double), ("method", _i32),
                ("beta", ctypes.c_double)]


class F0Config(ctypes.Structure):
    _fields_ = [("sample_rate", _i32), ("frame_length", _i32), ("hop_length", _i32), ("fmin", ctypes.c_double), ("fmax", ctypes.c_double),
                ("threshold", ctypes.c_double)]


class TemplateConfig(ctypes.Structure):
    _fields_ = [("sample_rate", _i32), ("hop_length", _i32), ("kind", _i32), ("amplitude", ctypes.c_float)]


class VQConfig(ctypes.Structure):
    _fields_ = [("dim", _i32), ("codebook_size", _i32), ("num_quantizers", _i32)]


POSTERIOR_MODES = {"vqvae": 0, "vae": 1, "bnvae": 2}


class PosteriorConfig(ctypes.Structure):
    _fields_ = [("in_channels", _i32), ("out_channels", _i32), ("hidden_channels", _i32), ("kernel_size", _i32), ("dilation_rate", _i32),
                ("dilation_cycle", _i32), ("n_layers", _i32), ("mode", _i32)]


W2V_MAX_CONV = 8


class W2VConfig(ctypes.Structure):
    """fv_w2v_config, field for field (include/fishvoc.h)."""
    _fields_ = [("hidden", _i32), ("layers", _i32), ("heads", _i32), ("intermediate", _i32), ("n_conv", _i32),
                ("conv_dim", _i32 * W2V_MAX_CONV), ("conv_kernel", _i32 * W2V_MAX_CONV), ("conv_stride", _i32 * W2V_MAX_CONV),
                ("pos_conv_kernel", _i32), ("pos_conv_groups", _i32), ("post_channels", _i32)]


FV_DISC_PERIOD, FV_DISC_RESOLUTION = 0, 1
DISC_MAX_SUB = 8
DISC_MAX_CHANNELS = 8


class DiscConfig(ctypes.Structure):
    """fv_disc_config, field for field (include/fishvoc.h)."""
    _fields_ = [("kind", _i32), ("n_sub", _i32), ("period", _i32 * DISC_MAX_SUB), ("n_fft", _i32 * DISC_MAX_SUB),
                ("hop_length", _i32 * DISC_MAX_SUB), ("win_length", _i32 * DISC_MAX_SUB), ("n_channels", _i32),
                ("channels", _i32 * DISC_MAX_CHANNELS), ("kernel_size", _i32), ("stride", _i32)]


class DiscMap(ctypes.Structure):
    """fv_disc_map, field for field."""
    _fields_ = [("offset", ctypes.c_int64), ("H", _i32), ("W", _i32), ("C", _i32), ("sub", _i32), ("layer", _i32)]


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean", "-s"])
    subprocess.check_call(["make", "-C", CSRC, f"-j{jobs}", "-s"])
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C vocoder_amd/csrc`). "
            "vocoder_amd has no CPU fallback.")
    # torch first: its wheel carries its own HIP runtime (torch/lib/libamdhip64.so), and the process must end up with ONE — loaded after torch, this
    # library's libamdhip64.so.7 dependency resolves to the copy torch already mapped; loaded before it, the system runtime comes in as a second one and
    # its first hipMalloc fails with "no ROCm-capable device is detected" once torch has initialised the device (build() followed by smoke() in one process)
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    vp, cp = ctypes.c_void_p, ctypes.c_char_p
    fp = ctypes.POINTER(ctypes.c_float)
    L.fv_create.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(vp)]
    L.fv_create.restype = _i32
    L.fv_load_weight.argtypes = [vp, cp, fp, ctypes.POINTER(ctypes.c_int64), _i32]
    L.fv_load_weight.restype = _i32
    L.fv_finalize.argtypes = [vp]
    L.fv_finalize.restype = _i32
    L.fv_destroy.argtypes = [vp]
    L.fv_destroy.restype = None
    L.fv_output_length.argtypes = [vp, _i32]
    L.fv_output_length.restype = ctypes.c_int64
    L.fv_output_channels.argtypes = [vp]
    L.fv_output_channels.restype = _i32
    L.fv_input_channels.argtypes = [vp]
    L.fv_input_channels.restype = _i32
    L.fv_workspace_bytes.argtypes = [vp, _i32, _i32]
    L.fv_workspace_bytes.restype = ctypes.c_size_t
    L.fv_forward.argtypes = [vp, vp, vp, _i32, _i32, vp, ctypes.c_size_t, vp]
    L.fv_forward.restype = _i32
    L.fv_forward_template.argtypes = [vp, vp, vp, vp, _i32, _i32, vp, ctypes.c_size_t, vp]
    L.fv_forward_template.restype = _i32
    L.fv_refinegan_noise_elems.argtypes = [vp, _i32, _i32]
    L.fv_refinegan_noise_elems.restype = ctypes.c_int64
    L.fv_forward_refinegan.argtypes = [vp, vp, vp, vp, vp, _i32, _i32, vp, ctypes.c_size_t, vp]
    L.fv_forward_refinegan.restype = _i32
    L.fv_refinegan_set_noise_seed.argtypes = [vp, ctypes.c_uint64, _i32]
    L.fv_refinegan_set_noise_seed.restype = _i32
    L.fv_refinegan_clear_noise_seed.argtypes = [vp]
    L.fv_refinegan_clear_noise_seed.restype = _i32
    L.fv_forward_refinegan_seeded.argtypes = [vp, vp, vp, vp, _i32, _i32, ctypes.c_int64, vp, ctypes.c_size_t, vp]
    L.fv_forward_refinegan_seeded.restype = _i32
    L.fv_refinegan_fill_noise.argtypes = [vp, vp, _i32, _i32, ctypes.c_int64, vp]
    L.fv_refinegan_fill_noise.restype = _i32
    L.fv_conv_create.argtypes = [ctypes.POINTER(ConvDesc), fp, fp, ctypes.POINTER(vp)]
    L.fv_conv_create.restype = _i32
    L.fv_conv_output_length.argtypes = [vp, _i32]
    L.fv_conv_output_length.restype = ctypes.c_int64
    L.fv_conv_forward.argtypes = [vp, vp, vp, vp, _i32, _i32, vp]
    L.fv_conv_forward.restype = _i32
    L.fv_conv_destroy.argtypes = [vp]
    L.fv_conv_destroy.restype = None
    L.fv_conv_pair_forward.argtypes = [vp, vp, vp, vp, _i32, _i32, vp]
    L.fv_conv_pair_forward.restype = _i32
    L.fv_aa_snake_forward.argtypes = [vp] * 8 + [_i32, _i32, ctypes.c_int64, vp]
    L.fv_aa_snake_forward.restype = _i32
    L.fv_dwconv_ln_forward.argtypes = [vp] * 6 + [_i32, _i32, ctypes.c_int64, _i32, ctypes.c_float, vp]
    L.fv_dwconv_ln_forward.restype = _i32
    L.fv_set_precision.argtypes = [vp, _i32]
    L.fv_set_precision.restype = _i32
    L.fv_reload_env.argtypes = []
    L.fv_reload_env.restype = None
    L.fv_set_graph_replay.argtypes = [vp, _i32]
    L.fv_set_graph_replay.restype = _i32
    L.fv_get_graph_replay.argtypes = [vp]
    L.fv_get_graph_replay.restype = _i32
    L.fv_set_conv_algorithm.argtypes = [vp, _i32]
    L.fv_set_conv_algorithm.restype = _i32
    L.fv_set_batch_invariant.argtypes = [vp, _i32]
    L.fv_set_batch_invariant.restype = _i32
    L.fv_conv_set_algorithm.argtypes = [vp, _i32]
    L.fv_conv_set_algorithm.restype = _i32
    L.fv_conv_set_precision.argtypes = [vp, _i32]
    L.fv_conv_set_precision.restype = _i32
    L.fv_profile_begin.argtypes = [vp]
    L.fv_profile_begin.restype = _i32
    L.fv_profile_end.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.fv_profile_end.restype = _i32
    L.fv_reach_frames.argtypes = [vp]
    L.fv_reach_frames.restype = _i32
    L.fv_stream_create.argtypes = [vp, ctypes.POINTER(StreamConfig), ctypes.POINTER(vp)]
    L.fv_stream_create.restype = _i32
    L.fv_stream_workspace_bytes.argtypes = [vp]
    L.fv_stream_workspace_bytes.restype = ctypes.c_size_t
    L.fv_stream_pending_frames.argtypes = [vp]
    L.fv_stream_pending_frames.restype = ctypes.c_int64
    i64p = ctypes.POINTER(ctypes.c_int64)
    L.fv_stream_push.argtypes = [vp, vp, vp, _i32, vp, i64p, vp, ctypes.c_size_t, vp]
    L.fv_stream_push.restype = _i32
    L.fv_stream_flush.argtypes = [vp, vp, i64p, vp, ctypes.c_size_t, vp]
    L.fv_stream_flush.restype = _i32
    L.fv_stream_reset.argtypes = [vp]
    L.fv_stream_reset.restype = _i32
    L.fv_stream_destroy.argtypes = [vp]
    L.fv_stream_destroy.restype = None
    i32p, rwp = ctypes.POINTER(_i32), ctypes.POINTER(RaggedWindow)
    L.fv_ragged_plan.argtypes = [_i32, i32p, _i32, _i32, _i32, rwp, _i32]
    L.fv_ragged_plan.restype = _i32
    L.fv_ragged_create.argtypes = [vp, i32p, _i32, _i32, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_ragged_create.restype = _i32
    L.fv_ragged_workspace_bytes.argtypes = [vp]
    L.fv_ragged_workspace_bytes.restype = ctypes.c_size_t
    L.fv_ragged_num_groups.argtypes = [vp]
    L.fv_ragged_num_groups.restype = _i32
    L.fv_ragged_group.argtypes = [vp, _i32, i32p, i32p]
    L.fv_ragged_group.restype = _i32
    L.fv_ragged_windows.argtypes = [vp, rwp, _i32]
    L.fv_ragged_windows.restype = _i32
    L.fv_ragged_forward.argtypes = [vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.fv_ragged_forward.restype = _i32
    L.fv_ragged_destroy.argtypes = [vp]
    L.fv_ragged_destroy.restype = None
    pip, prp = ctypes.POINTER(PoolItem), ctypes.POINTER(PoolRow)
    L.fv_pool_plan.argtypes = [ctypes.POINTER(PoolConfig), i64p, i64p, i32p, pip, _i32, _i32, _i32, prp, _i32, i32p, i32p, _i32, i32p]
    L.fv_pool_plan.restype = _i32
    L.fv_pool_create.argtypes = [vp, ctypes.POINTER(PoolConfig), ctypes.POINTER(vp)]
    L.fv_pool_create.restype = _i32
    L.fv_pool_workspace_bytes.argtypes = [vp]
    L.fv_pool_workspace_bytes.restype = ctypes.c_size_t
    L.fv_pool_pending_frames.argtypes = [vp, _i32]
    L.fv_pool_pending_frames.restype = ctypes.c_int64
    L.fv_pool_step.argtypes = [vp, pip, _i32, vp, vp, _i32, vp, _i32, i64p, vp, ctypes.c_size_t, vp]
    L.fv_pool_step.restype = _i32
    L.fv_pool_reset.argtypes = [vp, _i32]
    L.fv_pool_reset.restype = _i32
    L.fv_pool_destroy.argtypes = [vp]
    L.fv_pool_destroy.restype = None
    rcp, i64 = ctypes.POINTER(ResampleConfig), ctypes.c_int64
    L.fv_resample_design.argtypes = [rcp, i32p, i32p, i32p, i32p, i32p, i32p, _i32, fp, i64]
    L.fv_resample_design.restype = _i32
    L.fv_resample_input_tile.argtypes = []
    L.fv_resample_input_tile.restype = _i32
    L.fv_resample_create.argtypes = [rcp, ctypes.POINTER(vp)]
    L.fv_resample_create.restype = _i32
    L.fv_resample_destroy.argtypes = [vp]
    L.fv_resample_destroy.restype = None
    L.fv_resample_output_length.argtypes = [vp, i64]
    L.fv_resample_output_length.restype = i64
    L.fv_resample_forward.argtypes = [vp, vp, i64, vp, vp, i64, _i32, i64, vp]
    L.fv_resample_forward.restype = _i32
    L.fv_resample_check_lengths.argtypes = [vp, i32p, _i32, i64]
    L.fv_resample_check_lengths.restype = _i32
    L.fv_resample_stream_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_resample_stream_create.restype = _i32
    L.fv_resample_stream_pending.argtypes = [vp]
    L.fv_resample_stream_pending.restype = i64
    L.fv_resample_stream_push.argtypes = [vp, vp, i64, _i32, vp, i64, i64p, vp]
    L.fv_resample_stream_push.restype = _i32
    L.fv_resample_stream_flush.argtypes = [vp, vp, i64, i64p, vp]
    L.fv_resample_stream_flush.restype = _i32
    L.fv_resample_stream_reset.argtypes = [vp]
    L.fv_resample_stream_reset.restype = _i32
    L.fv_resample_stream_destroy.argtypes = [vp]
    L.fv_resample_stream_destroy.restype = None
    lcp = ctypes.POINTER(LogMelConfig)
    L.fv_logmel_frames.argtypes = [lcp, i64]
    L.fv_logmel_frames.restype = i64
    L.fv_logmel_frames_ready.argtypes = [lcp, i64]
    L.fv_logmel_frames_ready.restype = i64
    L.fv_logmel_ragged_forward.argtypes = [vp, vp, i64, i32p, _i32, _i32, vp, vp, ctypes.c_size_t, vp]
    L.fv_logmel_ragged_forward.restype = _i32
    L.fv_logmel_stream_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_logmel_stream_create.restype = _i32
    L.fv_logmel_stream_workspace_bytes.argtypes = [vp]
    L.fv_logmel_stream_workspace_bytes.restype = ctypes.c_size_t
    L.fv_logmel_stream_pending_samples.argtypes = [vp]
    L.fv_logmel_stream_pending_samples.restype = i64
    L.fv_logmel_stream_push.argtypes = [vp, vp, i64, _i32, vp, i64p, vp, ctypes.c_size_t, vp]
    L.fv_logmel_stream_push.restype = _i32
    L.fv_logmel_stream_flush.argtypes = [vp, vp, i64p, vp, ctypes.c_size_t, vp]
    L.fv_logmel_stream_flush.restype = _i32
    L.fv_logmel_stream_reset.argtypes = [vp]
    L.fv_logmel_stream_reset.restype = _i32
    L.fv_logmel_stream_destroy.argtypes = [vp]
    L.fv_logmel_stream_destroy.restype = None
    wip = ctypes.POINTER(WavPoolItem)
    # the sample pools (csrc/sample_pool.h): create, the counters, reset and destroy have one signature; the wav pool's counters have longer names
    for pre, received, emitted, pending in (("fv_wavpool", "_received_samples", "_emitted_frames", "_pending_samples"),
                                            ("fv_respool", "_received", "_emitted", "_pending"), ("fv_pvpool", "_received", "_emitted", "_pending"),
                                            ("fv_yinpool", "_received", "_emitted", "_pending"), ("fv_oscpool", "_received", "_emitted", "_pending")):
        getattr(L, pre + "_create").argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
        getattr(L, pre + "_create").restype = _i32
        for name in (received, emitted, pending):
            getattr(L, pre + name).argtypes = [vp, _i32]
            getattr(L, pre + name).restype = i64
        getattr(L, pre + "_reset").argtypes = [vp, _i32]
        getattr(L, pre + "_reset").restype = _i32
        getattr(L, pre + "_destroy").argtypes = [vp]
        getattr(L, pre + "_destroy").restype = None
    L.fv_wavpool_workspace_bytes.argtypes = [vp]
    L.fv_wavpool_workspace_bytes.restype = ctypes.c_size_t
    L.fv_wavpool_max_frames.argtypes = [vp]
    L.fv_wavpool_max_frames.restype = _i32
    L.fv_wavpool_plan.argtypes = [lcp, _i32, _i32, i64p, i64p, i32p, wip, _i32, i64p]
    L.fv_wavpool_plan.restype = _i32
    L.fv_wavpool_step.argtypes = [vp, wip, _i32, vp, i64, vp, _i32, i64p, vp, ctypes.c_size_t, vp]
    L.fv_wavpool_step.restype = _i32
    L.fv_global_resample_create.argtypes = [rcp, ctypes.POINTER(vp)]
    L.fv_global_resample_create.restype = _i32
    L.fv_respool_max_outputs.argtypes = [vp]
    L.fv_respool_max_outputs.restype = i64
    L.fv_respool_plan.argtypes = [rcp, _i32, _i32, i64p, i64p, i32p, wip, _i32, i64p]
    L.fv_respool_plan.restype = i64
    L.fv_respool_step.argtypes = [vp, wip, _i32, vp, i64, vp, i64, _i32, i64p, vp]
    L.fv_respool_step.restype = _i32
    pcp = ctypes.POINTER(PitchShiftConfig)
    L.fv_pitch_shift_plan.argtypes = [pcp, i32p, i32p, i32p]
    L.fv_pitch_shift_plan.restype = _i32
    L.fv_pitch_shift_lengths.argtypes = [pcp, i64, i64p, i64p, i64p, i64p]
    L.fv_pitch_shift_lengths.restype = _i32
    L.fv_pitch_shift_create.argtypes = [pcp, ctypes.POINTER(vp)]
    L.fv_pitch_shift_create.restype = _i32
    L.fv_pitch_shift_destroy.argtypes = [vp]
    L.fv_pitch_shift_destroy.restype = None
    L.fv_pitch_shift_workspace_bytes.argtypes = [vp, _i32, i64]
    L.fv_pitch_shift_workspace_bytes.restype = ctypes.c_size_t
    L.fv_pitch_shift_stretch.argtypes = [vp, vp, i64, vp, i64, _i32, i64, vp, ctypes.c_size_t, vp]
    L.fv_pitch_shift_stretch.restype = _i32
    L.fv_pitch_shift_forward.argtypes = [vp, vp, i64, vp, i64, _i32, i64, vp, ctypes.c_size_t, vp]
    L.fv_pitch_shift_forward.restype = _i32
    L.fv_pv_stream_ready.argtypes = [pcp, i64, i64p, i64p, i64p]
    L.fv_pv_stream_ready.restype = _i32
    L.fv_pv_set_batch_invariant.argtypes = [vp, _i32]
    L.fv_pv_set_batch_invariant.restype = _i32
    L.fv_pv_stream_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_pv_stream_create.restype = _i32
    L.fv_pv_stream_workspace_bytes.argtypes = [vp]
    L.fv_pv_stream_workspace_bytes.restype = ctypes.c_size_t
    L.fv_pv_stream_pending.argtypes = [vp]
    L.fv_pv_stream_pending.restype = i64
    L.fv_pv_stream_push.argtypes = [vp, vp, i64, _i32, vp, i64, i64p, vp, ctypes.c_size_t, vp]
    L.fv_pv_stream_push.restype = _i32
    L.fv_pv_stream_flush.argtypes = [vp, vp, i64, i64p, vp, ctypes.c_size_t, vp]
    L.fv_pv_stream_flush.restype = _i32
    L.fv_pv_stream_reset.argtypes = [vp]
    L.fv_pv_stream_reset.restype = _i32
    L.fv_pv_stream_destroy.argtypes = [vp]
    L.fv_pv_stream_destroy.restype = None
    L.fv_pvpool_workspace_bytes.argtypes = [vp]
    L.fv_pvpool_workspace_bytes.restype = ctypes.c_size_t
    L.fv_pvpool_max_outputs.argtypes = [vp]
    L.fv_pvpool_max_outputs.restype = i64
    L.fv_pvpool_bounds.argtypes = [pcp, _i32, i64p]
    L.fv_pvpool_bounds.restype = _i32
    L.fv_pvpool_plan.argtypes = [pcp, _i32, _i32, i64p, i64p, i32p, wip, _i32, i64p]
    L.fv_pvpool_plan.restype = i64
    L.fv_pvpool_step.argtypes = [vp, wip, _i32, vp, i64, vp, i64, _i32, i64p, vp, ctypes.c_size_t, vp]
    L.fv_pvpool_step.restype = _i32
    L.fv_spec_distance_tile.argtypes = []
    L.fv_spec_distance_tile.restype = _i32
    L.fv_spec_distance_workspace_bytes.argtypes = [_i32, i64]
    L.fv_spec_distance_workspace_bytes.restype = ctypes.c_size_t
    L.fv_spec_distance.argtypes = [vp, vp, i64, i64, _i32, i64, i32p, _i32, _i32, vp, vp, ctypes.c_size_t, vp]
    L.fv_spec_distance.restype = _i32
    fcp, tcp = ctypes.POINTER(F0Config), ctypes.POINTER(TemplateConfig)
    L.fv_f0_plan.argtypes = [fcp, i64, i32p, i32p, i32p, i64p]
    L.fv_f0_plan.restype = _i32
    L.fv_f0_create.argtypes = [fcp, ctypes.POINTER(vp)]
    L.fv_f0_create.restype = _i32
    L.fv_f0_destroy.argtypes = [vp]
    L.fv_f0_destroy.restype = None
    L.fv_f0_workspace_bytes.argtypes = [vp, _i32, i64]
    L.fv_f0_workspace_bytes.restype = ctypes.c_size_t
    L.fv_f0_forward.argtypes = [vp, vp, i64, i32p, vp, vp, i64, _i32, i64, vp, ctypes.c_size_t, vp]
    L.fv_f0_forward.restype = _i32
    L.fv_template_create.argtypes = [tcp, ctypes.POINTER(vp)]
    L.fv_template_create.restype = _i32
    L.fv_template_destroy.argtypes = [vp]
    L.fv_template_destroy.restype = None
    L.fv_template_workspace_bytes.argtypes = [vp, _i32, i64]
    L.fv_template_workspace_bytes.restype = ctypes.c_size_t
    L.fv_template_forward.argtypes = [vp, vp, i64, i32p, vp, i64, _i32, i64, vp, ctypes.c_size_t, vp]
    L.fv_template_forward.restype = _i32
    L.fv_yin_frames_ready.argtypes = [fcp, i64]
    L.fv_yin_frames_ready.restype = i64
    L.fv_yin_stream_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_yin_stream_create.restype = _i32
    L.fv_yin_stream_pending_samples.argtypes = [vp]
    L.fv_yin_stream_pending_samples.restype = i64
    L.fv_yin_stream_push.argtypes = [vp, vp, i64, _i32, vp, vp, i64, i64p, vp]
    L.fv_yin_stream_push.restype = _i32
    L.fv_yin_stream_flush.argtypes = [vp, vp, vp, i64, i64p, vp]
    L.fv_yin_stream_flush.restype = _i32
    L.fv_yin_stream_reset.argtypes = [vp]
    L.fv_yin_stream_reset.restype = _i32
    L.fv_yin_stream_destroy.argtypes = [vp]
    L.fv_yin_stream_destroy.restype = None
    L.fv_osc_stream_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_osc_stream_create.restype = _i32
    L.fv_osc_stream_pending_frames.argtypes = [vp]
    L.fv_osc_stream_pending_frames.restype = i64
    L.fv_osc_stream_push.argtypes = [vp, vp, i64, _i32, vp, i64, i64p, vp]
    L.fv_osc_stream_push.restype = _i32
    L.fv_osc_stream_flush.argtypes = [vp, vp, i64, i64p, vp]
    L.fv_osc_stream_flush.restype = _i32
    L.fv_osc_stream_reset.argtypes = [vp]
    L.fv_osc_stream_reset.restype = _i32
    L.fv_osc_stream_destroy.argtypes = [vp]
    L.fv_osc_stream_destroy.restype = None
    for pre, cfgp in (("fv_yinpool", fcp), ("fv_oscpool", tcp)):
        getattr(L, pre + "_max_frames").argtypes = [vp]
        getattr(L, pre + "_max_frames").restype = i64
        getattr(L, pre + "_plan").argtypes = [cfgp, _i32, _i32, i64p, i64p, i32p, wip, _i32, i64p]
        getattr(L, pre + "_plan").restype = i64
    L.fv_yinpool_step.argtypes = [vp, wip, _i32, vp, i64, vp, vp, i64, _i32, i64p, vp]
    L.fv_yinpool_step.restype = _i32
    L.fv_oscpool_step.argtypes = [vp, wip, _i32, vp, i64, vp, i64, _i32, i64p, vp]
    L.fv_oscpool_step.restype = _i32
    L.fv_pair_wino4_tile.argtypes = [_i32, _i32]
    L.fv_pair_wino4_tile.restype = _i32
    L.fv_pair_wino4_pack.argtypes = [fp, _i32, fp, i64]
    L.fv_pair_wino4_pack.restype = i64
    L.fv_vq_create.argtypes = [ctypes.POINTER(VQConfig), ctypes.POINTER(vp)]
    L.fv_vq_create.restype = _i32
    L.fv_vq_destroy.argtypes = [vp]
    L.fv_vq_destroy.restype = None
    L.fv_vq_load_codebook.argtypes = [vp, _i32, fp]
    L.fv_vq_load_codebook.restype = _i32
    L.fv_vq_set_slices.argtypes = [vp, _i32]
    L.fv_vq_set_slices.restype = _i32
    L.fv_vq_workspace_bytes.argtypes = [vp, _i32, i64]
    L.fv_vq_workspace_bytes.restype = ctypes.c_size_t
    L.fv_vq_encode.argtypes = [vp, vp, i64, i32p, vp, vp, _i32, i64, vp, ctypes.c_size_t, vp]
    L.fv_vq_encode.restype = _i32
    L.fv_vq_decode.argtypes = [vp, vp, i32p, vp, _i32, i64, vp]
    L.fv_vq_decode.restype = _i32
    L.fv_stream_create_codes.argtypes = [vp, vp, ctypes.POINTER(StreamConfig), ctypes.POINTER(vp)]
    L.fv_stream_create_codes.restype = _i32
    L.fv_stream_push_codes.argtypes = [vp, vp, vp, _i32, vp, i64p, vp, ctypes.c_size_t, vp]
    L.fv_stream_push_codes.restype = _i32
    L.fv_codepool_create.argtypes = [vp, vp, ctypes.POINTER(PoolConfig), ctypes.POINTER(vp)]
    L.fv_codepool_create.restype = _i32
    L.fv_codepool_step.argtypes = [vp, pip, _i32, vp, vp, _i32, vp, _i32, i64p, vp, ctypes.c_size_t, vp]
    L.fv_codepool_step.restype = _i32
    L.fv_stream_ring_bytes.argtypes = [vp]
    L.fv_stream_ring_bytes.restype = ctypes.c_size_t
    L.fv_codepool_ring_bytes.argtypes = [vp]
    L.fv_codepool_ring_bytes.restype = ctypes.c_size_t
    L.fv_posterior_create.argtypes = [ctypes.POINTER(PosteriorConfig), ctypes.POINTER(vp)]
    L.fv_posterior_create.restype = _i32
    L.fv_posterior_load_weight.argtypes = [vp, cp, fp, i64p, _i32]
    L.fv_posterior_load_weight.restype = _i32
    L.fv_posterior_finalize.argtypes = [vp]
    L.fv_posterior_finalize.restype = _i32
    L.fv_posterior_reach_frames.argtypes = [vp]
    L.fv_posterior_reach_frames.restype = _i32
    L.fv_posterior_output_channels.argtypes = [vp]
    L.fv_posterior_output_channels.restype = _i32
    L.fv_posterior_workspace_bytes.argtypes = [vp, _i32, i64]
    L.fv_posterior_workspace_bytes.restype = ctypes.c_size_t
    L.fv_posterior_forward.argtypes = [vp, vp, i64, i32p, vp, vp, vp, _i32, i64, vp, ctypes.c_size_t, vp]
    L.fv_posterior_forward.restype = _i32
    L.fv_posterior_destroy.argtypes = [vp]
    L.fv_posterior_destroy.restype = None
    L.fv_wnstream_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_wnstream_create.restype = _i32
    L.fv_wnstream_push.argtypes = [vp, vp, i64, i64, _i32, vp, vp, vp, i64, i64p, vp]
    L.fv_wnstream_push.restype = _i32
    L.fv_wnstream_flush.argtypes = [vp, vp, vp, vp, i64, i64p, vp]
    L.fv_wnstream_flush.restype = _i32
    L.fv_wnstream_reset.argtypes = [vp]
    L.fv_wnstream_reset.restype = _i32
    L.fv_wnstream_pending.argtypes = [vp]
    L.fv_wnstream_pending.restype = i64
    L.fv_wnstream_lookahead.argtypes = [vp]
    L.fv_wnstream_lookahead.restype = _i32
    L.fv_wnstream_destroy.argtypes = [vp]
    L.fv_wnstream_destroy.restype = None
    L.fv_cnxstream_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_cnxstream_create.restype = _i32
    L.fv_cnxstream_push.argtypes = [vp, vp, i64, i64, _i32, vp, i64, i64p, vp]
    L.fv_cnxstream_push.restype = _i32
    L.fv_cnxstream_flush.argtypes = [vp, vp, i64, i64p, vp]
    L.fv_cnxstream_flush.restype = _i32
    L.fv_cnxstream_reset.argtypes = [vp]
    L.fv_cnxstream_reset.restype = _i32
    L.fv_cnxstream_pending.argtypes = [vp]
    L.fv_cnxstream_pending.restype = i64
    L.fv_cnxstream_lookahead.argtypes = [vp]
    L.fv_cnxstream_lookahead.restype = _i32
    L.fv_cnxstream_state_bytes.argtypes = [vp]
    L.fv_cnxstream_state_bytes.restype = i64
    L.fv_cnxstream_destroy.argtypes = [vp]
    L.fv_cnxstream_destroy.restype = None
    L.fv_cnxstream_plan.argtypes = [i64, i64, _i32, _i32, _i32, _i32, i64p]
    L.fv_cnxstream_plan.restype = _i32
    L.fv_cnxpool_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_cnxpool_create.restype = _i32
    L.fv_cnxpool_plan.argtypes = [_i32, _i32, _i32, i64p, i64p, i32p, wip, _i32, i64p]
    L.fv_cnxpool_plan.restype = i64
    L.fv_cnxpool_step.argtypes = [vp, wip, _i32, vp, i64, i64, vp, _i32, i64p, vp]
    L.fv_cnxpool_step.restype = _i32
    L.fv_cnxpool_reset.argtypes = [vp, _i32]
    L.fv_cnxpool_reset.restype = _i32
    for name in ("received", "emitted", "pending"):
        getattr(L, "fv_cnxpool_" + name).argtypes = [vp, _i32]
        getattr(L, "fv_cnxpool_" + name).restype = i64
    L.fv_cnxpool_lookahead.argtypes = [vp]
    L.fv_cnxpool_lookahead.restype = _i32
    L.fv_cnxpool_max_frames.argtypes = [vp]
    L.fv_cnxpool_max_frames.restype = i64
    L.fv_cnxpool_launches.argtypes = [vp]
    L.fv_cnxpool_launches.restype = _i32
    L.fv_cnxpool_state_bytes.argtypes = [vp]
    L.fv_cnxpool_state_bytes.restype = i64
    L.fv_cnxpool_table_size.argtypes = []
    L.fv_cnxpool_table_size.restype = _i32
    L.fv_cnxpool_destroy.argtypes = [vp]
    L.fv_cnxpool_destroy.restype = None
    L.fv_wnpool_create.argtypes = [vp, _i32, _i32, ctypes.POINTER(vp)]
    L.fv_wnpool_create.restype = _i32
    L.fv_wnpool_plan.argtypes = [_i32, _i32, _i32, i64p, i64p, i32p, wip, _i32, i64p]
    L.fv_wnpool_plan.restype = i64
    L.fv_wnpool_step.argtypes = [vp, wip, _i32, vp, i64, i64, vp, vp, vp, _i32, i64p, vp]
    L.fv_wnpool_step.restype = _i32
    L.fv_wnpool_reset.argtypes = [vp, _i32]
    L.fv_wnpool_reset.restype = _i32
    for name in ("received", "emitted", "pending"):
        getattr(L, "fv_wnpool_" + name).argtypes = [vp, _i32]
        getattr(L, "fv_wnpool_" + name).restype = i64
    L.fv_wnpool_lookahead.argtypes = [vp]
    L.fv_wnpool_lookahead.restype = _i32
    L.fv_wnpool_max_frames.argtypes = [vp]
    L.fv_wnpool_max_frames.restype = i64
    L.fv_wnpool_launches.argtypes = [vp]
    L.fv_wnpool_launches.restype = _i32
    L.fv_wnpool_destroy.argtypes = [vp]
    L.fv_wnpool_destroy.restype = None
    L.fv_w2v_create.argtypes = [ctypes.POINTER(W2VConfig), ctypes.POINTER(vp)]
    L.fv_w2v_create.restype = _i32
    L.fv_w2v_load_weight.argtypes = [vp, cp, fp, i64p, _i32]
    L.fv_w2v_load_weight.restype = _i32
    L.fv_w2v_finalize.argtypes = [vp]
    L.fv_w2v_finalize.restype = _i32
    L.fv_w2v_frames.argtypes = [vp, i64, _i32]
    L.fv_w2v_frames.restype = i64
    L.fv_w2v_workspace_bytes.argtypes = [vp, _i32, i64]
    L.fv_w2v_workspace_bytes.restype = ctypes.c_size_t
    L.fv_w2v_forward.argtypes = [vp, vp, i64, i32p, _i32, vp, vp, vp, ctypes.c_size_t, vp]
    L.fv_w2v_forward.restype = _i32
    L.fv_w2v_destroy.argtypes = [vp]
    L.fv_w2v_destroy.restype = None
    L.fv_disc_create.argtypes = [ctypes.POINTER(DiscConfig), ctypes.POINTER(vp)]
    L.fv_disc_create.restype = _i32
    L.fv_disc_load_weight.argtypes = [vp, cp, fp, i64p, _i32]
    L.fv_disc_load_weight.restype = _i32
    L.fv_disc_finalize.argtypes = [vp]
    L.fv_disc_finalize.restype = _i32
    L.fv_disc_destroy.argtypes = [vp]
    L.fv_disc_destroy.restype = None
    L.fv_disc_layout.argtypes = [vp, _i32, i64, ctypes.POINTER(DiscMap), _i32, i32p]
    L.fv_disc_layout.restype = i64
    L.fv_disc_workspace_bytes.argtypes = [vp, _i32, i64]
    L.fv_disc_workspace_bytes.restype = ctypes.c_size_t
    L.fv_disc_forward.argtypes = [vp, vp, i64, i32p, _i32, vp, i64, vp, ctypes.c_size_t, vp]
    L.fv_disc_forward.restype = _i32
    L.fv_disc_distance.argtypes = [vp, vp, vp, i64, i32p, _i32, vp, vp, ctypes.c_size_t, vp]
    L.fv_disc_distance.restype = _i32
    L.fv_mms_normalize_workspace_bytes.argtypes = [_i32, i64]
    L.fv_mms_normalize_workspace_bytes.restype = ctypes.c_size_t
    L.fv_mms_normalize.argtypes = [vp, i64, i32p, _i32, vp, vp, ctypes.c_size_t, vp]
    L.fv_mms_normalize.restype = _i32
    L.fv_mms_interpolate.argtypes = [vp, i64, _i32, i32p, i32p, _i32, vp, i64, vp]
    L.fv_mms_interpolate.restype = _i32
    L.fv_mms_nearest_index.argtypes = [i64, i64, i64]
    L.fv_mms_nearest_index.restype = i64
    L.fv_last_error.restype = cp
    L.fv_abi_version.restype = _i32
    L.fv_last_kernel.restype = cp
    if L.fv_abi_version() != FV_ABI_VERSION:
        raise ImportError(f"libfishvoc_hip.so ABI {L.fv_abi_version()} != binding {FV_ABI_VERSION}; rebuild")
    _lib = L
    return L


class FishVocError(RuntimeError):
    """An fv_* call returned a non-zero status; carries fv_last_error()."""

    def __init__(self, status: int, message: str):
        super().__init__(f"libfishvoc_hip: {message} (status {status})")
        self.status = status


def check(status: int) -> None:
    if status != 0:
        raise FishVocError(status, lib().fv_last_error().decode("utf-8", "replace"))


def reload_env() -> None:
    """Re-read the experiment knobs (FV_PW ...) that the library caches at first use (fv_reload_env)."""
    lib().fv_reload_env()


def resample_input_tile() -> int:
    """Input samples of the resampler kernel's tile (fv_resample_input_tile): the tests size their rows from it."""
    return int(lib().fv_resample_input_tile())


def spec_distance_tile() -> int:
    """Columns per tile of the scoring reduction (fv_spec_distance_tile): the tests size their rows from it."""
    return int(lib().fv_spec_distance_tile())


def last_kernel() -> str:
    return lib().fv_last_kernel().decode()
