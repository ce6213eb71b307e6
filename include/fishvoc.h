/*
 * fishvoc.h — C ABI of libfishvoc_hip.so, the MI355X (gfx950) vocoder inference engine.
 *
 * The reference (fishaudio/vocoder, /root/reference) has NO FFI: its generator hot path is
 * `nn.Module.forward` built by Hydra `_target_` (fish_vocoder/test.py:31,89 ->
 * fish_vocoder/models/gan.py:282-288 -> fish_vocoder/modules/generators/).  This header is
 * therefore the boundary a maintainer would bind from Python (ctypes) to replace that forward:
 * each entry point names the reference interface it stands in for.  INTEGRATION.md shows the
 * reference-side stub.
 *
 * Conventions
 *   - plain C types only; tensors are contiguous fp32, layout (B, C, T) with T fastest — the
 *     reference's own layout (hifigan.py:226, forward(x: (B, num_mels, T_mel))).
 *   - `const float* host_*` pointers are HOST memory and are copied during the call (the caller keeps
 *     ownership); `d_*` pointers are DEVICE memory borrowed for the duration of the asynchronous
 *     work enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *   - every function returns FV_OK (0) or a negative fv_status; fv_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI.
 *   - one engine per device/model; fv_forward on one engine is re-entrant only with distinct
 *     workspaces and streams.
 */
#ifndef FISHVOC_H
#define FISHVOC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FV_ABI_VERSION 5

/* every entry point below is exported with default visibility (the library is built -fvisibility=hidden) */
#if defined(__GNUC__)
#define FV_API __attribute__((visibility("default")))
#else
#define FV_API
#endif

typedef int fv_status;
enum {
    FV_OK = 0,
    FV_ERR_INVALID = -1,      /* bad argument / config (e.g. prod(upsample_rates) != hop_length) */
    FV_ERR_UNSUPPORTED = -2,  /* valid in the reference but out of scope here (use_template=True) */
    FV_ERR_MISSING_WEIGHT = -3,
    FV_ERR_SHAPE = -4,
    FV_ERR_HIP = -5,          /* a HIP runtime call failed */
    FV_ERR_STATE = -6         /* e.g. fv_forward before fv_finalize */
};

/* Model families == the reference generator classes reachable from configs/model/generator/ YAMLs */
typedef enum fv_model_kind {
    FV_MODEL_HIFIGAN = 1,  /* fish_vocoder.modules.generators.hifigan.HiFiGANGenerator (hifigan.py:136) */
    FV_MODEL_BIGVGAN = 2,  /* fish_vocoder.modules.generators.bigvgan.BigVGANGenerator (bigvgan.py:255) */
    FV_MODEL_VOCOS = 3,    /* UnifyGenerator(ConvNeXtEncoder, ISTFTHead) (unify.py:5, convnext.py:146, vocos.py:6) */
    FV_MODEL_FIREFLY = 4,  /* UnifyGenerator(ConvNeXtEncoder, HiFiGANGenerator) (firefly-gan-base.yaml) */
    FV_MODEL_CONVNEXT = 5, /* ConvNeXtEncoder alone: (B, C_in, T) -> (B, dims[-1], T) */
    FV_MODEL_ISTFT_HEAD = 6, /* ISTFTHead alone: (B, dim, T) -> (B, 1, T*hop) (vocos.py:43-69) */
    FV_MODEL_LOGMEL = 7,     /* LogMelSpectrogram: (B, 1, L) wave -> (B, n_mels, frames) (data/transforms/spectrogram.py:59-104);
                                the step right before the generator in test.py:71 */
    FV_MODEL_REFINEGAN = 8   /* fish_vocoder.modules.generators.refinegan.RefineGANGenerator (refinegan.py:182): forward(mel, template)
                                with AdaIN noise supplied by the caller (fv_forward_refinegan) or seeded and computed in the AdaIN kernels
                                (fv_refinegan_set_noise_seed, fv_forward_refinegan_seeded) */
} fv_model_kind;

#define FV_MAX_STAGES 8
#define FV_MAX_KERNELS 8
#define FV_MAX_DILATIONS 3 /* ResBlock1 / AMPBlock hard-code three (c1, c2) pairs (hifigan.py:29-93) */

/* Activation selector for the fused conv kernels (the reference "HiFiGAN" uses SiLU). */
typedef enum fv_act {
    FV_ACT_NONE = 0,
    FV_ACT_SILU = 1,       /* F.silu (hifigan.py:103,105,230) */
    FV_ACT_LEAKY_RELU = 2, /* slope in fv_conv_desc.act_slope (refinegan.py:89; kept for completeness) */
    FV_ACT_GELU = 3,       /* nn.GELU() exact erf (convnext.py:114) */
    FV_ACT_TANH = 4,       /* torch.tanh (hifigan.py:247) */
    FV_ACT_LOG_CLAMP = 5   /* log(clamp(x, min=1e-5)) (spectrogram.py:93-94) */
} fv_act;

/* Arithmetic of the MFMA-bound conv layers.  The reference computes in fp32; FV_PRECISION_F32 reproduces that
 * with fp32 matrix instructions (direct sums, or Winograd F(2,3) tap groups for the dilated ResBlock convs of launches that fill the
 * chip: fp32 products and sums throughout, as close to a float64 forward as the direct sums) and is the default.  FV_PRECISION_F16X3 is opt-in: each fp32 operand is split in two
 * fp16 planes and three fp16 products accumulate in fp32 (error ~2^-22 per product instead of 2^-24; activations must
 * stay below 65504 in magnitude) — same API, same parity tolerance, several times the throughput. */
typedef enum fv_precision {
    FV_PRECISION_F32 = 0,
    FV_PRECISION_F16X3 = 1
} fv_precision;

/* fv_upsampler_config.post_activation values beside the fv_act ones (ABI 5) */
#define FV_POST_ACT_DEFAULT 0     /* the reference default: nn.SiLU (hifigan.py:150) */
#define FV_POST_ACT_IDENTITY (-1) /* nn.Identity */

/* HiFiGANGenerator / BigVGANGenerator ctor kwargs (hifigan.py:137-151, bigvgan.py:256-270). */
typedef struct fv_upsampler_config {
    int32_t hop_length;
    int32_t num_upsamples;
    int32_t upsample_rates[FV_MAX_STAGES];
    int32_t upsample_kernel_sizes[FV_MAX_STAGES];
    int32_t num_kernels;
    int32_t resblock_kernel_sizes[FV_MAX_KERNELS];
    int32_t resblock_dilation_sizes[FV_MAX_KERNELS][FV_MAX_DILATIONS];
    int32_t num_mels;
    int32_t upsample_initial_channel;
    int32_t use_template; /* 1: pitch-template noise_convs branch (the ctor default; every shipped YAML sets false) */
    int32_t pre_conv_kernel_size;
    int32_t post_conv_kernel_size;
    /* `post_activation()` in front of conv_post (hifigan.py:150,213,245 — any nn.Module factory upstream; HiFiGAN only, BigVGAN has its own
     * activation_post).  ABI 5: **0 = FV_POST_ACT_DEFAULT = the reference default, SiLU** (partial(nn.SiLU, inplace=True)), so that a
     * zero-initialised struct builds the reference's generator; FV_ACT_SILU says the same explicitly, FV_ACT_LEAKY_RELU with
     * post_activation_slope covers nn.LeakyReLU(slope) of classic HiFi-GAN checkpoints and nn.ReLU (slope 0), FV_ACT_GELU / FV_ACT_TANH
     * their exact forms, and nn.Identity is FV_POST_ACT_IDENTITY (-1; NOT FV_ACT_NONE, whose value 0 is the default here).
     * Anything else -> FV_ERR_UNSUPPORTED. */
    int32_t post_activation;
    float post_activation_slope;
} fv_upsampler_config;

/* ConvNeXtEncoder ctor kwargs (convnext.py:147-155); drop_path is identity in eval and not represented. */
typedef struct fv_convnext_config {
    int32_t input_channels;
    int32_t num_stages;
    int32_t depths[FV_MAX_STAGES];
    int32_t dims[FV_MAX_STAGES];
    int32_t kernel_size;
} fv_convnext_config;

/* ISTFTHead ctor kwargs (vocos.py:19-26).  padding: FV_ISTFT_SAME ("same", every shipped vocos YAML: output length T * hop) or
 * FV_ISTFT_CENTER ("center": vocos 0.0.2 falls back to torch.istft(center=True) — frames overlap-added at t * hop, n_fft / 2 samples
 * trimmed from both ends, output length (T - 1) * hop; torch raises when the window envelope has a zero there, here FV_ERR_INVALID
 * at fv_finalize). */
enum { FV_ISTFT_SAME = 0, FV_ISTFT_CENTER = 1 };
typedef struct fv_istft_head_config {
    int32_t dim;
    int32_t n_fft;
    int32_t hop_length;
    int32_t win_length;
    int32_t padding;
} fv_istft_head_config;

/* LogMelSpectrogram ctor kwargs (spectrogram.py:60-70); center must be 0 (the reference default), win_length == n_fft,
 * hop_length <= n_fft (hop need not divide n_fft: resolution/24000_2048_3072.yaml).  n_mels == 0 selects LinearSpectrogram
 * alone (spectrogram.py:25-56, mode "pow2_sqrt"): the output is the (B, n_fft/2+1, frames) magnitude, no filterbank, no log. */
typedef struct fv_logmel_config {
    int32_t sample_rate;
    int32_t n_fft;
    int32_t win_length;
    int32_t hop_length;
    int32_t n_mels;
    float f_min;
    float f_max; /* <= 0: sample_rate // 2 */
} fv_logmel_config;

/* RefineGANGenerator ctor kwargs (refinegan.py:183-193); prod(downsample_rates) == prod(upsample_rates) == hop_length. */
typedef struct fv_refinegan_config {
    int32_t hop_length;
    int32_t num_stages; /* len(downsample_rates) == len(upsample_rates) */
    int32_t downsample_rates[FV_MAX_STAGES];
    int32_t upsample_rates[FV_MAX_STAGES];
    int32_t num_mels;
    int32_t start_channels;
    float leaky_relu_slope;
} fv_refinegan_config;

typedef struct fv_config {
    int32_t abi_version; /* = FV_ABI_VERSION */
    int32_t model;       /* fv_model_kind */
    fv_upsampler_config ups;   /* HIFIGAN, BIGVGAN, FIREFLY(head) */
    fv_convnext_config backbone; /* VOCOS, FIREFLY, CONVNEXT */
    fv_istft_head_config head;   /* VOCOS */
    fv_logmel_config mel;        /* LOGMEL */
    fv_refinegan_config refine;  /* REFINEGAN */
} fv_config;

typedef struct fv_engine fv_engine;

/* -------- engine lifecycle: replaces `instantiate(cfg.model)` + `load_state_dict` (test.py:31-38) -------- */

/* Validates the config exactly as the reference ctor does (assert prod(upsample_rates) == hop_length,
 * hifigan.py:154-156 -> FV_ERR_INVALID) and allocates an engine on the current HIP device. */
FV_API fv_status fv_create(const fv_config* cfg, fv_engine** out);

/* Feed one tensor of the reference state dict, by its reference name (keys as produced by the reference
 * modules, e.g. "conv_pre.parametrizations.weight.original0", "ups.0.bias",
 * "resblocks.1.blocks.2.convs2.0.parametrizations.weight.original1"; legacy "weight_g"/"weight_v" and plain
 * "weight" are accepted too).  Unknown names -> FV_ERR_INVALID; wrong shape -> FV_ERR_SHAPE.  Data is copied. */
FV_API fv_status fv_load_weight(fv_engine* e, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);

/* Fold weight-norm (w = g * v / ||v||, dim 0 — hifigan.py:31; C_in for ConvTranspose1d), re-lay-out weights
 * into MFMA fragment order and upload.  FV_ERR_MISSING_WEIGHT names the first absent tensor (strict load,
 * like test.py:37). */
FV_API fv_status fv_finalize(fv_engine* e);

FV_API void fv_destroy(fv_engine* e);

/* Selects the arithmetic of the conv layers (fv_precision).  Call between fv_create and fv_finalize (the weight planes
 * are packed at finalize; later -> FV_ERR_STATE).  No reference counterpart: torch runs this path in fp32 only. */
FV_API fv_status fv_set_precision(fv_engine* e, int32_t precision);

/* How the fp32 conv layers form their sums (FV_PRECISION_F32 only; no reference counterpart: torch picks its own convolution algorithm per
 * call).  Every choice computes in fp32 and stays well inside the parity bar (whole forwards differ by <= 2e-5 of full scale between them);
 * what changes is the LAST BITS of a clip's output and the speed:
 *   FV_CONV_ALGO_AUTO      per launch, whatever is fastest.  The dilated k = 3 / 7 / 11 ResBlock / AMPBlock convs: launches that fill the chip (>= one
 *                          workgroup per CU: depends on batch size, clip length and the device's CU count) run the throughput Winograd kernels — F(4,4) tap
 *                          groups on the quad lattice for k = 7 / 11 on layers of whole 64-row tiles, F(2,3) on the pair lattice otherwise; launches below
 *                          that gate (single clips, small batches) run the Winograd LATENCY kernels (F(4,4) for k = 7 / 11, F(2,3) for k = 3; K split over the waves), direct split-K sums
 *                          where it has no instance; the fused (c1, c2) pairs of the narrow stages use Winograd whenever a kernel exists.  Default.
 *   FV_CONV_ALGO_DIRECT    direct sums everywhere.
 *   FV_CONV_ALGO_WINOGRAD  the throughput Winograd kernels wherever one exists, whatever the launch size (never the latency kernel: single clips are
 *                          slower than under AUTO).
 * fv_set_batch_invariant(e, 1) additionally makes every choice BETWEEN DIFFERENT SUMS a function of the layer shape alone (C, k, dilation) — never of the
 * batch size or the clip length: no split-K / latency kernels, the fused pairs and the pointwise GEMM wherever their
 * shape allows, and (under FV_CONV_ALGO_AUTO) Winograd wherever a kernel exists.  A clip's output is then bit-identical whichever other clips
 * share its batch — e.g. a 37-clip batch sharded 5/5/5/5/5/4/4/4 over 8 GPUs equals the single-GPU batch bit for bit (tests pin HiFiGAN, BigVGAN,
 * Vocos, Firefly and RefineGAN; a pointwise-GEMM launch past the 32-bit offset span — > 4 GiB per layer: the default engine moves it to the k = 1 conv
 * kernel, which forms other sums — is refused with FV_ERR_UNSUPPORTED in this mode: split the batch) — at the price of
 * single-clip latency (the launch-size gates exist because small launches are faster on the direct / split-K kernels).  Without it, batches
 * that differ in size may differ in the last bits (<= 2e-5 of full scale; tests/test_gpu_models.py pins the bound).
 * Both may be called at any time; captured graphs are dropped. */
typedef enum fv_conv_algo {
    FV_CONV_ALGO_AUTO = 0,
    FV_CONV_ALGO_DIRECT = 1,
    FV_CONV_ALGO_WINOGRAD = 2
} fv_conv_algo;
FV_API fv_status fv_set_conv_algorithm(fv_engine* e, int32_t algo);
FV_API fv_status fv_set_batch_invariant(fv_engine* e, int32_t enable);

/* hipGraph replay of the static launch sequence (on by default; a call with the same buffers / shape / stream as an
 * earlier one replays a captured graph; calls on the null stream are captured on a stream the engine owns and replayed on the null stream).
 * enable = 0 makes every fv_forward* enqueue its kernels eagerly — what a server
 * that never sees the same (buffers, batch, frames) twice gets.  May be called at any time.  No reference counterpart. */
FV_API fv_status fv_set_graph_replay(fv_engine* e, int32_t enable);
/* 1 while repeated calls are replayed, 0 when every call is enqueued eagerly — by fv_set_graph_replay(e, 0), by FV_NO_GRAPH=1 /
 * FV_DEBUG_STOP in the environment at fv_create, or because stream capture failed once in this context.  A binding that routes
 * eager null-stream calls through a side stream of its own (vocoder_amd/engine.py) asks this instead of mirroring the flag. */
FV_API int32_t fv_get_graph_replay(const fv_engine* e);

/* Kernel-selection knobs for experiments (FV_PW, FV_PW_PX, FV_DWLN_NG8, FV_DWLN_RR, FV_OLD_DWLN; FV_WINO = 0 / 1 / 2 — the process-wide default
 * of fv_set_conv_algorithm: direct / auto / Winograd —, FV_WINO_MIN_M, FV_WINO_CFG, FV_WINO_MIN_BLOCKS, FV_PAIR_WINO: these change which sums are
 * formed, i.e. the last bits of the output) are read from the environment
 * ONCE per process (no getenv on the launch path); a harness that changes them afterwards calls this to re-read them.
 * Not for production use; not thread-safe against concurrent forwards.  No reference counterpart. */
FV_API void fv_reload_env(void);

/* -------- forward: replaces `self.generator(input_spec)` (gan.py:286) -------- */

/* Output length per clip for T_in input frames (T_mel * hop_length for the generators). */
FV_API int64_t fv_output_length(const fv_engine* e, int32_t t_in);
/* Output channels (1 for the generators, dims[-1] for FV_MODEL_CONVNEXT). */
FV_API int32_t fv_output_channels(const fv_engine* e);
/* Input channels (num_mels / input_channels). */
FV_API int32_t fv_input_channels(const fv_engine* e);

/* Bytes of device scratch fv_forward needs for a (batch, t_in) call. */
FV_API size_t fv_workspace_bytes(const fv_engine* e, int32_t batch, int32_t t_in);

/* d_in: (batch, C_in, t_in) fp32; d_out: (batch, C_out, fv_output_length) fp32; d_workspace: >= fv_workspace_bytes,
 * 256-byte aligned.  Asynchronous on `stream`. */
FV_API fv_status fv_forward(fv_engine* e, const float* d_in, float* d_out, int32_t batch, int32_t t_in, void* d_workspace,
                     size_t workspace_bytes, void* stream);

/* Same, for generators built with use_template=1: d_template is the pitch template (batch, 1, fv_output_length) that the
 * reference adds through strided `noise_convs` after every up-sampling stage (hifigan.py:192-204,233-234;
 * forward(x, template), hifigan.py:226).  fv_forward == fv_forward_template with d_template = NULL. */
FV_API fv_status fv_forward_template(fv_engine* e, const float* d_in, const float* d_template, float* d_out, int32_t batch,
                                     int32_t t_in, void* d_workspace, size_t workspace_bytes, void* stream);

/* RefineGANGenerator.forward(mel, template) (refinegan.py:287-323).  d_mel: (batch, num_mels, t_in); d_template: (batch, 1,
 * t_in * hop_length); d_out likewise.  The reference's AdaIN layers draw torch.randn_like on every call (refinegan.py:125);
 * here the caller supplies those standard-normal samples in d_noise — fv_refinegan_noise_elems floats, laid out as the
 * concatenation, in order of use (up-sampling stage, branch k = 3 / 7 / 11, first / second AdaIN), of (batch, C_stage, T_stage)
 * tensors — so that a run is reproducible and parity with the reference can be pinned. */
FV_API int64_t fv_refinegan_noise_elems(const fv_engine* e, int32_t batch, int32_t t_in);
FV_API fv_status fv_forward_refinegan(fv_engine* e, const float* d_mel, const float* d_template, const float* d_noise,
                                      float* d_out, int32_t batch, int32_t t_in, void* d_workspace, size_t workspace_bytes,
                                      void* stream);

/* Seeded AdaIN noise.  With a seed set, the standard-normal sample that stands in for torch.randn_like (refinegan.py:125) is computed inside
 * the AdaIN kernel as a pure function of (seed s, noise row r, AdaIN layer l, channel c of C, absolute position p >= 0 at that layer's rate):
 *   q = p >> 2, lane = p & 3;
 *   (x0, x1, x2, x3) = Philox4x32-10(counter = (q & 0xffffffff, q >> 32, r * C + c, l), key = (s & 0xffffffff, s >> 32))  (Random123:
 *   multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds);
 *   Box-Muller per pair: u1 = ((xa >> 8) + 1) 2^-24 in (0, 1], u2 = (xb >> 8) 2^-24 in [0, 1), rad = sqrt(-2 ln u1); lanes 0 / 1 are
 *   rad cos(2 pi u2) / rad sin(2 pi u2) of (x0, x1), lanes 2 / 3 the same of (x2, x3)  (logf, sqrtf, sincospif(2 u2)).
 * l counts the AdaIN layers in the order of fv_forward_refinegan's d_noise (stage, branch k = 3 / 7 / 11, first / second AdaIN); p is counted
 * from the utterance's first sample; r = first_row + b for batch row b, so that a shard, or a clip run alone, reproduces row b of the global
 * batch.  No noise tensor exists, and a window of an utterance regenerates exactly the samples the whole utterance has at those positions: a
 * seeded engine has a finite reach (fv_reach_frames), runs clips of any length as time tiles and streams (fv_stream_*: a stream's pushes run
 * eagerly — the window's origin is a kernel scalar, which a captured graph would bake in; a push after the engine's seed was cleared or changed
 * is refused with FV_ERR_STATE before anything moves).  fv_ragged_* and fv_pool_* stay refused for RefineGAN: their rows start at per-row
 * origins, which the per-launch (origin, stride) does not express.  vocoder_amd/refinegan_noise.py restates the rule in numpy.
 *
 * fv_refinegan_set_noise_seed puts the engine in seeded mode (refinegan.py:125's draw becomes reproducible), fv_refinegan_clear_noise_seed
 * takes it out (refinegan.py:125 needs the caller's d_noise again); both drop the engine's captured graphs.  first_row >= 0. */
FV_API fv_status fv_refinegan_set_noise_seed(fv_engine* e, uint64_t seed, int32_t first_row);
FV_API fv_status fv_refinegan_clear_noise_seed(fv_engine* e);
/* fv_forward_refinegan with refinegan.py:125's draws computed in the kernels: the input is the frames [origin_frame, origin_frame + t_in) of
 * its utterance (0 for a whole clip).  FV_ERR_STATE on an engine without a seed.  Clips past the addressing span run as time tiles, each tile
 * with its clip's noise row at its own origin; at most 65535 clips x tiles per call.  fv_forward_refinegan with explicit d_noise keeps working
 * on a seeded engine for lengths that run whole; at a tiled length it is refused with FV_ERR_UNSUPPORTED (the explicit layout has no tiled
 * form). */
FV_API fv_status fv_forward_refinegan_seeded(fv_engine* e, const float* d_mel, const float* d_template, float* d_out, int32_t batch,
                                             int32_t t_in, int64_t origin_frame, void* d_workspace, size_t workspace_bytes, void* stream);
/* The draws of refinegan.py:125 that fv_forward_refinegan_seeded(batch, t_in, origin_frame) computes in its kernels, written in
 * fv_forward_refinegan's d_noise layout (fv_refinegan_noise_elems floats): the two paths then agree bit for bit.  Needs a seed
 * (FV_ERR_STATE). */
FV_API fv_status fv_refinegan_fill_noise(fv_engine* e, float* d_noise, int32_t batch, int32_t t_in, int64_t origin_frame, void* stream);

/* -------- streaming synthesis: push mel chunks, get audio after a fixed lookahead.  No reference counterpart: the reference has no
 *          streaming — its only caller (test.py:88-90) runs whole utterances through `self.generator(input_spec)`; this replaces cutting
 *          windows by hand around that call.  --------
 *
 * A stream serves `batch` sessions that advance in lockstep (every push gives each the same number of frames).  R = fv_reach_frames, the
 * generator's one-sided reach in input frames; K = context_frames and A = lookahead_frames (-1: R each).  Host counters: F frames received, E
 * frames emitted.  A push of n frames sets F += n, E' = max(E, F - A) and, if E' > E, runs the model ONCE on the window of frames [w, F),
 * w = max(0, E - K), and returns the output samples [(E - w) hop, (E' - w) hop) of that window: the frames [E, E').  A push emits at most n
 * frames; afterwards F - E <= A.  fv_stream_flush does the same with E' = F (the window's right edge is the utterance's end; at most A
 * frames) and then refuses pushes (FV_ERR_STATE) until fv_stream_reset (F = E = 0, allocations kept).
 *   - each call's output is bit-identical to the same slice of fv_forward on the frames [w, F) by the same engine and batch size;
 *   - K >= R and A >= R: the concatenated output is the whole utterance's shape and within 2e-5 * max(1, peak) of one fv_forward over it (the
 *     windows anchor the Winograd lattices elsewhere, as the time tiles do); an utterance of T <= A frames comes out of the flush alone, as
 *     the single window [0, T): bit-identical to fv_forward.
 * Models stream exactly when they are frame-aligned (what the time tiles need): HiFiGAN / BigVGAN (with or without use_template), Firefly,
 * Vocos and ISTFT heads with padding "same", the ConvNeXt encoder alone (hop = 1), RefineGAN once a noise seed is set
 * (fv_refinegan_set_noise_seed).  RefineGAN without a seed, LOGMEL, the "center" ISTFT head and upsamplers
 * whose output is not hop x frames get FV_ERR_UNSUPPORTED at fv_stream_create, with the reason in fv_last_error. */

/* R, the engine's one-sided reach in input frames (the halo of the time tiles); -1: this model cannot stream. */
FV_API int32_t fv_reach_frames(const fv_engine* e);

typedef struct fv_stream_config {
    int32_t batch;             /* sessions in lockstep (B) */
    int32_t max_chunk_frames;  /* largest n of one push */
    int32_t context_frames;    /* K; -1 = R */
    int32_t lookahead_frames;  /* A; -1 = R */
} fv_stream_config;

typedef struct fv_stream fv_stream;

/* The stream's only device allocation, made here on the current HIP device and freed by fv_stream_destroy: a ring of the last
 * K + A + max_chunk_frames frames per session, (batch, C_in, K + A + max_chunk_frames), plus (batch, 1, (K + A + max_chunk_frames) * hop) for
 * the pitch template of a use_template generator.  Everything else lives in the caller's workspace. */
FV_API fv_status fv_stream_create(fv_engine* e, const fv_stream_config* cfg, fv_stream** out);
/* Bytes of device scratch every push / flush needs (256-byte aligned): the window's input, template and output, and the forward's own
 * workspace for the largest window. */
FV_API size_t fv_stream_workspace_bytes(const fv_stream* s);
/* F - E: frames received but not yet emitted. */
FV_API int64_t fv_stream_pending_frames(const fv_stream* s);
/* d_mel: (batch, C_in, n) fp32, n <= max_chunk_frames (else FV_ERR_INVALID); d_template: (batch, 1, n * hop) for a use_template generator,
 * NULL otherwise (a missing or unexpected template: FV_ERR_INVALID); d_out: (batch, C_out, *frames_out * hop) fp32, contiguous — room for
 * min(n, max(0, pending + n - A)) frames, known before the call.  *frames_out receives the frames emitted; the counters are host-side, so the
 * call never synchronises.  n = 0 is a no-op.  Asynchronous on `stream`; calls on one stream must be ordered (one stream after another, or one
 * host thread), like fv_forward on its engine.  After a flush: FV_ERR_STATE. */
FV_API fv_status fv_stream_push(fv_stream* s, const float* d_mel, const float* d_template, int32_t n, float* d_out, int64_t* frames_out,
                                void* d_workspace, size_t workspace_bytes, void* stream);
/* Emits the pending frames (at most A) against the utterance's true end; d_out: (batch, C_out, pending * hop). */
FV_API fv_status fv_stream_flush(fv_stream* s, float* d_out, int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream);
/* F = E = 0 for the next utterance; the ring and its size are kept. */
FV_API fv_status fv_stream_reset(fv_stream* s);
/* Frees the ring (call it before fv_destroy of its engine, once the stream's work has finished). */
FV_API void fv_stream_destroy(fv_stream* s);

/* -------- ragged batches: one call for utterances of different lengths.  Replaces `sequence_mask(lengths)` over a padded forward
 *          (models/gan.py:237-238,291-299, utils/mask.py — the reference masks the result, it never makes a padded item equal to the item
 *          alone) and the per-file loop of test.py:52-99.  --------
 *
 * lengths[b] frames of clip b are valid inside a padded (batch, C_in, t_max) input.  One call writes (batch, C_out, t_max * hop):
 *   - samples [0, lengths[b] * hop) of row b are the clip's own forward: within 2e-5 * max(1, peak) of fv_forward on that clip alone (the
 *     bound of the time tiles, the streams and batches of other sizes), and bit-identical to the same slice of fv_forward over the clip's
 *     window (below) by the same engine and batch size;
 *   - samples from lengths[b] * hop on are exactly 0.0f (the reference's `fake_audio * audio_mask`);
 *   - nothing the caller left in the padding (x[b, :, lengths[b]:], NaN included) influences any output bit: it is never loaded.
 * The plan.  R = fv_reach_frames.  A window (clip b, start a, frames n, keep [lo, hi)) lets the forward see the frames [a, a + n) of clip b,
 * zero-filled from lengths[b] on, and copies out the samples of the clip's frames [lo, hi); windows of equal n run as ONE forward (a group).
 * A clip of T frames: T = 0: no window.  1 <= T <= 2R: the window (b, 0, T, [0, T)) — groups by exact length.  T > 2R: a body window
 * (b, 0, Tg, [0, T - R)) in a body group of Tg >= T frames (the zero fill past T is not the clip's end — the layers pad at the tensor edge —
 * so only frames >= R before T are kept) and a tail window (b, T - 2R, 2R, [T - R, T)), whose right edge is the clip's true end; a clip with
 * T == Tg keeps [0, T) of its body window and has no tail.  All tails and the clips of exactly 2R frames share one group.  Body groups: the
 * long clips sorted by (T, b), cut into at most max_groups contiguous runs (never between two clips of one length), minimising
 *     sum over runs ( clips * Tg + 2R * #{clips with T < Tg} + launch_frames ),   Tg = the run's longest clip,
 * ties: the fewest runs, then — from the last run backwards — the run that starts earliest.  Groups are numbered by descending length,
 * windows are listed by group, then by clip.  launch_frames (default 192) is the fixed cost of one more forward in frames, max_groups
 * (default 8) bounds the BODY groups (short clips group by exact length on top of it: up to 2R more forwards); both move speed only, never
 * a sample.  Equal lengths plan to one window per clip of n = T: exactly fv_forward.  vocoder_amd/ragged.py states the same plan in Python.
 * Eligible models are the ones that stream (fv_reach_frames >= 0); the others get FV_ERR_UNSUPPORTED at fv_ragged_create, with the reason
 * in fv_last_error.  A group longer than the addressing span of the conv kernels goes through the forward's own time tiles. */
typedef struct fv_ragged_window {
    int32_t clip, start, frames, keep_lo, keep_hi, group;
} fv_ragged_window;

/* Pure host: needs no device and no engine.  Writes the plan's windows to out (up to cap; out may be NULL when cap is 0) and returns how
 * many the plan has — a return value above cap says how large out must be.  reach < 1, batch < 1, a negative length: FV_ERR_INVALID.
 * launch_frames / max_groups <= 0: the defaults. */
FV_API int32_t fv_ragged_plan(int32_t reach, const int32_t* host_lengths, int32_t batch, int32_t launch_frames, int32_t max_groups,
                              fv_ragged_window* out, int32_t cap);

typedef struct fv_ragged fv_ragged;

/* Plans host_lengths (batch entries, each in [0, t_max]; else FV_ERR_INVALID) and uploads the window table — the plan's only device
 * allocation, made on the current HIP device and freed by fv_ragged_destroy.  May synchronise; fv_ragged_forward never does. */
FV_API fv_status fv_ragged_create(fv_engine* e, const int32_t* host_lengths, int32_t batch, int32_t t_max, int32_t launch_frames,
                                  int32_t max_groups, fv_ragged** out);
/* Bytes of device scratch fv_ragged_forward needs (256-byte aligned): window input | window template | window output, each sized for the
 * largest group, then the largest group's own fv_workspace_bytes. */
FV_API size_t fv_ragged_workspace_bytes(const fv_ragged* p);
FV_API int32_t fv_ragged_num_groups(const fv_ragged* p);
/* What forward g runs: *batch windows of *frames frames.  Returns FV_OK, or FV_ERR_INVALID for a g outside [0, fv_ragged_num_groups). */
FV_API int32_t fv_ragged_group(const fv_ragged* p, int32_t g, int32_t* batch, int32_t* frames);
/* The plan's windows, as fv_ragged_plan returns them. */
FV_API int32_t fv_ragged_windows(const fv_ragged* p, fv_ragged_window* out, int32_t cap);
/* d_in: (batch, C_in, t_max) fp32; d_template: (batch, 1, t_max * hop) for a use_template generator, NULL otherwise (a missing or
 * unexpected template: FV_ERR_INVALID, as fv_forward); d_out: (batch, C_out, t_max * hop) fp32, every sample of which is written.  Per
 * group, on `stream`, at fixed workspace addresses: gather of the windows, the unchanged forward (enqueued eagerly: the engine's captured
 * graphs and their bookkeeping are left alone), scatter of the kept samples; then the rows' tails are zeroed.  Asynchronous; ordered like
 * fv_forward on its engine.  Call fv_ragged_destroy before fv_destroy of the engine, once the plan's work has finished. */
FV_API fv_status fv_ragged_forward(fv_ragged* p, const float* d_in, const float* d_template, float* d_out, void* d_workspace,
                                   size_t workspace_bytes, void* stream);
FV_API void fv_ragged_destroy(fv_ragged* p);

/* -------- session pool: streaming sessions that advance independently.  No reference counterpart: the reference has no streaming and no
 *          server loop (test.py:52-99 runs whole files one by one); this replaces one fv_stream of batch 1, and one launch-bound forward,
 *          per live utterance.  --------
 *
 * A pool holds `sessions` slots.  Each slot has its own host counters F (frames received) and E (frames emitted), its own `flushed` flag
 * and its own ring row; K, A, R and the eligible models are the stream's (above).  One fv_pool_step serves any subset of the slots: item i
 * names a session, gives it n >= 0 frames and says whether the utterance ends with them (flush; n > 0 with flush is a last chunk).
 * Per item the counters move as a stream's: F' = F + n; E' = F' on a flush, else max(E, F' - A); w = max(0, E - K).  An item with E' > E is a
 * ROW: its window is the frames [w, F'), W = F' - w <= K + A + max_chunk_frames, it emits the frames [E, E').  A row owns its left edge iff
 * w = 0 and its right edge iff it flushes.
 * The plan.  Wg = the largest W over the rows.  Group 0 holds every row except those that own both edges and have W < Wg, as ONE
 * (rows, C_in, Wg) forward: a row that owns its left edge starts at column col0 = 0, any other row at col0 = Wg - W (right-aligned), and
 * every other column of the row is zero.  An emitted frame lies >= K frames inside a left edge the row does not own and >= A frames inside
 * such a right edge, so with K, A >= R it does not matter whether the tensor edge, zeros or other data lies beyond (the rule of the time
 * tiles, the streams and the ragged batches).  The rows left out are whole short utterances (a single window that owns both edges): they
 * form further groups by exact W, in descending W, at col0 = 0.  Rows within a group keep item order; rows are listed by group.
 *   - each row's samples are bit-identical to the same slice of fv_forward over its group's tensor by the same engine;
 *   - items in lockstep from equal state plan to one group with every col0 = 0: each step is bit-identical to fv_stream_push / _flush at
 *     batch = the number of items;
 *   - K >= R and A >= R: a session's concatenated output has the whole utterance's shape and is within 2e-5 * max(1, peak) of fv_forward
 *     on that utterance alone, whatever the other sessions do;
 *   - nothing in the chunk buffer's columns >= n of an item (NaN included), and nothing of another session, reaches any output bit;
 *   - every sample of d_out is written: past an item's emitted samples, and in the rows of items that emit nothing, exactly 0.0f.
 * vocoder_amd/sessions.py states the same plan in Python. */
typedef struct fv_pool_config {
    int32_t sessions;          /* slots (S) */
    int32_t max_chunk_frames;  /* largest n of one item */
    int32_t context_frames;    /* K; -1 = R (fv_pool_plan has no engine: >= 0 there) */
    int32_t lookahead_frames;  /* A; -1 = R (likewise) */
} fv_pool_config;

typedef struct fv_pool_item {
    int32_t session;           /* slot in [0, S); at most once per step */
    int32_t frames;            /* n in [0, max_chunk_frames] */
    int32_t flush;             /* 1: the utterance ends with these frames */
} fv_pool_item;

typedef struct fv_pool_row {
    int32_t item;              /* index into the step's items */
    int32_t group;             /* forward that runs it; group 0 is the aligned one */
    int32_t col0;              /* first column of the window inside the group's tensor */
    int32_t frames;            /* W */
    int64_t w;                 /* the window is the utterance's frames [w, w + W) */
    int64_t emit_lo, emit_hi;  /* the frames [E, E') the step emits: samples [(col0 + E - w) hop, (col0 + E' - w) hop) of the row's output */
} fv_pool_row;

/* Pure host: needs no device and no engine.  received / emitted / flushed: the S counters and flags (flushed may be NULL: none is).  Writes
 * the plan's rows to rows (up to row_cap; NULL when 0) and, per group, its number of rows and its length in frames to group_rows /
 * group_frames (up to group_cap; NULL when 0), the number of groups to *num_groups (may be NULL), and returns the number of rows — a plan
 * has at most `count` rows and `count` groups.  Nothing is changed: the caller moves the counters.  Refusals, each named in fv_last_error:
 * a session outside [0, S), a duplicate session, frames outside [0, max_chunk_frames], in_frames < the largest n, out_frames < the largest
 * E' - E (either may be -1: not checked), K or A < 0 (FV_ERR_INVALID); an item for a flushed session (FV_ERR_STATE). */
FV_API int32_t fv_pool_plan(const fv_pool_config* cfg, const int64_t* received, const int64_t* emitted, const int32_t* flushed,
                            const fv_pool_item* items, int32_t count, int32_t in_frames, int32_t out_frames, fv_pool_row* rows,
                            int32_t row_cap, int32_t* group_rows, int32_t* group_frames, int32_t group_cap, int32_t* num_groups);

typedef struct fv_pool fv_pool;

/* The pool's only device allocation, made here on the current HIP device and freed by fv_pool_destroy: one ring row per slot,
 * (S, C_in, cap) with cap = K + A + max_chunk_frames, plus (S, 1, cap * hop) for the pitch template of a use_template generator.  Models
 * that cannot stream get FV_ERR_UNSUPPORTED, with the reason in fv_last_error (as fv_stream_create). */
FV_API fv_status fv_pool_create(fv_engine* e, const fv_pool_config* cfg, fv_pool** out);
/* Bytes of device scratch every step needs (256-byte aligned): a group's input, template and output for S rows of cap frames, and the
 * forward's own workspace for the largest window at batch S. */
FV_API size_t fv_pool_workspace_bytes(const fv_pool* p);
/* F - E of one slot: frames received but not yet emitted (0 for a session outside [0, S)). */
FV_API int64_t fv_pool_pending_frames(const fv_pool* p, int32_t session);
/* One step.  d_chunks: (count, C_in, in_frames) fp32, row i holding item i's n frames first (the rest is never loaded; NULL when no item
 * has frames); d_templates: (count, 1, in_frames * hop) for a use_template generator, NULL otherwise; d_out: (count, C_out, out_frames *
 * hop), row i receiving item i's emitted samples first and 0.0f after them (NULL when out_frames is 0); frames_out (may be NULL): count
 * entries, E' - E of every item.  The whole step is checked before any counter moves or anything is enqueued — the refusals of
 * fv_pool_plan, a missing or unexpected template, a missing chunk buffer, a workspace below fv_pool_workspace_bytes (FV_ERR_INVALID) —
 * and a refused step leaves every counter and every ring as it was.  Per group, on `stream`: one gather launch (chunk -> ring, ring +
 * chunk -> the group's tensor), the unchanged forward, one crop launch.  Group 0 runs at fixed workspace addresses through the graph
 * bookkeeping of fv_forward: a steady state with the same rows and the same Wg replays its captured graph; further groups are enqueued
 * eagerly.  The step's row table travels in the kernel arguments: no device allocation, no copy, no host synchronisation.  Asynchronous;
 * ordered like fv_forward on its engine. */
FV_API fv_status fv_pool_step(fv_pool* p, const fv_pool_item* items, int32_t count, const float* d_chunks, const float* d_templates,
                              int32_t in_frames, float* d_out, int32_t out_frames, int64_t* frames_out, void* d_workspace,
                              size_t workspace_bytes, void* stream);
/* F = E = 0 and not flushed for one slot: the next utterance; the ring is kept.  A session outside [0, S): FV_ERR_INVALID. */
FV_API fv_status fv_pool_reset(fv_pool* p, int32_t session);
/* Frees the rings (call it before fv_destroy of its engine, once the pool's work has finished). */
FV_API void fv_pool_destroy(fv_pool* p);

/* -------- sample-rate conversion: audio at any rate in, audio at any rate out.  Replaces the reference's two resampling front doors:
 *          `librosa.load(..., sr=cfg.model.sampling_rate)` (test.py:54) and `torchaudio.functional.resample` (AF.resample,
 *          data/transforms/hq_pitch_shift.py:33).  --------
 *
 * The arithmetic is the polyphase windowed-sinc resampler of torchaudio.transforms.Resample (restated; torchaudio is not a dependency):
 *   g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g, base = min(o, n) * rolloff, width = ceil(lpw * o / base);
 *   for phase p in [0, n), tap j in [0, 2 width + o):  t = clamp(((j - width) / o - p / n) * base, -lpw, +lpw),
 *     h[p][j] = (t == 0 ? 1 : sin(pi t) / (pi t)) * win(t) * base / o,  win = cos(t pi / lpw / 2)^2 (hann) | I0(beta sqrt(1 - (t / lpw)^2)) / I0(beta);
 *   y[f n + p] = sum_j h[p][j] xp[f o + j], xp = x with `width` zeros in front; the first ceil(n L / o) outputs are kept.
 * The taps are computed on the host in float64 and rounded to fp32.  Only the band |t| < lpw of a phase is not zero: phase p keeps the taps
 * j in [first[p], first[p] + count[p]), count[p] <= Kp, and output m = f n + p reads x[f o + first[p] - width + i], i < count[p].  Each output is
 * summed over ascending i in one fp32 accumulator (fused multiply-adds), whatever the tile, the row, the launch or the chunking: the results of
 * fv_resample_forward on a row alone, on the same row inside a ragged batch, and of a stream's pushes over it are bit-identical.
 * The kernel is a banded FIR on the vector ALU, not an MFMA GEMM: the dense form holds 7 - 14 times the taps of the band.
 *
 * LDS limit: a workgroup keeps the whole table (n rows of Kp taps, rows padded to an odd length, plus first[] and count[]) and a tile of
 * fv_resample_input_tile() + Kp + 3 input samples in 64 KiB of LDS.  A rate pair whose table does not fit beside the tile (roughly
 * n * Kp > 7000, e.g. 44101 -> 48000) gets FV_ERR_UNSUPPORTED from fv_resample_create, with the pair and the size in fv_last_error. */
typedef enum fv_resample_method {
    FV_RESAMPLE_SINC_HANN = 0,   /* resampling_method="sinc_interp_hann", torchaudio's default (what hq_pitch_shift.py:33 gets) */
    FV_RESAMPLE_SINC_KAISER = 1  /* "sinc_interp_kaiser" */
} fv_resample_method;

/* The arguments of torchaudio.functional.resample / transforms.Resample (hq_pitch_shift.py:33 passes the first two; test.py:54 names the
 * target rate).  beta <= 0: torchaudio's default, 14.769656459379492 (kaiser only). */
typedef struct fv_resample_config {
    int32_t orig_freq;
    int32_t new_freq;
    int32_t lowpass_filter_width;  /* lpw, torchaudio's default 6 */
    double rolloff;                /* in (0, 1], torchaudio's default 0.99 */
    int32_t method;                /* fv_resample_method */
    double beta;
} fv_resample_config;

/* The filter design alone, on the host (no GPU), as fv_ragged_plan / fv_pool_plan are: what test.py:54 / hq_pitch_shift.py:33 leave to their
 * libraries.  *o, *n, *width, *kp always; first / count (n entries each, capacity phase_cap) and taps (n rows of kp, zero past count[p];
 * capacity taps_cap floats) when not NULL — call once with NULL arrays for the sizes.  FV_ERR_INVALID names the offending field. */
FV_API fv_status fv_resample_design(const fv_resample_config* cfg, int32_t* o, int32_t* n, int32_t* width, int32_t* kp, int32_t* first,
                                    int32_t* count, int32_t phase_cap, float* taps, int64_t taps_cap);
/* Input samples of the kernel's tile (a workgroup owns the outputs whose first input sample falls into one tile). */
FV_API int32_t fv_resample_input_tile(void);

typedef struct fv_resample fv_resample;

/* Designs the filter and uploads its table to the current HIP device (the object's only allocation); stands in for building
 * torchaudio.transforms.Resample(orig_freq, new_freq, ...) in front of test.py:54 / hq_pitch_shift.py:33. */
FV_API fv_status fv_resample_create(const fv_resample_config* cfg, fv_resample** out);
FV_API void fv_resample_destroy(fv_resample* r);
/* ceil(n L / o): the length librosa.load(sr=...) (test.py:54) / AF.resample (hq_pitch_shift.py:33) return for L input samples; -1: bad argument. */
FV_API int64_t fv_resample_output_length(const fv_resample* r, int64_t L);
/* d_x: `batch` rows of L fp32 samples, row b at d_x + b * x_row_stride (rows = the flattened leading dimensions of the waveform that
 * test.py:54 / hq_pitch_shift.py:33 resample); d_y: `batch` rows of fv_resample_output_length(r, L), row b at d_y + b * y_row_stride; the strides
 * count floats and are >= the row's width.  d_y must not overlap d_x (FV_ERR_INVALID).  d_lengths: NULL, or `batch` int32 on the device — row b
 * holds lengths[b] <= L samples (clamped to [0, L]; fv_resample_check_lengths refuses others from the host side); the samples past a row's length
 * are never loaded, its ceil(n lengths[b] / o) outputs are bit-identical to the row run alone and are followed by exact zeros.  Asynchronous on
 * `stream`. */
FV_API fv_status fv_resample_forward(fv_resample* r, const float* d_x, int64_t x_row_stride, const int32_t* d_lengths, float* d_y,
                                     int64_t y_row_stride, int32_t batch, int64_t L, void* stream);
/* Host-side check of a ragged call's lengths before they go to the device (test.py:54 resamples one file, this batches several): FV_ERR_INVALID
 * with the row named when a length is negative or > L. */
FV_API fv_status fv_resample_check_lengths(const fv_resample* r, const int32_t* host_lengths, int32_t batch, int64_t L);

/* Streaming form (no reference counterpart: test.py:54 / hq_pitch_shift.py:33 resample whole clips): `batch` rows advance in lockstep.  Host
 * counters: N input samples received, E outputs emitted.  Output m is emitted as soon as its band has arrived: a push sets N += c and emits the
 * outputs [E, M(N)), M(N) = #{m : first_input(m) + count[p(m)] <= N}; the flush emits [E, ceil(n N / o)) against zeros and then refuses pushes
 * (FV_ERR_STATE) until fv_resample_stream_reset.  The latency is the band's half width, about lpw * o / base input samples.  The concatenated
 * outputs are bit-identical to fv_resample_forward over the whole rows.  A refused call changes nothing. */
typedef struct fv_resample_stream fv_resample_stream;

/* The stream's only device allocation, made here and freed by fv_resample_stream_destroy: two (batch, Kp + max_chunk) buffers that carry each
 * row's last Kp input samples from push to push. */
FV_API fv_status fv_resample_stream_create(fv_resample* r, int32_t batch, int32_t max_chunk, fv_resample_stream** out);
/* ceil(n N / o) - E: the outputs a flush would emit now. */
FV_API int64_t fv_resample_stream_pending(const fv_resample_stream* s);
/* d_x: (batch, c) with row stride x_row_stride, c <= max_chunk (else FV_ERR_INVALID); d_y: (batch, M(N + c) - E) with row stride y_row_stride —
 * the count is known before the call (vocoder_amd.resample emit_count) and may be 0, then d_y may be NULL.  *emitted receives it; the counters are
 * host-side, so the call never synchronises.  c = 0 is a no-op.  Asynchronous on `stream`; calls on one stream object must be ordered. */
FV_API fv_status fv_resample_stream_push(fv_resample_stream* s, const float* d_x, int64_t x_row_stride, int32_t c, float* d_y,
                                         int64_t y_row_stride, int64_t* emitted, void* stream);
FV_API fv_status fv_resample_stream_flush(fv_resample_stream* s, float* d_y, int64_t y_row_stride, int64_t* emitted, void* stream);
/* N = E = 0 for the next utterance; the buffers are kept. */
FV_API fv_status fv_resample_stream_reset(fv_resample_stream* s);
/* Call it before fv_resample_destroy of its resampler, once the stream's work has finished. */
FV_API void fv_resample_stream_destroy(fv_resample_stream* s);

/* -------- audio in: the log-mel front-end on rows of different lengths and on chunks of a stream.  Replaces calling
 *          `LogMelSpectrogram.forward` (data/transforms/spectrogram.py:25-104) on one whole, equal-length tensor per file, as the wav branch of
 *          test.py:64-71 does (zero padding, then `mel_transforms.input`); the reference has neither a ragged nor a streaming form.  --------
 *
 * These entries take a FV_MODEL_LOGMEL engine (any other: FV_ERR_UNSUPPORTED).  fv_stream_create, fv_ragged_* and fv_pool_* keep refusing such
 * an engine: they window FRAMES under a reach rule, while the front-end windows SAMPLES under the framing rule below.
 * pad_l = (win_length - hop) / 2, pad_r = (win_length - hop + 1) / 2 (spectrogram.py:30-33).  Frame f of a row reads the wave indices
 * [f hop - pad_l, f hop - pad_l + n_fft), reflected at 0 and at the row's last sample.  Only the first step differs from fv_forward: one kernel
 * writes the polyphase signal of the frames [f0, f0 + n) with per-row edges (samples at or past a row's end are never loaded), and the
 * forward's own STFT conv, magnitude and filterbank conv run behind it.  With fv_set_batch_invariant(e, 1) every output column is one
 * fixed-order sum, so a frame's values do not depend on the call that produced it: a row inside a ragged batch, the same row through
 * fv_forward and any chunking of it through a stream agree bit for bit.  All calls enqueue eagerly and leave the captured graphs of fv_forward
 * alone. */

/* Pure host (no engine, no GPU), as fv_ragged_plan and fv_resample_design are; stand in for the frame count that torch.stft(center=False) derives
 * inside spectrogram.py:25-56 / test.py:64-71.  Frames of a whole row of L samples: 1 + (L + pad_l + pad_r - n_fft) / hop, 0 when the padded
 * row is shorter than one frame (or the config is unusable). */
FV_API int64_t fv_logmel_frames(const fv_logmel_config* cfg, int64_t L);
/* Frames that need no sample at or after N, i.e. that a stream can emit once N samples have arrived (spectrogram.py:25-56 / test.py:64-71 see
 * whole files only): 1 + (N + pad_l - n_fft) / hop once N + pad_l >= n_fft, else 0.  Never above fv_logmel_frames(cfg, N). */
FV_API int64_t fv_logmel_frames_ready(const fv_logmel_config* cfg, int64_t N);

/* One call for rows of different lengths (replaces one spectrogram.py:25-104 call per file, test.py:64-71).  d_wave: `batch` rows, row b at
 * d_wave + b * row_stride (floats, >= L_max) holding host_lengths[b] <= L_max samples; d_out: (batch, C_out, fv_logmel_frames(L_max)) fp32;
 * fv_workspace_bytes(e, batch, L_max) bytes of workspace are enough.  Row b holds its own log-mel in the columns [0, T_b),
 * T_b = fv_logmel_frames(lengths[b]) — within 2e-4 of the reference on the log values, the front-end's bar — and exactly 0.0f after them; a
 * length of 0 is an empty row, all zeros.  Samples at or after lengths[b] (NaN included) are never loaded.  Any other length that fv_forward
 * alone would refuse (no frame, or not longer than the reflect padding), a negative length and one above L_max get FV_ERR_INVALID with the
 * row named; everything is validated before anything is enqueued.  Known cost: every row's convs run over T_max = fv_logmel_frames(L_max)
 * columns, so the work is batch * T_max, not the sum of T_b — group rows of similar length into one call.  Asynchronous on `stream`; ordered
 * like fv_forward on its engine. */
FV_API fv_status fv_logmel_ragged_forward(fv_engine* e, const float* d_wave, int64_t row_stride, const int32_t* host_lengths, int32_t batch,
                                          int32_t L_max, float* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* Streaming form (no reference counterpart: spectrogram.py:25-104 / test.py:64-71 take whole files): `batch` rows advance in lockstep.  Host
 * counters: N samples received, E frames emitted.  A push sets N += c and emits the frames [E, fv_logmel_frames_ready(N)); the flush emits
 * [E, fv_logmel_frames(N)) against the rows' true end (right reflection) and then refuses pushes (FV_ERR_STATE) until
 * fv_logmel_stream_reset.  A flush at N = 0 emits nothing; a flush of an utterance too short for one frame or for the reflection is
 * FV_ERR_INVALID.  A refused call changes nothing.  Latency: a frame comes out pad_r samples after its own hop has arrived — 768 samples, 17 ms,
 * at 44100 Hz / n_fft 2048 / hop 512.  No call synchronises. */
typedef struct fv_logmel_stream fv_logmel_stream;

/* The stream's only device allocation, made here (spectrogram.py:25-104 / test.py:64-71 keep no state) and freed by fv_logmel_stream_destroy: two
 * (batch, n_fft) carry buffers used in turn, so that no launch writes the carry and reads it back.  After a call the carry covers the samples
 * [max(0, E hop - pad_l), N) that later frames still need: fewer than n_fft of them.  max_chunk_samples: the largest c of one push. */
FV_API fv_status fv_logmel_stream_create(fv_engine* e, int32_t batch, int32_t max_chunk_samples, fv_logmel_stream** out);
/* Bytes of device scratch every push / flush needs (256-byte aligned): the front-end's workspace (spectrogram.py:25-104 / test.py:64-71 allocate
 * theirs per call) for the most frames one call can emit. */
FV_API size_t fv_logmel_stream_workspace_bytes(const fv_logmel_stream* s);
/* N - max(0, E hop - pad_l): samples received that frames not yet emitted still read (what spectrogram.py:25-104 / test.py:64-71 would hold as
 * the file's tail). */
FV_API int64_t fv_logmel_stream_pending_samples(const fv_logmel_stream* s);
/* d_wave: (batch, c) with row stride row_stride, c <= max_chunk_samples (else FV_ERR_INVALID) — the next samples of what test.py:64-71 hands
 * spectrogram.py:25-104 whole; d_out: (batch, C_out, k) fp32, contiguous, k = fv_logmel_frames_ready(N + c) - E known before the call; k may be
 * 0, then d_out may be NULL.  *frames_out receives k.  c = 0 is a no-op.  Asynchronous on `stream`; calls on one stream must be ordered. */
FV_API fv_status fv_logmel_stream_push(fv_logmel_stream* s, const float* d_wave, int64_t row_stride, int32_t c, float* d_out,
                                       int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream);
/* Emits the frames [E, fv_logmel_frames(N)) against the utterance's end, the right edge of spectrogram.py:25-104 / test.py:64-71;
 * d_out: (batch, C_out, fv_logmel_frames(N) - E). */
FV_API fv_status fv_logmel_stream_flush(fv_logmel_stream* s, float* d_out, int64_t* frames_out, void* d_workspace, size_t workspace_bytes,
                                        void* stream);
/* N = E = 0 for the next utterance (the next file of test.py:64-71 / spectrogram.py:25-104); the carry buffers are kept. */
FV_API fv_status fv_logmel_stream_reset(fv_logmel_stream* s);
/* Frees the carry (call it before fv_destroy of its engine, once the stream's work has finished); spectrogram.py:25-104 / test.py:64-71 have
 * nothing to free. */
FV_API void fv_logmel_stream_destroy(fv_logmel_stream* s);

/* -------- audio in, per session: the log-mel front-end as a pool of sessions that advance independently — what fv_pool_* is to fv_stream_*,
 *          for samples.  No reference counterpart: spectrogram.py:25-104 / test.py:64-71 take one whole file at a time.  --------
 *
 * A wav pool holds S slots on a FV_MODEL_LOGMEL engine.  Each slot has its own counters N (samples received) and E (frames emitted), its own
 * flushed flag and its own n_fft carried samples.  A step is a list of items (session, samples, flush): any subset of the slots, each at
 * most once, each with its own chunk size.  Per item, the stream's push and flush folded into one call:
 *   N' = N + samples;  E' = max(E, flush ? fv_logmel_frames(N') : fv_logmel_frames_ready(N'));  the item emits the frames [E, E').
 * With flush the frames reflect at the true end N' and the slot refuses items (FV_ERR_STATE) until fv_wavpool_reset.  A flush at N' = 0
 * emits nothing; a flush of an utterance that fv_forward alone would refuse (no frame, or not longer than the reflect padding) refuses the
 * whole step with FV_ERR_INVALID and names the session.  The whole step is checked before any counter moves or anything is enqueued: a
 * refused step leaves every slot as it was.  One step is one window launch for all its rows (a table entry per row: chunk row, slot and
 * carry buffer, origins, end, first frame), the forward's own STFT conv, magnitude and filterbank conv on (rows, max k) columns, one crop
 * launch and one carry launch; the tables travel in the kernel arguments, 32 entries per launch.  With fv_set_batch_invariant(e, 1) every
 * frame has the bits of fv_forward over the session's whole utterance, whatever the other sessions do.  The entries enqueue eagerly and leave
 * the captured graphs of fv_forward alone.  fv_pool_create keeps refusing a log-mel engine; vocoder_amd/framing.py (PoolCounters) states
 * the same plan in Python. */
typedef struct fv_wavpool_item {
    int32_t session;           /* slot in [0, S); at most once per step */
    int32_t samples;           /* in [0, max_chunk_samples] */
    int32_t flush;             /* 1: the utterance ends with these samples */
} fv_wavpool_item;

typedef struct fv_wavpool fv_wavpool;

/* The pool's only device allocation, made here on the current HIP device (spectrogram.py:25-104 / test.py:64-71 keep no state) and freed by
 * fv_wavpool_destroy: two (S, n_fft) carry buffers; every slot has its own bit saying which of the two holds its samples, and only a slot
 * that pushed samples flips it, so no launch writes a slot's carry and reads it back and an idle slot's carry stays where it is read.
 * Engines other than FV_MODEL_LOGMEL: FV_ERR_UNSUPPORTED, by name; sessions outside [1, 65535] or max_chunk_samples outside [1, 2^28]:
 * FV_ERR_INVALID. */
FV_API fv_status fv_wavpool_create(fv_engine* logmel_engine, int32_t sessions, int32_t max_chunk_samples, fv_wavpool** out);
/* Bytes of device scratch every step needs (256-byte aligned): the front-end's workspace (spectrogram.py:25-104 / test.py:64-71 allocate theirs
 * per call) for S rows of fv_wavpool_max_frames frames, and the rows' result before the crop. */
FV_API size_t fv_wavpool_workspace_bytes(const fv_wavpool* p);
/* The most frames one item emits in one step — a first emission plus a flush: (n_fft + max_chunk_samples) / hop + 2 (the frame count that
 * spectrogram.py:25-104 / test.py:64-71 get for a whole file never enters).  An out_frames of this size serves every step. */
FV_API int32_t fv_wavpool_max_frames(const fv_wavpool* p);
/* N of one slot: the samples of the current utterance (the file of test.py:64-71 / spectrogram.py:25-104) received so far; 0 for a session
 * outside [0, S). */
FV_API int64_t fv_wavpool_received_samples(const fv_wavpool* p, int32_t session);
/* E of one slot: the frames (columns of spectrogram.py:25-104 / test.py:64-71's result) emitted so far; 0 for a session outside [0, S). */
FV_API int64_t fv_wavpool_emitted_frames(const fv_wavpool* p, int32_t session);
/* N - max(0, E hop - pad_l) of one slot: samples received that frames not yet emitted still read (what spectrogram.py:25-104 / test.py:64-71
 * would hold as the file's tail); 0 for a session outside [0, S). */
FV_API int64_t fv_wavpool_pending_samples(const fv_wavpool* p, int32_t session);
/* Pure host (no engine, no GPU), as fv_pool_plan is: what a step would emit, from the framing of spectrogram.py:25-104 / test.py:64-71 alone.
 * received / emitted / flushed: the S counters and flags (flushed may be NULL: none is).  Writes E' - E of every item to frames_out (count
 * entries) and returns the largest of them; nothing is changed: the caller moves the counters.  Refuses what fv_wavpool_step refuses of the
 * items, each named in fv_last_error, with the status as the (negative) result: a session outside [0, S), a duplicate session, samples
 * outside [0, max_chunk_samples], more than 2^40 samples, a flush of an utterance too short for the reflect padding or for one frame
 * (FV_ERR_INVALID); an item for a flushed session (FV_ERR_STATE); an unusable config or sessions outside [1, 65535] (FV_ERR_INVALID). */
FV_API int32_t fv_wavpool_plan(const fv_logmel_config* cfg, int32_t sessions, int32_t max_chunk_samples, const int64_t* received,
                               const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                               int64_t* frames_out);
/* One step (replaces one spectrogram.py:25-104 call per file, test.py:64-71, for sessions whose audio arrives at different times).  d_chunks:
 * (count, chunk_stride) fp32, row i holding item i's samples first — the rest of the row (NaN included) is never loaded; NULL when no item
 * has samples.  d_out: (count, C_out, out_frames) fp32 with out_frames >= the largest E' - E of the step (NULL when out_frames is 0): row i
 * receives item i's frames first and exactly 0.0f after them, an item that emits nothing a row of zeros; every element is written.
 * frames_out (may be NULL): count entries, E' - E of every item.  Refusals, checked for the whole step before anything moves: those of
 * fv_wavpool_plan, a NULL chunk buffer although an item has samples, chunk_stride shorter than the longest chunk, out_frames too small, a
 * workspace below fv_wavpool_workspace_bytes (FV_ERR_INVALID).  No device allocation, no copy, no host synchronisation.  Asynchronous on
 * `stream`; ordered like fv_forward on its engine. */
FV_API fv_status fv_wavpool_step(fv_wavpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_out, int32_t out_frames, int64_t* frames_out, void* d_workspace, size_t workspace_bytes,
                                 void* stream);
/* N = E = 0 and not flushed for one slot: its next utterance (the next file of test.py:64-71 / spectrogram.py:25-104).  The carry is kept:
 * samples before 0 are zeros by index, whatever it holds.  A session outside [0, S): FV_ERR_INVALID. */
FV_API fv_status fv_wavpool_reset(fv_wavpool* p, int32_t session);
/* Frees the carry (call it before fv_destroy of its engine, once the pool's work has finished); spectrogram.py:25-104 / test.py:64-71 have
 * nothing to free. */
FV_API void fv_wavpool_destroy(fv_wavpool* p);

/* -------- the resampler with its table in global memory: any rate pair.  fv_resample_create keeps the whole table in LDS and refuses the
 *          pairs whose table does not fit (44101 -> 48000; the 52400 -> 44100 of a pitch shift at lowpass_filter_width 64); this entry takes them.
 *          Same object, same design (fv_resample_design), same functions: fv_resample_forward with or without d_lengths and
 *          fv_resample_stream_* dispatch on where the table lives.  The kernel stages only the input tile in LDS and reads first[], count[] and
 *          the taps from global memory (they stay in L2); its tiling and every output's sum — ascending taps, one fp32 accumulator, fused
 *          multiply-adds — are those of the LDS kernel, so for a pair that both forms take the results agree bit for bit.  Stands in for
 *          torchaudio.transforms.Resample in front of test.py:54 / hq_pitch_shift.py:33 and for the resample step of
 *          librosa.effects.pitch_shift (test.py:61-62).  FV_ERR_UNSUPPORTED only when one phase's band does not fit beside the input tile
 *          (Kp of several thousand taps) or the table passes 1 GiB.  (Named outside the fv_resample_ prefix: that family's list of entries is
 *          pinned by its host test.) -------- */
FV_API fv_status fv_global_resample_create(const fv_resample_config* cfg, fv_resample** out);

/* -------- sample-rate conversion, per session: the resampler as a pool of sessions that advance independently — what fv_wavpool_* is to
 *          fv_logmel_stream_*, for fv_resample_stream_*.  No reference counterpart: test.py:54 / hq_pitch_shift.py:33 resample whole clips and
 *          keep no per-session state.  (Named fv_respool_*, outside the fv_resample_ prefix: that family's list of entries is pinned by its
 *          host test.)  --------
 *
 * A resample pool holds S slots on one fv_resample (either table form; one pool is one rate pair).  Each slot has its own counters N (input
 * samples received) and E (outputs emitted), its own flushed flag and its own H = Kp rounded up to 4 carried samples.  A step is a list of
 * fv_wavpool_item (session, samples, flush): any subset of the slots, each at most once, each with its own chunk size.  Per item, the
 * stream's push and flush folded into one call, with M(N) the emission rule of fv_resample_stream_push:
 *   N' = N + samples;  E' = flush ? ceil(n N' / o) : max(E, M(N'));  the item emits the outputs [E, E').
 * With flush the rest comes out against zeros and the slot refuses items (FV_ERR_STATE) until fv_respool_reset; a flush at N' = 0 emits
 * nothing.  The whole step is checked before any counter moves or anything is enqueued: a refused step leaves every slot as it was.  One step
 * is one FIR launch and one carry launch per 32 items; the items' table entries (chunk row, slot and carry buffer, origins, first output,
 * count) travel in the kernel arguments.  An item's workgroups stage their input tiles from the slot's carried samples and from its chunk
 * row, and every output is the sum fv_resample_forward forms — ascending taps, one fp32 accumulator, fused multiply-adds — so a session's
 * concatenated outputs are bit-identical to fv_resample_forward over its whole utterance and to an fv_resample_stream fed the same chunks,
 * whatever the other sessions do.  The entries enqueue eagerly. */
typedef struct fv_respool fv_respool;

/* The pool's only device allocation, made here on the current HIP device (test.py:54 / hq_pitch_shift.py:33 keep no state) and freed by
 * fv_respool_destroy: two (S, H) carry buffers; every slot has its own bit saying which of the two holds its samples, and only a slot that
 * pushed samples flips it.  sessions outside [1, 65535] or max_chunk outside [1, 2^28]: FV_ERR_INVALID. */
FV_API fv_status fv_respool_create(fv_resample* r, int32_t sessions, int32_t max_chunk, fv_respool** out);
/* The most one item can emit in one step (the length that test.py:54 / hq_pitch_shift.py:33 get for a whole clip never enters): a push of
 * max_chunk samples that also flushes.  Between flushes E = M(N), so such a step emits g(N) = ceil(n (N + max_chunk) / o) - M(N).  M jumps at
 * the N at which a band ends, N = f o + first[p] + count[p] - width, n times per o samples, and ceil() never falls: g is largest just before
 * a jump.  From N >= first[n - 1] + count[n - 1] - width - o on, M(N + o) = M(N) + n, and before that M is clamped at 0 from below, so g is
 * periodic there and no larger before: the result is the largest g(f o + first[p] + count[p] - width - 1) over the n phases of one frame f
 * past that point.  Exact: some state attains it.  An out_cols of this size serves every step.  0 for a NULL pool. */
FV_API int64_t fv_respool_max_outputs(const fv_respool* p);
/* N of one slot: the input samples of the current utterance (the clip of test.py:54 / hq_pitch_shift.py:33) received so far; 0 for a session
 * outside [0, S). */
FV_API int64_t fv_respool_received(const fv_respool* p, int32_t session);
/* E of one slot: the outputs (samples of what test.py:54 / hq_pitch_shift.py:33 return) emitted so far; 0 for a session outside [0, S). */
FV_API int64_t fv_respool_emitted(const fv_respool* p, int32_t session);
/* ceil(n N / o) - E of one slot: the outputs a flush would emit now (the tail of test.py:54 / hq_pitch_shift.py:33's result); 0 for a session
 * outside [0, S). */
FV_API int64_t fv_respool_pending(const fv_respool* p, int32_t session);
/* Pure host (no GPU), as fv_wavpool_plan is: what a step would emit, from the filter design alone (what test.py:54 / hq_pitch_shift.py:33
 * leave to their libraries).  received / emitted / flushed: the S counters and flags (flushed may be NULL: none is).  Designs the filter,
 * writes E' - E of every item to outputs_out (count entries) and returns the largest of them; nothing is changed: the caller moves the
 * counters.  Refuses what fv_respool_step refuses of the items, each named in fv_last_error, with the status as the (negative) result: a
 * session outside [0, S), a duplicate session, samples outside [0, max_chunk], more than 2^40 samples (FV_ERR_INVALID); an item for a flushed
 * session (FV_ERR_STATE); a config that fv_resample_design refuses, sessions outside [1, 65535] or max_chunk outside [1, 2^28]. */
FV_API int64_t fv_respool_plan(const fv_resample_config* cfg, int32_t sessions, int32_t max_chunk, const int64_t* received,
                               const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                               int64_t* outputs_out);
/* One step (replaces one test.py:54 / hq_pitch_shift.py:33 call per clip, for sessions whose audio arrives at different times).  d_chunks:
 * (count, chunk_stride) fp32, row i holding item i's samples first — the rest of the row (NaN included) is never loaded; NULL when no item
 * has samples.  d_out: (count, out_stride) fp32 with out_stride >= out_cols >= the largest E' - E of the step (NULL when out_cols is 0): the
 * first out_cols columns of row i receive item i's outputs and exactly 0.0f after them, an item that emits nothing a row of zeros; every one
 * of them is written.  outputs_out (may be NULL): count entries, E' - E of every item.  Refusals, checked for the whole step before anything
 * moves, each naming the item and the session: those of fv_respool_plan, a NULL chunk buffer although an item has samples, chunk_stride
 * shorter than the longest chunk, out_cols below the largest E' - E, out_stride < out_cols, a NULL d_out although an item emits
 * (FV_ERR_INVALID).  No device allocation, no copy, no host synchronisation.  Asynchronous on `stream`; steps of one pool must be ordered. */
FV_API fv_status fv_respool_step(fv_respool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_out, int64_t out_stride, int32_t out_cols, int64_t* outputs_out, void* stream);
/* N = E = 0 and not flushed for one slot: its next utterance (the next clip of test.py:54 / hq_pitch_shift.py:33).  The carry is kept:
 * samples before 0 are zeros by index, whatever it holds.  A session outside [0, S): FV_ERR_INVALID. */
FV_API fv_status fv_respool_reset(fv_respool* p, int32_t session);
/* Frees the carry (call it before fv_resample_destroy of its resampler, once the pool's work has finished); test.py:54 /
 * hq_pitch_shift.py:33 have nothing to free. */
FV_API void fv_respool_destroy(fv_respool* p);

/* -------- pitch shift: `librosa.effects.pitch_shift(gt_y, sr=sr, n_steps=cfg.pitch_shift)` (test.py:61-62), the step between loading /
 *          resampling a file and the mel front-end.  librosa is not a dependency; its arithmetic is restated: a time stretch by
 *          rate = 2^(-n_steps / bins_per_octave) with a phase vocoder (stft, n_fft 2048, hop n_fft / 4, periodic hann, center=True with zero
 *          padding; phase_vocoder; istft), then a resample from sr / rate back to sr, fixed to the input length.  --------
 *
 * Plan (integers): orig_freq = floor(sr * 2^(n_steps / bpo) + 0.5), then orig_freq -= orig_freq % freq_granularity (the reference's own rule,
 * hq_pitch_shift.py:30-31); g = gcd(orig_freq, sr), o = orig_freq / g, n = sr / g: the stretch rate is exactly n / o.  orig_freq == sr: the
 * output is a bit-for-bit copy of the input.
 * Analysis: T = 1 + L / hop frames; D[k][f] = rfft of the hann-windowed samples [f hop - n_fft / 2, ... + n_fft), zeros outside [0, L);
 * D[:, T] = D[:, T + 1] = 0.
 * Stretch: T' = ceil(T o / n) output frames; frame s: q = s n, j = q / o, alpha = (q % o) / o (no float time axis, so no drift);
 * mag = (1 - alpha) |D[k][j]| + alpha |D[k][j + 1]|.  The phase is held in turns in unsigned 32-bit fixed point:
 * Theta[k][f] = uint32(llrint(atan2(Im, Re) / (2 pi) * 2^32)) (0 where D = 0), Phi[k][s] = Theta[k][0] + sum_{u < s} (Theta[k][j_u + 1] -
 * Theta[k][j_u]) in wrapping arithmetic — the wrap is the modulo 2 pi, and librosa's phi_advance and its wrap cancel out of e^{i Phi}.  An fp32
 * accumulator holds ~1e6 rad after 200 000 samples and is off by 0.12 of peak; this form stays within 2e-6.  Integer addition is associative:
 * the scan gives the same bits whatever its decomposition.  S[k][s] = mag (cos, sin)(2 pi Phi / 2^32).
 * Synthesis: irfft(S[:, s]) times the window, overlap-added, divided by the overlap-added window^2 where that is positive, n_fft / 2 samples
 * cropped from the front, cut or zero-padded to Ls = (2 L o + n) / (2 n) (round(L o / n), halves up).
 * Resample: orig_freq -> sr with fv_resample_design's filter (table in global memory): ceil(n Ls / o) samples, cut or zero-padded to L.
 * The streaming form (fv_pv_stream_*) and the per-session pool (fv_pvpool_*) follow the whole-row entries.  Not built: ragged rows in one call,
 * a chunk-parallel scan for very long single rows, a per-session n_steps, the command line's --pitch-shift with --sessions / --chunk-frames. */
typedef struct fv_pitch_shift_config {
    int32_t sample_rate;           /* sr of test.py:61-62 */
    double n_steps;                /* cfg.pitch_shift (configs/train.yaml), in steps of an octave / bins_per_octave */
    int32_t bins_per_octave;       /* librosa's default 12 */
    int32_t n_fft;                 /* librosa's default 2048 */
    int32_t hop_length;            /* 0: n_fft / 4 (librosa's default) */
    int32_t freq_granularity;      /* 100 in hq_pitch_shift.py:31; 1 keeps orig_freq as rounded */
    int32_t lowpass_filter_width;  /* 64 with the values below: torchaudio's documented equivalent of librosa's kaiser_best */
    double rolloff;                /* 0.9475937167399596 */
    int32_t method;                /* fv_resample_method; FV_RESAMPLE_SINC_KAISER */
    double beta;                   /* 14.769656459379492; <= 0: that default */
} fv_pitch_shift_config;

/* Pure host (no GPU): the plan of test.py:61-62's pitch shift.  FV_ERR_INVALID names the offending field. */
FV_API fv_status fv_pitch_shift_plan(const fv_pitch_shift_config* cfg, int32_t* orig_freq, int32_t* o, int32_t* n);
/* Pure host: for L input samples (test.py:61-62's gt_y), T analysis frames, T' stretched frames, Ls stretched samples and ceil(n Ls / o) resampled
 * samples (before the cut / padding to L).  NULL outputs are skipped. */
FV_API fv_status fv_pitch_shift_lengths(const fv_pitch_shift_config* cfg, int64_t L, int64_t* frames, int64_t* frames_out, int64_t* stretched,
                                        int64_t* resampled);

typedef struct fv_pitch_shift fv_pitch_shift;

/* Builds the DFT bases, the window envelope and the resampler's table on the current HIP device (test.py:61-62 builds nothing: librosa
 * recomputes per call).  n_fft must be a multiple of hop_length and both even, else FV_ERR_UNSUPPORTED naming the values. */
FV_API fv_status fv_pitch_shift_create(const fv_pitch_shift_config* cfg, fv_pitch_shift** out);
FV_API void fv_pitch_shift_destroy(fv_pitch_shift* p);
/* Bytes of device scratch fv_pitch_shift_stretch / fv_pitch_shift_forward need for `batch` rows of L samples (test.py:61-62 allocates per
 * call); 0 for a bad argument. */
FV_API size_t fv_pitch_shift_workspace_bytes(const fv_pitch_shift* p, int32_t batch, int64_t L);
/* librosa.effects.time_stretch(rate = n / o), the first half of test.py:61-62: d_x `batch` rows of L samples (row b at d_x + b * x_row_stride),
 * d_y `batch` rows of Ls (fv_pitch_shift_lengths) samples.  d_y must not overlap d_x.  Asynchronous on `stream`. */
FV_API fv_status fv_pitch_shift_stretch(fv_pitch_shift* p, const float* d_x, int64_t x_row_stride, float* d_y, int64_t y_row_stride,
                                        int32_t batch, int64_t L, void* d_workspace, size_t workspace_bytes, void* stream);
/* The whole of test.py:61-62: d_y `batch` rows of L samples.  Rows are the flattened leading dimensions (stereo: two rows, test.py:56-64).
 * d_y must not overlap d_x (FV_ERR_INVALID).  Asynchronous on `stream`. */
FV_API fv_status fv_pitch_shift_forward(fv_pitch_shift* p, const float* d_x, int64_t x_row_stride, float* d_y, int64_t y_row_stride,
                                        int32_t batch, int64_t L, void* d_workspace, size_t workspace_bytes, void* stream);

/* -------- streaming pitch shift: test.py:61-62 chunk by chunk (no reference counterpart: librosa shifts whole files).  `batch` rows advance in
 *          lockstep, as in fv_resample_stream_*.  (Named fv_pv_*, outside the fv_pitch_shift_ prefix: that family's list of entries is pinned
 *          by its host test.)  --------
 *
 * The rule, in integers (F = n_fft, h = hop_length, rate n / o, N samples received per row):
 *   A(N) = 0 if N < F / 2, else (N - F / 2) / h + 1        analysis frames that read no sample at or after N (frame f reads [f h - F/2, f h + F/2))
 *   S(A) = 0 if A < 2, else ceil((A - 1) o / n)            stretched frames whose columns j = floor(s n / o) and j + 1 are both analysed
 *   Y    = min(max(0, S h - F / 2), Ls(N))                 stretched samples under which every covering frame exists; Ls(N) = (2 N o + n) / (2 n)
 *   E    = min(M(Y), N)                                    M: what fv_resample_stream_push has emitted after Y input samples (orig_freq -> sr)
 * A push sets N += c and emits the outputs [E, E(N)).  The flush, with L = N now known, analyses the frames [A, T) against zeros, takes the
 * columns T and T + 1 as zero, synthesises the frames [S, T'), emits the stretched samples up to Ls(L), flushes the resampler, cuts at
 * min(ceil(n Ls / o), L) and writes zeros up to L: after it E = L exactly.  Pushes are then refused (FV_ERR_STATE) until fv_pv_stream_reset.  A
 * flush at N = 0 emits nothing.  A refused call changes nothing.  The min with Ls(N) keeps a push from emitting a stretched sample that the cut
 * to Ls(L) would drop; it binds only when hop_length == n_fft.  The min with N never binds for lowpass_filter_width >= 1 (a push that would need
 * it is refused as an internal error, before anything is enqueued).  orig_freq == sr: a push emits its own c samples bit for bit, the flush nothing.
 * Latency: N - E is about F / 2 (the analysis frame's centre) + h (column j + 1) + (F / 2 + the resampler's half band, lowpass_filter_width *
 * o / (min(o, n) rolloff) stretched samples) * n / o input samples — 2460 samples (56 ms) at 44100 Hz / 2048 / 512 and n_steps = 3, 2910
 * (66 ms) at n_steps = -4; N - E <= F / 2 + h + ceil((F / 2 + D) n / o) with D = max_p(first[p] + count[p] - width - p o / n) of the resampler's
 * design.  The counts are host arithmetic (vocoder_amd.pitch_shift.stream_ready): no call synchronises.
 * Bits: the stream enqueues its two DFT convs in batch-invariant mode (every column one fixed-order sum, as fv_logmel_stream_* does), the scan
 * resumes from a carried uint32 total, the overlap-add sums a sample's frames in the whole-row order, and the resampler's stream is
 * bit-identical to its rows.  So the concatenated output of any chunking is bit-identical to fv_pitch_shift_forward over the whole rows after
 * fv_pv_set_batch_invariant(p, 1), and within the pitch shift's parity bar of it otherwise (the whole-row call may then pick split-K convs). */
typedef struct fv_pv_stream fv_pv_stream;

/* Pure host (no GPU): A(N), S(A(N)) and Y of the rule above for test.py:61-62's shift taken chunk by chunk.  NULL outputs are skipped;
 * FV_ERR_INVALID names the offending field, N must lie in [0, 2^30]. */
FV_API fv_status fv_pv_stream_ready(const fv_pitch_shift_config* cfg, int64_t N, int64_t* frames, int64_t* stretched_frames,
                                    int64_t* stretched_samples);
/* 1: fv_pitch_shift_stretch / fv_pitch_shift_forward (test.py:61-62) enqueue their two DFT convs in batch-invariant mode, as the stream always
 * does — the mode in which whole rows and streams agree bit for bit.  0 (the default): those calls keep the kernels and the bits they had. */
FV_API fv_status fv_pv_set_batch_invariant(fv_pitch_shift* p, int32_t enable);
/* All of the stream's device state is allocated here (test.py:61-62 keeps none) and freed by fv_pv_stream_destroy, every carry as a pair of
 * buffers used in turn so that no launch reads and writes one buffer: the last n_fft samples (batch, n_fft); |D| and Theta of the last analysed
 * column and the phase total Phi as uint32, (batch, n_fft / 2 + 1) each; the last n_fft / hop synthesised frames (batch, n_fft, n_fft / hop) —
 * one more than the overlap needs, for the pushes at which Ls(N) binds; and an fv_resample_stream on the shifter's own resampler.
 * max_chunk: the largest c of one push. */
FV_API fv_status fv_pv_stream_create(fv_pitch_shift* p, int32_t batch, int32_t max_chunk, fv_pv_stream** out);
/* Bytes of device scratch every push / flush of the stream needs (256-byte aligned; test.py:61-62 allocates per call); 0 for NULL. */
FV_API size_t fv_pv_stream_workspace_bytes(const fv_pv_stream* s);
/* N - E: the samples received and not yet emitted (what test.py:61-62 would still hold of the file); the flush emits exactly these. */
FV_API int64_t fv_pv_stream_pending(const fv_pv_stream* s);
/* d_x: (batch, c) with row stride x_row_stride, c <= max_chunk (else FV_ERR_INVALID) — the next samples of test.py:61-62's gt_y; d_y:
 * (batch, k) with row stride y_row_stride, k = E(N + c) - E known before the call and possibly 0, then d_y may be NULL.  *emitted receives k.
 * c = 0 is a no-op.  Asynchronous on `stream`; calls on one stream object must be ordered. */
FV_API fv_status fv_pv_stream_push(fv_pv_stream* s, const float* d_x, int64_t x_row_stride, int32_t c, float* d_y, int64_t y_row_stride,
                                   int64_t* emitted, void* d_workspace, size_t workspace_bytes, void* stream);
/* Emits the outputs [E, N): the end of test.py:61-62's file, zeros where the resampled row is shorter than the input. */
FV_API fv_status fv_pv_stream_flush(fv_pv_stream* s, float* d_y, int64_t y_row_stride, int64_t* emitted, void* d_workspace,
                                    size_t workspace_bytes, void* stream);
/* N = E = 0 for the next utterance (the next file of test.py:61-62); the buffers are kept. */
FV_API fv_status fv_pv_stream_reset(fv_pv_stream* s);
/* Call it before fv_pitch_shift_destroy of its shifter, once the stream's work has finished (test.py:61-62 has nothing to free). */
FV_API void fv_pv_stream_destroy(fv_pv_stream* s);

/* -------- pitch shift, per session: test.py:61-62 for a pool of sessions that advance independently — what fv_respool_* is to
 *          fv_resample_stream_*, for fv_pv_stream_*.  No reference counterpart: librosa shifts whole files and keeps no state.  (Named
 *          fv_pvpool_*, outside the fv_pv_ and fv_pitch_shift_ prefixes: those families' lists of entries are pinned by their host tests.)
 *          --------
 *
 * One pool is one fv_pitch_shift: one n_steps, so one rate n / o and one resampler table for all S slots.  Each slot has its own N and E, its
 * flushed flag, its n_fft carried samples, the polar carry (|D| and Theta of column A - 1, Phi after the frames [0, S)) and the last
 * n_fft / hop synthesised frames.  All three carries are pairs of buffers with one bit per slot; a bit flips only when the step's launch wrote
 * that slot's other half: samples > 0 for the sample carry, dA > 0 or dS > 0 for the polar pair, dS > 0 for the frames.  A, S, Y and the
 * resampler's count follow from N alone (fv_pv_stream_ready).  A step is a list of fv_wavpool_item (session, samples, flush); per item
 *   N' = N + samples;  E' = flush ? N' : max(E, min(M(Y(N')), N'));  the item emits the outputs [E, E').
 * A flush at N' = 0 emits nothing; a flushed slot refuses items (FV_ERR_STATE) until fv_pvpool_reset; an utterance holds at most 2^30 samples.
 * The whole step — the pool's plan, the inner resample pool's, every check of the output and the workspace — is made on the host before
 * anything is enqueued or any counter moves: a refused step leaves every slot as it was.  The items that have work form the rows of one set of
 * tensors: one window launch, the STFT conv over (rows, largest dA), the polar and scan launches, the inverse-DFT conv over (rows, largest dS),
 * the overlap-add, the frame carry, one step of an inner fv_respool on the shifter's resampler, the sample carry and one crop into the
 * caller's rows, each launch serving 32 rows; a row's columns past its own dA / dS are written as zeros.  Both convs run in batch-invariant
 * mode, so a session's concatenated outputs are bit-identical to fv_pitch_shift_forward over its whole utterance after
 * fv_pv_set_batch_invariant(p, 1) and to an fv_pv_stream fed the same chunks, whatever the other sessions do.  orig_freq == sr: every item's
 * samples come back bit for bit and nothing is carried.  Not built: a per-session n_steps (it needs a per-slot rate and resampler table). */
typedef struct fv_pvpool fv_pvpool;

/* All device state of the pool is allocated here on the current HIP device (test.py:61-62 keeps none) and freed by fv_pvpool_destroy: the three
 * pairs of carries and an fv_respool on the shifter's resampler.  sessions outside [1, 65535] or max_chunk outside [1, 2^28]: FV_ERR_INVALID; a
 * max_chunk whose one step passes 2^31 elements per row: FV_ERR_UNSUPPORTED. */
FV_API fv_status fv_pvpool_create(fv_pitch_shift* p, int32_t sessions, int32_t max_chunk, fv_pvpool** out);
/* Bytes of device scratch a step of up to `sessions` items needs (256-byte aligned; test.py:61-62 allocates per call); 0 for NULL and for the
 * identity shift. */
FV_API size_t fv_pvpool_workspace_bytes(const fv_pvpool* p);
/* The most one item can emit in one step (test.py:61-62's file length never enters): a push of max_chunk samples that also flushes, from any
 * state.  Such a step emits N + max_chunk - E(N), and N - E(N) grows by one per sample and falls only where A(N) steps, at N = F / 2 + a h: its
 * largest value stands at some N_a = F / 2 + a h - 1.  Moving a by n moves S by o, Y by o h, the resampler's count by n h and N by n h, so past
 * the start-up N_a - E(N_a) has period n in a; in the start-up every clamp (A, S, Y and the resampler's count at 0) only raises E.  The result
 * is max_chunk + the largest N_a - E(N_a) over n consecutive a past the start-up.  Exact: some state attains it.  The per-step sizes inside
 * the pool (fv_pvpool_bounds) cover the same step and are upper estimates.  An out_cols of this size serves every step.  0 for NULL. */
FV_API int64_t fv_pvpool_max_outputs(const fv_pvpool* p);
/* N of one slot: the samples of the current utterance (test.py:61-62's gt_y) received so far; 0 for a session outside [0, S). */
FV_API int64_t fv_pvpool_received(const fv_pvpool* p, int32_t session);
/* E of one slot: the shifted samples (what test.py:61-62 returns) emitted so far; 0 for a session outside [0, S). */
FV_API int64_t fv_pvpool_emitted(const fv_pvpool* p, int32_t session);
/* N - E of one slot: what its flush would emit now (the rest of test.py:61-62's file); 0 for a session outside [0, S). */
FV_API int64_t fv_pvpool_pending(const fv_pvpool* p, int32_t session);
/* Pure host (no GPU): the sizes a pool of this config and max_chunk is built with (test.py:61-62 sizes nothing), five entries: the most
 * analysis frames, stretched frames and stretched samples one item makes ready in one step, the most its resampler emits, and
 * fv_pvpool_max_outputs.  The first four are upper estimates: (max_chunk + F / 2) / h + 2; ceil((maxA + 1) o / n) + 2;
 * max(maxS h + F, ceil(max_chunk o / n) + 2); fv_respool_max_outputs of a pool of maxY.  Zeros but the last for the identity shift. */
FV_API fv_status fv_pvpool_bounds(const fv_pitch_shift_config* cfg, int32_t max_chunk, int64_t* bounds);
/* Pure host, as fv_respool_plan is: what a step would emit, from the config alone (what test.py:61-62 leaves to librosa).  received / emitted
 * / flushed: the S counters and flags (flushed may be NULL: none is).  Writes E' - E of every item to outputs_out (count entries) and returns
 * the largest; nothing is changed.  Refuses what fv_pvpool_step refuses of the items, each named in fv_last_error, with the status as the
 * (negative) result: those of fv_respool_plan, in its order, then more than 2^30 samples in one utterance, then an item that passes the
 * pool's own bounds or counters that no sequence of steps gives (FV_ERR_INVALID, "internal"). */
FV_API int64_t fv_pvpool_plan(const fv_pitch_shift_config* cfg, int32_t sessions, int32_t max_chunk, const int64_t* received,
                              const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                              int64_t* outputs_out);
/* One step (replaces one test.py:61-62 call per file, for sessions whose audio arrives at different times).  d_chunks, d_out, out_stride,
 * out_cols and outputs_out as in fv_respool_step: the first out_cols columns of row i receive item i's outputs and exactly 0.0f after them,
 * every one of them is written.  d_workspace: fv_pvpool_workspace_bytes.  Refusals, for the whole step before anything moves, each naming the
 * item and the session: those of the items in fv_respool_plan's order, a NULL chunk buffer although an item has samples, chunk_stride shorter
 * than the longest chunk; then the pool's own of fv_pvpool_plan; then out_cols below the largest E' - E, out_stride < out_cols, a NULL d_out
 * although an item emits; then a workspace that is NULL or too small although an item has work.  No device allocation, no host synchronisation.  Asynchronous on `stream`; steps of one pool must be ordered. */
FV_API fv_status fv_pvpool_step(fv_pvpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                float* d_out, int64_t out_stride, int32_t out_cols, int64_t* outputs_out, void* d_workspace,
                                size_t workspace_bytes, void* stream);
/* N = E = 0 and not flushed for one slot, and the same for its slot of the inner resample pool: the next file of test.py:61-62.  The carries
 * are kept: what lies before sample, column and frame 0 is zero by index.  A session outside [0, S): FV_ERR_INVALID. */
FV_API fv_status fv_pvpool_reset(fv_pvpool* p, int32_t session);
/* Call it before fv_pitch_shift_destroy of its shifter, once the pool's work has finished (test.py:61-62 has nothing to free). */
FV_API void fv_pvpool_destroy(fv_pvpool* p);

/* -------- pitch template: the `template (B, 1, T * hop)` that refinegan.py:287 / hifigan.py:226 take next to the mel.  The reference does not
 *          make one: its users bring an F0 track from a CPU tracker (pyworld, parselmouth, librosa.yin) and synthesise the template from it.
 *          Both steps are here: a YIN tracker and an exact-phase oscillator driven by its F0.  --------
 *
 * Plan (integers): tau_max = sr / fmin, tau_min = max(2, sr / fmax) (floors), Wi = W - (tau_max + 1) the integration window, the same for
 * every lag; T = L / hop frames, one per mel frame.
 * Framing: frame t is centred on sample c = t hop + hop / 2 (the centre of mel frame t under the log-mel front-end's framing) and covers
 * [c - W / 2, c + W / 2); samples before 0 or at or past the row's length are zeros and are never loaded (a ragged row's padding may hold NaN).
 * Difference function, direct form: d(tau) = sum_{j < Wi} (x[j] - x[j + tau])^2 for tau = 1 ... tau_max + 1, one fp32 accumulator over
 * ascending j (not E(0) + E(tau) - 2 r(tau): that cancels where d is small, the voiced case).
 * Normalisation: d'(tau) = d(tau) tau / sum_{k <= tau} d(k); 1 where the running sum is 0 (silence stays finite and unvoiced).
 * Decision: the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, d'(tau) <= d'(tau - 1) and d'(tau) < d'(tau + 1): voiced,
 * delta = (a - c) / (2 (a - 2 b + c)) on d'(tau - 1, tau, tau + 1) (0 when the denominator is <= 0), f0 = sr / (tau + delta),
 * aperiodicity = d'(tau).  None: unvoiced, f0 = 0, aperiodicity = min d' over the range.
 * Template: F_t = rint(f0_t / sr * 2^32) in double, held as uint32, 0 (unvoiced) unless 0 < f0_t < sr.  Sample n lies between the frame
 * centres a = floor((n - hop / 2) / hop) and a + 1, both clamped to the row's frames, k in [0, hop) samples past centre a:
 * inc[n] = (F_a (hop - k) + F_b k) / hop in 64-bit integers, an unvoiced neighbour taking the other one's value; the phase
 * phi[n] = sum_{m <= n} inc[m] mod 2^32 is an integer prefix sum, exact in any order (an fp32 accumulator drifts audibly within seconds).
 * Output amplitude sin(2 pi phi / 2^32) or amplitude (2 phi / 2^32 - 1), exactly 0 where frame n / hop is unvoiced.
 * The streaming form (fv_yin_stream_*, fv_osc_stream_*) and the pool form (fv_yinpool_*, fv_oscpool_*) follow the whole-row entries.  Not
 * built: pYIN / Viterbi smoothing, octave-error correction. */
typedef struct fv_f0_config {
    int32_t sample_rate;   /* the model's rate: the tracker runs on the samples the mel is made from */
    int32_t frame_length;  /* W, even; 2048 */
    int32_t hop_length;    /* the model's hop: one F0 value per mel frame */
    double fmin;           /* 40 Hz */
    double fmax;           /* 1100 Hz */
    double threshold;      /* in (0, 1]; 0.1 */
} fv_f0_config;

typedef enum fv_template_kind { FV_TEMPLATE_SINE = 0, FV_TEMPLATE_SAWTOOTH = 1 } fv_template_kind;

typedef struct fv_template_config {
    int32_t sample_rate;
    int32_t hop_length;
    int32_t kind;      /* fv_template_kind */
    float amplitude;   /* 1.0 */
} fv_template_config;

/* Pure host (no GPU): the plan of the tracker that stands in for the CPU F0 tracker in front of refinegan.py:287 / hifigan.py:226, and the
 * frames of a row of L samples.  NULL outputs are skipped.  FV_ERR_INVALID says which knob to move: tau_min >= tau_max (fmin, fmax),
 * Wi < tau_max / 2 (frame_length or fmin), an odd frame_length, hop_length < 1, threshold outside (0, 1]. */
FV_API fv_status fv_f0_plan(const fv_f0_config* cfg, int64_t L, int32_t* tau_min, int32_t* tau_max, int32_t* window, int64_t* frames);

typedef struct fv_f0 fv_f0;
typedef struct fv_template fv_template;

/* The tracker (replaces the CPU F0 tracker a user of refinegan.py:287 / hifigan.py:226 runs today).  FV_ERR_UNSUPPORTED for a frame_length
 * above 4096: one workgroup stages the frame in LDS. */
FV_API fv_status fv_f0_create(const fv_f0_config* cfg, fv_f0** out);
FV_API void fv_f0_destroy(fv_f0* p);
/* Bytes of device scratch fv_f0_forward needs (the CPU trackers in front of refinegan.py:287 / hifigan.py:226 allocate per call): 0 today,
 * every frame lives in its workgroup's LDS; callers pass what this returns. */
FV_API size_t fv_f0_workspace_bytes(const fv_f0* p, int32_t batch, int64_t L);
/* F0 and aperiodicity per mel frame, the input of fv_template_forward (refinegan.py:287 / hifigan.py:226 take its output).  d_x: `batch` rows
 * of L samples, row b at d_x + b * x_row_stride; host_lengths (NULL: every row has L): row b holds host_lengths[b] <= L samples, the rest is
 * never loaded.  d_f0 / d_aperiodicity: `batch` rows of T = L / hop values, row b at + b * out_row_stride; frames at or past
 * host_lengths[b] / hop are exact zeros in both.  A row's values are bit-identical alone, in any batch and at any L.  Everything is validated
 * before anything is enqueued.  Asynchronous on `stream`. */
FV_API fv_status fv_f0_forward(fv_f0* p, const float* d_x, int64_t x_row_stride, const int32_t* host_lengths, float* d_f0,
                               float* d_aperiodicity, int64_t out_row_stride, int32_t batch, int64_t L, void* d_workspace,
                               size_t workspace_bytes, void* stream);

/* The synthesiser of the template refinegan.py:287 / hifigan.py:226 take (replaces the CPU oscillator their users write).  FV_ERR_INVALID
 * names the field. */
FV_API fv_status fv_template_create(const fv_template_config* cfg, fv_template** out);
FV_API void fv_template_destroy(fv_template* p);
/* Bytes of device scratch fv_template_forward needs for `batch` rows of T frames (F and the chunk sums; a CPU oscillator in front of
 * refinegan.py:287 / hifigan.py:226 allocates per call); 0 for a bad argument. */
FV_API size_t fv_template_workspace_bytes(const fv_template* p, int32_t batch, int64_t T);
/* The template of refinegan.py:287 / hifigan.py:226 from frame-level F0.  d_f0: `batch` rows of T values in Hz (0, negative, NaN or >= sr:
 * unvoiced), row b at d_f0 + b * f0_row_stride; host_frames (NULL: every row has T): row b holds host_frames[b] <= T frames, the rest is
 * never loaded.  d_out: `batch` rows of T * hop samples, row b at d_out + b * out_row_stride, exact zeros from host_frames[b] * hop on.  A
 * row's samples are bit-identical alone, in any batch and at any T.  T * hop <= 2^30.  Asynchronous on `stream`. */
FV_API fv_status fv_template_forward(fv_template* p, const float* d_f0, int64_t f0_row_stride, const int32_t* host_frames, float* d_out,
                                     int64_t out_row_stride, int32_t batch, int64_t T, void* d_workspace, size_t workspace_bytes,
                                     void* stream);

/* Streaming form of both steps (no reference counterpart: the CPU trackers in front of refinegan.py:287 / hifigan.py:226 take whole files):
 * `batch` rows advance in lockstep, as in fv_resample_stream_* and fv_logmel_stream_*; what comes out feeds fv_stream_push's d_template.  (Named
 * outside the fv_f0_ / fv_template_ prefixes: those families' lists of entries are pinned by their host test.)
 *
 * Tracker stream.  Host counters: N samples received, E frames emitted.  Frame t reads the samples [t hop + hop / 2 - W / 2, ... + W) and
 * leaves once none of them is at or after N: ready(N) = 0 for N < hop / 2 + W / 2, else min(1 + (N - hop / 2 - W / 2) / hop, N / hop).  A
 * push sets N += c and emits the frames [E, ready(N)); the flush emits [E, N / hop) against the rows' true end (samples at or past N are
 * zeros by index, as fv_f0_forward treats a row's length) and then refuses pushes (FV_ERR_STATE) until the reset.  Latency: a frame leaves
 * W / 2 + hop / 2 - hop samples after its own hop has arrived — 768 samples, 17 ms, at 44100 Hz / W 2048 / hop 512, the log-mel stream's own
 * figure.  A YIN frame's bits depend on the plan alone, so the concatenated values are bit-identical to fv_f0_forward over the whole rows.
 *
 * Oscillator stream.  Host counters: Tn F0 frames received, E frames emitted, each `hop` samples.  The samples of frame t interpolate between
 * the frame centres t - 1, t and t + 1: a push sets Tn += c and emits the samples of the frames [E, max(E, Tn - 1)); the flush emits [E, Tn)
 * with the last centre clamped to Tn - 1, as fv_template_forward clamps to the row's last frame.  Latency: one F0 frame.  The phase at the start
 * of frame E is carried on the device as a wrapping uint32; integer addition is exact in any order, so the concatenated samples are
 * bit-identical to fv_template_forward over the whole rows.
 *
 * Every call validates everything before it enqueues anything, enqueues eagerly on `stream` and never synchronises; a refused call changes
 * nothing.  Sessions that do not advance in lockstep — what fv_pool_step's d_templates needs — have the pool form below (fv_yinpool_*,
 * fv_oscpool_*). */
typedef struct fv_yin_stream fv_yin_stream;
typedef struct fv_osc_stream fv_osc_stream;

/* Pure host (no GPU): ready(N) above, the frames a tracker stream has emitted once N samples have arrived (the CPU trackers in front of
 * refinegan.py:287 / hifigan.py:226 see whole files only); never above N / hop.  -1: N < 0 or a configuration fv_f0_plan refuses. */
FV_API int64_t fv_yin_frames_ready(const fv_f0_config* cfg, int64_t N);

/* The stream's only device allocation (a CPU tracker in front of refinegan.py:287 / hifigan.py:226 keeps no state), freed by
 * fv_yin_stream_destroy: two (batch, H + max_chunk_samples) buffers used in turn that carry each row's last H = W / 2 + max(W / 2,
 * (hop + 1) / 2) samples (W when hop <= W) from push to push.  `p` must outlive the stream. */
FV_API fv_status fv_yin_stream_create(fv_f0* p, int32_t batch, int32_t max_chunk_samples, fv_yin_stream** out);
/* N - max(0, E hop + hop / 2 - W / 2), never negative: samples received that frames not yet emitted still read, fewer than H (what a CPU
 * tracker in front of refinegan.py:287 / hifigan.py:226 would hold as the file's tail). */
FV_API int64_t fv_yin_stream_pending_samples(const fv_yin_stream* s);
/* d_wave: (batch, c) with row stride row_stride, c <= max_chunk_samples (else FV_ERR_INVALID) — the next samples of what the tracker in front
 * of refinegan.py:287 / hifigan.py:226 is handed whole; d_f0 / d_aperiodicity: (batch, k) with row stride out_row_stride,
 * k = fv_yin_frames_ready(N + c) - E known before the call; k may be 0, then both may be NULL.  *frames_out receives k.  c = 0 is a no-op.
 * Asynchronous on `stream`; calls on one stream object must be ordered. */
FV_API fv_status fv_yin_stream_push(fv_yin_stream* s, const float* d_wave, int64_t row_stride, int32_t c, float* d_f0, float* d_aperiodicity,
                                    int64_t out_row_stride, int64_t* frames_out, void* stream);
/* Emits the frames [E, N / hop) against the utterance's end, the last values a whole-file tracker in front of refinegan.py:287 /
 * hifigan.py:226 returns; d_f0 / d_aperiodicity: (batch, N / hop - E).  A flush at N = 0 emits nothing. */
FV_API fv_status fv_yin_stream_flush(fv_yin_stream* s, float* d_f0, float* d_aperiodicity, int64_t out_row_stride, int64_t* frames_out,
                                     void* stream);
/* N = E = 0 for the next utterance (the next file of a tracker in front of refinegan.py:287 / hifigan.py:226); the buffers are kept, and
 * samples before 0 are zeros by index whatever they hold. */
FV_API fv_status fv_yin_stream_reset(fv_yin_stream* s);
/* Call it before fv_f0_destroy of its tracker, once the stream's work has finished (a CPU tracker in front of refinegan.py:287 /
 * hifigan.py:226 has nothing to free). */
FV_API void fv_yin_stream_destroy(fv_yin_stream* s);

/* The stream's only device allocations (a CPU oscillator in front of refinegan.py:287 / hifigan.py:226 keeps its phase in a host float), freed
 * by fv_osc_stream_destroy: two (batch, 2 + max_chunk_frames) buffers used in turn that carry the F0 of the frames [E - 1, Tn), the
 * increments and chunk sums of one call, and two (batch) uint32 phases used in turn.  (2 + max_chunk_frames) * hop <= 2^30.  `p` must outlive
 * the stream. */
FV_API fv_status fv_osc_stream_create(fv_template* p, int32_t batch, int32_t max_chunk_frames, fv_osc_stream** out);
/* Tn - E: F0 frames received whose samples have not left, 0 or 1 between calls (a CPU oscillator in front of refinegan.py:287 /
 * hifigan.py:226 waits for the whole track). */
FV_API int64_t fv_osc_stream_pending_frames(const fv_osc_stream* s);
/* d_f0: (batch, c) in Hz with row stride row_stride, c <= max_chunk_frames (else FV_ERR_INVALID) — the next frames of the track a user of
 * refinegan.py:287 / hifigan.py:226 brings whole; d_out: (batch, k hop) with row stride out_row_stride, k = max(E, Tn + c - 1) - E frames known
 * before the call; k may be 0, then d_out may be NULL.  *samples_out receives k hop.  c = 0 is a no-op.  Asynchronous on `stream`; calls on
 * one stream object must be ordered. */
FV_API fv_status fv_osc_stream_push(fv_osc_stream* s, const float* d_f0, int64_t row_stride, int32_t c, float* d_out, int64_t out_row_stride,
                                    int64_t* samples_out, void* stream);
/* Emits the samples of the frames [E, Tn), the end of the template refinegan.py:287 / hifigan.py:226 take; d_out: (batch, (Tn - E) hop). */
FV_API fv_status fv_osc_stream_flush(fv_osc_stream* s, float* d_out, int64_t out_row_stride, int64_t* samples_out, void* stream);
/* Tn = E = 0 for the next utterance (the next track of refinegan.py:287 / hifigan.py:226's user); the buffers are kept: the first call of an
 * utterance takes phase 0 by index, not from memory. */
FV_API fv_status fv_osc_stream_reset(fv_osc_stream* s);
/* Call it before fv_template_destroy of its synthesiser, once the stream's work has finished (refinegan.py:287 / hifigan.py:226's users free
 * nothing). */
FV_API void fv_osc_stream_destroy(fv_osc_stream* s);

/* Pool form of both steps: S sessions that advance independently, what fv_wavpool_* is to fv_logmel_stream_* and fv_respool_* to
 * fv_resample_stream_*, for fv_yin_stream_* and fv_osc_stream_* (no reference counterpart: the CPU trackers in front of refinegan.py:287 /
 * hifigan.py:226 take whole files).  What the two pools emit per session is what fv_pool_step takes as d_templates.  (Named fv_yinpool_* /
 * fv_oscpool_*, outside the fv_yin_ / fv_osc_ prefixes: those families' lists of entries are pinned by their host test.)
 *
 * Both pools hold S slots on the per-session carry core: each slot has its own counters, its own flushed flag and its own bit saying which of
 * two carry buffers holds its history.  A step is a list of fv_wavpool_item (session, samples, flush): any subset of the slots, each at most
 * once, each with its own chunk size; the stream's push and flush folded into one call.  With flush the slot then refuses items (FV_ERR_STATE)
 * until its reset.  The whole step is checked before any counter moves or anything is enqueued: a refused step leaves every slot as it was.
 * The items' table entries travel in the kernel arguments, 32 per launch.  The entries enqueue eagerly and never synchronise.
 *
 * Tracker pool.  Per slot N samples received, E frames emitted and the last H = W / 2 + max(W / 2, (hop + 1) / 2) samples, as the stream.
 *   N' = N + samples;  E' = flush ? N' / hop : max(E, ready(N'));  the item emits the frames [E, E')      (ready: fv_yin_frames_ready)
 * A flush at N' = 0 emits nothing.  One workgroup per (item, frame) stages the frame from the slot's carried samples and the item's chunk row —
 * samples before 0 and at or past N' are zeros by index and never loaded — and then runs the device code fv_f0_forward runs, so a session's
 * concatenated values are bit-identical to fv_f0_forward over its whole utterance, whatever the other sessions do.  One step is one tracker
 * launch and one carry launch per 32 items.
 *
 * Oscillator pool.  An item's `samples` counts F0 frames.  Per slot Tn frames received, E emitted, the F0 of the last two frames received (the
 * frames [E - 1, Tn) among them) and the phase at the start of frame E, a wrapping uint32 in one of two (S) arrays picked by a second bit of
 * the slot: an item that emits reads one and writes the other, so no launch reads and writes the same buffer of a slot.
 *   Tn' = Tn + samples;  E' = flush ? Tn' : max(E, Tn' - 1);  the item emits the samples of the frames [E, E'), hop each
 * The flush clamps the last centre to Tn' - 1, as fv_template_forward clamps to the row's last frame.  At E = 0 the phase is 0 by index, not
 * from memory: a slot's first utterance, a slot after its reset, a slot whose first push was one frame and emitted nothing.  A session's
 * concatenated samples are bit-identical to fv_template_forward over its whole track.  One step is three launches (increments, chunk sums,
 * samples) and one carry launch per 32 items, whatever the number of sessions. */
typedef struct fv_yinpool fv_yinpool;
typedef struct fv_oscpool fv_oscpool;

/* The tracker pool's only device allocation (a CPU tracker in front of refinegan.py:287 / hifigan.py:226 keeps no state), made on the current
 * HIP device and freed by fv_yinpool_destroy: two (S, H) carry buffers.  sessions outside [1, 65535] or max_chunk outside [1, 2^28]:
 * FV_ERR_INVALID.  `p` must outlive the pool. */
FV_API fv_status fv_yinpool_create(fv_f0* p, int32_t sessions, int32_t max_chunk, fv_yinpool** out);
/* The most frames one item can emit in one step (a whole-file tracker in front of refinegan.py:287 / hifigan.py:226 has no such bound): a push
 * of max_chunk samples that also flushes, the largest (N + max_chunk) / hop - ready(N) over one period of N.  Exact: some state attains it.
 * An out_cols of this size serves every step.  0 for a NULL pool. */
FV_API int64_t fv_yinpool_max_frames(const fv_yinpool* p);
/* N of one slot: the samples of the current utterance (the file of a tracker in front of refinegan.py:287 / hifigan.py:226) received so far;
 * 0 for a session outside [0, S). */
FV_API int64_t fv_yinpool_received(const fv_yinpool* p, int32_t session);
/* E of one slot: the frames (values of what a tracker in front of refinegan.py:287 / hifigan.py:226 returns) emitted so far; 0 for a session
 * outside [0, S). */
FV_API int64_t fv_yinpool_emitted(const fv_yinpool* p, int32_t session);
/* N - max(0, E hop + hop / 2 - W / 2) of one slot, never negative: samples received that frames not yet emitted still read (the file's tail
 * of a tracker in front of refinegan.py:287 / hifigan.py:226); 0 for a session outside [0, S). */
FV_API int64_t fv_yinpool_pending(const fv_yinpool* p, int32_t session);
/* Pure host (no GPU): what a step would emit (a whole-file tracker in front of refinegan.py:287 / hifigan.py:226 has nothing to plan).
 * received / emitted / flushed: the S counters and flags (flushed may be NULL: none is).  Writes E' - E of every item to frames_out (count
 * entries) and returns the largest of them; nothing is changed: the caller moves the counters.  Refuses what fv_yinpool_step refuses of the
 * items, each named in fv_last_error, with the status as the (negative) result: a session outside [0, S), a duplicate session, samples
 * outside [0, max_chunk], more than 2^40 samples (FV_ERR_INVALID); an item for a flushed session (FV_ERR_STATE); a config that fv_f0_plan
 * refuses, sessions outside [1, 65535] or max_chunk outside [1, 2^28]. */
FV_API int64_t fv_yinpool_plan(const fv_f0_config* cfg, int32_t sessions, int32_t max_chunk, const int64_t* received, const int64_t* emitted,
                               const int32_t* flushed, const fv_wavpool_item* items, int32_t count, int64_t* frames_out);
/* One step (replaces one run of the tracker in front of refinegan.py:287 / hifigan.py:226 per file, for sessions whose audio arrives at
 * different times).  d_chunks: (count, chunk_stride) fp32, row i holding item i's samples first — the rest of the row (NaN included) is never
 * loaded; NULL when no item has samples.  d_f0 / d_aperiodicity: (count, out_stride) fp32 with out_stride >= out_cols >= the largest E' - E
 * of the step (d_f0 NULL when out_cols is 0; d_aperiodicity may always be NULL: it is then not stored): the first out_cols columns of row i
 * receive item i's frames and exactly 0.0f after them, an item that emits nothing a row of zeros; every one of them is written.  frames_out
 * (may be NULL): count entries, E' - E of every item.  Refusals, checked for the whole step before anything moves, each naming the item and
 * the session: those of fv_yinpool_plan, a NULL chunk buffer although an item has samples, chunk_stride shorter than the longest chunk,
 * out_cols below the largest E' - E, out_stride < out_cols, a NULL d_f0 although an item emits (FV_ERR_INVALID).  No device allocation, no
 * copy, no host synchronisation.  Asynchronous on `stream`; steps of one pool must be ordered. */
FV_API fv_status fv_yinpool_step(fv_yinpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_f0, float* d_aperiodicity, int64_t out_stride, int32_t out_cols, int64_t* frames_out, void* stream);
/* N = E = 0 and not flushed for one slot: its next utterance (the next file of a tracker in front of refinegan.py:287 / hifigan.py:226).  The
 * carry is kept: samples before 0 are zeros by index, whatever it holds.  A session outside [0, S): FV_ERR_INVALID. */
FV_API fv_status fv_yinpool_reset(fv_yinpool* p, int32_t session);
/* Frees the carry (call it before fv_f0_destroy of its tracker, once the pool's work has finished); a CPU tracker in front of
 * refinegan.py:287 / hifigan.py:226 has nothing to free. */
FV_API void fv_yinpool_destroy(fv_yinpool* p);

/* The oscillator pool's device allocations (a CPU oscillator in front of refinegan.py:287 / hifigan.py:226 keeps its phase in a host float),
 * made on the current HIP device and freed by fv_oscpool_destroy: two (S, 2) carry buffers, the increments and chunk sums of one step — sized
 * for S items of 2 + max_chunk_frames frames — and two (S) uint32 phases.  (2 + max_chunk_frames) * hop <= 2^30; sessions outside [1, 65535]
 * or max_chunk_frames outside [1, 2^28]: FV_ERR_INVALID.  `p` must outlive the pool. */
FV_API fv_status fv_oscpool_create(fv_template* p, int32_t sessions, int32_t max_chunk_frames, fv_oscpool** out);
/* The most frames one item can emit in one step (refinegan.py:287 / hifigan.py:226 take the whole template at once): max_chunk_frames + 1, a
 * push of max_chunk_frames that also flushes while one frame waits.  An out_cols of hop times this serves every step.  0 for a NULL pool. */
FV_API int64_t fv_oscpool_max_frames(const fv_oscpool* p);
/* Tn of one slot: the F0 frames of the current utterance (the track a user of refinegan.py:287 / hifigan.py:226 brings whole) received so far;
 * 0 for a session outside [0, S). */
FV_API int64_t fv_oscpool_received(const fv_oscpool* p, int32_t session);
/* E of one slot: the frames whose samples (of the template refinegan.py:287 / hifigan.py:226 take) have been emitted; 0 for a session outside
 * [0, S). */
FV_API int64_t fv_oscpool_emitted(const fv_oscpool* p, int32_t session);
/* Tn - E of one slot: F0 frames received whose samples have not left, 0 or 1 between steps (a CPU oscillator in front of refinegan.py:287 /
 * hifigan.py:226 waits for the whole track); 0 for a session outside [0, S). */
FV_API int64_t fv_oscpool_pending(const fv_oscpool* p, int32_t session);
/* Pure host (no GPU), as fv_yinpool_plan: what a step would emit, in frames (a CPU oscillator in front of refinegan.py:287 / hifigan.py:226
 * has nothing to plan).  The items' `samples` count F0 frames.  Writes E' - E of every item to frames_out and returns the largest; refuses
 * what fv_oscpool_step refuses of the items, a config that fv_template_create refuses, sessions outside [1, 65535] or max_chunk_frames
 * outside [1, 2^28], with the status as the (negative) result. */
FV_API int64_t fv_oscpool_plan(const fv_template_config* cfg, int32_t sessions, int32_t max_chunk_frames, const int64_t* received,
                               const int64_t* emitted, const int32_t* flushed, const fv_wavpool_item* items, int32_t count,
                               int64_t* frames_out);
/* One step (the next pieces of the template refinegan.py:287 / hifigan.py:226 take, for sessions whose F0 arrives at different times).
 * d_chunks: (count, chunk_stride) fp32 in Hz (0, negative, NaN or >= sr: unvoiced), row i holding item i's frames first — the rest of the row
 * is never loaded; NULL when no item has frames; an fv_yinpool_step's d_f0 serves as it is.  d_out: (count, out_stride) fp32, out_stride >=
 * out_cols >= hop times the largest E' - E of the step, counted in samples (NULL when out_cols is 0): the first out_cols columns of row i
 * receive the (E' - E) hop samples of item i and exactly 0.0f after them; every one of them is written.  frames_out (may be NULL): E' - E of
 * every item, in frames.  Refusals as fv_yinpool_step's, the output's counted in samples.  No device allocation, no copy, no host
 * synchronisation.  Asynchronous on `stream`; steps of one pool must be ordered. */
FV_API fv_status fv_oscpool_step(fv_oscpool* p, const fv_wavpool_item* items, int32_t count, const float* d_chunks, int64_t chunk_stride,
                                 float* d_out, int64_t out_stride, int32_t out_cols, int64_t* frames_out, void* stream);
/* Tn = E = 0 and not flushed for one slot: its next utterance (the next track of refinegan.py:287 / hifigan.py:226's user).  The buffers are
 * kept: the first emission of an utterance takes phase 0 by index, not from memory.  A session outside [0, S): FV_ERR_INVALID. */
FV_API fv_status fv_oscpool_reset(fv_oscpool* p, int32_t session);
/* Call it before fv_template_destroy of its synthesiser, once the pool's work has finished (refinegan.py:287 / hifigan.py:226's users free
 * nothing). */
FV_API void fv_oscpool_destroy(fv_oscpool* p);

/* -------- scoring generated audio: the distances eval.py and the STFT loss compute between a source and a generated waveform, as metrics.
 *          eval.py:29-33's spec_diff is mean |LogMelSpectrogram(target) - LogMelSpectrogram(preds)|; stft.py:55 is the spectral convergence
 *          ||y_mag - x_mag||_F / ||y_mag||_F and stft.py:74 the log-magnitude L1, mean |log y_mag - log x_mag|.  All three are ratios of the
 *          four sums below, taken per row over the valid columns of two spectrogram tensors.  eval.py's PESQ is not built (a standardised CPU
 *          algorithm).  Deviation for the STFT formulas: the callers feed this project's LinearSpectrogram magnitudes
 *          (win_length = n_fft, center=False, sqrt(re^2 + im^2 + 1e-6)), not stft.py:24-36's torch.stft(center=True, win_length < n_fft)
 *          with a clamp: the front-end config, frozen at ABI 5, has neither.  No gradients: a metric, not a loss. -------- */
#define FV_SPEC_DISTANCE_LOG 1 /* fv_spec_distance flags: also form S_log (positive magnitudes; leave it off for log-mels, which may be negative) */

/* Columns per tile of the reduction (eval.py:29-33 / stft.py:55,74 reduce whole tensors with torch.mean / torch.norm): a row's sums are its
 * tiles' partial sums added in tile order.  Exported for the tests' shapes, as fv_resample_input_tile is. */
FV_API int32_t fv_spec_distance_tile(void);
/* Bytes of device scratch fv_spec_distance needs for `batch` rows of T columns (the tiles' partial sums; eval.py:29-33 / stft.py:55,74
 * allocate theirs per call): 256-byte aligned, non-decreasing in both arguments, 0 for an empty or negative one. */
FV_API size_t fv_spec_distance_workspace_bytes(int32_t batch, int64_t T);
/* The sums behind eval.py:29-33 (spec_diff = S_l1 / count), stft.py:55 (sqrt(S_sq) / sqrt(S_ref)) and stft.py:74 (S_log / count) for rows of
 * different lengths in one call.  d_est / d_ref: fp32 (batch, channels, T); element (b, c, t) at b * row_stride + c * ld + t floats in both,
 * ld >= T, row_stride >= channels * ld — none of them, nor the base pointers, need be a multiple of 4 floats (a view x[:, :, 1:] is fine).
 * host_frames[b] <= T: the valid columns of row b.  d_out: (batch, 4) doubles per row,
 *   S_l1 = sum |est - ref|, S_sq = sum (est - ref)^2, S_ref = sum ref^2, S_log = sum |log ref - log est|     over c < channels, t < frames[b];
 * S_log only with FV_SPEC_DISTANCE_LOG in flags, otherwise exactly 0.0.  Every term is formed in fp32 with one rounding per operation
 * (d = est - ref, |d|, d * d, ref * ref, logf(ref) - logf(est); no clamp: non-positive inputs give what torch.log gives), widened to double
 * and accumulated in fp64 in a fixed order: no float atomics.  A row's four doubles are therefore bit-identical whether it is scored alone,
 * inside any batch, at any T >= frames[b], at any strides, and on every run.  Columns at or past frames[b] (NaN included) are never loaded;
 * a row with frames[b] = 0 gives four zeros.  count = channels * frames[b] is the caller's division (0 / 0 = NaN for an empty row).
 * Everything is validated before any device call: a null pointer, channels < 1, ld < T, row_stride < channels * ld, a frame count below 0 or
 * above T (the row is named), too little workspace -> FV_ERR_INVALID.  batch = 0 is a no-op.  Asynchronous on `stream`; never synchronises. */
FV_API fv_status fv_spec_distance(const float* d_est, const float* d_ref, int64_t row_stride, int64_t ld, int32_t channels, int64_t T,
                                  const int32_t* host_frames, int32_t batch, int32_t flags, double* d_out, void* d_workspace,
                                  size_t workspace_bytes, void* stream);

/* -------- single fused conv layer (the hot kernel on its own; used by the parity tests and the roofline
 *          bench).  Stands in for one weight-normed nn.Conv1d / nn.ConvTranspose1d call plus the elementwise
 *          ops the reference runs around it (F.silu before, residual add after: hifigan.py:101-108). -------- */
typedef struct fv_conv_desc {
    int32_t transposed; /* 0: Conv1d weight (C_out, C_in, k); 1: ConvTranspose1d weight (C_in, C_out, k) */
    int32_t c_in, c_out, kernel_size;
    int32_t dilation; /* Conv1d only */
    int32_t padding;  /* Conv1d: zero padding each side; ConvTranspose1d: `padding` argument */
    int32_t stride;   /* ConvTranspose1d only (Conv1d stride is always 1 on this path) */
    int32_t pre_act;  /* fv_act applied to the input (fused into the LDS staging) */
    int32_t post_act; /* fv_act applied after bias (+ residual) */
    float act_slope;
} fv_conv_desc;

typedef struct fv_conv fv_conv;

/* host_weight: already-folded weight in the torch layout named by `transposed`; host_bias may be NULL. */
FV_API fv_status fv_conv_create(const fv_conv_desc* desc, const float* host_weight, const float* host_bias, fv_conv** out);
FV_API int64_t fv_conv_output_length(const fv_conv* c, int32_t t_in);
/* y = post_act(conv(pre_act(x)) + bias [+ d_residual]); d_residual may be NULL or alias d_y. */
FV_API fv_status fv_conv_forward(fv_conv* c, const float* d_x, float* d_y, const float* d_residual, int32_t batch,
                          int32_t t_in, void* stream);
/* One ResBlock1 iteration in a single launch: y = x + c2(silu(c1(silu(x)))) (hifigan.py:102-107).  c1 is the dilated
 * conv, c2 the dilation-1 conv; both C -> C with the same odd kernel size and 'same' padding; exact-fp32 kernels for C in {16, 32},
 * k in {3, 7, 11} and (C, k) = (64, 3); split-fp16 kernels for C in {16, 32, 64, 128, 256} when both layers are set to FV_PRECISION_F16X3 (C = 16: even t and
 * 8-byte aligned tensors, otherwise the fp32 kernel runs);
 * dilation in {1, 3, 5} (else FV_ERR_UNSUPPORTED).  d_y must not alias d_x. */
FV_API fv_status fv_conv_pair_forward(fv_conv* c1, fv_conv* c2, const float* d_x, float* d_y, int32_t batch, int32_t t,
                                      void* stream);
/* The wide k = 3 pairs (C in {64, 128}, dilation in {1, 3, 5}) also have a Winograd F(4,3) quad-lattice kernel, "pair_wino4<k=3 d C>": 6 matrix
 * products per four outputs instead of F(2,3)'s 8.  An engine's pair branches take it on launches that fill the chip, outside batch-invariant mode;
 * fv_conv_pair_forward takes it only under FV_PAIR_WINO4=2 (FV_PAIR_WINO4=0: nobody does).  Host helpers, no GPU: the kernel's tile width in final
 * samples (0 for a shape it has no instance for), exported for the tests' shapes, and the weight packer — w: one layer's (c, c, 3) weights; returns the
 * packed size in floats (0: unsupported c) and fills out[0 .. size) when cap >= size.  Fragment order: float4 [(m_tile * c / 8 + chunk) * 6 + plane] * 64
 * + lane, component pp = U[32 m_tile + (lane & 31)][8 chunk + 2 pp + (lane >> 5)][plane], U = G w at the points 0, +1, -1, +2, -2, inf; then 8 zero
 * fragments. */
FV_API int32_t fv_pair_wino4_tile(int32_t c, int32_t dilation);
FV_API int64_t fv_pair_wino4_pack(const float* w, int32_t c, float* out, int64_t cap);
/* fv_precision for the following fv_conv_forward calls on this layer; layers the split-fp16 kernels do not cover
 * (transposed, C_in < 32, kernel size not in {3, 7, 11}) keep running in fp32. */
FV_API fv_status fv_conv_set_precision(fv_conv* c, int32_t precision);
/* fv_conv_algo for the following fv_conv_forward / fv_conv_pair_forward calls on this layer (for a pair: c1's setting). */
FV_API fv_status fv_conv_set_algorithm(fv_conv* c, int32_t algo);
FV_API void fv_conv_destroy(fv_conv* c);

/* -------- single helper ops (the kernels between the convs on their own; used by the parity tests) --------
 * All pointers are device pointers to contiguous float32 (batch, channels, T) tensors and per-channel vectors.  Everything is validated before
 * anything is enqueued: a NULL required pointer, channels < 1, batch < 0, T < 0 or past the launcher's 32-bit span, an even kernel_size, or
 * d_y overlapping an input (workgroups read their neighbours' halo) -> FV_ERR_INVALID with the argument named in fv_last_error, and nothing is
 * written.  batch = 0 or T = 0 is a no-op.  Asynchronous on `stream`; never synchronises.  fv_last_kernel names the form that ran.
 *
 * fv_aa_snake_forward: BigVGAN's Activation1d(SnakeBeta), y = down2(snake(up2(x))) with replicate padding at both rates (bigvgan.py:121-135,
 * 226-233).  d_alpha = exp(alpha) and d_inv_beta = 1 / (exp(beta) + 1e-9) per channel; d_up_taps / d_down_taps: 12 floats each.  d_x2 and d_x3
 * are both NULL or both set: the input is then ((x + x2) + x3) / 3.  Forms: "aa_snake<vec4>" (16-byte accesses: T % 4 == 0, T >= 8, d_x and
 * d_y 16-byte aligned, one operand, FV_AA_VEC4 not 0) or "aa_snake<pair>", the same bits; " sum3" follows with three operands.
 *
 * fv_dwconv_ln_forward: depthwise Conv1d(kernel_size, 'same' zero padding) + LayerNorm over channels (convnext.py:126-129); d_dw_weight is
 * (channels, kernel_size), d_dw_bias may be NULL.  d_dw_weight == NULL: the channels-first LayerNorm alone (convnext.py:71-74); kernel_size
 * must then be 1 and d_dw_bias NULL.  Forms: "dwconv_ln_tile<k=7 cmax=512 ng=16>" (LayerNorm alone, k = 1, and k = 7 up to 1024 channels;
 * cmax in {256, 512, 1024}, ng = 8 for cmax = 256 and under FV_DWLN_NG8), "dwconv_ln_reg<k=3>" (other k up to 1024 channels, every k under
 * FV_OLD_DWLN), "dwconv_ln<k=7>" (wider). */
FV_API fv_status fv_aa_snake_forward(const float* d_x, const float* d_x2, const float* d_x3, float* d_y, const float* d_alpha,
                                     const float* d_inv_beta, const float* d_up_taps, const float* d_down_taps, int32_t batch,
                                     int32_t channels, int64_t T, void* stream);
FV_API fv_status fv_dwconv_ln_forward(const float* d_x, const float* d_dw_weight, const float* d_dw_bias, const float* d_ln_weight,
                                      const float* d_ln_bias, float* d_y, int32_t batch, int32_t channels, int64_t T, int32_t kernel_size,
                                      float eps, void* stream);

/* -------- vector quantiser: VQ / residual VQ, encode and decode --------
 * The stage between generator.encoder and generator.decoder of VQVAEModel (vae.py:66-87: encodec's VectorQuantization for
 * num_quantizers == 1, ResidualVectorQuantization above) and the `vq` slot of UnifyGenerator (unify.py:21-53), inference arithmetic only
 * (no EMA, k-means init, dead-code expiry, straight-through or commitment loss; no project_in / project_out: codebook_dim == dim):
 *   search(x, embed) = argmax_j (x . e_j - h_j), h_j = |e_j|^2 / 2 formed in fp64 at load and rounded to fp32; the lowest index wins on
 *   equal scores, a NaN score never wins and a frame whose scores are all NaN takes code 0;
 *   r_0 = x, c_q = search(r_q, embed_q), r_{q+1} = r_q - e_{c_q}, z = ((e_{c_0} + e_{c_1}) + ...): fp32, one rounding per operation.
 * A frame's scores are formed in an order that depends on dim alone, so its codes and z have the same bits alone, in any batch, under
 * any chunking along T and any slice count (fv_vq_set_slices).
 * Limits: dim in [1, 4096], codebook_size in [1, 65536], num_quantizers in [1, 32]; batch in [0, 65535], batch * T at most 2^30 frames.
 * Every entry validates all a host can see before it enqueues anything, and names the offending field; encode and decode are
 * asynchronous on `stream`. */
typedef struct fv_vq_config {
    int32_t dim;            /* D: channels of a frame (vae.py:68 latent_size) */
    int32_t codebook_size;  /* K (vae.py:69) */
    int32_t num_quantizers; /* n_q (vae.py:70); 1 = VectorQuantization */
} fv_vq_config;

typedef struct fv_vq fv_vq;

/* vae.py:66-78: no device memory yet; FV_ERR_INVALID names the field outside its limits. */
FV_API fv_status fv_vq_create(const fv_vq_config* cfg, fv_vq** out);
FV_API void fv_vq_destroy(fv_vq* vq);
/* vae.py:66-78 (`layers.{layer}._codebook.embed`): host_embed (codebook_size, dim) row-major, copied (synchronously), packed into MFMA
 * fragment order and h formed.  May be called again to replace a layer's codebook once the device is idle. */
FV_API fv_status fv_vq_load_codebook(fv_vq* vq, int32_t layer, const float* host_embed);
/* Codebook slices of the search's grid: 0 (default) = by launch size.  Results do not depend on it; fv_vq_workspace_bytes does.
 * No reference counterpart (vae.py:82 is one torch call). */
FV_API fv_status fv_vq_set_slices(fv_vq* vq, int32_t slices);
/* Bytes of device scratch fv_vq_encode needs for (batch, T): the residual (num_quantizers > 1) and the per-slice partials (vae.py:82
 * allocates the N x K distance matrix instead).  0 for an invalid shape. */
FV_API size_t fv_vq_workspace_bytes(const fv_vq* vq, int32_t batch, int64_t T);
/* vae.py:82 / unify.py:21-23,39-41: d_x is a (batch, dim, T) activation, x_row_stride >= T the distance in floats between its channels
 * (batch rows are dim * x_row_stride apart: a slice along T of a contiguous tensor passes as it is).  host_frames: NULL, or `batch` frame
 * counts in [0, T]; frames at or past a row's count are never loaded, get code -1 and exact zeros in z.  d_codes: (num_quantizers,
 * batch, T) int32; d_z: NULL (codes only) or (batch, dim, T) contiguous.  2 * num_quantizers launches per 256 batch rows. */
FV_API fv_status fv_vq_encode(fv_vq* vq, const float* d_x, int64_t x_row_stride, const int32_t* host_frames, int32_t* d_codes, float* d_z,
                              int32_t batch, int64_t T, void* d_workspace, size_t workspace_bytes, void* stream);
/* unify.py:47 (vq.from_codes) / vae.py:87: d_codes (num_quantizers, batch, T) int32 -> d_z (batch, dim, T), the same layer-ordered sum.
 * A negative code contributes nothing (an all-negative frame is exact zeros), and so does one >= codebook_size, which the caller is
 * expected to have refused; frames at or past host_frames[b] are zeros. */
FV_API fv_status fv_vq_decode(fv_vq* vq, const int32_t* d_codes, const int32_t* host_frames, float* d_z, int32_t batch, int64_t T, void* stream);

/* -------- code streams and code session pools: the decode direction of a codec, served chunk by chunk.  No reference counterpart
 *          (vae.py:87 / unify.py:39-53 decode whole rows); replaces fv_vq_decode followed by fv_stream_push / fv_pool_step.  --------
 *
 * An fv_stream / fv_pool made by fv_stream_create_codes / fv_codepool_create keeps the CODES of its last cap = K + A + max_chunk_frames
 * frames, (rows, num_quantizers, cap) int32, instead of the (rows, C_in, cap) floats of its float twin: 4 n_q cap bytes per row instead of
 * 4 C_in cap.  The window-forming launch looks the codes up and forms fv_vq_decode's own layer-ordered sum (the first valid layer assigned,
 * one fp32 rounding per add, a code < 0 or >= codebook_size contributes nothing, a frame without a valid code is exact zeros), so the
 * window — and with it every emitted sample — has the bits of fv_vq_decode followed by the float entry point.  Everything else is the float
 * handle's: the emission rule, fv_pool_plan, the forward, the crop, the workspace and its size, the graph key, and "the whole call is
 * checked before anything moves".  The pitch-template ring of a use_template generator stays a float ring at the hop rate.
 *   - `vq` must outlive the handle: its codebooks are read at every push / step (not copied), so fv_vq_load_codebook on it changes what
 *     the frames already in the ring decode to.  Its dim must equal fv_input_channels(e) and every layer must be loaded.
 *   - flush, reset, destroy, workspace_bytes and pending_frames are the float handle's own entry points.  A code handle refuses
 *     fv_stream_push / fv_pool_step, and a float handle fv_stream_push_codes / fv_codepool_step, with FV_ERR_STATE and the name of the
 *     entry point to call instead; nothing moves.
 *   - creation refuses, by name: a NULL vq, a vq whose dim differs from the engine's input channels (FV_ERR_INVALID), a vq with an unloaded
 *     layer (FV_ERR_STATE), and the models fv_stream_create / fv_pool_create refuse, as they do.
 * The additions are additive: FV_ABI_VERSION does not change.  (The pool's entries are named fv_codepool_*, outside the fv_pool_ prefix: that
 * family's list of entries is pinned by its host test.  They take and make an fv_pool.) */
FV_API fv_status fv_stream_create_codes(fv_engine* e, const fv_vq* vq, const fv_stream_config* cfg, fv_stream** out);
/* fv_stream_push with d_codes (num_quantizers, batch, n) int32 in place of d_mel. */
FV_API fv_status fv_stream_push_codes(fv_stream* s, const int32_t* d_codes, const float* d_template, int32_t n, float* d_out,
                                      int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream);
FV_API fv_status fv_codepool_create(fv_engine* e, const fv_vq* vq, const fv_pool_config* cfg, fv_pool** out);
/* fv_pool_step with d_codes (num_quantizers, count, in_frames) int32 in place of d_chunks: item i's n frames first in row i of every layer
 * (the rest is never loaded). */
FV_API fv_status fv_codepool_step(fv_pool* p, const fv_pool_item* items, int32_t count, const int32_t* d_codes, const float* d_templates,
                                    int32_t in_frames, float* d_out, int32_t out_frames, int64_t* frames_out, void* d_workspace,
                                    size_t workspace_bytes, void* stream);
/* Device bytes of the handle's rings (the mel or code ring, plus the template ring of a use_template generator), for float and code handles
 * alike; 0 for NULL. */
FV_API size_t fv_stream_ring_bytes(const fv_stream* s);
FV_API size_t fv_codepool_ring_bytes(const fv_pool* p);

/* -------- posterior encoder: the WaveNet encoder of VITS / RVC (modules/encoders/posterior_encoder.py) --------
 * PosteriorEncoder in eval mode, the fourth encoder of the reference's modules/encoders package and one that VQVAEModel's generator.encoder
 * slot can take (vae.py:81).  With C = hidden_channels, k = kernel_size, m[b][t] = t < lengths[b], d_i = dilation_rate ** (i % dilation_cycle):
 *   h = pre(x) m;  out = 0
 *   layer i:  a = in_i(h)  (C -> 2C, k taps, dilation d_i, zero padding (k - 1) d_i / 2);  g = tanh(a[:C]) sigmoid(a[C:]);  r = rs_i(g)
 *             i < n_layers - 1 (rs_i: C -> 2C):  h = (h + r[:C]) m,  out = out + r[C:];   the last layer (rs_i: C -> C):  out = out + r
 *   y = proj(out m) m;  vqvae: z = y;  vae: mean, logvar = y[:out], clamp(y[out:], -30, 20), z = mean m;  bnvae: mean = BatchNorm1d_eval(mean)
 *   before z (the mean of a padded frame is BN(0), a per-channel constant; z is zero there).
 * Exact fp32 on v_mfma_f32_32x32x2_f32; weight norm (weight_g, weight_v) and the BatchNorm are folded in fp64 at finalize and rounded once.
 * `a` never reaches memory; the padding of x, and every frame at or past a row's length, is never loaded.  Every output element's sum is
 * formed in an order fixed by the layer's shape alone (8-channel chunk, tap, channel pair), so a row has the same bits alone, in any batch
 * and padded to any T.  Training-mode draws, dropout and f16x3 are not built: fp32 only.
 * Limits: hidden_channels in [1, 1024]; in_channels, out_channels in [1, 4096]; kernel_size odd in [1, 11]; n_layers in [1, 64];
 * dilation_rate >= 1, dilation_cycle >= 1 with (kernel_size - 1) * the largest dilation at most 896 frames (the staged window's LDS budget;
 * above: FV_ERR_UNSUPPORTED); batch in [0, 65535], batch * T at most 2^30 frames, lengths in [0, T].
 * Every entry validates all a host can see before it enqueues anything, and names the offending field. */
typedef struct fv_posterior_config {
    int32_t in_channels;     /* posterior_encoder.py:94 */
    int32_t out_channels;    /* :95 — proj has 2 * out_channels rows in the vae modes (:124-126) */
    int32_t hidden_channels; /* :96 */
    int32_t kernel_size;     /* :97, reference default 5 */
    int32_t dilation_rate;   /* :98, 1 */
    int32_t dilation_cycle;  /* :99, 1 */
    int32_t n_layers;        /* :100, 16 */
    int32_t mode;            /* :101 — 0 = "vqvae", 1 = "vae", 2 = "bnvae" */
} fv_posterior_config;

typedef struct fv_posterior fv_posterior;

/* posterior_encoder.py:92-131 (the constructor): validates on the host, no device work.  FV_ERR_INVALID / FV_ERR_UNSUPPORTED name the field. */
FV_API fv_status fv_posterior_create(const fv_posterior_config* cfg, fv_posterior** out);
/* `load_state_dict` on posterior_encoder.py:116-131,30-55: the reference's key names — pre.{weight,bias}, enc.in_layers.{i}.{bias,weight_g,
 * weight_v}, enc.res_skip_layers.{i}.{bias,weight_g,weight_v}, proj.{weight,bias} and, in bnvae mode, mu_bn.{weight,bias,running_mean,
 * running_var,num_batches_tracked} (the last is accepted, carries no eval arithmetic and is not required).  host: fp32, torch layout, copied.
 * An unknown key -> FV_ERR_INVALID, a wrong shape -> FV_ERR_SHAPE, both by name; after fv_posterior_finalize -> FV_ERR_STATE. */
FV_API fv_status fv_posterior_load_weight(fv_posterior* p, const char* name, const float* host, const int64_t* shape, int32_t ndim);
/* Strict load: FV_ERR_MISSING_WEIGHT names the first absent key (before any device work).  Folds g v / |v| per output channel
 * (posterior_encoder.py:44,54) and the BatchNorm (:129) in fp64, packs MFMA fragments with a gate pair's halves adjacent, uploads. */
FV_API fv_status fv_posterior_finalize(fv_posterior* p);
/* R = sum_i (kernel_size - 1) d_i / 2 (posterior_encoder.py:35-36): output frame t depends on the input frames [t - R, t + R] only. */
FV_API int32_t fv_posterior_reach_frames(const fv_posterior* p);
/* Rows of z (and of mean / logvar): out_channels (posterior_encoder.py:124-126,146). */
FV_API int32_t fv_posterior_output_channels(const fv_posterior* p);
/* Bytes of device scratch fv_posterior_forward needs: h, g and out of posterior_encoder.py:57-80, 3 * batch * hidden_channels * T floats.
 * 0 for an invalid shape (fv_last_error says which) and for batch = 0 or T = 0. */
FV_API size_t fv_posterior_workspace_bytes(const fv_posterior* p, int32_t batch, int64_t T);
/* posterior_encoder.py:133-160 in eval mode.  d_x: (batch, in_channels, T) fp32, x_row_stride >= T the distance in floats between its
 * channels (batch rows are in_channels * x_row_stride apart: a slice along T of a contiguous tensor passes as it is).  host_lengths: NULL
 * (every row holds T frames) or `batch` values in [0, T], read before the call returns.  d_z: (batch, out_channels, T), every element
 * written, exact zeros at and past a row's length.  d_mean / d_logvar: must be NULL in vqvae mode; in the vae modes each is NULL (not
 * wanted) or (batch, out_channels, T), where padded frames hold 0 — in bnvae mode the mean there is BN(0).  The fourth value of :157, the
 * mask, is lengths again and is not written.  2 * n_layers + 2 launches per 256 batch rows, whatever batch and T are; batch = 0 or T = 0 is
 * FV_OK and does nothing.  Asynchronous on `stream`. */
FV_API fv_status fv_posterior_forward(fv_posterior* p, const float* d_x, int64_t x_row_stride, const int32_t* host_lengths, float* d_z,
                                      float* d_mean, float* d_logvar, int32_t batch, int64_t T, void* d_workspace, size_t workspace_bytes,
                                      void* stream);
FV_API void fv_posterior_destroy(fv_posterior* p);

/* -------- posterior encoder, chunk by chunk (fv_wnstream_*) --------
 * `batch` rows advance in lockstep, as in fv_logmel_stream_* and fv_pv_stream_*.  With R = fv_posterior_reach_frames, N frames received and
 * E emitted: a push of c frames sets N += c, E' = max(E, N - R) and writes the latent frames [E, E'); the flush sets E' = N — the utterance
 * ends at N and zero padding follows it — and writes the rest, at most R frames.  After the flush pushes are refused (FV_ERR_STATE) until
 * fv_wnstream_reset.  The concatenated frames are BIT-identical to fv_posterior_forward over the whole utterance, under any chunking:
 * with p_i = (kernel_size - 1) d_i / 2, every layer keeps a ring of its input whose frontier lies p_0 + ... + p_{i-1} frames behind N, a
 * call runs each layer's gate and res / skip GEMM over the new columns only (the kernels are the whole-row body, addressed through the
 * rings), and an element's sum order is fixed by the layer's shape alone.  A ring position at or past a frontier is never read: the flush
 * stages zeros there.  A call enqueues at most 2 * n_layers + 2 launches, none when it has nothing to compute; it neither synchronises nor
 * allocates.  All device state is allocated by fv_wnstream_create:
 *   batch * hidden_channels * (sum_i pow2(2 p_i + S) + pow2(R + S) + S) floats, S = max(max_chunk, R), pow2 = the next power of two.
 * The stream reads the encoder's weights: destroy it before the encoder.  Every entry validates all a host can see before it enqueues
 * anything and names what it refuses; a refused call changes no counter. */
typedef struct fv_wnstream fv_wnstream;
/* p must be finalized (FV_ERR_STATE otherwise); batch in [1, 65535], max_chunk in [1, 2^20]. */
FV_API fv_status fv_wnstream_create(fv_posterior* p, int32_t batch, int32_t max_chunk, fv_wnstream** out);
/* d_x: frame t of channel ch of row b at d_x[b * x_batch_stride + ch * x_row_stride + t], x_row_stride >= c (a slice along T passes as it
 * is); c in [0, max_chunk], d_x may be NULL when c = 0.  d_z, d_mean, d_logvar: (batch, out_channels, y_row_stride) with
 * y_row_stride >= E' - E, frame E + j in column j; d_mean / d_logvar must be NULL in vqvae mode and may be NULL in the vae modes; d_z may
 * be NULL when the call emits nothing.  *emitted (may be NULL) receives E' - E.  At most 2^30 frames per utterance. */
FV_API fv_status fv_wnstream_push(fv_wnstream* s, const float* d_x, int64_t x_batch_stride, int64_t x_row_stride, int32_t c, float* d_z,
                                  float* d_mean, float* d_logvar, int64_t y_row_stride, int64_t* emitted, void* stream);
FV_API fv_status fv_wnstream_flush(fv_wnstream* s, float* d_z, float* d_mean, float* d_logvar, int64_t y_row_stride, int64_t* emitted,
                                   void* stream);
/* N = E = 0 for the next utterance; no device work (nothing a ring holds from the last one is read). */
FV_API fv_status fv_wnstream_reset(fv_wnstream* s);
/* N - E; -1 for NULL. */
FV_API int64_t fv_wnstream_pending(const fv_wnstream* s);
/* R; -1 for NULL. */
FV_API int32_t fv_wnstream_lookahead(const fv_wnstream* s);
FV_API void fv_wnstream_destroy(fv_wnstream* s);

/* -------- posterior encoder, sessions that advance independently (fv_wnpool_*) --------
 * What fv_wnstream_* is to rows in lockstep, for `sessions` slots with their own N, E and flushed flag, as fv_wavpool_* / fv_respool_* are to
 * their streams.  A step is a list of items (fv_wavpool_item: session, `samples` counting FRAMES here, flush: the utterance ends with these
 * frames), each session at most once.  Per item N' = N + frames and E' = flush ? N' : max(E, N' - R); the item emits the latent frames
 * [E, E').  A flush at N' = 0 emits nothing.  After its flush a slot refuses items (FV_ERR_STATE) until fv_wnpool_reset.  A session's
 * concatenated frames are BIT-identical to fv_posterior_forward over its whole utterance, whatever the other sessions do: the kernels are
 * the stream's (the whole-row body addressed through per-layer rings), with the column origin, the end and the frontier taken per item from
 * a by-value table of 128 entries, and a slot's state is its own row of every ring.  A step enqueues at most
 * (2 * n_layers + 2) * ceil(count / 128) launches, each serving every item of its block; a layer in which no item of the block has a new
 * column is not launched.  A step neither allocates, copies nor synchronises.  All device state is allocated by fv_wnpool_create:
 *   sessions * hidden_channels * (sum_i pow2(2 p_i + S) + pow2(R + S) + S) floats, S = max_chunk + R, pow2 = the next power of two
 * (S is max_chunk + R where the stream has max(max_chunk, R): an item may flush together with its last frames, and its layers then advance
 * by up to max_chunk + R frames in one step).  The pool reads the encoder's weights: destroy it before the encoder.  The whole step is
 * validated before any counter moves or anything is enqueued, and a refusal names the item and the session: a refused step leaves every
 * slot as it was. */
typedef struct fv_wnpool fv_wnpool;
/* p must be finalized (FV_ERR_STATE otherwise); sessions in [1, 65535], max_chunk in [1, 2^20]. */
FV_API fv_status fv_wnpool_create(fv_posterior* p, int32_t sessions, int32_t max_chunk, fv_wnpool** out);
/* Pure host, no GPU: what a step of `items` would emit on slots with the counters received[s], emitted[s], flushed[s] (flushed may be NULL:
 * none is) of an encoder of reach R.  Writes E' - E per item into frames_out and returns the largest, or the negative fv_status of a refusal:
 * a session outside [0, sessions), a duplicate session, frames outside [0, max_chunk], more than 2^30 frames in one utterance
 * (FV_ERR_INVALID), an item for a flushed slot (FV_ERR_STATE).  Changes nothing. */
FV_API int64_t fv_wnpool_plan(int32_t reach, int32_t sessions, int32_t max_chunk, const int64_t* received, const int64_t* emitted,
                              const int32_t* flushed, const fv_wavpool_item* items, int32_t count, int64_t* frames_out);
/* d_x: (count, in_channels, x_row_stride): frame j of channel ch of item i's chunk at d_x[i * x_item_stride + ch * x_row_stride + j],
 * x_row_stride >= the longest chunk; what follows an item's frames in its row, NaN included, is never loaded; NULL when no item has frames.
 * d_z, d_mean, d_logvar: (count, out_channels, out_cols), out_cols >= the largest E' - E: row i receives item i's frames first and exactly
 * 0.0f after them (the mean too, in bnvae mode), every element written.  d_mean / d_logvar must be NULL in vqvae mode and may be NULL in the
 * vae modes; d_z may be NULL when out_cols = 0.  frames_out (may be NULL) receives E' - E per item.  The plan's refusals apply, and null
 * buffers, a row stride shorter than a chunk and out_cols below the largest E' - E are refused as well.  Asynchronous on `stream`. */
FV_API fv_status fv_wnpool_step(fv_wnpool* p, const fv_wavpool_item* items, int32_t count, const float* d_x, int64_t x_item_stride,
                                int64_t x_row_stride, float* d_z, float* d_mean, float* d_logvar, int32_t out_cols, int64_t* frames_out,
                                void* stream);
/* N = E = 0 and the flushed flag cleared for one slot; no device work (nothing at or past a frontier or before frame 0 is ever read). */
FV_API fv_status fv_wnpool_reset(fv_wnpool* p, int32_t session);
/* N, E and N - E of one slot; -1 for NULL or a session out of range. */
FV_API int64_t fv_wnpool_received(const fv_wnpool* p, int32_t session);
FV_API int64_t fv_wnpool_emitted(const fv_wnpool* p, int32_t session);
FV_API int64_t fv_wnpool_pending(const fv_wnpool* p, int32_t session);
/* R; -1 for NULL. */
FV_API int32_t fv_wnpool_lookahead(const fv_wnpool* p);
/* The most one item can emit in a step: max_chunk + R (a flush with max_chunk frames after R pending ones); -1 for NULL. */
FV_API int64_t fv_wnpool_max_frames(const fv_wnpool* p);
/* Host counter: the kernel launches the last accepted step enqueued; -1 for NULL. */
FV_API int32_t fv_wnpool_launches(const fv_wnpool* p);
FV_API void fv_wnpool_destroy(fv_wnpool* p);

/* -------- wav2vec2 / HuBERT encoder (modules/encoders/hubert.py: HubertModel in its "stable layer norm" form, then `post`) --------
 * Eval-mode fp32 forward of the family feat_extract_norm = "layer", do_stable_layer_norm, conv_bias, feat_proj_layer_norm, GELU, eps 1e-5
 * (facebook/hubert-large-ll60k, facebook/mms-300m).  Activations are time major, (row, frame, channel).  With len_0 = the row's samples and
 * len_l = floor((len_{l-1} - kernel_l) / stride_l) + 1 (0 where that is not positive) — HF's _get_feat_extract_output_lengths:
 *   conv layer l:   c = GELU(LN_channels(conv_l(c) + bias)), no padding: a valid frame reads valid samples only
 *   projection:     h = W LN(c) + b
 *   pos conv:       h = h + GELU(conv_grouped(h)), k = pos_conv_kernel taps, zero padding k / 2 (an even k drops the last sample: SamePad);
 *                   weight norm over dim 2, w[:, :, j] = g[j] v[:, :, j] / |v[:, :, j]|, folded in fp64 at finalize
 *   layer i:        h = h + out(attn(LN(h)));  h = h + W2 GELU(W1 LN(h))     attn: softmax(Q K' / 8) V per head over the row's own frames
 *   last:           y = LN(h)
 *   post (post_channels > 0): Conv1d(hidden, O, 3, pad 1), SiLU, Conv1d(O, O, 3, stride 2, pad 1), SiLU, Conv1d(O, O, 1)
 * Every matrix product, the convs included, is one implicit GEMM on v_mfma_f32_32x32x2_f32; an output element's sum runs over k in
 * ascending order from one accumulator, then the bias is added.  The attention keeps a running maximum and sum over tiles of 32 keys: no
 * frames x frames tensor exists.  Keys, frames and samples at or past a row's own count are never loaded, and every output and hidden
 * state holds exact zeros there, so a row has the same bits alone, in any batch and padded to any T.
 * Limits: head size hidden / heads = 64; hidden, conv_dim in [1, 1024] (a LayerNorm row lives in one wave's registers) and multiples of 4;
 * intermediate, post_channels at most 8192 and multiples of 4; layers in [1, 64]; n_conv in [1, 8] with kernel[0] at most 32; kernel,
 * stride in [1, 64]; pos_conv_kernel in [1, 256], pos_conv_groups dividing hidden; batch in [0, 65535], batch * T at most 2^30 samples.
 * Every entry validates all a host can see before it enqueues anything, and names the offending field. */
typedef struct fv_w2v_config {
    int32_t hidden;            /* HF hidden_size */
    int32_t layers;            /* num_hidden_layers */
    int32_t heads;             /* num_attention_heads */
    int32_t intermediate;      /* intermediate_size */
    int32_t n_conv;            /* len(conv_dim) */
    int32_t conv_dim[8];
    int32_t conv_kernel[8];
    int32_t conv_stride[8];
    int32_t pos_conv_kernel;   /* num_conv_pos_embeddings */
    int32_t pos_conv_groups;   /* num_conv_pos_embedding_groups */
    int32_t post_channels;     /* hubert.py's output_size; 0 = the backbone alone (last_hidden_state) */
} fv_w2v_config;

typedef struct fv_w2v fv_w2v;

/* Validates on the host, no device work.  FV_ERR_INVALID / FV_ERR_UNSUPPORTED name the field. */
FV_API fv_status fv_w2v_create(const fv_w2v_config* cfg, fv_w2v** out);
/* The reference module's state-dict keys: "model." + HF's (feature_extractor.conv_layers.{l}.{conv,layer_norm}.{weight,bias},
 * feature_projection.{layer_norm,projection}.*, encoder.pos_conv_embed.conv.{bias,parametrizations.weight.original0,original1},
 * encoder.layers.{i}.{attention.{k,v,q,out}_proj,layer_norm,feed_forward.{intermediate,output}_dense,final_layer_norm}.*,
 * encoder.layer_norm.*) and post.{0,2,4}.{weight,bias}.  The legacy ...conv.weight_g / weight_v are taken for original0 / original1;
 * model.masked_spec_embed is accepted and ignored.  host: fp32, torch layout, copied.  An unknown key -> FV_ERR_INVALID, a wrong shape ->
 * FV_ERR_SHAPE, both by name; after fv_w2v_finalize -> FV_ERR_STATE. */
FV_API fv_status fv_w2v_load_weight(fv_w2v* w, const char* name, const float* host, const int64_t* shape, int32_t ndim);
/* Strict load: FV_ERR_MISSING_WEIGHT names the first absent key (before any device work).  Folds the weight norm, reorders conv weights
 * to (out, tap, in), fuses q | k | v into one matrix, uploads. */
FV_API fv_status fv_w2v_finalize(fv_w2v* w);
/* Frames that `samples` samples give: stage 0 after the backbone, stage 1 after `post` (floor((F - 1) / 2) + 1; 0 for F = 0).  -1: bad argument. */
FV_API int64_t fv_w2v_frames(const fv_w2v* w, int64_t samples, int32_t stage);
/* Bytes of device scratch fv_w2v_forward needs; 0 for an invalid shape (fv_last_error says which) and where no frame comes out. */
FV_API size_t fv_w2v_workspace_bytes(const fv_w2v* w, int32_t batch, int64_t T);
/* d_x: (batch, T) fp32 samples.  host_lengths: NULL (every row holds T samples) or `batch` sample counts in [0, T], read before the call
 * returns.  With F = fv_w2v_frames(T, 0), F2 = fv_w2v_frames(T, 1):  d_out is (batch, post_channels, F2), the reference's layout — or, with
 * post_channels = 0, last_hidden_state (batch, F, hidden); d_hidden_states: NULL or (layers + 1, batch, F, hidden), the input of layer 0
 * and every layer's output (HF's output_hidden_states without the final norm).  Every element is written, exact zeros at and past a row's
 * own frame count.  d_workspace, d_out and d_hidden_states must be 16-byte aligned.  batch = 0 or F = 0 is FV_OK and launches nothing.
 * Asynchronous on `stream`. */
FV_API fv_status fv_w2v_forward(fv_w2v* w, const float* d_x, int64_t T, const int32_t* host_lengths, int32_t batch, float* d_out,
                                float* d_hidden_states, void* d_workspace, size_t workspace_bytes, void* stream);
FV_API void fv_w2v_destroy(fv_w2v* w);

/* -------- MMSEncoder's front and back (modules/encoders/mms.py) --------
 * The reference resamples to 16 kHz (mms.py:20-22), moves every row through numpy into HF's Wav2Vec2FeatureExtractor (mms.py:23-27), runs
 * Wav2Vec2Model (mms.py:29) and maps the backbone's frames to L / hop_length frames (mms.py:30-31).  The resampler is fv_global_resample_*,
 * the backbone fv_w2v_forward on a post_channels = 0 encoder; the two steps between and after them are the entries below.  Both take ragged
 * rows: per-row counts are host arrays read before the call returns, nothing at or past a row's count is read, the outputs hold exact
 * zeros there, and a row has the same bits alone, in any batch, in any row order and padded to any width.  Every entry validates all a
 * host can see, and names the offending argument, before it enqueues anything.  batch in [0, 65535]; batch * T, batch * F and batch * N at
 * most 2^30. */
/* Bytes of device scratch fv_mms_normalize needs for the sums behind mms.py:23-27 (16 per row and segment of 4096 samples); 0 for an
 * invalid shape (fv_last_error says which) and for batch = 0 or T = 0. */
FV_API size_t fv_mms_normalize_workspace_bytes(int32_t batch, int64_t T);
/* mms.py:23-27, the processor's do_normalize (HF's zero_mean_unit_var_norm): y = (x - mean) / sqrt(var + 1e-7) with the population
 * variance, each row over its own length.  d_x, d_y: (batch, T) fp32, d_y may be d_x.  host_lengths: NULL (every row holds T samples) or
 * `batch` counts in [0, T].  The sums of x and x^2 are fp64, over segments of 4096 samples and then over the segments in ascending order —
 * an order fixed by the row's length alone, no atomics; mean and 1 / sqrt(var + 1e-7) are rounded to fp32 once, and an output is one
 * rounded subtraction and one rounded product.  A row of length 0 gives zeros; a constant row gives zeros, as numpy does.  d_workspace
 * must be 16-byte aligned; 16-byte accesses are used where T is a multiple of 4 and d_x, d_y are 16-byte aligned, with the same bits
 * either way.  Asynchronous on `stream`. */
FV_API fv_status fv_mms_normalize(const float* d_x, int64_t T, const int32_t* host_lengths, int32_t batch, float* d_y, void* d_workspace,
                                  size_t workspace_bytes, void* stream);
/* mms.py:30-31, x.transpose(1, 2) then F.interpolate(size = N, mode = "nearest"): d_x (batch, F, H) time major, fv_w2v_forward's
 * last_hidden_state -> d_y (batch, H, N) channel major.  host_frames / host_out_frames: NULL (every row holds F source frames / N output
 * frames) or `batch` counts in [0, F] / [0, N].  y[b][h][j] = x[b][src][h] for j < N_b with PyTorch's legacy rule in fp32,
 * src = min((int)floorf(j * scale), F_b - 1), scale = (float)F_b / (float)N_b, the product one rounded multiply; exact zeros for
 * j >= N_b.  A row with F_b = 0 and N_b > 0 has nothing to read and is refused.  H in [4, 8192], a multiple of 4; d_x 16-byte aligned;
 * 16-byte stores where N is a multiple of 4 and d_y is 16-byte aligned, with the same bits either way.  Asynchronous on `stream`. */
FV_API fv_status fv_mms_interpolate(const float* d_x, int64_t F, int32_t H, const int32_t* host_frames, const int32_t* host_out_frames,
                                    int32_t batch, float* d_y, int64_t N, void* stream);
/* Pure host: the source frame fv_mms_interpolate takes for output frame j of a row with F source and N output frames (mms.py:31); -1 for
 * F < 1, N < 1 or j outside [0, N). */
FV_API int64_t fv_mms_nearest_index(int64_t F, int64_t N, int64_t j);

/* -------- ConvNeXt backbone, layer by layer and chunk by chunk (fv_cnxstream_*) --------
 * What fv_wnstream_* is to the posterior encoder, for an FV_MODEL_CONVNEXT engine with kernel_size 7 (p = 3).  `batch` rows advance in
 * lockstep.  Level 0 is the stem conv, levels 1 .. L the blocks (L = sum of depths); R = p (L + 1) is the lookahead — the backbone's own
 * reach, fv_reach_frames less the 2 frames of margin that engine's windows keep.  With N frames received and E emitted: a push of c frames
 * sets N += c, E' = max(E, N - R) and writes the frames [E, E'); the flush sets E' = N and writes the rest, at most R frames; afterwards
 * pushes are refused (FV_ERR_STATE) until fv_cnxstream_reset.
 *   After a call level l has produced its output on [0, flush ? N : max(0, N - p (l + 1))), and the call ran every level over the columns
 * that are new at that level (none: no launch).  A block keeps the last 6 columns of its input in a ring of its own — (batch, dim, cap), cap
 * the power of two >= 6 + S, S = max(max_chunk, R), slot = frame & (cap - 1) — and its depthwise conv + LayerNorm runs in the stream form of
 * the whole-row tile kernel: frames below the input's old frontier come from the ring, the call's new frames from the level below, frames
 * before 0 and past the frontier are zeros by predicate (an uninitialised or stale ring is never read), and the same launch files the new
 * frames into the ring.  The stem conv runs over the last 6 input frames ++ the chunk; everything per-frame (LayerNorms, the pointwise
 * convs) runs the whole-row kernels over the new columns.  Every launch takes its kernel from the layer's shape alone.
 *   The claim: the concatenated frames are BIT-identical to fv_forward over the whole utterance with fv_set_batch_invariant(e, 1), under any
 * chunking and for any batch, for utterances with max(dims) * T < 2^28 (past that the whole-row forward leaves the tile kernel).  One
 * narrowing: where input_channels == dims[0] the stem is a C -> C k = 7 conv, which the batch-invariant forward runs as Winograd tap groups
 * under FV_CONV_ALGO_AUTO; a Winograd output's bits depend on where its pair / quad lies in the launch, so the stream runs the stem as
 * direct sums and its bits are those of fv_forward with fv_set_conv_algorithm(e, FV_CONV_ALGO_DIRECT) as well (the default decoder backbone,
 * 512 -> 512; for the default encoder, 513 -> 512, the algorithm setting changes nothing).  The claim is about the shipped whole-row
 * path, the depthwise tile kernel: the experiment switch FV_OLD_DWLN sends the whole-row forward to the register kernel, which sums the
 * channels in another order, while the stream always runs the tile body (FV_DWLN_NG8 moves both launches alike, FV_DWLN_RR changes no sum).
 *   A call neither synchronises nor allocates nor copies to the host.  All device state is allocated at create; fv_cnxstream_state_bytes
 * reports it.  The stream reads the engine's weights: destroy it before the engine.  A refused call changes no counter. */
typedef struct fv_cnxstream fv_cnxstream;
/* Refused by name: an engine that is not finalized or in f16x3 precision (FV_ERR_STATE); a model other than FV_MODEL_CONVNEXT,
 * kernel_size != 7, a stage wider than 1024 channels, batch outside [1, 65535], max_chunk outside [1, 2^16] (FV_ERR_INVALID). */
FV_API fv_status fv_cnxstream_create(fv_engine* e, int32_t batch, int32_t max_chunk, fv_cnxstream** out);
/* d_x: frame t of channel ch of row b at d_x[b * x_batch_stride + ch * x_row_stride + t], x_row_stride >= c (a slice along T passes as it
 * is); c in [0, max_chunk], d_x may be NULL when c = 0.  d_y: (batch, out_channels, y_row_stride), y_row_stride >= E' - E, frame E + j in
 * column j; may be NULL when the call emits nothing.  *emitted (may be NULL) receives E' - E.  At most 2^30 frames per utterance. */
FV_API fv_status fv_cnxstream_push(fv_cnxstream* s, const float* d_x, int64_t x_batch_stride, int64_t x_row_stride, int32_t c, float* d_y,
                                   int64_t y_row_stride, int64_t* emitted, void* stream);
FV_API fv_status fv_cnxstream_flush(fv_cnxstream* s, float* d_y, int64_t y_row_stride, int64_t* emitted, void* stream);
/* N = E = 0 for the next utterance; no device work (nothing a ring holds from the last one is read). */
FV_API fv_status fv_cnxstream_reset(fv_cnxstream* s);
/* N - E; -1 for NULL. */
FV_API int64_t fv_cnxstream_pending(const fv_cnxstream* s);
/* R; -1 for NULL. */
FV_API int32_t fv_cnxstream_lookahead(const fv_cnxstream* s);
/* Bytes of device memory the stream holds; -1 for NULL. */
FV_API int64_t fv_cnxstream_state_bytes(const fv_cnxstream* s);
FV_API void fv_cnxstream_destroy(fv_cnxstream* s);
/* Pure host: the plan of one level of a call that takes a stream of `levels` blocks from N0 to N1 frames (flush: N1 == N0 and the utterance
 * ends), as the engine computes it.  out[0..5] = in0, in1, out0, out1 and, for level 0 (the stem), the window's width and the column of
 * out0 in it; for a block, the workgroups per row and the first frame workgroup 1 files (-1 with fewer than two).  Returns the ring's
 * slots for max_chunk, or -1 for arguments outside 0 <= N0 <= N1, 0 <= level <= levels, max_chunk >= 1, out != NULL. */
FV_API int32_t fv_cnxstream_plan(int64_t N0, int64_t N1, int32_t flush, int32_t level, int32_t max_chunk, int32_t levels, int64_t* out);

/* -------- ConvNeXt backbone, layer by layer, for sessions that advance independently (fv_cnxpool_*) --------
 * What fv_cnxstream_* is to rows in lockstep, for `sessions` slots with their own N, E and flushed flag, as fv_wnpool_* is to fv_wnstream_*.
 * A step is a list of items (fv_wavpool_item: session, `samples` counting FRAMES here, flush: the utterance ends with these frames), each
 * session at most once.  Per item N' = N + frames and E' = flush ? N' : max(E, N' - R); the item emits the frames [E, E').  A flush at
 * N' = 0 emits nothing.  After its flush a slot refuses items (FV_ERR_STATE) until fv_cnxpool_reset.
 *   A slot's state is its own row of the input ring and of every block's ring, (sessions, dim, cap), cap the power of two >= 6 + S,
 * S = max_chunk + R (where the stream has max(max_chunk, R): an item may flush together with its last frames, and a level's frontier then
 * moves by up to max_chunk + R frames in one step).  A step plans every item at every level on the host, from its slot's (N, N', flush)
 * with the stream's plan, and runs per level over the columns that are new at that level: the depthwise conv + LayerNorm as the pool form
 * of the whole-row tile kernel, one launch per fv_cnxpool_table_size() items, each entry reading and filing into its slot's ring row; H and
 * the residual are PACKED, (dim, P) with P the sum of the items' new columns at that level, and everything per-frame (the LayerNorms, the
 * pointwise convs) runs the whole-row kernels over the packed buffer as one row of P columns.  The stem conv runs over (count, C_in, Wmax),
 * Wmax = 6 + the step's longest chunk: row i holds the last 6 input frames of session i ++ its chunk ++ exact zeros.
 *   Launches of a step in which every level has work, with T = ceil(count / fv_cnxpool_table_size()):
 *       stem: T window launches + the conv + its LayerNorm;  every block: T depthwise launches + 2 pointwise launches;
 *       every stage change: 2;  emission: the final LayerNorm + ceil(count / 32) crop launches
 *   = T (1 + L) + 2 + 2 L + 2 (num_stages - 1) + 1 + ceil(count / 32).  With T = 1 that is the layer stream's count for the same call — 22
 * for the default encoder (one stage of 6 blocks), 33 for the default backbone (6 + 3 blocks) — plus the crop, which stands in place of the
 * stream's optional 2-D copy.  A level at which no item of the step has a new column or chunk frame launches nothing; fv_cnxpool_launches
 * reports what the last accepted step enqueued.
 *   The claim: a session's concatenated frames are BIT-identical to fv_forward over its whole utterance with fv_set_batch_invariant(e, 1)
 * — and, where input_channels == dims[0] (a C -> C stem, which has a Winograd form), with fv_set_conv_algorithm(e, FV_CONV_ALGO_DIRECT)
 * as well: the pool runs the stem as direct sums, as the stream does — whatever the other sessions do, in any item order, after any
 * fv_cnxpool_reset(session), for utterances with max(dims) * T < 2^28.
 *   A step neither allocates device memory, copies to the host nor synchronises.  All device state is allocated by fv_cnxpool_create;
 * fv_cnxpool_state_bytes reports it.  The whole step is validated before any counter moves or anything is enqueued, and a refusal names
 * the item and the session: a refused step leaves every slot as it was.  The pool reads the engine's weights: destroy it before the engine. */
typedef struct fv_cnxpool fv_cnxpool;
/* Refused by name: what fv_cnxstream_create refuses (an engine that is not finalized or in f16x3 precision: FV_ERR_STATE; a model other
 * than FV_MODEL_CONVNEXT, kernel_size != 7, a stage wider than 1024 channels, max_chunk outside [1, 2^16]: FV_ERR_INVALID), sessions
 * outside [1, 65535], and sizes that leave the kernels' 32-bit addressing — 4 max(dims) sessions (max_chunk + R) >= 2^29 floats, a ring row
 * of max(dims, input_channels) * cap >= 2^28 floats or a stem window of 2^29 floats (FV_ERR_INVALID). */
FV_API fv_status fv_cnxpool_create(fv_engine* e, int32_t sessions, int32_t max_chunk, fv_cnxpool** out);
/* Pure host, no GPU: what a step of `items` would emit on slots with the counters received[s], emitted[s], flushed[s] (flushed may be NULL:
 * none is) of a backbone of lookahead `reach`.  Writes E' - E per item into frames_out and returns the largest, or the negative fv_status of
 * a refusal: a session outside [0, sessions), a duplicate session, frames outside [0, max_chunk], more than 2^30 frames in one utterance
 * (FV_ERR_INVALID), an item for a flushed slot (FV_ERR_STATE).  sessions in [1, 65535], max_chunk in [1, 2^20].  Changes nothing. */
FV_API int64_t fv_cnxpool_plan(int32_t reach, int32_t sessions, int32_t max_chunk, const int64_t* received, const int64_t* emitted,
                               const int32_t* flushed, const fv_wavpool_item* items, int32_t count, int64_t* frames_out);
/* d_x: (count, input_channels, x_row_stride): frame j of channel ch of item i's chunk at d_x[i * x_item_stride + ch * x_row_stride + j],
 * x_row_stride >= the longest chunk; what follows an item's frames in its row, NaN included, is never loaded; NULL when no item has frames.
 * d_y: (count, out_channels, out_cols), out_cols >= the largest E' - E: row i receives item i's frames first and exactly 0.0f after them,
 * every element written; may be NULL when out_cols = 0.  frames_out (may be NULL) receives E' - E per item.  The plan's refusals apply, and
 * null buffers, a row stride shorter than a chunk and out_cols below the largest E' - E are refused as well.  Asynchronous on `stream`. */
FV_API fv_status fv_cnxpool_step(fv_cnxpool* p, const fv_wavpool_item* items, int32_t count, const float* d_x, int64_t x_item_stride,
                                 int64_t x_row_stride, float* d_y, int32_t out_cols, int64_t* frames_out, void* stream);
/* N = E = 0 and the flushed flag cleared for one slot; no device work (nothing at or past a frontier or before frame 0 is ever read). */
FV_API fv_status fv_cnxpool_reset(fv_cnxpool* p, int32_t session);
/* N, E and N - E of one slot; -1 for NULL or a session out of range. */
FV_API int64_t fv_cnxpool_received(const fv_cnxpool* p, int32_t session);
FV_API int64_t fv_cnxpool_emitted(const fv_cnxpool* p, int32_t session);
FV_API int64_t fv_cnxpool_pending(const fv_cnxpool* p, int32_t session);
/* R; -1 for NULL. */
FV_API int32_t fv_cnxpool_lookahead(const fv_cnxpool* p);
/* The most one item can emit in a step: max_chunk + R (a flush with max_chunk frames after R pending ones); -1 for NULL. */
FV_API int64_t fv_cnxpool_max_frames(const fv_cnxpool* p);
/* Host counter: the kernel launches the last accepted step enqueued (the formula above); -1 for NULL. */
FV_API int32_t fv_cnxpool_launches(const fv_cnxpool* p);
/* Bytes of device memory the pool holds; -1 for NULL. */
FV_API int64_t fv_cnxpool_state_bytes(const fv_cnxpool* p);
/* Items per by-value launch table of the depthwise and the stem-window kernel. */
FV_API int32_t fv_cnxpool_table_size(void);
FV_API void fv_cnxpool_destroy(fv_cnxpool* p);

/* -------- the GAN's critics, forward only (fv_disc_*) --------
 * modules/discriminators/mpd.py (MultiPeriodDiscriminator, kind FV_DISC_PERIOD) and modules/discriminators/mrd.py
 * (MultiResolutionDiscriminator, kind FV_DISC_RESOLUTION) in eval mode, and the sums behind models/gan.py:149 / 155 / 204.  One handle
 * holds up to 8 sub-discriminators of one kind.  Activations are channel last, (row, H, W, C):
 *   period i:      the wave read as (ceil(L / p), p, 1) with zeros past L (mpd.py:47-52); Conv2d(c[l], c[l + 1], (kernel_size, 1),
 *                  (stride, 1), pad (kernel_size / 2, 0)) + SiLU per channel pair (mpd.py:54-57); conv_post Conv2d(c[-1], 1, (3, 1), pad (1, 0))
 *   resolution i:  reflect padding ((n_fft - hop) / 2, (n_fft - hop + 1) / 2) at the row's own ends, frames of n_fft at hop, a window of
 *                  ones of win_length centred in n_fft, sqrt(re^2 + im^2) (mrd.py:52-73): (n_fft / 2 + 1, L / hop, 1); then Conv2d(1, 32,
 *                  (3, 9), pad (1, 4)), three Conv2d(32, 32, (3, 9), stride (1, 2), pad (1, 4)), Conv2d(32, 32, (3, 3), pad (1, 1)), each
 *                  + SiLU (mrd.py:41-44); conv_post Conv2d(32, 1, (3, 3), pad (1, 1))
 * Every conv, the fold and the DFT are one implicit GEMM on v_mfma_f32_32x32x2_f32: an element's sum runs over k ascending in the order
 * (kh, kw, c) from one accumulator, then the bias.  Weight norm (dim 0: the norm over dims 1-3 per output channel) is folded in fp64 and
 * rounded once at finalize.  Ragged rows: nothing at or past a row's own (H, W) extent is read, feature maps and scores hold exact zeros
 * there, and a row has the same bits alone, in any batch, in any order and padded to any T — the reference run on the row alone.
 * Limits: n_sub in [1, 8]; n_channels in [2, 8], channels[0] = 1, the others multiples of 4 in [4, 1024]; kernel_size in [1, 15], stride
 * in [1, 16]; period in [1, 4096]; n_fft a multiple of 4 in [4, 4096], hop_length and win_length in [1, n_fft]; batch in [0, 65535], T at
 * most 2^26 and every feature map at most 2^31 - 1 elements per row.  Not built: spectral norm, gradients. */
#define FV_DISC_PERIOD 0
#define FV_DISC_RESOLUTION 1
typedef struct fv_disc_config {
    int32_t kind;              /* FV_DISC_PERIOD | FV_DISC_RESOLUTION */
    int32_t n_sub;             /* sub-discriminators */
    int32_t period[8];         /* period kind: DiscriminatorP(period=) */
    int32_t n_fft[8];          /* resolution kind: DiscriminatorR(n_fft=, hop_length=, win_length=) */
    int32_t hop_length[8];
    int32_t win_length[8];
    int32_t n_channels;        /* period kind: len(channels) */
    int32_t channels[8];       /* DiscriminatorP(channels=), default 1, 64, 128, 256, 512, 1024 */
    int32_t kernel_size;       /* DiscriminatorP(kernel_size=) */
    int32_t stride;            /* DiscriminatorP(stride=) */
} fv_disc_config;
/* One feature map of the output buffer: (batch, H, W, C) floats at `offset`; the last layer of a sub-discriminator is its score map (C = 1). */
typedef struct fv_disc_map {
    int64_t offset;            /* in floats, a multiple of 4 */
    int32_t H, W, C;           /* the extent of a row of T samples */
    int32_t sub, layer;
} fv_disc_map;

typedef struct fv_disc fv_disc;

/* mpd.py:10-41 / mrd.py:8-33.  Validates on the host, no device work.  FV_ERR_INVALID names the field. */
FV_API fv_status fv_disc_create(const fv_disc_config* cfg, fv_disc** out);
/* The reference modules' state-dict keys (mpd.py:27-41, mrd.py:24-33 under weight_norm): discriminators.{i}.convs.{l}.bias,
 * .parametrizations.weight.original0 (N, 1, 1, 1), .parametrizations.weight.original1 (N, C, KH, KW), and discriminators.{i}.conv_post.
 * the same; the legacy .weight_g / .weight_v are taken for original0 / original1.  host: fp32, torch layout, copied.  An unknown key ->
 * FV_ERR_INVALID, a wrong shape -> FV_ERR_SHAPE, both by name; after fv_disc_finalize -> FV_ERR_STATE. */
FV_API fv_status fv_disc_load_weight(fv_disc* d, const char* name, const float* host, const int64_t* shape, int32_t ndim);
/* Strict load: FV_ERR_MISSING_WEIGHT names the first absent key.  Folds the weight norm (torch's weight_norm, dim 0), reorders to
 * (out, kh, kw, in), builds the windowed DFT of every resolution (mrd.py:62-69), uploads. */
FV_API fv_status fv_disc_finalize(fv_disc* d);
FV_API void fv_disc_destroy(fv_disc* d);
/* mpd.py:57,60 / mrd.py:44,47, the fmap lists: where every feature map of a (batch, T) call lies in the output buffer, sub-discriminator
 * by sub-discriminator, layer by layer (maps[sub * layers + layer]; `capacity` entries; maps may be NULL).  *n_maps (may be NULL) receives
 * their number.  Returns the buffer's size in floats, or -1 for a bad argument (fv_last_error says which).  Pure host. */
FV_API int64_t fv_disc_layout(const fv_disc* d, int32_t batch, int64_t T, fv_disc_map* maps, int32_t capacity, int32_t* n_maps);
/* Bytes of device scratch fv_disc_forward and fv_disc_distance need (the larger): the padded wave, the DFT and the magnitudes of one
 * resolution (mrd.py:52-73); the partial sums of the distance.  0 for a bad argument. */
FV_API size_t fv_disc_workspace_bytes(const fv_disc* d, int32_t batch, int64_t T);
/* mpd.py:43-63, :82-86 / mrd.py:35-50, :94-98.  d_x: (batch, T) fp32 samples.  host_lengths: NULL (every row holds T samples) or `batch`
 * sample counts in [1, T], read before the call returns.  d_out: out_floats >= fv_disc_layout(batch, T) floats; every element of every
 * map is written, exact zeros at and past a row's own extent.  Refused by name, before anything is enqueued: a row of 0 samples; for the
 * resolution kind a row not longer than its reflect padding or shorter than one hop (by row and minimum length); buffers that are too
 * small or not 16-byte aligned.  No allocation, copy or synchronisation.  Asynchronous on `stream`. */
FV_API fv_status fv_disc_forward(fv_disc* d, const float* d_x, int64_t T, const int32_t* host_lengths, int32_t batch, float* d_out,
                                 int64_t out_floats, void* d_workspace, size_t workspace_bytes, void* stream);
/* gan.py:149 (generator's adversarial term), :155 (the critic's) and :204 (feature matching), as sums: d_real / d_fake are two output
 * buffers of fv_disc_forward for the same (batch, T, host_lengths).  d_sums: (batch, n_sub, layers, 5) float64; per row, sub-discriminator
 * and layer, over the row's own extent: sum |real - fake|, sum (1 - fake)^2, sum fake^2, sum (real - 1)^2 and the element count (the last
 * layer's are the score terms).  Terms are fp32 with one rounding per operation, accumulated in fp64 per tile of 4096 elements in a fixed
 * order, then a finish launch: no float atomics, and a row's sums are bit-identical alone and in any batch.  Asynchronous on `stream`. */
FV_API fv_status fv_disc_distance(fv_disc* d, const float* d_real, const float* d_fake, int64_t T, const int32_t* host_lengths, int32_t batch,
                                  double* d_sums, void* d_workspace, size_t workspace_bytes, void* stream);

/* -------- per-launch timing (measurement aid; bench.py's roofline leg) --------
 * Between fv_profile_begin and fv_profile_end every kernel that fv_forward enqueues is bracketed by hipEvents recorded
 * on the launch stream.  fv_profile_end synchronises them and writes a JSON array
 *   [{"kernel": label, "launches": n, "total_ms": .., "avg_ms": .., "flops_per_launch": .., "bytes_per_launch": ..}]
 * (algorithmic flops / per-layer compulsory bytes) into json_buf (truncated to cap); *needed
 * receives the full size.  The reference has no counterpart (its only timer is test.py:88-90). */
FV_API fv_status fv_profile_begin(fv_engine* e);
FV_API fv_status fv_profile_end(fv_engine* e, char* json_buf, size_t cap, size_t* needed);

/* -------- misc -------- */
FV_API const char* fv_last_error(void);
FV_API int32_t fv_abi_version(void);
/* Name of the device kernel variant the last fv_conv_forward / fv_aa_snake_forward / fv_dwconv_ln_forward on this thread dispatched (diagnostics). */
FV_API const char* fv_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* FISHVOC_H */
