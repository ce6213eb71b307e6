// Internal declarations shared by the host engine and the HIP kernels of libfishvoc_hip.so.
// gfx950 (MI355X / CDNA4) only: 64-wide wavefronts, v_mfma_f32_32x32x2_f32, 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "conv_pack.h"
#include "fishvoc.h"

namespace fv {

void set_error(const char* fmt, ...);
void set_last_kernel(const char* name);
int num_cus();   // compute units of the current device (cached)

// Experiment knobs, read from the environment once per process (fv_reload_env() re-reads them): the launch path never calls getenv
struct Knobs {
    int pw = -2;          // FV_PW: forced gemm_pw configuration, -1 = "old" (the conv kernel), -2 = unset
    int pw_px = 0;        // FV_PW_PX: forced XCD row groups, 0 = unset
    bool dwln_ng8 = false, dwln_rr = false, old_dwln = false;   // FV_DWLN_NG8 / FV_DWLN_RR / FV_OLD_DWLN
    int wino = 1;         // FV_WINO: 0 = direct sums only, 1 = Winograd F(2,3) tap groups for the dilated k = 3 / 7 / 11 convs of launches that
                          // fill the chip (conv_wino_impl.h), 2 = for every eligible launch (tests)
    int wino_min_m = 32;  // FV_WINO_MIN_M: narrowest layer (output rows) that takes it
    int wino_cfg = -1;    // FV_WINO_CFG: forced tile (WinoCfg 0 ... 2), -1 = by shape
    int wino_min_blocks = -1;   // FV_WINO_MIN_BLOCKS: fewest workgroups of a launch that takes it, -1 = default
    int vec_store = 1;    // FV_VEC_STORE: 0 = the stride-8 upsamplers store single floats instead of 16-byte output quads (A/B runs, tests)
    // (FV_WINO4 / FV_WINO44 are also read when a layer is CREATED: it packs only the Winograd form they select — layer_forms() in conv_layer.hip)
    int pair_wino44 = 1;  // FV_PAIR_WINO44: 1 = the fused narrow pairs at k = 7 / 11 on F(4,4) tap groups (pair_wino44_impl.h), 0 = F(2,3) (pair_wino_impl.h)
    int wino44 = 1;       // FV_WINO44: 1 = F(4,4) tap groups (conv_wino44_impl.h) for k = 7 / 11 where FV_WINO4 would take F(4,3), 0 = F(4,3) there
    int wino44_rows = 0;  // FV_WINO44_ROWS: 64 = one 32-row tile per wave (64-row workgroups) everywhere; otherwise two (128 rows) where the layer has whole 128-row blocks
    int wino4 = 1;        // FV_WINO4: 1 = the quad-lattice kernels (conv_wino44_impl.h / conv_wino4_impl.h) for k = 7 / 11 where the Winograd path is taken and the layer has whole 64-row blocks, 0 = F(2,3) everywhere
    int lat_wino44 = 1;   // FV_LAT_WINO44: 1 = launches below the Winograd gate at k = 7 / 11 run F(4,4) tap groups (conv_wino_lat44_impl.h), 0 = F(2,3) (conv_wino_lat_impl.h);
                          //   n >= 2: ... only launches of >= n / 2 workgroups per CU in its 16-row tiling (experiments)
    int splitk_direct = 1;   // FV_SPLITK_DIRECT: 1 = the few-tap split-K launches (conv_pre, the upsamplers of a single clip) load their B operands straight from global memory (conv_mfma_splitk_direct_kernel), 0 = staged through LDS
    int wino44_flat = 1;  // FV_WINO44_FLAT: 1 = conv_wino44 tiles a flattened (clip, quad column) axis where that needs fewer 32-column tiles than tiling every clip on its own (T = 688: 5.4 tiles per clip), 0 = per clip
    int wino_lat = 1;     // FV_WINO_LAT: 0 = launches below the Winograd gate run the direct split-K kernels, 1 = the Winograd latency kernel
    int pair_wino4 = -1;  // FV_PAIR_WINO4: the fused wide k = 3 pairs (C = 64 / 128) on one F(4,3) tap group (pair_wino4_impl.h) — unset = where the engine's pair
                          //   branches ask for it (launches that fill the chip, not in batch-invariant mode), 0 = never, 2 = every conv_pair_run (tests)
    int pair_wino = 1;    // FV_PAIR_WINO: 0 = the fused (c1, c2) pairs run direct sums (resblock_pair.hip), 1 = Winograd tap groups where a kernel exists
    int conv_tile = -1;   // FV_CONV_TILE: a TileCfg name ("128x64", "splitK32x32", ...) forced on every conv_mfma launch that has that tile instantiated
                          //   (after all the shape remaps; tests pin the kernel instance by instance), -1 = by shape
    int ups_tile256 = 1;  // FV_X_UPS_TILE256: 0 = the two-tap polyphase upsamplers keep the 128-row tiles instead of 256 x 64 (A/B runs, tests)
    bool no_sum3 = false; // FV_NO_SUM3: the three-operand stack-mean goes through mean_of_three_kernel instead of the conv's staging (A/B runs, tests)
    bool branch_mean_chain = false;   // FV_BRANCH_MEAN=chain: the branch mean as the ordered accumulate on branch streams too (engine_forward.hip plan_stage; experiments, tests)
    int splitk = 0;       // FV_SPLITK: 32 / 64 = that tile of the split-K latency kernel wherever one is taken, 0 = by shape (experiments)
    long long splitk_max = 200;   // FV_SPLITK_MAX: largest launch, in workgroups of the small tile, that still takes the split-K latency kernel (experiments)
    bool aa_vec4 = true;  // FV_AA_VEC4=0: aa_snake runs the pair form on every tile instead of 16-byte accesses on interior tiles
    bool no_f16x3_pairs = false;   // FV_NO_F16X3_PAIRS: f16x3 precision mode runs per-layer split-fp16 convs instead of the fused pair kernels (diagnostics)
    bool w44_no_qr = false;   // FV_X_W44_NO_QR: conv_wino44 without the row-split 16-byte-store epilogue (A/B runs)
};
// TileCfg index of a tile name ("128x128", ..., "128x96"), -1 if there is none (conv_layer.hip)
int conv_tile_by_name(const char* name);
const Knobs& knobs();

// Conv algorithm selection of the call being enqueued (fv_set_conv_algorithm / fv_set_batch_invariant): thread-local, set by the C-ABI entry
// points for the duration of the call — conv_layer_run / conv_pair_run and the engine's fusion decisions read it
struct AlgoScope {
    AlgoScope(int algo, bool invariant);
    ~AlgoScope();
    int prev_algo;
    bool prev_inv;
};
int cur_algo();          // fv_conv_algo
bool cur_invariant();    // kernel choices from the layer shape alone
// fv_set_conv_algorithm of the running call, with the process-wide FV_WINO knob as the default behind FV_CONV_ALGO_AUTO
int effective_algo();

// Compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{}).  Register-resident operand
// rings need every index to be a constant expression in the source (an index that only becomes constant after loop unrolling
// can leave the array in scratch memory: the optimiser promotes arrays to registers before it unrolls).
template <class F, int... Is>
__device__ __host__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __host__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Optional per-launch timing (fv_profile_begin / fv_profile_end): hipEvents recorded on the launch stream around every
// kernel of a forward, aggregated by label together with the launch's ALGORITHMIC flops and bytes.
struct ProfRec {
    std::string label;
    double flops = 0, bytes = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};
struct Profiler {
    std::vector<ProfRec> recs;
};
Profiler* current_profiler();              // thread-local; nullptr when profiling is off
int prof_begin(hipStream_t s);             // returns record index or -1
void prof_end(hipStream_t s, int idx, const char* label, double flops, double bytes);

#define FV_HIP_CHECK(expr)                                                                       \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            ::fv::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return FV_ERR_HIP;                                                                   \
        }                                                                                        \
    } while (0)

// Per-row values that change with every call (a step's session tables, the lengths of a ragged batch) travel BY VALUE in the kernel
// arguments, N entries per launch: no device table, and no async copy that could read a host buffer after the next call has rewritten it.
// The kernel indexes `e` with the block index that runs over the launch's rows.  HIP's kernel-argument segment is 4 KiB; a table may take
// half of it, which leaves 2 KiB for the pointers and scalars beside it (the largest table holds 1792 bytes, the fullest kernel 1336).
template <class T, int N>
struct LaunchTable {
    static_assert(sizeof(T) * N <= 2048, "a by-value table takes at most half of the 4 KiB kernel-argument segment");
    static constexpr int size = N;
    T e[N];
};
// The one blocking loop over such tables: entries [first, first + nz) of `src` — a pointer to the entries, or a callable int -> entry — go
// into a zeroed Table, launch(table, first, nz) -> fv_status enqueues that block's kernels (per-block reductions and the launches they
// skip are its business), and the launch error is checked here.  Stops at the first status that is not FV_OK; count <= 0 launches nothing.
template <class Table, class Src, class Launch>
fv_status for_each_launch_table(int count, const Src& src, Launch&& launch) {
    for (int first = 0; first < count; first += Table::size) {
        const int nz = count - first < Table::size ? count - first : Table::size;
        Table blk{};
        for (int i = 0; i < nz; ++i) {
            if constexpr (std::is_pointer_v<Src>) blk.e[i] = src[first + i];
            else blk.e[i] = src(first + i);
        }
        if (const fv_status st = launch(blk, first, nz)) return st;
        FV_HIP_CHECK(hipGetLastError());
    }
    return FV_OK;
}

// Opt a kernel in to more than 64 KiB of dynamic LDS (gfx950: 160 KiB per CU).  The attribute is PER DEVICE, so the
// "already done" state is a bit per device ordinal (one mask per call site), set with an atomic OR: a process that drives
// several GPUs, or several host threads, gets every (kernel, device) pair opted in exactly once.  Returns false and sets
// the error string when the runtime refuses.
bool ensure_dynamic_lds(const void* kernel, int bytes, unsigned long long* done_mask);
bool dynamic_lds_refused();
#define FV_ENSURE_DYN_LDS(kernel, bytes)                                                   \
    ([&]() -> bool {                                                                       \
        static unsigned long long _fv_mask = 0;                                            \
        return ::fv::ensure_dynamic_lds((const void*)(kernel), (int)(bytes), &_fv_mask);   \
    }())

// ---------------------------------------------------------------------------------------------
// Fused conv layer ("implicit GEMM on fp32 MFMA").
//
//   out[b][m][n] = post( bias[m] + sum_{ci<Cin} sum_{j<ks} W[m][ci][j] * pre(x[b][ci][n + j*dil - pad_l]) )
//
// Conv1d:           m = c_out, n = t, pad_l = padding.
// ConvTranspose1d:  polyphase form.  m = (c_out, r) with r = output phase in [0, stride), n = q, ks' = ceil(k/stride),
//                   dil = 1, pad_l = ks'-1, and the result lands at t = q*stride + r - padding (scatter store).
// ---------------------------------------------------------------------------------------------
enum OutMode : int { OUT_SET = 0, OUT_ACCUM = 1 };  // OUT_ACCUM: y = (y_old + v) * out_scale  (MRF stack-mean)

struct ConvParams {
    const float* x;      // (B, Cin, Tin)
    const float* x2;     // SUM3 kernels: the input is ((x + x2) + x3) / 3 — the stack-mean of three ResBlock branches formed while
    const float* x3;     //   staging (same layout as x); NULL otherwise
    const float4* wp;    // packed weights, see pack_conv_weights() (conv_pack.hip)
    const float* bias;   // (m_pad) zero padded, never NULL
    float* y;
    const float* res;    // residual, same indexing as y (may be NULL, may alias y)
    const float* gamma;  // per-row scale applied before the residual (ConvNeXt layer-scale), may be NULL
    int Cin, Tin;
    int M, N;            // valid GEMM rows / columns per batch item
    int nchunk;          // 8-channel sub-chunks in the packed weights (ceil(Cin / 8) rounded up to a multiple of 4)
    int nchunk_real;     // ceil(Cin / 8): sub-chunks that actually hold channels
    int n_tiles, m_blks; // grid = B * m_blks * n_tiles
    int pad_l;
    int ks, dil;         // runtime copies (used by the generic variant)
    int pre_act, post_act;
    float slope;
    int out_mode;
    float out_scale;
    int convt;           // scatter store for the transposed conv
    int u, pad_t, Tout, Cout;
    long long x_bstride, y_bstride;
    int flat;            // pointwise convs (ks == 1): GEMM columns run over the flattened (batch, time) axis
    int n_total;         // flat: batch * N
    float acc_scale;     // accumulator scale applied before the bias (1 for the fp32 kernels, 1/s_w for f16x3)
    int xcd_rows;        // gemm_pw.hip: row groups the 8 XCDs split the m-tiles into (1, 2, 4 or 8)
    int wg_total;        // conv_wino_impl.h: workgroups of the launch (the grid is rounded up to a multiple of the 8 XCDs)
    int vec_store;       // conv_epilogue: stride-8 polyphase transposed conv whose output quads can go out as 16-byte stores
    int col_S, col_batch;   // conv_wino44_impl.h: > 0 = the launch's quad columns run over a flattened (clip, column) axis with col_S columns per clip, col_batch clips (grid batch 1)
#if defined(FV_X_SPLITK_TS) || defined(FV_X_CONV_TS)
    long long* dbg_ts;   // experiment: per-workgroup phase time stamps (split-K kernel / tiled conv kernel)
#endif
    // f16x3 precision mode (conv_f16x3_impl.h)
    const void* wph;     // split fp16 weight planes, see pack_conv_weights_f16x3() (conv_pack.hip)
    int nch16;           // 16-channel chunks in the packed planes
    int nch16_real;      // ceil(Cin / 16)
};

struct ConvLayer {
    // logical description
    bool transposed = false;
    int c_in = 0, c_out = 0, k = 0, dil = 1, padding = 0, stride = 1;
    // GEMM view
    int M = 0, ks = 0, pad_l = 0, nchunk = 0, nchunk_real = 0, m_pad = 0;
    float4* d_wp = nullptr;
    bool wino = false;         // a ResBlock / AMPBlock conv (k in {3, 7, 11}, dilation in {1, 3, 5}, 'same', C -> C): Winograd forms below, as its shape admits
    float4* d_wpw = nullptr;   // Winograd-transformed weights in the same fragment order, nv virtual taps (conv_wino_impl.h); optional
    int nv = 0;
    float4* d_wp16 = nullptr;  // 16x16x4-fragment layout, only for 16 -> 16 channel Conv1d (fused pair kernel)
    float4* d_wpw44 = nullptr; // Winograd F(4,4)-transformed weights (conv_wino44_impl.h): (32-row tile, plane half) x chunk x (3 ng + 1) fragments; optional
    float4* d_wpw4 = nullptr;  // Winograd F(4,3)-transformed weights (conv_wino4_impl.h): (32-row tile, plane half) x chunk x nv4 fragments; optional
    int nv4 = 0;
    float4* d_wpwl = nullptr;  // Winograd-transformed weights of the latency kernel: 16-row tiles, 8-channel blocks, tap pairs (conv_wino_lat_impl.h); optional
    float4* d_wpq16 = nullptr; // Winograd F(4,4)-transformed weights in 16x16x4 fragment order, C -> C, k in {7, 11}: C in {16, 32} for pair_wino44_impl.h, whole 32-row blocks for conv_wino_lat44_impl.h; optional
    float4* d_wpw16 = nullptr; // Winograd-transformed weights in 16x16x4 fragment order, C -> C with C in {16, 32} (pair_wino_impl.h); optional
    float4* d_wpq3 = nullptr;  // Winograd F(4,3)-transformed weights of the wide k = 3 pairs, C -> C with C in {64, 128}: (32-row tile) x chunk x 6 fragments (pair_wino4_impl.h); optional
    void* d_wph16 = nullptr;   // f16x3 mode, 16 -> 16 channel Conv1d: (wh, wl) planes of the two-samples-per-row layout (pair16_f16x3.hip)
    void* d_wph = nullptr;     // f16x3 mode: (wh, wl, wh * 2^-11) fp16 planes in 32x32x16 fragment order (optional)
    float w_scale = 1.f;       // s_w: power of two folded into those planes
    int nch16 = 0;
    int precision = FV_PRECISION_F32;   // FV_PRECISION_F16X3: conv_layer_run uses the split-fp16 kernel (needs d_wph)
    int algo = FV_CONV_ALGO_AUTO;       // fv_conv_set_algorithm (single layers; an engine's layers follow the engine's setting)
    float* d_bias = nullptr;   // m_pad values, followed by their negatives (m_pad more)
    size_t wp_bytes = 0;

    // every device allocation of the layer, in one place: conv_layer_destroy walks this list (a buffer added above is added here too)
    template <class F>
    void for_each_buffer(F&& f) {
        f(d_wp), f(d_bias), f(d_wp16), f(d_wpw), f(d_wpw16), f(d_wpq16), f(d_wpw44), f(d_wpw4), f(d_wpwl), f(d_wpq3), f(d_wph), f(d_wph16);
    }

    int64_t out_len(int t_in) const {
        return transposed ? (int64_t)(t_in - 1) * stride - 2 * padding + k
                          : (int64_t)t_in + 2 * padding - (int64_t)dil * (k - 1);
    }
    // number of GEMM columns per item
    int64_t gemm_cols(int t_in) const {
        if (!transposed) return out_len(t_in);
        const int64_t tout = out_len(t_in);
        return (tout + padding + stride - 1) / stride;  // q in [0, ceil((Tout+pad)/u))
    }
};

// Builds the device-side layer from an already-folded torch-layout weight (host).  bias may be NULL.
// with_f16x3: also pack the split fp16 planes when the layer is eligible for the f16x3 kernels.
fv_status conv_layer_create(ConvLayer& L, bool transposed, int c_in, int c_out, int k, int dil, int padding,
                            int stride, const float* host_w, const float* host_bias, bool with_f16x3 = false);
void conv_layer_destroy(ConvLayer& L);

// do the specialised kernels of this tap count form the three-operand input mean themselves (ConvParams::x2 / x3)?  The tap counts
// of the polyphase transposed convs (the upsamplers): conv_mfma_impl.h instantiates SUM3 variants for exactly these
constexpr bool conv_sum3_supported(int ks) { return ks == 1 || ks == 2 || ks == 4; }

struct ConvRun {
    const float* x = nullptr;
    // the input is ((x + x2) + x3) / 3 when x2 / x3 are given (stack-mean of three branch outputs, formed by the conv's staging
    // where the kernel supports it, otherwise by mean_of_three_kernel into sum_tmp first)
    const float* x2 = nullptr;
    const float* x3 = nullptr;
    float* sum_tmp = nullptr;
    float* y = nullptr;
    const float* res = nullptr;
    const float* gamma = nullptr;
    int batch = 0, t_in = 0;
    int pre_act = FV_ACT_NONE, post_act = FV_ACT_NONE;
    float slope = 0.f;
    int out_mode = OUT_SET;
    float out_scale = 1.f;
};
fv_status conv_layer_run(const ConvLayer& L, const ConvRun& r, hipStream_t stream);

// Per-(kernel size) translation units (parallel builds): return false if (ks, dil) has no specialisation.
bool launch_conv_k1(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_k3(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_k7(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_k11(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_misc(const ConvParams& p, int cfg, int batch, hipStream_t s);   // k=2, 4, 5, 13 ...
bool launch_conv_generic(const ConvParams& p, int cfg, int batch, hipStream_t s, size_t* lds_bytes);
// f16x3 precision mode: tiles of the split-fp16 kernel (rows x columns per workgroup)
enum SplitCfg : int { SPLIT_128x128 = 0, SPLIT_64x256 = 1, SPLIT_32x256 = 2, SPLIT_COUNT };
bool launch_conv_f16x3_k1(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_f16x3_k3(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_f16x3_misc(const ConvParams& p, int cfg, int batch, hipStream_t s);   // k = 2, 4 (polyphase transposed convs)
bool launch_conv_f16x3_k7(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_f16x3_k11(const ConvParams& p, int cfg, int batch, hipStream_t s);

// Pointwise (k = 1) convs as a persistent fp32-MFMA GEMM without LDS (gemm_pw.hip).  p as for a flat conv launch
// (n_total = batch * N); pair: even T and 8-byte aligned tensors.  Returns the workgroup count (0: unknown configuration).
enum GemmPwCfg : int { GEMM_PW_64x64_W2 = 0, GEMM_PW_32x64_W3 = 1, GEMM_PW_COUNT };
int launch_gemm_pw(const ConvParams& p, int cfg, bool pair, hipStream_t s);

#ifndef FV_X_PAIRCOLS
#define FV_X_PAIRCOLS 2048   // round 3: 128-column tiles at C = 16 too (4096: 256 columns) — same B = 32 step, single-clip p50 -4 %
#endif
constexpr int kPairCols = FV_X_PAIRCOLS;   // c1 columns per workgroup x channels (LDS budget of the fused pair kernel)

// Fused ResBlock (c1, c2) pair for narrow stages: y = x + c2(silu(c1(silu(x))))  (resblock_pair.hip)
struct PairParams {
    const float* x;       // (B, C, T)
    const float4* w1;     // c1 packed weights (32x32x2 layout for C >= 32, 16x16x4 layout for C == 16)
    const float* b1;
    const float4* w2;
    const float* b2;
    const float* b1n;     // -b1 / -b2 (pair_wino_impl.h: the bias rides in two accumulator planes, one of them negated)
    const float* b2n;
    float* y;             // (B, C, T); must NOT alias x (neighbouring workgroups read x's halo)
    int T, n_tiles;
    int out_mode;
    float out_scale;
    int batch;            // items in the launch (the kernels map workgroups to (item, tile) themselves)
    int n_frag;           // pair_wino32_kernel: weight fragments per 32-row m-tile of w1 / w2 (nchunk * nv)
};
bool pair_supported(int C, int ks, int dil);

bool pair_f16x3_supported(const ConvLayer& c1, const ConvLayer& c2);   // wide SiLU pairs of the f16x3 precision mode
bool launch_resblock_pair(const PairParams& p, int C, int ks, int dil, int batch, hipStream_t s);
// Winograd F(2,3) form of the same pair (pair_wino_impl.h): p.w1 / p.w2 = the layers' d_wpw16; C in {16, 32}, dil in {1, 3, 5}
bool pair_wino_supported(int C, int ks, int dil);
bool launch_pair_wino_k3(const PairParams& p, int C, int dil, int batch, hipStream_t s);
bool launch_pair_wino_k7(const PairParams& p, int C, int dil, int batch, hipStream_t s);
bool launch_pair_wino_k11(const PairParams& p, int C, int dil, int batch, hipStream_t s);
// Winograd F(4,3) form of the wide k = 3 pairs (pair_wino4_impl.h): p.w1 / p.w2 = the layers' d_wpq3; C in {64, 128}, dil in {1, 3, 5}
bool launch_pair_wino4_k3(const PairParams& p, int C, int dil, int batch, hipStream_t s);
// ... and its tile width (final samples per workgroup): 32 (C = 128) or 64 (C = 64) quad columns of whole 4 D-sample blocks, less c2's halo
constexpr int pair_wino4_tile(int dil, int C) { return 4 * ((C == 128 ? 32 : 64) / dil * dil) - 2; }
// quad: the caller (the engine's pair branches, on launches that fill the chip) lets the wide k = 3 pairs take the F(4,3) family
fv_status conv_pair_run(const ConvLayer& c1, const ConvLayer& c2, const float* x, float* y, int batch, int t, int out_mode,
                        float out_scale, hipStream_t stream, bool quad = false);

// BigVGAN AMPBlock conv with its anti-aliased SnakeBeta fused in front (amp_conv.hip): y = conv(Activation1d(x)) + bias [+ res]
// for C_in = C_out in {32, 64}, k in {3, 7, 11}, 'same' padding; alpha / inv_beta / taps as for launch_aa_snake
bool amp_conv_supported(int C, int ks, int dil);
bool launch_amp_conv(const ConvLayer& L, const float* x, float* y, const float* res, const float* alpha, const float* inv_beta,
                     const float* up_taps, const float* down_taps, int batch, int t, int out_mode, float out_scale, hipStream_t s);

// Tile configurations (block = 4 waves): rows = WM*MT*32, cols = WN*NT*32.
// conv_mfma_splitk_direct_kernel (conv_mfma_impl.h): registers of one ring slot — 4 KS NT operands (x 3: SUM3) + KS weight float4s — decide the prefetch
// distance in chunks; 0 = the rings would spill and the launch stays on the LDS-staged split-K kernel.  Few-tap convs only (conv_pre, the polyphase
// upsamplers): every other single-clip conv is on the Winograd latency kernels.  KS = 4 — the k = 4, stride-2 upsampler at C = 128: four chunks, 2.7
// workgroups per CU — measured 21.1 us this way against 18.4 staged through LDS: with few chunks and several waves per SIMD the per-operand loads cost more
// issue than the barriers they replace.
constexpr int splitk_direct_pf(int ks, int nt, bool sum3) {
    const int r = 4 * ks * nt * (sum3 ? 3 : 1) + 4 * ks;
    return r <= 32 ? 3 : r <= 48 ? 2 : r <= 56 ? 1 : 0;
}
constexpr bool splitk_direct_shape(int ks, int dil, int nt, bool sum3) {
    return (ks == 1 || ks == 2 || ks == 7) && dil == 1 && splitk_direct_pf(ks, nt, sum3) > 0;
}

enum TileCfg : int { TILE_128x128 = 0, TILE_64x256 = 1, TILE_32x512 = 2, TILE_128x64 = 3, TILE_32x128 = 4, TILE_64x128 = 5, TILE_SPLITK_32x64 = 6, TILE_SPLITK_32x32 = 7, TILE_256x64 = 8, TILE_256x32 = 9, TILE_128x96 = 10, TILE_COUNT };
void tile_dims(int cfg, int* m_blk, int* n_blk);
// conv_wino_impl.h: Winograd F(2,3) variant of the dilated "same" convs; tiles = output rows x output PAIRS per workgroup
// (two-n-tile variants — 128 x 64 and 64 x 128 pairs, 128 accumulator registers, two waves per SIMD — measured 8 % slower: LOG R3.16)
enum WinoCfg : int { WINO_128x32 = 0, WINO_64x64 = 1, WINO_32x128 = 2, WINO_COUNT };
// p.wp = the layer's d_wpw, p.n_tiles in pair columns
bool launch_conv_wino_k3(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_wino_k7(const ConvParams& p, int cfg, int batch, hipStream_t s);
bool launch_conv_wino_k11(const ConvParams& p, int cfg, int batch, hipStream_t s);
// conv_wino4_impl.h: F(4,3) tap groups (k = 7 / 11), 64 rows x 32 quad columns per workgroup; p.wp = the layer's d_wpw4, p.m_blks = M / 64, p.n_tiles over quad columns
bool have_conv_wino4();   // false in the shipped library (make ABPARTNERS=1 builds the F(4,3) kernels: conv_wino4_k{7,11}.hip / abpartner_stubs.hip)
bool launch_conv_wino4_k7(const ConvParams& p, int batch, hipStream_t s);
bool launch_conv_wino4_k11(const ConvParams& p, int batch, hipStream_t s);
// conv_wino44_impl.h: F(4,4) tap groups, 64 rows x 32 quad columns per workgroup; p.wp = the layer's d_wpw44, p.m_blks = M / 64, p.n_tiles over quad columns
bool launch_pair_wino44_k7(const PairParams& p, int C, int dil, int batch, hipStream_t s);
bool launch_pair_wino44_k11(const PairParams& p, int C, int dil, int batch, hipStream_t s);
bool launch_conv_wino44_k7(const ConvParams& p, int rows, int batch, hipStream_t s);
bool launch_conv_wino44_k11(const ConvParams& p, int rows, int batch, hipStream_t s);
// conv_wino_lat_impl.h: latency variant (16 rows x 16 nt pairs per workgroup, K split over the four waves); p.wp = the layer's d_wpwl,
// p.m_blks = C / 16, p.n_tiles in units of 16 nt pair columns
bool launch_conv_wino_lat_k3(const ConvParams& p, int nt, int batch, hipStream_t s);
bool launch_conv_wino_lat_k7(const ConvParams& p, int nt, int batch, hipStream_t s);
bool launch_conv_wino_lat_k11(const ConvParams& p, int nt, int batch, hipStream_t s);
// conv_wino_lat44_impl.h: the same on F(4,4) tap groups (16 or 32 rows x 16 quad columns per workgroup); p.wp = the layer's d_wpq16, p.m_blks = C / rows,
// p.n_tiles in units of 16 quad columns
bool launch_conv_wino_lat44_k7(const ConvParams& p, int rows, int batch, hipStream_t s);
bool launch_conv_wino_lat44_k11(const ConvParams& p, int rows, int batch, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Small fused kernels (elementwise / narrow-output / reduction)
// ---------------------------------------------------------------------------------------------
// y[b][co][t] = post( bias[co] + sum_{ci,j} w[co][ci][j] * pre(x[b][ci][t + j - pad]) ), c_out <= 4 (conv_post).
// x2 / x3 (optional): the input is ((x + x2) + x3) / 3, formed while staging — only where conv_narrow_sum3_ok() says so
fv_status launch_conv_narrow(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int T,
                             int Cout, int k, int pad, int pre_act, int post_act, float slope, hipStream_t s,
                             const float* x2 = nullptr, const float* x3 = nullptr);
bool conv_narrow_sum3_ok(int B, int Cin, int T, int Cout, int k, int pad);

// Anti-aliased SnakeBeta: y = down2(snake(up2(x))) with 12-tap kaiser-sinc filters (alias_free_torch Activation1d).
// alpha_eff/inv_beta are per-channel, already exp()'d / inverted on the host.
// x2 / x3 (optional): the input is ((x + x2) + x3) / 3 (three branch outputs), formed while loading.
fv_status launch_aa_snake(const float* x, float* y, const float* alpha_eff, const float* inv_beta, const float* up_taps,
                          const float* down_taps, int B, int C, int T, hipStream_t s, const float* x2 = nullptr,
                          const float* x3 = nullptr);
// The form launch_aa_snake runs on these tensors: vec4_rows is the kernel's `vec4` argument, vec4 what the kernel then takes
struct AaSnakeForm {
    int vec4_rows = 0;
    bool vec4 = false, sum3 = false;
};
AaSnakeForm aa_snake_form(const float* x, const float* y, const float* x2, int T);
const char* aa_snake_form_name(const AaSnakeForm& f);   // "aa_snake<vec4>" | "aa_snake<pair>" [+ " sum3"]

// The kernel launch_dwconv_ln takes for a shape, and its name: "dwconv_ln_tile<k=7 cmax=512 ng=16>" | "dwconv_ln_reg<k=3>" | "dwconv_ln<k=7>"
struct DwlnForm {
    enum Kind { TILE, REG, GENERIC } kind = GENERIC;
    int k = 1, cmax = 0, ng = 0;
};
DwlnForm dwln_form(bool has_dw, int C, int T, int k);
void dwln_form_name(const DwlnForm& f, char* out, size_t cap);

// Depthwise conv (k taps, zero pad) + LayerNorm over channels, fused: y = LN_c(dwconv(x)) * w + b.
// With dw_w == NULL: plain channels-first LayerNorm.
fv_status launch_dwconv_ln(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                           float* y, int B, int C, int T, int k, float eps, hipStream_t s);

// The k = 7 form chunk by chunk (fv_cnxstream_*, cnx_stream_plan.h): one block's launch of a call.  Staged frames below in0 come from the
// block's ring (B, C, cap), the frames [in0, in1) from `chunk` (B, C, chunk_stride), frame in0 at column chunk_off, and are filed into the
// ring; h and xres, (B, C, out1 - out0), take the LayerNorm output and the block's input (its residual) at the columns [out0, out1).  The
// (CMAX, NG) instantiation for C is the whole-row launch's, and so is every column's arithmetic.  C <= 1024, C * cap < 2^28.
struct DwStreamRun {
    float* ring = nullptr;
    const float* chunk = nullptr;
    float *h = nullptr, *xres = nullptr;
    int cap = 0, chunk_stride = 0, chunk_off = 0;
    int in0 = 0, in1 = 0, out0 = 0, out1 = 0, tiles = 0;
};
fv_status launch_dwconv_ln_stream(const DwStreamRun& r, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, int B, int C,
                                  float eps, hipStream_t s);
// win (B, C, 6 + c) = the input frames [N0 - 6, N0 + c), zeros below frame 0: six from the input ring (B, C, cap), c from the caller's chunk
// (element (b, ci, t) at b * x_bstride + ci * x_rstride + t), which is filed into the ring
fv_status launch_cnx_stem_window(const float* chunk, long long x_bstride, long long x_rstride, float* ring, float* win, int B, int C, int cap,
                                 long long N0, int c, hipStream_t s);
// The pool form (fv_cnxpool_*): one block's launches of a step, kCnxPoolBlock entries per launch.  An entry is one item at one level:
// cnx_level_plan's values for its slot's (N0, N1, flush), the slot whose ring row (ring + slot * C * cap) it reads and files into, where frame
// in0 of its chunk lies (an element offset into `chunk`; chunk_stride elements between channels) and the column at which its outputs start in
// the packed (C, ostride) buffers h and xres.  A level-0 entry (launch_cnx_stem_pool_window) states the input frames: in0 = N0, in1 = N1.
struct CnxPoolEntry {
    int slot;
    int in0, in1, out0, out1, tiles;
    int chunk_base, out_col;
};
static constexpr int kCnxPoolBlock = 64;         // 64 entries of 32 bytes: the 2 KiB a table may take
using CnxPoolBlock = LaunchTable<CnxPoolEntry, kCnxPoolBlock>;
struct DwPoolRun {
    float* ring = nullptr;           // (sessions, C, cap)
    const float* chunk = nullptr;
    float *h = nullptr, *xres = nullptr;
    int cap = 0, chunk_stride = 0, ostride = 0;
};
// *launches (may be NULL) is incremented per launch; a block of the table in which no entry has a tile launches nothing
fv_status launch_dwconv_ln_pool(const DwPoolRun& r, const CnxPoolEntry* tab, int count, const float* dw_w, const float* dw_b, const float* ln_w,
                                const float* ln_b, int C, float eps, hipStream_t s, int* launches);
// win (count, C, Wmax): row i = the frames [N0_i - 6, N1_i) of entry i's session, then exact zeros to Wmax; the chunk row of item i is at
// chunk + i * x_istride, channel stride x_rstride, and is filed into the slot's row of ring (sessions, C, cap)
fv_status launch_cnx_stem_pool_window(const float* chunk, long long x_istride, long long x_rstride, float* ring, float* win, const CnxPoolEntry* tab,
                                      int count, int C, int cap, int Wmax, hipStream_t s, int* launches);

// x[b][c][t] += bias[c] + sum_j w[c][j] * template[b][t*stride + j - pad]  (use_template branch, hifigan.py:233-234)
fv_status launch_noise_conv_add(const float* tmpl, const float* w, const float* bias, float* x, int B, int C, int T, int Ta,
                                int k, int stride, int pad, hipStream_t s);

// Log-mel front-end glue (frame_kernels.hip, small_kernels.hip)
// yp[b][r][tp] = wave[b][reflect(tp*hop + r - pad_l)] (0 past the padded length): polyphase layout so that the STFT becomes
// a stride-1 conv with hop channels and n_fft/hop taps
fv_status launch_polyphase_reflect(const float* wave, float* yp, int B, int L, int hop, int TP, int pad_l, int pad_r, hipStream_t s);
// mag[b][k][t] = sqrt(re^2 + im^2 + 1e-6) from spec rows [0,nb) = Re, [nb,2nb) = Im
fv_status launch_magnitude(const float* spec, float* mag, int B, int nb, int T, hipStream_t s);

// ISTFT head glue: h (B, 2*n_fft, T) rows [0,nb) = log-mag, [n_fft, n_fft+nb) = phase -> spec (B, 2*nbp, T):
// long clips as a batch of equal-length time tiles (engine_windows.hip run_model); hop: frames -> samples of the tensor being moved
fv_status launch_gather_tiles(const float* x, float* tiles, int B, int C, int T, int n, int L, int stride, int hop, hipStream_t s);
fv_status launch_scatter_tiles(const float* tiles, float* y, int B, int C, int T, int n, int L, int stride, int halo, int hop, hipStream_t s);
// streaming synthesis (fv_stream_push): chunk -> ring + window; the emitted samples of the window's output -> the caller's buffer
fv_status launch_stream_window(const float* chunk, float* ring, float* win, int B, int C, long long cap, long long c0, long long n, long long w,
                               hipStream_t s);
fv_status launch_stream_crop(const float* y, float* out, int B, int C, long long Ly, long long a, long long len, hipStream_t s);
// ragged batches (fv_ragged_forward): windows [first, first + count) of the device table `tab` <-> one group's buffers; T / L: columns of a
// clip's row / of a window (frames x hop); the rows' tails past each clip's length zeroed
fv_status launch_ragged_gather(const float* x, float* win, const fv_ragged_window* tab, const int* lens, int first, int count, int C,
                               long long T, long long L, int hop, hipStream_t s);
fv_status launch_ragged_scatter(const float* win, float* y, const fv_ragged_window* tab, int first, int count, int C, long long T,
                                long long L, int hop, hipStream_t s);
fv_status launch_ragged_zero_tail(float* y, const int* lens, int B, int C, long long T, long long span, int hop, hipStream_t s);
// session pool (fv_pool_step): the step's tables are LaunchTables of kPoolBlock entries.  Entries count in frames; the launchers take `hop`
// (1 for the mel, the generator's hop for the pitch template and the waveform) and scale to columns.
static constexpr int kPoolBlock = 32;
struct PoolGatherEntry {
    int item, slot;       // row of the chunk buffer, row of the ring
    int row;              // row of the group's tensor; -1: no window in this launch, the chunk only goes into the ring
    int col0, W, n;       // first column of the window in the group's tensor, its length, the chunk's frames
    long long w, F;       // the window is the frames [w, w + W); F frames were received before this step
};
struct PoolCropEntry {
    int item, row;        // row of the caller's output; row of the group's output, -1: the item emits nothing (a row of zeros)
    long long src, len;   // out[item][c][j] = j < len ? y[row][c][src + j] : 0
};
using PoolGatherBlock = LaunchTable<PoolGatherEntry, kPoolBlock>;
using PoolCropBlock = LaunchTable<PoolCropEntry, kPoolBlock>;
// chunk (., C, in_frames) -> ring (., C, cap) at F mod cap, and ring + chunk -> win (rows, C, Wg), zero outside [col0, col0 + W)
fv_status launch_pool_gather(const float* chunk, float* ring, float* win, const PoolGatherEntry* tab, int count, int C, long long cap,
                             long long in_frames, long long Wg, int hop, hipStream_t s);
// y (rows, C, Ly) -> out (., C, out_frames): each entry's samples, then zeros to the row's end
// out_stride: columns between the rows of `out` (0: out_frames * hop, rows back to back)
fv_status launch_pool_crop(const float* y, float* out, const PoolCropEntry* tab, int count, int C, long long Ly, long long out_frames,
                           int hop, hipStream_t s, long long out_stride = 0);
// code rings (fv_stream_push_codes, fv_codepool_step; vq.hip, beside vq_gather_kernel): the twins of launch_stream_window / launch_pool_gather
// for a ring of codes — chunk (n_q, rows, n) int32 -> ring (rows, n_q, cap) int32, and win (rows, D, .) = fv_vq_decode's sum of the window's codes.
// vq_describe: what a code handle checks at creation (`fn` names the caller): a quantiser with every layer loaded -> its dim and n_q.
fv_status vq_describe(const char* fn, const fv_vq* vq, int* dim, int* n_q);
fv_status launch_stream_window_codes(const fv_vq* vq, const int* chunk, int* ring, float* win, int B, long long cap, long long c0, long long n,
                                     long long w, hipStream_t s);
fv_status launch_pool_gather_codes(const fv_vq* vq, const int* chunk, int* ring, float* win, const PoolGatherEntry* tab, int count, int items,
                                   long long cap, long long in_frames, long long Wg, hipStream_t s);
// sample streams (sample_stream.h): next[b][i] = sample next_origin + i of row b, i < count, where `N` samples have arrived before this call — from
// chunk[b][idx - N] at or after N, from prev[b][idx - prev_origin] before it, 0.0f before the utterance's start; prev and next are two buffers
// of row stride `stride`
fv_status launch_sample_carry(const float* prev, float* next, const float* chunk, long long stride, long long chunk_stride, int B, long long N,
                              long long next_origin, long long prev_origin, long long count, hipStream_t s);
// log-mel front-end on ragged rows and stream chunks (frame_kernels.hip; fv_logmel_ragged_forward, fv_logmel_stream_*): a LaunchTable of the
// rows' lengths or column counts, kLogmelRows rows per launch
static constexpr int kLogmelRows = 32;
using LogmelRowBlock = LaunchTable<long long, kLogmelRows>;
// yp[b][r][tp] = sample (f0 + tp) hop + r - pad_l of row b, reflected at 0 and — where row_len[b] >= 0 (row_len NULL: no row's end is known) — at
// the row's end, 0 past the padded row / from `avail` on; the sample is read from `chunk` (samples [chunk_origin, ...)) or from `carry`
// (samples [carry_origin, chunk_origin)); either may be NULL only when it holds no sample of any row (refused otherwise)
fv_status launch_logmel_window(const float* carry, long long carry_stride, long long carry_origin, const float* chunk, long long chunk_stride,
                               long long chunk_origin, const long long* row_len, long long avail, float* yp, int B, long long f0, int hop,
                               int TP, int pad_l, int pad_r, hipStream_t s);
// Per-session sample pools (sample_pool.h; fv_wavpool_step): every slot advances on its own, so origins, ends and the slot's carry buffer are
// per table entry of a LaunchTable, kSamplePoolBlock entries per launch.
static constexpr int kSamplePoolBlock = 32;
struct SamplePoolEntry {
    int item, slot;            // row of the chunk buffer; the slot's row in both carry buffers
    int bit;                   // the carried samples are in buf[bit]; a push writes buf[bit ^ 1]
    int count;                 // outputs (frames) of this row; slots past what they read are exact zeros
    long long carry_origin;    // N - H: the carry holds the samples [N - H, N)
    long long chunk_origin;    // N: the chunk holds the samples [N, avail)
    long long end;             // the utterance's end N2 when the item flushes, else -1
    long long avail;           // N2 = N + the item's samples
    long long first;           // E: the first output (frame) of this row
};
using SamplePoolBlock = LaunchTable<SamplePoolEntry, kSamplePoolBlock>;
// yp[k][r][tp] = sample (first_k + tp) hop + r - pad_l of entry k's session for the tp < count_k + taps - 1 slots its frames read, 0.0f in the
// other slots (nothing is loaded for them); reflected and cut off as launch_logmel_window does, per entry.  buf0 / buf1: the pool's two
// (S, H) carry buffers; chunk (., chunk_stride) may be NULL when no entry's chunk holds a sample.
fv_status launch_logmel_pool_window(const float* buf0, const float* buf1, long long H, const float* chunk, long long chunk_stride,
                                    const SamplePoolEntry* tab, int rows, float* yp, int hop, int TP, int taps, int pad_l, int pad_r,
                                    hipStream_t s);
// sample_carry per entry: buf[bit ^ 1][slot][i] = sample avail - H + i of the slot, i < H — from the chunk at or after chunk_origin, from
// buf[bit][slot] before it, 0.0f before the utterance's start.  Only the entries' slots are touched.
fv_status launch_sample_pool_carry(float* buf0, float* buf1, long long H, const float* chunk, long long chunk_stride,
                                   const SamplePoolEntry* tab, int count, hipStream_t s);
// y (B, C, T): columns >= row_cols[b] of row b set to 0.0f
fv_status launch_zero_columns(float* y, const long long* row_cols, int B, int C, long long T, hipStream_t s);
// rows [0,nb) = Re, [nbp, nbp+nb) = Im, zero padded to nbp = round_up(nb, 8)
fv_status launch_istft_spec(const float* h, float* spec, int B, int n_fft, int T, int nb, int nbp, hipStream_t s);
// frames (B, n_fft, T) (already windowed by the synthesis basis) -> overlap-add, crop, divide by the envelope (frame_kernels.hip).
fv_status launch_istft_ola(const float* frames, const float* inv_env, float* y, int B, int n_fft, int T, int hop, int pad, long long out_len,
                           hipStream_t s);
// the same sum for the samples [Y, Y2) of a stream, y (B, Y2 - Y): the frames [S, S + dS) from `frames` (B, n_fft, dS), the frames [S - G, S) from
// the carried `cfr` (B, n_fft, G); only frames in [0, Tend) exist
fv_status launch_istft_ola_window(const float* frames, const float* cfr, const float* win2, float* y, int B, int n_fft, int hop, int pad, int G,
                                  long long S, int dS, long long Tend, long long Y, long long Y2, hipStream_t s);
// nfr (B, n_fft, G) = the frames [S + dS - G, S + dS) of the same two pieces, 0 before frame 0
fv_status launch_pv_frame_carry(const float* frames, const float* cfr, float* nfr, int B, int n_fft, int G, long long S, int dS, hipStream_t s);
// the pitch shift's frames: yp[b][r][tp] = wave[b][tp hop + r - pad] inside [0, L), else 0 ...
fv_status launch_pv_frame(const float* wave, long long x_stride, float* yp, int B, long long L, int hop, int TP, int pad, hipStream_t s);
// ... and for the frames from f0 on of a stream: sample (f0 + tp) hop + r - pad, 0 before sample 0 and from `end` on; `carry` holds the samples
// [N - H, N), `chunk` the samples [N, end)
fv_status launch_pv_frame_window(const float* carry, long long carry_stride, const float* chunk, long long chunk_stride, float* yp, int B,
                                 long long N, int H, long long end, long long f0, int hop, int TP, int pad, hipStream_t s);

// The pitch-shift pool's forms (fv_pvpool_step): tensor row k of each launch is one table entry.  The window takes SamplePoolEntry with
// first = A and count = dA: yp[k][r][tp] = sample (A_k + tp) hop + r - pad of the entry's session for tp < dA_k + taps - 1, zeros before sample 0
// and from avail on, 0.0f in the other slots.
fv_status launch_pv_frame_pool_window(const float* buf0, const float* buf1, long long H, const float* chunk, long long chunk_stride,
                                      const SamplePoolEntry* tab, int rows, float* yp, int hop, int TP, int taps, int pad, hipStream_t s);
struct PvOlaEntry {
    int slot, fbit;            // the slot's carried frames [S - G, S) are in fr[fbit]; an entry with dS > 0 writes fr[fbit ^ 1]
    int dS, pad_;              // frames [S, S + dS) of this row are new
    long long S, Tend;         // only frames in [0, Tend) exist
    long long Y, Y2;           // the stretched samples this row emits
};
using PvOlaBlock = LaunchTable<PvOlaEntry, kSamplePoolBlock>;
// launch_istft_ola_window and launch_pv_frame_carry per entry: frames (rows, n_fft, ld), y (rows, y_stride) receives the samples [Y, Y2) of each
// entry; fr0 / fr1: the pool's two (S, n_fft, G) frame carries
fv_status launch_pv_pool_ola(const float* frames, float* fr0, float* fr1, const float* win2, float* y, const PvOlaEntry* tab, int rows, int n_fft,
                             int hop, int pad, int G, int ld, long long y_stride, hipStream_t s);

// The DFT bases the STFT / ISTFT convs are built from (engine_build.hip): the log-mel front-end, the ISTFT head and the pitch shift share them.
// stft_basis: the window-folded real DFT in polyphase form, a (2 nb, hop, taps) conv weight — rows [0, nb) win[n] cos, [nb, 2 nb) -win[n] sin at
// n = q hop + r, zero for n >= N.  istft_basis: the windowed inverse real DFT, an (N, 2 nb) pointwise weight — c_k cos / N win[n] | -c_k sin / N win[n].
std::vector<float> stft_basis(const std::vector<float>& win, int N, int hop, int taps);
std::vector<float> istft_basis(const std::vector<float>& win, int N);
// resample.hip: the outputs [0, m_end) of `batch` rows of `len` samples through r's kernel, unchecked (pitch_shift.hip)
fv_status resample_rows(const fv_resample* r, const char* fn, const float* x, long long x_stride, long long len, float* y, long long y_stride,
                        int batch, long long m_end, hipStream_t s);
// resample.hip: what a stream on r has emitted once N input samples have arrived (fv_resample_stream_push's rule), and Kp, the longest band
long long resample_emit_count(const fv_resample* r, long long N);
int resample_band_taps(const fv_resample* r);
// resample.hip: the host half of a resampler — the design's sizes and the emission rule, no device table (fv_pvpool_plan); freed by
// fv_resample_destroy.  And fv_respool_max_outputs for a pool of `max_chunk` on r.
fv_status resample_rule_create(const fv_resample_config* cfg, const char* fn, fv_resample** out);
long long resample_pool_max_outputs(const fv_resample* r, int max_chunk);

// RefineGAN glue (small_kernels.hip): linear interpolation (nn.Upsample(mode="linear")) with optional leaky_relu, written into
// a channel slice of a wider tensor; channel-slice copy; AdaIN with caller-supplied noise
fv_status launch_leaky_interp(const float* x, float* y, int B, int C, int Lin, int Lout, float scale, int leaky, float slope,
                              int ctot, int coff, hipStream_t s);
fv_status launch_copy_channels(const float* x, float* y, int B, int C, int T, int ctot, int coff, hipStream_t s);
fv_status launch_mean_of_three(const float* a, const float* b, const float* c, float* y, long long n, hipStream_t s);   // ((a + b) + c) / 3
fv_status launch_adain(const float* x, const float* noise, const float* w, float* y, int B, int C, int T, float slope,
                       int accumulate, float scale, hipStream_t s);
// Seeded AdaIN noise (fv_refinegan_set_noise_seed): the sample is computed in the kernel from (seed, noise row, layer, channel, absolute position).
// Tensor row i is clip i / n (noise row first_row + i / n) at sample origin origin0 + min((i % n) * stride, last), all in samples at the
// launch's own rate (TilePlan::start's rule; n = 1 for a whole forward and a stream window).
struct SeededNoise {
    unsigned long long seed = 0;
    int first_row = 0, n = 1;
    long long origin0 = 0, stride = 0, last = 0;
};
fv_status launch_adain_seeded(const float* x, const float* w, float* y, int B, int C, int T, float slope, int accumulate, float scale,
                              const SeededNoise& sn, int layer, hipStream_t s);
fv_status launch_refinegan_fill_noise(float* out, int B, int C, int T, const SeededNoise& sn, int layer, hipStream_t s);   // the explicit layout

}  // namespace fv
