// libfishvoc_hip.so — C ABI (include/fishvoc.h) and the model-level forward orchestration.
//
// The engine owns: folded + MFMA-packed weights in HBM, and the static launch plan of a generator forward.
// Per forward it only enqueues kernels on the caller's stream into the caller's workspace (no allocation, no sync).
//
// Reference call stack replaced (paths under /root/reference/fish_vocoder):
//   test.py:89 -> models/gan.py:286 -> modules/generators/hifigan.py:226-249 (HiFiGAN)
//                                       modules/generators/bigvgan.py:352-371 (BigVGAN)
//                                       modules/generators/unify.py:18-33 + encoders/convnext.py:206-214
//                                       + generators/vocos.py:43-69 (Vocos)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>

#include "fv_internal.h"

namespace fv {

static thread_local std::string g_err;
static thread_local std::string g_kernel;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
void set_last_kernel(const char* name) { g_kernel = name; }
static thread_local bool g_lds_refused = false;
bool dynamic_lds_refused() {   // true once after a failed ensure_dynamic_lds (lets the caller keep that error text)
    const bool r = g_lds_refused;
    g_lds_refused = false;
    return r;
}
bool ensure_dynamic_lds(const void* kernel, int bytes, unsigned long long* done_mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev >= 0 && dev < 64 && (__atomic_load_n(done_mask, __ATOMIC_ACQUIRE) >> dev & 1ull)) return true;
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d B) failed on device %d: %s", bytes, dev, hipGetErrorString(e));
        g_lds_refused = true;
        return false;
    }
    if (dev >= 0 && dev < 64) __atomic_fetch_or(done_mask, 1ull << dev, __ATOMIC_RELEASE);   // devices >= 64: set every time
    return true;
}
// The knob set is immutable once published: knobs() is one acquire load on the launch path, fv_reload_env() publishes a fresh
// copy (the old one is leaked on purpose — a concurrent forward may still be reading it; a harness reloads a handful of times)
static std::atomic<const Knobs*> g_knobs{nullptr};
static std::once_flag g_knobs_once;
static const Knobs* load_knobs() {
    Knobs* k = new Knobs();
    if (const char* v = std::getenv("FV_PW")) {
        const int n = std::atoi(v);
        k->pw = (v[0] == 'o' || n < 0 || n >= GEMM_PW_COUNT) ? -1 : n;
    }
    if (const char* v = std::getenv("FV_PW_PX")) k->pw_px = std::atoi(v);
    k->dwln_ng8 = std::getenv("FV_DWLN_NG8") != nullptr;
    k->dwln_rr = std::getenv("FV_DWLN_RR") != nullptr;
    k->old_dwln = std::getenv("FV_OLD_DWLN") != nullptr;
    if (const char* v = std::getenv("FV_WINO")) k->wino = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_MIN_M")) k->wino_min_m = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_CFG")) k->wino_cfg = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_MIN_BLOCKS")) k->wino_min_blocks = std::atoi(v);
    if (const char* v = std::getenv("FV_PAIR_WINO")) k->pair_wino = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO4")) k->wino4 = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO44")) k->wino44 = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO44_ROWS")) k->wino44_rows = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_LAT")) k->wino_lat = std::atoi(v);
    if (const char* v = std::getenv("FV_LAT_WINO44")) k->lat_wino44 = std::atoi(v);
    if (const char* v = std::getenv("FV_SPLITK_DIRECT")) k->splitk_direct = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO44_FLAT")) k->wino44_flat = std::atoi(v);
    if (const char* v = std::getenv("FV_VEC_STORE")) k->vec_store = std::atoi(v);
    if (const char* v = std::getenv("FV_PAIR_WINO44")) k->pair_wino44 = std::atoi(v);
    if (const char* v = std::getenv("FV_CONV_TILE")) {
        k->conv_tile = conv_tile_by_name(v);
        if (k->conv_tile < 0 && v[0]) std::fprintf(stderr, "fishvoc: FV_CONV_TILE=%s names no conv tile; ignored\n", v);
    }
    if (const char* v = std::getenv("FV_X_UPS_TILE256")) k->ups_tile256 = std::atoi(v);
    k->no_sum3 = std::getenv("FV_NO_SUM3") != nullptr;
    return k;
}
const Knobs& knobs() {
    const Knobs* k = g_knobs.load(std::memory_order_acquire);
    if (!k) {
        std::call_once(g_knobs_once, [] { g_knobs.store(load_knobs(), std::memory_order_release); });
        k = g_knobs.load(std::memory_order_acquire);
    }
    return *k;
}
static void reload_knobs() {
    (void)knobs();   // (the first-use initialisation has happened: nothing can overwrite the copy published below)
    g_knobs.store(load_knobs(), std::memory_order_release);
}

static thread_local int g_algo = FV_CONV_ALGO_AUTO;
static thread_local bool g_invariant = false;
AlgoScope::AlgoScope(int algo, bool invariant) : prev_algo(g_algo), prev_inv(g_invariant) {
    g_algo = algo;
    g_invariant = invariant;
}
AlgoScope::~AlgoScope() {
    g_algo = prev_algo;
    g_invariant = prev_inv;
}
int cur_algo() { return g_algo; }
bool cur_invariant() { return g_invariant; }

int num_cus() {
    static thread_local int cached_dev = -1, cached = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != cached_dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached = n;
        cached_dev = dev;
    }
    return cached;
}

static thread_local Profiler* g_prof = nullptr;
Profiler* current_profiler() { return g_prof; }
int prof_begin(hipStream_t s) {
    if (!g_prof) return -1;
    ProfRec r;
    if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return -1;
    (void)hipEventRecord(r.e0, s);
    g_prof->recs.push_back(r);
    return (int)g_prof->recs.size() - 1;
}
void prof_end(hipStream_t s, int idx, const char* label, double flops, double bytes) {
    if (!g_prof || idx < 0) return;
    ProfRec& r = g_prof->recs[idx];
    (void)hipEventRecord(r.e1, s);
    r.label = label;
    r.flops = flops;
    r.bytes = bytes;
}
// wraps a small-kernel launch expression with the profiler
#define FV_PROF(stream, label, flops, bytes, call)                      \
    do {                                                                \
        const int _pi = prof_begin(stream);                             \
        fv_status _st = (call);                                         \
        if (_pi >= 0) prof_end(stream, _pi, label, flops, bytes);       \
        if (_st) return _st;                                            \
    } while (0)

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

// alias_free_torch.kaiser_sinc_filter1d (third-party 0.0.6; restated from the published algorithm)
static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}
static std::vector<float> kaiser_sinc_filter(double cutoff, double half_width, int ks) {
    const bool even = ks % 2 == 0;
    const int half = ks / 2;
    const double delta_f = 4.0 * half_width;
    const double A = 2.285 * (half - 1) * M_PI * delta_f + 7.95;
    const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : (A >= 21.0 ? 0.5842 * std::pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
    std::vector<double> f(ks);
    double sum = 0.0;
    for (int n = 0; n < ks; ++n) {
        const double r = ks > 1 ? 2.0 * n / (ks - 1.0) - 1.0 : 0.0;
        const double win = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(beta);
        const double tm = even ? (n - half) + 0.5 : (double)(n - half);
        const double xs = 2.0 * cutoff * tm;
        const double sinc = xs == 0.0 ? 1.0 : std::sin(M_PI * xs) / (M_PI * xs);
        f[n] = 2.0 * cutoff * win * sinc;
        sum += f[n];
    }
    std::vector<float> out(ks);
    for (int n = 0; n < ks; ++n) out[n] = (float)(f[n] / sum);
    return out;
}

template <typename T>
static fv_status upload(const std::vector<T>& h, T** d) {
    FV_HIP_CHECK(hipMalloc((void**)d, std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) FV_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return FV_OK;
}

// ------------------------------------------------------------------------------------------------
struct AASnake {  // Activation1d(SnakeBeta(C, alpha_logscale=True))
    float* d_alpha = nullptr;    // exp(alpha)
    float* d_inv_beta = nullptr; // 1 / (exp(beta) + 1e-9)
    float* d_up = nullptr;
    float* d_down = nullptr;
    int C = 0;
    void destroy() {
        for (float* p : {d_alpha, d_inv_beta, d_up, d_down})
            if (p) (void)hipFree(p);
        d_alpha = d_inv_beta = d_up = d_down = nullptr;
    }
};

struct ResBranch {
    int k = 0;
    int dil[FV_MAX_DILATIONS] = {1, 1, 1};
    ConvLayer c1[FV_MAX_DILATIONS], c2[FV_MAX_DILATIONS];
    AASnake act[2 * FV_MAX_DILATIONS];  // BigVGAN only
};

struct UpStage {
    ConvLayer up;
    int ch = 0;
    // use_template: noise_convs[i] = Conv1d(1, ch, k, stride, pad) on the pitch template (hifigan.py:192-204)
    float *d_nw = nullptr, *d_nb = nullptr;
    int nk = 0, nstride = 1, npad = 0;
    std::vector<std::unique_ptr<ResBranch>> branches;
};

struct UpsamplerModel {
    bool bigvgan = false;
    fv_upsampler_config cfg{};
    ConvLayer conv_pre;
    std::vector<std::unique_ptr<UpStage>> stages;
    AASnake act_post;  // BigVGAN only
    float* d_wpost = nullptr;
    float* d_bpost = nullptr;
    int post_cin = 0;

    int64_t out_len(int t_in) const {
        int64_t t = conv_pre.out_len(t_in);
        for (auto& st : stages) t = st->up.out_len((int)t);
        return t;
    }
    // largest (C * T) of any intermediate activation, per batch item
    int64_t max_elems(int t_in) const {
        int64_t t = conv_pre.out_len(t_in);
        int64_t m = (int64_t)conv_pre.c_out * t;
        for (auto& st : stages) {
            t = st->up.out_len((int)t);
            m = std::max<int64_t>(m, (int64_t)st->ch * t);
        }
        return m;
    }
    void destroy() {
        conv_layer_destroy(conv_pre);
        for (auto& st : stages) {
            conv_layer_destroy(st->up);
            if (st->d_nw) (void)hipFree(st->d_nw);
            if (st->d_nb) (void)hipFree(st->d_nb);
            for (auto& br : st->branches) {
                for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
                    conv_layer_destroy(br->c1[n]);
                    conv_layer_destroy(br->c2[n]);
                }
                for (auto& a : br->act) a.destroy();
            }
        }
        act_post.destroy();
        if (d_wpost) (void)hipFree(d_wpost);
        if (d_bpost) (void)hipFree(d_bpost);
        d_wpost = d_bpost = nullptr;
    }
};

struct CnxBlock {
    float *d_dw_w = nullptr, *d_dw_b = nullptr, *d_ln_w = nullptr, *d_ln_b = nullptr, *d_gamma = nullptr;
    ConvLayer pw1, pw2;
    int dim = 0;
};
struct CnxStage {
    // transition: i == 0: stem conv(k) then LN ; i > 0: LN then 1x1 conv
    ConvLayer conv;
    float *d_ln_w = nullptr, *d_ln_b = nullptr;
    int ln_dim = 0;
    std::vector<std::unique_ptr<CnxBlock>> blocks;
};
struct ConvNeXtModel {
    fv_convnext_config cfg{};
    std::vector<std::unique_ptr<CnxStage>> stages;
    float *d_norm_w = nullptr, *d_norm_b = nullptr;
    int out_dim() const { return cfg.dims[cfg.num_stages - 1]; }
    int max_dim() const {
        int m = cfg.input_channels;
        for (int i = 0; i < cfg.num_stages; ++i) m = std::max(m, cfg.dims[i]);
        return m;
    }
    void destroy() {
        for (auto& st : stages) {
            conv_layer_destroy(st->conv);
            for (float* p : {st->d_ln_w, st->d_ln_b})
                if (p) (void)hipFree(p);
            for (auto& b : st->blocks) {
                conv_layer_destroy(b->pw1);
                conv_layer_destroy(b->pw2);
                for (float* p : {b->d_dw_w, b->d_dw_b, b->d_ln_w, b->d_ln_b, b->d_gamma})
                    if (p) (void)hipFree(p);
            }
        }
        for (float* p : {d_norm_w, d_norm_b})
            if (p) (void)hipFree(p);
        stages.clear();
        d_norm_w = d_norm_b = nullptr;
    }
};

struct IstftHeadModel {
    fv_istft_head_config cfg{};
    ConvLayer out;    // 1x1 conv dim -> rows: only the 2*nb live rows are packed
    ConvLayer idft;   // (n_fft) x (2*nb) windowed inverse real-DFT basis as a 1x1 conv
    float* d_win2 = nullptr;
    int nb = 0;
    std::vector<float> win2;   // window^2 on the host: the envelope check of padding="center"
    bool center() const { return cfg.padding == FV_ISTFT_CENTER; }
    int64_t out_len(int T) const { return center() ? (int64_t)(T - 1) * cfg.hop_length : (int64_t)T * cfg.hop_length; }
    int crop() const { return center() ? cfg.n_fft / 2 : (cfg.win_length - cfg.hop_length) / 2; }
    // torch.istft(center=True) raises "window overlap add min" when the overlap-added window^2 is below 1e-11 anywhere in the samples
    // it keeps (vocos 0.0.2 ISTFT.forward falls back to it for padding="center").  The envelope's edge regions repeat for every T
    // beyond a few window lengths, so a short frame count decides it.
    // The answer depends only on min(T, Tc_max) and the fixed window: cached per value (it ran on every call, replayed ones too).
    mutable std::vector<signed char> env_ok_cache;   // by Tc: 0 unknown, 1 ok, -1 not ok (a forward holds the engine: no concurrent writers)
    bool center_envelope_ok(int T) const {
        const int N = cfg.n_fft, hop = cfg.hop_length;
        const int Tc_max = 2 * ((N + hop - 1) / hop) + 2;
        const int Tc = std::min(T, Tc_max);
        if (env_ok_cache.empty()) env_ok_cache.assign((size_t)Tc_max + 1, 0);
        if (Tc >= 0 && env_ok_cache[(size_t)Tc]) return env_ok_cache[(size_t)Tc] > 0;
        const bool ok = center_envelope_compute(Tc);
        if (Tc >= 0) env_ok_cache[(size_t)Tc] = ok ? 1 : -1;
        return ok;
    }
    bool center_envelope_compute(int Tc) const {
        const int N = cfg.n_fft, hop = cfg.hop_length;
        const int64_t L = (int64_t)(Tc - 1) * hop;
        for (int64_t q = 0; q < L; ++q) {
            const int64_t pos = q + N / 2;   // position in the un-trimmed overlap-add
            double env = 0.0;
            for (int64_t t = std::max<int64_t>(0, (pos - N + hop) / hop); t < Tc && t * hop <= pos; ++t)
                if (pos - t * hop < N) env += win2[(size_t)(pos - t * hop)];
            if (!(env >= 1e-11)) return false;
        }
        return true;
    }
    void destroy() {
        conv_layer_destroy(out);
        conv_layer_destroy(idft);
        if (d_win2) (void)hipFree(d_win2);
        d_win2 = nullptr;
    }
};

struct LogMelModel {
    fv_logmel_config cfg{};
    ConvLayer stft;   // (2*nb) x hop x (n_fft/hop): windowed real DFT in polyphase form (rows [0,nb) Re, [nb,2nb) Im)
    ConvLayer mel;    // n_mels x nb pointwise: slaney filterbank, epilogue log(clamp(., 1e-5))
    int nb = 0, taps = 0, pad_l = 0, pad_r = 0;
    int frames(int L) const { return 1 + (L + pad_l + pad_r - cfg.n_fft) / cfg.hop_length; }
    void destroy() {
        conv_layer_destroy(stft);
        conv_layer_destroy(mel);
    }
};

// RefineGANGenerator (refinegan.py:182-323): U-Net over the pitch template with the mel injected at the bottleneck.
struct RefineResBlock {   // refinegan.ResBlock (refinegan.py:38-110): both convs of a pair are dilated
    int k = 0, cin = 0, cout = 0;
    ConvLayer c1[3], c2[3];
    void destroy() {
        for (int n = 0; n < 3; ++n) {
            conv_layer_destroy(c1[n]);
            conv_layer_destroy(c2[n]);
        }
    }
};
struct RefineUp {         // nn.Upsample + ParallelResBlock (refinegan.py:130-179,262-273)
    int rate = 1, cin = 0, cskip = 0, cout = 0;
    ConvLayer input_conv;
    float* d_w1[3] = {nullptr, nullptr, nullptr};   // AdaIN weights before / after each branch's ResBlock
    float* d_w2[3] = {nullptr, nullptr, nullptr};
    RefineResBlock rb[3];
};
struct RefineModel {
    fv_refinegan_config cfg{};
    ConvLayer template_conv, mel_conv;
    std::vector<std::unique_ptr<RefineResBlock>> downs;
    std::vector<std::unique_ptr<RefineUp>> ups;
    float *d_wout = nullptr, *d_bout = nullptr;
    int out_cin = 0;
    void destroy() {
        conv_layer_destroy(template_conv);
        conv_layer_destroy(mel_conv);
        for (auto& d : downs) d->destroy();
        for (auto& u : ups) {
            conv_layer_destroy(u->input_conv);
            for (int j = 0; j < 3; ++j) {
                u->rb[j].destroy();
                if (u->d_w1[j]) (void)hipFree(u->d_w1[j]);
                if (u->d_w2[j]) (void)hipFree(u->d_w2[j]);
            }
        }
        if (d_wout) (void)hipFree(d_wout);
        if (d_bout) (void)hipFree(d_bout);
        d_wout = d_bout = nullptr;
        downs.clear();
        ups.clear();
    }
    // tensor lengths along the U: down[i] = length after i down-sampling steps (down[0] = T * hop), up[i] likewise upwards
    // from T.  nn.Upsample sizes its output as floor(L * scale_factor) in double (refinegan.py:229: scale_factor = 1 / rate).
    bool lengths(int T, std::vector<int64_t>& down, std::vector<int64_t>& up) const {
        const int S = cfg.num_stages;
        down.assign(S + 1, 0);
        up.assign(S + 1, 0);
        down[0] = (int64_t)T * cfg.hop_length;
        for (int i = 0; i < S; ++i) down[i + 1] = (int64_t)std::floor((double)down[i] * (1.0 / (double)cfg.downsample_rates[i]));
        up[0] = T;
        for (int i = 0; i < S; ++i) up[i + 1] = (int64_t)std::floor((double)up[i] * (double)cfg.upsample_rates[i]);
        if (down[S] != T) return false;                        // torch.cat([x, mel_conv(mel)]) needs equal lengths
        for (int i = 0; i < S; ++i)
            if (up[i + 1] != down[S - 1 - i]) return false;      // torch.cat([x, down]) (refinegan.py:314)
        return true;
    }
};

}  // namespace fv

using namespace fv;

struct fv_engine {
    fv_config cfg{};
    std::map<std::string, HostTensor> raw;
    std::set<std::string> used;
    bool finalized = false;
    UpsamplerModel ups;
    ConvNeXtModel cnx;
    IstftHeadModel head;
    LogMelModel mel;
    RefineModel refine;
    bool has_ups = false, has_cnx = false, has_head = false;
    Profiler prof;
    bool profiling = false;
    int precision = FV_PRECISION_F32;   // fv_set_precision
    int algo = FV_CONV_ALGO_AUTO;       // fv_set_conv_algorithm
    bool invariant = false;             // fv_set_batch_invariant
    void drop_graphs();
    bool fuse_pairs = true;   // FV_NO_PAIR_FUSION=1 in the environment disables the fused (c1, c2) kernels (A/B runs)
    bool post_mean_fused = true;   // FV_NO_POST_SUM3=1: mean_of_three_kernel before conv_post instead of the mean formed in its staging (A/B runs)
    int chain_max_c = 0;      // FV_CHAIN_MAX_C: stages this narrow accumulate the branch mean in the branches' last epilogues (ordered by events) instead of keeping three outputs
    int pair_max_c = 128;     // FV_PAIR_MAXC: widest stage whose (c1, c2) pairs fuse where a kernel exists (experiments)
    bool fuse_amp_convs = true;   // FV_NO_AMP_FUSION=1: BigVGAN's narrow stages run aa_snake + conv launches instead of amp_conv (A/B runs)
    // Measured in the step (BigVGAN-24k B = 64, interleaved, tools/ab_bigvgan.py): none 37.35 ms; k = 3 only 37.15; k <= 7 37.5; all 38.1.
    // Serialized, amp_conv equals conv + aa_snake within 5 % everywhere, but the separate activation pass is HBM-bound work that the
    // other branches' MFMA-bound convs overlap, while the fused one is VALU work inside an MFMA kernel (12 - 20 cycles of matrix
    // time per VALU instruction of a co-resident wave, tools/ubench/mfma_mix.hip) — so only the shortest convs fuse by default.
    // Round 6: with the unfused convs on Winograd tap groups the fused form lost its margin — BigVGAN-24k B = 64, interleaved: fused at C <= 64 25.98 - 26.04 ms,
    // at C = 32 only 25.85 - 25.93, nowhere 25.79 - 25.93 (profiles/r06v_bigvgan_amp_fusion.txt): C = 32 stays fused (its launches are the HBM-bound ones).
    int fuse_amp_max_c = 32, fuse_amp_max_k = 3;   // FV_AMP_MAXC / FV_AMP_MAXK override (experiments, tests)
    struct GraphKey {
        const void* in;
        void* out;
        void* ws;
        const void* tmpl;
        const void* noise;
        int batch, t_in;
        hipStream_t stream;
        bool operator==(const GraphKey& o) const {
            return in == o.in && out == o.out && ws == o.ws && tmpl == o.tmpl && noise == o.noise && batch == o.batch && t_in == o.t_in &&
                   stream == o.stream;
        }
    };
    struct GraphEntry {
        GraphKey key;
        hipGraph_t graph;
        hipGraphExec_t exec;
    };
    std::vector<GraphEntry> graphs;
    GraphKey last_key{};
    bool have_last = false;
    bool use_graph = true;        // FV_NO_GRAPH=1 disables hipGraph replay
    bool branch_streams = true;   // FV_SINGLE_STREAM=1 runs the ResBlock branches back to back on the caller's stream (the chain form of the branch mean)
    bool single_tree = false;     // FV_SINGLE_STREAM=2: one stream too, but the TREE form — the kernel instances of the shipped three-stream step, launch by launch (rocprofv3 / PMC passes: tools/probe_model.py)
    std::vector<hipStream_t> bstreams;   // nk-1 auxiliary streams (branch 0 runs on the caller's stream)
    hipStream_t null_capture = nullptr;   // calls on the legacy default stream: the launch sequence is captured here, the graph is launched on stream 0
    std::vector<hipEvent_t> bev_fork, bev_last;
    fv_status ensure_branch_streams(int nk);

    // ---- weight lookup helpers (reference state-dict names) ----
    const HostTensor* find(const std::string& name) {
        auto it = raw.find(name);
        if (it == raw.end()) return nullptr;
        used.insert(name);
        return &it->second;
    }
    fv_status need(const std::string& name, const std::vector<int64_t>& shape, const HostTensor** out,
                   bool allow_flat = false) {
        const HostTensor* t = find(name);
        if (!t) {
            set_error("missing weight '%s'", name.c_str());
            return FV_ERR_MISSING_WEIGHT;
        }
        int64_t n = 1;
        for (auto s : shape) n *= s;
        const bool same = t->shape == shape || (allow_flat && t->numel() == n);
        if (!same) {
            std::string got, want;
            for (auto s : t->shape) got += std::to_string(s) + ",";
            for (auto s : shape) want += std::to_string(s) + ",";
            set_error("weight '%s' has shape (%s), expected (%s)", name.c_str(), got.c_str(), want.c_str());
            return FV_ERR_SHAPE;
        }
        *out = t;
        return FV_OK;
    }
    // Folded conv weight: weight-norm g * v / ||v|| over all dims but 0 (torch._weight_norm(v, g, 0); for
    // ConvTranspose1d dim 0 is C_in — SURVEY §0.4), or a plain ".weight".
    // The lookup half (names, shapes: on the caller's thread, in state-dict order, so that error messages are deterministic) and the arithmetic half
    // (fold_weight: any thread) are separate since round 6: fv_finalize folds, packs and uploads the layers on all host cores (run_jobs).
    struct WeightRef {
        const HostTensor *g = nullptr, *v = nullptr, *plain = nullptr;
        int64_t n0 = 0, inner = 1;
    };
    fv_status conv_weight_ref(const std::string& prefix, const std::vector<int64_t>& shape, WeightRef& r) {
        r.n0 = shape[0];
        r.inner = 1;
        for (size_t i = 1; i < shape.size(); ++i) r.inner *= shape[i];
        std::string gk = prefix + ".parametrizations.weight.original0", vk = prefix + ".parametrizations.weight.original1";
        if (!raw.count(gk) && raw.count(prefix + ".weight_g")) {
            gk = prefix + ".weight_g";
            vk = prefix + ".weight_v";
        }
        if (raw.count(gk)) {
            fv_status st = need(gk, {r.n0}, &r.g, true);
            if (st) return st;
            return need(vk, shape, &r.v);
        }
        return need(prefix + ".weight", shape, &r.plain, true);
    }
    static void fold_weight(const WeightRef& r, std::vector<float>& w) {
        if (!r.g) {
            w = r.plain->data;
            return;
        }
        w.resize((size_t)r.n0 * r.inner);
        for (int64_t i = 0; i < r.n0; ++i) {
            const float* vi = r.v->data.data() + i * r.inner;
            double s = 0.0;
            for (int64_t j = 0; j < r.inner; ++j) s += (double)vi[j] * vi[j];
            const float scale = r.g->data[i] / (float)std::sqrt(s);
            for (int64_t j = 0; j < r.inner; ++j) w[i * r.inner + j] = vi[j] * scale;
        }
    }
    fv_status conv_weight(const std::string& prefix, const std::vector<int64_t>& shape, std::vector<float>& w) {
        WeightRef r;
        fv_status st = conv_weight_ref(prefix, shape, r);
        if (st) return st;
        fold_weight(r, w);
        return FV_OK;
    }
    // Deferred layer builds (fold -> fragment packing in up to three forms -> upload): queued by make_conv, run by run_jobs on the host's cores.  A job
    // touches only its own ConvLayer and tensors of `raw` (alive until fv_finalize clears it); `cost` orders the queue largest first.
    struct BuildJob {
        int64_t cost;
        std::function<fv_status()> fn;
    };
    std::vector<BuildJob> jobs;
    fv_status run_jobs();
    fv_status vec(const std::string& name, int64_t n, std::vector<float>& out) {
        const HostTensor* t;
        fv_status st = need(name, {n}, &t, true);
        if (st) return st;
        out = t->data;
        return FV_OK;
    }
    fv_status make_conv(ConvLayer& L, const std::string& prefix, bool transposed, int c_in, int c_out, int k, int dil,
                        int padding, int stride) {
        const std::vector<int64_t> shape = transposed ? std::vector<int64_t>{c_in, c_out, k} : std::vector<int64_t>{c_out, c_in, k};
        WeightRef r;
        fv_status st = conv_weight_ref(prefix, shape, r);
        if (st) return st;
        const HostTensor* bt;
        st = need(prefix + ".bias", {c_out}, &bt, true);
        if (st) return st;
        const int prec = precision;
        ConvLayer* Lp = &L;   // (owned by a unique_ptr'd stage / a member of the engine: the address is stable)
        jobs.push_back({(int64_t)c_in * c_out * k, [=]() -> fv_status {
                            std::vector<float> w;
                            fold_weight(r, w);
                            const fv_status s2 = conv_layer_create(*Lp, transposed, c_in, c_out, k, dil, padding, stride, w.data(), bt->data.data(),
                                                                   prec == FV_PRECISION_F16X3);
                            Lp->precision = prec;
                            return s2;
                        }});
        return FV_OK;
    }
    fv_status make_dev_vec(const std::string& name, int64_t n, float** d) {
        std::vector<float> v;
        fv_status st = vec(name, n, v);
        if (st) return st;
        return upload(v, d);
    }
    fv_status make_aasnake(AASnake& a, const std::string& prefix, int C) {
        std::vector<float> al, be;
        fv_status st = vec(prefix + ".act.alpha", C, al);
        if (st) return st;
        if (find(prefix + ".act.beta")) {   // SnakeBeta (bigvgan.py:74-135)
            st = vec(prefix + ".act.beta", C, be);
            if (st) return st;
        } else {
            be = al;                        // Snake (bigvgan.py:18-71): x + sin^2(alpha x) / alpha, one parameter per channel
        }
        for (int c = 0; c < C; ++c) {  // alpha_logscale=True (bigvgan.py:128-133,229,336)
            al[c] = std::exp(al[c]);
            be[c] = 1.0f / (std::exp(be[c]) + 0.000000001f);
        }
        std::vector<float> up = kaiser_sinc_filter(0.25, 0.3, 12), down = up;
        if (const HostTensor* t = find(prefix + ".upsample.filter")) {
            if (t->numel() != 12) {
                set_error("'%s.upsample.filter' must have 12 taps", prefix.c_str());
                return FV_ERR_SHAPE;
            }
            up = t->data;
        }
        if (const HostTensor* t = find(prefix + ".downsample.lowpass.filter")) {
            if (t->numel() != 12) {
                set_error("'%s.downsample.lowpass.filter' must have 12 taps", prefix.c_str());
                return FV_ERR_SHAPE;
            }
            down = t->data;
        }
        a.C = C;
        if ((st = upload(al, &a.d_alpha))) return st;
        if ((st = upload(be, &a.d_inv_beta))) return st;
        if ((st = upload(up, &a.d_up))) return st;
        return upload(down, &a.d_down);
    }

    fv_status build_upsampler(const std::string& pfx, bool bigvgan);
    fv_status build_convnext(const std::string& pfx);
    fv_status build_head(const std::string& pfx);
    fv_status build_logmel(const std::string& pfx);
    fv_status run_logmel(const float* d_in, float* d_out, int B, int L, float* ws, hipStream_t s);

    fv_status build_refinegan();
    fv_status run_refinegan(const float* d_mel, float* d_out, int B, int T, float* ws, hipStream_t s);
    const float* cur_noise = nullptr;      // set by fv_forward_refinegan for the duration of one call
    fv_status run_model(const float* d_in, float* d_out, int batch, int t_in, float* ws, hipStream_t s);
    fv_status run_model_whole(const float* d_in, float* d_out, int batch, int t_in, float* ws, hipStream_t s);
    // Long clips: time tiles with halo recompute, run as a BATCH of tiles (SURVEY §5 long-context row; VERDICT r4 missing 3)
    struct TilePlan {
        int n = 1;        // tiles per clip (1: the clip runs whole)
        int L = 0;        // frames per tile, halo included (every tile has the same length: one batched forward)
        int halo = 0;     // frames at a tile's inner edges whose outputs are discarded (>= the model's one-sided reach)
        int stride = 0;   // L - 2 * halo: frames a regular tile contributes
        int start(int i, int T) const { return std::min(i * stride, T - L); }
        int lo(int i) const { return i == 0 ? 0 : (i - 1) * stride + L - halo; }            // first clip frame tile i contributes
        int hi(int i, int T) const { return i + 1 == n ? T : i * stride + L - halo; }      // one past its last
    };
    int reach_frames() const;
    int frame_hop(int t_a, int t_b, const char** why) const;
    int tile_frame_limit() const;
    TilePlan tile_plan(int t_in) const;
    int tile_frames_override = 0;   // FV_TILE_FRAMES: tile length in frames (tests / experiments); 0 = only when the addressing span needs it
    fv_status run_upsampler(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s);
    const float* cur_template = nullptr;   // set by fv_forward_template for the duration of one call
    fv_status run_convnext(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s);
    fv_status run_head(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s);

    ~fv_engine() {
        for (auto& g : graphs) {
            (void)hipGraphExecDestroy(g.exec);
            (void)hipGraphDestroy(g.graph);
        }
        for (auto st : bstreams) (void)hipStreamDestroy(st);
        if (null_capture) (void)hipStreamDestroy(null_capture);
        for (auto e : bev_fork) (void)hipEventDestroy(e);
        for (auto e : bev_last) (void)hipEventDestroy(e);
        ups.destroy();
        cnx.destroy();
        head.destroy();
        mel.destroy();
        refine.destroy();
    }
};

static int get_padding(int k, int d = 1) { return (k * d - d) / 2; }  // hifigan.py:21-22
// RefineGAN builds AdaIN(channels=...) without forwarding the generator's slope (refinegan.py:157,165): always 0.2
constexpr float kAdaINSlope = 0.2f;

// Engine creation is the latency of the reference's one-shot caller (test.py:31-38: build, load, ONE forward per file): the weight-norm fold and the
// fragment packing of HiFiGAN-V1's 97 convs took ~95 ms on one host thread (profiles/r06a_engine_create_probe.txt).  The layers are independent: worker
// threads take them largest first.  FV_BUILD_THREADS=1 is the serial path (A/B, debugging).
fv_status fv_engine::run_jobs() {
    if (jobs.empty()) return FV_OK;
    std::stable_sort(jobs.begin(), jobs.end(), [](const BuildJob& a, const BuildJob& b) { return a.cost > b.cost; });
    int nt = (int)std::thread::hardware_concurrency();
    if (const char* v = std::getenv("FV_BUILD_THREADS")) nt = std::atoi(v);
    nt = std::max(1, std::min({nt, 32, (int)jobs.size()}));
    if (nt == 1) {
        for (auto& j : jobs)
            if (fv_status st = j.fn()) return st;
        return FV_OK;
    }
    int dev = 0;
    FV_HIP_CHECK(hipGetDevice(&dev));
    std::atomic<size_t> next{0};
    std::atomic<int> failed{FV_OK};
    std::mutex mu;
    std::string first_error;
    auto work = [&]() {
        if (hipSetDevice(dev) != hipSuccess) {   // (the current device is per thread)
            failed = FV_ERR_HIP;
            return;
        }
        for (size_t i; failed == FV_OK && (i = next.fetch_add(1)) < jobs.size();) {
            const fv_status st = jobs[i].fn();
            if (st) {
                std::lock_guard<std::mutex> lk(mu);
                if (failed == FV_OK) {
                    failed = st;
                    first_error = g_err;   // this worker's thread-local message: handed to the caller's thread below
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (failed != FV_OK) {
        set_error("%s", first_error.empty() ? "a layer build failed on a worker thread" : first_error.c_str());
        return (fv_status)failed.load();
    }
    return FV_OK;
}

fv_status fv_engine::build_upsampler(const std::string& pfx, bool bigvgan) {
    const fv_upsampler_config& c = cfg.ups;
    ups.cfg = c;
    ups.bigvgan = bigvgan;
    fv_status st;
    const int c0 = c.upsample_initial_channel;
    if ((st = make_conv(ups.conv_pre, pfx + "conv_pre", false, c.num_mels, c0, c.pre_conv_kernel_size, 1,
                        get_padding(c.pre_conv_kernel_size), 1)))
        return st;
    int ch = c0;
    for (int i = 0; i < c.num_upsamples; ++i) {
        const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
        const int cin = c0 >> i;
        ch = c0 >> (i + 1);
        if (ch < 1) {
            set_error("upsample_initial_channel=%d too small for %d upsampling stages", c0, c.num_upsamples);
            return FV_ERR_INVALID;
        }
        auto stg = std::make_unique<UpStage>();
        stg->ch = ch;
        if ((st = make_conv(stg->up, pfx + "ups." + std::to_string(i), true, cin, ch, k, 1, (k - u) / 2, u))) return st;
        if (c.use_template) {
            int s_f0 = 1;
            for (int q = i + 1; q < c.num_upsamples; ++q) s_f0 *= c.upsample_rates[q];
            const bool last_stage = i + 1 == c.num_upsamples;
            stg->nk = last_stage ? 1 : 2 * s_f0;
            stg->nstride = last_stage ? 1 : s_f0;
            stg->npad = last_stage ? 0 : s_f0 / 2;
            const std::string np_ = pfx + "noise_convs." + std::to_string(i);
            const HostTensor* t;
            if ((st = need(np_ + ".weight", {ch, 1, stg->nk}, &t, true))) return st;
            if ((st = upload(t->data, &stg->d_nw))) return st;
            if ((st = make_dev_vec(np_ + ".bias", ch, &stg->d_nb))) return st;
        }
        for (int j = 0; j < c.num_kernels; ++j) {
            auto br = std::make_unique<ResBranch>();
            br->k = c.resblock_kernel_sizes[j];
            // HiFiGAN: resblocks.{i}.blocks.{j}  (hifigan.py:206-211);  BigVGAN: flat resblocks.{i*nk+j} (bigvgan.py:327-332)
            const std::string bp = bigvgan ? pfx + "resblocks." + std::to_string(i * c.num_kernels + j)
                                           : pfx + "resblocks." + std::to_string(i) + ".blocks." + std::to_string(j);
            for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
                const int d = c.resblock_dilation_sizes[j][n];
                br->dil[n] = d;
                if ((st = make_conv(br->c1[n], bp + ".convs1." + std::to_string(n), false, ch, ch, br->k, d,
                                    get_padding(br->k, d), 1)))
                    return st;
                if ((st = make_conv(br->c2[n], bp + ".convs2." + std::to_string(n), false, ch, ch, br->k, 1,
                                    get_padding(br->k, 1), 1)))
                    return st;
            }
            if (bigvgan)
                for (int m = 0; m < 2 * FV_MAX_DILATIONS; ++m)
                    if ((st = make_aasnake(br->act[m], bp + ".activations." + std::to_string(m), ch))) return st;
            stg->branches.push_back(std::move(br));
        }
        ups.stages.push_back(std::move(stg));
    }
    if (bigvgan && (st = make_aasnake(ups.act_post, pfx + "activation_post", ch))) return st;
    // conv_post: (1, ch, k) -> narrow VALU kernel, plain layout
    std::vector<float> w, b;
    if ((st = conv_weight(pfx + "conv_post", {1, ch, c.post_conv_kernel_size}, w))) return st;
    if ((st = vec(pfx + "conv_post.bias", 1, b))) return st;
    ups.post_cin = ch;
    if ((st = upload(w, &ups.d_wpost))) return st;
    if ((st = upload(b, &ups.d_bpost))) return st;
    has_ups = true;
    return FV_OK;
}

fv_status fv_engine::build_convnext(const std::string& pfx) {
    const fv_convnext_config& c = cfg.backbone;
    cnx.cfg = c;
    fv_status st;
    const int ks = c.kernel_size;
    for (int i = 0; i < c.num_stages; ++i) {
        auto stg = std::make_unique<CnxStage>();
        const std::string dp = pfx + "downsample_layers." + std::to_string(i);
        if (i == 0) {  // stem: Conv1d(k, pad k//2) + LN_cf (convnext.py:164-174)
            if ((st = make_conv(stg->conv, dp + ".0", false, c.input_channels, c.dims[0], ks, 1, ks / 2, 1))) return st;
            stg->ln_dim = c.dims[0];
            if ((st = make_dev_vec(dp + ".1.weight", c.dims[0], &stg->d_ln_w))) return st;
            if ((st = make_dev_vec(dp + ".1.bias", c.dims[0], &stg->d_ln_b))) return st;
        } else {  // LN_cf + 1x1 conv (convnext.py:177-182)
            stg->ln_dim = c.dims[i - 1];
            if ((st = make_dev_vec(dp + ".0.weight", c.dims[i - 1], &stg->d_ln_w))) return st;
            if ((st = make_dev_vec(dp + ".0.bias", c.dims[i - 1], &stg->d_ln_b))) return st;
            if ((st = make_conv(stg->conv, dp + ".1", false, c.dims[i - 1], c.dims[i], 1, 1, 0, 1))) return st;
        }
        const int dim = c.dims[i];
        for (int j = 0; j < c.depths[i]; ++j) {
            auto blk = std::make_unique<CnxBlock>();
            blk->dim = dim;
            const std::string bp = pfx + "stages." + std::to_string(i) + "." + std::to_string(j);
            std::vector<float> w;
            const HostTensor* t;
            if ((st = need(bp + ".dwconv.weight", {dim, 1, ks}, &t, true))) return st;
            if ((st = upload(t->data, &blk->d_dw_w))) return st;
            if ((st = make_dev_vec(bp + ".dwconv.bias", dim, &blk->d_dw_b))) return st;
            if ((st = make_dev_vec(bp + ".norm.weight", dim, &blk->d_ln_w))) return st;
            if ((st = make_dev_vec(bp + ".norm.bias", dim, &blk->d_ln_b))) return st;
            // nn.Linear(dim, 4*dim) weight (4*dim, dim) == Conv1d weight (4*dim, dim, 1)  (convnext.py:111-115)
            if ((st = make_conv(blk->pw1, bp + ".pwconv1", false, dim, 4 * dim, 1, 1, 0, 1))) return st;
            if ((st = make_conv(blk->pw2, bp + ".pwconv2", false, 4 * dim, dim, 1, 1, 0, 1))) return st;
            if (raw.count(bp + ".gamma"))
                if ((st = make_dev_vec(bp + ".gamma", dim, &blk->d_gamma))) return st;
            stg->blocks.push_back(std::move(blk));
        }
        cnx.stages.push_back(std::move(stg));
    }
    const int last = c.dims[c.num_stages - 1];
    if ((st = make_dev_vec(pfx + "norm.weight", last, &cnx.d_norm_w))) return st;
    if ((st = make_dev_vec(pfx + "norm.bias", last, &cnx.d_norm_b))) return st;
    has_cnx = true;
    return FV_OK;
}

fv_status fv_engine::build_head(const std::string& pfx) {
    const fv_istft_head_config& c = cfg.head;
    head.cfg = c;
    const int N = c.n_fft, nb = N / 2 + 1;
    head.nb = nb;
    fv_status st;
    // out: Conv1d(dim, 2*n_fft, 1); keep rows [0, nb) (log-magnitude) and [n_fft, n_fft + nb) (phase): the other
    // bins are discarded by irfft (vocos.py:40-41,57).  Packed as a 2*nb-row layer.
    const HostTensor *w, *b;
    if ((st = need(pfx + "out.weight", {2 * N, c.dim, 1}, &w, true))) return st;
    if ((st = need(pfx + "out.bias", {2 * N}, &b))) return st;
    std::vector<float> wl((size_t)2 * nb * c.dim), bl(2 * nb);
    for (int r = 0; r < nb; ++r) {
        std::copy_n(w->data.data() + (size_t)r * c.dim, c.dim, wl.data() + (size_t)r * c.dim);
        std::copy_n(w->data.data() + (size_t)(N + r) * c.dim, c.dim, wl.data() + (size_t)(nb + r) * c.dim);
        bl[r] = b->data[r];
        bl[nb + r] = b->data[N + r];
    }
    if ((st = conv_layer_create(head.out, false, c.dim, 2 * nb, 1, 1, 0, 1, wl.data(), bl.data()))) return st;
    // window: checkpoint buffer "istft.window" if present, else torch.hann_window(win) (periodic)
    std::vector<float> win(c.win_length);
    if (const HostTensor* t = find(pfx + "istft.window")) {
        if (t->numel() != c.win_length) {
            set_error("'%sistft.window' has %lld taps, expected %d", pfx.c_str(), (long long)t->numel(), c.win_length);
            return FV_ERR_SHAPE;
        }
        win = t->data;
    } else {
        for (int n = 0; n < c.win_length; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / c.win_length));
    }
    // windowed inverse real DFT as a (n_fft) x (2 nb) matrix: frame[n] = win[n]/N * sum_k c_k (Re_k cos - Im_k sin),
    // c_0 = c_{N/2} = 1, else 2  == torch.fft.irfft(S, n_fft, norm="backward") * window  (vocos ISTFT, restated)
    std::vector<float> basis((size_t)N * 2 * nb);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < nb; ++k) {
            const double ck = (k == 0 || k == N / 2) ? 1.0 : 2.0;
            const double ang = 2.0 * M_PI * (double)(((int64_t)k * n) % N) / N;
            basis[(size_t)n * 2 * nb + k] = (float)(ck * std::cos(ang) / N * win[n]);
            basis[(size_t)n * 2 * nb + nb + k] = (float)(-ck * std::sin(ang) / N * win[n]);
        }
    if ((st = conv_layer_create(head.idft, false, 2 * nb, N, 1, 1, 0, 1, basis.data(), nullptr))) return st;
    std::vector<float> win2(N);
    for (int n = 0; n < N; ++n) win2[n] = win[n] * win[n];
    if ((st = upload(win2, &head.d_win2))) return st;
    head.win2 = win2;
    has_head = true;
    return FV_OK;
}

// ------------------------------------------------------------------------------------------------
// forward passes
// ------------------------------------------------------------------------------------------------
// Workspace of the upsampler: cur / S / Y plus (XB, XT, XA) per concurrent branch = 3 + 3 * num_kernels buffers

fv_status fv_engine::ensure_branch_streams(int nk) {
    if ((int)bstreams.size() >= nk - 1 && !bev_fork.empty()) return FV_OK;
    while ((int)bstreams.size() < nk - 1) {
        hipStream_t st;
        FV_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        bstreams.push_back(st);
    }
    const size_t stages = std::max<size_t>(ups.stages.size(), 1);
    while (bev_fork.size() < stages) {
        hipEvent_t e;
        FV_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        bev_fork.push_back(e);
    }
    while (bev_last.size() < stages * (size_t)nk) {
        hipEvent_t e;
        FV_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        bev_last.push_back(e);
    }
    return FV_OK;
}

fv_status fv_engine::run_upsampler(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s) {
    const int64_t me = (ups.max_elems(T) * B + 63) / 64 * 64;
    const int nk = ups.cfg.num_kernels;
    float *cur = ws, *S = ws + me, *Y = ws + 2 * me;
    auto XB = [&](int j) { return ws + (size_t)(3 + 3 * j) * me; };
    auto XT = [&](int j) { return ws + (size_t)(4 + 3 * j) * me; };
    auto XA = [&](int j) { return ws + (size_t)(5 + 3 * j) * me; };
    fv_status st;
    // The nk ResBlock branches of a stage are independent until the stack-mean: run them on their own streams
    // (fork after the upsampler conv, join after the last branch) so that one branch's tail / barrier phases are
    // filled by the others' workgroups.  The MRF accumulate into Y stays ordered j = 0, 1, 2 through events.
    // Profiling runs stay on one stream so that per-kernel hipEvent durations do not overlap.
    const bool multi = branch_streams && nk > 1 && !profiling;
    if (multi && (st = ensure_branch_streams(nk))) return st;
    ConvRun r;
    r.batch = B;
    // conv_pre (hifigan.py:227)
    r.x = d_in;
    r.y = cur;
    r.t_in = T;
    if ((st = conv_layer_run(ups.conv_pre, r, s))) return st;
    int t = (int)ups.conv_pre.out_len(T);
    int stage_idx = 0;
    bool sum_pending = false;   // tree mode: the stage output is still three branch buffers (XB(0..2))
    bool post_sum3 = false;     // ... and so is the last stage's, for conv_post to average
    const int n_stages = (int)ups.stages.size();
    for (auto& stg : ups.stages) {
        // x = ups[i](silu(x))  — HiFiGAN (hifigan.py:230-231); BigVGAN has no pre-activation (bigvgan.py:355-356)
        r = ConvRun();
        r.batch = B;
        r.x = cur;
        if (sum_pending) {   // the previous stage left its three branch outputs: the upsampler conv forms their mean itself
            r.x = XB(0);
            r.x2 = XB(1);
            r.x3 = XB(2);
            r.sum_tmp = cur;   // (kernels without the three-operand staging form it here first)
            sum_pending = false;
        }
        r.y = S;
        r.t_in = t;
        r.pre_act = ups.bigvgan ? FV_ACT_NONE : FV_ACT_SILU;
        if ((st = conv_layer_run(stg->up, r, s))) return st;
        t = (int)stg->up.out_len(t);
        const int ch = stg->ch;
        if (ups.cfg.use_template) {   // x = x + noise_convs[i](template)  (hifigan.py:233-234)
            const int Ta = (int)ups.out_len(T);
            FV_PROF(s, "noise_conv_add", 2.0 * B * ch * stg->nk * t, 8.0 * B * ch * t,
                    launch_noise_conv_add(cur_template, stg->d_nw, stg->d_nb, S, B, ch, t, Ta, stg->nk, stg->nstride, stg->npad, s));
        }
        if (multi) FV_HIP_CHECK(hipEventRecord(bev_fork[stage_idx], s));
        // debugging knob: FV_DEBUG_STOP = stage * 100 + pair * 10 + half stops the forward after that stage's dilation pair (half 0:
        // after c1, 1: after c2) with the branch buffers left in the workspace for inspection (tools/probe_f16_locate.py)
        static const int dbg_stop = std::getenv("FV_DEBUG_STOP") ? std::atoi(std::getenv("FV_DEBUG_STOP")) : -1;
        const bool dbg_here = dbg_stop >= 0 && dbg_stop / 100 == stage_idx;
        const int dbg_pair = (dbg_stop / 10) % 10, dbg_half = dbg_stop % 10;
        // ParralelBlock / stack-mean of the three ResBlock1 / AMPBlock branches (hifigan.py:132-133, bigvgan.py:358-365)
        // Y = ((y0 + y1) + y2) / 3 is formed in one of two ways — the same additions in the same order, so bit-identical:
        //   chain  y0 -> Y, (Y + y1) -> Y, (Y + y2) / 3 -> Y in the branches' last epilogues, ordered by events (single stream, other
        //          branch counts, FV_BRANCH_MEAN=chain)
        //   tree   the branches keep their outputs in their own buffers and mean_of_three_kernel forms Y after the join.
        // The chain makes each branch's last kernel wait for the previous branch's: a single clip paid 20-65 us of cross-queue
        // waits per stage (tools/latency_timeline.py), and at B = 32 the k = 7 and k = 11 branches' final convs ran one after the
        // other, alone on the chip, at the end of every stage (rocprofv3 trace).  Without it the host is also free to enqueue the
        // branches longest first (k = 11, 7, 3): a replayed graph starts sibling nodes in creation order, and the k = 11 chain —
        // every stage's critical path — used to start last (53 us after the fork in stage 0 of a single clip).  Tree + longest
        // first: B = 1 1.07 -> 0.97 ms per forward, B = 32 15.12 -> 15.00 ms (the extra pass over four tensors included; with
        // the branches enqueued shortest first the tree was 0.1 ms *slower* than the chain at B = 32).  Summing the other two
        // outputs in the last branch's final epilogue instead of a separate kernel measured 15.02 / 1.04 ms: not kept.  Neither
        // were: two streams, the longest branch on the caller's stream, a wake-up kernel on the side queues, stream priorities.
        static const char* const mean_env = std::getenv("FV_BRANCH_MEAN");   // experiments: "chain"
        // Narrow stages (ch <= chain_max_c, FV_CHAIN_MAX_C): the chain, so that the HBM-bound consumers — the last upsamplers, conv_post — read ONE
        // tensor instead of three; the k = 3 / 7 / 11 branches finish in that order anyway
        // Profiling runs (one stream, hipEvents around every launch: the source of the bench line's `roofline`) take the tree form too since round 6 — the
        // branches back to back, each into its own buffers — so that the table holds the kernel instances the shipped step launches: the chain's last
        // epilogues accumulate (the slow general epilogue of conv_wino44: 321 against 265 us for the dominant layer) and its upsamplers read one tensor,
        // neither of which the three-stream step ever runs.
        const bool tree = (multi || profiling || single_tree) && nk == 3 && !(mean_env && mean_env[0] == 'c') && stg->ch > chain_max_c;
        const bool order_desc = true;
        for (int jj = 0; jj < nk; ++jj) {
            const int j = (tree && order_desc) ? nk - 1 - jj : jj;
            ResBranch& br = *stg->branches[j];
            hipStream_t bs = (multi && j > 0) ? bstreams[j - 1] : s;
            if (multi && j > 0) FV_HIP_CHECK(hipStreamWaitEvent(bs, bev_fork[stage_idx], 0));
            const int bj = (multi || tree) ? j : 0;   // single-stream chain: branches run back to back and share one buffer set
            // ordering of the accumulate into Y: branch j's last kernel runs after branch j-1's
            auto before_last = [&]() -> fv_status {
                if (multi && j > 0 && !tree) FV_HIP_CHECK(hipStreamWaitEvent(bs, bev_last[stage_idx * nk + j - 1], 0));
                return FV_OK;
            };
            auto after_last = [&]() -> fv_status {
                if (multi) FV_HIP_CHECK(hipEventRecord(bev_last[stage_idx * nk + j], bs));
                return FV_OK;
            };
            int mode_last = OUT_SET;
            float scale_last = 1.0f;
            if (nk > 1 && !tree) {
                mode_last = j == 0 ? OUT_SET : OUT_ACCUM;
                scale_last = (j == nk - 1) ? 1.0f / (float)nk : 1.0f;
            }
            float* const y_last = tree ? XB(bj) : Y;   // tree: the branch keeps its own output, summed after the join
            // HiFiGAN narrow stages: the whole (c1, c2) pair in one kernel, intermediate kept in LDS.  Not in place
            // (workgroups read their neighbours' halo), so the branch ping-pongs S -> XB -> XT -> Y.
            // (C = 64 / 128 pairs — k = 3 only — fuse when the launch fills the chip; a single clip's 44 - 88 tiles are better served by the
            //  per-layer latency kernels: conv_wino_lat_impl.h)
            const bool fuse_narrow = ch <= pair_max_c && pair_supported(ch, br.k, br.dil[0]) && pair_supported(ch, br.k, br.dil[1]) &&
                                     pair_supported(ch, br.k, br.dil[2]) && (ch < 64 || cur_invariant() || (long long)B * ((t + 125) / 126) >= 2LL * num_cus());
            // f16x3 precision mode: the wide stages (C = 128 / 64) fuse too (pair_f16x3_impl.h)
            const bool fuse_wide = pair_f16x3_supported(br.c1[0], br.c2[0]) && pair_f16x3_supported(br.c1[1], br.c2[1]) &&
                                   pair_f16x3_supported(br.c1[2], br.c2[2]);
            const bool fuse = !ups.bigvgan && (fuse_narrow || fuse_wide) && fuse_pairs;
            if (fuse) {
                const float* src = S;
                for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
                    const bool last = n == FV_MAX_DILATIONS - 1;
                    float* dst = last ? y_last : (n == 0 ? XB(bj) : XT(bj));
                    if (last && (st = before_last())) return st;
                    if ((st = conv_pair_run(br.c1[n], br.c2[n], src, dst, B, t, last ? mode_last : OUT_SET,
                                            last ? scale_last : 1.0f, bs)))
                        return st;
                    src = dst;
                }
                if ((st = after_last())) return st;
                continue;
            }
            // BigVGAN narrow stages (C = 32 / 64): each conv runs with its anti-aliased SnakeBeta fused in front (amp_conv.hip) —
            // no activation launches, no activated tensors in HBM
            bool fuse_amp = ups.bigvgan && fuse_amp_convs && !dbg_here && ch <= fuse_amp_max_c && br.k <= fuse_amp_max_k;
            for (int n = 0; n < FV_MAX_DILATIONS && fuse_amp; ++n)
                fuse_amp = br.c1[n].precision == FV_PRECISION_F32 && br.c2[n].precision == FV_PRECISION_F32 && br.c1[n].c_in == ch &&
                           br.c1[n].c_out == ch && br.c2[n].c_in == ch && br.c2[n].c_out == ch && br.c1[n].k == br.k && br.c2[n].k == br.k &&
                           amp_conv_supported(ch, br.k, br.c1[n].dil) && br.c2[n].dil == 1 &&
                           br.c1[n].padding == (br.k - 1) / 2 * br.c1[n].dil && br.c2[n].padding == (br.k - 1) / 2 && (long long)ch * t < (1LL << 30);
            if (fuse_amp) {
                for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
                    const float* src = n == 0 ? S : XB(bj);
                    const bool last = n == FV_MAX_DILATIONS - 1;
                    const AASnake &a1 = br.act[2 * n], &a2 = br.act[2 * n + 1];
                    const double fl = 2.0 * ch * ch * br.k * (double)t * B, el = (double)B * ch * t * 4.0;
                    char lbl[96];
                    std::snprintf(lbl, sizeof(lbl), "amp_conv<k=%d d=%d C=%d>", br.k, br.c1[n].dil, ch);
                    FV_PROF(bs, lbl, fl + 60.0 * B * ch * t, 2.0 * el,
                            (launch_amp_conv(br.c1[n], src, XT(bj), nullptr, a1.d_alpha, a1.d_inv_beta, a1.d_up, a1.d_down, B, t, OUT_SET,
                                             1.0f, bs) ? FV_OK : FV_ERR_HIP));
                    if (last && (st = before_last())) return st;
                    std::snprintf(lbl, sizeof(lbl), "amp_conv<k=%d d=1 C=%d>+res", br.k, ch);
                    FV_PROF(bs, lbl, fl + 60.0 * B * ch * t, (last && mode_last == OUT_ACCUM ? 4.0 : 3.0) * el,
                            (launch_amp_conv(br.c2[n], XT(bj), last ? y_last : XB(bj), src, a2.d_alpha, a2.d_inv_beta, a2.d_up, a2.d_down, B, t,
                                             last ? mode_last : OUT_SET, last ? scale_last : 1.0f, bs) ? FV_OK : FV_ERR_HIP));
                }
                if ((st = after_last())) return st;
                continue;
            }
            for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
                if (dbg_here && n > dbg_pair) break;
                const float* src = n == 0 ? S : XB(bj);
                const bool last = n == FV_MAX_DILATIONS - 1;
                const float* c1_in = src;
                // FV_X_ABL_AA_SNAKE=1 (timing experiment, wrong results): the stand-alone activation passes in front of the k = 7 / 11 convs are skipped — what a
                // step would take if that activation were free, i.e. the ceiling of ANY fusion of it into a producer or consumer (LOG R5.14)
                // (= 2: skipped only in front of the k = 7 / 11 convs of the one-row-block stages, C = 64 / 128 — the layers a consumer-side fusion would cover;
                //  with -DFV_X_W44_SURR those convs carry the activation's vector issue instead: LOG R6.5)
                static const int abl_level = std::getenv("FV_X_ABL_AA_SNAKE") ? std::atoi(std::getenv("FV_X_ABL_AA_SNAKE")) : 0;
                const bool abl_aa = abl_level == 1 || (abl_level == 2 && (ch == 64 || ch == 128) && (br.k == 7 || br.k == 11));
                if (ups.bigvgan && !abl_aa) {
                    FV_PROF(bs, "aa_snake", 60.0 * B * ch * t, 8.0 * B * ch * t,
                            launch_aa_snake(src, XA(bj), br.act[2 * n].d_alpha, br.act[2 * n].d_inv_beta,
                                            br.act[2 * n].d_up, br.act[2 * n].d_down, B, ch, t, bs));
                    c1_in = XA(bj);
                }
                // xt = c1(act(x)); the second activation is fused into c1's epilogue for SiLU
                r = ConvRun();
                r.batch = B;
                r.t_in = t;
                r.x = c1_in;
                r.y = XT(bj);
                r.pre_act = ups.bigvgan ? FV_ACT_NONE : FV_ACT_SILU;
                r.post_act = ups.bigvgan ? FV_ACT_NONE : FV_ACT_SILU;
                if ((st = conv_layer_run(br.c1[n], r, bs))) return st;
                if (dbg_here && n == dbg_pair && dbg_half == 0) break;
                const float* c2_in = XT(bj);
                if (ups.bigvgan && !abl_aa) {
                    FV_PROF(bs, "aa_snake", 60.0 * B * ch * t, 8.0 * B * ch * t,
                            launch_aa_snake(XT(bj), XA(bj), br.act[2 * n + 1].d_alpha, br.act[2 * n + 1].d_inv_beta,
                                            br.act[2 * n + 1].d_up, br.act[2 * n + 1].d_down, B, ch, t, bs));
                    c2_in = XA(bj);
                }
                // x = c2(act(xt)) + x ; the last pair of each branch accumulates the branch mean into Y
                r = ConvRun();
                r.batch = B;
                r.t_in = t;
                r.x = c2_in;
                r.res = src;
                if (!last) {
                    r.y = XB(bj);
                } else {
                    r.y = y_last;
                    r.out_mode = mode_last;
                    r.out_scale = scale_last;
                    if ((st = before_last())) return st;
                }
                if ((st = conv_layer_run(br.c2[n], r, bs))) return st;
            }
            if ((st = after_last())) return st;
        }
        if (tree) {
            // join all three, then Y = ((y0 + y1) + y2) / 3 — the same additions in the same order as the accumulate chain
            if (multi)
                for (int j = 1; j < nk; ++j) FV_HIP_CHECK(hipStreamWaitEvent(s, bev_last[stage_idx * nk + j], 0));
            // the next stage's upsampler conv forms the mean while staging its input (conv_mfma_impl.h, SUM3); the last stage's
            // output goes through mean_of_three_kernel (its consumers are the narrow post kernels)
            const bool fuse_mean = !knobs().no_sum3;
            if (stage_idx + 1 < n_stages && fuse_mean && !dbg_here) {
                sum_pending = true;
            } else if (stage_idx + 1 == n_stages && fuse_mean && post_mean_fused && !dbg_here &&
                       (ups.bigvgan || conv_narrow_sum3_ok(B, ups.post_cin, t, 1, ups.cfg.post_conv_kernel_size,
                                                           get_padding(ups.cfg.post_conv_kernel_size)))) {
                post_sum3 = true;   // conv_post (HiFiGAN) / activation_post (BigVGAN) forms the last stage's branch mean while loading its input
            } else if ((st = launch_mean_of_three(XB(0), XB(1), XB(2), Y, (long long)B * ch * t, s))) {
                return st;
            }
        } else if (multi) {
            // join: the last branch's final kernel is ordered after every other branch's
            FV_HIP_CHECK(hipStreamWaitEvent(s, bev_last[stage_idx * nk + nk - 1], 0));
        }
        if (dbg_here) {
            std::fprintf(stderr, "FV_DEBUG_STOP: stage %d ch=%d t=%d me=%lld S=%lld Y=%lld\n", stage_idx, ch, t, (long long)me,
                         (long long)(S - ws), (long long)(Y - ws));
            return FV_OK;
        }
        std::swap(cur, Y);
        ++stage_idx;
    }
    // activation_post -> conv_post -> tanh (hifigan.py:245-247 / bigvgan.py:367-369)
    const float* post_in = cur;
    int pre = ups.cfg.post_activation;   // post_activation() (hifigan.py:213,245): SiLU by default
    const float pre_slope = ups.cfg.post_activation_slope;
    if (ups.bigvgan) {
        // (XA(0) is free again: every branch has joined)
        FV_PROF(s, post_sum3 ? "aa_snake sum3" : "aa_snake", 60.0 * B * ups.post_cin * t, (post_sum3 ? 16.0 : 8.0) * B * ups.post_cin * t,
                launch_aa_snake(post_sum3 ? XB(0) : cur, XA(0), ups.act_post.d_alpha, ups.act_post.d_inv_beta, ups.act_post.d_up,
                                ups.act_post.d_down, B, ups.post_cin, t, s, post_sum3 ? XB(1) : nullptr, post_sum3 ? XB(2) : nullptr));
        post_in = XA(0);
        pre = FV_ACT_NONE;
        post_sum3 = false;   // the mean is in: conv_post reads the activated tensor
    }
    const int qk = ups.cfg.post_conv_kernel_size;
    if (post_sum3) {
        FV_PROF(s, "conv_post_narrow sum3", 2.0 * B * ups.post_cin * qk * t, 4.0 * B * (3 * ups.post_cin + 1) * t,
                launch_conv_narrow(XB(0), ups.d_wpost, ups.d_bpost, d_out, B, ups.post_cin, t, 1, qk, get_padding(qk), pre, FV_ACT_TANH, pre_slope,
                                   s, XB(1), XB(2)));
        return FV_OK;
    }
    FV_PROF(s, "conv_post_narrow", 2.0 * B * ups.post_cin * qk * t, 4.0 * B * (ups.post_cin + 1) * t,
            launch_conv_narrow(post_in, ups.d_wpost, ups.d_bpost, d_out, B, ups.post_cin, t, 1, qk, get_padding(qk), pre,
                               FV_ACT_TANH, pre_slope, s));
    return FV_OK;
}

fv_status fv_engine::run_convnext(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s) {
    const int64_t me = ((int64_t)cnx.max_dim() * T * B + 63) / 64 * 64;
    float* X = ws;               // running activation (dim, T)
    float* H = ws + me;          // LN output (dim, T)
    float* G = ws + 2 * me;      // hidden (4*dim, T)
    fv_status st;
    const int ks = cnx.cfg.kernel_size;
    ConvRun r;
    for (int i = 0; i < cnx.cfg.num_stages; ++i) {
        CnxStage& stg = *cnx.stages[i];
        const int dim = cnx.cfg.dims[i];
        if (i == 0) {
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = d_in;
            r.y = H;
            if ((st = conv_layer_run(stg.conv, r, s))) return st;
            FV_PROF(s, "layernorm_cf", 8.0 * B * dim * T, 8.0 * B * dim * T,
                    launch_dwconv_ln(H, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, X, B, dim, T, 1, 1e-6f, s));
        } else {
            FV_PROF(s, "layernorm_cf", 8.0 * B * stg.ln_dim * T, 8.0 * B * stg.ln_dim * T,
                    launch_dwconv_ln(X, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, H, B, stg.ln_dim, T, 1, 1e-6f, s));
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = H;
            r.y = X;
            if ((st = conv_layer_run(stg.conv, r, s))) return st;
        }
        for (auto& bp : stg.blocks) {
            CnxBlock& blk = *bp;
            // dwconv -> LN (convnext.py:126-129)
            FV_PROF(s, "dwconv_ln", (2.0 * ks + 8.0) * B * dim * T, 8.0 * B * dim * T,
                    launch_dwconv_ln(X, blk.d_dw_w, blk.d_dw_b, blk.d_ln_w, blk.d_ln_b, H, B, dim, T, ks, 1e-6f, s));
            // pwconv1 + GELU (convnext.py:130-131)
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = H;
            r.y = G;
            r.post_act = FV_ACT_GELU;
            if ((st = conv_layer_run(blk.pw1, r, s))) return st;
            // pwconv2, * gamma, + input (convnext.py:132-141)
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = G;
            r.y = X;
            r.res = X;
            r.gamma = blk.d_gamma;
            if ((st = conv_layer_run(blk.pw2, r, s))) return st;
        }
    }
    FV_PROF(s, "layernorm_cf", 8.0 * B * cnx.out_dim() * T, 8.0 * B * cnx.out_dim() * T,
            launch_dwconv_ln(X, nullptr, nullptr, cnx.d_norm_w, cnx.d_norm_b, d_out, B, cnx.out_dim(), T, 1, 1e-6f, s));
    return FV_OK;
}

fv_status fv_engine::run_head(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s) {
    const int N = head.cfg.n_fft, nb = head.nb;
    const int64_t rows = std::max<int64_t>(2 * nb, N);
    const int64_t me = (rows * T * B + 63) / 64 * 64;
    float* Hh = ws;            // (2nb, T) log-mag / phase
    float* Sp = ws + me;       // (2nb, T) Re / Im
    float* Fr = ws + 2 * me;   // (n_fft, T) windowed frames
    fv_status st;
    ConvRun r;
    r.batch = B;
    r.t_in = T;
    r.x = d_in;
    r.y = Hh;
    if ((st = conv_layer_run(head.out, r, s))) return st;
    // Hh is already compacted to 2*nb rows: reuse the spec kernel with n_fft' = nb (rows [0,nb) mag, [nb,2nb) phase)
    FV_PROF(s, "istft_spec", 30.0 * B * nb * T, 16.0 * B * nb * T, launch_istft_spec(Hh, Sp, B, nb, T, nb, nb, s));
    r = ConvRun();
    r.batch = B;
    r.t_in = T;
    r.x = Sp;
    r.y = Fr;
    if ((st = conv_layer_run(head.idft, r, s))) return st;
    // "same": crop (win - hop) / 2 -> T * hop samples (vocos ISTFT); "center": crop n_fft / 2 -> (T - 1) * hop (torch.istft(center=True))
    FV_PROF(s, "istft_ola", 2.0 * B * N * T, 4.0 * B * (N * (double)T + (double)head.out_len(T)),
            launch_istft_ola(Fr, head.d_win2, d_out, B, N, T, head.cfg.hop_length, head.crop(), head.out_len(T), s));
    return FV_OK;
}


// slaney mel scale of torchaudio.functional.melscale_fbanks (third-party, restated from the published formula; the
// reference call site is data/transforms/spectrogram.py:83-91)
static double hz_to_mel_slaney(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_hz / f_sp + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz_slaney(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, logstep = std::log(6.4) / 27.0, min_log_mel = min_log_hz / f_sp;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

fv_status fv_engine::build_logmel(const std::string& pfx) {
    const fv_logmel_config& c = cfg.mel;
    mel.cfg = c;
    const int N = c.n_fft, hop = c.hop_length, nb = N / 2 + 1;
    // frames are cut into ceil(N / hop) hop-sized pieces; when hop does not divide N (resolution/24000_2048_3072.yaml) the
    // last piece is only partly covered by the window and the rest of its DFT weights stay zero
    const int taps = (N + hop - 1) / hop;
    mel.nb = nb;
    mel.taps = taps;
    mel.pad_l = (c.win_length - hop) / 2;        // spectrogram.py:30-33
    mel.pad_r = (c.win_length - hop + 1) / 2;
    std::vector<float> win(N);
    if (const HostTensor* t = find(pfx + "spectrogram.window")) {
        if (t->numel() != N) {
            set_error("'%sspectrogram.window' has %lld taps, expected %d", pfx.c_str(), (long long)t->numel(), N);
            return FV_ERR_SHAPE;
        }
        win = t->data;
    } else {
        for (int n = 0; n < N; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / N));   // hann, periodic
    }
    // STFT as a stride-1 conv over the polyphase signal: X_k[t] = sum_{r<hop} sum_{q<taps} w[qh+r] e^{-2 pi i k (qh+r)/N} yp[r][t+q]
    std::vector<float> wst((size_t)2 * nb * hop * taps, 0.f);
    for (int k = 0; k < nb; ++k)
        for (int r = 0; r < hop; ++r)
            for (int q = 0; q < taps; ++q) {
                const int n = q * hop + r;
                if (n >= N) continue;
                const double ang = 2.0 * M_PI * (double)(((int64_t)k * n) % N) / N;
                wst[((size_t)k * hop + r) * taps + q] = (float)(win[n] * std::cos(ang));
                wst[((size_t)(nb + k) * hop + r) * taps + q] = (float)(-(double)win[n] * std::sin(ang));
            }
    fv_status st;
    if ((st = conv_layer_create(mel.stft, false, hop, 2 * nb, taps, 1, 0, 1, wst.data(), nullptr))) return st;
    if (c.n_mels == 0) return FV_OK;   // linear spectrogram only: no filterbank
    // filterbank (n_freqs, n_mels) -> pointwise conv weight (n_mels, n_freqs)
    std::vector<float> fbw((size_t)c.n_mels * nb);
    if (const HostTensor* t = find(pfx + "mel_scale.fb")) {
        if (t->numel() != (int64_t)nb * c.n_mels) {
            set_error("'%smel_scale.fb' has %lld elements, expected %d x %d", pfx.c_str(), (long long)t->numel(), nb, c.n_mels);
            return FV_ERR_SHAPE;
        }
        for (int f = 0; f < nb; ++f)
            for (int m = 0; m < c.n_mels; ++m) fbw[(size_t)m * nb + f] = t->data[(size_t)f * c.n_mels + m];
    } else {
        const double f_max = c.f_max > 0 ? c.f_max : (double)(c.sample_rate / 2);
        const double m_min = hz_to_mel_slaney(c.f_min), m_max = hz_to_mel_slaney(f_max);
        std::vector<double> f_pts(c.n_mels + 2);
        for (int i = 0; i < c.n_mels + 2; ++i) f_pts[i] = mel_to_hz_slaney(m_min + (m_max - m_min) * i / (c.n_mels + 1));
        for (int f = 0; f < nb; ++f) {
            const double freq = (double)(c.sample_rate / 2) * f / (nb - 1);
            for (int m = 0; m < c.n_mels; ++m) {
                const double down = (freq - f_pts[m]) / (f_pts[m + 1] - f_pts[m]);
                const double up = (f_pts[m + 2] - freq) / (f_pts[m + 2] - f_pts[m + 1]);
                const double v = std::max(0.0, std::min(down, up)) * (2.0 / (f_pts[m + 2] - f_pts[m]));
                fbw[(size_t)m * nb + f] = (float)v;
            }
        }
    }
    return conv_layer_create(mel.mel, false, nb, c.n_mels, 1, 1, 0, 1, fbw.data(), nullptr);
}

fv_status fv_engine::run_logmel(const float* d_in, float* d_out, int B, int L, float* ws, hipStream_t s) {
    const int hop = mel.cfg.hop_length, nb = mel.nb;
    const int T = mel.frames(L);
    const int TP = T + mel.taps - 1;
    const size_t n_yp = ((size_t)B * hop * TP + 63) / 64 * 64, n_sp = ((size_t)B * 2 * nb * T + 63) / 64 * 64;
    float* Yp = ws;
    float* Sp = ws + n_yp;
    float* Mg = Sp + n_sp;
    FV_PROF(s, "polyphase_reflect", 0.0, 8.0 * B * (double)hop * TP,
            launch_polyphase_reflect(d_in, Yp, B, L, hop, TP, mel.pad_l, mel.pad_r, s));
    fv_status st;
    ConvRun r;
    r.batch = B;
    r.t_in = TP;
    r.x = Yp;
    r.y = Sp;
    if ((st = conv_layer_run(mel.stft, r, s))) return st;
    if (mel.cfg.n_mels == 0) {   // LinearSpectrogram alone (spectrogram.py:25-56): the magnitude is the result
        FV_PROF(s, "magnitude", 4.0 * B * nb * T, 12.0 * B * nb * T, launch_magnitude(Sp, d_out, B, nb, T, s));
        return FV_OK;
    }
    FV_PROF(s, "magnitude", 4.0 * B * nb * T, 12.0 * B * nb * T, launch_magnitude(Sp, Mg, B, nb, T, s));
    r = ConvRun();
    r.batch = B;
    r.t_in = T;
    r.x = Mg;
    r.y = d_out;
    r.post_act = FV_ACT_LOG_CLAMP;   // compress(): log(clamp(x, 1e-5))  (spectrogram.py:93-94)
    return conv_layer_run(mel.mel, r, s);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static fv_status validate_ups(const fv_upsampler_config& c) {
    if (c.num_upsamples < 1 || c.num_upsamples > FV_MAX_STAGES || c.num_kernels < 1 || c.num_kernels > FV_MAX_KERNELS) {
        set_error("num_upsamples=%d / num_kernels=%d out of range", c.num_upsamples, c.num_kernels);
        return FV_ERR_INVALID;
    }
    int64_t prod = 1;
    for (int i = 0; i < c.num_upsamples; ++i) {
        if (c.upsample_rates[i] < 1 || c.upsample_kernel_sizes[i] < c.upsample_rates[i]) {
            set_error("stage %d: upsample rate %d / kernel %d invalid", i, c.upsample_rates[i], c.upsample_kernel_sizes[i]);
            return FV_ERR_INVALID;
        }
        prod *= c.upsample_rates[i];
    }
    if (prod != c.hop_length) {  // hifigan.py:154-156
        set_error("hop_length must be %lld", (long long)prod);
        return FV_ERR_INVALID;
    }
    if (c.use_template) {
        // noise_convs[i] must produce exactly the stage's length: stride_f0 even (or 1), as with every power-of-two rate
        int s_f0 = 1;
        for (int i = c.num_upsamples - 1; i >= 1; --i) {
            s_f0 *= c.upsample_rates[i];
            if (s_f0 % 2) {
                set_error("use_template: the product of upsample_rates[%d:] = %d must be even", i, s_f0);
                return FV_ERR_UNSUPPORTED;
            }
        }
    }
    if (c.num_mels < 1 || c.upsample_initial_channel < 1 || c.pre_conv_kernel_size < 1 || c.post_conv_kernel_size < 1 ||
        c.pre_conv_kernel_size % 2 == 0 || c.post_conv_kernel_size % 2 == 0) {
        set_error("invalid num_mels / upsample_initial_channel / pre,post kernel sizes (must be odd)");
        return FV_ERR_INVALID;
    }
    if (c.post_activation != FV_POST_ACT_DEFAULT && c.post_activation != FV_POST_ACT_IDENTITY && c.post_activation != FV_ACT_SILU &&
        c.post_activation != FV_ACT_LEAKY_RELU && c.post_activation != FV_ACT_GELU && c.post_activation != FV_ACT_TANH) {
        set_error("post_activation %d: only nn.Identity / nn.SiLU / nn.LeakyReLU / nn.ReLU / nn.GELU / nn.Tanh have a kernel form", c.post_activation);
        return FV_ERR_UNSUPPORTED;
    }
    if (!(c.post_activation_slope == c.post_activation_slope) || (c.post_activation != FV_ACT_LEAKY_RELU && c.post_activation_slope != 0.f)) {
        set_error("post_activation_slope must be a number, and 0 unless post_activation is FV_ACT_LEAKY_RELU");
        return FV_ERR_INVALID;
    }
    for (int j = 0; j < c.num_kernels; ++j) {
        if (c.resblock_kernel_sizes[j] < 1 || c.resblock_kernel_sizes[j] % 2 == 0) {
            set_error("resblock kernel size %d must be odd", c.resblock_kernel_sizes[j]);
            return FV_ERR_INVALID;
        }
        for (int n = 0; n < FV_MAX_DILATIONS; ++n)
            if (c.resblock_dilation_sizes[j][n] < 1) {
                set_error("resblock dilation must be >= 1");
                return FV_ERR_INVALID;
            }
    }
    return FV_OK;
}

extern "C" {

FV_API fv_status fv_create(const fv_config* cfg, fv_engine** out) {
    if (!cfg || !out) {
        set_error("fv_create: null argument");
        return FV_ERR_INVALID;
    }
    if (cfg->abi_version != FV_ABI_VERSION) {
        set_error("fv_create: ABI version %d, library is %d", cfg->abi_version, FV_ABI_VERSION);
        return FV_ERR_INVALID;
    }
    fv_status st = FV_OK;
    switch (cfg->model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: st = validate_ups(cfg->ups); break;
        case FV_MODEL_FIREFLY:
            st = validate_ups(cfg->ups);
            if (!st && cfg->ups.num_mels != cfg->backbone.dims[cfg->backbone.num_stages - 1]) {
                set_error("firefly: head num_mels (%d) must equal the backbone output dim (%d)", cfg->ups.num_mels,
                          cfg->backbone.dims[cfg->backbone.num_stages - 1]);
                st = FV_ERR_INVALID;
            }
            break;
        case FV_MODEL_VOCOS:
        case FV_MODEL_ISTFT_HEAD:
            if (cfg->head.win_length != cfg->head.n_fft || cfg->head.hop_length < 1 || cfg->head.n_fft < 2 ||
                cfg->head.n_fft % 2 || cfg->head.hop_length > cfg->head.win_length || cfg->head.dim < 1 ||
                (cfg->head.win_length - cfg->head.hop_length) % 2 || (cfg->head.padding != FV_ISTFT_SAME && cfg->head.padding != FV_ISTFT_CENTER) ||
                (cfg->model == FV_MODEL_VOCOS &&
                 cfg->head.dim != cfg->backbone.dims[cfg->backbone.num_stages > 0 ? cfg->backbone.num_stages - 1 : 0])) {
                set_error("istft head: need even n_fft == win_length >= hop_length, even (win-hop), padding same / center, dim == backbone dims[-1]");
                st = FV_ERR_INVALID;
            }
            break;
        case FV_MODEL_CONVNEXT: break;
        case FV_MODEL_REFINEGAN: {
            const fv_refinegan_config& g = cfg->refine;
            long long pd = 1, pu = 1;
            bool ok = g.num_stages >= 1 && g.num_stages <= FV_MAX_STAGES && g.num_mels >= 1 && g.start_channels >= 1 && g.hop_length >= 1;
            for (int i = 0; ok && i < g.num_stages; ++i) {
                ok = g.downsample_rates[i] >= 1 && g.upsample_rates[i] >= 1;
                pd *= g.downsample_rates[i];
                pu *= g.upsample_rates[i];
            }
            // assert np.prod(downsample_rates) == np.prod(upsample_rates) == hop_length (refinegan.py:202)
            if (!ok || pd != g.hop_length || pu != g.hop_length) {
                set_error("refinegan: prod(downsample_rates) and prod(upsample_rates) must both equal hop_length (%d)", g.hop_length);
                st = FV_ERR_INVALID;
            }
            break;
        }
        case FV_MODEL_LOGMEL: {
            const fv_logmel_config& m = cfg->mel;
            if (m.n_fft < 2 || m.n_fft % 2 || m.hop_length < 1 || m.win_length != m.n_fft || m.hop_length > m.n_fft ||
                m.n_mels < 0 || m.sample_rate < 2 || m.f_min < 0) {
                set_error("logmel: need even n_fft == win_length, hop_length <= n_fft, n_mels >= 0");
                st = FV_ERR_INVALID;
            }
            break;
        }
        default: set_error("fv_create: unknown model kind %d", cfg->model); st = FV_ERR_INVALID;
    }
    if (!st && cfg->model != FV_MODEL_HIFIGAN && cfg->model != FV_MODEL_BIGVGAN && cfg->model != FV_MODEL_ISTFT_HEAD &&
        cfg->model != FV_MODEL_LOGMEL && cfg->model != FV_MODEL_REFINEGAN) {
        const fv_convnext_config& b = cfg->backbone;
        if (b.num_stages < 1 || b.num_stages > FV_MAX_STAGES || b.input_channels < 1 || b.kernel_size < 1 || b.kernel_size % 2 == 0) {
            set_error("convnext: invalid num_stages / input_channels / kernel_size");
            st = FV_ERR_INVALID;
        }
        for (int i = 0; !st && i < b.num_stages; ++i)
            if (b.depths[i] < 0 || b.dims[i] < 1) {
                set_error("convnext: invalid depths/dims at stage %d", i);
                st = FV_ERR_INVALID;
            }
    }
    if (st) return st;
    fv_engine* e = new (std::nothrow) fv_engine();
    if (!e) {
        set_error("out of host memory");
        return FV_ERR_INVALID;
    }
    e->cfg = *cfg;
    // ABI 5: 0 (a zero-initialised struct) is the reference default SiLU, -1 nn.Identity; inside the engine the field is a plain fv_act
    if (e->cfg.ups.post_activation == FV_POST_ACT_DEFAULT) e->cfg.ups.post_activation = FV_ACT_SILU;
    else if (e->cfg.ups.post_activation == FV_POST_ACT_IDENTITY) e->cfg.ups.post_activation = FV_ACT_NONE;
    if (const char* v = std::getenv("FV_NO_PAIR_FUSION")) e->fuse_pairs = !(v[0] == '1');
    if (const char* v = std::getenv("FV_PAIR_MAXC")) e->pair_max_c = std::atoi(v);
    if (const char* v = std::getenv("FV_CHAIN_MAX_C")) e->chain_max_c = std::atoi(v);
    if (const char* v = std::getenv("FV_NO_POST_SUM3")) e->post_mean_fused = !(v[0] == '1');
    if (const char* v = std::getenv("FV_NO_AMP_FUSION")) e->fuse_amp_convs = !(v[0] == '1');
    if (const char* v = std::getenv("FV_AMP_MAXC")) e->fuse_amp_max_c = std::atoi(v);
    if (const char* v = std::getenv("FV_AMP_MAXK")) e->fuse_amp_max_k = std::atoi(v);
    if (const char* v = std::getenv("FV_SINGLE_STREAM")) {
        e->branch_streams = !(v[0] == '1' || v[0] == '2');
        e->single_tree = v[0] == '2';
    }
    if (const char* v = std::getenv("FV_NO_GRAPH")) e->use_graph = !(v[0] == '1');
    if (std::getenv("FV_DEBUG_STOP")) e->use_graph = false;   // the early return leaves forked branch streams unjoined: not capturable
    if (const char* v = std::getenv("FV_TILE_FRAMES")) e->tile_frames_override = std::atoi(v);
    *out = e;
    return FV_OK;
}

FV_API fv_status fv_load_weight(fv_engine* e, const char* name, const float* host_data, const int64_t* shape, int32_t ndim) {
    if (!e || !name || !host_data || ndim < 0 || ndim > 8 || (ndim > 0 && !shape)) {
        set_error("fv_load_weight: invalid argument");
        return FV_ERR_INVALID;
    }
    if (e->finalized) {
        set_error("fv_load_weight: engine already finalized");
        return FV_ERR_STATE;
    }
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    const int64_t n = t.numel();
    if (n < 0) {
        set_error("fv_load_weight: negative dimension");
        return FV_ERR_SHAPE;
    }
    t.data.assign(host_data, host_data + n);
    e->raw[name] = std::move(t);
    return FV_OK;
}

FV_API fv_status fv_set_precision(fv_engine* e, int32_t precision) {
    if (!e) {
        set_error("fv_set_precision: null engine");
        return FV_ERR_INVALID;
    }
    if (precision != FV_PRECISION_F32 && precision != FV_PRECISION_F16X3) {
        set_error("fv_set_precision: unknown precision %d", precision);
        return FV_ERR_INVALID;
    }
    if (e->finalized) {
        set_error("fv_set_precision: engine already finalized (the weight planes are packed at fv_finalize)");
        return FV_ERR_STATE;
    }
    e->precision = precision;
    return FV_OK;
}

void fv_engine::drop_graphs() {
    for (auto& g : graphs) {
        (void)hipGraphExecDestroy(g.exec);
        (void)hipGraphDestroy(g.graph);
    }
    graphs.clear();
    have_last = false;
}

FV_API fv_status fv_set_conv_algorithm(fv_engine* e, int32_t algo) {
    if (!e) {
        set_error("fv_set_conv_algorithm: null engine");
        return FV_ERR_INVALID;
    }
    if (algo != FV_CONV_ALGO_AUTO && algo != FV_CONV_ALGO_DIRECT && algo != FV_CONV_ALGO_WINOGRAD) {
        set_error("fv_set_conv_algorithm: unknown algorithm %d", algo);
        return FV_ERR_INVALID;
    }
    if (e->algo != algo) e->drop_graphs();   // captured launch sequences hold the old choice
    e->algo = algo;
    return FV_OK;
}

FV_API fv_status fv_set_batch_invariant(fv_engine* e, int32_t enable) {
    if (!e) {
        set_error("fv_set_batch_invariant: null engine");
        return FV_ERR_INVALID;
    }
    if (e->invariant != (enable != 0)) e->drop_graphs();
    e->invariant = enable != 0;
    return FV_OK;
}

FV_API fv_status fv_set_graph_replay(fv_engine* e, int32_t enable) {
    if (!e) {
        set_error("fv_set_graph_replay: null engine");
        return FV_ERR_INVALID;
    }
    e->use_graph = enable != 0;
    return FV_OK;
}

FV_API int32_t fv_get_graph_replay(const fv_engine* e) { return e && e->use_graph ? 1 : 0; }

FV_API fv_status fv_finalize(fv_engine* e) {
    if (!e) {
        set_error("fv_finalize: null engine");
        return FV_ERR_INVALID;
    }
    if (e->finalized) return FV_OK;
    fv_status st = FV_OK;
    switch (e->cfg.model) {
        case FV_MODEL_HIFIGAN: st = e->build_upsampler("", false); break;
        case FV_MODEL_BIGVGAN: st = e->build_upsampler("", true); break;
        case FV_MODEL_CONVNEXT: st = e->build_convnext(""); break;
        case FV_MODEL_ISTFT_HEAD: st = e->build_head(""); break;
        case FV_MODEL_LOGMEL: st = e->build_logmel(""); break;
        case FV_MODEL_REFINEGAN: st = e->build_refinegan(); break;
        case FV_MODEL_VOCOS:
            st = e->build_convnext("backbone.");
            if (!st) st = e->build_head("head.");
            break;
        case FV_MODEL_FIREFLY:
            st = e->build_convnext("backbone.");
            if (!st) st = e->build_upsampler("head.", false);
            break;
    }
    if (!st) st = e->run_jobs();
    e->jobs.clear();
    if (st) return st;
    // strict load: unexpected keys are an error, as load_state_dict(strict=True) (test.py:37)
    for (auto& kv : e->raw)
        if (!e->used.count(kv.first)) {
            set_error("unexpected key '%s' in state dict", kv.first.c_str());
            return FV_ERR_INVALID;
        }
    e->raw.clear();
    e->finalized = true;
    return FV_OK;
}

FV_API void fv_destroy(fv_engine* e) { delete e; }

FV_API int32_t fv_input_channels(const fv_engine* e) {
    if (!e) return 0;
    if (e->cfg.model == FV_MODEL_ISTFT_HEAD) return e->cfg.head.dim;
    if (e->cfg.model == FV_MODEL_LOGMEL) return 1;
    if (e->cfg.model == FV_MODEL_REFINEGAN) return e->cfg.refine.num_mels;
    return (e->cfg.model == FV_MODEL_HIFIGAN || e->cfg.model == FV_MODEL_BIGVGAN) ? e->cfg.ups.num_mels
                                                                                    : e->cfg.backbone.input_channels;
}
FV_API int32_t fv_output_channels(const fv_engine* e) {
    if (!e) return 0;
    if (e->cfg.model == FV_MODEL_LOGMEL) return e->cfg.mel.n_mels ? e->cfg.mel.n_mels : e->cfg.mel.n_fft / 2 + 1;
    return e->cfg.model == FV_MODEL_CONVNEXT ? e->cfg.backbone.dims[e->cfg.backbone.num_stages - 1] : 1;
}
FV_API int64_t fv_output_length(const fv_engine* e, int32_t t_in) {
    if (!e || !e->finalized || t_in < 1) return 0;
    switch (e->cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN:
        case FV_MODEL_FIREFLY: return e->ups.out_len(t_in);
        case FV_MODEL_VOCOS:
        case FV_MODEL_ISTFT_HEAD: return e->head.out_len(t_in);
        case FV_MODEL_LOGMEL: return std::max(0, e->mel.frames(t_in));
        case FV_MODEL_REFINEGAN: return (int64_t)t_in * e->cfg.refine.hop_length;
        default: return t_in;
    }
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static size_t refine_ws_elems(const fv_engine* e, int B, int T);

static size_t ups_ws_elems(const fv_engine* e, int B, int T) {
    return (size_t)(3 + 3 * e->ups.cfg.num_kernels) * ((e->ups.max_elems(T) * B + 63) / 64 * 64);
}
static size_t cnx_ws_elems(const fv_engine* e, int B, int T) {
    const size_t me = ((size_t)e->cnx.max_dim() * T * B + 63) / 64 * 64;
    return 2 * me + 4 * me;  // X, H, and the 4x hidden
}
static size_t head_ws_elems(const fv_engine* e, int B, int T) {
    const size_t rows = std::max<size_t>(2 * e->head.nb, e->cfg.head.n_fft);
    return 3 * ((rows * T * B + 63) / 64 * 64);
}

static size_t whole_workspace_bytes(const fv_engine* e, int32_t batch, int32_t t_in);

FV_API size_t fv_workspace_bytes(const fv_engine* e, int32_t batch, int32_t t_in) {
    if (!e || !e->finalized || batch < 1 || t_in < 1) return 0;
    const fv_engine::TilePlan tp = e->tile_plan(t_in);
    if (tp.n <= 1) return whole_workspace_bytes(e, batch, t_in);
    if ((long long)batch * tp.n > (1 << 24)) return 0;
    const int bn = batch * tp.n;
    const size_t lout = (size_t)fv_output_length(e, tp.L);
    size_t elems = align_up((size_t)bn * fv_input_channels(e) * tp.L, 64) + align_up((size_t)bn * fv_output_channels(e) * lout, 64);
    if (e->cfg.ups.use_template && (e->cfg.model == FV_MODEL_HIFIGAN || e->cfg.model == FV_MODEL_BIGVGAN || e->cfg.model == FV_MODEL_FIREFLY))
        elems += align_up((size_t)bn * lout, 64);
    return align_up(elems * sizeof(float), 256) + whole_workspace_bytes(e, bn, tp.L);
}

static size_t whole_workspace_bytes(const fv_engine* e, int32_t batch, int32_t t_in) {
    size_t elems = 0;
    switch (e->cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: elems = ups_ws_elems(e, batch, t_in); break;
        case FV_MODEL_CONVNEXT: elems = cnx_ws_elems(e, batch, t_in); break;
        case FV_MODEL_ISTFT_HEAD: elems = head_ws_elems(e, batch, t_in); break;
        case FV_MODEL_LOGMEL: {
            const size_t T = (size_t)std::max(1, e->mel.frames(t_in));
            elems = ((size_t)batch * e->cfg.mel.hop_length * (T + e->mel.taps) + 64) +
                    ((size_t)batch * 3 * e->mel.nb * T + 128);
            break;
        }
        case FV_MODEL_REFINEGAN: elems = refine_ws_elems(e, batch, t_in); break;
        case FV_MODEL_VOCOS: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            elems = mid + std::max(cnx_ws_elems(e, batch, t_in), head_ws_elems(e, batch, t_in));
            break;
        }
        case FV_MODEL_FIREFLY: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            elems = mid + std::max(cnx_ws_elems(e, batch, t_in), ups_ws_elems(e, batch, t_in));
            break;
        }
    }
    return align_up(elems * sizeof(float), 256);
}

FV_API fv_status fv_forward(fv_engine* e, const float* d_in, float* d_out, int32_t batch, int32_t t_in, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
    return fv_forward_template(e, d_in, nullptr, d_out, batch, t_in, d_workspace, workspace_bytes, stream);
}

static fv_status forward_common(fv_engine* e, const float* d_in, const float* d_template, const float* d_noise, float* d_out,
                                int32_t batch, int32_t t_in, void* d_workspace, size_t workspace_bytes, void* stream);

FV_API fv_status fv_forward_template(fv_engine* e, const float* d_in, const float* d_template, float* d_out, int32_t batch,
                                     int32_t t_in, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (e && e->cfg.model == FV_MODEL_REFINEGAN) {
        set_error("fv_forward: a RefineGAN engine needs fv_forward_refinegan (template + AdaIN noise)");
        return FV_ERR_INVALID;
    }
    return forward_common(e, d_in, d_template, nullptr, d_out, batch, t_in, d_workspace, workspace_bytes, stream);
}

FV_API int64_t fv_refinegan_noise_elems(const fv_engine* e, int32_t batch, int32_t t_in) {
    if (!e || !e->finalized || e->cfg.model != FV_MODEL_REFINEGAN || batch < 1 || t_in < 1) return 0;
    int64_t n = 0, t = t_in;
    for (auto& u : e->refine.ups) {
        t *= u->rate;
        n += 6LL * batch * u->cout * t;
    }
    return n;
}

FV_API fv_status fv_forward_refinegan(fv_engine* e, const float* d_mel, const float* d_template, const float* d_noise,
                                      float* d_out, int32_t batch, int32_t t_in, void* d_workspace, size_t workspace_bytes,
                                      void* stream) {
    if (!e || e->cfg.model != FV_MODEL_REFINEGAN) {
        set_error("fv_forward_refinegan: not a RefineGAN engine");
        return FV_ERR_INVALID;
    }
    if (!d_template || !d_noise) {
        set_error("fv_forward_refinegan: template (B, 1, T*hop) and noise (fv_refinegan_noise_elems floats) are required");
        return FV_ERR_INVALID;
    }
    return forward_common(e, d_mel, d_template, d_noise, d_out, batch, t_in, d_workspace, workspace_bytes, stream);
}

// What every entry that runs the model checks before it enqueues anything (forward_common; fv_ragged_forward for each of its groups)
static fv_status check_forward(fv_engine* e, const float* d_in, const float* d_template, float* d_out, int32_t batch, int32_t t_in,
                               void* d_workspace, size_t workspace_bytes) {
    if (!e || !d_in || !d_out) {
        set_error("fv_forward: null argument");
        return FV_ERR_INVALID;
    }
    if (!e->finalized) {
        set_error("fv_forward: call fv_finalize first");
        return FV_ERR_STATE;
    }
    if (batch < 1 || t_in < 1) {
        set_error("fv_forward: empty input (batch=%d, t_in=%d)", batch, t_in);
        return FV_ERR_INVALID;
    }
    {
        const fv_engine::TilePlan tp = e->tile_plan(t_in);
        if (tp.n > 1 && (long long)batch * tp.n > (1 << 24)) {
            set_error("fv_forward: %d clips x %d time tiles of %d frames exceed 2^24 tiles per call: split the batch (or raise FV_TILE_FRAMES)", batch,
                      tp.n, tp.L);
            return FV_ERR_UNSUPPORTED;
        }
    }
    const size_t need = fv_workspace_bytes(e, batch, t_in);
    if (e->cfg.model == FV_MODEL_REFINEGAN && need == 0) {
        set_error("refinegan: the down/up-sampling lengths do not line up for %d frames (the reference's torch.cat would fail)", t_in);
        return FV_ERR_INVALID;
    }
    if (!d_workspace || workspace_bytes < need) {
        set_error("fv_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
        return FV_ERR_INVALID;
    }
    if ((e->cfg.model == FV_MODEL_VOCOS || e->cfg.model == FV_MODEL_ISTFT_HEAD) && e->head.center()) {
        if (t_in < 2) {   // (T - 1) * hop = 0 samples: torch.istft fails on the empty envelope
            set_error("istft head, padding=\"center\": %d frame(s) leave no output samples ((T - 1) * hop)", t_in);
            return FV_ERR_INVALID;
        }
        if (!e->head.center_envelope_ok(t_in)) {
            set_error("istft head, padding=\"center\": window overlap add min < 1e-11 (torch.istft raises here too)");
            return FV_ERR_INVALID;
        }
    }
    const bool wants_template = e->cfg.model == FV_MODEL_REFINEGAN ||
                                ((e->cfg.model == FV_MODEL_HIFIGAN || e->cfg.model == FV_MODEL_BIGVGAN || e->cfg.model == FV_MODEL_FIREFLY) &&
                                 e->cfg.ups.use_template);
    if (wants_template && !d_template) {
        set_error("fv_forward: this generator was built with use_template=True and needs a template (B, 1, T*hop)");
        return FV_ERR_INVALID;
    }
    if (!wants_template && d_template) {
        set_error("fv_forward: template given but the generator was built with use_template=False");
        return FV_ERR_INVALID;
    }
    return FV_OK;
}
// ... and what it sets up around run_model for the duration of the call: the template / noise of this call, the engine's conv algorithm and
// the profiler (detached again when the scope ends)
struct ForwardScope {
    AlgoScope algo;
    ForwardScope(fv_engine* e, const float* d_template, const float* d_noise) : algo(e->algo, e->invariant) {
        e->cur_template = d_template;
        e->cur_noise = d_noise;
        g_prof = e->profiling ? &e->prof : nullptr;
    }
    ~ForwardScope() { g_prof = nullptr; }
};

static fv_status forward_common(fv_engine* e, const float* d_in, const float* d_template, const float* d_noise, float* d_out,
                                int32_t batch, int32_t t_in, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (const fv_status st = check_forward(e, d_in, d_template, d_out, batch, t_in, d_workspace, workspace_bytes)) return st;
    const ForwardScope scope(e, d_template, d_noise);
    hipStream_t s = (hipStream_t)stream;
    float* ws = (float*)d_workspace;

    // hipGraph replay: a forward is ~110 launches plus fork/join events; at small batch the host launch cost dominates
    // (p50 clip latency).  The launch sequence is static for a given (pointers, batch, frames, stream), so the second
    // consecutive call with the same key is stream-captured (including the branch streams) and later calls replay it.
    // The legacy default stream (0: where the reference's own call runs, test.py:88-90) cannot be captured, but an instantiated graph can be launched on
    // it: the sequence is captured on an engine-owned stream and replayed on stream 0 — without the two cross-stream waits a redirect through a side
    // stream costs every call (single clip: ~0.04 ms of 0.75).
    fv_engine::GraphKey key{d_in, d_out, d_workspace, d_template, d_noise, batch, t_in, s};
    const bool graphable = e->use_graph && !e->profiling;
    if (graphable) {
        for (auto& g : e->graphs)
            if (g.key == key) {
                FV_HIP_CHECK(hipGraphLaunch(g.exec, s));
                return FV_OK;
            }
        if (e->have_last && e->last_key == key) {
            hipStream_t cs = s;
            if (!cs) {
                if (!e->null_capture && hipStreamCreateWithFlags(&e->null_capture, hipStreamNonBlocking) != hipSuccess) {
                    (void)hipGetLastError();
                    e->null_capture = nullptr;
                }
                cs = e->null_capture;
            }
            hipError_t be = cs ? hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) : hipErrorInvalidValue;
            if (be == hipSuccess) {
                fv_status st = e->run_model(d_in, d_out, batch, t_in, ws, cs);
                hipGraph_t graph = nullptr;
                hipError_t ee = hipStreamEndCapture(cs, &graph);
                if (st == FV_OK && ee == hipSuccess && graph) {
                    hipGraphExec_t exec = nullptr;
                    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                        if (e->graphs.size() >= 8) {
                            (void)hipGraphExecDestroy(e->graphs.front().exec);
                            (void)hipGraphDestroy(e->graphs.front().graph);
                            e->graphs.erase(e->graphs.begin());
                        }
                        e->graphs.push_back({key, graph, exec});
                        FV_HIP_CHECK(hipGraphLaunch(exec, s));
                        return FV_OK;
                    }
                    (void)hipGraphDestroy(graph);
                } else if (graph) {
                    (void)hipGraphDestroy(graph);
                }
                (void)hipGetLastError();
                e->use_graph = false;   // capture is not available in this context: stay eager from now on
                if (st) return st;
            } else {
                (void)hipGetLastError();
                e->use_graph = false;
            }
        }
        e->last_key = key;
        e->have_last = true;
    }
    return e->run_model(d_in, d_out, batch, t_in, ws, s);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// RefineGAN (refinegan.py:182-323)
// ------------------------------------------------------------------------------------------------
fv_status fv_engine::build_refinegan() {
    const fv_refinegan_config& c = cfg.refine;
    refine.cfg = c;
    const int S = c.num_stages;
    const bool f16 = false;   // the U-Net's narrow convs stay on the exact-fp32 kernels
    (void)f16;
    fv_status st;
    int ch = c.start_channels;
    if ((st = make_conv(refine.template_conv, "template_conv", false, 1, ch, 7, 1, 3, 1))) return st;
    auto make_resblock = [&](RefineResBlock& rb, const std::string& prefix, int cin, int cout, int k) -> fv_status {
        rb.k = k;
        rb.cin = cin;
        rb.cout = cout;
        static const int dil[3] = {1, 3, 5};
        for (int n = 0; n < 3; ++n) {
            fv_status s1 = make_conv(rb.c1[n], prefix + ".convs1." + std::to_string(n), false, n == 0 ? cin : cout, cout, k,
                                     dil[n], get_padding(k, dil[n]), 1);
            if (s1) return s1;
        }
        for (int n = 0; n < 3; ++n) {
            fv_status s2 = make_conv(rb.c2[n], prefix + ".convs2." + std::to_string(n), false, cout, cout, k, dil[n],
                                     get_padding(k, dil[n]), 1);
            if (s2) return s2;
        }
        return FV_OK;
    };
    for (int i = 0; i < S; ++i) {
        refine.downs.emplace_back(new RefineResBlock());
        if ((st = make_resblock(*refine.downs.back(), "downsample_blocks." + std::to_string(i) + ".1", ch, ch * 2, 7))) return st;
        ch *= 2;
    }
    if ((st = make_conv(refine.mel_conv, "mel_conv", false, c.num_mels, ch, 7, 1, 3, 1))) return st;
    ch *= 2;
    static const int ks[3] = {3, 7, 11};
    for (int i = 0; i < S; ++i) {
        refine.ups.emplace_back(new RefineUp());
        RefineUp& u = *refine.ups.back();
        u.rate = c.upsample_rates[i];
        u.cin = ch;
        u.cskip = ch / 4;
        u.cout = ch / 2;
        const std::string p = "upsample_conv_blocks." + std::to_string(i);
        if ((st = make_conv(u.input_conv, p + ".input_conv", false, u.cin + u.cskip, u.cout, 7, 1, 3, 1))) return st;
        for (int j = 0; j < 3; ++j) {
            const std::string bp = p + ".blocks." + std::to_string(j);
            if ((st = make_dev_vec(bp + ".0.weight", u.cout, &u.d_w1[j]))) return st;
            if ((st = make_resblock(u.rb[j], bp + ".1", u.cout, u.cout, ks[j]))) return st;
            if ((st = make_dev_vec(bp + ".2.weight", u.cout, &u.d_w2[j]))) return st;
        }
        ch = u.cout;
    }
    // output_conv: weight-normed Conv1d(ch -> 1, k7) + tanh on the narrow-output kernel
    std::vector<float> w, b;
    if ((st = conv_weight("output_conv", {1, ch, 7}, w))) return st;
    if ((st = vec("output_conv.bias", 1, b))) return st;
    if ((st = upload(w, &refine.d_wout))) return st;
    if ((st = upload(b, &refine.d_bout))) return st;
    refine.out_cin = ch;
    return FV_OK;
}

// Workspace: S skip tensors (sized exactly) + 7 transient buffers of the largest (C x length) tensor.
static size_t refine_max_elems(const RefineModel& m, const std::vector<int64_t>& down, const std::vector<int64_t>& up) {
    const int S = m.cfg.num_stages;
    int64_t mx = 0;
    int ch = m.cfg.start_channels;
    for (int i = 0; i < S; ++i) {
        mx = std::max<int64_t>(mx, (int64_t)2 * ch * down[i + 1]);   // ResBlock tensors of down block i (and the interp output)
        ch *= 2;
    }
    mx = std::max<int64_t>(mx, (int64_t)2 * ch * down[S]);           // cat([x, mel_conv(mel)])
    for (int i = 0; i < S; ++i) {
        const RefineUp& u = *m.ups[i];
        mx = std::max<int64_t>(mx, (int64_t)(u.cin + u.cskip) * up[i + 1]);
    }
    return (size_t)mx;
}
static size_t refine_ws_elems(const fv_engine* e, int B, int T) {
    std::vector<int64_t> down, up;
    if (!e->refine.lengths(T, down, up)) return 0;
    size_t skips = 0;
    int ch = e->refine.cfg.start_channels;
    for (int i = 0; i < e->refine.cfg.num_stages; ++i) {
        skips += ((size_t)ch * down[i] * B + 63) / 64 * 64;
        ch *= 2;
    }
    return skips + 7 * ((refine_max_elems(e->refine, down, up) * B + 63) / 64 * 64);
}

fv_status fv_engine::run_refinegan(const float* d_mel, float* d_out, int B, int T, float* ws, hipStream_t s) {
    const RefineModel& m = refine;
    const int S = m.cfg.num_stages;
    const float slope = m.cfg.leaky_relu_slope;
    std::vector<int64_t> down, up;
    if (!m.lengths(T, down, up)) {
        set_error("refinegan: the down/up-sampling lengths do not line up for %d frames (the reference's torch.cat would fail)", T);
        return FV_ERR_INVALID;
    }
    if (down[0] >= (1LL << 31)) {
        set_error("refinegan: clip too long");
        return FV_ERR_UNSUPPORTED;
    }
    // ---- workspace ----
    std::vector<float*> skip(S);
    float* wp = ws;
    {
        int ch = m.cfg.start_channels;
        for (int i = 0; i < S; ++i) {
            skip[i] = wp;
            wp += ((size_t)ch * down[i] * B + 63) / 64 * 64;
            ch *= 2;
        }
    }
    const size_t me = (refine_max_elems(m, down, up) * B + 63) / 64 * 64;
    float* P[7];
    for (int i = 0; i < 7; ++i) P[i] = wp + (size_t)i * me;
    fv_status st;
    ConvRun r;
    // one refinegan.ResBlock (refinegan.py:87-100): in -> out; XT, XB scratch; leaky_relu fused into c1's staging and epilogue
    auto resblock = [&](const RefineResBlock& rb, const float* in, float* out, float* XT, float* XB, int t,
                        bool post_leaky) -> fv_status {
        const float* src = in;
        for (int n = 0; n < 3; ++n) {
            ConvRun q;
            q.batch = B;
            q.t_in = t;
            q.x = src;
            q.y = XT;
            q.pre_act = FV_ACT_LEAKY_RELU;
            q.post_act = FV_ACT_LEAKY_RELU;
            q.slope = slope;
            fv_status e1 = conv_layer_run(rb.c1[n], q, s);
            if (e1) return e1;
            q = ConvRun();
            q.batch = B;
            q.t_in = t;
            q.x = XT;
            q.y = n == 2 ? out : XB;
            q.res = (n != 0 || rb.cin == rb.cout) ? src : nullptr;   // refinegan.py:95-98
            if (n == 2 && post_leaky) {
                q.post_act = FV_ACT_LEAKY_RELU;
                q.slope = slope;
            }
            fv_status e2 = conv_layer_run(rb.c2[n], q, s);
            if (e2) return e2;
            src = XB;
        }
        return FV_OK;
    };

    // ---- down path: x = template_conv(template); every leaky_relu_(x) of refinegan.py:305 is folded into its producer ----
    int ch = m.cfg.start_channels;
    r = ConvRun();
    r.batch = B;
    r.t_in = (int)down[0];
    r.x = cur_template;
    r.y = skip[0];
    r.post_act = FV_ACT_LEAKY_RELU;
    r.slope = slope;
    if ((st = conv_layer_run(m.template_conv, r, s))) return st;
    float* cat0 = P[5];   // cat([x, mel_conv(mel)]) : (2 * c_S, T)
    int c_s = ch;
    for (int i = 0; i < S; ++i) c_s *= 2;
    for (int i = 0; i < S; ++i) {
        const int rate = m.cfg.downsample_rates[i];
        const float scale = (float)(1.0 / (1.0 / (double)rate));   // aten: static_cast<float>(1.0 / scale_factor)
        FV_PROF(s, "linear_interp", 3.0 * B * ch * down[i + 1], 4.0 * B * ch * (down[i] + down[i + 1]),
                launch_leaky_interp(skip[i], P[0], B, ch, (int)down[i], (int)down[i + 1], scale, 0, slope, ch, 0, s));
        float* out = i + 1 < S ? skip[i + 1] : P[3];
        if ((st = resblock(*m.downs[i], P[0], out, P[1], P[2], (int)down[i + 1], /*post_leaky=*/true))) return st;
        ch *= 2;
    }
    FV_PROF(s, "copy_channels", 0.0, 8.0 * B * c_s * T, launch_copy_channels(P[3], cat0, B, c_s, T, 2 * c_s, 0, s));
    r = ConvRun();
    r.batch = B;
    r.t_in = T;
    r.x = d_mel;
    r.y = P[4];
    r.post_act = FV_ACT_LEAKY_RELU;   // the concatenated tensor is activated in place at the top of the up loop
    r.slope = slope;
    if ((st = conv_layer_run(m.mel_conv, r, s))) return st;
    FV_PROF(s, "copy_channels", 0.0, 8.0 * B * c_s * T, launch_copy_channels(P[4], cat0, B, c_s, T, 2 * c_s, c_s, s));

    // ---- up path ----
    const float* xcur = cat0;
    const float* noise = cur_noise;
    for (int i = 0; i < S; ++i) {
        const RefineUp& u = *m.ups[i];
        const int t = (int)up[i + 1];
        float* CAT = P[0];
        float* XI = P[1];
        float* XA = P[2];
        float* XT = P[3];
        float* XB = P[4];
        float* Y = (xcur == P[5]) ? P[6] : P[5];
        const float scale = (float)(1.0 / (double)u.rate);
        // x = leaky_relu_(x) (already applied by the producers for i == 0), upsample, cat with the skip
        FV_PROF(s, "linear_interp", 3.0 * B * u.cin * t, 4.0 * B * u.cin * (up[i] + t),
                launch_leaky_interp(xcur, CAT, B, u.cin, (int)up[i], t, scale, i > 0, slope, u.cin + u.cskip, 0, s));
        FV_PROF(s, "copy_channels", 0.0, 8.0 * B * u.cskip * t,
                launch_copy_channels(skip[S - 1 - i], CAT, B, u.cskip, t, u.cin + u.cskip, u.cin, s));
        r = ConvRun();
        r.batch = B;
        r.t_in = t;
        r.x = CAT;
        r.y = XI;
        if ((st = conv_layer_run(u.input_conv, r, s))) return st;
        const size_t nelem = (size_t)B * u.cout * t;
        for (int j = 0; j < 3; ++j) {
            FV_PROF(s, "adain", 3.0 * nelem, 12.0 * nelem, launch_adain(XI, noise, u.d_w1[j], XA, B, u.cout, t, kAdaINSlope, 0, 1.0f, s));
            noise += nelem;
            if ((st = resblock(u.rb[j], XA, CAT, XT, XB, t, /*post_leaky=*/false))) return st;   // CAT is free again: branch output
            FV_PROF(s, "adain", 4.0 * nelem, 16.0 * nelem,
                    launch_adain(CAT, noise, u.d_w2[j], Y, B, u.cout, t, kAdaINSlope, j > 0, j == 2 ? 1.0f / 3.0f : 1.0f, s));
            noise += nelem;
        }
        xcur = Y;
    }
    // leaky_relu -> output_conv -> tanh (refinegan.py:319-321)
    const int L = (int)up[S];
    FV_PROF(s, "conv_post_narrow", 2.0 * B * m.out_cin * 7 * L, 4.0 * B * (m.out_cin + 1) * L,
            launch_conv_narrow(xcur, m.d_wout, m.d_bout, d_out, B, m.out_cin, L, 1, 7, 3, FV_ACT_LEAKY_RELU, FV_ACT_TANH, slope, s));
    return FV_OK;
}

// ---- long clips as a batch of time tiles -------------------------------------------------------------------------
// One-sided reach of the generator in INPUT frames: an output sample depends on input frames no further away than this (an upper
// bound, walked backwards through the layers: every conv adds (k - 1) / 2 * dilation at its own rate, a transposed conv divides by
// its stride; the anti-aliased activations of BigVGAN add their two 12-tap filters at the doubled rate).
static int64_t ups_reach(const UpsamplerModel& m) {
    const fv_upsampler_config& c = m.cfg;
    const int aa = m.bigvgan ? 7 : 0;   // Activation1d: replicate-pad 5 + 6-tap polyphase up, 12-tap low-pass at 2x: <= 6.5 samples
    int64_t R = (c.post_conv_kernel_size - 1) / 2 + aa;
    for (int i = c.num_upsamples - 1; i >= 0; --i) {
        int64_t br = 0;
        for (int j = 0; j < c.num_kernels; ++j) {
            const int k = c.resblock_kernel_sizes[j];
            int64_t r = 0;
            for (int n = 0; n < FV_MAX_DILATIONS; ++n) r += (int64_t)(k - 1) / 2 * (c.resblock_dilation_sizes[j][n] + 1) + 2 * aa;
            br = std::max(br, r);
        }
        R += br + (c.use_template ? 2 : 0);   // noise_convs[i]: one stage sample either side of the strided template conv
        const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
        R = (R + k - 1) / u + 1;
    }
    return R + (c.pre_conv_kernel_size - 1) / 2;
}
static int64_t cnx_reach(const ConvNeXtModel& m) {
    int64_t R = m.cfg.kernel_size / 2;   // stem
    for (int i = 0; i < m.cfg.num_stages; ++i) R += (int64_t)m.cfg.depths[i] * (m.cfg.kernel_size / 2);
    return R;
}
int fv_engine::reach_frames() const {
    int64_t R = 0;
    switch (cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: R = ups_reach(ups); break;
        case FV_MODEL_CONVNEXT: R = cnx_reach(cnx); break;
        case FV_MODEL_ISTFT_HEAD: R = (cfg.head.n_fft + cfg.head.hop_length - 1) / cfg.head.hop_length; break;
        case FV_MODEL_VOCOS: R = cnx_reach(cnx) + (cfg.head.n_fft + cfg.head.hop_length - 1) / cfg.head.hop_length; break;
        case FV_MODEL_FIREFLY: R = cnx_reach(cnx) + ups_reach(ups); break;
        default: return -1;   // LOGMEL / REFINEGAN: not tiled
    }
    return (int)std::min<int64_t>(R + 2, 1 << 20);
}
// The frame-aligned models, the ones a window of frames [a, b) can stand in for: a finite reach, no "center" ISTFT trim, and exactly hop output
// samples per input frame at both t_a and t_b frames — the gather / scatter of the time tiles and the window / crop of a stream address rows at
// frames x hop.  Returns hop, or 0 with the reason in *why (may be NULL).  Used by tile_plan and fv_stream_create.
int fv_engine::frame_hop(int t_a, int t_b, const char** why) const {
    const char* r = nullptr;
    if (cfg.model == FV_MODEL_LOGMEL)
        r = "the log-mel front-end (wave -> mel) is not frame-windowed";
    else if (cfg.model == FV_MODEL_REFINEGAN)
        r = "RefineGAN cannot be windowed (its U-Net spans the whole clip and its AdaIN noise is drawn per call)";
    else if (reach_frames() < 0)
        r = "the model has no finite reach";
    else if ((cfg.model == FV_MODEL_VOCOS || cfg.model == FV_MODEL_ISTFT_HEAD) && head.center())
        r = "ISTFT head with padding=\"center\": the output is (T - 1) * hop samples, trimmed at both ends";
    if (!r && t_a >= 1 && t_b >= 1) {
        // A transposed conv with odd (kernel - rate) yields T u + 1 samples per stage (ConvLayer::out_len): not frames x hop
        const int64_t la = fv_output_length(this, t_a), lb = fv_output_length(this, t_b);
        const int64_t hop = la / t_a;
        if (hop >= 1 && la == hop * t_a && lb == hop * (int64_t)t_b) return (int)hop;
        r = "the output is not hop x frames samples (a transposed conv with odd kernel - rate adds a sample per stage)";
    }
    if (why) *why = r ? r : "empty input";
    return 0;
}
// Longest tile (frames) whose largest per-item tensor stays under HALF the 4 GiB addressing span of the conv kernels
int fv_engine::tile_frame_limit() const {
    int64_t per_frame = 1;
    switch (cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: per_frame = ups.max_elems(1 << 10) >> 10; break;
        case FV_MODEL_CONVNEXT: per_frame = 4LL * cnx.max_dim(); break;
        case FV_MODEL_ISTFT_HEAD: per_frame = std::max<int64_t>(2 * head.nb, cfg.head.n_fft); break;
        case FV_MODEL_VOCOS: per_frame = std::max<int64_t>(4LL * cnx.max_dim(), std::max<int64_t>(2 * head.nb, cfg.head.n_fft)); break;
        case FV_MODEL_FIREFLY: per_frame = std::max<int64_t>(4LL * cnx.max_dim(), ups.max_elems(1 << 10) >> 10); break;
        default: return 0;
    }
    return (int)std::min<int64_t>((1LL << 29) / std::max<int64_t>(per_frame, 1), 1 << 30);
}
fv_engine::TilePlan fv_engine::tile_plan(int t_in) const {
    TilePlan p;
    const int reach = reach_frames();
    int limit = tile_frame_limit();   // 0 for the models that are never tiled (LOGMEL / REFINEGAN)
    if (tile_frames_override > 0) limit = std::min(limit, std::max(tile_frames_override, 4 * reach));
    if (limit <= 0 || t_in <= limit) return p;
    if (limit < 4 * reach) return p;   // (a model whose reach does not fit the span: the per-layer check reports it)
    // The gather / scatter address tiles and clips at exactly frames x hop samples: a model that is not frame-aligned (frame_hop: e.g. a "center"
    // ISTFT head, or odd (kernel - rate) upsamplers) runs whole, and past the addressing span the per-layer check refuses it by name.
    if (frame_hop(limit, t_in, nullptr) < 1) return p;
    p.halo = reach;
    p.L = limit;
    p.stride = p.L - 2 * p.halo;
    // n tiles cover [0, T): the last one is pulled back to end at T
    p.n = (int)(((int64_t)t_in - 2 * p.halo + p.stride - 1) / p.stride);
    if (p.n < 2) p.n = 2;
    return p;
}

fv_status fv_engine::run_model(const float* d_in, float* d_out, int batch, int t_in, float* ws, hipStream_t s) {
    const TilePlan tp = tile_plan(t_in);
    if (tp.n <= 1) return run_model_whole(d_in, d_out, batch, t_in, ws, s);
    // [input tiles | template tiles | output tiles | the model's own workspace for (batch * n) items of L frames]
    const int cin = fv_input_channels(this), cout = fv_output_channels(this);
    const int64_t lout = fv_output_length(this, tp.L), clip_out = fv_output_length(this, t_in);
    const int hop = (int)(lout / tp.L);
    const int bn = batch * tp.n;
    const size_t n_in = align_up((size_t)bn * cin * tp.L, 64), n_out = align_up((size_t)bn * cout * lout, 64);
    const size_t n_tm = cur_template ? align_up((size_t)bn * lout, 64) : 0;
    float* tin = ws;
    float* ttm = ws + n_in;
    float* tout = ttm + n_tm;
    float* mws = tout + n_out;
    fv_status st;
    FV_PROF(s, "gather_tiles", 0.0, 8.0 * bn * cin * tp.L, launch_gather_tiles(d_in, tin, batch, cin, t_in, tp.n, tp.L, tp.stride, 1, s));
    const float* clip_template = cur_template;
    if (cur_template) {
        FV_PROF(s, "gather_tiles", 0.0, 8.0 * bn * lout, launch_gather_tiles(cur_template, ttm, batch, 1, t_in, tp.n, tp.L, tp.stride, hop, s));
        cur_template = ttm;
    }
    st = run_model_whole(tin, tout, bn, tp.L, mws, s);
    cur_template = clip_template;
    if (st) return st;
    FV_PROF(s, "scatter_tiles", 0.0, 8.0 * batch * cout * clip_out,
            launch_scatter_tiles(tout, d_out, batch, cout, t_in, tp.n, tp.L, tp.stride, tp.halo, hop, s));
    return FV_OK;
}

fv_status fv_engine::run_model_whole(const float* d_in, float* d_out, int batch, int t_in, float* ws, hipStream_t s) {
    fv_engine* e = this;
    switch (e->cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: return e->run_upsampler(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_CONVNEXT: return e->run_convnext(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_ISTFT_HEAD: return e->run_head(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_LOGMEL:
            if (e->mel.frames(t_in) < 1 || t_in <= std::max(e->mel.pad_l, e->mel.pad_r)) {
                set_error("logmel: %d samples is too short for reflect padding %d/%d and one %d-sample frame", t_in, e->mel.pad_l,
                          e->mel.pad_r, e->cfg.mel.n_fft);
                return FV_ERR_INVALID;
            }
            return e->run_logmel(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_REFINEGAN: return e->run_refinegan(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_VOCOS: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            fv_status st = e->run_convnext(d_in, ws, batch, t_in, ws + mid, s);
            if (st) return st;
            return e->run_head(ws, d_out, batch, t_in, ws + mid, s);
        }
        case FV_MODEL_FIREFLY: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            fv_status st = e->run_convnext(d_in, ws, batch, t_in, ws + mid, s);
            if (st) return st;
            return e->run_upsampler(ws, d_out, batch, t_in, ws + mid, s);
        }
    }
    set_error("fv_forward: unknown model");
    return FV_ERR_INVALID;
}

// ---- streaming synthesis ---------------------------------------------------------------------------------------------
// B sessions advance in lockstep.  Host counters: F frames received, E emitted.  A push of n frames appends them (F += n) and emits the frames
// [E, E'), E' = max(E, F - A), out of ONE forward over the window [w, F), w = max(0, E - K); a flush does the same with E' = F.  With K and A
// >= the reach every emitted frame lies >= R frames inside each window edge that is not the utterance's own, so the window reproduces the whole
// utterance's samples there (the rule of the time tiles, tile_plan).  The window is assembled in the caller's workspace at fixed addresses: a
// steady-state push (fixed n: W = K + A + n frames) hands forward_common the same (buffers, batch, frames, stream) as the one before and
// replays its captured graph.
struct fv_stream {
    fv_engine* e = nullptr;
    int B = 0, max_chunk = 0, K = 0, A = 0, cin = 0, cout = 0, hop = 0;
    int64_t cap = 0;              // ring length in frames: K + A + max_chunk, >= every window the stream forms
    bool tmpl = false;            // use_template generator: a template ring at the hop rate beside the mel ring
    float* ring = nullptr;        // (B, C_in, cap), then (B, 1, cap * hop) for the template: the stream's only device allocation
    float* ring_tmpl = nullptr;
    size_t n_win_in = 0, n_win_tmpl = 0, n_win_out = 0;   // workspace: window input | window template | window output (floats, 256-byte
    size_t model_bytes = 0;                                //   aligned each) | the forward's own workspace for the largest window
    int64_t F = 0, E = 0;
    bool flushed = false;
    size_t ws_bytes() const { return (n_win_in + n_win_tmpl + n_win_out) * sizeof(float) + model_bytes; }
    ~fv_stream() {
        if (ring) (void)hipFree(ring);
    }
};

static fv_status stream_step(fv_stream* st, const float* d_mel, const float* d_template, int32_t n, bool flush, float* d_out,
                             int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = flush ? "fv_stream_flush" : "fv_stream_push";
    if (frames_out) *frames_out = 0;
    if (!st || !frames_out) {
        set_error("%s: null argument", fn);
        return FV_ERR_INVALID;
    }
    if (st->flushed) {
        set_error("%s: the stream was flushed; fv_stream_reset it before the next utterance", fn);
        return FV_ERR_STATE;
    }
    if (!flush) {
        if (n < 0 || n > st->max_chunk) {
            set_error("fv_stream_push: %d frames, more than max_chunk_frames = %d of this stream", n, st->max_chunk);
            return FV_ERR_INVALID;
        }
        if (n == 0) return FV_OK;
        if (!d_mel) {
            set_error("fv_stream_push: null mel chunk");
            return FV_ERR_INVALID;
        }
        if (st->tmpl && !d_template) {
            set_error("fv_stream_push: the generator was built with use_template=True and every push needs a template chunk (B, 1, n*hop)");
            return FV_ERR_INVALID;
        }
        if (!st->tmpl && d_template) {
            set_error("fv_stream_push: template given but the generator was built with use_template=False");
            return FV_ERR_INVALID;
        }
    }
    if (!d_workspace || workspace_bytes < st->ws_bytes()) {
        set_error("%s: workspace too small (%zu < %zu bytes, fv_stream_workspace_bytes)", fn, d_workspace ? workspace_bytes : (size_t)0,
                  st->ws_bytes());
        return FV_ERR_INVALID;
    }
    const int64_t F = st->F + (flush ? 0 : n);
    const int64_t E2 = flush ? F : std::max(st->E, F - st->A);
    const bool emit = E2 > st->E;
    if (emit && !d_out) {
        set_error("%s: null output (this call emits %lld frames)", fn, (long long)(E2 - st->E));
        return FV_ERR_INVALID;
    }
    fv_engine* e = st->e;
    const int B = st->B, hop = st->hop;
    const int64_t w = emit ? std::max<int64_t>(0, st->E - st->K) : st->F;   // no emission: the chunk only goes into the ring
    hipStream_t s = (hipStream_t)stream;
    float* win_in = (float*)d_workspace;
    float* win_tmpl = win_in + st->n_win_in;
    float* win_out = win_tmpl + st->n_win_tmpl;
    float* mws = win_out + st->n_win_out;
    struct ProfGuard {
        fv_engine* e;
        void on() { g_prof = e->profiling ? &e->prof : nullptr; }
        ~ProfGuard() { g_prof = nullptr; }
    } guard{e};
    guard.on();
    if (!flush || emit) {
        // the chunk into the ring at F mod cap, and the window [w, F) beside it; a flush has no chunk (n = 0: the window comes from the ring alone)
        const int64_t nc = flush ? 0 : n, W = F - w;
        FV_PROF(s, "stream_window", 0.0, 4.0 * B * st->cin * (2.0 * nc + (emit ? 2.0 * W : 0.0)),
                launch_stream_window(d_mel, st->ring, emit ? win_in : nullptr, B, st->cin, st->cap, st->F, nc, w, s));
        if (st->tmpl)
            FV_PROF(s, "stream_window", 0.0, 4.0 * B * hop * (2.0 * nc + (emit ? 2.0 * W : 0.0)),
                    launch_stream_window(d_template, st->ring_tmpl, emit ? win_tmpl : nullptr, B, 1, st->cap * hop, st->F * hop, nc * hop, w * hop, s));
    }
    if (emit) {
        const int W = (int)(F - w);
        const fv_status r = forward_common(e, win_in, st->tmpl ? win_tmpl : nullptr, nullptr, win_out, B, W, mws, st->model_bytes, stream);
        if (r) return r;
        guard.on();   // (forward_common leaves the profiler detached)
        const int64_t len = (E2 - st->E) * hop;
        FV_PROF(s, "stream_crop", 0.0, 8.0 * B * st->cout * len,
                launch_stream_crop(win_out, d_out, B, st->cout, (int64_t)W * hop, (st->E - w) * hop, len, s));
    }
    *frames_out = E2 - st->E;
    st->F = F;
    st->E = E2;
    if (flush) st->flushed = true;
    return FV_OK;
}

extern "C" {

FV_API int32_t fv_reach_frames(const fv_engine* e) {
    if (!e || !e->finalized || e->frame_hop(1, 2, nullptr) < 1) return -1;
    return e->reach_frames();
}

FV_API fv_status fv_stream_create(fv_engine* e, const fv_stream_config* cfg, fv_stream** out) {
    if (!e || !cfg || !out) {
        set_error("fv_stream_create: null argument");
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (!e->finalized) {
        set_error("fv_stream_create: call fv_finalize first");
        return FV_ERR_STATE;
    }
    const char* why = nullptr;
    const int hop = e->frame_hop(1, 2, &why);
    if (hop < 1) {
        set_error("fv_stream_create: this model cannot stream: %s", why);
        return FV_ERR_UNSUPPORTED;
    }
    const int R = e->reach_frames();
    if (cfg->batch < 1 || cfg->max_chunk_frames < 1 || cfg->context_frames < -1 || cfg->lookahead_frames < -1) {
        set_error("fv_stream_create: batch (%d) and max_chunk_frames (%d) must be >= 1, context_frames (%d) and lookahead_frames (%d) >= 0 "
                  "(-1: the reach, %d frames)", cfg->batch, cfg->max_chunk_frames, cfg->context_frames, cfg->lookahead_frames, R);
        return FV_ERR_INVALID;
    }
    std::unique_ptr<fv_stream> st(new fv_stream());
    st->e = e;
    st->B = cfg->batch;
    st->max_chunk = cfg->max_chunk_frames;
    st->K = cfg->context_frames < 0 ? R : cfg->context_frames;
    st->A = cfg->lookahead_frames < 0 ? R : cfg->lookahead_frames;
    st->cin = fv_input_channels(e);
    st->cout = fv_output_channels(e);
    st->hop = hop;
    st->cap = (int64_t)st->K + st->A + st->max_chunk;
    st->tmpl = (e->cfg.model == FV_MODEL_HIFIGAN || e->cfg.model == FV_MODEL_BIGVGAN || e->cfg.model == FV_MODEL_FIREFLY) && e->cfg.ups.use_template;
    if (st->cap > (1 << 20)) {
        set_error("fv_stream_create: context + lookahead + max_chunk_frames = %lld frames, more than 2^20", (long long)st->cap);
        return FV_ERR_INVALID;
    }
    // Every window length the stream can form (1 ... cap frames) must be frame-aligned; the forward's workspace is the largest over them
    // (fv_workspace_bytes need not be monotone in t_in: the tile plan switches in at the addressing span)
    for (int W = 1; W <= st->cap; ++W) {
        if (e->frame_hop(1, W, &why) != hop) {
            set_error("fv_stream_create: this model cannot stream: %s (%d-frame window)", why, W);
            return FV_ERR_UNSUPPORTED;
        }
        const size_t b = fv_workspace_bytes(e, st->B, W);
        if (b == 0) {
            set_error("fv_stream_create: no forward of %d x %d frames fits (split the batch)", st->B, W);
            return FV_ERR_UNSUPPORTED;
        }
        st->model_bytes = std::max(st->model_bytes, b);
    }
    const size_t cap = (size_t)st->cap, B = (size_t)st->B;
    st->n_win_in = align_up(B * st->cin * cap, 64);
    st->n_win_tmpl = st->tmpl ? align_up(B * cap * hop, 64) : 0;
    st->n_win_out = align_up(B * st->cout * cap * hop, 64);
    const size_t n_ring = align_up(B * st->cin * cap, 64), n_ring_tmpl = st->tmpl ? B * cap * hop : 0;
    FV_HIP_CHECK(hipMalloc((void**)&st->ring, (n_ring + n_ring_tmpl) * sizeof(float)));
    st->ring_tmpl = st->tmpl ? st->ring + n_ring : nullptr;
    *out = st.release();
    return FV_OK;
}

FV_API size_t fv_stream_workspace_bytes(const fv_stream* s) { return s ? s->ws_bytes() : 0; }

FV_API int64_t fv_stream_pending_frames(const fv_stream* s) { return s ? s->F - s->E : 0; }

FV_API fv_status fv_stream_push(fv_stream* s, const float* d_mel, const float* d_template, int32_t n, float* d_out, int64_t* frames_out,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    return stream_step(s, d_mel, d_template, n, false, d_out, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_stream_flush(fv_stream* s, float* d_out, int64_t* frames_out, void* d_workspace, size_t workspace_bytes, void* stream) {
    return stream_step(s, nullptr, nullptr, 0, true, d_out, frames_out, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_stream_reset(fv_stream* s) {
    if (!s) {
        set_error("fv_stream_reset: null stream");
        return FV_ERR_INVALID;
    }
    s->F = s->E = 0;
    s->flushed = false;
    return FV_OK;
}

FV_API void fv_stream_destroy(fv_stream* s) { delete s; }

}  // extern "C"

// ---- ragged batches ----------------------------------------------------------------------------------------------------
// The plan (include/fishvoc.h states it; vocoder_amd/ragged.py restates it in Python, and the tests compare the two window for window).
static constexpr int kRaggedLaunchFrames = 192, kRaggedMaxGroups = 8;

static fv_status ragged_plan(int reach, const int32_t* lengths, int batch, int launch_frames, int max_groups, std::vector<fv_ragged_window>& out) {
    out.clear();
    if (reach < 1 || reach > (1 << 20) || !lengths || batch < 1) {
        set_error("fv_ragged_plan: reach (%d) and batch (%d) must be >= 1 and the lengths given", reach, batch);
        return FV_ERR_INVALID;
    }
    for (int b = 0; b < batch; ++b)
        if (lengths[b] < 0) {
            set_error("fv_ragged_plan: negative length %d of clip %d", lengths[b], b);
            return FV_ERR_INVALID;
        }
    if (launch_frames <= 0) launch_frames = kRaggedLaunchFrames;
    if (max_groups <= 0) max_groups = kRaggedMaxGroups;
    const int R2 = 2 * reach;
    std::vector<std::pair<int, int>> lng;   // (T, b) of the long clips, ascending
    for (int b = 0; b < batch; ++b)
        if (lengths[b] > R2) lng.emplace_back(lengths[b], b);
    std::sort(lng.begin(), lng.end());
    const int m = (int)lng.size();
    struct Item {
        int n, b, a, lo, hi;
    };
    std::vector<Item> items;
    if (m > 0) {
        // f[k][j]: the least cost of the first j clips in exactly k runs; a run [i, j) costs (j - i) Tg + 2R #{T < Tg} + launch_frames
        const int K = std::min(max_groups, m);
        const int64_t INF = (int64_t)1 << 62;
        std::vector<int> first_eq(m);   // first index of the block of equal lengths that clip j belongs to
        for (int j = 0; j < m; ++j) first_eq[j] = (j > 0 && lng[j].first == lng[j - 1].first) ? first_eq[j - 1] : j;
        std::vector<std::vector<int64_t>> f(K + 1, std::vector<int64_t>(m + 1, INF));
        std::vector<std::vector<int>> arg(K + 1, std::vector<int>(m + 1, -1));
        f[0][0] = 0;
        for (int k = 1; k <= K; ++k)
            for (int j = k; j <= m; ++j) {
                if (j < m && lng[j].first == lng[j - 1].first) continue;   // no cut between two clips of one length
                for (int i = k - 1; i < j; ++i) {
                    if (f[k - 1][i] >= INF) continue;
                    const int64_t c = f[k - 1][i] + (int64_t)(j - i) * lng[j - 1].first + (int64_t)R2 * std::max(0, first_eq[j - 1] - i) + launch_frames;
                    if (c < f[k][j]) {   // strict: the earliest start wins a tie
                        f[k][j] = c;
                        arg[k][j] = i;
                    }
                }
            }
        int best = 1;
        for (int k = 2; k <= K; ++k)
            if (f[k][m] < f[best][m]) best = k;   // strict: the fewest runs win a tie
        for (int k = best, j = m; k >= 1; --k) {
            const int i = arg[k][j], tg = lng[j - 1].first;
            for (int t = i; t < j; ++t) {
                const int T = lng[t].first, b = lng[t].second;
                if (T == tg) {
                    items.push_back({tg, b, 0, 0, T});
                } else {
                    items.push_back({tg, b, 0, 0, T - reach});
                    items.push_back({R2, b, T - R2, T - reach, T});
                }
            }
            j = i;
        }
    }
    for (int b = 0; b < batch; ++b)
        if (lengths[b] >= 1 && lengths[b] <= R2) items.push_back({lengths[b], b, 0, 0, lengths[b]});
    std::sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.n != y.n ? x.n > y.n : x.b < y.b; });
    int group = -1, prev = -1;
    for (const Item& it : items) {
        if (it.n != prev) {
            ++group;
            prev = it.n;
        }
        out.push_back({it.b, it.a, it.n, it.lo, it.hi, group});
    }
    return FV_OK;
}

struct fv_ragged {
    fv_engine* e = nullptr;
    int B = 0, t_max = 0, cin = 0, cout = 0, hop = 0, min_len = 0;
    bool tmpl = false;
    std::vector<fv_ragged_window> win;
    struct Group {
        int first, count, frames;
    };
    std::vector<Group> groups;
    fv_ragged_window* d_win = nullptr;   // the window table, then the lengths: the plan's only device allocation
    int32_t* d_len = nullptr;
    size_t n_in = 0, n_tmpl = 0, n_out = 0;   // workspace: window input | window template | window output (floats, sized for the largest group)
    size_t model_bytes = 0;                   //   | the largest group's own workspace
    size_t ws_bytes() const { return (n_in + n_tmpl + n_out) * sizeof(float) + model_bytes; }
    ~fv_ragged() {
        if (d_win) (void)hipFree(d_win);
    }
};

static int32_t copy_windows(const std::vector<fv_ragged_window>& w, fv_ragged_window* out, int32_t cap) {
    if (out && cap > 0) std::copy(w.begin(), w.begin() + std::min<size_t>(w.size(), (size_t)cap), out);
    return (int32_t)w.size();
}

extern "C" {

FV_API int32_t fv_ragged_plan(int32_t reach, const int32_t* host_lengths, int32_t batch, int32_t launch_frames, int32_t max_groups,
                              fv_ragged_window* out, int32_t cap) {
    std::vector<fv_ragged_window> w;
    if (const fv_status st = ragged_plan(reach, host_lengths, batch, launch_frames, max_groups, w)) return st;
    if (cap < 0 || (cap > 0 && !out)) {
        set_error("fv_ragged_plan: cap = %d without room for it", cap);
        return FV_ERR_INVALID;
    }
    return copy_windows(w, out, cap);
}

FV_API fv_status fv_ragged_create(fv_engine* e, const int32_t* host_lengths, int32_t batch, int32_t t_max, int32_t launch_frames,
                                  int32_t max_groups, fv_ragged** out) {
    if (!e || !host_lengths || !out) {
        set_error("fv_ragged_create: null argument");
        return FV_ERR_INVALID;
    }
    *out = nullptr;
    if (!e->finalized) {
        set_error("fv_ragged_create: call fv_finalize first");
        return FV_ERR_STATE;
    }
    const char* why = nullptr;
    const int hop = e->frame_hop(1, 2, &why);
    if (hop < 1) {
        set_error("fv_ragged_create: this model cannot run ragged batches: %s", why);
        return FV_ERR_UNSUPPORTED;
    }
    if (batch < 1 || t_max < 1) {
        set_error("fv_ragged_create: batch (%d) and t_max (%d) must be >= 1", batch, t_max);
        return FV_ERR_INVALID;
    }
    for (int b = 0; b < batch; ++b)
        if (host_lengths[b] < 0 || host_lengths[b] > t_max) {
            set_error("fv_ragged_create: length %d of clip %d is outside [0, t_max = %d]", host_lengths[b], b, t_max);
            return FV_ERR_INVALID;
        }
    std::unique_ptr<fv_ragged> p(new fv_ragged());
    p->e = e;
    p->B = batch;
    p->t_max = t_max;
    p->cin = fv_input_channels(e);
    p->cout = fv_output_channels(e);
    p->hop = hop;
    p->tmpl = (e->cfg.model == FV_MODEL_HIFIGAN || e->cfg.model == FV_MODEL_BIGVGAN || e->cfg.model == FV_MODEL_FIREFLY) && e->cfg.ups.use_template;
    p->min_len = *std::min_element(host_lengths, host_lengths + batch);
    if (const fv_status st = ragged_plan(e->reach_frames(), host_lengths, batch, launch_frames, max_groups, p->win)) return st;
    size_t max_items = 0;
    for (int i = 0; i < (int)p->win.size(); ++i) {
        const fv_ragged_window& w = p->win[i];
        // what the kernels rely on: the window starts inside the clip and its kept frames lie inside the window and the clip
        if (w.start < 0 || w.start >= host_lengths[w.clip] || w.keep_lo < w.start || w.keep_hi > std::min(w.start + w.frames, host_lengths[w.clip]) ||
            w.keep_lo >= w.keep_hi) {
            set_error("fv_ragged_create: internal error, window %d of the plan is malformed", i);
            return FV_ERR_STATE;
        }
        if (p->groups.empty() || w.group != (int)p->groups.size() - 1) p->groups.push_back({i, 0, w.frames});
        p->groups.back().count++;
    }
    for (const auto& g : p->groups) {
        if (e->frame_hop(1, g.frames, &why) != hop) {
            set_error("fv_ragged_create: this model cannot run ragged batches: %s (%d-frame window)", why, g.frames);
            return FV_ERR_UNSUPPORTED;
        }
        const size_t b = fv_workspace_bytes(e, g.count, g.frames);
        if (b == 0) {
            set_error("fv_ragged_create: no forward of %d x %d frames fits (split the batch)", g.count, g.frames);
            return FV_ERR_UNSUPPORTED;
        }
        p->model_bytes = std::max(p->model_bytes, b);
        max_items = std::max(max_items, (size_t)g.count * g.frames);
    }
    p->n_in = align_up(max_items * p->cin, 64);
    p->n_tmpl = p->tmpl ? align_up(max_items * hop, 64) : 0;
    p->n_out = align_up(max_items * p->cout * hop, 64);
    const size_t wbytes = align_up(p->win.size() * sizeof(fv_ragged_window), 256);
    FV_HIP_CHECK(hipMalloc((void**)&p->d_win, wbytes + (size_t)batch * sizeof(int32_t)));
    p->d_len = (int32_t*)((char*)p->d_win + wbytes);
    if (!p->win.empty()) FV_HIP_CHECK(hipMemcpy(p->d_win, p->win.data(), p->win.size() * sizeof(fv_ragged_window), hipMemcpyHostToDevice));
    FV_HIP_CHECK(hipMemcpy(p->d_len, host_lengths, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice));
    *out = p.release();
    return FV_OK;
}

FV_API size_t fv_ragged_workspace_bytes(const fv_ragged* p) { return p ? p->ws_bytes() : 0; }

FV_API int32_t fv_ragged_num_groups(const fv_ragged* p) { return p ? (int32_t)p->groups.size() : 0; }

FV_API int32_t fv_ragged_group(const fv_ragged* p, int32_t g, int32_t* batch, int32_t* frames) {
    if (!p || g < 0 || g >= (int32_t)p->groups.size()) {
        set_error("fv_ragged_group: no group %d", g);
        return FV_ERR_INVALID;
    }
    if (batch) *batch = p->groups[g].count;
    if (frames) *frames = p->groups[g].frames;
    return FV_OK;
}

FV_API int32_t fv_ragged_windows(const fv_ragged* p, fv_ragged_window* out, int32_t cap) {
    if (!p || cap < 0 || (cap > 0 && !out)) {
        set_error("fv_ragged_windows: null argument");
        return FV_ERR_INVALID;
    }
    return copy_windows(p->win, out, cap);
}

FV_API fv_status fv_ragged_forward(fv_ragged* p, const float* d_in, const float* d_template, float* d_out, void* d_workspace,
                                   size_t workspace_bytes, void* stream) {
    if (!p || !d_in || !d_out) {
        set_error("fv_ragged_forward: null argument");
        return FV_ERR_INVALID;
    }
    if (!d_workspace || workspace_bytes < p->ws_bytes()) {
        set_error("fv_ragged_forward: workspace too small (%zu < %zu bytes, fv_ragged_workspace_bytes)", d_workspace ? workspace_bytes : (size_t)0,
                  p->ws_bytes());
        return FV_ERR_INVALID;
    }
    fv_engine* e = p->e;
    float* win_in = (float*)d_workspace;
    float* win_tmpl = win_in + p->n_in;
    float* win_out = win_tmpl + p->n_tmpl;
    float* mws = win_out + p->n_out;
    const float* group_tmpl = d_template ? win_tmpl : nullptr;   // (a missing / unexpected template: check_forward's message)
    if (p->tmpl != (d_template != nullptr)) {   // (stated here too: a batch of empty clips runs no forward that would check it)
        set_error(p->tmpl ? "fv_forward: this generator was built with use_template=True and needs a template (B, 1, T*hop)"
                          : "fv_forward: template given but the generator was built with use_template=False");
        return FV_ERR_INVALID;
    }
    for (const auto& g : p->groups)   // everything is checked before anything is enqueued
        if (const fv_status st = check_forward(e, win_in, group_tmpl, win_out, g.count, g.frames, mws, p->model_bytes)) return st;
    hipStream_t s = (hipStream_t)stream;
    const int hop = p->hop;
    const long long T = p->t_max;
    const ForwardScope scope(e, nullptr, nullptr);
    for (const auto& g : p->groups) {
        const long long n = g.frames;
        FV_PROF(s, "ragged_gather", 0.0, 8.0 * g.count * p->cin * n,
                launch_ragged_gather(d_in, win_in, p->d_win, p->d_len, g.first, g.count, p->cin, T, n, 1, s));
        if (p->tmpl)
            FV_PROF(s, "ragged_gather", 0.0, 8.0 * g.count * n * hop,
                    launch_ragged_gather(d_template, win_tmpl, p->d_win, p->d_len, g.first, g.count, 1, T * hop, n * hop, hop, s));
        e->cur_template = group_tmpl;
        // eagerly, past forward_common's graph bookkeeping: a ragged call neither evicts a captured graph nor resets the last key
        const fv_status st = e->run_model(win_in, win_out, g.count, g.frames, mws, s);
        if (st) return st;
        FV_PROF(s, "ragged_scatter", 0.0, 8.0 * g.count * p->cout * n * hop,
                launch_ragged_scatter(win_out, d_out, p->d_win, g.first, g.count, p->cout, T * hop, n * hop, hop, s));
    }
    FV_PROF(s, "ragged_zero_tail", 0.0, 4.0 * p->B * p->cout * (double)(p->t_max - p->min_len) * hop,
            launch_ragged_zero_tail(d_out, p->d_len, p->B, p->cout, T * hop, (long long)(p->t_max - p->min_len) * hop, hop, s));
    return FV_OK;
}

FV_API void fv_ragged_destroy(fv_ragged* p) { delete p; }

// ---- per-launch profile ----
FV_API fv_status fv_profile_begin(fv_engine* e) {
    if (!e) {
        set_error("fv_profile_begin: null engine");
        return FV_ERR_INVALID;
    }
    for (auto& r : e->prof.recs) {
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
    }
    e->prof.recs.clear();
    e->profiling = true;
    return FV_OK;
}

FV_API fv_status fv_profile_end(fv_engine* e, char* json_buf, size_t cap, size_t* needed) {
    if (!e) {
        set_error("fv_profile_end: null engine");
        return FV_ERR_INVALID;
    }
    e->profiling = false;
    struct Agg {
        int count = 0;
        double ms = 0, flops = 0, bytes = 0;
    };
    std::map<std::string, Agg> agg;
    std::vector<std::string> order;
    for (auto& r : e->prof.recs) {
        if (!r.e0 || !r.e1) continue;
        FV_HIP_CHECK(hipEventSynchronize(r.e1));
        float ms = 0.f;
        FV_HIP_CHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
        if (!agg.count(r.label)) order.push_back(r.label);
        Agg& a = agg[r.label];
        a.count++;
        a.ms += ms;
        a.flops += r.flops;
        a.bytes += r.bytes;
    }
    std::string js = "[";
    for (size_t i = 0; i < order.size(); ++i) {
        const Agg& a = agg[order[i]];
        char buf[512];
        std::snprintf(buf, sizeof(buf),
                      "%s{\"kernel\": \"%s\", \"launches\": %d, \"total_ms\": %.6f, \"avg_ms\": %.6f, "
                      "\"flops_per_launch\": %.1f, \"bytes_per_launch\": %.1f}",
                      i ? ", " : "", order[i].c_str(), a.count, a.ms, a.ms / a.count, a.flops / a.count, a.bytes / a.count);
        js += buf;
    }
    js += "]";
    for (auto& r : e->prof.recs) {
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
    }
    e->prof.recs.clear();
    if (needed) *needed = js.size() + 1;
    if (json_buf && cap > 0) {
        const size_t n = std::min(cap - 1, js.size());
        std::memcpy(json_buf, js.data(), n);
        json_buf[n] = 0;
    }
    return FV_OK;
}

// ---- single conv layer ----
struct fv_conv {
    ConvLayer L;
    fv_conv_desc desc;
};

FV_API fv_status fv_conv_create(const fv_conv_desc* d, const float* host_weight, const float* host_bias, fv_conv** out) {
    if (!d || !host_weight || !out) {
        set_error("fv_conv_create: null argument");
        return FV_ERR_INVALID;
    }
    fv_conv* c = new (std::nothrow) fv_conv();
    if (!c) {
        set_error("out of host memory");
        return FV_ERR_INVALID;
    }
    c->desc = *d;
    fv_status st = conv_layer_create(c->L, d->transposed != 0, d->c_in, d->c_out, d->kernel_size,
                                     d->transposed ? 1 : d->dilation, d->padding, d->transposed ? d->stride : 1,
                                     host_weight, host_bias, /*with_f16x3=*/true);
    if (st) {
        conv_layer_destroy(c->L);
        delete c;
        return st;
    }
    *out = c;
    return FV_OK;
}

FV_API int64_t fv_conv_output_length(const fv_conv* c, int32_t t_in) { return c ? c->L.out_len(t_in) : 0; }

FV_API fv_status fv_conv_forward(fv_conv* c, const float* d_x, float* d_y, const float* d_residual, int32_t batch, int32_t t_in,
                          void* stream) {
    if (!c || !d_x || !d_y) {
        set_error("fv_conv_forward: null argument");
        return FV_ERR_INVALID;
    }
    ConvRun r;
    r.x = d_x;
    r.y = d_y;
    r.res = d_residual;
    r.batch = batch;
    r.t_in = t_in;
    r.pre_act = c->desc.pre_act;
    r.post_act = c->desc.post_act;
    r.slope = c->desc.act_slope;
    const AlgoScope algo_scope(c->L.algo, false);
    return conv_layer_run(c->L, r, (hipStream_t)stream);
}

/* y = x + c2(silu(c1(silu(x)))) in one launch (narrow channels only); c1/c2 are fv_conv handles of equal C and k. */
FV_API fv_status fv_conv_pair_forward(fv_conv* c1, fv_conv* c2, const float* d_x, float* d_y, int32_t batch, int32_t t,
                                      void* stream) {
    if (!c1 || !c2 || !d_x || !d_y) {
        set_error("fv_conv_pair_forward: null argument");
        return FV_ERR_INVALID;
    }
    if (batch < 1 || t < 1) {
        set_error("fv_conv_pair_forward: empty input");
        return FV_ERR_INVALID;
    }
    const AlgoScope algo_scope(c1->L.algo, false);
    return conv_pair_run(c1->L, c2->L, d_x, d_y, batch, t, OUT_SET, 1.0f, (hipStream_t)stream);
}

FV_API fv_status fv_conv_set_precision(fv_conv* c, int32_t precision) {
    if (!c || (precision != FV_PRECISION_F32 && precision != FV_PRECISION_F16X3)) {
        set_error("fv_conv_set_precision: invalid argument");
        return FV_ERR_INVALID;
    }
    c->L.precision = precision;
    return FV_OK;
}

FV_API fv_status fv_conv_set_algorithm(fv_conv* c, int32_t algo) {
    if (!c || (algo != FV_CONV_ALGO_AUTO && algo != FV_CONV_ALGO_DIRECT && algo != FV_CONV_ALGO_WINOGRAD)) {
        set_error("fv_conv_set_algorithm: invalid argument");
        return FV_ERR_INVALID;
    }
    c->L.algo = algo;
    return FV_OK;
}

FV_API void fv_conv_destroy(fv_conv* c) {
    if (!c) return;
    conv_layer_destroy(c->L);
    delete c;
}

FV_API void fv_reload_env(void) { fv::reload_knobs(); }
FV_API const char* fv_last_error(void) { return g_err.c_str(); }
FV_API int32_t fv_abi_version(void) { return FV_ABI_VERSION; }
FV_API const char* fv_last_kernel(void) { return g_kernel.c_str(); }

}  // extern "C"
