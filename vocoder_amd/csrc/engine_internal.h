// Shared by the engine's translation units (engine_*.hip): the model structs, struct fv_engine and the prototypes the units share.
// The kernel-side header is fv_internal.h; nothing here is seen by a conv unit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>

#include "fv_internal.h"

// wraps a small-kernel launch expression with the profiler
#define FV_PROF(stream, label, flops, bytes, call)                      \
    do {                                                                \
        const int _pi = prof_begin(stream);                             \
        fv_status _st = (call);                                         \
        if (_pi >= 0) prof_end(stream, _pi, label, flops, bytes);       \
        if (_st) return _st;                                            \
    } while (0)

namespace fv {

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

std::vector<float> kaiser_sinc_filter(double cutoff, double half_width, int ks);   // engine_build.hip
// attaches `p` to this thread's prof_begin / prof_end (nullptr: detached) and returns what was attached before (engine_runtime.hip)
Profiler* set_profiler(Profiler* p);

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

// Per-engine options: read from the environment once, at fv_create (read_engine_options, engine_build.hip) — an engine keeps the values it was
// created under, so two engines of one process can differ (the tests' A/B pairs)
struct EngineOptions {
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
    bool use_graph = true;        // FV_NO_GRAPH=1 disables hipGraph replay (so do FV_DEBUG_STOP, fv_set_graph_replay(0) and a failed capture)
    bool branch_streams = true;   // FV_SINGLE_STREAM=1 runs the ResBlock branches back to back on the caller's stream (the chain form of the branch mean)
    bool single_tree = false;     // FV_SINGLE_STREAM=2: one stream too, but the TREE form — the kernel instances of the shipped three-stream step, launch by launch (rocprofv3 / PMC passes: tools/probe_model.py)
    int tile_frames_override = 0;   // FV_TILE_FRAMES: tile length in frames (tests / experiments); 0 = only when the addressing span needs it
    // FV_DEBUG_STOP = stage * 100 + pair * 10 + half stops the upsampler forward after that stage's dilation pair (half 0: after c1, 1: after c2)
    // with the branch buffers left in the workspace for inspection (tools/archive/probe_f16_locate.py); -1 = unset
    int debug_stop = -1;
};

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
    EngineOptions opt;
    struct GraphKey {
        const void* in;
        void* out;
        void* ws;
        const void* tmpl;
        const void* noise;
        int batch, t_in;
        hipStream_t stream;
        // seeded RefineGAN: kernel scalars are baked into a captured graph, so a replay under another seed, row or origin would draw other noise
        bool seeded;
        uint64_t seed;
        int32_t first_row;
        int64_t origin_frame;
        bool operator==(const GraphKey& o) const {
            return in == o.in && out == o.out && ws == o.ws && tmpl == o.tmpl && noise == o.noise && batch == o.batch && t_in == o.t_in &&
                   stream == o.stream && seeded == o.seeded && seed == o.seed && first_row == o.first_row && origin_frame == o.origin_frame;
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
    struct LogmelParts {
        float *Yp, *Sp, *Mg;
    };
    LogmelParts logmel_carve(float* ws, int B, int T) const;
    size_t logmel_ws_elems(int B, int T) const;   // floats that logmel_carve's parts span (what fv_workspace_bytes reports for T frames)
    fv_status run_logmel_tail(const LogmelParts& p, float* d_out, int B, int T, hipStream_t s);

    fv_status build_refinegan();
    fv_status run_refinegan(const float* d_mel, float* d_out, int B, int T, float* ws, hipStream_t s);
    const float* cur_noise = nullptr;      // set by fv_forward_refinegan for the duration of one call
    // Seeded AdaIN noise (fv_refinegan_set_noise_seed): engine state, then what one call sets for its duration — cur_seeded: this call's AdaIN
    // launches compute their noise (no cur_noise); cur_origin_frame: the utterance frame its input starts at; cur_tile: run_model's tile plan
    // (n tiles per clip, stride and the pulled-back last start in frames)
    bool noise_seeded = false;
    uint64_t noise_seed = 0;
    int32_t noise_first_row = 0;
    bool cur_seeded = false;
    int64_t cur_origin_frame = 0;
    int cur_tile_n = 1, cur_tile_stride = 0, cur_tile_last = 0;
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
    size_t tile_workspace_bytes(int batch, const TilePlan& tp) const;   // what run_model carves for batch clips as tp.n tiles each
    fv_status run_upsampler(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s);
    const float* cur_template = nullptr;   // set by fv_forward_template for the duration of one call
    // the generators that take a pitch template beside the mel: RefineGAN always, the upsampler family when built with use_template
    bool wants_template() const {
        return cfg.model == FV_MODEL_REFINEGAN ||
               ((cfg.model == FV_MODEL_HIFIGAN || cfg.model == FV_MODEL_BIGVGAN || cfg.model == FV_MODEL_FIREFLY) && cfg.ups.use_template);
    }
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
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Attaches the engine's profiler (when fv_profile_begin switched it on) to this thread for the scope's duration, then restores what it found:
// scopes nest (a stream push around its forward)
struct ProfScope {
    Profiler* prev;
    explicit ProfScope(fv_engine* e) : prev(set_profiler(e->profiling ? &e->prof : nullptr)) {}
    ~ProfScope() { set_profiler(prev); }
};
// What every entry that runs the model sets up around run_model for the duration of the call: the template / noise of this call, the engine's
// conv algorithm and the profiler
struct ForwardScope {
    AlgoScope algo;
    ProfScope prof;
    ForwardScope(fv_engine* e, const float* d_template, const float* d_noise, bool seeded = false, int64_t origin_frame = 0)
        : algo(e->algo, e->invariant), prof(e) {
        e->cur_template = d_template;
        e->cur_noise = d_noise;
        e->cur_seeded = seeded;
        e->cur_origin_frame = origin_frame;
    }
};

// engine_forward.hip
fv_status check_template(const fv_engine* e, const float* d_template);
fv_status check_forward(fv_engine* e, const float* d_in, const float* d_template, float* d_out, int32_t batch, int32_t t_in,
                        void* d_workspace, size_t workspace_bytes);
// seeded: a RefineGAN forward whose AdaIN noise is computed in the kernels, for an input that starts at frame origin_frame of its utterance
fv_status forward_common(fv_engine* e, const float* d_in, const float* d_template, const float* d_noise, float* d_out,
                         int32_t batch, int32_t t_in, void* d_workspace, size_t workspace_bytes, void* stream, bool seeded = false,
                         int64_t origin_frame = 0);
// engine_refinegan.hip
size_t refine_ws_elems(const fv_engine* e, int B, int T);
int64_t refine_reach(const RefineModel& m);               // one-sided reach in input frames (reach_frames)
int64_t refine_max_elems_per_frame(const RefineModel& m);   // largest per-item tensor per input frame; 0: the lengths do not line up (tile_frame_limit)
