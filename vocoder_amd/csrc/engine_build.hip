// Building an engine: config validation, the weight builders (state dict -> folded, packed, uploaded layers) and the create / load /
// finalize / destroy ABI with its setters and shape queries.
#include <atomic>
#include <mutex>
#include <thread>

#include "engine_internal.h"

namespace fv {

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
std::vector<float> kaiser_sinc_filter(double cutoff, double half_width, int ks) {
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

}  // namespace fv

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
                    first_error = fv_last_error();   // this worker's thread-local message: handed to the caller's thread below
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

std::vector<float> fv::stft_basis(const std::vector<float>& win, int N, int hop, int taps) {
    const int nb = N / 2 + 1;
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
    return wst;
}

std::vector<float> fv::istft_basis(const std::vector<float>& win, int N) {
    const int nb = N / 2 + 1;
    std::vector<float> basis((size_t)N * 2 * nb);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < nb; ++k) {
            const double ck = (k == 0 || k == N / 2) ? 1.0 : 2.0;
            const double ang = 2.0 * M_PI * (double)(((int64_t)k * n) % N) / N;
            basis[(size_t)n * 2 * nb + k] = (float)(ck * std::cos(ang) / N * win[n]);
            basis[(size_t)n * 2 * nb + nb + k] = (float)(-ck * std::sin(ang) / N * win[n]);
        }
    return basis;
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
    const std::vector<float> basis = istft_basis(win, N);
    if ((st = conv_layer_create(head.idft, false, 2 * nb, N, 1, 1, 0, 1, basis.data(), nullptr))) return st;
    std::vector<float> win2(N);
    for (int n = 0; n < N; ++n) win2[n] = win[n] * win[n];
    if ((st = upload(win2, &head.d_win2))) return st;
    head.win2 = win2;
    has_head = true;
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
    const std::vector<float> wst = stft_basis(win, N, hop, taps);
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

// The per-engine options of the environment fv_create runs in (EngineOptions, engine_internal.h)
static EngineOptions read_engine_options() {
    EngineOptions o;
    if (const char* v = std::getenv("FV_NO_PAIR_FUSION")) o.fuse_pairs = !(v[0] == '1');
    if (const char* v = std::getenv("FV_PAIR_MAXC")) o.pair_max_c = std::atoi(v);
    if (const char* v = std::getenv("FV_CHAIN_MAX_C")) o.chain_max_c = std::atoi(v);
    if (const char* v = std::getenv("FV_NO_POST_SUM3")) o.post_mean_fused = !(v[0] == '1');
    if (const char* v = std::getenv("FV_NO_AMP_FUSION")) o.fuse_amp_convs = !(v[0] == '1');
    if (const char* v = std::getenv("FV_AMP_MAXC")) o.fuse_amp_max_c = std::atoi(v);
    if (const char* v = std::getenv("FV_AMP_MAXK")) o.fuse_amp_max_k = std::atoi(v);
    if (const char* v = std::getenv("FV_SINGLE_STREAM")) {
        o.branch_streams = !(v[0] == '1' || v[0] == '2');
        o.single_tree = v[0] == '2';
    }
    if (const char* v = std::getenv("FV_NO_GRAPH")) o.use_graph = !(v[0] == '1');
    if (const char* v = std::getenv("FV_DEBUG_STOP")) {
        o.debug_stop = std::atoi(v);
        o.use_graph = false;   // the early return leaves forked branch streams unjoined: not capturable
    }
    if (const char* v = std::getenv("FV_TILE_FRAMES")) o.tile_frames_override = std::atoi(v);
    return o;
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
    e->opt = read_engine_options();
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
    e->opt.use_graph = enable != 0;
    return FV_OK;
}

FV_API int32_t fv_get_graph_replay(const fv_engine* e) { return e && e->opt.use_graph ? 1 : 0; }

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

}  // extern "C"
