// RefineGAN: builder, workspace sizing, reach, forward and its ABI entries (template + AdaIN noise, given by the caller or seeded and computed in
// the AdaIN kernels).
#include "engine_internal.h"

// RefineGAN builds AdaIN(channels=...) without forwarding the generator's slope (refinegan.py:157,165): always 0.2
constexpr float kAdaINSlope = 0.2f;

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
size_t refine_ws_elems(const fv_engine* e, int B, int T) {
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

int64_t refine_max_elems_per_frame(const RefineModel& m) {
    std::vector<int64_t> down, up;
    if (!m.lengths(1 << 10, down, up)) return 0;
    return (int64_t)(refine_max_elems(m, down, up) >> 10);
}

// One-sided reach in input frames (vocoder_amd/refinegan_noise.py refinegan_reach restates it): an upper bound on how far an output sample's
// inputs, mel and template, lie from it.  Walked backwards from the output in samples at each layer's own rate: a conv adds (k - 1) / 2 *
// dilation, a ResBlock's six convs 2 * (k - 1) / 2 * (1 + 3 + 5); the up-sampling interpolation divides by its rate and adds its two taps, the
// down-sampling one multiplies by its rate and adds rate + 1; AdaIN is pointwise (refinegan.py:124-127: no normalisation).  Every skip tensor
// is needed as far as its farther consumer reaches: the up stage that concatenates it, or the rest of the down path.
int64_t refine_reach(const RefineModel& m) {
    const fv_refinegan_config& c = m.cfg;
    const int S = c.num_stages;
    int64_t R = 3;   // output_conv (k = 7)
    std::vector<int64_t> at_skip((size_t)S, 0);
    for (int i = S - 1; i >= 0; --i) {
        R += 2 * 5 * 9 + 3;   // the widest branch (k = 11) and input_conv (k = 7)
        at_skip[(size_t)(S - 1 - i)] = R;
        const int u = c.upsample_rates[i];
        R = (R + u - 1) / u + 2;
    }
    const int64_t mel = R + 3;   // mel_conv (k = 7), at the frame rate
    int64_t need = R;
    for (int k = S - 1; k >= 0; --k) {
        const int d = c.downsample_rates[k];
        need = std::max(at_skip[(size_t)k], (need + 2 * 3 * 9) * d + d + 1);
    }
    const int64_t tmpl = need + 3;   // template_conv (k = 7), in samples
    return std::max(mel, (tmpl + c.hop_length - 1) / c.hop_length + 1);
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
    if (!cur_noise && !(cur_seeded && noise_seeded)) {
        set_error("refinegan: no AdaIN noise for this forward (fv_forward_refinegan's d_noise, or fv_refinegan_set_noise_seed)");
        return FV_ERR_STATE;
    }
    if (!cur_noise && B > 65535) {
        set_error("refinegan: %d rows (clips x time tiles) in one seeded forward, more than 65535: split the batch", B);
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
    int layer = 0;             // AdaIN layers in order of use: the seeded noise's `l`
    int64_t spf = 1;           // samples per frame at stage i
    // v = leaky_relu(x + noise * weight[c]): the noise from the caller's tensor, or computed in the kernel (seeded: refinegan.py:125's draw
    // becomes a function of the absolute position, so a window of an utterance sees the whole utterance's samples)
    auto adain = [&](const float* x, const float* w, float* y, int C, int t, int accumulate, float scale) -> fv_status {
        const size_t nelem = (size_t)B * C * t;
        if (noise) {
            FV_PROF(s, "adain", (accumulate ? 4.0 : 3.0) * nelem, (accumulate ? 16.0 : 12.0) * nelem,
                    launch_adain(x, noise, w, y, B, C, t, kAdaINSlope, accumulate, scale, s));
            noise += nelem;
        } else {
            const SeededNoise sn{noise_seed, noise_first_row, cur_tile_n, cur_origin_frame * spf, cur_tile_stride * spf, cur_tile_last * spf};
            FV_PROF(s, "adain_seeded", (accumulate ? 4.0 : 3.0) * nelem, (accumulate ? 12.0 : 8.0) * nelem,
                    launch_adain_seeded(x, w, y, B, C, t, kAdaINSlope, accumulate, scale, sn, layer, s));
        }
        ++layer;
        return FV_OK;
    };
    for (int i = 0; i < S; ++i) {
        const RefineUp& u = *m.ups[i];
        const int t = (int)up[i + 1];
        spf *= u.rate;
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
        for (int j = 0; j < 3; ++j) {
            if ((st = adain(XI, u.d_w1[j], XA, u.cout, t, 0, 1.0f))) return st;
            if ((st = resblock(u.rb[j], XA, CAT, XT, XB, t, /*post_leaky=*/false))) return st;   // CAT is free again: branch output
            if ((st = adain(CAT, u.d_w2[j], Y, u.cout, t, j > 0, j == 2 ? 1.0f / 3.0f : 1.0f))) return st;
        }
        xcur = Y;
    }
    // leaky_relu -> output_conv -> tanh (refinegan.py:319-321)
    const int L = (int)up[S];
    FV_PROF(s, "conv_post_narrow", 2.0 * B * m.out_cin * 7 * L, 4.0 * B * (m.out_cin + 1) * L,
            launch_conv_narrow(xcur, m.d_wout, m.d_bout, d_out, B, m.out_cin, L, 1, 7, 3, FV_ACT_LEAKY_RELU, FV_ACT_TANH, slope, s));
    return FV_OK;
}

extern "C" {

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
    if (e->noise_seeded && e->finalized && t_in >= 1 && e->tile_plan(t_in).n > 1) {
        set_error("fv_forward_refinegan: RefineGAN with explicit noise runs whole clips only and %d frames run as time tiles on this seeded "
                  "engine (the explicit noise layout has no tiled form): use fv_forward_refinegan_seeded", t_in);
        return FV_ERR_UNSUPPORTED;
    }
    return forward_common(e, d_mel, d_template, d_noise, d_out, batch, t_in, d_workspace, workspace_bytes, stream);
}

static fv_status seeded_preamble(const fv_engine* e, const char* fn, int64_t origin_frame) {
    if (!e || e->cfg.model != FV_MODEL_REFINEGAN) {
        set_error("%s: not a RefineGAN engine", fn);
        return FV_ERR_INVALID;
    }
    if (!e->finalized) {
        set_error("%s: call fv_finalize first", fn);
        return FV_ERR_STATE;
    }
    if (!e->noise_seeded) {
        set_error("%s: the engine has no noise seed (fv_refinegan_set_noise_seed)", fn);
        return FV_ERR_STATE;
    }
    if (origin_frame < 0 || origin_frame > (1LL << 40)) {
        set_error("%s: origin_frame = %lld, outside [0, 2^40]", fn, (long long)origin_frame);
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

FV_API fv_status fv_refinegan_set_noise_seed(fv_engine* e, uint64_t seed, int32_t first_row) {
    if (!e || e->cfg.model != FV_MODEL_REFINEGAN) {
        set_error("fv_refinegan_set_noise_seed: not a RefineGAN engine");
        return FV_ERR_INVALID;
    }
    if (first_row < 0) {
        set_error("fv_refinegan_set_noise_seed: first_row = %d must be >= 0", first_row);
        return FV_ERR_INVALID;
    }
    e->noise_seeded = true;
    e->noise_seed = seed;
    e->noise_first_row = first_row;
    e->drop_graphs();
    return FV_OK;
}

FV_API fv_status fv_refinegan_clear_noise_seed(fv_engine* e) {
    if (!e || e->cfg.model != FV_MODEL_REFINEGAN) {
        set_error("fv_refinegan_clear_noise_seed: not a RefineGAN engine");
        return FV_ERR_INVALID;
    }
    e->noise_seeded = false;
    e->noise_seed = 0;
    e->noise_first_row = 0;
    e->drop_graphs();
    return FV_OK;
}

FV_API fv_status fv_forward_refinegan_seeded(fv_engine* e, const float* d_mel, const float* d_template, float* d_out, int32_t batch,
                                             int32_t t_in, int64_t origin_frame, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (const fv_status st = seeded_preamble(e, "fv_forward_refinegan_seeded", origin_frame)) return st;
    if (!d_template) {
        set_error("fv_forward_refinegan_seeded: the template (B, 1, T*hop) is required");
        return FV_ERR_INVALID;
    }
    if (batch >= 1 && t_in >= 1 && (int64_t)batch * e->tile_plan(t_in).n > 65535) {
        set_error("fv_forward_refinegan_seeded: %d clips x %d time tiles exceed 65535 rows per call: split the batch", batch, e->tile_plan(t_in).n);
        return FV_ERR_UNSUPPORTED;
    }
    return forward_common(e, d_mel, d_template, nullptr, d_out, batch, t_in, d_workspace, workspace_bytes, stream, true, origin_frame);
}

FV_API fv_status fv_refinegan_fill_noise(fv_engine* e, float* d_noise, int32_t batch, int32_t t_in, int64_t origin_frame, void* stream) {
    if (const fv_status st = seeded_preamble(e, "fv_refinegan_fill_noise", origin_frame)) return st;
    if (!d_noise || batch < 1 || batch > 65535 || t_in < 1) {
        set_error("fv_refinegan_fill_noise: null noise buffer, or batch (%d) outside [1, 65535], or t_in (%d) < 1", batch, t_in);
        return FV_ERR_INVALID;
    }
    int64_t t = t_in, spf = 1;
    for (auto& u : e->refine.ups) {
        t *= u->rate;
        if (t >= (1LL << 31)) {
            set_error("fv_refinegan_fill_noise: clip too long");
            return FV_ERR_UNSUPPORTED;
        }
    }
    const ProfScope prof(e);
    hipStream_t s = (hipStream_t)stream;
    int layer = 0;
    t = t_in;
    for (auto& u : e->refine.ups) {
        t *= u->rate;
        spf *= u->rate;
        const SeededNoise sn{e->noise_seed, e->noise_first_row, 1, origin_frame * spf, 0, 0};
        const size_t nelem = (size_t)batch * u->cout * (size_t)t;
        for (int j = 0; j < 6; ++j, ++layer, d_noise += nelem)
            FV_PROF(s, "refinegan_fill_noise", 0.0, 4.0 * nelem, launch_refinegan_fill_noise(d_noise, batch, u->cout, (int)t, sn, layer, s));
    }
    return FV_OK;
}

}  // extern "C"
