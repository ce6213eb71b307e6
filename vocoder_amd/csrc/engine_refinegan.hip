// RefineGAN: builder, workspace sizing, forward and its two ABI entries (template + AdaIN noise).
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
    return forward_common(e, d_mel, d_template, d_noise, d_out, batch, t_in, d_workspace, workspace_bytes, stream);
}

}  // extern "C"
